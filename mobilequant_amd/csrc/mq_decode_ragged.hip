// Ragged decode step: up to MQ_DECODE_MAX_BATCH attention rows in one launch, each a (sequence, position) of a batch of caches, where
// consecutive rows of one sequence at consecutive positions see each other (BatchDecodeEngine.step_tokens / extend and batched
// speculative verification, mobilequant_amd/decode_batch.py).
//   mq_decode_attention_ragged : decode_attention_multi_kernel<D, false> (mq_decode_multi.hip: flat value layout) generalised from
//                                "rows p .. p + R - 1 of one cache" to a row table on a (heads, nsplit, rows) grid over `batch` caches;
//                                the phases are the MQ_ATTN_* texts of mq_decode_attention.h
// Row r names sequence row_seq[r] and position row_pos[r].  A RUN is a maximal stretch of consecutive rows of one sequence whose
// positions rise by exactly one; the workgroup finds the distance j of its row from the run's first row by walking the table back, and
// is then the multi kernel at (that sequence's cache, p = row_pos[r] - j, j): the keys and values of rows r - j .. r are formed in LDS
// with the batched kernel's RoPE / quantizer expressions (attn_new_elem), no position >= p is read from memory, the KV group's first
// head at split 0 appends the row's own position, and the new positions enter p.v through the split that owns their 64-position block.
// Everything else -- the score expression, the max, the float sum of the exponentials in its thread / wave order, the probability grid,
// the split protocol -- is decode_attention_batch_kernel's at T = row_pos[r] + 1, so row r's bits are that launch's for its position.
// A row whose sequence is outside [0, batch) or whose position is outside [0, cache_len) is idle: it reads and writes nothing, and it
// ends a run.  The table is device data: whatever it holds, j <= r < rows, the sequence and the position are range-checked before any
// address is formed from them, and the run's positions p .. row_pos[r] lie in [0, cache_len).
#include "mq_decode_attention.h"

namespace mq {

#pragma clang fp contract(off)

template <int D>
__global__ void __launch_bounds__(256) decode_attention_ragged_kernel(const mq_decode_attention_ragged_args ra) {
  const mq_decode_attention_args& a = ra.a;
  MQ_ATTN_GEOMETRY(D);
  MQ_ATTN_LDS(s_q8[D], s_kn[DB_MAXB * D], s_vn[DB_MAXB * D]);      // this row's q; the run's rows r - j .. r: new k / v
  const int H = a.heads, rot = a.rot_dim, r = blockIdx.z, CL = a.cache_len;
  const int sb = ra.row_seq[r], pos = ra.row_pos[r];
  if (sb < 0 || sb >= ra.batch || pos < 0 || pos >= CL) return;    // an idle row: nothing is read or written
  int j = 0;                                                       // rows of this run in front of row r (uniform: scalar loads)
  while (j < r && j < DB_MAXB - 1 && pos - 1 - j >= 0 && ra.row_seq[r - 1 - j] == sb && ra.row_pos[r - 1 - j] == pos - 1 - j) ++j;
  const int p = pos - j, r0 = r - j;
  const int nsplit = pos >= ra.split_from ? a.nsplit : 1;
  const int h = blockIdx.x, c = blockIdx.y, kvh = h / (H / a.kv_heads);
  if (c >= nsplit) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float cv = a.consts[lane];
  const size_t cache_seq = (size_t)a.kv_heads * CL * D;
  const int8_t* kc = a.k_cache + sb * cache_seq + (size_t)kvh * CL * D;
  const int8_t* vc = a.v_cache + sb * cache_seq + (size_t)kvh * CL * D;
  const int T = pos + 1;
  MQ_ATTN_KEY_LOADER(t < p);
  MQ_ATTN_VALUE_LOADER(p);
  load_values(0);
  MQ_ATTN_GRIDS;
  // ---- RoPE + the input quantizers: this row's q, the run's new k / v up to this row ---------------------------------------------------
  int qsum_part = 0;
  if (tid < D) {
    const int half = rot >> 1;
    const int dpart = tid < rot ? (tid < half ? tid + half : tid - half) : tid;
    const int dr = tid < rot ? tid : 0;
    float cs = 0.f, sn = 0.f;
    for (int i = 0; i <= j; ++i) {
      const float* row = a.qkv + (size_t)(r0 + i) * ra.qkv_stride;
      const float* kp = row + (size_t)H * D + (size_t)kvh * D;
      const float* vp = row + (size_t)(H + a.kv_heads) * D + (size_t)kvh * D;
      cs = a.cos[(size_t)(p + i) * rot + dr];
      sn = a.sin[(size_t)(p + i) * rot + dr];
      s_kn[i * D + tid] = attn_new_elem(kp[tid], kp[dpart], cs, sn, tid, rot, qb);
      s_vn[i * D + tid] = attn_new_elem(vp[tid], 0.f, 0.f, 0.f, tid, 0, pb);
    }
    const float* qp = a.qkv + (size_t)r * ra.qkv_stride + (size_t)h * D;
    const int8_t sq = attn_new_elem(qp[tid], qp[dpart], cs, sn, tid, rot, qa);      // (cs / sn: position pos, the loop's last)
    s_q8[tid] = sq;
    qsum_part = sq;
    if (c == 0 && h % (H / a.kv_heads) == 0) {                     // the group's first head appends row r's position
      int8_t* k_cache = a.k_cache + sb * cache_seq + (size_t)kvh * CL * D;
      int8_t* v_cache = a.v_cache + sb * cache_seq + (size_t)kvh * CL * D;
      k_cache[(size_t)pos * D + tid] = s_kn[j * D + tid];
      v_cache[(size_t)pos * D + tid] = s_vn[j * D + tid];
    }
  }
  MQ_ATTN_QSUM_REDUCE;
  MQ_ATTN_CONSTS;
  v4i qf[CH];
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) qf[ch] = MQ_ATTN_LDS_FRAG(s_q8, ch);
  // cached positions from registers, the run's (t >= p: row t - p, clamped -- t >= T is masked) from LDS
  MQ_ATTN_SCORES(t >= p ? MQ_ATTN_LDS_FRAG(s_kn + (t - p < j ? t - p : j) * D, ch) : kbuf[u][ch]);
  MQ_ATTN_SOFTMAX;
  // ---- p.v: exact integers.  Cached positions t < p over this split's blocks, then the run's positions p .. pos from LDS -------------
  long long acc[4] = {0, 0, 0, 0};
  long long psum = 0;
  MQ_ATTN_SPLIT_BLOCKS(p);
  const int items = my_blocks * PPB;
  MQ_ATTN_PV_FLAT(p)
  if (grp == 0) {
    for (int i = 0; i <= j; ++i) {
      const int t = p + i;
      if (nsplit == 1 || ((t >> 6) % nsplit) == c) MQ_ATTN_PV_ADD_NEW(s_vn + i * D, s_pi[t])   // the split that owns position t's block adds it
    }
  }
  MQ_ATTN_FOLD_GROUPS;
  __syncthreads();
  // this row's split scratch, tickets and output row
  MQ_ATTN_FINISH(G,
                 unsigned long long* part = reinterpret_cast<unsigned long long*>(a.part) + (size_t)r * a.nsplit * H * D;
                 unsigned* ticket = a.ticket + (size_t)r * H;, part, ticket,
                 const size_t o = ((size_t)r * H + h) * D + tid;, o)
}

}  // namespace mq

using namespace mq;

extern "C" {

int mq_decode_attention_ragged(const mq_decode_attention_ragged_args* args, mq_stream_t stream) {
  MQ_REQUIRE(args != nullptr, "mq_decode_attention_ragged: null argument block");
  const int R = args->rows, B = args->batch;
  MQ_REQUIRE(R >= 1 && R <= MQ_DECODE_MAX_BATCH, "mq_decode_attention_ragged: rows=%d outside 1..%d", R, MQ_DECODE_MAX_BATCH);
  MQ_REQUIRE(B >= 1 && B <= MQ_DECODE_MAX_BATCH, "mq_decode_attention_ragged: batch=%d outside 1..%d", B, MQ_DECODE_MAX_BATCH);
  MQ_REQUIRE(args->row_seq && args->row_pos, "mq_decode_attention_ragged: null row table (row_seq / row_pos)");
  mq_decode_attention_args a = args->a;
  a.pos = args->row_pos;                                           // (a.pos is not read: the positions are the table's)
  int rc = check_five_launch_attention_shape("mq_decode_attention_ragged", a);
  if (rc != MQ_OK) return rc;
  rc = check_five_launch_attention_grids("mq_decode_attention_ragged", a);
  if (rc != MQ_OK) return rc;
  MQ_REQUIRE(a.prefetch_wgs == 0, "mq_decode_attention_ragged: no prefetch rows (prefetch_wgs must be 0)");
  MQ_REQUIRE(R == 1 || args->qkv_stride >= (int64_t)(a.heads + 2 * a.kv_heads) * a.head_dim, "mq_decode_attention_ragged: qkv_stride must cover a q | k | v row");
  const size_t lds = (size_t)a.cache_len * sizeof(float);
  const int di = a.head_dim == 32 ? 0 : a.head_dim == 64 ? 1 : a.head_dim == 128 ? 2 : 3;
  static const void* const fns[4] = {
      reinterpret_cast<const void*>(decode_attention_ragged_kernel<32>), reinterpret_cast<const void*>(decode_attention_ragged_kernel<64>),
      reinterpret_cast<const void*>(decode_attention_ragged_kernel<128>), reinterpret_cast<const void*>(decode_attention_ragged_kernel<256>)};
  static std::atomic<size_t> lds_set[4][kMaxDevices];
  rc = set_lds(fns[di], lds_set[di], lds, "mq_decode_attention_ragged");
  if (rc != MQ_OK) return rc;
  const dim3 grid((unsigned)a.heads, (unsigned)a.nsplit, (unsigned)R);
  hipStream_t st = as_stream(stream);
  switch (a.head_dim) {
    case 32: decode_attention_ragged_kernel<32><<<grid, 256, lds, st>>>(*args); break;
    case 64: decode_attention_ragged_kernel<64><<<grid, 256, lds, st>>>(*args); break;
    case 128: decode_attention_ragged_kernel<128><<<grid, 256, lds, st>>>(*args); break;
    default: decode_attention_ragged_kernel<256><<<grid, 256, lds, st>>>(*args); break;
  }
  MQ_LAUNCH_CHECK("mq_decode_attention_ragged");
  return MQ_OK;
}

}  // extern "C"
