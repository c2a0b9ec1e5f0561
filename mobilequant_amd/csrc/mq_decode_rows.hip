// Decode steps of several attention rows per launch, where a row sees the rows in front of it: ONE kernel behind two entries.
//   mq_decode_attention_multi  : up to MQ_DECODE_MAX_BATCH CONSECUTIVE positions of one sequence (DecodeEngine.step_tokens / extend and
//                                speculative verification, mobilequant_amd/decode.py); flat or chunked value cache
//   mq_decode_attention_ragged : up to MQ_DECODE_MAX_BATCH rows, each a (sequence, position) of a batch of caches, named by a row table
//                                (BatchDecodeEngine.step_tokens / extend and batched speculative verification,
//                                mobilequant_amd/decode_batch.py); flat value cache
// Both run decode_attention_rows_kernel<D, VCH, TABLE> on a (heads, nsplit, rows) grid; its phases are the MQ_ATTN_* texts of
// mq_decode_attention.h, shared with decode_attention_batch_kernel<D> (mq_decode_batch.hip).  The entries differ in the ROW LOCATOR at
// the kernel's top alone: where workgroup row r finds its sequence sb, its position pos and the number j of rows of its RUN in front
// of it (a run: consecutive rows of one sequence at positions rising by exactly one).
//   TABLE = false: one cache, one run: sb = 0 (a constant: the per-sequence offsets fold away), pos = *a.pos + r, j = r.
//   TABLE = true : sb = row_seq[r], pos = row_pos[r], and j found by walking the table back.  A row whose sequence is outside
//                  [0, batch) or whose position is outside [0, cache_len) is idle: it reads and writes nothing, and it ends a run.  The
//                  table is device data: whatever it holds, j <= r < rows and j < DB_MAXB, the sequence and the position are
//                  range-checked before any address is formed from them, and the run's positions p .. pos lie in [0, cache_len).
// Behind the locator, with p = pos - j the run's first position: the row reads the cached positions t < p, and positions p .. pos are
// appended by rows r - j .. r of this very launch, so no workgroup may read them back from memory: each workgroup builds the run's new
// keys and values of its KV head in LDS with the batched kernel's RoPE / quantizer expressions (attn_new_elem) and takes them from
// there; the KV group's first head at split 0 appends the row's own position.  Everything else -- the score expression, the max, the
// float sum of the exponentials in its thread / wave order, the probability grid, the split protocol -- is
// decode_attention_batch_kernel's at T = pos + 1, so the row's bits are that launch's for its position.  The p.v sums are exact
// integers: the cached positions go through the batched kernel's loop (flat value layout) or, with VCH, through 16-position chunks of
// one dimension per 16-byte request (the four-launch kernel's mapping); the new positions are added from LDS by the split that owns
// their 64-position block.
#include "mq_decode_attention.h"
#include "mq_row_runs.h"

namespace mq {

#pragma clang fp contract(off)

template <int D, bool VCH, bool TABLE>
__global__ void __launch_bounds__(256) decode_attention_rows_kernel(const mq_decode_attention_ragged_args ra) {
  static_assert(!(VCH && TABLE), "the row table is served for the flat value layout");
  const mq_decode_attention_args& a = ra.a;
  MQ_ATTN_GEOMETRY(D);
  MQ_ATTN_LDS(s_q8[D], s_kn[DB_MAXB * D], s_vn[DB_MAXB * D]);      // this row's q; the run's rows r - j .. r: new k / v
  const int H = a.heads, rot = a.rot_dim, r = blockIdx.z, CL = a.cache_len;
  // ---- the row locator: sb, pos, j --------------------------------------------------------------------------------------------------
  int sb = 0, pos, j;
  if constexpr (TABLE) {
    sb = ra.row_seq[r], pos = ra.row_pos[r];
    if (sb < 0 || sb >= ra.batch || pos < 0 || pos >= CL) return;  // an idle row: nothing is read or written
    j = run_rows_in_front(ra.row_seq, ra.row_pos, r, sb, pos, DB_MAXB - 1);      // rows of this run in front of row r (uniform: scalar loads)
  } else {
    const int p0 = a.pos[0];
    j = r, pos = p0 + j;
    if (p0 < 0 || pos >= CL) return;                               // a row past the cache: nothing is read or written
  }
  const int p = pos - j, r0 = r - j;
  const int nsplit = pos >= ra.split_from ? a.nsplit : 1;
  const int h = blockIdx.x, c = blockIdx.y, kvh = h / (H / a.kv_heads);
  if (c >= nsplit) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float cv = a.consts[lane];
  const size_t cache_seq = (size_t)a.kv_heads * CL * D;            // (both layouts: a KV head's values are cache_len * D bytes)
  const int8_t* kc = a.k_cache + sb * cache_seq + (size_t)kvh * CL * D;
  const int8_t* vc = a.v_cache + sb * cache_seq + (size_t)kvh * CL * D;
  const int T = pos + 1;
  MQ_ATTN_KEY_LOADER(t < p);
  MQ_ATTN_VALUE_LOADER(p);                                         // (flat layout) dimensions 4 dq .. 4 dq + 3 of VB positions
  // (chunked layout) thread (vd, vg) owns dimension vd of 16-position chunks vg, vg + NG, ... of this split's blocks: ONE 16-byte request
  // per chunk, a wave's requests one coalesced KiB (the four-launch kernel's mapping)
  constexpr int NG = 256 / D, VCB = 4;                           // chunk requests in flight per thread
  const int vd = tid & (D - 1), vg = tid / D;
  v4i cbuf[VCB];
  auto chunk_of = [&](int ci) { return 4 * (c + nsplit * (ci >> 2)) + (ci & 3); };      // ci-th chunk of this split's 64-blocks
  auto load_chunks = [&](int ci0) {
#pragma unroll
    for (int u = 0; u < VCB; ++u) {
      const int jj = chunk_of(ci0 + u * NG + vg);
      cbuf[u] = *reinterpret_cast<const v4i*>(vc + ((size_t)(16 * jj < p ? jj : 0) * D + vd) * 16);
    }
  };
  if constexpr (VCH) load_chunks(0);
  else load_values(0);
  MQ_ATTN_GRIDS;
  // ---- RoPE + the input quantizers: this row's q, the run's new k / v up to this row ------------------------------------------------
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
      if constexpr (VCH) v_cache[((size_t)(pos >> 4) * D + tid) * 16 + (pos & 15)] = s_vn[j * D + tid];
      else v_cache[(size_t)pos * D + tid] = s_vn[j * D + tid];
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
  // ---- p.v: exact integers.  Cached positions t < p over this split's blocks, then the run's positions p .. pos from LDS -----------
  long long acc[4] = {0, 0, 0, 0};
  long long psum = 0;
  MQ_ATTN_SPLIT_BLOCKS(p);
  if constexpr (VCH) {
    const int nch = my_blocks * 4;
    for (int ci0 = 0; ci0 < nch; ci0 += VCB * NG) {
      if (ci0 > 0) load_chunks(ci0);
#pragma unroll
      for (int u = 0; u < VCB; ++u) {
        const int ci = ci0 + u * NG + vg, t0 = 16 * chunk_of(ci);
        if (ci >= nch || t0 >= p) continue;
        int a32 = 0, p32 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const v4i pq = *reinterpret_cast<const v4i*>(s_pi + t0 + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int pim = t0 + 4 * q + e < p ? pq[e] : 0;
            p32 += pim;
            a32 += (int)__builtin_amdgcn_sbfe(cbuf[u][q], 8 * e, 8) * pim;
          }
        }
        acc[0] += a32;
        psum += p32;
      }
    }
    if (vg == 0) {
      for (int i = 0; i <= j; ++i) {
        const int t = p + i;
        if (nsplit == 1 || ((t >> 6) % nsplit) == c) {            // the split that owns position t's block adds it
          const int pi = s_pi[t];
          psum += pi;
          acc[0] += (long long)((int)s_vn[i * D + vd] * pi);
        }
      }
    }
    s_acc[vg * D + vd] = acc[0] - (long long)zv * psum;
  }
  const int items = VCH ? 0 : my_blocks * PPB;
  MQ_ATTN_PV_FLAT(p)
  if (!VCH && grp == 0) {
    for (int i = 0; i <= j; ++i) {
      const int t = p + i;
      if (nsplit == 1 || ((t >> 6) % nsplit) == c) MQ_ATTN_PV_ADD_NEW(s_vn + i * D, s_pi[t])   // the split that owns position t's block adds it
    }
  }
  if constexpr (!VCH) {
    MQ_ATTN_FOLD_GROUPS;
  }
  __syncthreads();
  // this row's split scratch, tickets and output row
  MQ_ATTN_FINISH(VCH ? NG : G,
                 unsigned long long* part = reinterpret_cast<unsigned long long*>(a.part) + (size_t)r * a.nsplit * H * D;
                 unsigned* ticket = a.ticket + (size_t)r * H;, part, ticket,
                 const size_t o = ((size_t)r * H + h) * D + tid;, o)
}

template <bool VCH, bool TABLE>
struct RowsKernels {
  template <int D>
  static constexpr auto kernel = decode_attention_rows_kernel<D, VCH, TABLE>;
};

}  // namespace mq

using namespace mq;

extern "C" {

int mq_decode_attention_multi(const mq_decode_attention_multi_args* args, mq_stream_t stream) {
  MQ_REQUIRE(args != nullptr, "mq_decode_attention_multi: null argument block");
  const int rc = check_row_run_attention("mq_decode_attention_multi", args->a, args->rows, args->qkv_stride, args->v_chunked);
  if (rc != MQ_OK) return rc;
  mq_decode_attention_ragged_args ra = {};                         // one cache, no table: the kernel's TABLE = false locator
  ra.a = args->a, ra.rows = args->rows, ra.batch = 1, ra.split_from = args->split_from, ra.qkv_stride = args->qkv_stride;
  return args->v_chunked ? launch_attention_rows<RowsKernels<true, false>>("mq_decode_attention_multi", ra, ra.a, ra.rows, stream)
                         : launch_attention_rows<RowsKernels<false, false>>("mq_decode_attention_multi", ra, ra.a, ra.rows, stream);
}

int mq_decode_attention_ragged(const mq_decode_attention_ragged_args* args, mq_stream_t stream) {
  MQ_REQUIRE(args != nullptr, "mq_decode_attention_ragged: null argument block");
  const int R = args->rows, B = args->batch;
  MQ_REQUIRE(R >= 1 && R <= MQ_DECODE_MAX_BATCH, "mq_decode_attention_ragged: rows=%d outside 1..%d", R, MQ_DECODE_MAX_BATCH);      // (its message wins over batch's and the table's)
  MQ_REQUIRE(B >= 1 && B <= MQ_DECODE_MAX_BATCH, "mq_decode_attention_ragged: batch=%d outside 1..%d", B, MQ_DECODE_MAX_BATCH);
  MQ_REQUIRE(args->row_seq && args->row_pos, "mq_decode_attention_ragged: null row table (row_seq / row_pos)");
  mq_decode_attention_args a = args->a;
  a.pos = args->row_pos;                                           // (a.pos is not read: the positions are the table's)
  const int rc = check_row_run_attention("mq_decode_attention_ragged", a, R, args->qkv_stride, 0);
  if (rc != MQ_OK) return rc;
  return launch_attention_rows<RowsKernels<false, true>>("mq_decode_attention_ragged", *args, args->a, R, stream);
}

}  // extern "C"
