// Multi-token decode step: the attention of up to MQ_DECODE_MAX_BATCH CONSECUTIVE positions of one sequence in one launch
// (DecodeEngine.step_tokens / extend and speculative verification, mobilequant_amd/decode.py).
//   mq_decode_attention_multi : decode_attention_batch_kernel<D> (mq_decode_batch.hip) on a (heads, nsplit, rows) grid over ONE cache;
//                               the phases both share are the MQ_ATTN_* texts of mq_decode_attention.h
// Row j is position p + j.  It reads the cached positions t < p, and positions p .. p + j are appended by rows 0 .. j of this very
// launch, so no workgroup may read them back from memory: each workgroup builds the rows' new keys and values of its KV head in LDS
// with the batched kernel's RoPE / quantizer expressions (attn_new_elem) and takes them from there.  Everything else -- the score
// expression, the max, the float sum of the exponentials in its thread / wave order, the probability grid, the split protocol -- is
// decode_attention_batch_kernel's at T = p + j + 1, so row j's bits are that launch's for position p + j.  The p.v sums are exact
// integers: the cached positions go through the batched kernel's loop (flat value layout) or, with v_chunked, through 16-position
// chunks of one dimension per 16-byte request (the four-launch kernel's mapping); the new positions are added from LDS by the split
// that owns their 64-position block.
#include "mq_decode_attention.h"

namespace mq {

#pragma clang fp contract(off)

template <int D, bool VCH>
__global__ void __launch_bounds__(256) decode_attention_multi_kernel(const mq_decode_attention_multi_args ma) {
  const mq_decode_attention_args& a = ma.a;
  MQ_ATTN_GEOMETRY(D);
  MQ_ATTN_LDS(s_q8[D], s_kn[DB_MAXB * D], s_vn[DB_MAXB * D]);      // this row's q; rows 0 .. j's new k / v
  const int H = a.heads, rot = a.rot_dim, j = blockIdx.z, CL = a.cache_len;
  const int p = a.pos[0], pos = p + j;
  if (p < 0 || pos >= CL) return;                                  // a row past the cache: nothing is read or written
  const int nsplit = pos >= ma.split_from ? a.nsplit : 1;
  const int h = blockIdx.x, c = blockIdx.y, kvh = h / (H / a.kv_heads);
  if (c >= nsplit) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float cv = a.consts[lane];
  const int8_t* kc = a.k_cache + (size_t)kvh * CL * D;
  const int8_t* vc = a.v_cache + (size_t)kvh * CL * D;            // (both layouts: a KV head's values are cache_len * D bytes)
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
  // ---- RoPE + the input quantizers: this row's q, rows 0 .. j's new k / v ---------------------------------------------------------
  int qsum_part = 0;
  if (tid < D) {
    const int half = rot >> 1;
    const int dpart = tid < rot ? (tid < half ? tid + half : tid - half) : tid;
    const int dr = tid < rot ? tid : 0;
    float cs = 0.f, sn = 0.f;
    for (int i = 0; i <= j; ++i) {
      const float* row = a.qkv + (size_t)i * ma.qkv_stride;
      const float* kp = row + (size_t)H * D + (size_t)kvh * D;
      const float* vp = row + (size_t)(H + a.kv_heads) * D + (size_t)kvh * D;
      cs = a.cos[(size_t)(p + i) * rot + dr];
      sn = a.sin[(size_t)(p + i) * rot + dr];
      s_kn[i * D + tid] = attn_new_elem(kp[tid], kp[dpart], cs, sn, tid, rot, qb);
      s_vn[i * D + tid] = attn_new_elem(vp[tid], 0.f, 0.f, 0.f, tid, 0, pb);
    }
    const float* qp = a.qkv + (size_t)j * ma.qkv_stride + (size_t)h * D;
    const int8_t sq = attn_new_elem(qp[tid], qp[dpart], cs, sn, tid, rot, qa);      // (cs / sn: position p + j, the loop's last)
    s_q8[tid] = sq;
    qsum_part = sq;
    if (c == 0 && h % (H / a.kv_heads) == 0) {                     // the group's first head appends row j's position
      int8_t* k_cache = a.k_cache + (size_t)kvh * CL * D;
      int8_t* v_cache = a.v_cache + (size_t)kvh * CL * D;
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
  // cached positions from registers, the new ones (t >= p: row t - p, clamped -- t >= T is masked) from LDS
  MQ_ATTN_SCORES(t >= p ? MQ_ATTN_LDS_FRAG(s_kn + (t - p < j ? t - p : j) * D, ch) : kbuf[u][ch]);
  MQ_ATTN_SOFTMAX;
  // ---- p.v: exact integers.  Cached positions t < p over this split's blocks, then the new positions p .. pos from LDS -------------
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
                 unsigned long long* part = reinterpret_cast<unsigned long long*>(a.part) + (size_t)j * a.nsplit * H * D;
                 unsigned* ticket = a.ticket + (size_t)j * H;, part, ticket,
                 const size_t o = ((size_t)j * H + h) * D + tid;, o)
}

}  // namespace mq

using namespace mq;

extern "C" {

int mq_decode_attention_multi(const mq_decode_attention_multi_args* args, mq_stream_t stream) {
  MQ_REQUIRE(args != nullptr, "mq_decode_attention_multi: null argument block");
  const mq_decode_attention_args& a = args->a;
  const int R = args->rows;
  MQ_REQUIRE(R >= 1 && R <= MQ_DECODE_MAX_BATCH, "mq_decode_attention_multi: rows=%d outside 1..%d", R, MQ_DECODE_MAX_BATCH);
  int rc = check_five_launch_attention_shape("mq_decode_attention_multi", a);
  if (rc != MQ_OK) return rc;
  MQ_REQUIRE(args->v_chunked == 0 || args->v_chunked == 1, "mq_decode_attention_multi: v_chunked=%d (0 or 1)", args->v_chunked);
  MQ_REQUIRE(!args->v_chunked || a.cache_len % 16 == 0, "mq_decode_attention_multi: v_chunked needs cache_len %% 16 == 0 (cache_len=%d)", a.cache_len);
  rc = check_five_launch_attention_grids("mq_decode_attention_multi", a);
  if (rc != MQ_OK) return rc;
  MQ_REQUIRE(a.prefetch_wgs == 0, "mq_decode_attention_multi: no prefetch rows (prefetch_wgs must be 0)");
  MQ_REQUIRE(R == 1 || args->qkv_stride >= (int64_t)(a.heads + 2 * a.kv_heads) * a.head_dim, "mq_decode_attention_multi: qkv_stride must cover a q | k | v row");
  const size_t lds = (size_t)a.cache_len * sizeof(float);
  const int di = a.head_dim == 32 ? 0 : a.head_dim == 64 ? 1 : a.head_dim == 128 ? 2 : 3, vi = args->v_chunked ? 1 : 0;
  static const void* const fns[4][2] = {
      {reinterpret_cast<const void*>(decode_attention_multi_kernel<32, false>), reinterpret_cast<const void*>(decode_attention_multi_kernel<32, true>)},
      {reinterpret_cast<const void*>(decode_attention_multi_kernel<64, false>), reinterpret_cast<const void*>(decode_attention_multi_kernel<64, true>)},
      {reinterpret_cast<const void*>(decode_attention_multi_kernel<128, false>), reinterpret_cast<const void*>(decode_attention_multi_kernel<128, true>)},
      {reinterpret_cast<const void*>(decode_attention_multi_kernel<256, false>), reinterpret_cast<const void*>(decode_attention_multi_kernel<256, true>)}};
  static std::atomic<size_t> lds_set[8][kMaxDevices];
  rc = set_lds(fns[di][vi], lds_set[2 * di + vi], lds, "mq_decode_attention_multi");
  if (rc != MQ_OK) return rc;
  const dim3 grid((unsigned)a.heads, (unsigned)a.nsplit, (unsigned)R);
  hipStream_t st = as_stream(stream);
#define MQ_DM_LAUNCH(DD)                                                                                          \
  if (vi) decode_attention_multi_kernel<DD, true><<<grid, 256, lds, st>>>(*args);                                 \
  else decode_attention_multi_kernel<DD, false><<<grid, 256, lds, st>>>(*args);
  switch (a.head_dim) {
    case 32: MQ_DM_LAUNCH(32); break;
    case 64: MQ_DM_LAUNCH(64); break;
    case 128: MQ_DM_LAUNCH(128); break;
    default: MQ_DM_LAUNCH(256); break;
  }
#undef MQ_DM_LAUNCH
  MQ_LAUNCH_CHECK("mq_decode_attention_multi");
  return MQ_OK;
}

}  // extern "C"
