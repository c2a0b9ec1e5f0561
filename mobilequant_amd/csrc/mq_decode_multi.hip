// Multi-token decode step: the attention of up to MQ_DECODE_MAX_BATCH CONSECUTIVE positions of one sequence in one launch
// (DecodeEngine.step_tokens / extend and speculative verification, mobilequant_amd/decode.py).
//   mq_decode_attention_multi : decode_attention_batch_kernel<D> (mq_decode_batch.hip) on a (heads, nsplit, rows) grid over ONE cache
// Row j is position p + j.  It reads the cached positions t < p, and positions p .. p + j are appended by rows 0 .. j of this very
// launch, so no workgroup may read them back from memory: each workgroup builds the rows' new keys and values of its KV head in LDS
// with the batched kernel's RoPE / quantizer expressions (attn_new_elem) and takes them from there.  Everything else -- the score
// expression, the max, the float sum of the exponentials in its thread / wave order, the probability grid, the split protocol -- is
// decode_attention_batch_kernel's at T = p + j + 1, so row j's bits are that launch's for position p + j.  The p.v sums are exact
// integers: the cached positions go through the batched kernel's loop (flat value layout) or, with v_chunked, through 16-position
// chunks of one dimension per 16-byte request (the four-launch kernel's mapping); the new positions are added from LDS by the split
// that owns their 64-position block.
#include "mq_decode_common.h"

namespace mq {

#pragma clang fp contract(off)

template <int D, bool VCH>
__global__ void __launch_bounds__(256) decode_attention_multi_kernel(const mq_decode_attention_multi_args ma) {
  const mq_decode_attention_args& a = ma.a;
  constexpr int LPP = D >= 64 ? 4 : 2, CH = D >= 64 ? D / 64 : 1, PPP = 256 / LPP, KB = 8 / CH;
  constexpr int DQ = D / 4, G = 256 / DQ, PPB = 64 / G, VB = 16;
  static_assert(PPB * G == 64 && VB % PPB == 0, "block mapping");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* s_sc = reinterpret_cast<float*>(smem_raw);              // [cache_len] scores -> exp -> (p index - zp) as int
  __shared__ __attribute__((aligned(16))) int8_t s_q8[D], s_kn[DB_MAXB * D], s_vn[DB_MAXB * D];   // this row's q; rows 0 .. j's new k / v
  __shared__ float s_redf[4];
  __shared__ int s_redq[4];
  __shared__ long long s_acc[1024];                              // [G][D] partial p.v sums
  __shared__ unsigned s_ticket;
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
  const int sub = tid & (LPP - 1), slot = tid / LPP;
  v4i kbuf[KB][CH];
  auto load_keys = [&](int t0) {
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      const int t = t0 + u * PPP + slot;
      const int tc = t < p ? t : 0;                                 // position 0 stands in (always valid memory); masked below
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) kbuf[u][ch] = *reinterpret_cast<const v4i*>(kc + (size_t)tc * D + (sub * CH + ch) * 16);
    }
  };
  load_keys(0);
  const int dq = tid & (DQ - 1), grp = tid / DQ;
  int vbuf[VB];
  auto item_pos = [&](int i) { return 64 * (c + nsplit * (i / PPB)) + grp + G * (i % PPB); };
  auto load_values = [&](int i0) {                               // (flat layout) dimensions 4 dq .. 4 dq + 3 of VB positions
#pragma unroll
    for (int u = 0; u < VB; ++u) {
      const int t = item_pos(i0 + u);
      vbuf[u] = *reinterpret_cast<const int*>(vc + (size_t)(t < p ? t : 0) * D + dq * 4);
    }
  };
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
  // ---- RoPE + the input quantizers: this row's q, rows 0 .. j's new k / v ---------------------------------------------------------
  const Grid qa = const_grid(cv, AG_QK_A, a.qk_a), qb = const_grid(cv, AG_QK_B, a.qk_b), qo = const_grid(cv, AG_QK_OUT, a.qk_out);
  const Grid pa = const_grid(cv, AG_PV_A, a.pv_a), pb = const_grid(cv, AG_PV_B, a.pv_b), po = const_grid(cv, AG_PV_OUT, a.pv_out);
  const Grid oi = const_grid(cv, AG_O_IN, a.o_in);
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
  {
    const int w = wave_sum_dpp(qsum_part);
    if (lane == 0) s_redq[wv] = w;
  }
  __syncthreads();
  const int qsum = (s_redq[0] + s_redq[1]) + (s_redq[2] + s_redq[3]);
  const int zq = (int)qa.o - 128, zk = (int)qb.o - 128, zv = (int)pb.o - 128, zp = (int)pa.o;
  const float alpha_qk = __fmul_rn(qa.s, qb.s), alpha_pv = __fmul_rn(pa.s, pb.s);
  const int qconst = D * zq * zk - zk * qsum;
  v4i qf[CH];
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) qf[ch] = *reinterpret_cast<const v4i*>(s_q8 + (sub * CH + ch) * 16);
  const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
  // ---- scores: cached positions from registers, the new ones from LDS ------------------------------------------------------------
  float lmax = -INFINITY;
  for (int t0 = 0; t0 < T; t0 += KB * PPP) {
    if (t0 > 0) load_keys(t0);
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      if (t0 + u * PPP >= T) break;
      const int t = t0 + u * PPP + slot;
      const int ni = t < p ? 0 : (t - p < j ? t - p : j);           // new row of position t >= p (clamped: t >= T is masked)
      int dot = 0, ks = 0;
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) {
        const v4i kf = t >= p ? *reinterpret_cast<const v4i*>(s_kn + ni * D + (sub * CH + ch) * 16) : kbuf[u][ch];
        dot = dot16(kf, qf[ch], dot);
        ks = dot16(kf, ones, ks);
      }
      dot = quad_sum<LPP>(dot);
      ks = quad_sum<LPP>(ks);
      if (t < T && sub == 0) {
        const float sc = attn_score<D>(dot, ks, zq, qconst, alpha_qk, qo);
        s_sc[t] = sc;
        lmax = fmaxf(lmax, sc);
      }
    }
  }
  lmax = wave_max_f(lmax);
  if (lane == 0) s_redf[wv] = lmax;
  __syncthreads();
  const float mx = fmaxf(fmaxf(s_redf[0], s_redf[1]), fmaxf(s_redf[2], s_redf[3]));
  __syncthreads();
  float lsum = 0.f;
  for (int t = tid; t < T; t += 256) {
    const float e = expf(s_sc[t] - mx);
    s_sc[t] = e;
    lsum += e;
  }
  lsum = wave_sum_f(lsum);
  if (lane == 0) s_redf[wv] = lsum;
  __syncthreads();
  const float tot_e = (s_redf[0] + s_redf[1]) + (s_redf[2] + s_redf[3]);
  int* s_pi = reinterpret_cast<int*>(s_sc);
  for (int t = tid; t < T; t += 256) {
    if (nsplit == 1 || ((t >> 6) % nsplit) == c) {
      const float pr = __fdiv_rn(s_sc[t], tot_e);
      const float ip = dq_index(pr, pa.s, pa.inv_s, pa.o, pa.qmin, pa.qmax);
      s_pi[t] = (ip != ip ? 0 : (int)ip) - zp;
    }
  }
  __syncthreads();
  // ---- p.v: exact integers.  Cached positions t < p over this split's blocks, then the new positions p .. pos from LDS -------------
  long long acc[4] = {0, 0, 0, 0};
  long long psum = 0;
  const int nblk = (p + 63) >> 6;
  const int my_blocks = c < nblk ? (nblk - 1 - c) / nsplit + 1 : 0;
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
  for (int i0 = 0; i0 < items; i0 += VB) {
    if (i0 > 0) load_values(i0);
    int a32[4] = {0, 0, 0, 0}, p32 = 0;
#pragma unroll
    for (int u = 0; u < VB; ++u) {
      const int t = item_pos(i0 + u);
      const bool ok = i0 + u < items && t < p;
      const int pi = s_pi[ok ? t : 0];
      const int pim = ok ? pi : 0;
      p32 += pim;
#pragma unroll
      for (int e = 0; e < 4; ++e) a32[e] += (int)__builtin_amdgcn_sbfe(vbuf[u], 8 * e, 8) * pim;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += a32[e];
    psum += p32;
  }
  if (!VCH && grp == 0) {
    for (int i = 0; i <= j; ++i) {
      const int t = p + i;
      if (nsplit == 1 || ((t >> 6) % nsplit) == c) {              // the split that owns position t's block adds it
        const int sv4 = *reinterpret_cast<const int*>(s_vn + i * D + dq * 4);
        const int pi = s_pi[t];
        psum += pi;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += (long long)((int)__builtin_amdgcn_sbfe(sv4, 8 * e, 8) * pi);
      }
    }
  }
  if constexpr (!VCH) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] -= (long long)zv * psum;
#pragma unroll
    for (int e = 0; e < 4; ++e) s_acc[grp * D + dq * 4 + e] = acc[e];
  }
  __syncthreads();
  long long tot = 0;
  if (tid < D) {
#pragma unroll
    for (int gq = 0; gq < (VCH ? NG : G); ++gq) tot += s_acc[gq * D + tid];
  }
  if (nsplit > 1) {
    // this row's split scratch and tickets; the protocol of decode_attention_kernel
    unsigned long long* part = reinterpret_cast<unsigned long long*>(a.part) + (size_t)j * a.nsplit * H * D;
    unsigned* ticket = a.ticket + (size_t)j * H;
    if (tid < D) __hip_atomic_store(part + ((size_t)c * H + h) * D + tid, (unsigned long long)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(ticket + h, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != (unsigned)(nsplit - 1)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (tid == 0) __hip_atomic_store(ticket + h, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < D) {
      tot = 0;
      for (int cc = 0; cc < nsplit; ++cc)
        tot += (long long)__hip_atomic_load(part + ((size_t)cc * H + h) * D + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (tid < D) {
    const size_t o = ((size_t)j * H + h) * D + tid;
    const float pre = (float)((double)tot * (double)alpha_pv);
    const float y = po.fq(pre);
    if (a.out) a.out[o] = y;
    if (a.out_q) {
      const float qi = dq_index(y, oi.s, oi.inv_s, oi.o, oi.qmin, oi.qmax);
      a.out_q[o] = (int8_t)((qi != qi ? (int)oi.qmin : (int)qi) - 128);
    }
  }
}

}  // namespace mq

using namespace mq;

extern "C" {

// the five-launch attention's bound (mq_decode.hip kAttnMaxCache): 4 bytes of LDS per cached position plus the static arrays (<= 13 KiB
// at head_dim 256 with the new rows' keys and values)
constexpr int kMultiAttnMaxCache = 32768;

int mq_decode_attention_multi(const mq_decode_attention_multi_args* args, mq_stream_t stream) {
  MQ_REQUIRE(args != nullptr, "mq_decode_attention_multi: null argument block");
  const mq_decode_attention_args& a = args->a;
  const int R = args->rows;
  MQ_REQUIRE(R >= 1 && R <= MQ_DECODE_MAX_BATCH, "mq_decode_attention_multi: rows=%d outside 1..%d", R, MQ_DECODE_MAX_BATCH);
  MQ_REQUIRE(a.qkv && a.k_cache && a.v_cache && a.cos && a.sin && a.pos && a.consts && (a.out || a.out_q), "mq_decode_attention_multi: null pointer");
  MQ_REQUIRE(a.heads > 0 && a.kv_heads > 0 && a.heads % a.kv_heads == 0 && (a.head_dim == 32 || a.head_dim == 64 || a.head_dim == 128 || a.head_dim == 256) &&
                 a.cache_len > 0 && a.cache_len <= kMultiAttnMaxCache && a.rot_dim > 0 && a.rot_dim <= a.head_dim && a.rot_dim % 2 == 0,
             "mq_decode_attention_multi: heads=%d kv_heads=%d head_dim=%d (32 / 64 / 128 / 256) cache_len=%d (<= %d) rot_dim=%d", a.heads, a.kv_heads,
             a.head_dim, a.cache_len, kMultiAttnMaxCache, a.rot_dim);
  MQ_REQUIRE(args->v_chunked == 0 || args->v_chunked == 1, "mq_decode_attention_multi: v_chunked=%d (0 or 1)", args->v_chunked);
  MQ_REQUIRE(!args->v_chunked || a.cache_len % 16 == 0, "mq_decode_attention_multi: v_chunked needs cache_len %% 16 == 0 (cache_len=%d)", a.cache_len);
  MQ_REQUIRE(a.nsplit >= 1 && a.nsplit <= 16 && (a.nsplit == 1 || (a.part && a.ticket)), "mq_decode_attention_multi: nsplit=%d (1..16; > 1 needs part and ticket)", a.nsplit);
  MQ_REQUIRE(a.qk_a.scale && a.qk_b.scale && a.pv_a.scale && a.pv_b.scale && a.qk_a.qmin == 0.f && a.qk_a.qmax == 255.f && a.qk_b.qmin == 0.f &&
                 a.qk_b.qmax == 255.f && a.pv_b.qmin == 0.f && a.pv_b.qmax == 255.f && a.pv_a.qmin == 0.f && a.pv_a.qmax <= 65535.f,
             "mq_decode_attention_multi: q / k / v need 8-bit unsigned grids, the probabilities an unsigned grid of at most 16 bits");
  MQ_REQUIRE(!a.out_q || (a.o_in.scale && a.o_in.qmin == 0.f && a.o_in.qmax == 255.f), "mq_decode_attention_multi: the int8 output image needs the consumer's 8-bit unsigned grid (o_in)");
  MQ_REQUIRE(aligned(a.k_cache, 16) && aligned(a.v_cache, 16) && aligned(a.consts, 16) && aligned(a.qkv, 4), "mq_decode_attention_multi: caches / consts must be 16-byte aligned");
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
  const int rc = set_lds(fns[di][vi], lds_set[2 * di + vi], lds, "mq_decode_attention_multi");
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
