// Batched decode step: up to MQ_DECODE_MAX_BATCH independent sequences advanced by the same launches (BatchDecodeEngine,
// mobilequant_amd/decode_batch.py).  At one token per step every launch of mq_decode.hip streams the whole weight image for one
// activation row and leaves the dot-product units almost idle; here the same stream feeds B rows.  The contract is PER SEQUENCE: row b
// of every launch computes, bit for bit, what the single-sequence launch computes for that sequence alone -- the same fp32 expressions
// in the same reduction orders (integer sums are exact in any order).
//   mq_decode_gemv_batch      : decode_gemv_kernel (five-launch subset) for B rows: B prologues interleaved over shared barriers, the
//                               B int8 images side by side in LDS, every 16-byte weight chunk contracted with all of them
//   mq_decode_attention_batch : decode_attention_kernel<D>'s phases (mq_decode_attention.h) on a (heads, nsplit, B) grid, per-sequence
//                               positions, caches and scratch
//   mq_decode_head_batch      : decode_head_kernel's final norm for B rows, then the fp32 lm_head streamed once for all of them
#include "mq_decode_attention.h"

namespace mq {

#pragma clang fp contract(off)

constexpr int DB_INFLIGHT = 12;      // weight chunks per lane in flight, as decode_gemv_kernel

// ---- weight stream x B activation rows ---------------------------------------------------------------------------------------------
// Roles, barriers, geometry and epilogue as decode_gemv_kernel (mq_decode.hip): PROLOGUE waves 0 .. DG_PRO-1 build the images, STREAM
// waves request weights and epilogue parameters first.  Per row b the prologue is thread p's walk over float4 p + 512 u, the per-thread
// partial in that order, wave_sum_f_rowbcast, then the DG_PRO wave partials added in wave order -- the rows' chains interleave, the barriers are
// shared.  Beyond DB_XH float4 per row the prologue re-reads x (and the norm weights) instead of holding them: the same values, so the
// same bits.
template <int XMODE, bool GATE, bool W4>
__global__ void __launch_bounds__(DG_THREADS) decode_gemv_batch_kernel(const mq_decode_gemv_batch_args ba, const int rows_per_wg) {
  const mq_decode_gemv_args& g = ba.g;
  const int B = ba.batch;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [B][K] int8 activation images
  __shared__ float s_red[DB_MAXB][DG_PRO], s_red2[DB_MAXB][DG_PRO];
  __shared__ int s_redi[DB_MAXB][DG_PRO];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int K = g.K;
  const float cv = g.consts[lane & 63];

  if (wave < DG_PRO) {
    // ================================================ PROLOGUE role ====================================================================
    gemv_batch_prologue<XMODE, DB_MAXB>(ba, smem, s_red, s_red2, s_redi, cv, lane, wave);
    return;
  }

  // ================================================== STREAM role ======================================================================
  const int sw = wave - DG_PRO;
  const int NL = GATE ? g.N >> 1 : g.N;                            // logical rows
  const int kchunks = W4 ? K >> 5 : K >> 4;                        // 16-byte chunks per weight row
  const int wrow = W4 ? K >> 1 : K;                                // bytes per weight row
  const int lchunks = GATE ? 2 * kchunks : kchunks;                // chunks per logical row
  const int cpl = (lchunks + 63) >> 6;
  const int row0 = blockIdx.x * rows_per_wg + sw;
  const int row_end = (blockIdx.x + 1) * rows_per_wg < NL ? (blockIdx.x + 1) * rows_per_wg : NL;
  const int prow = row0 + DG_STR * lane;                           // lane t keeps the parameters / results of row slot t
  const bool prow_ok = prow < row_end;
  v4i buf[DB_INFLIGHT];
  auto issue_pass = [&](int t, int j) {
#pragma unroll
    for (int u = 0; u < DB_INFLIGHT; ++u) {
      const int row = row0 + DG_STR * t;
      const int c = lane + 64 * j;
      if (row < row_end && c < lchunks)
        buf[u] = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(g.w + (size_t)row * (GATE ? 2 : 1) * wrow) + c);
      else
        buf[u] = v4i{0, 0, 0, 0};
      if (++j == cpl) { j = 0; ++t; }
    }
  };
  issue_pass(0, 0);
  float p_alpha[GATE ? 2 : 1], p_bias[GATE ? 2 : 1];
  int p_zp[GATE ? 2 : 1], p_ct[GATE ? 2 : 1];
#pragma unroll
  for (int h = 0; h < (GATE ? 2 : 1); ++h) {
    const int wr = GATE ? 2 * prow + h : prow;
    p_alpha[h] = prow_ok ? g.alpha[wr] : 0.f;
    p_zp[h] = prow_ok ? g.w_zp[wr] : 0;
    p_ct[h] = prow_ok ? g.col_term[wr] : 0;
    p_bias[h] = (prow_ok && g.bias) ? g.bias[wr] : 0.f;
  }
  float p_res[DB_MAXB];
#pragma unroll
  for (int b = 0; b < DB_MAXB; ++b) p_res[b] = (!GATE && g.resid && prow_ok && b < B) ? g.resid[(size_t)b * ba.y_stride + prow] : 0.f;
  gemv_batch_stream_barriers<XMODE>();
  if (row0 >= row_end) return;

  const GemvBatchEpilogue ep(cv, g);

  // ---- dot products against all B images, DPP reductions per completed logical row ----------------------------------------------
  const int nslots = (row_end - row0 + DG_STR - 1) / DG_STR;
  int acc0[DB_MAXB], acc1[DB_MAXB], sum0[DB_MAXB], sum1[DB_MAXB];
#pragma unroll
  for (int b = 0; b < DB_MAXB; ++b) acc0[b] = acc1[b] = sum0[b] = sum1[b] = 0;
  int t = 0, j = 0;
  while (t < nslots) {
    int t2 = t, j2 = j;
#pragma unroll
    for (int u = 0; u < DB_INFLIGHT; ++u) {
      if (t2 < nslots) {
        int c = lane + 64 * j2;
        c = c < lchunks ? c : lchunks - 1;                       // buf[u] is zero there
        const int ck = GATE ? (c >= kchunks ? c - kchunks : c) : c;
        const bool second = GATE && c >= kchunks;
        v4i w_lo = buf[u], w_hi = buf[u];
        if constexpr (W4) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            w_lo[e] = buf[u][e] & 0x0f0f0f0f;
            w_hi[e] = (int)(((unsigned)buf[u][e] >> 4) & 0x0f0f0f0fu);
          }
        }
#pragma unroll
        for (int b = 0; b < DB_MAXB; ++b) {
          if (b < B) {
            const char* img = smem + (size_t)b * K;
            int part;
            if constexpr (W4) {
              const v4i a_lo = *reinterpret_cast<const v4i*>(img + (size_t)ck * 32), a_hi = *reinterpret_cast<const v4i*>(img + (size_t)ck * 32 + 16);
              part = dot16(w_hi, a_hi, dot16(w_lo, a_lo, 0));
            } else {
              part = dot16(w_lo, *reinterpret_cast<const v4i*>(img + (size_t)ck * 16), 0);
            }
            if (second) acc1[b] += part;
            else acc0[b] += part;
          }
        }
        if (j2 == cpl - 1) {                                     // logical row slot t2 complete
#pragma unroll
          for (int b = 0; b < DB_MAXB; ++b) {
            if (b < B) {
              const int s0 = wave_sum_dpp(acc0[b]), s1 = GATE ? wave_sum_dpp(acc1[b]) : 0;
              acc0[b] = acc1[b] = 0;
              if (lane == t2) {
                sum0[b] = s0;
                sum1[b] = s1;
              }
            }
          }
        }
        if (++j2 == cpl) { j2 = 0; ++t2; }
      }
    }
    t = t2;
    j = j2;
    if (t < nslots) issue_pass(t, j);
  }
  // ---- epilogue, one row per LANE, every batch row in turn ----------------------------------------------------------------------------
  if (lane < nslots) {
    const int row = prow;
#pragma unroll
    for (int b = 0; b < DB_MAXB; ++b) {
      if (b < B) {
        int rsb = 0;                                             // row b's image sum (read here: no registers held over the stream)
#pragma unroll
        for (int w = 0; w < DG_PRO; ++w) rsb += s_redi[b][w];
        float e0, e1 = 0.f;
        {
          const int tt = (int)((unsigned)sum0[b] - (unsigned)p_zp[0] * (unsigned)rsb + (unsigned)p_ct[0]);
          e0 = __fadd_rn(__fmul_rn((float)tt, p_alpha[0]), p_bias[0]);
        }
        if constexpr (GATE) {
          const int tt = (int)((unsigned)sum1[b] - (unsigned)p_zp[GATE ? 1 : 0] * (unsigned)rsb + (unsigned)p_ct[GATE ? 1 : 0]);
          e1 = __fadd_rn(__fmul_rn((float)tt, p_alpha[GATE ? 1 : 0]), p_bias[GATE ? 1 : 0]);
        }
        ep.store<GATE>(ba, b, row, e0, e1, p_res[b]);
      }
    }
  }
}

// ---- attention of one query token per sequence over its own static INTEGER KV cache -------------------------------------------------
// decode_attention_kernel<D> (mq_decode.hip) with a third grid dimension: workgroup (h, c, b) is head h, split c of sequence b, with
// that sequence's position, q | k | v row, caches, output row and split scratch.  The split count is chosen here from the position
// (nsplit from split_from cached positions on, else 1; the other workgroups exit): the scores and the softmax are computed whole by
// every split and the p.v partials are exact integers, so the result bits do not depend on it.  No prefetch rows.
// The phases are the MQ_ATTN_* texts of mq_decode_attention.h; this kernel's own are the per-sequence offsets and split_from.
template <int D>
__global__ void __launch_bounds__(256) decode_attention_batch_kernel(const mq_decode_attention_batch_args ba) {
  const mq_decode_attention_args& a = ba.a;
  MQ_ATTN_GEOMETRY(D);
  MQ_ATTN_LDS(s_q8[D], s_k8[D], s_v8[D]);
  const int H = a.heads, rot = a.rot_dim, sb = blockIdx.z;
  const int pos = a.pos[sb];
  if (pos < 0 || pos >= a.cache_len) return;                       // an idle slot (or a step past the cache): nothing is read or written
  const int nsplit = pos >= ba.split_from ? a.nsplit : 1;
  const int h = blockIdx.x, c = blockIdx.y, kvh = h / (H / a.kv_heads);
  if (c >= nsplit) return;                                         // surplus split workgroup of a short sequence
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float cv = a.consts[lane];
  const size_t cache_seq = (size_t)a.kv_heads * a.cache_len * D;
  int8_t* const k_cache = a.k_cache + sb * cache_seq;
  int8_t* const v_cache = a.v_cache + sb * cache_seq;
  const float* qkv = a.qkv + (size_t)sb * ba.qkv_stride;
  const float* qp = qkv + (size_t)h * D;
  const float* kp = qkv + (size_t)H * D + (size_t)kvh * D;
  const float* vp = qkv + (size_t)(H + a.kv_heads) * D + (size_t)kvh * D;
  const int dd = tid < D ? tid : D - 1;
  const int half = rot >> 1;
  const int dpart = dd < rot ? (dd < half ? dd + half : dd - half) : dd;
  const float q_raw = qp[dd], q_par = qp[dpart], k_raw = kp[dd], k_par = kp[dpart], v_raw = vp[dd];
  const int T = pos + 1;
  const int dr = dd < rot ? dd : 0;
  const float cs = a.cos[(size_t)pos * rot + dr], sn = a.sin[(size_t)pos * rot + dr];
  const int8_t* kc = k_cache + (size_t)kvh * a.cache_len * D;
  const int8_t* vc = v_cache + (size_t)kvh * a.cache_len * D;
  MQ_ATTN_KEY_LOADER(t < T && t != pos);
  MQ_ATTN_VALUE_LOADER(pos);
  load_values(0);
  MQ_ATTN_GRIDS;
  MQ_ATTN_NEW_TOKEN(k_cache, v_cache)                              // (appends to this sequence's cache)
  MQ_ATTN_QSUM_REDUCE;
  MQ_ATTN_CONSTS;
  v4i qf[CH], kn[CH];                                              // this lane's share of the query / of the NEW key (never via memory)
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) {
    qf[ch] = MQ_ATTN_LDS_FRAG(s_q8, ch);
    kn[ch] = MQ_ATTN_LDS_FRAG(s_k8, ch);
  }
  MQ_ATTN_SCORES(t == pos ? kn[ch] : kbuf[u][ch]);
  MQ_ATTN_SOFTMAX;
  long long acc[4] = {0, 0, 0, 0};
  long long psum = 0;
  MQ_ATTN_SPLIT_BLOCKS(pos);
  const int items = my_blocks * PPB;
  MQ_ATTN_PV_FLAT(pos)
  if (grp == 0 && ((pos >> 6) % nsplit) == c) MQ_ATTN_PV_ADD_NEW(s_v8, s_pi[pos])
  MQ_ATTN_FOLD_GROUPS;
  __syncthreads();
  // this sequence's split scratch, tickets and output row
  MQ_ATTN_FINISH(G,
                 unsigned long long* part = reinterpret_cast<unsigned long long*>(a.part) + (size_t)sb * a.nsplit * H * D;
                 unsigned* ticket = a.ticket + (size_t)sb * H;, part, ticket,
                 const size_t o = ((size_t)sb * H + h) * D + tid;, o)
}

struct BatchKernels {
  template <int D>
  static constexpr auto kernel = decode_attention_batch_kernel<D>;
};

// ---- final norm for B rows + the fp32 lm_head streamed once -----------------------------------------------------------------------
// decode_head_kernel's arithmetic per row: the norm's reductions over 256 threads (i = tid, tid + 256, ...), wave_sum_f_rowbcast, the four wave
// partials as (w0 + w1) + (w2 + w3); a vocabulary row per wave, lane l summing float4 chunks l, l + 64, ... ascending with four adds
// each, then wave_sum_f_rowbcast.  Each lane holds B accumulators against one weight request.
__global__ void __launch_bounds__(256) decode_head_batch_kernel(const mq_decode_head_batch_args hb) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* s_x = reinterpret_cast<float*>(smem_raw);               // [B][K] normalised rows
  __shared__ float s_red[DB_MAXB][4], s_red2[DB_MAXB][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int B = hb.batch, K = (int)hb.K, V = (int)hb.V;
  const float* __restrict__ norm_w = hb.norm_weight;
  const float* __restrict__ norm_b = hb.norm_bias;
  const float eps = hb.eps;
  bool act[DB_MAXB];
#pragma unroll
  for (int b = 0; b < DB_MAXB; ++b) {
    const int pb = (hb.pos && b < B) ? hb.pos[b] : 0;
    act[b] = b < B && pb >= 0 && (!hb.pos || pb < hb.cache_len);
  }
  auto xr = [&](int b) { return hb.x + (size_t)b * hb.x_stride; };
  if (hb.layernorm) {
    float s1[DB_MAXB];
#pragma unroll
    for (int b = 0; b < DB_MAXB; ++b) s1[b] = 0.f;
    for (int i = tid; i < K; i += 256) {
#pragma unroll
      for (int b = 0; b < DB_MAXB; ++b)
        if (act[b]) s1[b] += xr(b)[i];
    }
#pragma unroll
    for (int b = 0; b < DB_MAXB; ++b) {
      if (act[b]) {
        const float t = wave_sum_f_rowbcast(s1[b]);
        if (lane == 0) s_red[b][wv] = t;
      }
    }
    __syncthreads();
    float mu[DB_MAXB], s2[DB_MAXB];
#pragma unroll
    for (int b = 0; b < DB_MAXB; ++b) {
      mu[b] = act[b] ? __fdiv_rn((s_red[b][0] + s_red[b][1]) + (s_red[b][2] + s_red[b][3]), (float)K) : 0.f;
      s2[b] = 0.f;
    }
    for (int i = tid; i < K; i += 256) {
#pragma unroll
      for (int b = 0; b < DB_MAXB; ++b) {
        if (act[b]) {
          const float d = xr(b)[i] - mu[b];
          s2[b] += d * d;
        }
      }
    }
#pragma unroll
    for (int b = 0; b < DB_MAXB; ++b) {
      if (act[b]) {
        const float t = wave_sum_f_rowbcast(s2[b]);
        if (lane == 0) s_red2[b][wv] = t;
      }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < DB_MAXB; ++b) {
      if (act[b]) {
        const float var = __fdiv_rn((s_red2[b][0] + s_red2[b][1]) + (s_red2[b][2] + s_red2[b][3]), (float)K);
        const float r = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(var, eps))), sh = __fmul_rn(-r, mu[b]);
        for (int i = tid; i < K; i += 256) {
          float y = __fadd_rn(__fmul_rn(xr(b)[i], r), sh);
          if (norm_w) y = __fmul_rn(y, norm_w[i]);
          if (norm_b) y = __fadd_rn(y, norm_b[i]);
          s_x[(size_t)b * K + i] = y;
        }
      }
    }
  } else {
    float ss[DB_MAXB];
#pragma unroll
    for (int b = 0; b < DB_MAXB; ++b) ss[b] = 0.f;
    for (int i = tid; i < K; i += 256) {
#pragma unroll
      for (int b = 0; b < DB_MAXB; ++b) {
        if (act[b]) {
          const float v = xr(b)[i];
          ss[b] += v * v;
        }
      }
    }
#pragma unroll
    for (int b = 0; b < DB_MAXB; ++b) {
      if (act[b]) {
        const float t = wave_sum_f_rowbcast(ss[b]);
        if (lane == 0) s_red[b][wv] = t;
      }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < DB_MAXB; ++b) {
      if (act[b]) {
        const float mean = __fdiv_rn((s_red[b][0] + s_red[b][1]) + (s_red[b][2] + s_red[b][3]), (float)K);
        const float r = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(mean, eps)));
        for (int i = tid; i < K; i += 256) s_x[(size_t)b * K + i] = norm_w ? __fmul_rn(norm_w[i], __fmul_rn(xr(b)[i], r)) : xr(b)[i];
      }
    }
  }
  __syncthreads();
  // a wave per vocabulary row; NV requests per lane in flight, each contracted with every active row
  constexpr int NV = 8;
  typedef float v4f __attribute__((ext_vector_type(4)));
  const int nvec = K >> 2;
  const int stride = gridDim.x * 4;
  for (int row = blockIdx.x * 4 + wv; row < V; row += stride) {
    const v4f* wr = reinterpret_cast<const v4f*>(hb.w + (size_t)row * K);
    float acc[DB_MAXB];
#pragma unroll
    for (int b = 0; b < DB_MAXB; ++b) acc[b] = 0.f;
    for (int i0 = lane; i0 < nvec; i0 += 64 * NV) {
      v4f wb[NV];
#pragma unroll
      for (int jj = 0; jj < NV; ++jj) {
        const int i = i0 + 64 * jj;
        wb[jj] = __builtin_nontemporal_load(wr + (i < nvec ? i : i0));
      }
#pragma unroll
      for (int jj = 0; jj < NV; ++jj) {
        const int i = i0 + 64 * jj;
        if (i < nvec) {
#pragma unroll
          for (int b = 0; b < DB_MAXB; ++b) {
            if (act[b]) {
              const float4 xb = reinterpret_cast<const float4*>(s_x + (size_t)b * K)[i];
              acc[b] += wb[jj][0] * xb.x;
              acc[b] += wb[jj][1] * xb.y;
              acc[b] += wb[jj][2] * xb.z;
              acc[b] += wb[jj][3] * xb.w;
            }
          }
        }
      }
    }
#pragma unroll
    for (int b = 0; b < DB_MAXB; ++b) {
      if (act[b]) {
        const float s = wave_sum_f_rowbcast(acc[b]);
        if (lane == 0) hb.logits[(size_t)b * hb.logits_stride + row] = hb.bias ? s + hb.bias[row] : s;
      }
    }
  }
}

}  // namespace mq

using namespace mq;

extern "C" {

int mq_decode_gemv_batch(const mq_decode_gemv_batch_args* args, mq_stream_t stream) {
  MQ_REQUIRE(args != nullptr, "mq_decode_gemv_batch: null argument block");
  const mq_decode_gemv_args& g = args->g;
  const int B = args->batch;
  MQ_REQUIRE(B >= 1 && B <= MQ_DECODE_MAX_BATCH, "mq_decode_gemv_batch: batch=%d outside 1..%d", B, MQ_DECODE_MAX_BATCH);
  MQ_REQUIRE(g.alpha && g.w_zp && g.col_term, "mq_decode_gemv_batch: null pointer");
  if (const int rc = check_gemv("mq_decode_gemv_batch", g, B, args->x_stride, args->y_stride, args->gate_stride, false)) return rc;
  MQ_REQUIRE((int64_t)B * g.K <= DB_MAX_IMAGE, "mq_decode_gemv_batch: batch * K = %lld exceeds the %d bytes of int8 images the workgroup holds in LDS",
             (long long)B * g.K, DB_MAX_IMAGE);
  MQ_REQUIRE(!g.zero_acc && !g.o_acc, "mq_decode_gemv_batch: zero_acc / o_acc (the four-launch chain) are not served by the batched launch");
  const bool gate = g.gate_q != nullptr;
  int rows_per_wg;
  unsigned grid;
  gemv_row_geometry(gate ? g.N / 2 : g.N, &rows_per_wg, &grid);
  const size_t lds = (size_t)B * g.K;
  hipStream_t st = as_stream(stream);
  const int xmode = gemv_xmode(g);
  static std::atomic<size_t> lds_set[16][kMaxDevices];            // per instantiation: xmode (4) x gate (2) x w4 (2)
  std::atomic<size_t>* const lds_cache = lds_set[gemv_kernel_index(xmode, gate, g.w4)];
  return gemv_dispatch(xmode, gate, g.w4, [&](auto xm, auto gt, auto w4) -> int {
    const auto kernel = decode_gemv_batch_kernel<decltype(xm)::value, decltype(gt)::value, decltype(w4)::value>;
    if (const int rc = set_lds(reinterpret_cast<const void*>(kernel), lds_cache, lds, "mq_decode_gemv_batch")) return rc;
    kernel<<<grid, DG_THREADS, lds, st>>>(*args, rows_per_wg);
    MQ_LAUNCH_CHECK("mq_decode_gemv_batch");
    return MQ_OK;
  });
}

int mq_decode_attention_batch(const mq_decode_attention_batch_args* args, mq_stream_t stream) {
  MQ_REQUIRE(args != nullptr, "mq_decode_attention_batch: null argument block");
  const mq_decode_attention_args& a = args->a;
  const int B = args->batch;
  MQ_REQUIRE(B >= 1 && B <= MQ_DECODE_MAX_BATCH, "mq_decode_attention_batch: batch=%d outside 1..%d", B, MQ_DECODE_MAX_BATCH);
  int rc = check_five_launch_attention("mq_decode_attention_batch", a);
  if (rc != MQ_OK) return rc;
  MQ_REQUIRE(a.prefetch_wgs == 0, "mq_decode_attention_batch: no prefetch rows (prefetch_wgs must be 0)");
  MQ_REQUIRE(B == 1 || args->qkv_stride >= (int64_t)(a.heads + 2 * a.kv_heads) * a.head_dim, "mq_decode_attention_batch: qkv_stride must cover a q | k | v row");
  return launch_attention_rows<BatchKernels>("mq_decode_attention_batch", *args, a, B, stream);
}

int mq_decode_head_batch(const mq_decode_head_batch_args* args, mq_stream_t stream) {
  MQ_REQUIRE(args != nullptr, "mq_decode_head_batch: null argument block");
  const mq_decode_head_batch_args& h = *args;
  const int B = h.batch;
  MQ_REQUIRE(B >= 1 && B <= MQ_DECODE_MAX_BATCH, "mq_decode_head_batch: batch=%d outside 1..%d", B, MQ_DECODE_MAX_BATCH);
  MQ_REQUIRE(h.x && h.w && h.logits, "mq_decode_head_batch: null pointer");
  MQ_REQUIRE(h.K > 0 && h.K % 4 == 0 && h.K <= 12288 && h.V > 0 && h.V <= INT32_MAX, "mq_decode_head_batch: bad arguments (K %% 4 == 0, K <= 12288, V > 0)");
  MQ_REQUIRE((int64_t)B * h.K <= 32768, "mq_decode_head_batch: batch * K = %lld exceeds the 32768 normalised floats the workgroup holds in LDS", (long long)B * h.K);
  MQ_REQUIRE(B == 1 || (h.x_stride >= h.K && h.logits_stride >= h.V), "mq_decode_head_batch: x_stride / logits_stride must cover a row");
  MQ_REQUIRE(aligned(h.w, 16), "mq_decode_head_batch: the weight must be 16-byte aligned");
  MQ_REQUIRE(!h.pos || h.cache_len > 0, "mq_decode_head_batch: pos needs cache_len > 0");
  int64_t blocks = (h.V + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;
  const size_t lds = (size_t)B * h.K * sizeof(float);
  static std::atomic<size_t> lds_set[kMaxDevices];
  const int rc = set_lds(reinterpret_cast<const void*>(decode_head_batch_kernel), lds_set, lds, "mq_decode_head_batch");
  if (rc != MQ_OK) return rc;
  decode_head_batch_kernel<<<(unsigned)blocks, 256, lds, as_stream(stream)>>>(h);
  MQ_LAUNCH_CHECK("mq_decode_head_batch");
  return MQ_OK;
}

}  // extern "C"
