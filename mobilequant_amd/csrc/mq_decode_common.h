// Device helpers shared by the single-sequence decode kernels (mq_decode.hip), the batched ones (mq_decode_batch.hip), the grouped
// GEMV (mq_decode_grouped.hip) and the multi-token / ragged attention (mq_decode_rows.hip): the
// launch-constants line, the layout constants the families agree on, the batched GEMV's prologue and epilogue and, on the host, what
// the three GEMV entries share: their argument checks (check_gemv), the dispatch over instantiations (gemv_dispatch) and the row
// geometry.  The five-launch attention's phases build on this header in mq_decode_attention.h.
#pragma once
#include <type_traits>
#include "mq_common.h"

namespace mq {

#pragma clang fp contract(off)

typedef int v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int dot16(const v4i a, const v4i b, int c) {
#pragma unroll
  for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_sdot4(a[e], b[e], c, false);
  return c;
}

constexpr int DG_THREADS = 1024, DG_WAVES = 16, DG_INFLIGHT = 12;   // 12: the w1|w3 launch (22 row pairs per CU over 8 stream waves: 3 x 4 chunks per lane) has every load in flight at once

// Constants block of a launch (mq_decode_pack_grids): grid k at floats [4k .. 4k+2] = scale, offset, 1 / scale.  ONE 128-byte load
// per wave at the very top of the kernel replaces up to 16 dependent pointer chases behind the barriers.
__device__ __forceinline__ Grid const_grid(const float cv, const int k, const mq_grid& g) {
  Grid r;
  r.on = g.scale != nullptr;
  r.s = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cv), 4 * k));
  r.o = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cv), 4 * k + 1));
  r.inv_s = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cv), 4 * k + 2));
  r.qmin = g.qmin;
  r.qmax = g.qmax;
  return r;
}
enum { CG_NORM_IN = 0, CG_A = 1, CG_OUT0 = 2, CG_OUT1 = 3, CG_OUT2 = 4, CG_GATE_MID = 5, CG_GATE_ACTOUT = 6, CG_GATE_OUT = 7, CG_COUNT = 8,
       CG_O_OUT = 8, CG_COUNT_R6 = 9 };   // round 6: slot 8 = o_proj's output grid (OPRE prologue; zero when unused)

enum { XM_NORM = 0, XM_F32 = 1, XM_I8 = 2, XM_LNORM = 3 };
constexpr int DG_PRO = 8, DG_STR = DG_WAVES - DG_PRO, DG_XPRE = 4;      // 512 prologue threads x 4 float4 -> K <= 8192 (fp32)

enum { AG_QK_A = 0, AG_QK_B = 1, AG_QK_OUT = 2, AG_PV_A = 3, AG_PV_B = 4, AG_PV_OUT = 5, AG_O_IN = 6, AG_COUNT = 7 };

// sum over aligned groups of N = 2 / 4 adjacent lanes: DPP quad permutes (a __shfl_xor is an LDS round trip, ~100 cycles each)
template <int N>
__device__ __forceinline__ int quad_sum(int v) {
  if (N == 1) return v;
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);                 // quad_perm [1,0,3,2]
  if (N == 4) v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);     // quad_perm [2,3,0,1]
  return v;
}

// ---- the five-launch GEMV over B activation rows: pieces shared by decode_gemv_batch_kernel (mq_decode_batch.hip) and
// decode_gemv_grouped_kernel (mq_decode_grouped.hip), which differ only in how a weight row is contracted with the images ----------
constexpr int DB_MAXB = MQ_DECODE_MAX_BATCH;
constexpr int DB_XH = 1;             // float4 per row and thread the prologue holds between its passes (K <= 2048); beyond that it re-reads

// PROLOGUE role (waves 0 .. DG_PRO-1): the B rows' int8 images (index - 128) into smem [B][K] and the per-wave partials of their
// image sums into s_redi[b][wave].  Per row b the prologue is thread p's walk over float4 p + 512 u, the per-thread partial in that
// order, wave_sum_f_rowbcast, then the DG_PRO wave partials added in wave order -- decode_gemv_kernel's arithmetic (mq_decode.hip); the rows'
// chains interleave, the barriers are shared (the STREAM waves mirror them with gemv_batch_stream_barriers).  Beyond DB_XH float4 per
// row the prologue re-reads x (and the norm weights) instead of holding them: the same values, so the same bits.  Ends on the
// barrier after which the images and the sums are complete.
template <int XMODE, int NB>
__device__ __forceinline__ void gemv_batch_prologue(const mq_decode_gemv_batch_args& ba, char* smem, float (*s_red)[DG_PRO], float (*s_red2)[DG_PRO],
                                                    int (*s_redi)[DG_PRO], const float cv, const int lane, const int wave) {
  const mq_decode_gemv_args& g = ba.g;
  const int B = ba.batch;
  const int K = g.K;
  const int p = threadIdx.x;                                     // 0 .. 511
  int my_sum[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) my_sum[b] = 0;
  if constexpr (XMODE == XM_I8) {                                // ready int8 images: copy + row sums
    const int nq = K >> 4;
    for (int i = p; i < nq; i += DG_PRO * 64) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b < B) {
          const v4i v = reinterpret_cast<const v4i*>(g.xq + (size_t)b * ba.x_stride)[i];
          reinterpret_cast<v4i*>(smem + (size_t)b * K)[i] = v;
#pragma unroll
          for (int e = 0; e < 4; ++e) my_sum[b] = __builtin_amdgcn_sdot4(v[e], 0x01010101, my_sum[b], false);
        }
      }
    }
  } else {
    const int nvec = K >> 2;
    constexpr bool ANYNORM = XMODE == XM_NORM || XMODE == XM_LNORM;
    const Grid ag = const_grid(cv, CG_A, g.a_grid);
    const Grid ng = const_grid(cv, CG_NORM_IN, g.norm_in);
    float4 xv[NB][DB_XH], nw[DB_XH], nb[DB_XH];
    auto xrow = [&](int b, int ic) { return reinterpret_cast<const float4*>(g.x + (size_t)b * ba.x_stride)[ic]; };
    auto fqv = [&](float4 v) {                                   // the norm's input quantizer, two elements per instruction
      const v2f lo2 = ng.fq2((v2f){v.x, v.y}), hi2 = ng.fq2((v2f){v.z, v.w});
      return make_float4(lo2.x, lo2.y, hi2.x, hi2.y);
    };
#pragma unroll
    for (int u = 0; u < DB_XH; ++u) {
      if (u * DG_PRO * 64 < nvec) {                              // wave-uniform
        const int i = p + u * DG_PRO * 64;
        const int ic = i < nvec ? i : nvec - 1;
#pragma unroll
        for (int b = 0; b < NB; ++b)
          if (b < B) xv[b][u] = xrow(b, ic);
        if constexpr (ANYNORM) nw[u] = reinterpret_cast<const float4*>(g.norm_w)[ic];
        if constexpr (XMODE == XM_LNORM)
          nb[u] = g.norm_bias ? reinterpret_cast<const float4*>(g.norm_bias)[ic] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    // row b's (normalised-input) float4 u: held, or re-read and re-quantised (fq: the norm modes' input quantizer applied)
    auto xval = [&](int b, int u, int ic, bool fq) {
      if (u < DB_XH) return xv[b][u < DB_XH ? u : 0];
      const float4 v = xrow(b, ic);
      return fq ? fqv(v) : v;
    };
    float r[NB], shiftv[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) r[b] = 1.f, shiftv[b] = 0.f;
    if constexpr (XMODE == XM_LNORM) {                           // QLayerNorm.forward, decode_gemv_kernel's arithmetic
      float s1[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) s1[b] = 0.f;
#pragma unroll
      for (int u = 0; u < DG_XPRE; ++u) {
        if (u * DG_PRO * 64 < nvec) {
          const int i = p + u * DG_PRO * 64, ic = i < nvec ? i : nvec - 1;
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            if (b < B) {
              float4 v;
              if (u < DB_XH) v = xv[b][u < DB_XH ? u : 0] = fqv(xv[b][u < DB_XH ? u : 0]);
              else v = fqv(xrow(b, ic));
              if (i < nvec) s1[b] += (v.x + v.y) + (v.z + v.w);
            }
          }
        }
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b < B) {
          const float t = wave_sum_f_rowbcast(s1[b]);
          if (lane == 0) s_red[b][wave] = t;
        }
      }
      __syncthreads();                                           // barrier 1 of 3
      float mu[NB], s2[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < DG_PRO; ++w) tot += s_red[b][w];
        mu[b] = __fdiv_rn(tot, (float)K);
        s2[b] = 0.f;
      }
#pragma unroll
      for (int u = 0; u < DG_XPRE; ++u) {
        if (u * DG_PRO * 64 < nvec && p + u * DG_PRO * 64 < nvec) {
          const int ic = p + u * DG_PRO * 64;
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            if (b < B) {
              const float4 v = xval(b, u, ic, true);
              const float d0 = v.x - mu[b], d1 = v.y - mu[b], d2 = v.z - mu[b], d3 = v.w - mu[b];
              s2[b] += d0 * d0;
              s2[b] += d1 * d1;
              s2[b] += d2 * d2;
              s2[b] += d3 * d3;
            }
          }
        }
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b < B) {
          const float t = wave_sum_f_rowbcast(s2[b]);
          if (lane == 0) s_red2[b][wave] = t;
        }
      }
      __syncthreads();                                           // barrier 2 of 3
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float tot2 = 0.f;
#pragma unroll
        for (int w = 0; w < DG_PRO; ++w) tot2 += s_red2[b][w];
        const float var = __fdiv_rn(tot2, (float)K);
        r[b] = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(var, g.eps)));
        shiftv[b] = __fmul_rn(-r[b], mu[b]);
      }
    }
    if constexpr (XMODE == XM_NORM) {                            // QRMSNorm.forward, decode_gemv_kernel's arithmetic
      float ss[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) ss[b] = 0.f;
#pragma unroll
      for (int u = 0; u < DG_XPRE; ++u) {
        if (u * DG_PRO * 64 < nvec) {
          const int i = p + u * DG_PRO * 64, ic = i < nvec ? i : nvec - 1;
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            if (b < B) {
              float4 v;
              if (u < DB_XH) v = xv[b][u < DB_XH ? u : 0] = fqv(xv[b][u < DB_XH ? u : 0]);
              else v = fqv(xrow(b, ic));
              if (i < nvec) {
                const v2f lo2 = (v2f){v.x, v.y}, hi2 = (v2f){v.z, v.w};
                const v2f sl = lo2 * lo2, sh = hi2 * hi2;
                ss[b] += sl.x;
                ss[b] += sl.y;
                ss[b] += sh.x;
                ss[b] += sh.y;
              }
            }
          }
        }
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b < B) {
          const float t = wave_sum_f_rowbcast(ss[b]);
          if (lane == 0) s_red[b][wave] = t;
        }
      }
      __syncthreads();                                           // barrier 1 of 2
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < DG_PRO; ++w) tot += s_red[b][w];
        const float mean = __fdiv_rn(tot, (float)K);
        r[b] = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(mean, g.eps)));
      }
    }
#pragma unroll
    for (int u = 0; u < DG_XPRE; ++u) {
      if (u * DG_PRO * 64 < nvec) {
        const int i = p + u * DG_PRO * 64, ic = i < nvec ? i : nvec - 1;
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f), bb = w;
        if constexpr (ANYNORM) w = u < DB_XH ? nw[u < DB_XH ? u : 0] : reinterpret_cast<const float4*>(g.norm_w)[ic];
        if constexpr (XMODE == XM_LNORM)
          bb = u < DB_XH ? nb[u < DB_XH ? u : 0] : (g.norm_bias ? reinterpret_cast<const float4*>(g.norm_bias)[ic] : make_float4(0.f, 0.f, 0.f, 0.f));
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if (b < B) {
            float4 v = xval(b, u, ic, ANYNORM);
            if constexpr (XMODE == XM_NORM) {
              const v2f a2 = (v2f){w.x, w.y} * ((v2f){v.x, v.y} * splat2(r[b])), b2 = (v2f){w.z, w.w} * ((v2f){v.z, v.w} * splat2(r[b]));
              v = make_float4(a2.x, a2.y, b2.x, b2.y);
            }
            if constexpr (XMODE == XM_LNORM) {
              v.x = __fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(v.x, r[b]), shiftv[b]), w.x), bb.x);
              v.y = __fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(v.y, r[b]), shiftv[b]), w.y), bb.y);
              v.z = __fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(v.z, r[b]), shiftv[b]), w.z), bb.z);
              v.w = __fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(v.w, r[b]), shiftv[b]), w.w), bb.w);
            }
            const v2f u01 = image_u8f2((v2f){v.x, v.y}, ag.s, ag.inv_s, ag.o, ag.qmin, ag.qmax, 0.f);
            const v2f u23 = image_u8f2((v2f){v.z, v.w}, ag.s, ag.inv_s, ag.o, ag.qmin, ag.qmax, 0.f);
            uint32_t usum = 0;
            const uint32_t pk = image_pack4(u01.x, u01.y, u23.x, u23.y, usum);
            if (i < nvec) {
              my_sum[b] += (int)usum - 512;
              reinterpret_cast<unsigned*>(smem + (size_t)b * K)[i] = pk;
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b < B) {
      const int part = wave_sum_dpp(my_sum[b]);
      if (lane == 0) s_redi[b][wave] = part;
    }
  }
  __syncthreads();                                               // the images and the row sums are complete
}

// the STREAM waves' side of the prologue's barriers: the norm reductions, then the one after which the images are complete
template <int XMODE>
__device__ __forceinline__ void gemv_batch_stream_barriers() {
  if constexpr (XMODE == XM_LNORM) {                               // the prologue waves' mean and variance reductions
    __syncthreads();
    __syncthreads();
  }
  if constexpr (XMODE == XM_NORM) __syncthreads();                 // barrier 1 of 2: the prologue waves' sums of squares
  __syncthreads();                                                 // the images and the row sums are complete
}

// Epilogue of one output row of one activation row, from the fp32 value(s) in front of the output grid(s): out_grid by q|k|v segment
// (+ residual), or the gate (QSiLU / QGELU, the product, w2's input quantizer written as int8).
struct GemvBatchEpilogue {
  Grid og0, og1, og2, gmid, gact, gout;
  __device__ __forceinline__ GemvBatchEpilogue(const float cv, const mq_decode_gemv_args& g)
      : og0(const_grid(cv, CG_OUT0, g.out_grid[0])), og1(const_grid(cv, CG_OUT1, g.out_grid[1])), og2(const_grid(cv, CG_OUT2, g.out_grid[2])),
        gmid(const_grid(cv, CG_GATE_MID, g.gate_mid)), gact(const_grid(cv, CG_GATE_ACTOUT, g.gate_actout)), gout(const_grid(cv, CG_GATE_OUT, g.gate_out)) {}
  // output quantizer as the GEMM / GEMV epilogues evaluate it (reciprocal multiply)
  __device__ __forceinline__ static float out_q(const Grid& q, float f) {
    if (!q.on) return f;
    float v = rintf(f * q.inv_s) + q.o;
    v = fminf(fmaxf(v, q.qmin), q.qmax);
    return __fmul_rn(__fsub_rn(v, q.o), q.s);
  }
  template <bool GATE>
  __device__ __forceinline__ void store(const mq_decode_gemv_batch_args& ba, const int b, const int row, const float e0, const float e1, const float res) const {
    const mq_decode_gemv_args& g = ba.g;
    if constexpr (GATE) {
      const float fa = out_q(og0, e0), fb = out_q(og1, e1);
      float rr;
      if (g.gate_act == 0) {                                       // QSiLU (qmodule.py:739-753)
        const float gate = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-fa)));
        rr = __fmul_rn(fa, gmid.fq(gate));
      } else {                                                     // QGELU (qmodule.py:790-798), erf form
        rr = __fmul_rn(__fmul_rn(0.5f, fa), __fadd_rn(1.0f, erff(__fmul_rn(fa, 0.70710678118654752440f))));
      }
      const float prod = __fmul_rn(gact.fq(rr), fb);
      const float qi = index_decode_keepnan(prod, gout.s, gout.inv_s, gout.o, gout.qmin, gout.qmax);
      g.gate_q[(size_t)b * ba.gate_stride + row] = (int8_t)((qi != qi ? (int)gout.qmin : (int)qi) - 128);
      if (g.y) g.y[(size_t)b * ba.y_stride + row] = prod;
    } else {
      float v = row < g.seg_end[0] ? out_q(og0, e0) : (row < g.seg_end[1] ? out_q(og1, e0) : out_q(og2, e0));
      if (g.resid) v = __fadd_rn(res, v);
      g.y[(size_t)b * ba.y_stride + row] = v;
    }
  }
};

// ---- host side of the decode GEMV launches (mq_decode.hip, mq_decode_batch.hip, mq_decode_grouped.hip) -------------------------
// rows per workgroup and grid: the NL logical rows (a gate launch's w1 | w3 pair is one) spread over the device's CUs, at most
// DG_STR * 64 per workgroup
inline int gemv_row_geometry(int NL, int* rows_per_wg, unsigned* grid) {
  fat_row_geometry(NL, DG_STR * 64, rows_per_wg, grid);
  return NL;
}

// What mq_decode_gemv, mq_decode_gemv_batch and mq_decode_gemv_grouped all require of the argument block g and its B rows at
// x_stride / y_stride / gate_stride, refused under the entry's name `who`.  `single`: mq_decode_gemv, whose rows have no strides --
// three messages keep its wording, and its int8 image is copied in 4-byte pieces.  The entry's own conditions (the per-channel or
// per-group vectors, zero_acc / o_acc, the LDS bound of B images, the group size) stay at the entry, behind these.
inline int check_gemv(const char* who, const mq_decode_gemv_args& g, const int B, const int64_t x_stride, const int64_t y_stride, const int64_t gate_stride,
                      const bool single) {
  MQ_REQUIRE(g.w && (g.x || g.xq), "%s: null pointer", who);
  MQ_REQUIRE(g.consts != nullptr && aligned(g.consts, 16),
             single ? "%s: consts (64 floats: mq_decode_pack_grids of this launch's 8 grids, zero padded) is required"
                    : "%s: consts (mq_decode_pack_grids of this launch's grids) is required, 16-byte aligned", who);
  MQ_REQUIRE(g.K > 0 && g.K % 256 == 0 && g.K <= 32768 && g.N > 0, "%s: K=%d must be a positive multiple of 256 (<= 32768), N=%d", who, g.K, g.N);
  MQ_REQUIRE(g.xq || g.K <= DG_XPRE * 4 * DG_PRO * 64,
             single ? "%s: K=%d exceeds the fp32 activation row the prologue waves hold in registers (8192)"
                    : "%s: K=%d exceeds the fp32 activation row the prologue serves (8192)", who, g.K);
  MQ_REQUIRE(g.xq || (g.a_grid.scale && g.a_grid.offset && g.a_grid.qmin == 0.f && g.a_grid.qmax == 255.f),
             "%s: fp32 activations need an 8-bit unsigned activation grid", who);
  MQ_REQUIRE(x_stride >= (B > 1 ? g.K : 0) && x_stride % 16 == 0 && aligned(g.w, 16) && (!g.x || aligned(g.x, 16)) &&
                 (!g.xq || aligned(g.xq, single ? 4 : 16)) && (!g.norm_w || aligned(g.norm_w, 16)),
             single ? "%s: pointers must be 16-byte aligned" : "%s: pointers must be 16-byte aligned and x_stride a multiple of 16 covering K", who);
  const bool gate = g.gate_q != nullptr;
  MQ_REQUIRE(gate || g.y, "%s: no output", who);
  MQ_REQUIRE(!gate || (g.norm_w && !g.xq), "%s: gate mode is served for the norm-fused prologue (fp32 x + norm_w)", who);
  MQ_REQUIRE(!gate || (g.N % 2 == 0 && g.gate_out.scale && g.out_grid[0].scale && g.out_grid[1].scale && (g.gate_act == 0 || g.gate_act == 1)),
             "%s: gate mode needs an even N (interleaved w1 / w3 rows), both output grids and the w2 input grid", who);
  const int NLr = gate ? g.N / 2 : g.N;
  MQ_REQUIRE(B == 1 || ((!g.y || y_stride >= NLr) && (!g.resid || y_stride >= NLr) && (!gate || gate_stride >= NLr)),
             "%s: y_stride / gate_stride must cover a row (%d)", who, NLr);
  MQ_REQUIRE(!g.norm_bias || (g.layernorm && aligned(g.norm_bias, 16)), "%s: norm_bias belongs to the LayerNorm prologue (layernorm = 1), 16-byte aligned", who);
  return MQ_OK;
}

constexpr int DB_MAX_IMAGE = 128 * 1024;   // B * K int8 images in LDS (the batched and the grouped launch)

inline int gemv_xmode(const mq_decode_gemv_args& g) { return g.xq ? XM_I8 : (g.norm_w ? (g.layernorm ? XM_LNORM : XM_NORM) : XM_F32); }

// (xmode, gate, w4) of a launch as compile-time constants: launch(XM, GATE, W4) is called with std::integral_constant values.  Gate
// launches exist for the two norm prologues only (check_gemv), so an entry instantiates 12 kernels per further flag of its own.
template <class Launch>
inline int gemv_dispatch(const int xmode, const bool gate, const bool w4, Launch&& launch) {
  auto with_w4 = [&](auto xm, auto gt) { return w4 ? launch(xm, gt, std::true_type{}) : launch(xm, gt, std::false_type{}); };
  if (gate) {
    if (xmode == XM_LNORM) return with_w4(std::integral_constant<int, XM_LNORM>{}, std::true_type{});
    return with_w4(std::integral_constant<int, XM_NORM>{}, std::true_type{});
  }
  switch (xmode) {
    case XM_LNORM: return with_w4(std::integral_constant<int, XM_LNORM>{}, std::false_type{});
    case XM_NORM: return with_w4(std::integral_constant<int, XM_NORM>{}, std::false_type{});
    case XM_F32: return with_w4(std::integral_constant<int, XM_F32>{}, std::false_type{});
    default: return with_w4(std::integral_constant<int, XM_I8>{}, std::false_type{});
  }
}
// index of an instantiation in an entry's set_lds cache
inline int gemv_kernel_index(const int xmode, const bool gate, const bool w4) { return (xmode * 2 + (gate ? 1 : 0)) * 2 + (w4 ? 1 : 0); }

}  // namespace mq
