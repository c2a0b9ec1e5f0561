// Device helpers shared by the single-sequence decode kernels (mq_decode.hip) and the batched ones (mq_decode_batch.hip): quantizer
// arithmetic, DPP wave reductions, the launch-constants line and the layout constants both families agree on.
#pragma once
#include "mq_common.h"

namespace mq {

#pragma clang fp contract(off)

typedef int v4i __attribute__((ext_vector_type(4)));

// torch.clamp propagates NaN; so do v_maximum3_f32 / v_minimum3_f32 (gfx950) -- two instructions where fmaxf / fminf + a NaN select
// cost five (round 5: every quantizer of the decode step sits on a launch's critical path)
__device__ __forceinline__ float dq_clamp_nan(float q, float lo, float hi) {
  return __builtin_elementwise_minimum(__builtin_elementwise_maximum(q, lo), hi);
}
// (x / s: div_by_scale of mq_common.h -- at M = 1 every CU quantises the whole activation row, and that arithmetic is on the
// launch's critical path)
// qmodule.py:286-290.  round_ste = (round(t) - t) + t IS rint(t) in fp32 for every t div_by_scale returns (finite or NaN, never inf:
// mq_common.h image_idxf has the argument) -- two instructions fewer on the M = 1 critical path
__device__ __forceinline__ float dq_index(float x, float s, float inv_s, float o, float qmin, float qmax) {
  const float t = div_by_scale(x, s, inv_s);
  return dq_clamp_nan(__fadd_rn(rintf(t), o), qmin, qmax);
}
__device__ __forceinline__ float dq_dequant(float q, float s, float o) { return __fmul_rn(__fsub_rn(q, o), s); }

struct Grid {          // device view of mq_grid
  float s, o, qmin, qmax, inv_s;
  bool on;
  __device__ __forceinline__ float fq(float v) const { return on ? dq_dequant(dq_index(v, s, inv_s, o, qmin, qmax), s, o) : v; }
  // two elements per instruction where a packed form exists (v_pk_mul / v_pk_fma / v_pk_add are IEEE fp32 on register pairs: the same
  // bits as fq on each half; rint and the clamp stay scalar).  q - o == q + (-o) exactly.
  __device__ __forceinline__ v2f fq2(v2f v) const {
    if (!on) return v;
    const v2f t = div_by_scale2(v, s, inv_s);
    v2f r = {rintf(t.x), rintf(t.y)};
    r = r + splat2(o);
    r.x = dq_clamp_nan(r.x, qmin, qmax);
    r.y = dq_clamp_nan(r.y, qmin, qmax);
    return (r + splat2(-o)) * splat2(s);
  }
};
__device__ __forceinline__ Grid load_grid(const mq_grid& g) {
  Grid r;
  r.on = g.scale != nullptr;
  r.s = r.on ? g.scale[0] : 1.f;
  r.o = r.on ? g.offset[0] : 0.f;
  r.qmin = g.qmin;
  r.qmax = g.qmax;
  r.inv_s = __fdiv_rn(1.0f, r.s);
  return r;
}

__device__ __forceinline__ int dot16(const v4i a, const v4i b, int c) {
#pragma unroll
  for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_sdot4(a[e], b[e], c, false);
  return c;
}
__device__ __forceinline__ int wave_sum_dpp(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return __builtin_amdgcn_readlane(v, 63);
}
// float wave reductions on DPP moves (a __shfl_xor is an LDS round trip of ~100 cycles; six of them in a row cost ~0.25 us of
// a kernel that lasts 3): same lane pattern as wave_sum_dpp; the result is the value of lane 63, broadcast
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, BOUND));
}
__device__ __forceinline__ float wave_sum_f(float v) {
  v += dpp_f<0xB1, 0xf, true>(v);
  v += dpp_f<0x4E, 0xf, true>(v);
  v += dpp_f<0x141, 0xf, true>(v);
  v += dpp_f<0x140, 0xf, true>(v);
  v += dpp_f<0x142, 0xa, false>(v);                                 // row_bcast15 into rows 1 and 3 (0 elsewhere: x + 0 = x)
  v += dpp_f<0x143, 0xc, false>(v);                                 // row_bcast31 into rows 2 and 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float wave_max_f(float v) {              // inputs are finite or -inf, never NaN
  v = fmaxf(v, dpp_f<0xB1, 0xf, true>(v));
  v = fmaxf(v, dpp_f<0x4E, 0xf, true>(v));
  v = fmaxf(v, dpp_f<0x141, 0xf, true>(v));
  v = fmaxf(v, dpp_f<0x140, 0xf, true>(v));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 15));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 31));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 47));
  const float r4 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
  return fmaxf(fmaxf(r1, r2), fmaxf(r3, r4));
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

}  // namespace mq
