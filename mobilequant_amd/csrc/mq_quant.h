// Quantizer arithmetic of the libmobilequant_amd kernels, each form once (included at the end of mq_common.h).
//
// The reference's quantizer (qmodule.py:286-290) is  index = clamp(round_ste(x / s) + o, qmin, qmax),  value = (index - o) * s.
// The kernels evaluate the index in FOUR forms.  They agree bit for bit on every finite quotient (round_ste(t) = (rint(t) - t) + t IS
// rint(t) in fp32: |t| >= 0.5 -- rint(t) and t are within a factor of two, the difference is exact and adding t back lands on the
// representable rint(t); |t| < 0.5 -- (0 - t) + t = 0) and differ in what a NaN becomes and in what the clamp costs.  Which form a
// kernel uses is a numerical decision: the name says it.
#pragma once

namespace mq {

#pragma clang fp contract(off)

// round_ste (qmodule.py:17-21) is (round(t) - t) + t: exact for finite t, NaN for t = +-inf (inf - inf)
__device__ __forceinline__ float round_ste(float t) { return __fadd_rn(__fsub_rn(rintf(t), t), t); }
// torch.clamp propagates NaN (v_min / v_max drop it): the float-valued kernels follow the reference there
__device__ __forceinline__ float clamp_nan(float q, float lo, float hi) {
  const float c = fminf(fmaxf(q, lo), hi);
  return q != q ? q : c;
}
// the same result from v_maximum3_f32 / v_minimum3_f32 (gfx950), which propagate NaN themselves -- two instructions where fmaxf / fminf
// + a NaN select cost five (every quantizer of the decode step sits on a launch's critical path)
__device__ __forceinline__ float clamp_nan_minmax(float q, float lo, float hi) {
  return __builtin_elementwise_minimum(__builtin_elementwise_maximum(q, lo), hi);
}

// VALUE form, NaN stays NaN: round_ste spelled out and the NaN-propagating select.  Every kernel whose result is a float VALUE of the
// prefill path: fake-quant and LWC (mq_fake_quant.hip), the norms (mq_norm.hip), the activation / gate chain (mq_activation.hip).
// `fast` = false takes the IEEE divide (mq_common.h div_by_scale_guarded): only the public element-wise entry points pass it.
__device__ __forceinline__ float index_value_keepnan(float x, float s, float inv_s, float o, float qmin, float qmax, bool fast = true) {
  return clamp_nan(__fadd_rn(round_ste(div_by_scale_guarded(x, s, inv_s, fast)), o), qmin, qmax);
}
// STORAGE form, NaN -> qmin (integer storage has no NaN): rint and fminf / fmaxf, which drop a NaN operand.  The row-major and the
// lane-per-fragment quantizers (mq_quantize.hip) and the GEMV's fused activation quantize (mq_gemv.hip).
__device__ __forceinline__ float index_storage_nan2qmin(float x, float s, float inv_s, float o, float qmin, float qmax, bool fast = true) {
  return fminf(fmaxf(__fadd_rn(rintf(div_by_scale_guarded(x, s, inv_s, fast)), o), qmin), qmax);
}
// DECODE form, NaN stays NaN: rint (div_by_scale returns a finite quotient or NaN, never inf, so rint IS round_ste) and the
// minimum / maximum clamp.  The decode engines (mq_decode*.hip, mq_decode_attention.h), through Grid::fq / fq2 as well.
__device__ __forceinline__ float index_decode_keepnan(float x, float s, float inv_s, float o, float qmin, float qmax) {
  return clamp_nan_minmax(__fadd_rn(rintf(div_by_scale(x, s, inv_s)), o), qmin, qmax);
}
// IMAGE form, NaN -> qmin: rint and ONE v_med3_f32, which returns min3 when an operand is a (quiet) NaN.  The image-only kernels:
// the staged tiled norm and quantizer, the decode prologues (through image_u8f2 below), prefill attention's prep (mq_attention.hip).
__device__ __forceinline__ float index_image_nan2qmin(float x, float s, float inv_s, float o, float qmin, float qmax) {
  return __builtin_amdgcn_fmed3f(__fadd_rn(rintf(div_by_scale(x, s, inv_s)), o), qmin, qmax);
}
// qmodule.py:290
__device__ __forceinline__ float dequant(float q, float s, float o) { return __fmul_rn(__fsub_rn(q, o), s); }
// an index of a keepnan form -> integer storage (index - shift): NaN saturates to the grid's low end, as the STORAGE form does
__device__ __forceinline__ int to_storage_nan2qmin(float qi, float qmin, int shift) { return (qi != qi ? (int)qmin : (int)qi) - shift; }

// Four activations -> the dword of their int8 image bytes (index - shift), for the image-only kernels.  u = index + (128 - shift) lies
// in [0, 255] (the host checks that index - shift fits int8), so v_cvt_pk_u8_f32 converts AND packs in one instruction; the int8 bytes
// are u ^ 0x80 and sum(index - shift) = sum(u) - 128 n with sum(u) from one v_sad_u8 per dword (`usum` accumulates it).  ~8.5 VALU
// instructions per element instead of ~16.
__device__ __forceinline__ float image_u8f(float x, float s, float inv_s, float o, float qmin, float qmax, float bias) {
  return __fadd_rn(index_image_nan2qmin(x, s, inv_s, o, qmin, qmax), bias);
}
// two elements per instruction (mq_common.h div_by_scale2): the bits of the scalar form; rint, med3 and the u8 conversion have no packed form
__device__ __forceinline__ v2f image_u8f2(v2f x, float s, float inv_s, float o, float qmin, float qmax, float bias) {
  const v2f t = div_by_scale2(x, s, inv_s);
  v2f r = {rintf(t.x), rintf(t.y)};
  r = r + splat2(o);
  r.x = __builtin_amdgcn_fmed3f(r.x, qmin, qmax);
  r.y = __builtin_amdgcn_fmed3f(r.y, qmin, qmax);
  return r + splat2(bias);
}
__device__ __forceinline__ uint32_t image_pack4(float u0, float u1, float u2, float u3, uint32_t& usum) {
  uint32_t pk = __builtin_amdgcn_cvt_pk_u8_f32(u0, 0u, 0u);
  pk = __builtin_amdgcn_cvt_pk_u8_f32(u1, 1u, pk);
  pk = __builtin_amdgcn_cvt_pk_u8_f32(u2, 2u, pk);
  pk = __builtin_amdgcn_cvt_pk_u8_f32(u3, 3u, pk);
  usum = __builtin_amdgcn_sad_u8(pk, 0u, usum);
  return pk ^ 0x80808080u;
}

struct Grid {          // device view of a per-tensor grid (mq_grid, or a scale / offset pointer pair with its limits); off = identity
  float s, o, qmin, qmax, inv_s;
  bool on;
  // fake-quant of one value, VALUE form (the prefill norm and activation kernels)
  __device__ __forceinline__ float fq_value(float v) const { return on ? dequant(index_value_keepnan(v, s, inv_s, o, qmin, qmax), s, o) : v; }
  // fake-quant of one value, DECODE form
  __device__ __forceinline__ float fq(float v) const { return on ? dequant(index_decode_keepnan(v, s, inv_s, o, qmin, qmax), s, o) : v; }
  // two elements per instruction where a packed form exists (v_pk_mul / v_pk_fma / v_pk_add are IEEE fp32 on register pairs: the same
  // bits as fq on each half; rint and the clamp stay scalar).  q - o == q + (-o) exactly.
  __device__ __forceinline__ v2f fq2(v2f v) const {
    if (!on) return v;
    const v2f t = div_by_scale2(v, s, inv_s);
    v2f r = {rintf(t.x), rintf(t.y)};
    r = r + splat2(o);
    r.x = clamp_nan_minmax(r.x, qmin, qmax);
    r.y = clamp_nan_minmax(r.y, qmin, qmax);
    return (r + splat2(-o)) * splat2(s);
  }
};
__device__ __forceinline__ Grid load_grid(const float* scale, const float* offset, float qmin, float qmax) {
  Grid r;
  r.on = scale != nullptr;
  r.s = r.on ? scale[0] : 1.f;
  r.o = r.on ? offset[0] : 0.f;
  r.qmin = qmin;
  r.qmax = qmax;
  r.inv_s = __fdiv_rn(1.0f, r.s);
  return r;
}
__device__ __forceinline__ Grid load_grid(const mq_grid& g) { return load_grid(g.scale, g.offset, g.qmin, g.qmax); }

}  // namespace mq
