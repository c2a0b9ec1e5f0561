// What mq_w4a16.hip (mq_w4a16_linear) and mq_w4a16_decode.hip (the decode engine's weight streams) share of the W4A16 contract
// (DESIGN.md 4.9): the packed-fp16 dequantize of one dword of the mq_pack_w4 image, the fp16 packing of the activations and the
// "unit order" in which both kernels lay the activations out in LDS.  Inline device functions only: each file keeps its own kernels.
#pragma once
#include "mq_common.h"

namespace mq {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));

#pragma clang fp contract(off)

__device__ __forceinline__ unsigned pack_h2(float a, float b) {
  return (unsigned)__half_as_ushort(__float2half_rn(a)) | ((unsigned)__half_as_ushort(__float2half_rn(b)) << 16);
}

// eight dequantized weights of packed dword d, unit order; sz = (s16, s16), nz = -(1024 + z') twice
__device__ __forceinline__ void dequant8(unsigned d, h2 sz, h2 nz, h2 (&w)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const unsigned p = ((d >> (4 * t)) & 0x000f000fu) | 0x64006400u;
    w[t] = (__builtin_bit_cast(h2, p) + nz) * sz;
  }
}
__device__ __forceinline__ h2 splat_scale(uint16_t s) { return __builtin_bit_cast(h2, (unsigned)s | ((unsigned)s << 16)); }
__device__ __forceinline__ h2 splat_negzero(uint16_t z) {
  const _Float16 zf = __builtin_bit_cast(_Float16, z);
  const _Float16 v = -((_Float16)1024.0f + zf);              // exact: |z'| <= 1024, an integer
  return h2{v, v};
}

// byte offset inside a 16-byte unit of the (j0, j2) dword of the quad that is half h (k bit 4) of its 32-block; (j1, j3) sits 8 further
__device__ __forceinline__ int quad_slot(int h) { return 4 * h; }

// rotation of the four 16-byte units of chunk c in the GEMV's LDS image: 16 neighbouring lanes' ds_read_b128 cover all 64 banks
__device__ __forceinline__ int unit_rot(int c) { return (c + (c >> 2)) & 3; }

// where the fp16 quad x[kk .. kk + 3] (kk % 4 == 0) of a row sits in the GEMV's LDS image of that row: its (j0, j2) dword; (j1, j3) 8 further
__device__ __forceinline__ int gemv_quad_offset(int kk) {
  const int c = kk >> 5, unit = (((kk & 15) >> 2) + unit_rot(c)) & 3;
  return c * 64 + unit * 16 + quad_slot((kk >> 4) & 1);
}

}  // namespace mq
