// Shared helpers for the libmobilequant_amd translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <atomic>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "mobilequant_amd.h"

namespace mq {

// Thread-local error text behind mq_last_error(); defined in mq_quantize.hip.
void set_error(const char* fmt, ...);

inline hipStream_t as_stream(mq_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// The library may be driven on several devices of one process (a caller that switches devices, one model per GPU in one
// process): everything cached per kernel or per launch configuration is cached PER DEVICE.
constexpr int kMaxDevices = 64;
inline int current_device() {
  int d = 0;
  return (hipGetDevice(&d) == hipSuccess && d >= 0 && d < kMaxDevices) ? d : 0;
}
// once-per-device flag set (one bit per device; setting an attribute twice in a race is harmless)
struct PerDeviceOnce {
  std::atomic<unsigned long long> mask{0};
  bool done(int dev) const { return (mask.load(std::memory_order_acquire) >> dev) & 1ull; }
  void mark(int dev) { mask.fetch_or(1ull << dev, std::memory_order_release); }
};

#define MQ_REQUIRE(cond, ...)      \
  do {                             \
    if (!(cond)) {                 \
      mq::set_error(__VA_ARGS__);  \
      return MQ_EINVAL;            \
    }                              \
  } while (0)

#define MQ_LAUNCH_CHECK(name)                                                        \
  do {                                                                               \
    hipError_t e__ = hipGetLastError();                                              \
    if (e__ != hipSuccess) {                                                         \
      mq::set_error("%s: kernel launch failed: %s", name, hipGetErrorString(e__));   \
      return MQ_EHIP;                                                                \
    }                                                                                \
  } while (0)

// CU count of the current device, read once per device (256 where the property cannot be read)
inline int device_cus() {
  static std::atomic<int> cus_of[kMaxDevices];      // 0 = not read yet
  const int dev = current_device();
  int cus = cus_of[dev].load(std::memory_order_relaxed);
  if (!cus) {
    hipDeviceProp_t prop;
    cus = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    cus_of[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}
// Launch geometry of the weight-streaming GEMVs, one fat workgroup per CU: `rows` spread over the device's CUs, at most max_rows_per_wg
// per workgroup (16 waves x 64 row slots, whose per-row parameters live one per lane; the W4A8 decode kernels stream with 8 waves).
inline void fat_row_geometry(int rows, int max_rows_per_wg, int* rows_per_wg, unsigned* grid) {
  const int cus = device_cus();
  int rpw = (rows + cus - 1) / cus;
  if (rpw > max_rows_per_wg) rpw = max_rows_per_wg;
  *rows_per_wg = rpw;
  *grid = (unsigned)((rows + rpw - 1) / rpw);
}

// Raise a kernel's dynamic-LDS ceiling once per device, when a launch needs `lds` bytes above the 32 KiB every kernel may use as it
// is.  The ceiling asked for is `lds` itself (the kernel is opted in size by size) or, where given, `ceiling`, the kernel's maximum:
// one call then serves every later launch, so a larger launch inside a graph capture needs no attribute call.  cache: a slot per device.
inline int set_lds(const void* fn, std::atomic<size_t>* cache, size_t lds, const char* name, size_t ceiling = 0) {
  const int dev = current_device();
  if (!ceiling) ceiling = lds;
  if (lds > 32768 && cache[dev].load(std::memory_order_relaxed) < lds) {
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ceiling) != hipSuccess) {
      set_error("%s: %zu bytes of dynamic LDS rejected", name, ceiling);
      return MQ_EHIP;
    }
    cache[dev].store(ceiling, std::memory_order_relaxed);
  }
  return MQ_OK;
}

// x / s through the correctly rounded reciprocal inv_s = RN(1 / s) and one fma correction (Markstein): bit-identical to the IEEE
// divide for |x / s| in [2^-2, 1e30] -- tools/div_check.cpp compares every fp32 dividend for 48 divisors on the GPU, incl. all-ones
// significands and the scale clamps 1e-5 / 1e6 (profiles/r03/div_check.log) -- and faithful below 2^-2, where round(x / s) = 0 and
// round_ste's (round(t) - t) + t = 0 whatever the last bit of t is: a quantizer INDEX (qmodule.py:286-287) can not tell the two
// apart.  +-inf and NaN dividends give NaN, which is what the reference's round_ste makes of them.  3 VALU instructions instead of
// the ~10 + two mode switches of v_div_scale / v_rcp / v_fma x4 / v_div_fmas / v_div_fixup: the quantize / norm kernels spend
// most of their issue slots on this division.  NOT for quotients that are themselves results (x / chan_scale, gradients).
__device__ __forceinline__ float div_by_scale(float x, float s, float inv_s) {
  const float q0 = __fmul_rn(x, inv_s);
  return __builtin_fmaf(__builtin_fmaf(-q0, s, x), inv_s, q0);
}
// The fast form needs a NORMAL reciprocal and no over / underflow in its intermediates.  tools/div_check.cpp sweeps every dividend for
// divisors drawn over +-[2^-60, 2^60] (profiles/r04/div_check.log): inside that range it is the IEEE quotient on the quantizer's
// domain; outside (a scale of 0, a denormal, inf, NaN, |s| beyond 2^+-60 -- nothing set_scale_offset_from_minmax's [1e-5, 1e6] clamp
// (qmodule.py:58) produces, but a trained scale parameter or a C-ABI caller is not bound by it) the reciprocal is inf / denormal and
// the fast form returns NaN where x / s is +-inf or finite.  The PUBLIC element-wise entry points (mq_fake_quant / mq_quantize and the
// per-row weight grids of training: HBM-bound kernels, the select is free) therefore take the IEEE divide for such a scale
// (div_by_scale_guarded, a per-tensor / per-row uniform choice).  The fused image kernels (norm, GEMV, decode, attention, tiled
// quantize) are reached through static calibrated grids only and keep the unguarded form: with a scale outside the range their
// indices saturate to qmin (NaN -> qmin) where the reference saturates to qmin or qmax -- a degenerate grid either way
// (dequantised values are (q - o) * s with s = 0 / inf / NaN).
__device__ __forceinline__ bool scale_in_fast_range(float s) {
  const float a = __builtin_fabsf(s);
  return a >= 0x1p-60f && a <= 0x1p60f;          // false for NaN
}
__device__ __forceinline__ float div_by_scale_guarded(float x, float s, float inv_s, bool fast) {
  return fast ? div_by_scale(x, s, inv_s) : __fdiv_rn(x, s);
}

// Two elements per instruction: v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32 are IEEE fp32 operations on register pairs (full rate on
// CDNA3 / 4), so the packed forms return the bits of the scalar ones; rint, med3 and the u8 conversion have no packed form.
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f splat2(float v) { return (v2f)(v); }
__device__ __forceinline__ v2f div_by_scale2(v2f x, float s, float inv_s) {
  const v2f q0 = x * splat2(inv_s);
  return __builtin_elementwise_fma(__builtin_elementwise_fma(-q0, splat2(s), x), splat2(inv_s), q0);
}

// 64-lane wave reductions on DPP moves (wave = 64 on gfx950): quad permutes, row_half_mirror, row_mirror leave every lane of a
// 16-lane row with the row's result; the four rows meet through v_readlane.  A __shfl_xor is a ds_bpermute -- an LDS round trip
// of ~100 cycles -- and six dependent ones cost a short kernel more than its arithmetic (decode: 0.25 us of a 3 us launch).  The
// result is wave-uniform.  (Float sums: another association than the xor butterfly -- every caller's tolerance covers the order
// of a row reduction; min / max are exact either way.)
template <int CTRL>
__device__ __forceinline__ int dpp_mov_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ __forceinline__ float dpp_mov_f(float v) { return __builtin_bit_cast(float, dpp_mov_i<CTRL>(__builtin_bit_cast(int, v))); }
__device__ __forceinline__ float readlane_f(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
template <class Op>
__device__ __forceinline__ float wave_reduce_f(float v, Op op) {
  v = op(v, dpp_mov_f<0xB1>(v));                                    // quad_perm [1,0,3,2]
  v = op(v, dpp_mov_f<0x4E>(v));                                    // quad_perm [2,3,0,1]
  v = op(v, dpp_mov_f<0x141>(v));                                   // row_half_mirror
  v = op(v, dpp_mov_f<0x140>(v));                                   // row_mirror
  return op(op(readlane_f(v, 15), readlane_f(v, 31)), op(readlane_f(v, 47), readlane_f(v, 63)));
}
__device__ __forceinline__ float wave_min(float v) {
  return wave_reduce_f(v, [](float a, float b) { return fminf(a, b); });
}
__device__ __forceinline__ float wave_max(float v) {
  return wave_reduce_f(v, [](float a, float b) { return fmaxf(a, b); });
}
// The two float wave sums run the same four steps inside a 16-lane row and differ in how the four row totals r0 .. r3 meet.  They are
// kept apart so that no kernel's instruction stream or summation order changes by accident.
// rows met through v_readlane: (r0 + r1) + (r2 + r3).  The prefill kernels (norms, fake-quant backward, training softmax, reductions).
__device__ __forceinline__ float wave_sum_f_readlane(float v) {
  return wave_reduce_f(v, [](float a, float b) { return a + b; });
}
__device__ __forceinline__ int wave_sum(int v) {
  v += dpp_mov_i<0xB1>(v);
  v += dpp_mov_i<0x4E>(v);
  v += dpp_mov_i<0x141>(v);
  v += dpp_mov_i<0x140>(v);
  return (__builtin_amdgcn_readlane(v, 15) + __builtin_amdgcn_readlane(v, 31)) + (__builtin_amdgcn_readlane(v, 47) + __builtin_amdgcn_readlane(v, 63));
}
// The decode kernels' forms (six DPP adds, the result read from lane 63): rows met through row broadcasts.
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, BOUND));
}
__device__ __forceinline__ int wave_sum_dpp(int v) {               // all lanes active
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);    // quad_perm [1,0,3,2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);    // quad_perm [2,3,0,1]
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);   // row_half_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);   // row_mirror: every lane = its row-of-16 total
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
  return __builtin_amdgcn_readlane(v, 63);
}
// rows met through row broadcasts: (r3 + r2) + (r1 + r0), the value of lane 63
__device__ __forceinline__ float wave_sum_f_rowbcast(float v) {
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

// Sum of the four waves' (wave-uniform) values of a 256-thread group, for every thread: wave `wave` leaves v in slots[wave], one
// barrier, (0 + 1) + (2 + 3).  Float or int.  The slots may be rewritten after the next barrier.
template <typename T>
__device__ __forceinline__ T block_sum4(T v, T* slots, int wave) {
  if ((threadIdx.x & 63) == 0) slots[wave] = v;
  __syncthreads();
  return (slots[0] + slots[1]) + (slots[2] + slots[3]);
}

// Sum or maximum over ALL lanes of a WAVES-wave workgroup (4 or 16), for every thread, in a fixed order: the wave's own reduction, then
// the wave totals through red[WAVES] met as ((0 + 1) + (2 + 3)) per four waves and the fours likewise.  Two barriers: the first because
// the slots may still be read from the previous reduction.
struct BlockSum {
  static __device__ __forceinline__ float wave(float v) { return wave_sum_f_rowbcast(v); }
  static __device__ __forceinline__ float two(float a, float b) { return a + b; }
};
struct BlockMax {                                                   // inputs are finite or -inf, never NaN
  static __device__ __forceinline__ float wave(float v) { return wave_max_f(v); }
  static __device__ __forceinline__ float two(float a, float b) { return fmaxf(a, b); }
};
template <int WAVES, class Op>
__device__ __forceinline__ float block_reduce(float v, float* red, int wave, int lane) {
  static_assert(WAVES == 4 || WAVES == 16, "four waves, or four fours");
  v = Op::wave(v);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float t[WAVES / 4];
#pragma unroll
  for (int i = 0; i < WAVES / 4; ++i) t[i] = Op::two(Op::two(red[4 * i], red[4 * i + 1]), Op::two(red[4 * i + 2], red[4 * i + 3]));
  if constexpr (WAVES == 4) return t[0];
  else return Op::two(Op::two(t[0], t[1]), Op::two(t[2], t[3]));
}

// Exact float atomic min/max on the IEEE bit pattern (no CAS loop): non-negative floats order as
// signed ints, negative floats order reversed as unsigned ints.
__device__ __forceinline__ void atomic_max_f32(float* addr, float v) {
  if (v >= 0.0f) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
  else atomicMin(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_min_f32(float* addr, float v) {
  if (v >= 0.0f) atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
  else atomicMax(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}

// The (value, index) sort key of the selection kernels (mq_sample.hip, mq_logprob.hip, mq_beam.hip), for a value that is no NaN and an
// index below 2^20: (monotone u32 of z) << 20 | (2^20 - 1 - i).  Keys are distinct and never 0, and their descending order is value
// descending, ties by index ascending.
constexpr unsigned long long SORT_KEY_IDX_MASK = (1ull << 20) - 1;
__device__ __forceinline__ unsigned long long sort_key(float z, int i) {
  const unsigned u = __float_as_uint(z);
  const unsigned k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)k << 20) | (SORT_KEY_IDX_MASK - (unsigned long long)i);
}
__device__ __forceinline__ int sort_key_id(unsigned long long key) { return (int)(SORT_KEY_IDX_MASK - (key & SORT_KEY_IDX_MASK)); }
__device__ __forceinline__ float sort_key_value(unsigned long long key) {
  const unsigned k = (unsigned)(key >> 20);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// Byte offset of element (row, k) in the fragment-blocked ("tiled") int8 image of a [rows, cols] activation -- the layout
// include/mobilequant_amd.h describes at mq_quantize_tiled: 1-KiB blocks of 16 rows x 64 k ordered [row block][k block]; inside a block
// lane (row & 15) + 16 * ((k >> 4) & 3) owns the 16 bytes k & 15.
__device__ __forceinline__ int64_t tiled_block_base(int64_t row_block, int64_t k_block, int64_t cols) { return (row_block * (cols >> 6) + k_block) << 10; }
__device__ __forceinline__ int64_t tiled_image_offset(int64_t row, int64_t k, int64_t cols) {
  return tiled_block_base(row >> 4, k >> 6, cols) + ((((int)row & 15) + 16 * (((int)k >> 4) & 3)) << 4) + ((int)k & 15);
}
// Copy-out of the staged tiled kernels (norm_tiled8_kernel, quantize_tiled8_kernel): the LDS tile holds RW rows (row0 .. row0 + RW - 1,
// inside one row block) as 16-byte units p = RW * piece + r, piece = k >> 4; unit p goes to block (row0 >> 4, piece >> 2), byte
// 256 (piece & 3) + 16 ((row0 & 15) + r) -- RW x 16 B contiguous per piece: whole cache lines of a fragment block.  PAD: the rows
// past `rows` (padding of the image's last row block) are written like the others; otherwise they stay untouched.
// POLICY: cache policy of the image stores.  STORE_DEFAULT keeps the written lines in the XCD's L2 like any store (today's statement,
// word for word: norm_tiled8_kernel compiles to the code it always had); STORE_NT marks them streaming.
enum StorePolicy { STORE_DEFAULT = 0, STORE_NT = 1 };
template <int RW, int THREADS, bool PAD, int POLICY = STORE_DEFAULT>
__device__ __forceinline__ void staged_copy_out(const int8_t* stage, int8_t* q_tiled, int64_t row0, int64_t rows, int64_t cols) {
  typedef uint32_t v4u __attribute__((ext_vector_type(4)));
  const int units = (int)(cols >> 4) * RW;
  const int64_t rb = row0 >> 4;
  const int half = (int)(row0 & 15);
  for (int p = threadIdx.x; p < units; p += THREADS) {
    const int piece = p / RW, r = p % RW;
    if (PAD || row0 + r < rows) {
      if constexpr (POLICY == STORE_DEFAULT) {
        *reinterpret_cast<uint4*>(q_tiled + tiled_block_base(rb, piece >> 2, cols) + ((piece & 3) << 8) + ((half + r) << 4)) =
            *reinterpret_cast<const uint4*>(stage + (p << 4));
      } else {
        int8_t* dst = q_tiled + tiled_block_base(rb, piece >> 2, cols) + ((piece & 3) << 8) + ((half + r) << 4);
        const v4u v = *reinterpret_cast<const v4u*>(stage + (p << 4));
        __builtin_nontemporal_store(v, reinterpret_cast<v4u*>(dst));
      }
    }
  }
}

// ---- 16 bytes of fp32 / fp16 elements per lane (the element-wise kernels of mq_fake_quant.hip and mq_quantize.hip) ---------------
template <typename T>
struct Vec16;
template <>
struct Vec16<float> {
  static constexpr int N = 4;
  float v[4];
  __device__ static float get(const Vec16& a, int i) { return a.v[i]; }
  __device__ static void set(Vec16& a, int i, float f) { a.v[i] = f; }
};
template <>
struct Vec16<__half> {
  static constexpr int N = 8;
  __half v[8];
  __device__ static float get(const Vec16& a, int i) { return __half2float(a.v[i]); }
  __device__ static void set(Vec16& a, int i, float f) { a.v[i] = __float2half_rn(f); }
};

template <typename T>
__device__ __forceinline__ float ld(const T* p, int64_t i);
template <>
__device__ __forceinline__ float ld<float>(const float* p, int64_t i) { return p[i]; }
template <>
__device__ __forceinline__ float ld<__half>(const __half* p, int64_t i) { return __half2float(p[i]); }
template <typename T>
__device__ __forceinline__ void st(T* p, int64_t i, float v);
template <>
__device__ __forceinline__ void st<float>(float* p, int64_t i, float v) { p[i] = v; }
template <>
__device__ __forceinline__ void st<__half>(__half* p, int64_t i, float v) { p[i] = __float2half_rn(v); }

}  // namespace mq

#include "mq_quant.h"
