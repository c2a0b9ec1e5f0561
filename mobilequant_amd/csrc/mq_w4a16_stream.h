// The W4A16 device contract, once: the packed image and its group lookup, the packed-fp16 dequantize of one dword of the
// mq_pack_w4 image, the fp16 packing of the activations, the "unit order" in which the kernels lay the activations out in LDS, and the
// weight-stream walk of the M <= 8 GEMVs -- w4a16_gemv_kernel<MT> (mq_w4a16.hip, mq_w4a16_linear) and w4a16_decode_gemv_kernel<GATED>
// (mq_w4a16_decode.hip, the decode engine's launches) are one w4_stream_walk each, between a staging lambda and a row-completion lambda.
//
// The walk.  One 1024-thread workgroup per CU; a wave owns whole output rows, one per ROW SLOT t (which row that is, is the kernel's
// slot map), its lanes split K into 16-byte chunks (32 k; lane l takes chunks l, l + 64, ...: CHUNK SLOT j of cpl per row).  An issue
// pass requests the next INFLIGHT (row slot, chunk slot) pairs in walk order -- the 16-byte chunk with its group's s16 / z' -- all before
// the first wait; chunks past the row's end or past the last slot are zero with a zero scale.  The first pass goes out before the
// kernel stages its activations.  A pass is consumed by dequant8 and fp32 fma against the row images in LDS ([M][K] fp16, unit order; the
// four 16-byte units of a chunk are rotated by unit_rot so that 16 neighbouring lanes' ds_read_b128 cover all 64 banks); when a row
// slot's last chunk slot is done, a DPP wave sum per activation row and the kernel's row completion; then the next pass is issued.
#pragma once
#include <type_traits>
#include "mq_common.h"

namespace mq {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));

#pragma clang fp contract(off)

// The packed image of an [N, K] weight: mq_pack_w4 bytes [N, K / 2], fp16 scales and zeros [N, K / group_size].
struct W4Image {
  int N, K, gs;
  int lg_gs32;                    // group_size / 32 is a power of two: its log2, else -1 (a division per chunk)
  const uint8_t* w;
  const uint16_t* scales;
  const uint16_t* zeros;
  // group of the 32-wide k block kb
  __device__ __forceinline__ int group_of(int kb) const { return lg_gs32 >= 0 ? kb >> lg_gs32 : kb / (gs >> 5); }
};
inline W4Image w4_image(const uint8_t* w_packed, const void* scales, const void* zeros, int64_t N, int64_t K, int64_t group_size) {
  W4Image g;
  g.N = (int)N;
  g.K = (int)K;
  g.gs = (int)group_size;
  const int g32 = g.gs >> 5;
  g.lg_gs32 = (g32 & (g32 - 1)) == 0 ? __builtin_ctz(g32) : -1;
  g.w = w_packed;
  g.scales = static_cast<const uint16_t*>(scales);
  g.zeros = static_cast<const uint16_t*>(zeros);
  return g;
}

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
// the staging store of that quad into the row image `row`
__device__ __forceinline__ void stage_quad(char* row, int kk, const float (&v)[4]) {
  char* dst = row + gemv_quad_offset(kk);
  *reinterpret_cast<unsigned*>(dst) = pack_h2(v[0], v[2]);
  *reinterpret_cast<unsigned*>(dst + 8) = pack_h2(v[1], v[3]);
}

// The walk of one wave over its nslots row slots (wave-uniform), for the whole workgroup: issue the first pass, stage(), consume.
//   SZ_DWORDS  how a chunk's s16 and z' are fetched.  false -- two 16-bit loads packed into one register (s16 | z' << 16): scales and
//              zeros need 2-byte alignment only (mq_w4a16_linear's contract), and hipcc waits for each chunk in front of the next
//              request.  true -- the whole dwords that hold them (4-byte aligned, N G even: mq_w4a16_decode_gemv's contract), the half
//              picked at use: the INFLIGHT requests of a pass stay in flight together.
//   slot_row   int(int t): the weight row of this wave's row slot t < nslots.
//   stage      void(): what the kernel does behind the first requests -- per-row parameters, the M <= MT row images into smem (2 K
//              bytes each), and the barrier after which they are complete.  Every wave calls it, also one with no row slot: it
//              must not return before its barrier.
//   row_done   void(int t, const float (&sums)[MT]): row slot t is complete; sums[m] (wave-uniform) is its fp32 dot product with
//              activation row m, 0 for m >= M.
// (Why a function over lambdas and not an object with issue() / run() members: DESIGN.md 4.11.)
template <int INFLIGHT, bool SZ_DWORDS, int MT, class SlotRow, class Stage, class RowDone>
__device__ __forceinline__ void w4_stream_walk(const W4Image& g, const int nslots, SlotRow slot_row, Stage stage, const char* smem, const int M,
                                               RowDone row_done) {
  const int lane = threadIdx.x & 63;
  const int K = g.K;
  const int kchunks = K >> 5;
  const int wrow = K >> 1;
  const int G = K / g.gs;
  const int cpl = (kchunks + 63) >> 6;
  v4i buf[INFLIGHT];
  typename std::conditional<SZ_DWORDS, v2u, unsigned>::type bsz[INFLIGHT];     // (scale dword, zero dword), or s16 | z' << 16
  auto issue = [&](int t, int j) {
#pragma unroll
    for (int u = 0; u < INFLIGHT; ++u) {
      const int row = slot_row(t);
      const int c = lane + 64 * j;
      if (t < nslots && c < kchunks) {
        buf[u] = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(g.w + (size_t)row * wrow) + c);
        const size_t gi = (size_t)row * G + g.group_of(c);
        if constexpr (SZ_DWORDS) {
          bsz[u] = v2u{reinterpret_cast<const unsigned*>(g.scales)[gi >> 1], reinterpret_cast<const unsigned*>(g.zeros)[gi >> 1]};
        } else {
          bsz[u] = (unsigned)g.scales[gi] | ((unsigned)g.zeros[gi] << 16);
        }
      } else {
        buf[u] = v4i{0, 0, 0, 0};
        if constexpr (SZ_DWORDS) bsz[u] = v2u{0, 0};
        else bsz[u] = 0;
      }
      if (++j == cpl) { j = 0; ++t; }
    }
  };
  issue(0, 0);
  stage();

  float acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = 0.f;
  int t = 0, j = 0;
  while (t < nslots) {
    int t2 = t, j2 = j;
#pragma unroll
    for (int u = 0; u < INFLIGHT; ++u) {
      if (t2 < nslots) {                                           // wave-uniform
        int c = lane + 64 * j2;
        c = c < kchunks ? c : kchunks - 1;                         // buf[u] and its scale are zero there
        h2 sz, nz;
        if constexpr (SZ_DWORDS) {
          const int half = 16 * ((slot_row(t2) * G + g.group_of(c)) & 1);          // which half of the two dwords (zero dwords past the end)
          sz = splat_scale((uint16_t)(bsz[u][0] >> half)), nz = splat_negzero((uint16_t)(bsz[u][1] >> half));
        } else {
          sz = splat_scale((uint16_t)(bsz[u] & 0xffff)), nz = splat_negzero((uint16_t)(bsz[u] >> 16));
        }
        const int rot = unit_rot(c);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          h2 w[4];
          dequant8((unsigned)buf[u][i], sz, nz, w);
          const int uoff = c * 64 + (((i + rot) & 3) << 4);
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            if (m < M) {
              const v8h xv = *reinterpret_cast<const v8h*>(smem + (size_t)m * K * 2 + uoff);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                acc[m] = __builtin_fmaf((float)w[e][0], (float)xv[2 * e], acc[m]);
                acc[m] = __builtin_fmaf((float)w[e][1], (float)xv[2 * e + 1], acc[m]);
              }
            }
          }
        }
        if (j2 == cpl - 1) {                                       // row slot t2 complete
          float sums[MT];
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            sums[m] = wave_sum_f_rowbcast(acc[m]);
            acc[m] = 0.f;
          }
          row_done(t2, sums);
        }
        if (++j2 == cpl) { j2 = 0; ++t2; }
      }
    }
    t = t2;
    j = j2;
    if (t < nslots) issue(t, j);
  }
}

}  // namespace mq
