// The per-slice pass and the fixed-order row sum of the log-probability rule (csrc/mq_logprob.hip's header), shared by
// mq_logprob_top (mq_logprob.hip) and mq_beam_select (mq_beam.hip): ONE body, so both entry points give a row the same order, the same
// m and the same bits of logf(S) by construction.  The rule, the order of the sum and the error bound are written in mq_logprob.hip.
#ifndef MQ_LOGPROB_SLICE_H
#define MQ_LOGPROB_SLICE_H

#include "mq_common.h"

namespace mq {
namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr int LP_SLICE = 4096;                       // entries per slice: 16 per thread, held in registers
constexpr int LP_STEPS = LP_SLICE / (4 * LP_THREADS);
constexpr int LP_MAX_SLICES = (1 << 20) / LP_SLICE;  // 256
constexpr int LP_MAX_TOP = MQ_LOGPROB_MAX_TOP;
typedef unsigned long long u64;

struct LpPart {
  float m, s;                     // the slice's maximum and its sum of e_i
  int c, pad;                     // keys of the slice above the chosen token's key
};

static_assert(MQ_LOGPROB_SCRATCH_BYTES == MQ_DECODE_MAX_BATCH * LP_MAX_SLICES * (sizeof(LpPart) + LP_MAX_TOP * sizeof(u64)),
              "scratch holds every row's partials and candidate keys");
static_assert(LP_STEPS == 4 && LP_WAVES == 4, "the order of the sum in the header is written for 4 steps and 4 waves");

// reduction slots of one body (each reduction has its own: no barrier is needed between two of them)
struct LpRed {
  float f[2][LP_WAVES];
  int i[LP_WAVES];
  u64 k[2][LP_WAVES];
  float sum;
};

__device__ __forceinline__ float lp_norm(float l) { return l != l ? -__builtin_inff() : l + 0.f; }

// step 3 of the rule
__device__ __forceinline__ float lp_term(float l, float m) { return l == m ? 1.f : expf(l - m); }
__device__ __forceinline__ float lp_of(float l, float m, float log_s) {
  if (m == -__builtin_inff()) return m;
  const float d = l == m ? 0.f : l - m;
  return d - log_s;
}

// a barrier with none of this wave's LDS operations (the shuffles are LDS operations) in flight
__device__ __forceinline__ void lp_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

__device__ __forceinline__ float lp_wave_sum(float a) {           // the xor butterfly of the header: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) a = a + __shfl_xor(a, o);
  return a;
}
__device__ __forceinline__ float lp_wave_max(float a) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) a = fmaxf(a, __shfl_xor(a, o));
  return a;
}
__device__ __forceinline__ int lp_wave_sum_i(int a) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o);
  return a;
}
// The key maximum of a wave (all 64 lanes active), wave-uniform: mq_common.h's DPP row reduction on the key's two dwords -- a shuffle is
// an LDS round trip, and the n_top dependent rounds of a launch are nothing but this reduction and a barrier.  A maximum is exact in any order.
template <int CTRL>
__device__ __forceinline__ u64 lp_dpp_k(u64 v) {
  const unsigned lo = (unsigned)dpp_mov_i<CTRL>((int)(unsigned)v), hi = (unsigned)dpp_mov_i<CTRL>((int)(unsigned)(v >> 32));
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 lp_readlane_k(u64 v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 lp_max_k(u64 a, u64 b) { return b > a ? b : a; }
__device__ __forceinline__ u64 lp_wave_max_k(u64 a) {
  a = lp_max_k(a, lp_dpp_k<0xB1>(a));                                // quad_perm [1,0,3,2]
  a = lp_max_k(a, lp_dpp_k<0x4E>(a));                                // quad_perm [2,3,0,1]
  a = lp_max_k(a, lp_dpp_k<0x141>(a));                               // row_half_mirror
  a = lp_max_k(a, lp_dpp_k<0x140>(a));                               // row_mirror: every lane = its row-of-16 maximum
  return lp_max_k(lp_max_k(lp_readlane_k(a, 15), lp_readlane_k(a, 31)), lp_max_k(lp_readlane_k(a, 47), lp_readlane_k(a, 63)));
}

// One slice of a live row: (m_s, S_s), the count of keys above the chosen token's and the slice's first n_top keys in order (0: none
// left), written by thread 0 through o_part / o_keys (scratch, or LDS in the one-launch form).
__device__ __forceinline__ void lp_slice(const float* __restrict__ row, int V, int s, long long t, int n_top, LpPart* o_part, u64* o_keys, LpRed& R) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = s * LP_SLICE, hi = min(V, lo + LP_SLICE);
  const float NEG_INF = -__builtin_inff();
  float x[4 * LP_STEPS];
  bool in[LP_STEPS];
#pragma unroll
  for (int k = 0; k < LP_STEPS; ++k) {
    const int i = lo + 4 * LP_THREADS * k + 4 * tid;
    in[k] = i < hi;                                                  // (lo, hi and i are multiples of 4: i < hi covers i + 3)
    const float4 l = in[k] ? *reinterpret_cast<const float4*>(row + i) : make_float4(NEG_INF, NEG_INF, NEG_INF, NEG_INF);
    x[4 * k] = lp_norm(l.x); x[4 * k + 1] = lp_norm(l.y); x[4 * k + 2] = lp_norm(l.z); x[4 * k + 3] = lp_norm(l.w);
  }
  const bool have_t = t >= 0 && t < (long long)V;
  const u64 kt = have_t ? sort_key(lp_norm(row[t]), (int)t) : ~0ull;   // uniform load, behind the range check

  float mx = NEG_INF;
#pragma unroll
  for (int j = 0; j < 4 * LP_STEPS; ++j) mx = fmaxf(mx, x[j]);
  mx = lp_wave_max(mx);
  if (lane == 0) R.f[0][wave] = mx;
  lp_sync();
  const float ms = fmaxf(fmaxf(R.f[0][0], R.f[0][1]), fmaxf(R.f[0][2], R.f[0][3]));

  float a = 0.f;
  int c = 0;
  u64 key[4 * LP_STEPS];
  u64 best = 0;
#pragma unroll
  for (int k = 0; k < LP_STEPS; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = 4 * k + e;
      if (ms != NEG_INF) a = a + lp_term(x[j], ms);
      key[j] = in[k] ? sort_key(x[j], lo + 4 * LP_THREADS * k + 4 * tid + e) : 0ull;          // (a key of an entry is never 0)
      c += key[j] > kt ? 1 : 0;
      best = key[j] > best ? key[j] : best;
    }
  a = lp_wave_sum(a);
  c = lp_wave_sum_i(c);
  if (lane == 0) { R.f[1][wave] = a; R.i[wave] = c; }
  lp_sync();
  if (tid == 0) {
    LpPart p;
    p.m = ms;
    p.s = ((R.f[1][0] + R.f[1][1]) + R.f[1][2]) + R.f[1][3];
    p.c = (R.i[0] + R.i[1]) + (R.i[2] + R.i[3]);
    p.pad = 0;
    *o_part = p;
  }

  // the first n_top keys: per round the block's best key; its owner drops it and rescans its 16
  for (int r = 0; r < n_top; ++r) {
    const u64 wb = lp_wave_max_k(best);
    if (lane == 0) R.k[r & 1][wave] = wb;
    lp_sync();                                                       // (double-buffered: round r + 2 writes after round r + 1's barrier)
    u64 g = R.k[r & 1][0];
#pragma unroll
    for (int w = 1; w < LP_WAVES; ++w) g = R.k[r & 1][w] > g ? R.k[r & 1][w] : g;
    if (tid == 0) o_keys[r] = g;
    if (g != 0ull && best == g) {                                    // keys are distinct: one owner
      best = 0;
#pragma unroll
      for (int j = 0; j < 4 * LP_STEPS; ++j) {
        if (key[j] == g) key[j] = 0ull;
        best = key[j] > best ? key[j] : best;
      }
    }
  }
}

// The row's m, logf(S) (0 when m == -inf) and count of keys above the chosen token's from its ns partials (in LDS): the maxima and
// counts order-free, the sum in the fixed order of the rule.  Workgroup-uniform results; two barriers.
__device__ __forceinline__ void lp_row_stats(const LpPart* part, int ns, LpRed& R, float* o_m, float* o_log_s, int* o_in_front) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float NEG_INF = -__builtin_inff();
  float mx = tid < ns ? part[tid].m : NEG_INF;
  int c = tid < ns ? part[tid].c : 0;
  mx = lp_wave_max(mx);
  c = lp_wave_sum_i(c);
  if (lane == 0) { R.f[0][wave] = mx; R.i[wave] = c; }
  lp_sync();
  const float m = fmaxf(fmaxf(R.f[0][0], R.f[0][1]), fmaxf(R.f[0][2], R.f[0][3]));
  *o_in_front = (R.i[0] + R.i[1]) + (R.i[2] + R.i[3]);
  if (wave == 0) {
    float b = 0.f;
    if (m != NEG_INF) {
#pragma unroll
      for (int q = 0; q < LP_MAX_SLICES / 64; ++q) {
        const int s = lane + 64 * q;
        if (s < ns && part[s].m != NEG_INF) {
          const float f = lp_term(part[s].m, m);
          const float w = part[s].s * f;
          b = b + w;
        }
      }
    }
    b = lp_wave_sum(b);
    if (lane == 0) R.sum = b;
  }
  lp_sync();
  *o_m = m;
  *o_log_s = m != NEG_INF ? logf(R.sum) : 0.f;
}

}  // namespace
}  // namespace mq

#endif  // MQ_LOGPROB_SLICE_H
