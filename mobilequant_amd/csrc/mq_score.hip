// Token scoring: the fp32 lm_head fused with its log-softmax (mq_score_head).  No logits tensor is ever written.
//
// Launch 1 (score_tiles_kernel): one workgroup per (128-row tile of y, 128-entry tile of the vocabulary).  The logits of the tile are
// computed with exact fp32-input MFMA (v_mfma_f32_32x32x2_f32) from LDS-staged y / W tiles (k in stages of 32, the next stage's
// global loads in flight behind the current stage's MFMAs) and reduced, per row, to a partial
// (max, sum exp(l - max), first argmax) written to scratch [M][T] (T = ceil(V / 128)); the one workgroup whose tile holds a row's
// target writes that logit to tlogit[M].  Workgroups are numbered so that consecutive ones share a W tile (the row tile runs fastest)
// and, when the grid is a multiple of 8, each XCD takes a contiguous range of them, so every W tile is read from HBM about once.
// Launch 2 (score_merge_kernel): one wave per row merges the T partials: lane i takes tiles i, i + 64, ... in order, the lanes combine
// in a fixed xor butterfly.  No atomics anywhere: the result bits are the same run to run.
//
// Row independence.  Every logit is the MFMA's fp32 fma chain over k in one fixed order (a fixed permutation of 0 .. K-1, the same for
// every row and column), started from 0; the bias is added once.  The tile reductions visit a row's 128 logits in an order fixed by the
// vocabulary index alone, and the merge visits tiles in an order fixed by T.  So a row's outputs depend on its own y row, W, bias and
// target only -- not on M, not on its position in a row tile, not on the other rows.
//
// Special values.  A column past V is -inf with index INT_MAX (it never wins and adds exp(-inf) = 0).  A tile whose row is entirely
// -inf gives (max -inf, sum 0), merged as 0: no NaN.  NaN is the largest value and, among NaNs, the lowest index wins: a NaN logit
// makes lse and logprob NaN and argmax its first NaN, as torch.logsumexp / torch.argmax do.  Among equal logits the lowest index wins.
//
// Error bound (u = 2^-24, gamma_n = n u / (1 - n u)).  Per logit, with s_v = |b_v| + sum_k |y_k w_vk|:
//     |l^_v - l_v| <= e_v = gamma_{K+1} s_v                 (K fma roundings in the chain, one for the bias add; any k order)
// lse is 1-Lipschitz in the max norm, so lse(l^) is within E = max_v e_v of lse(l).  Its evaluation adds, relative to S = sum exp:
//   the two subtractions l - m_tile and m_tile - m (each rounded once, both <= m - l): 2 u (m - l_v) per term, which weighted by
//   p_v sums to at most 2 u log V (sum_v p_v (m - l_v) = log p_max + H(p) <= log V); two expf per term within 2 ulp each (4 u each,
//   ASSUMED: the device expf / logf ulp figures are not measured here); the products and sums: gamma_{127 + T + 2}.  Then
//   lse = m + log S (logf within 2 ulp of log S <= log V, one add):
//     |lse^ - lse| <= E + 1.01 (2 u log V + 8 u + gamma_{T + 129}) + 4 u log V + u |lse|
//     |logprob^ - logprob| <= e_target + |lse^ - lse| + u |logprob|
// tests/test_gpu_score.py evaluates these bounds per row in float64.
#include "mq_common.h"

#include <limits.h>

namespace mq {
namespace {

constexpr int SC_BV = 128;               // vocabulary entries per tile (the partials' granularity: T = ceil(V / SC_BV))
constexpr int SC_BM = 128;               // rows of y per tile
constexpr int SC_BK = 32;                // k per LDS stage (64 measured slower: 126-129 TF against 132 at V = 32 000 ... 256 000)
constexpr int SC_LD = SC_BK + 4;         // LDS row stride in floats: 144 B, the 16-byte fragment reads of 8 lanes hit distinct banks
constexpr int SC_CPR = SC_BK / 4;        // float4 columns per staged row
constexpr int SC_THREADS = 256;          // 4 waves: 2 (vocab halves) x 2 (row halves), each 64 x 64 = 2 x 2 MFMA tiles of 32 x 32
constexpr int SC_RPP = SC_THREADS / SC_CPR;    // rows staged per pass

typedef float f32x16 __attribute__((ext_vector_type(16)));

// (a, ia) ranks above (b, ib): NaN above everything, then the larger value, then the lower index.  A total order, so any merge
// order selects the same element.
__device__ __forceinline__ bool better(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na || nb) return na && (!nb || ia < ib);
  return a > b || (a == b && ia < ib);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

__global__ __launch_bounds__(SC_THREADS, 2) void score_tiles_kernel(const float* __restrict__ y, long long ldy, const float* __restrict__ w,
                                                                    const float* __restrict__ bias, const long long* __restrict__ tgt, int M,
                                                                    int K, int V, int n_mt, int T, float* __restrict__ pmax,
                                                                    float* __restrict__ psum, int* __restrict__ pidx,
                                                                    float* __restrict__ tlogit) {
  __shared__ float sw[SC_BV * SC_LD];
  __shared__ float sy[SC_BM * SC_LD];
  __shared__ float red_v[2][SC_BM];
  __shared__ int red_i[2][SC_BM];
  __shared__ float red_s[2][SC_BM];

  unsigned g = blockIdx.x;
  const unsigned G = gridDim.x;
  if ((G & 7u) == 0) g = (g & 7u) * (G >> 3) + (g >> 3);        // XCD x (dispatch order g % 8) takes logical tiles [x G/8, (x+1) G/8)
  const int mt = (int)(g % (unsigned)n_mt), vt = (int)(g / (unsigned)n_mt);
  const int m0 = mt * SC_BM, v0 = vt * SC_BV;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wv = wave & 1, wm = wave >> 1;
  const int h = lane >> 5, i = lane & 31;

  // staging: thread t copies float4 column t % SC_CPR of rows t / SC_CPR + SC_RPP p of both tiles; rows past V / M read the last
  // row (their results are masked / never stored), k past K reads zeros (0 * 0 adds exactly nothing to the chain)
  constexpr int NP = SC_BV / SC_RPP;
  const int lr = t / SC_CPR, lc = (t % SC_CPR) * 4;
  const float* wsrc[NP];
  const float* ysrc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int v = min(v0 + lr + SC_RPP * p, V - 1), m = min(m0 + lr + SC_RPP * p, M - 1);
    wsrc[p] = w + (long long)v * K + lc;
    ysrc[p] = y + (long long)m * ldy + lc;
  }
  float4 rw[NP], ry[NP];
  auto load = [&](int k0) {
    const bool in = k0 + lc < K;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      rw[p] = in ? *reinterpret_cast<const float4*>(wsrc[p] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
      ry[p] = in ? *reinterpret_cast<const float4*>(ysrc[p] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int nk = (K + SC_BK - 1) / SC_BK;
  load(0);
  for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      *reinterpret_cast<float4*>(&sw[(lr + SC_RPP * p) * SC_LD + lc]) = rw[p];
      *reinterpret_cast<float4*>(&sy[(lr + SC_RPP * p) * SC_LD + lc]) = ry[p];
    }
    __syncthreads();
    if (kt + 1 < nk) load((kt + 1) * SC_BK);         // in flight while the MFMAs run
    // 32x32x2 operands: lane (i, h) gives A[v i][k h] and B[k h][m i].  Lane half h reads k = 4 (2 q + h) + r at step (q, r): a fixed
    // permutation of the stage's k, the same for W and y, so every product pairs the right k.
#pragma unroll
    for (int q = 0; q < SC_BK / 8; ++q) {
      float4 a[2], b[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        a[s] = *reinterpret_cast<const float4*>(&sw[(wv * 64 + s * 32 + i) * SC_LD + 4 * (2 * q + h)]);
        b[s] = *reinterpret_cast<const float4*>(&sy[(wm * 64 + s * 32 + i) * SC_LD + 4 * (2 * q + h)]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int vs = 0; vs < 2; ++vs)
#pragma unroll
          for (int ms = 0; ms < 2; ++ms)
            acc[vs][ms] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[vs][r], b[ms][r], acc[vs][ms], 0, 0, 0);
    }
    __syncthreads();
  }

  // acc[vs][ms][reg] = logit of v = v0 + wv 64 + vs 32 + (reg & 3) + 8 (reg >> 2) + 4 h, row m = m0 + wm 64 + ms 32 + i
  const float NEG_INF = -__builtin_inff();
#pragma unroll
  for (int ms = 0; ms < 2; ++ms) {
    const int ml = wm * 64 + ms * 32 + i, m = m0 + ml;
    const long long tg = (tgt && m < M) ? tgt[m] : -1;
    float bv = NEG_INF;
    int bi = INT_MAX;
#pragma unroll
    for (int vs = 0; vs < 2; ++vs)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int v = v0 + wv * 64 + vs * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        float l = acc[vs][ms][r];
        if (v < V) {
          if (bias) l = l + bias[v];
          if ((long long)v == tg) tlogit[m] = l;
        } else {
          l = NEG_INF;
        }
        acc[vs][ms][r] = l;
        const int vi = v < V ? v : INT_MAX;
        if (better(l, vi, bv, bi)) {
          bv = l;
          bi = vi;
        }
      }
    const float ov = __shfl_xor(bv, 32);
    const int oi = __shfl_xor(bi, 32);
    if (better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
    if (h == 0) {
      red_v[wv][ml] = bv;
      red_i[wv][ml] = bi;
    }
  }
  __syncthreads();
#pragma unroll
  for (int ms = 0; ms < 2; ++ms) {
    const int ml = wm * 64 + ms * 32 + i;
    const bool hi = better(red_v[1][ml], red_i[1][ml], red_v[0][ml], red_i[0][ml]);
    const float mx = red_v[hi ? 1 : 0][ml];
    float s = 0.f;
    if (mx != NEG_INF) {
#pragma unroll
      for (int vs = 0; vs < 2; ++vs)
#pragma unroll
        for (int r = 0; r < 16; ++r) s = s + expf(acc[vs][ms][r] - mx);
    }
    s = s + __shfl_xor(s, 32);                       // a + b: both lanes get the same bits
    if (h == 0) red_s[wv][ml] = s;
  }
  __syncthreads();
  if (t < SC_BM && m0 + t < M) {
    const int m = m0 + t;
    const bool hi = better(red_v[1][t], red_i[1][t], red_v[0][t], red_i[0][t]);
    const long long o = (long long)m * T + vt;
    pmax[o] = red_v[hi ? 1 : 0][t];
    pidx[o] = red_i[hi ? 1 : 0][t];
    psum[o] = red_s[0][t] + red_s[1][t];
  }
}

constexpr int MG_THREADS = 256;                   // one wave per row, 4 rows per workgroup

__global__ __launch_bounds__(MG_THREADS) void score_merge_kernel(const float* __restrict__ pmax, const float* __restrict__ psum,
                                                                 const int* __restrict__ pidx, const float* __restrict__ tlogit,
                                                                 const long long* __restrict__ tgt, int M, int T, int V,
                                                                 float* __restrict__ logprob, float* __restrict__ lse,
                                                                 long long* __restrict__ amax) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (MG_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= M) return;                            // wave-uniform
  const float NEG_INF = -__builtin_inff();
  const float* pm = pmax + (long long)row * T;
  const float* ps = psum + (long long)row * T;
  const int* pi = pidx + (long long)row * T;
  float bv = NEG_INF;
  int bi = INT_MAX;
  for (int j = lane; j < T; j += 64) {
    const float a = pm[j];
    const int ia = pi[j];
    if (better(a, ia, bv, bi)) {
      bv = a;
      bi = ia;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  const float mx = bv;                              // every lane holds the same (value, index)
  float s = 0.f;
  for (int j = lane; j < T; j += 64) {
    const float a = pm[j];
    if (a != NEG_INF) s = s + ps[j] * expf(a - mx);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s = s + __shfl_xor(s, o);      // xor butterfly: every lane ends with the same bits
  if (lane == 0) {
    const float l = mx + logf(s);
    const long long tg = tgt ? tgt[row] : -1;
    lse[row] = l;
    logprob[row] = (tg >= 0 && tg < V) ? tlogit[row] - l : 0.f;
    amax[row] = bi;
  }
}

}  // namespace
}  // namespace mq

using namespace mq;

extern "C" {

int64_t mq_score_head_scratch_bytes(int64_t M, int64_t V) {
  if (M < 0 || V < 1) return -1;
  const size_t T = (size_t)((V + SC_BV - 1) / SC_BV);
  return (int64_t)(3 * align256((size_t)M * T * 4) + align256((size_t)M * 4));
}

int mq_score_head(const float* y, int64_t y_stride, const float* w, const float* bias, const int64_t* targets, int64_t M, int64_t K, int64_t V,
                  void* scratch, int64_t scratch_bytes, float* logprob, float* lse, int64_t* argmax, mq_stream_t stream) {
  MQ_REQUIRE(M >= 0, "mq_score_head: M < 0");
  if (M == 0) return MQ_OK;
  MQ_REQUIRE(y && w && scratch && logprob && lse && argmax, "mq_score_head: null pointer (y, w, scratch and the three outputs are required)");
  MQ_REQUIRE(V >= 1 && V <= (int64_t)INT_MAX - SC_BV, "mq_score_head: V must be in [1, 2^31 - 129]");
  MQ_REQUIRE(K >= 4 && K % 4 == 0 && K <= 65536, "mq_score_head: K must be a multiple of 4 in [4, 65536]");
  MQ_REQUIRE(y_stride >= K && y_stride % 4 == 0, "mq_score_head: y_stride must be >= K and a multiple of 4");
  MQ_REQUIRE(M <= (1 << 24), "mq_score_head: M must be <= 2^24");
  MQ_REQUIRE(aligned(y, 16) && aligned(w, 16), "mq_score_head: y and w must be 16-byte aligned");
  MQ_REQUIRE(aligned(scratch, 256), "mq_score_head: scratch must be 256-byte aligned");
  MQ_REQUIRE(scratch_bytes >= mq_score_head_scratch_bytes(M, V), "mq_score_head: scratch_bytes below mq_score_head_scratch_bytes(M, V)");
  const int T = (int)((V + SC_BV - 1) / SC_BV);
  const int n_mt = (int)((M + SC_BM - 1) / SC_BM);
  MQ_REQUIRE((int64_t)n_mt * T < (int64_t)UINT_MAX, "mq_score_head: too many tiles (M x V)");
  char* base = static_cast<char*>(scratch);
  const size_t part = align256((size_t)M * T * 4);
  float* pmax = reinterpret_cast<float*>(base);
  float* psum = reinterpret_cast<float*>(base + part);
  int* pidx = reinterpret_cast<int*>(base + 2 * part);
  float* tlogit = reinterpret_cast<float*>(base + 3 * part);
  const long long* tg = reinterpret_cast<const long long*>(targets);
  hipStream_t st = as_stream(stream);
  score_tiles_kernel<<<(unsigned)((int64_t)n_mt * T), SC_THREADS, 0, st>>>(y, (long long)y_stride, w, bias, tg, (int)M, (int)K, (int)V, n_mt, T,
                                                                           pmax, psum, pidx, tlogit);
  MQ_LAUNCH_CHECK("mq_score_head");
  score_merge_kernel<<<(unsigned)((M + 3) / 4), MG_THREADS, 0, st>>>(pmax, psum, pidx, tlogit, tg, (int)M, T, (int)V, logprob, lse,
                                                                     reinterpret_cast<long long*>(argmax));
  MQ_LAUNCH_CHECK("mq_score_head");
  return MQ_OK;
}

}  // extern "C"
