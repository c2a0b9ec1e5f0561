// Clip search for learnable weight clipping (VALU-bound): every row of a weight is read ONCE, stays in registers, and a table of
// candidate clip factors is walked over it; per row the kernel reports the candidate with the least quantization error.
//
// What mq_lwc_search computes (tests/lwc_search_ref.py restates it).  For row r of w [rows, cols] and candidate c < C:
//   mn, mx   the row's min / max as mq_lwc_fake_quant takes them (one NaN in the row makes both NaN)
//   grid     lwc_grid(mn, mx, sig_lo[c], sig_hi[c], qmax, symmetric)                                 (mq_lwc.h, the forward's expression)
//   y[k]     dequant(index_value_keepnan(w[r, k], scale, 1 / scale, offset, qmin, qmax), scale, offset)   -- the bits mq_lwc_fake_quant
//            writes for that pair of factors
//   e[k]     __fsub_rn(y[k], w[r, k])           on the ROUNDED y: the dequant multiply is not contracted into the subtraction
//   term[k]  ((double)e[k] * (double)e[k]) * (double)col_weight[(r % (cw_len / cols)) * cols + k]
//            the square is exact in fp64, the weighting is one rounding and is left out when col_weight is NULL
//   cost[r, c] = the fp64 sum of the row's terms, in an order that depends on the geometry below
// Selection: candidate 0 is the incumbent; a later candidate replaces the best so far only if its cost is strictly smaller (`<`: every
// comparison with a NaN is false).  Ties go to the lowest index; a row with a NaN reports index 0 and NaN costs.
// lwc_grid's scale is inside [1e-5, 1e6] or NaN, so x / scale always takes the reciprocal form (mq_common.h): inside that range it gives
// the index of the IEEE divide, and with a NaN scale both forms give NaN.
//
// Three geometries, by row length (the host picks; the results differ in summation order only):
//   cols <= 128          a LANE owns a row (64 rows per 64-thread workgroup): a group_size row of 64 / 128 columns would leave most of
//                        a wave idle, and here no lane is idle and no candidate needs a reduction at all
//   128 < cols <= 1024   a WAVE owns a row (4 rows per workgroup), four 16-byte vectors per lane at most
//   1024 < cols          a WORKGROUP owns a row, 4 or 16 vectors per thread (cols <= 4096 / <= 16384)
// In the last two every thread carries the partial sums of a block of FOUR candidates; the block is reduced together: the partials go
// through LDS transposed, so that 16 lanes (wave form) or one wave (workgroup form) sum ONE candidate -- 2 barriers, 4 LDS reads and one
// short DPP reduction per four candidates instead of four full wave (+ workgroup) reductions.
#include "mq_common.h"
#include "mq_lwc.h"

#pragma clang fp contract(off)

namespace mq {

constexpr int LWC_SEARCH_CB = 4;          // candidates whose partial sums are carried and reduced together

struct LwcSearchArgs {
  const float* w;
  const float* sig_lo;
  const float* sig_hi;
  const float* col_weight;
  int64_t rows;
  int cols, n_cand, cw_rows, symmetric;
  float qmin, qmax;
  int* best_idx;
  double* best_cost;
  double* base_cost;
  double* costs;
};

template <int CTRL>
__device__ __forceinline__ double dpp_mov_d(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const unsigned lo = (unsigned)dpp_mov_i<CTRL>((int)(unsigned)b), hi = (unsigned)dpp_mov_i<CTRL>((int)(unsigned)(b >> 32));
  return __builtin_bit_cast(double, (long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double readlane_d(double v, int l) {
  const long long b = __builtin_bit_cast(long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
  return __builtin_bit_cast(double, (long long)(((unsigned long long)hi << 32) | lo));
}
// every lane of a 16-lane DPP row gets the row's sum (all 64 lanes active)
__device__ __forceinline__ double row16_sum_d(double v) {
  v += dpp_mov_d<0xB1>(v);                                          // quad_perm [1,0,3,2]
  v += dpp_mov_d<0x4E>(v);                                          // quad_perm [2,3,0,1]
  v += dpp_mov_d<0x141>(v);                                         // row_half_mirror
  v += dpp_mov_d<0x140>(v);                                         // row_mirror
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
  v = row16_sum_d(v);
  return (readlane_d(v, 15) + readlane_d(v, 31)) + (readlane_d(v, 47) + readlane_d(v, 63));
}

// the running (base, best) of one row, kept by the one thread that sees the row's finished costs in candidate order
struct LwcBest {
  double base, best;
  int idx;
  __device__ __forceinline__ void take(int c, double cost) {
    if (c == 0) {
      base = best = cost;
      idx = 0;
    } else if (cost < best) {                                       // strict: a tie keeps the lower index, a NaN never wins
      best = cost;
      idx = c;
    }
  }
};

// what the element loop needs of a candidate's grid
struct LwcCand {
  float scale, offset, inv_s;
};
__device__ __forceinline__ LwcCand lwc_cand(float mn, float mx, float sig_lo, float sig_hi, float qmax, int symmetric) {
  const LwcGrid g = lwc_grid(mn, mx, sig_lo, sig_hi, qmax, symmetric);
  return {g.scale, g.offset, __fdiv_rn(1.0f, g.scale)};
}

// TPR threads per row: 1 (lane), 64 (wave) or 256 (workgroup); VPT 16-byte vectors of the row per thread; WEIGHTED: col_weight given.
template <int VPT, int TPR, bool WEIGHTED>
__global__ void __launch_bounds__(TPR == 1 ? 64 : 256) lwc_search_kernel(const LwcSearchArgs a) {
  constexpr int THREADS = TPR == 1 ? 64 : 256;
  constexpr int ROWS_PER_WG = THREADS / TPR;
  constexpr int CB = TPR == 1 ? 1 : LWC_SEARCH_CB;
  const int tid = threadIdx.x;
  const int sub = TPR == 1 ? 0 : (tid & (TPR - 1));                  // this thread's place in its row
  const int slot = TPR == 1 ? tid : tid / TPR;                      // the row's place in the workgroup
  const int64_t row_raw = (int64_t)blockIdx.x * ROWS_PER_WG + slot;
  const bool live = row_raw < a.rows;
  const int64_t row = live ? row_raw : a.rows - 1;                  // a workgroup's surplus threads redo the last row (barriers stay uniform) and write nothing
  const int cols = a.cols, nvec = cols >> 2, C = a.n_cand;
  const vf4* wr = reinterpret_cast<const vf4*>(a.w + row * cols);
  LwcRow<VPT> r, cw;                                               // cw: the row's col_weight, beside it in registers (not in the lane form)
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int i = sub + TPR * k;
    if (i < nvec) r.v[k] = __builtin_nontemporal_load(wr + i);
  }
  // lane form: 32 more vectors per lane would halve the occupancy; every candidate re-reads them through the vector L1 instead
  const vf4* cr = WEIGHTED ? reinterpret_cast<const vf4*>(a.col_weight + (row % a.cw_rows) * cols) : nullptr;
  if (WEIGHTED && TPR != 1) {
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      const int i = sub + TPR * k;
      if (i < nvec) cw.v[k] = cr[i];                                // shared by many rows: a normal load
    }
  }

  // ---- the row's range, as lwc_fake_quant_kernel takes it -------------------------------------------------------------------------
  float mn = INFINITY, mx = -INFINITY;
  int nan = 0;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    if (sub + TPR * k < nvec) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = r.v[k][e];
        mn = fminf(mn, x);
        mx = fmaxf(mx, x);
        nan |= (x != x);
      }
    }
  }
  __shared__ float s_mn[4], s_mx[4];
  __shared__ int s_nan[4];
  if (TPR >= 64) {
    mn = wave_min(mn);
    mx = wave_max(mx);
    nan = __builtin_amdgcn_ballot_w64(nan != 0) != 0;
  }
  if (TPR == 256) {
    const int wv = tid >> 6;
    if ((tid & 63) == 0) {
      s_mn[wv] = mn;
      s_mx[wv] = mx;
      s_nan[wv] = nan;
    }
    __syncthreads();
    mn = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
    mx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    nan = s_nan[0] | s_nan[1] | s_nan[2] | s_nan[3];
  }
  if (nan) mn = mx = __builtin_nanf("");                             // amin / amax propagate NaN

  // ---- the candidates --------------------------------------------------------------------------------------------------------------
  __shared__ double s_part[TPR == 1 ? 1 : CB * 256];                // [candidate of the block][thread]
  __shared__ double s_cost[TPR == 1 ? 1 : ROWS_PER_WG * CB];        // [row of the workgroup][candidate of the block]
  __shared__ float s_rng[2 * ROWS_PER_WG];                          // the rows' (min, max)
  __shared__ LwcCand s_cand[TPR == 1 ? 1 : ROWS_PER_WG * CB];       // the block's grids: one thread derives each, nobody repeats the divisions
  // thread t < ROWS_PER_WG * CB derives the grid of (row t / CB, candidate c0 + t % CB) for the whole row
  auto fill_grids = [&](int c0) {
    if (tid < ROWS_PER_WG * CB) {
      const int c = min(c0 + tid % CB, C - 1);                      // past the table: the last candidate again, its cost is dropped below
      s_cand[tid] = lwc_cand(s_rng[2 * (tid / CB)], s_rng[2 * (tid / CB) + 1], a.sig_lo[c], a.sig_hi[c], a.qmax, a.symmetric);
    }
  };
  if constexpr (TPR != 1) {
    if (sub == 0) {
      s_rng[2 * slot] = mn;
      s_rng[2 * slot + 1] = mx;
    }
    __syncthreads();
    fill_grids(0);
    __syncthreads();
  }
  LwcBest best = {0.0, 0.0, 0};
  double* cost_row = a.costs ? a.costs + row * (int64_t)C : nullptr;
  for (int c0 = 0; c0 < C; c0 += CB) {
    double acc[CB];
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const LwcCand g = TPR == 1 ? lwc_cand(mn, mx, a.sig_lo[c0], a.sig_hi[c0], a.qmax, a.symmetric) : s_cand[slot * CB + j];
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < VPT; ++k) {
        if (sub + TPR * k < nvec) {
          vf4 cwk;
          if (WEIGHTED) cwk = TPR == 1 ? cr[k] : cw.v[k];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float x = r.v[k][e];
            const float y = dequant(index_value_keepnan(x, g.scale, g.inv_s, g.offset, a.qmin, a.qmax, true), g.scale, g.offset);
            const double d = (double)__fsub_rn(y, x);
            double t = d * d;
            if (WEIGHTED) t = t * (double)cwk[e];
            s += t;
          }
        }
      }
      acc[j] = s;
    }
    if constexpr (TPR == 1) {
      if (live) {
        if (cost_row) cost_row[c0] = acc[0];
        best.take(c0, acc[0]);
      }
    } else {
      // the block's partials, transposed through LDS: 16 lanes (TPR 64) / one wave (TPR 256) sum one candidate
#pragma unroll
      for (int j = 0; j < CB; ++j) s_part[j * 256 + tid] = acc[j];
      __syncthreads();                                              // every thread is done with this block's grids as well
      const int lane = tid & 63, wv = tid >> 6;
      if constexpr (TPR == 64) {
        const int j = lane >> 4, p = lane & 15;
        const double* src = s_part + j * 256 + wv * 64 + p;
        const double t = row16_sum_d((src[0] + src[16]) + (src[32] + src[48]));
        if (p == 0) s_cost[wv * CB + j] = t;
      } else {
        const double* src = s_part + wv * 256 + lane;
        const double t = wave_sum_d((src[0] + src[64]) + (src[128] + src[192]));
        if (lane == 0) s_cost[wv] = t;
      }
      if (c0 + CB < C) fill_grids(c0 + CB);
      __syncthreads();
      // the row's first thread takes the block in candidate order; s_cost is rewritten only behind the next block's first barrier
      if (sub == 0 && live) {
#pragma unroll
        for (int j = 0; j < CB; ++j) {
          if (c0 + j < C) {
            const double cost = s_cost[slot * CB + j];
            if (cost_row) cost_row[c0 + j] = cost;
            best.take(c0 + j, cost);
          }
        }
      }
    }
  }
  if (sub == 0 && live) {
    a.best_idx[row] = best.idx;
    a.best_cost[row] = best.best;
    a.base_cost[row] = best.base;
  }
}

template <int VPT, int TPR>
static void launch_lwc_search(const LwcSearchArgs& a, hipStream_t st) {
  constexpr int THREADS = TPR == 1 ? 64 : 256, ROWS_PER_WG = THREADS / TPR;
  const unsigned grid = (unsigned)((a.rows + ROWS_PER_WG - 1) / ROWS_PER_WG);
  if (a.col_weight) lwc_search_kernel<VPT, TPR, true><<<grid, THREADS, 0, st>>>(a);
  else lwc_search_kernel<VPT, TPR, false><<<grid, THREADS, 0, st>>>(a);
}

}  // namespace mq

using namespace mq;

extern "C" int mq_lwc_search(const float* w, int64_t rows, int64_t cols, const float* sig_lo, const float* sig_hi, int64_t n_cand, int bitwidth,
                             int is_symmetric, const float* col_weight, int64_t cw_len, int32_t* best_idx, double* best_cost,
                             double* base_cost, double* costs, mq_stream_t stream) {
  MQ_REQUIRE(rows >= 0 && rows < (int64_t)0x7fffffff, "mq_lwc_search: bad row count %lld", (long long)rows);
  MQ_REQUIRE(cols % 4 == 0 && cols >= 16 && cols <= 16384, "mq_lwc_search: rows of 16 to 16384 columns, a multiple of 4 (cols=%lld)",
             (long long)cols);
  MQ_REQUIRE(n_cand >= 1 && n_cand <= 1024, "mq_lwc_search: 1 to 1024 candidates (n_cand=%lld)", (long long)n_cand);
  MQ_REQUIRE(bitwidth >= 2 && bitwidth <= 16, "mq_lwc_search: bitwidth=%d", bitwidth);
  MQ_REQUIRE(!col_weight || (cw_len >= cols && cw_len % cols == 0 && cw_len / cols < (int64_t)0x7fffffff),
             "mq_lwc_search: col_weight holds a multiple of cols=%lld entries (cw_len=%lld)", (long long)cols, (long long)cw_len);
  if (rows == 0) return MQ_OK;
  MQ_REQUIRE(w && sig_lo && sig_hi && best_idx && best_cost && base_cost, "mq_lwc_search: null pointer");
  MQ_REQUIRE(aligned(w, 16) && aligned(col_weight, 16), "mq_lwc_search: w and col_weight must be 16-byte aligned");
  LwcSearchArgs a;
  a.w = w;
  a.sig_lo = sig_lo;
  a.sig_hi = sig_hi;
  a.col_weight = col_weight;
  a.rows = rows;
  a.cols = (int)cols;
  a.n_cand = (int)n_cand;
  a.cw_rows = col_weight ? (int)(cw_len / cols) : 1;                 // cw_len / cols < 2^31: checked above
  a.symmetric = is_symmetric ? 1 : 0;
  a.qmin = is_symmetric ? -(float)(1 << (bitwidth - 1)) : 0.0f;
  a.qmax = is_symmetric ? (float)((1 << (bitwidth - 1)) - 1) : (float)((1 << bitwidth) - 1);
  a.best_idx = best_idx;
  a.best_cost = best_cost;
  a.base_cost = base_cost;
  a.costs = costs;
  hipStream_t st = as_stream(stream);
  if (cols <= 128) launch_lwc_search<32, 1>(a, st);
  else if (cols <= 1024) launch_lwc_search<4, 64>(a, st);
  else if (cols <= 4096) launch_lwc_search<4, 256>(a, st);
  else launch_lwc_search<16, 256>(a, st);
  MQ_LAUNCH_CHECK("mq_lwc_search");
  return MQ_OK;
}
