// Decode GEMV with PER-GROUP weight grids (QuantConfig group_size; qmodule.py:259-260, :292-293): the five-launch GEMV of both decode
// engines (mobilequant_amd/decode.py, decode_batch.py) for a model quantised with groups -- the prefill recipe of mq_gemm_grouped.hip
// at one token per sequence, for 1 .. MQ_DECODE_MAX_BATCH activation rows.
//
//   y[b, n] = sum_g alpha[g, n] * (P_g + cw[g, n] A_g + t[g, n]) + bias[n],   P_g = sum_{k in g} a'[b, k] w'[n, k],  A_g = sum_{k in g} a'[b, k]
//
// with the stored image bytes a' = ia - 128 and the stored weights w' (int8: index - 128; packed 4-bit: the unsigned nibble, cw
// carrying the shift).  Every bracket is an exact int32; they are folded in ascending g as acc = fmaf((float)bracket, alpha, acc)
// from acc = 0, then + bias as a separate add: mq_gemm_grouped.hip's order, so the value in front of the output grid equals
// mq_w8a8_linear_grouped's on the same image bit for bit.
//
// Everything outside the contraction is decode_gemv_batch_kernel's code (mq_decode_common.h: gemv_batch_prologue, GemvBatchEpilogue):
// PROLOGUE waves build the B int8 images in LDS, STREAM waves request weights and group vectors first.  Lane -> K mapping: lane l
// of pass j holds 16-byte chunk l + 64 j of a logical row, as in the per-channel launch, so a group of cg = group_size / 16 (int8) or
// / 32 (nibbles) chunks is cg ADJACENT lanes of one pass (cg <= 64) or whole passes (cg > 64; group_size a power of two).  Per chunk a
// lane adds P + cw A of its piece (cw: the lane's own group vector load; A: dot of the image piece with ones), so one DPP reduction
// over the group's lanes gives P_g + cw A_g, and t is added once.  The brackets of a pass's groups are then read lane by lane
// (v_readlane) and folded into a wave-uniform accumulator: 64-wide, no one-lane tail; the row's result lands in lane t (row slot t)
// as the per-channel launch's integer sums do.
#include "mq_decode_common.h"

namespace mq {

#pragma clang fp contract(off)

// chunks per lane in flight, each with its three group-vector words: 12 as decode_gemv_kernel for one row; 6 for B rows (8 spills the
// gate launch's W4 instantiation at 128 VGPRs)
template <int NB>
constexpr int dgr_inflight() { return NB == 1 ? 12 : 6; }

// sum over aligned groups of 2^lg adjacent lanes (lg <= 6, wave-uniform): wave_sum_dpp's steps, stopped where the group ends.  The
// group's sum is valid in its LAST lane (every lane of it for lg <= 4; lanes 16..31 / 48..63 for lg = 5; lane 63 for lg = 6).
__device__ __forceinline__ int group_sum_dpp(int v, const int lg) {
  if (lg >= 1) v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);       // quad_perm [1,0,3,2]
  if (lg >= 2) v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);       // quad_perm [2,3,0,1]
  if (lg >= 3) v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);      // row_half_mirror
  if (lg >= 4) v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);      // row_mirror
  if (lg >= 5) v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);     // row_bcast15 into rows 1 and 3
  if (lg >= 6) v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);     // row_bcast31 into rows 2 and 3
  return v;
}

template <int XMODE, bool GATE, bool W4, int NB>
__global__ void __launch_bounds__(DG_THREADS) decode_gemv_grouped_kernel(const mq_decode_gemv_grouped_args ga, const int rows_per_wg) {
  const mq_decode_gemv_batch_args& ba = ga.b;
  const mq_decode_gemv_args& g = ba.g;
  const int B = ba.batch;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [B][K] int8 activation images
  __shared__ float s_red[NB][DG_PRO], s_red2[NB][DG_PRO];
  __shared__ int s_redi[NB][DG_PRO];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int K = g.K;
  const float cv = g.consts[lane & 63];

  if (wave < DG_PRO) {
    // ================================================ PROLOGUE role ====================================================================
    gemv_batch_prologue<XMODE, NB>(ba, smem, s_red, s_red2, s_redi, cv, lane, wave);
    return;
  }

  // ================================================== STREAM role ======================================================================
  const int sw = wave - DG_PRO;
  const int NL = GATE ? g.N >> 1 : g.N;                            // logical rows
  const int kchunks = W4 ? K >> 5 : K >> 4;                        // 16-byte chunks per weight row
  const int wrow = W4 ? K >> 1 : K;                                // bytes per weight row
  const int lchunks = GATE ? 2 * kchunks : kchunks;                // chunks per logical row
  const int cpl = (lchunks + 63) >> 6;
  const int lg_cg = __builtin_ctz((unsigned)ga.group_size) - (W4 ? 5 : 4);     // chunks per group = 2^lg_cg (>= 2 chunks)
  const int lg_gl = lg_cg < 6 ? lg_cg : 6;                         // lanes per group within a pass
  const int pmask = (1 << (lg_cg > 6 ? lg_cg - 6 : 0)) - 1;        // passes per group - 1
  const int row0 = blockIdx.x * rows_per_wg + sw;
  const int row_end = (blockIdx.x + 1) * rows_per_wg < NL ? (blockIdx.x + 1) * rows_per_wg : NL;
  const int prow = row0 + DG_STR * lane;                           // lane t keeps the parameters / results of row slot t
  const bool prow_ok = prow < row_end;
  constexpr int DGR_INFLIGHT = dgr_inflight<NB>();
  v4i buf[DGR_INFLIGHT];
  int q_cw[DGR_INFLIGHT], q_t[DGR_INFLIGHT];
  float q_al[DGR_INFLIGHT];
  auto issue_pass = [&](int t, int j) {
#pragma unroll
    for (int u = 0; u < DGR_INFLIGHT; ++u) {
      const int row = row0 + DG_STR * t;
      const int c = lane + 64 * j;
      if (row < row_end && c < lchunks) {
        buf[u] = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(g.w + (size_t)row * (GATE ? 2 : 1) * wrow) + c);
        const bool second = GATE && c >= kchunks;
        const size_t vi = (size_t)((second ? c - kchunks : c) >> lg_cg) * g.N + (GATE ? 2 * row + (second ? 1 : 0) : row);
        q_cw[u] = ga.cw[vi];
        q_t[u] = ga.t[vi];
        q_al[u] = ga.alpha[vi];
      } else {
        buf[u] = v4i{0, 0, 0, 0};
        q_cw[u] = q_t[u] = 0;
        q_al[u] = 0.f;
      }
      if (++j == cpl) { j = 0; ++t; }
    }
  };
  issue_pass(0, 0);
  float p_bias[GATE ? 2 : 1];
#pragma unroll
  for (int h = 0; h < (GATE ? 2 : 1); ++h) p_bias[h] = (prow_ok && g.bias) ? g.bias[GATE ? 2 * prow + h : prow] : 0.f;
  float p_res[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) p_res[b] = (!GATE && g.resid && prow_ok && b < B) ? g.resid[(size_t)b * ba.y_stride + prow] : 0.f;
  gemv_batch_stream_barriers<XMODE>();
  if (row0 >= row_end) return;
  const GemvBatchEpilogue ep(cv, g);

  // ---- per chunk: P + cw A of the lane's piece; per pass: the groups' exact brackets, folded in ascending g ------------------------
  const int nslots = (row_end - row0 + DG_STR - 1) / DG_STR;
  const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
  int part[NB];
  float f0[NB], f1[NB], r0[NB], r1[NB];                            // wave-uniform fold (w1 | w3 halves), row slot results per lane
#pragma unroll
  for (int b = 0; b < NB; ++b) part[b] = 0, f0[b] = f1[b] = r0[b] = r1[b] = 0.f;
  int t = 0, j = 0;
  while (t < nslots) {
    int t2 = t, j2 = j;
#pragma unroll
    for (int u = 0; u < DGR_INFLIGHT; ++u) {
      if (t2 < nslots) {
        int c = lane + 64 * j2;
        c = c < lchunks ? c : lchunks - 1;                         // buf[u] is zero there; its (whole) groups are never folded
        const int ck = GATE ? (c >= kchunks ? c - kchunks : c) : c;
        v4i w_lo = buf[u], w_hi = buf[u];
        if constexpr (W4) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            w_lo[e] = buf[u][e] & 0x0f0f0f0f;
            w_hi[e] = (int)(((unsigned)buf[u][e] >> 4) & 0x0f0f0f0fu);
          }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if (b < B) {
            const char* img = smem + (size_t)b * K;
            int pw, pa;
            if constexpr (W4) {
              const v4i a_lo = *reinterpret_cast<const v4i*>(img + (size_t)ck * 32), a_hi = *reinterpret_cast<const v4i*>(img + (size_t)ck * 32 + 16);
              pw = dot16(w_hi, a_hi, dot16(w_lo, a_lo, 0));
              pa = dot16(ones, a_hi, dot16(ones, a_lo, 0));
            } else {
              const v4i a = *reinterpret_cast<const v4i*>(img + (size_t)ck * 16);
              pw = dot16(w_lo, a, 0);
              pa = dot16(ones, a, 0);
            }
            // |cw| < 2^23 (the engine's fold check), |pa| <= 32 * 128: a 24-bit multiply; int32 wrap-around is exact mod 2^32 and the
            // bracket fits (the same check), so the reduction order does not matter
            part[b] += pw + __mul24(q_cw[u], pa);
          }
        }
        if ((j2 & pmask) == pmask) {                               // the groups of this pass end here
          const int nch = lchunks - 64 * j2 < 64 ? lchunks - 64 * j2 : 64;
          const int ngr = nch >> lg_gl;
          float brf[NB];
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            if (b < B) {
              brf[b] = (float)(group_sum_dpp(part[b], lg_gl) + q_t[u]);
              part[b] = 0;
            }
          }
          for (int gi = 0; gi < ngr; ++gi) {                       // wave-uniform: group gi's bracket and alpha sit in its last lane
            const int src = ((gi + 1) << lg_gl) - 1;
            const float al = readlane_f(q_al[u], src);
            const bool second = GATE && 64 * j2 + (gi << lg_gl) >= kchunks;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
              if (b < B) {
                const float br = readlane_f(brf[b], src);
                if (second) f1[b] = __builtin_fmaf(br, al, f1[b]);
                else f0[b] = __builtin_fmaf(br, al, f0[b]);
              }
            }
          }
        }
        if (j2 == cpl - 1) {                                       // logical row slot t2 complete
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            if (lane == t2) {
              r0[b] = f0[b];
              r1[b] = f1[b];
            }
            f0[b] = f1[b] = 0.f;
          }
        }
        if (++j2 == cpl) { j2 = 0; ++t2; }
      }
    }
    t = t2;
    j = j2;
    if (t < nslots) issue_pass(t, j);
  }
  // ---- epilogue, one row per LANE, every batch row in turn: + bias (as mq_gemm_grouped.hip), then the batched launch's epilogue -------
  if (lane < nslots) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b < B) {
        const float e0 = g.bias ? __fadd_rn(r0[b], p_bias[0]) : r0[b];
        const float e1 = GATE ? (g.bias ? __fadd_rn(r1[b], p_bias[GATE ? 1 : 0]) : r1[b]) : 0.f;
        ep.store<GATE>(ba, b, prow, e0, e1, p_res[b]);
      }
    }
  }
}

}  // namespace mq

using namespace mq;

extern "C" {

int mq_decode_gemv_grouped(const mq_decode_gemv_grouped_args* args, mq_stream_t stream) {
  MQ_REQUIRE(args != nullptr, "mq_decode_gemv_grouped: null argument block");
  const mq_decode_gemv_batch_args& ba = args->b;
  const mq_decode_gemv_args& g = ba.g;
  const int B = ba.batch, gs = args->group_size;
  MQ_REQUIRE(B >= 1 && B <= MQ_DECODE_MAX_BATCH, "mq_decode_gemv_grouped: batch=%d outside 1..%d", B, MQ_DECODE_MAX_BATCH);
  MQ_REQUIRE(args->alpha && args->cw && args->t, "mq_decode_gemv_grouped: null pointer");
  if (const int rc = check_gemv("mq_decode_gemv_grouped", g, B, ba.x_stride, ba.y_stride, ba.gate_stride, false)) return rc;
  MQ_REQUIRE(gs >= 64 && gs % 64 == 0 && g.K % gs == 0, "mq_decode_gemv_grouped: group_size=%d must be a multiple of 64 that divides K=%d", gs, g.K);
  if ((gs & (gs - 1)) != 0) {
    set_error("mq_decode_gemv_grouped: group_size=%d is not a power of two (a group must be whole lanes of a pass or whole passes)", gs);
    return MQ_EUNSUPPORTED;
  }
  MQ_REQUIRE((int64_t)B * g.K <= DB_MAX_IMAGE, "mq_decode_gemv_grouped: batch * K = %lld exceeds the %d bytes of int8 images the workgroup holds in LDS",
             (long long)B * g.K, DB_MAX_IMAGE);
  MQ_REQUIRE((int64_t)(g.K / gs) * g.N < (1ll << 31), "mq_decode_gemv_grouped: the [G, N] group vectors are too large");
  MQ_REQUIRE(!g.zero_acc && !g.o_acc, "mq_decode_gemv_grouped: zero_acc / o_acc (the four-launch chain) are not served by the grouped launch");
  MQ_REQUIRE(aligned(args->alpha, 16) && aligned(args->cw, 16) && aligned(args->t, 16),
             "mq_decode_gemv_grouped: pointers must be 16-byte aligned and x_stride a multiple of 16 covering K");
  const bool gate = g.gate_q != nullptr;
  int rows_per_wg;
  unsigned grid;
  gemv_row_geometry(gate ? g.N / 2 : g.N, &rows_per_wg, &grid);
  const size_t lds = (size_t)B * g.K;
  hipStream_t st = as_stream(stream);
  const int xmode = gemv_xmode(g);
  static std::atomic<size_t> lds_set[32][kMaxDevices];            // per instantiation: xmode (4) x gate (2) x w4 (2) x (B == 1) (2)
  std::atomic<size_t>* const lds_cache = lds_set[gemv_kernel_index(xmode, gate, g.w4) * 2 + (B == 1 ? 1 : 0)];
  return gemv_dispatch(xmode, gate, g.w4, [&](auto xm, auto gt, auto w4) -> int {
    constexpr int XM = decltype(xm)::value;
    constexpr bool GT = decltype(gt)::value, W4 = decltype(w4)::value;
    const auto kernel = B == 1 ? decode_gemv_grouped_kernel<XM, GT, W4, 1> : decode_gemv_grouped_kernel<XM, GT, W4, DB_MAXB>;
    if (const int rc = set_lds(reinterpret_cast<const void*>(kernel), lds_cache, lds, "mq_decode_gemv_grouped")) return rc;
    kernel<<<grid, DG_THREADS, lds, st>>>(*args, rows_per_wg);
    MQ_LAUNCH_CHECK("mq_decode_gemv_grouped");
    return MQ_OK;
  });
}

}  // extern "C"
