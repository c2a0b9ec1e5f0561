// GPTQ error-compensated rounding of a weight onto a FIXED per-(row, group) grid (tests/gptq_ref.py restates it).
//
// What mq_gptq_round computes, for every row n of w [N, K] independently, in fp32 with round-to-nearest:
//   for t = 0 .. K-1:   k = perm[t] (identity without perm), g = k / group_size
//     q   = clamp(round_ste(w[k] / s[g]) + o[g], qmin, qmax)   index_value_keepnan with the IEEE divide (what mq_quantize takes)
//     dq  = dequant(q, s[g], o[g])                              (q - o) * s
//     e   = __fdiv_rn(__fsub_rn(w[k], dq), u[t][t])
//     loss += (double)e * (double)e                             ascending t
//     for every t' > t:   w[perm[t']] = fmaf(-e, u[t][t'], w[perm[t']])
// Every element receives its updates as ONE fmaf each, in ascending t: how the work is blocked below changes no bit of the result.
// A NaN weight stores qmin (to_storage_nan2qmin) and poisons the later columns of its own row only.
//
// Structure.  Three stages (six launches) on the caller's stream, no host synchronisation:
//   1. transposes: w -> the working copy wT [K, Npad] (ORIGINAL column order, Npad = N rounded up to 64), scale / offset -> [G, Npad]:
//      a wave's access to one column of 64 rows is one coalesced request, and perm only picks which column a step takes
//   2. gptq_kernel: a workgroup of GPTQ_WAVES waves owns a strip of GPTQ_STRIP = 64 rows, ONE LANE PER ROW, and walks all K steps:
//        chain     wave 0 holds a block of GPTQ_BLOCK walk-order columns in registers and runs their quantize-and-update chain; the
//                  block's dq and q go back into wT / qT (the column is final), its e values go to LDS
//        trailing  every wave takes chunks of GPTQ_CHUNK = 16 later walk positions (chunk c: wave c % GPTQ_WAVES) and applies the block's
//                  GPTQ_BLOCK updates to them in ascending t, from the e values in registers
//      u[t][t'] is the same for every lane.  The trailing update keeps the chunk's 16 entries of each of the block's 32 rows of u in ONE
//      VGPR a row (lane l: entry l & 15, a 64-byte load) and the v_fmac reads its entry through DPP row_newbcast: no SGPR, no
//      broadcast instruction, and the loads of the next chunk are in flight while this one computes (scalar loads of u cannot run
//      that far ahead: 128 SGPRs a chunk of 4 columns; measured in DESIGN.md 4.10).  The chain's
//      triangle of u is staged in LDS by the whole workgroup while the previous trailing update runs, and read as a broadcast; perm[t]
//      comes through the constant address space as a scalar load.
//   3. transposes back: wT (now dq) -> w_deq [N, K], qT -> index [N, K]
#include "mq_common.h"

#pragma clang fp contract(off)

namespace mq {

constexpr int GPTQ_STRIP = 64;           // rows of a workgroup: one lane each
constexpr int GPTQ_BLOCK = 32;           // walk-order columns of the in-register chain
constexpr int GPTQ_WAVES = 8;            // waves of a workgroup
constexpr int GPTQ_CHUNK = 16;           // trailing walk positions a wave updates together: 64 bytes of a row of u, one entry per lane of a DPP row
constexpr int GPTQ_TILE = 64;            // the transposes' tile
static_assert(GPTQ_CHUNK == 16, "a chunk's entries of one row of u sit in the 16 lanes of a DPP row");

typedef const int __attribute__((address_space(4))) gptq_ci;       // perm behind the constant address space (see gptq_kernel)

// src [rows, cols] row-major -> dst [cols, ld] (dst[c * ld + r]); rows beyond `rows` up to the tile's end are written as `pad`
template <typename T>
__global__ void __launch_bounds__(256) gptq_transpose_in_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t rows, int cols, int64_t ld, T pad) {
  __shared__ T tile[GPTQ_TILE][GPTQ_TILE + 1];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * GPTQ_TILE;
  const int c0 = blockIdx.y * GPTQ_TILE;
  for (int r = ty; r < GPTQ_TILE; r += 4) {
    const int64_t row = r0 + r;
    const int col = c0 + tx;
    tile[r][tx] = (row < rows && col < cols) ? src[row * cols + col] : pad;
  }
  __syncthreads();
  for (int c = ty; c < GPTQ_TILE; c += 4) {
    const int col = c0 + c;
    if (col < cols) dst[(int64_t)col * ld + r0 + tx] = tile[tx][c];          // r0 + tx < ld: ld is a multiple of the tile
  }
}

// src [cols, ld] (src[c * ld + r]) -> dst [rows, cols] row-major
template <typename T>
__global__ void __launch_bounds__(256) gptq_transpose_out_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t rows, int cols, int64_t ld) {
  __shared__ T tile[GPTQ_TILE][GPTQ_TILE + 1];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * GPTQ_TILE;
  const int c0 = blockIdx.y * GPTQ_TILE;
  for (int c = ty; c < GPTQ_TILE; c += 4) {
    const int col = c0 + c;
    if (col < cols) tile[c][tx] = src[(int64_t)col * ld + r0 + tx];
  }
  __syncthreads();
  for (int r = ty; r < GPTQ_TILE; r += 4) {
    const int64_t row = r0 + r;
    const int col = c0 + tx;
    if (row < rows && col < cols) dst[row * cols + col] = tile[tx][r];
  }
}

// the original column of walk step t: perm's entry, held inside [0, K) (the contents of perm are the caller's duty; a bad entry must
// not become an address outside the working copy)
template <bool PERM>
__device__ __forceinline__ int gptq_col(const gptq_ci* perm, int t, int K) {
  if (!PERM) return t;
  return min(max(perm[t], 0), K - 1);
}
// k / group_size for 0 <= k < 2^14 and 4 <= group_size <= 2^14 without a division: magic = 2^32 / group_size + 1 (the host forms it),
// and k * magic / 2^32 = k / group_size + k * r / (group_size * 2^32) with 0 < r <= group_size, an excess below 2^-4 / group_size
__device__ __forceinline__ int gptq_group(int k, unsigned magic) { return (int)__umulhi((unsigned)k, magic); }

// The block's own square of u, rows and columns [t0, t0 + GPTQ_BLOCK), staged in LDS by the whole workgroup (two entries a thread): the
// chain reads its triangle from there, every lane the same address (a broadcast read).  Past the end of a short last block the last
// row / column stands in: those entries feed only the steps that store nothing.
__device__ __forceinline__ void gptq_stage_u(float (*s_u)[GPTQ_BLOCK], const float* __restrict__ u, int t0, int K) {
  static_assert(GPTQ_WAVES * 64 * 2 == GPTQ_BLOCK * GPTQ_BLOCK, "two entries of the block's square per thread");
  const int r = threadIdx.x >> 4, c = (threadIdx.x & 15) * 2;
  const float* row = u + (int64_t)min(t0 + r, K - 1) * K;
  s_u[r][c] = row[min(t0 + c, K - 1)];
  s_u[r][c + 1] = row[min(t0 + c + 1, K - 1)];
}

// The chain of one block on the strip's wave 0: GPTQ_BLOCK walk-order columns from step t0 on, held in registers.  FULL: all of them
// exist.  Otherwise (a short last block of nb columns) the steps past the end run on the last column's values and store nothing: a
// step only ever updates LATER columns, so what they compute reaches no real column.
// wstrip / qstrip / sstrip / ostrip: the strip's first row in the transposed buffers (uniform), indexed by the lane.
template <bool FULL, bool PERM>
__device__ __forceinline__ void gptq_chain(float* __restrict__ wstrip, uint8_t* __restrict__ qstrip, const float* __restrict__ sstrip,
                                           const float* __restrict__ ostrip, const gptq_ci* perm, const float (*s_u)[GPTQ_BLOCK],
                                           float (*s_e)[GPTQ_STRIP], unsigned lane, int t0, int nb, int K, unsigned magic, unsigned npad,
                                           float qmin, float qmax, double& loss) {
  const int shift = (int)qmin;
  float w[GPTQ_BLOCK], s[GPTQ_BLOCK], o[GPTQ_BLOCK];
#pragma unroll
  for (int i = 0; i < GPTQ_BLOCK; ++i) {
    const int k = gptq_col<PERM>(perm, FULL ? t0 + i : min(t0 + i, K - 1), K);
    const int g = gptq_group(k, magic);
    w[i] = wstrip[(unsigned)k * npad + lane];          // K * npad < 2^31 (the host checks): 32-bit element offsets
    s[i] = sstrip[(unsigned)g * npad + lane];
    o[i] = ostrip[(unsigned)g * npad + lane];
  }
  // row i + 1 of the square is requested while step i runs and no further ahead (the scheduling barrier): all 496 entries at once
  // would not fit the register file beside the block
  float ur[GPTQ_BLOCK];
#pragma unroll
  for (int j = 0; j < GPTQ_BLOCK; ++j) ur[j] = s_u[0][j];
#pragma unroll
  for (int i = 0; i < GPTQ_BLOCK; ++i) {
    float un[GPTQ_BLOCK];
    if (i + 1 < GPTQ_BLOCK) {
#pragma unroll
      for (int j = i + 1; j < GPTQ_BLOCK; ++j) un[j] = s_u[i + 1][j];
    }
    const float q = index_value_keepnan(w[i], s[i], 0.0f, o[i], qmin, qmax, false);
    const float dq = dequant(q, s[i], o[i]);
    const float e = __fdiv_rn(__fsub_rn(w[i], dq), ur[i]);
    if (FULL || i < nb) {
      const unsigned at = (unsigned)gptq_col<PERM>(perm, t0 + i, K) * npad + lane;
      loss += (double)e * (double)e;
      wstrip[at] = dq;
      qstrip[at] = (uint8_t)to_storage_nan2qmin(q, qmin, shift);
    }
    s_e[i][lane] = e;
    const float ne = -e;
#pragma unroll
    for (int j = i + 1; j < GPTQ_BLOCK; ++j) {
      w[j] = __builtin_fmaf(ne, ur[j], w[j]);
      // the update happens HERE: left alone the compiler sinks every column's updates to the step that quantizes it, which keeps all
      // e values and the whole triangle of u live (spills) -- the same bits either way
      asm volatile("" : "+v"(w[j]));
    }
#pragma unroll
    for (int j = i + 1; j < GPTQ_BLOCK; ++j) ur[j] = un[j];
    __builtin_amdgcn_sched_barrier(0);
  }
}

// GPTQ_CHUNK trailing columns of one lane's row with where they live, and the chunk's entries of the block's GPTQ_BLOCK rows of u: lane l
// holds u[t0 + i][c + (l & 15)] in uv[i], so every DPP row of 16 lanes holds the chunk's 16 entries of row i.  Walk positions past K
// (a last chunk of 4, 8 or 12 columns) stand for the last column: computed, never stored.
struct GptqChunk {
  float x[GPTQ_CHUNK];
  unsigned at[GPTQ_CHUNK];
  float uv[GPTQ_BLOCK];
};
template <bool PERM>
__device__ __forceinline__ void gptq_chunk_load(GptqChunk& ch, const float* __restrict__ wstrip, const float* __restrict__ u, const gptq_ci* perm,
                                                int t0, int c, int K, unsigned npad, unsigned lane) {
#pragma unroll
  for (int j = 0; j < GPTQ_CHUNK; ++j) {
    ch.at[j] = (unsigned)gptq_col<PERM>(perm, min(c + j, K - 1), K) * npad + lane;
    ch.x[j] = wstrip[ch.at[j]];
  }
  const unsigned off = (unsigned)min((int)(lane & 15), K - 1 - c);
#pragma unroll
  for (int i = 0; i < GPTQ_BLOCK; ++i) ch.uv[i] = (u + (int64_t)(t0 + i) * K + c)[off];
}
// x[j] = fmaf(uv of the row's lane j, ne, x[j]) for the chunk's 16 columns: v_fmac_f32 (a fused multiply-add, one rounding) takes its
// first factor through DPP row_newbcast:j, so the wave-uniform u[t][c + j] costs neither an SGPR nor an instruction of its own.  Every
// lane is active here.  (s_nop 1: a VALU write of uv -- a register copy -- needs two wait states before a DPP read, and the
// compiler does not look into the statement.)
__device__ __forceinline__ void gptq_fmac16(float (&x)[GPTQ_CHUNK], float uv, float ne) {
#define MQ_GPTQ_F(j) "v_fmac_f32_dpp %" #j ", %16, %17 row_newbcast:" #j " row_mask:0xf bank_mask:0xf\n\t"
  asm("s_nop 1\n\t" MQ_GPTQ_F(0) MQ_GPTQ_F(1) MQ_GPTQ_F(2) MQ_GPTQ_F(3) MQ_GPTQ_F(4) MQ_GPTQ_F(5) MQ_GPTQ_F(6) MQ_GPTQ_F(7) MQ_GPTQ_F(8)
          MQ_GPTQ_F(9) MQ_GPTQ_F(10) MQ_GPTQ_F(11) MQ_GPTQ_F(12) MQ_GPTQ_F(13) MQ_GPTQ_F(14) MQ_GPTQ_F(15)
      : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]), "+v"(x[8]), "+v"(x[9]), "+v"(x[10]),
        "+v"(x[11]), "+v"(x[12]), "+v"(x[13]), "+v"(x[14]), "+v"(x[15])
      : "v"(uv), "v"(ne));
#undef MQ_GPTQ_F
}

template <bool PERM>
__global__ void __launch_bounds__(GPTQ_WAVES * 64)
gptq_kernel(float* __restrict__ wT, uint8_t* __restrict__ qT, const float* __restrict__ sT, const float* __restrict__ oT,
            const float* __restrict__ u, const int* __restrict__ perm_g, double* __restrict__ loss_out, int64_t N, int K, unsigned magic,
            unsigned npad, float qmin, float qmax) {
  __shared__ float s_e[GPTQ_BLOCK][GPTQ_STRIP];
  __shared__ float s_u[GPTQ_BLOCK][GPTQ_BLOCK];
  const unsigned lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t n0 = (int64_t)blockIdx.x * GPTQ_STRIP;               // n0 + lane < npad
  float* wstrip = wT + n0;
  // perm is never written while the kernel runs: read through the constant address space, a uniform address is a scalar load
  const gptq_ci* perm = (const gptq_ci*)perm_g;
  double loss = 0.0;
  gptq_stage_u(s_u, u, 0, K);
  __syncthreads();
  for (int t0 = 0; t0 < K; t0 += GPTQ_BLOCK) {
    const int nb = min(GPTQ_BLOCK, K - t0);
    if (wave == 0) {
      if (nb == GPTQ_BLOCK) gptq_chain<true, PERM>(wstrip, qT + n0, sT + n0, oT + n0, perm, s_u, s_e, lane, t0, nb, K, magic, npad, qmin, qmax, loss);
      else gptq_chain<false, PERM>(wstrip, qT + n0, sT + n0, oT + n0, perm, s_u, s_e, lane, t0, nb, K, magic, npad, qmin, qmax, loss);
    }
    __syncthreads();
    // ---- trailing: the block's updates on every later walk position, a chunk of columns per wave --------------------------------------
    if (t0 + GPTQ_BLOCK < K) {                                        // (a short block is the last one: nb == GPTQ_BLOCK here)
      gptq_stage_u(s_u, u, t0 + GPTQ_BLOCK, K);                       // the next chain's square: this block's chain is behind the barrier
      float ne[GPTQ_BLOCK];
#pragma unroll
      for (int i = 0; i < GPTQ_BLOCK; ++i) ne[i] = -s_e[i][lane];
      constexpr int STEP = GPTQ_WAVES * GPTQ_CHUNK;
      int c = t0 + GPTQ_BLOCK + wave * GPTQ_CHUNK;
      GptqChunk cur, nxt;
      if (c < K) gptq_chunk_load<PERM>(cur, wstrip, u, perm, t0, c, K, npad, lane);
      for (; c < K; c += STEP) {
        if (c + STEP < K) gptq_chunk_load<PERM>(nxt, wstrip, u, perm, t0, c + STEP, K, npad, lane);   // the next chunk, a trip ahead
#pragma unroll
        for (int i = 0; i < GPTQ_BLOCK; ++i) gptq_fmac16(cur.x, cur.uv[i], ne[i]);
#pragma unroll
        for (int j = 0; j < GPTQ_CHUNK; ++j)
          if (c + j < K) wstrip[cur.at[j]] = cur.x[j];
        cur = nxt;
      }
    }
    __syncthreads();                                                  // the next chain reads what the other waves wrote; s_e is free again
  }
  if (wave == 0 && loss_out && n0 + lane < N) loss_out[n0 + lane] = loss;
}

static inline int64_t gptq_npad(int64_t N) { return (N + GPTQ_STRIP - 1) / GPTQ_STRIP * GPTQ_STRIP; }
static inline size_t gptq_up256(size_t b) { return (b + 255) / 256 * 256; }

// the workspace: wT fp32 [K, Npad] | sT fp32 [G, Npad] | oT fp32 [G, Npad] | qT u8 [K, Npad], each from a 256-byte boundary
struct GptqWorkspace {
  size_t w, s, o, q, total;
};
static inline GptqWorkspace gptq_workspace(int64_t N, int64_t K, int64_t G) {
  const size_t npad = (size_t)gptq_npad(N);
  GptqWorkspace ws;
  ws.w = 0;
  ws.s = ws.w + gptq_up256((size_t)K * npad * 4);
  ws.o = ws.s + gptq_up256((size_t)G * npad * 4);
  ws.q = ws.o + gptq_up256((size_t)G * npad * 4);
  ws.total = ws.q + gptq_up256((size_t)K * npad);
  return ws;
}

}  // namespace mq

using namespace mq;

// Sized for the finest grid the entry serves (group_size 4: G = K / 4), so that the size depends on the shape alone.
extern "C" int64_t mq_gptq_workspace_bytes(int64_t N, int64_t K) {
  if (N < 0 || N >= (int64_t)0x7fffffff || K < 16 || K > 16384 || K % 4 != 0 || K * gptq_npad(N) >= (int64_t)0x7fffffff) return -1;
  if (N == 0) return 0;
  return (int64_t)gptq_workspace(N, K, K / 4).total;
}

extern "C" int mq_gptq_round(const mq_gptq_args* args, mq_stream_t stream) {
  MQ_REQUIRE(args, "mq_gptq_round: null argument block");
  const mq_gptq_args& a = *args;
  MQ_REQUIRE(a.N >= 0 && a.N < (int64_t)0x7fffffff, "mq_gptq_round: bad row count %lld", (long long)a.N);
  MQ_REQUIRE(a.K % 4 == 0 && a.K >= 16 && a.K <= 16384, "mq_gptq_round: rows of 16 to 16384 columns, a multiple of 4 (K=%lld)", (long long)a.K);
  MQ_REQUIRE(a.group_size >= 4 && a.group_size % 4 == 0 && a.K % a.group_size == 0,
             "mq_gptq_round: group_size must be a multiple of 4 that divides K=%lld (group_size=%lld)", (long long)a.K, (long long)a.group_size);
  MQ_REQUIRE(a.qmin == (float)(int)a.qmin && a.qmax == (float)(int)a.qmax && a.qmax > a.qmin && a.qmax - a.qmin <= 255.0f,
             "mq_gptq_round: integer qmin < qmax with qmax - qmin <= 255, the range of the uint8 index (got %g, %g)", (double)a.qmin, (double)a.qmax);
  MQ_REQUIRE(!(a.perm && !a.u), "mq_gptq_round: perm given without u");
  MQ_REQUIRE(a.K * ((a.N + 63) / 64 * 64) < (int64_t)0x7fffffff, "mq_gptq_round: K times N rounded up to 64 must stay below 2^31 (N=%lld, K=%lld)",
             (long long)a.N, (long long)a.K);
  if (a.N == 0) return MQ_OK;
  MQ_REQUIRE(a.w && a.scale && a.offset && a.u && a.index && a.workspace, "mq_gptq_round: null pointer (w, scale, offset, u, index, workspace)");
  MQ_REQUIRE(aligned(a.w, 16) && aligned(a.scale, 16) && aligned(a.offset, 16) && aligned(a.u, 16) && aligned(a.perm, 16) && aligned(a.index, 16) &&
                 aligned(a.w_deq, 16) && aligned(a.loss, 16) && aligned(a.workspace, 16),
             "mq_gptq_round: every pointer must be 16-byte aligned");
  const int64_t G = a.K / a.group_size;
  const GptqWorkspace ws = gptq_workspace(a.N, a.K, G);
  MQ_REQUIRE(a.workspace_bytes >= (int64_t)ws.total, "mq_gptq_round: workspace of %lld bytes, mq_gptq_workspace_bytes asks for %lld",
             (long long)a.workspace_bytes, (long long)mq_gptq_workspace_bytes(a.N, a.K));
  char* base = static_cast<char*>(a.workspace);
  float* wT = reinterpret_cast<float*>(base + ws.w);
  float* sT = reinterpret_cast<float*>(base + ws.s);
  float* oT = reinterpret_cast<float*>(base + ws.o);
  uint8_t* qT = reinterpret_cast<uint8_t*>(base + ws.q);
  const int64_t npad = gptq_npad(a.N);
  const unsigned strips = (unsigned)(npad / GPTQ_STRIP);
  const int K = (int)a.K;
  hipStream_t st = as_stream(stream);
  const dim3 tk(strips, (unsigned)((K + GPTQ_TILE - 1) / GPTQ_TILE)), tg(strips, (unsigned)((G + GPTQ_TILE - 1) / GPTQ_TILE));
  gptq_transpose_in_kernel<float><<<tk, 256, 0, st>>>(a.w, wT, a.N, K, npad, 0.0f);
  gptq_transpose_in_kernel<float><<<tg, 256, 0, st>>>(a.scale, sT, a.N, (int)G, npad, 1.0f);
  gptq_transpose_in_kernel<float><<<tg, 256, 0, st>>>(a.offset, oT, a.N, (int)G, npad, 0.0f);
  const unsigned magic = (unsigned)((1ull << 32) / (unsigned long long)a.group_size + 1);
  if (a.perm) gptq_kernel<true><<<strips, GPTQ_WAVES * 64, 0, st>>>(wT, qT, sT, oT, a.u, a.perm, a.loss, a.N, K, magic, (unsigned)npad, a.qmin, a.qmax);
  else gptq_kernel<false><<<strips, GPTQ_WAVES * 64, 0, st>>>(wT, qT, sT, oT, a.u, a.perm, a.loss, a.N, K, magic, (unsigned)npad, a.qmin, a.qmax);
  gptq_transpose_out_kernel<uint8_t><<<tk, 256, 0, st>>>(qT, a.index, a.N, K, npad);
  if (a.w_deq) gptq_transpose_out_kernel<float><<<tk, 256, 0, st>>>(wT, a.w_deq, a.N, K, npad);
  MQ_LAUNCH_CHECK("mq_gptq_round");
  return MQ_OK;
}
