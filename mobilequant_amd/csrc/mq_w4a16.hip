// W4A16: fp16 activations times packed 4-bit group-wise weights (the reference reaches auto_gptq's QuantLinear for this,
// qmodule.py:803-829).  One entry, mq_w4a16_linear, two kernels.
//
// Contract (every layer above follows it): for row n, group G = k / group_size,
//   w16[n, k] = fp16_rne(float(s16[n, G]) * float(u[n, k] - z'[n, G]))     u = the stored nibble 0..15, z' = the stored zero, an integer
//                                                                           with |z'| <= 1024 held as fp16: u - z' is exact in fp16, the
//                                                                           product has ONE rounding (a packed fp16 multiply here)
//   x16[m, k] = fp16_rne(x[m, k])                                           (fp16 x: as is)
//   y[m, n]   = out_dtype(sum_k x16[m, k] * w16[n, k] + bias[n])            exact products, fp32 accumulation in the kernel's order, the
//                                                                           fp32 bias added in fp32, one final rounding
// No fp16 accumulation anywhere.
//
// Both kernels read the mq_pack_w4 image [N, K / 2]: byte j (0..15) of a 16-byte group holds element j (low nibble) and j + 16 (high
// nibble) of a 32-wide k block.  A dword d of the group (bytes B0 .. B0 + 3, B0 = 4 i) splits into four fp16 PAIRS with a shift, an and
// and an or each -- ((d >> 4 t) & 0x000f000f) | 0x64006400 is (1024 + u_a, 1024 + u_b) -- in the k order
//   B0, B0 + 2 | 16 + B0, 16 + B0 + 2 | B0 + 1, B0 + 3 | 16 + B0 + 1, 16 + B0 + 3                                    ("unit order")
// and the activations are laid out in LDS in that same order (quad_slot), so neither side moves a byte to line the two up.
// (1024 + u) - (1024 + z') is exact (integers below 2049), the multiply by s16 rounds once.
//
// M <= 8: weight-streaming GEMV.  The walk is mq_w4a16_stream.h's (w4_stream_walk, described there): here it runs over M <= MT row images of
// x16, staged once per workgroup, with the packed 16-bit fetch of s16 / z' (scales and zeros 2-byte aligned: the entry's contract), and a
// completed row gets its fp32 bias and one store per activation row.
// M > 8 (and M <= 8 rows too long for the staging buffer): MFMA GEMM, 64 rows x 64 NT columns of outputs per 256-thread workgroup (NT = 2;
// 1 when N <= 64), k in chunks of 128.  Wave w owns NT tiles of 16 weight rows (n0 + 16 NT w ..) and all 64 activation rows: its packed
// weights go global -> registers (nobody else needs them), lane (n = lane & 15, kq = lane >> 4) holding the 16-byte group kq of the chunk
// for each tile; dword s of it is the A fragment of
// k-step s (v_mfma_f32_16x16x32_f16: A[row = lane & 15][k = 8 (lane >> 4) + j]).  The step therefore sums k = 32 kq + {unit order of
// dword s}, kq = 0..3 -- a permutation of the chunk's k, the same on both operands.  x16 goes through a double-buffered LDS tile
// [64][128] fp16 in unit order (row pitch 272 B), B fragment = one ds_read_b128.  With the weights as A the accumulator holds
// out[m = lane & 15][n = 4 (lane >> 4) + reg]: four consecutive n per lane, one 16-byte (fp32) or 8-byte (fp16) store.
#include "mq_w4a16_stream.h"

namespace mq {

struct W4A16Args {
  const void* x;
  int x_f16;
  int M;
  W4Image g;
  const float* bias;
  void* out;
  int out_f16;
};

// Four consecutive activations x[k .. k + 3] (k % 4 == 0) as the two dwords of the unit order: (j0, j2) and (j1, j3).
template <typename XT>
__device__ __forceinline__ void load_quad(const void* x, size_t idx, float (&v)[4]);
template <>
__device__ __forceinline__ void load_quad<float>(const void* x, size_t idx, float (&v)[4]) {
  const float4 f = *reinterpret_cast<const float4*>(static_cast<const float*>(x) + idx);
  v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
}
template <>
__device__ __forceinline__ void load_quad<__half>(const void* x, size_t idx, float (&v)[4]) {
  const uint2 u = *reinterpret_cast<const uint2*>(static_cast<const __half*>(x) + idx);
  v[0] = __half2float(__ushort_as_half((unsigned short)(u.x & 0xffff)));
  v[1] = __half2float(__ushort_as_half((unsigned short)(u.x >> 16)));
  v[2] = __half2float(__ushort_as_half((unsigned short)(u.y & 0xffff)));
  v[3] = __half2float(__ushort_as_half((unsigned short)(u.y >> 16)));
}
// ---- M <= 8 -------------------------------------------------------------------------------------------------------------------------
constexpr int WV_THREADS = 1024, WV_WAVES = 16;
constexpr size_t WV_MAX_LDS = 128 * 1024;

template <int MT>
__global__ void __launch_bounds__(WV_THREADS) w4a16_gemv_kernel(const W4A16Args a, const int rows_per_wg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];     // [M][K] fp16, unit order
  // chunks in flight per lane: eight, four with eight rows of accumulators (the unrolled body is MT x 32 fmas per chunk)
  constexpr int WV_INFLIGHT = MT == 8 ? 4 : 8;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int K = a.g.K, N = a.g.N, M = a.M;
  const int row0 = blockIdx.x * rows_per_wg + wave;
  const int row_end = (blockIdx.x + 1) * rows_per_wg < N ? (blockIdx.x + 1) * rows_per_wg : N;
  const int nslots = (row_end - row0 + WV_WAVES - 1) / WV_WAVES;  // (row_end - row0 > -WV_WAVES: a wave past the rows has none)
  auto slot_row = [&](int t) { return row0 + WV_WAVES * t; };
  float p_bias = 0.f;                                             // lane t keeps the bias of row slot t

  w4_stream_walk<WV_INFLIGHT, false, MT>(
      a.g, nslots, slot_row,
      [&] {                                                       // behind the first requests: activations -> LDS as fp16, once per workgroup
        if (a.bias && lane < nslots) p_bias = a.bias[slot_row(lane)];
        const int qpr = K >> 2;                                   // quads per row
        for (int i = threadIdx.x; i < M * qpr; i += WV_THREADS) {
          const int m = i / qpr, kk = (i - m * qpr) << 2;
          float v[4];
          if (a.x_f16) load_quad<__half>(a.x, (size_t)m * K + kk, v);
          else load_quad<float>(a.x, (size_t)m * K + kk, v);
          stage_quad(smem + (size_t)m * K * 2, kk, v);
        }
        __syncthreads();
      },
      smem, M,
      [&](int t, const float (&sums)[MT]) {                       // a completed row: bias, one store per activation row
        const int row = slot_row(t);
        const float bias = readlane_f(p_bias, t);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          if (m < M && lane == 0) {
            const float f = __fadd_rn(sums[m], bias);
            const size_t idx = (size_t)m * N + row;
            if (a.out_f16) reinterpret_cast<__half*>(a.out)[idx] = __float2half_rn(f);
            else reinterpret_cast<float*>(a.out)[idx] = f;
          }
        }
      });
}

// ---- M > 8 --------------------------------------------------------------------------------------------------------------------------
constexpr int GM_BM = 64, GM_BN = 64, GM_BK = 128, GM_THREADS = 256, GM_PITCH = 272;

// NT: 16-row weight tiles per wave (the workgroup covers 64 NT output columns): every B fragment read from LDS feeds NT MFMAs
template <typename XT, int NT>
__global__ void __launch_bounds__(GM_THREADS) w4a16_gemm_kernel(const W4A16Args a) {
  __shared__ __attribute__((aligned(16))) char s_x[2][GM_BM * GM_PITCH];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int M = a.M, N = a.g.N, K = a.g.K;
  const int m0 = blockIdx.x * GM_BM;
  const int n0 = blockIdx.y * (GM_BN * NT) + 16 * NT * wave;      // tile t of this wave: rows n0 + 16 t .. + 15
  const int ntiles = n0 >= N ? 0 : (N - n0) / 16 < NT ? (N - n0) / 16 : NT;   // wave-uniform (N % 16 == 0: a tile is all inside or all outside)
  const bool active = ntiles > 0;
  const int ln = lane & 15, kq = lane >> 4;
  const int G = K / a.g.gs;
  const int nchunks = (K + GM_BK - 1) / GM_BK;

  // staging: thread t owns quad qi = t & 31 (k = 4 qi of the chunk) of rows (t >> 5) + 8 i
  const int qi = threadIdx.x & 31, sr = threadIdx.x >> 5;
  const int st_off = (qi >> 3) * 64 + (qi & 3) * 16 + quad_slot((qi >> 2) & 1);
  float xr[8][4];
  auto load_x = [&](int chunk) {
    const int k = chunk * GM_BK + 4 * qi;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = m0 + sr + 8 * i;
      if (m < M && k < K) {
        load_quad<XT>(a.x, (size_t)m * K + k, xr[i]);
      } else {
        xr[i][0] = xr[i][1] = xr[i][2] = xr[i][3] = 0.f;
      }
    }
  };
  auto store_x = [&](int b) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      char* dst = s_x[b] + (sr + 8 * i) * GM_PITCH + st_off;
      *reinterpret_cast<unsigned*>(dst) = pack_h2(xr[i][0], xr[i][2]);
      *reinterpret_cast<unsigned*>(dst + 8) = pack_h2(xr[i][1], xr[i][3]);
    }
  };
  v4i wq[NT];
  unsigned wsz[NT];                                               // s16 | z' << 16 of the lane's group
  auto load_w = [&](int chunk, v4i (&q)[NT], unsigned (&sz)[NT]) {
    const int kb = chunk * (GM_BK / 32) + kq;                     // 32-wide k block of this lane
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t < ntiles && kb * 32 < K) {
        const int n = n0 + 16 * t + ln;
        q[t] = *(reinterpret_cast<const v4i*>(a.g.w + (size_t)n * (K >> 1)) + kb);
        const size_t gi = (size_t)n * G + a.g.group_of(kb);
        sz[t] = (unsigned)a.g.scales[gi] | ((unsigned)a.g.zeros[gi] << 16);
      } else {
        q[t] = v4i{0, 0, 0, 0};
        sz[t] = 0;
      }
    }
  };

  v4f acc[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[t][mt] = v4f{0.f, 0.f, 0.f, 0.f};

  load_x(0);
  load_w(0, wq, wsz);
  store_x(0);
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    v4i wq_n[NT];
    unsigned wsz_n[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      wq_n[t] = v4i{0, 0, 0, 0};
      wsz_n[t] = 0;
    }
    const bool more = c + 1 < nchunks;
    if (more) {
      load_x(c + 1);
      load_w(c + 1, wq_n, wsz_n);
    }
    if (active) {                                                  // (a tile past N multiplies zeros: its weights and scale are zero)
      const char* xb = s_x[c & 1] + ln * GM_PITCH + kq * 64;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        v8h wf[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          h2 w[4];
          dequant8((unsigned)wq[t][s], splat_scale((uint16_t)(wsz[t] & 0xffff)), splat_negzero((uint16_t)(wsz[t] >> 16)), w);
          wf[t] = v8h{w[0][0], w[0][1], w[1][0], w[1][1], w[2][0], w[2][1], w[3][0], w[3][1]};
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          const v8h xf = *reinterpret_cast<const v8h*>(xb + mt * 16 * GM_PITCH + s * 16);
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[t], xf, acc[t][mt], 0, 0, 0);
        }
      }
    }
    if (more) store_x((c + 1) & 1);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      wq[t] = wq_n[t];
      wsz[t] = wsz_n[t];
    }
  }

  // ---- epilogue: acc[t][mt][r] = out[m0 + 16 mt + ln][n0 + 16 t + 4 kq + r] -----------------------------------------------------------
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t < ntiles) {
      const int nb = n0 + 16 * t + 4 * kq;
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (a.bias) b = *reinterpret_cast<const float4*>(a.bias + nb);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int m = m0 + 16 * mt + ln;
        if (m < M) {
          const float f0 = __fadd_rn(acc[t][mt][0], b.x), f1 = __fadd_rn(acc[t][mt][1], b.y), f2 = __fadd_rn(acc[t][mt][2], b.z),
                      f3 = __fadd_rn(acc[t][mt][3], b.w);
          const size_t idx = (size_t)m * N + nb;
          if (a.out_f16) {
            *reinterpret_cast<uint2*>(reinterpret_cast<__half*>(a.out) + idx) = make_uint2(pack_h2(f0, f1), pack_h2(f2, f3));
          } else {
            *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.out) + idx) = make_float4(f0, f1, f2, f3);
          }
        }
      }
    }
  }
}

// 0: not served (why: the rule, for the message), 1: the GEMV, 2: the GEMM
static int w4a16_variant(int64_t M, int64_t N, int64_t K, int64_t gs, const char** why) {
  const char* w = nullptr;
  if (M < 1 || M > (1ll << 30)) w = "1 <= M <= 2^30";
  else if (N < 16 || N % 16 != 0) w = "N % 16 == 0";
  else if (N > 65535ll * GM_BN) w = "N <= 4194240";
  else if (K < 64 || K % 64 != 0) w = "K % 64 == 0";
  else if (K > (1ll << 24)) w = "K <= 2^24";
  else if (gs < 32 || gs % 32 != 0) w = "group_size must be a multiple of 32";
  else if (K % gs != 0) w = "group_size must divide K";
  if (why) *why = w;
  if (w) return 0;
  return (M <= 8 && (size_t)M * K * 2 <= WV_MAX_LDS) ? 1 : 2;
}

}  // namespace mq

using namespace mq;

extern "C" int mq_w4a16_supported(int64_t M, int64_t N, int64_t K, int64_t group_size) { return w4a16_variant(M, N, K, group_size, nullptr); }

extern "C" int mq_w4a16_linear(const mq_w4a16_args* p, mq_stream_t stream) {
  MQ_REQUIRE(p, "mq_w4a16_linear: null pointer (argument block)");
  MQ_REQUIRE(p->M >= 0, "mq_w4a16_linear: M=%lld must not be negative", (long long)p->M);
  if (p->M == 0) return MQ_OK;
  MQ_REQUIRE((p->x_dtype == MQ_F32 || p->x_dtype == MQ_F16) && (p->out_dtype == MQ_F32 || p->out_dtype == MQ_F16),
             "mq_w4a16_linear: x_dtype / out_dtype must be MQ_F32 or MQ_F16 (got %d / %d)", p->x_dtype, p->out_dtype);
  MQ_REQUIRE(p->x && p->w_packed && p->scales && p->zeros && p->out, "mq_w4a16_linear: null pointer (x, w_packed, scales, zeros, out)");
  MQ_REQUIRE(aligned(p->x, 16) && aligned(p->w_packed, 16) && aligned(p->out, 16) && aligned(p->scales, 2) && aligned(p->zeros, 2) &&
                 aligned(p->bias, 16),
             "mq_w4a16_linear: misaligned pointer (x, w_packed, out, bias: 16 bytes; scales, zeros: 2)");
  const char* why = nullptr;
  const int variant = w4a16_variant(p->M, p->N, p->K, p->group_size, &why);
  if (!variant) {
    set_error("mq_w4a16_linear: M=%lld N=%lld K=%lld group_size=%lld is not served (mq_w4a16_supported: %s)", (long long)p->M, (long long)p->N,
              (long long)p->K, (long long)p->group_size, why);
    return MQ_EUNSUPPORTED;
  }
  W4A16Args a;
  a.x = p->x;
  a.x_f16 = p->x_dtype == MQ_F16;
  a.M = (int)p->M;
  a.g = w4_image(p->w_packed, p->scales, p->zeros, p->N, p->K, p->group_size);
  a.bias = p->bias;
  a.out = p->out;
  a.out_f16 = p->out_dtype == MQ_F16;
  hipStream_t st = as_stream(stream);
  if (variant == 1) {
    // one fat workgroup per CU; a wave keeps at most 64 row slots (their bias lives one per lane)
    int rows_per_wg;
    unsigned grid;
    fat_row_geometry(a.g.N, WV_WAVES * 64, &rows_per_wg, &grid);
    const size_t lds = (size_t)a.M * a.g.K * 2;
    static std::atomic<size_t> lds_set[4][kMaxDevices];
    const int ki = a.M == 1 ? 0 : a.M == 2 ? 1 : a.M <= 4 ? 2 : 3;
    const void* fn = ki == 0 ? (const void*)w4a16_gemv_kernel<1> : ki == 1 ? (const void*)w4a16_gemv_kernel<2>
                   : ki == 2 ? (const void*)w4a16_gemv_kernel<4> : (const void*)w4a16_gemv_kernel<8>;
    if (const int rc = set_lds(fn, lds_set[ki], lds, "mq_w4a16_linear", WV_MAX_LDS)) return rc;
    switch (ki) {
      case 0: w4a16_gemv_kernel<1><<<grid, WV_THREADS, lds, st>>>(a, rows_per_wg); break;
      case 1: w4a16_gemv_kernel<2><<<grid, WV_THREADS, lds, st>>>(a, rows_per_wg); break;
      case 2: w4a16_gemv_kernel<4><<<grid, WV_THREADS, lds, st>>>(a, rows_per_wg); break;
      default: w4a16_gemv_kernel<8><<<grid, WV_THREADS, lds, st>>>(a, rows_per_wg); break;
    }
    MQ_LAUNCH_CHECK("mq_w4a16_linear(gemv)");
    return MQ_OK;
  }
  // 64 x 128 outputs per workgroup (two weight tiles per wave) once N has more than one 64-column block, 64 x 64 below
  const int nt = a.g.N > GM_BN ? 2 : 1;
  const dim3 grid((unsigned)((a.M + GM_BM - 1) / GM_BM), (unsigned)((a.g.N + GM_BN * nt - 1) / (GM_BN * nt)));
  if (nt == 2) {
    if (a.x_f16) w4a16_gemm_kernel<__half, 2><<<grid, GM_THREADS, 0, st>>>(a);
    else w4a16_gemm_kernel<float, 2><<<grid, GM_THREADS, 0, st>>>(a);
  } else {
    if (a.x_f16) w4a16_gemm_kernel<__half, 1><<<grid, GM_THREADS, 0, st>>>(a);
    else w4a16_gemm_kernel<float, 1><<<grid, GM_THREADS, 0, st>>>(a);
  }
  MQ_LAUNCH_CHECK("mq_w4a16_linear(gemm)");
  return MQ_OK;
}
