// Quantize-to-integer kernels of the inference path (HBM-bound): row-major indices (+ row sums), the fragment-blocked ("tiled")
// int8 image for the generated-ISA GEMM loop, GEMM epilogue-vector preparation, W4 packing -- and the library's process-wide entry
// points (version, error text, device info).
//
// Bit-exactness contract (DESIGN.md "Numerics"): the reference's fp32 expression tree op for op -- IEEE division (or the reciprocal
// form that equals it on the quantizer's domain, mq_common.h), round-half-even, separate add / clamp -- so the integer indices equal
// the reference CPU path's bit for bit.  STORAGE form of mq_quant.h (NaN -> qmin); the staged tiled kernel uses the IMAGE form.
#include <type_traits>

#include "mq_common.h"

#pragma clang fp contract(off)

namespace mq {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- quantize to integers, one workgroup per row, optional row sum ------------------------------
template <typename QT>
__device__ __forceinline__ QT to_store(float q, int shift) {
  return static_cast<QT>(static_cast<int>(q) - shift);
}

// CS: SmoothQuant per-channel scale fused in front of the quantizer: x[m,k] / chan_scale[k] (IEEE divide), then the index
// arithmetic op for op -- the run-time form of the reference's offline fold `ln.weight /= s; fc.weight *= s`
// (ptq/smoothquant.py:64-69, algorithm.py:47-68) for activations whose producer cannot absorb 1/s.
template <typename T, typename QT, bool PER_ROW, bool CS = false>
__global__ void __launch_bounds__(256) quantize_rows_kernel(const T* __restrict__ x, QT* __restrict__ q,
                                                            int64_t cols, const float* __restrict__ scale,
                                                            const float* __restrict__ offset, float qmin,
                                                            float qmax, int shift, int32_t* __restrict__ row_sum,
                                                            int vec_ok, const float* __restrict__ chan_scale = nullptr) {
  using V = Vec16<T>;
  const int64_t row = blockIdx.x;
  const float s = scale[PER_ROW ? row : 0];
  const float o = offset[PER_ROW ? row : 0];
  const float inv_s = __fdiv_rn(1.0f, s);
  const bool fast = scale_in_fast_range(s);
  const T* xr = x + row * cols;
  QT* qr = q + row * cols;
  int acc = 0;
  if (vec_ok) {
    const int64_t nvec = cols / V::N;
    const V* xv = reinterpret_cast<const V*>(xr);
    for (int64_t i = threadIdx.x; i < nvec; i += 256) {
      V a = xv[i];
      QT out[V::N];
#pragma unroll
      for (int j = 0; j < V::N; ++j) {
        float xv = V::get(a, j);
        if constexpr (CS) xv = __fdiv_rn(xv, chan_scale[i * V::N + j]);
        float qi = index_storage_nan2qmin(xv, s, inv_s, o, qmin, qmax, fast);
        int st_v = static_cast<int>(qi) - shift;
        acc += st_v;
        out[j] = static_cast<QT>(st_v);
      }
      // V::N elements of QT: 4 B (f32->i8) .. 16 B; a single naturally aligned store
      struct alignas(sizeof(QT) * V::N) Pack { QT e[V::N]; };
      Pack p;
#pragma unroll
      for (int j = 0; j < V::N; ++j) p.e[j] = out[j];
      reinterpret_cast<Pack*>(qr)[i] = p;
    }
  } else {
    for (int64_t i = threadIdx.x; i < cols; i += 256) {
      float xv = ld<T>(xr, i);
      if constexpr (CS) xv = __fdiv_rn(xv, chan_scale[i]);
      float qi = index_storage_nan2qmin(xv, s, inv_s, o, qmin, qmax, fast);
      int st_v = static_cast<int>(qi) - shift;
      acc += st_v;
      qr[i] = static_cast<QT>(st_v);
    }
  }
  if (row_sum != nullptr) {
    __shared__ int part[4];
    const int total = block_sum4(wave_sum(acc), part, (int)(threadIdx.x >> 6));
    if (threadIdx.x == 0) row_sum[row] = total;
  }
}

// fp32 -> 1-byte indices, wave-per-row: a lane converts 16 consecutive elements (four independent 16-byte
// loads in flight, one 16-byte store), so a wave instruction stores 1 KiB contiguous; the row sum is a
// wave reduction (no LDS, no barrier).  Needs cols % 16 == 0 and 16-byte aligned rows.
template <typename QT, bool PER_ROW, bool CS = false>
__global__ void __launch_bounds__(256) quantize_rows_f32_b16_kernel(const float* __restrict__ x, QT* __restrict__ q,
                                                                    int64_t rows, int64_t cols,
                                                                    const float* __restrict__ scale,
                                                                    const float* __restrict__ offset, float qmin,
                                                                    float qmax, int shift, int32_t* __restrict__ row_sum,
                                                                    const float* __restrict__ chan_scale = nullptr) {
  static_assert(sizeof(QT) == 1, "one byte per index");
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t row = wave0; row < rows; row += nwaves) {
    const float s = scale[PER_ROW ? row : 0];
    const float o = offset[PER_ROW ? row : 0];
    const float inv_s = __fdiv_rn(1.0f, s);
    const bool fast = scale_in_fast_range(s);
    const float* xr = x + row * cols;
    QT* qr = q + row * cols;
    int acc = 0;
    for (int64_t c = (int64_t)lane * 16; c < cols; c += 1024) {
      const float4* p = reinterpret_cast<const float4*>(xr + c);
      const float4 v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3];
      float f[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
      if constexpr (CS) {      // the [cols] vector is shared by every row: L2 / L1 resident after the first rows
        const float4* cp = reinterpret_cast<const float4*>(chan_scale + c);
        const float4 c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3];
        const float cs[16] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
#pragma unroll
        for (int e = 0; e < 16; ++e) f[e] = __fdiv_rn(f[e], cs[e]);
      }
      uint32_t w[4];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        uint32_t pk = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int st_v = static_cast<int>(index_storage_nan2qmin(f[d * 4 + e], s, inv_s, o, qmin, qmax, fast)) - shift;
          acc += st_v;
          pk |= (static_cast<uint32_t>(st_v) & 0xffu) << (8 * e);
        }
        w[d] = pk;
      }
      *reinterpret_cast<uint4*>(qr + c) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (row_sum != nullptr) {
      acc = wave_sum(acc);
      if (lane == 0) row_sum[row] = acc;
    }
  }
}

// ---- epilogue vectors of one QLinear ------------------------------------------------------------
__global__ void linear_epilogue_prepare_kernel(const float* __restrict__ a_scale, const float* __restrict__ a_offset,
                                               int a_shift, const float* __restrict__ w_scale,
                                               const float* __restrict__ w_offset, int per_row, int w_shift,
                                               const int32_t* __restrict__ w_colsum, int64_t N, int K,
                                               float* __restrict__ alpha, int32_t* __restrict__ w_zp,
                                               int32_t* __restrict__ col_term) {
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float sa = a_scale[0];
  const int za = static_cast<int>(a_offset[0]) - a_shift;
  const float sw = w_scale[per_row ? n : 0];
  const int zw = static_cast<int>(w_offset[per_row ? n : 0]) - w_shift;
  alpha[n] = __fmul_rn(sa, sw);
  w_zp[n] = zw;
  // two's-complement wrap-around is fine: the GEMM's final sum is exact when it fits int32
  col_term[n] = (int32_t)((uint32_t)(-za) * (uint32_t)w_colsum[n] + (uint32_t)K * (uint32_t)za * (uint32_t)zw);
}

// ---- W4 packing ---------------------------------------------------------------------------------
// out byte (n, kb*16 + j) = nib(n, kb*32 + j) | nib(n, kb*32 + 16 + j) << 4
__global__ void pack_w4_kernel(const uint8_t* __restrict__ nib, int64_t total_out, uint8_t* __restrict__ packed) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total_out) return;
  int64_t grp = i >> 4;      // 16-byte output group == 32-element input block
  int j = (int)(i & 15);
  const uint8_t* src = nib + grp * 32;
  packed[i] = (uint8_t)((src[j] & 15) | ((src[j + 16] & 15) << 4));
}

// ---- a5 -> int8, fragment-blocked ("tiled") output for the generated-ISA GEMM loop ------------------------------
// Layout: 1-KiB blocks of 16 rows x 64 k, ordered [row block][k block]; inside a block lane l = (row & 15) + 16 * ((k & 63) >> 4)
// owns the 16 bytes k & 15 -- the register image of a v_mfma_i32_16x16x64_i8 operand, so the GEMM loads one fragment
// with ONE fully coalesced global_load_dwordx4 (a row-major fragment is 16 rows x 64 B = 16 half cache lines: measured
// 4 us slower per launch).  A workgroup owns a row block: its 8 waves split the k blocks, every lane reads 64 B of
// fp32 per block (four float4; the four lanes of a row cover 256 contiguous bytes) and writes its 16 bytes; row sums
// of the stored values go through LDS atomics.  Same index arithmetic as quantize_rows_* (bit-exact indices).
// A workgroup owns 8 rows (half a row block: at M = 2048 that is 256 workgroups, one per CU; the conversion is
// ~20 VALU ops per element, so leaving half the CUs idle doubles the kernel).  A wave converts 8 rows x 2 k blocks per
// step: lane = r + 8 * kq + 32 * ksel reads the 64 bytes (16 fp32) of row r, k block kb0 + ksel, quarter kq and stores
// its 16 bytes at the fragment position; the 8 lanes (kq, ksel) of a row reduce the row sum, LDS atomics across waves.
template <typename T, bool HAS_SUM, int STEPS, bool CS = false>   // STEPS: (k block pairs per wave) held in flight at once (0: generic loop)
__global__ void __launch_bounds__(512) quantize_tiled_kernel(const T* __restrict__ x, int8_t* __restrict__ q, int64_t rows,
                                                             int64_t cols, const float* __restrict__ scale,
                                                             const float* __restrict__ offset, float qmin, float qmax,
                                                             int shift, int32_t* __restrict__ row_sum,
                                                             const float* __restrict__ chan_scale = nullptr) {
  __shared__ int s_sum[8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 7, kq = (lane >> 3) & 3, ksel = lane >> 5;
  const int64_t row_raw = (int64_t)blockIdx.x * 8 + r;
  const int64_t row = row_raw < rows ? row_raw : rows - 1;      // rows past the end are padding (written, never used)
  const float s = scale[0], o = offset[0];
  const float inv_s = __fdiv_rn(1.0f, s);
  const int kblocks = (int)(cols >> 6), kpairs = kblocks >> 1;
  if (HAS_SUM && threadIdx.x < 8) s_sum[threadIdx.x] = 0;
  if (HAS_SUM) __syncthreads();
  int acc = 0;
  const T* xrow = x + row * cols + kq * 16;
  int8_t* qdst = q + tiled_image_offset(row_raw, kq * 16, cols);     // this lane's 16 bytes of k block 0; k block kb is kb KiB further
  auto emit = [&](int kb, const float (&fin)[16]) {
    float f[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) f[e] = fin[e];
    if constexpr (CS) {        // this lane's 16 channels: k = kb * 64 + kq * 16 + e
      const float4* cp = reinterpret_cast<const float4*>(chan_scale + (int64_t)kb * 64 + kq * 16);
      const float4 c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3];
      const float cs[16] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
#pragma unroll
      for (int e = 0; e < 16; ++e) f[e] = __fdiv_rn(f[e], cs[e]);
    }
    uint32_t w[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      uint32_t pk = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int st_v = static_cast<int>(index_storage_nan2qmin(f[d * 4 + e], s, inv_s, o, qmin, qmax)) - shift;
        acc += st_v;
        pk |= (static_cast<uint32_t>(st_v) & 0xffu) << (8 * e);
      }
      w[d] = pk;
    }
    *reinterpret_cast<uint4*>(qdst + ((int64_t)kb << 10)) = make_uint4(w[0], w[1], w[2], w[3]);
  };
  if constexpr (STEPS > 0 && std::is_same<T, float>::value) {
    float4 v[STEPS][4];       // everything this wave converts is requested before the first conversion
#pragma unroll
    for (int i = 0; i < STEPS; ++i) {
      const float4* p = reinterpret_cast<const float4*>(xrow + (int64_t)(2 * (wave + 8 * i) + ksel) * 64);
#pragma unroll
      for (int d = 0; d < 4; ++d) v[i][d] = p[d];
    }
#pragma unroll
    for (int i = 0; i < STEPS; ++i) {
      const float f[16] = {v[i][0].x, v[i][0].y, v[i][0].z, v[i][0].w, v[i][1].x, v[i][1].y, v[i][1].z, v[i][1].w,
                           v[i][2].x, v[i][2].y, v[i][2].z, v[i][2].w, v[i][3].x, v[i][3].y, v[i][3].z, v[i][3].w};
      emit(2 * (wave + 8 * i) + ksel, f);
    }
  } else {
    for (int kp = wave; kp < kpairs; kp += 8) {
      const int kb = 2 * kp + ksel;
      float f[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) f[e] = ld<T>(xrow + (int64_t)kb * 64, e);
      emit(kb, f);
    }
  }
  if (HAS_SUM) {
    acc += __shfl_xor(acc, 8, 64);
    acc += __shfl_xor(acc, 16, 64);
    acc += __shfl_xor(acc, 32, 64);
    if (lane < 8) atomicAdd(&s_sum[r], acc);
    __syncthreads();
    if (threadIdx.x < 8 && (int64_t)blockIdx.x * 8 + threadIdx.x < rows) row_sum[(int64_t)blockIdx.x * 8 + threadIdx.x] = s_sum[threadIdx.x];
  }
}

template <typename T, typename QT>
static int launch_quantize(const T* x, QT* q, int64_t rows, int64_t cols, const float* scale, const float* offset,
                           bool per_row, float qmin, float qmax, int shift, int32_t* row_sum, const float* chan_scale,
                           hipStream_t st) {
  constexpr int VN = Vec16<T>::N;
  const int vec_ok = aligned(x, 16) && aligned(q, sizeof(QT) * VN) && (cols % VN == 0);
  if (chan_scale != nullptr) {       // SmoothQuant channel scale: per-tensor grids of fp32 activations (checked by the caller)
    if constexpr (std::is_same<T, float>::value) {
      if constexpr (sizeof(QT) == 1) {
        if (aligned(x, 16) && aligned(q, 16) && aligned(chan_scale, 16) && cols % 16 == 0 && cols >= 256) {
          int64_t blocks = (rows + 3) / 4;
          if (blocks > 256 * 16) blocks = 256 * 16;
          quantize_rows_f32_b16_kernel<QT, false, true><<<(unsigned)blocks, 256, 0, st>>>(x, q, rows, cols, scale, offset, qmin,
                                                                                          qmax, shift, row_sum, chan_scale);
          MQ_LAUNCH_CHECK("mq_quantize");
          return MQ_OK;
        }
      }
      quantize_rows_kernel<T, QT, false, true><<<(unsigned)rows, 256, 0, st>>>(x, q, cols, scale, offset, qmin, qmax, shift,
                                                                             row_sum, vec_ok, chan_scale);
      MQ_LAUNCH_CHECK("mq_quantize");
      return MQ_OK;
    }
  }
  if constexpr (std::is_same<T, float>::value && sizeof(QT) == 1) {
    if (aligned(x, 16) && aligned(q, 16) && cols % 16 == 0 && cols >= 256) {
      int64_t blocks = (rows + 3) / 4;
      if (blocks > 256 * 16) blocks = 256 * 16;           // 16 workgroups per CU, wave-stride over the rest
      if (per_row)
        quantize_rows_f32_b16_kernel<QT, true><<<(unsigned)blocks, 256, 0, st>>>(x, q, rows, cols, scale, offset, qmin,
                                                                                 qmax, shift, row_sum);
      else
        quantize_rows_f32_b16_kernel<QT, false><<<(unsigned)blocks, 256, 0, st>>>(x, q, rows, cols, scale, offset, qmin,
                                                                                  qmax, shift, row_sum);
      MQ_LAUNCH_CHECK("mq_quantize");
      return MQ_OK;
    }
  }
  if (per_row)
    quantize_rows_kernel<T, QT, true><<<(unsigned)rows, 256, 0, st>>>(x, q, cols, scale, offset, qmin, qmax, shift,
                                                                    row_sum, vec_ok);
  else
    quantize_rows_kernel<T, QT, false><<<(unsigned)rows, 256, 0, st>>>(x, q, cols, scale, offset, qmin, qmax, shift,
                                                                     row_sum, vec_ok);
  MQ_LAUNCH_CHECK("mq_quantize");
  return MQ_OK;
}


// fp32 rows of 1024 .. 4096 columns: loads along the rows (a wave reads 1 KiB runs), the int8 results staged in an LDS tile in the
// image's order, stores as 128-byte runs (8 rows x 16 B: whole lines of a fragment block).  1024 threads = four groups of 256, two
// rows each, every load in flight before the first conversion (held to that in full workgroups: see the request order below).  Same
// index arithmetic as quantize_tiled_kernel: identical images.
// GRPS = 2: four rows per 512-thread workgroup, TWO workgroups per CU -- one's loads fly while the other converts and stores
// (mq_quantize_tiled_set_rows; the same change as in mq_norm.hip's norm_tiled8_kernel).
template <int V, bool HAS_SUM, int GRPS = 4>
__global__ void __launch_bounds__(256 * GRPS) quantize_tiled8_kernel(const float* __restrict__ x, int8_t* __restrict__ q, const float* __restrict__ scale,
                                                               const float* __restrict__ offset, int32_t* __restrict__ row_sum, int rows32, int shift,
                                                               float qmin, float qmax) {
  // The parameter list is 14 dwords, the most gfx950 delivers in user SGPRs at wave launch (kernarg preload, build.PER_FILE_FLAGS): the
  // body reads nothing from the kernel-argument segment (tools/kernarg_audit.py).  cols is the compile-time KCOLS; rows fits 32 bits
  // (checked by mq_quantize_tiled).
  const int64_t rows = rows32;
  typedef float v4f __attribute__((ext_vector_type(4)));
  constexpr int RW = 2 * GRPS;                                      // rows per workgroup
  constexpr int KCOLS = 1024 * V;                                   // == cols (mq_quantize_tiled's dispatch)
  extern __shared__ __attribute__((aligned(16))) int8_t stage8[];   // [cols / 16 pieces][RW rows][16 B]
  __shared__ int s_part[RW][4];
  // Request order (it matters on cold caches only, DESIGN 4.1: every wait below is a round trip to the fabric, and they stand in a row).
  // The kernel arguments arrive preloaded, so the first request is the grid values'; on firmware that does not preload, the compiler's
  // entry block reads all of them in ONE batch.  (The empty asm consumes the image and row-sum pointers here: it kept hipcc from leaving
  // their reads to the tail behind the barrier, each waited for in front of the stores it feeds, and still would if the list outgrew
  // the preload.)
  asm volatile("" ::"s"(q), "s"(row_sum));
  // the grid values: requested before any address arithmetic, waited for behind the last x request (as bit patterns: scalar registers)
  uint32_t s_bits = reinterpret_cast<const uint32_t*>(scale)[0], o_bits = reinterpret_cast<const uint32_t*>(offset)[0];
  asm volatile("; mq-grid-requested" ::: "memory");
  const int grp = threadIdx.x >> 8, lane = threadIdx.x & 255, wv_id = (threadIdx.x >> 6) & 3;
  const int64_t row0 = (int64_t)blockIdx.x * RW;
  const float ubias = (float)(128 - shift);               // image_u8f / image_pack4 (mq_common.h)
  // vector lane + 256 k of row j of this group -> its dword of the staging tile; two elements per VALU instruction where a packed form
  // exists (mq_common.h image_u8f2: the same bits)
  auto convert = [&](int j, int k, const float4 f, float s, float inv_s, float o, uint32_t& usum) {
    const int i = lane + 256 * k;
    const v2f u01 = image_u8f2((v2f){f.x, f.y}, s, inv_s, o, qmin, qmax, ubias), u23 = image_u8f2((v2f){f.z, f.w}, s, inv_s, o, qmin, qmax, ubias);
    const uint32_t pk = image_pack4(u01.x, u01.y, u23.x, u23.y, usum);
    *reinterpret_cast<uint32_t*>(stage8 + (i >> 2) * (RW * 16) + ((grp * 2 + j) << 4) + ((i & 3) << 2)) = pk;
  };
  auto row_done = [&](int j, uint32_t usum) {
    if (HAS_SUM) {
      const int acc = mq::wave_sum((int)usum);
      if ((threadIdx.x & 63) == 0) s_part[grp * 2 + j][wv_id] = acc;
    }
  };
  if (row0 + RW <= rows) {
    // Full workgroup (every one of a launch whose rows are a multiple of 16): no clamped address and no per-vector condition, so
    // nothing stands between a load and its use -- a conditional use makes hipcc sink the load into the branch, behind the grid
    // values' wait and the divide, and wait for it with vmcnt(0).  All 2 V requests go out behind the argument wait, the
    // conversions follow in issue order behind counted waits.  tools/load_order_audit.py holds the compiled order to this
    // (the two comment markers delimit the path for it).
    asm volatile("; mq-full-path-begin" ::: "memory");
    const char* xb = reinterpret_cast<const char*>(x + row0 * KCOLS);
    const uint32_t off = (uint32_t)(grp * 2) * (KCOLS * 4) + (uint32_t)lane * 16;
    float4 xs[2][V];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const char* xjk = xb + (j * KCOLS * 4 + k * 4096);            // a scalar base per request and ONE lane offset: no vector address
        asm("" : "+s"(xjk));                                          // arithmetic stands between two requests (hipcc would fold the constant into 64-bit lane adds)
        const v4f g = *reinterpret_cast<const __attribute__((address_space(1))) v4f*>((const __attribute__((address_space(1))) char*)xjk + off);   // (the tie hides that x is global memory)
        xs[j][k] = make_float4(g.x, g.y, g.z, g.w);
      }
    // the grid values' wait, and the divide, behind the last request: nothing is scheduled across the barrier, and the values pass
    // through the marker, so neither they nor a copy of them can be needed (and waited for) in front of it
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("; mq-x-requested" : "+s"(s_bits), "+s"(o_bits)::"memory");
    const float s = __builtin_bit_cast(float, s_bits), o = __builtin_bit_cast(float, o_bits);
    const float inv_s = __fdiv_rn(1.0f, s);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      uint32_t usum = 0;
#pragma unroll
      for (int k = 0; k < V; ++k) convert(j, k, xs[j][k], s, inv_s, o, usum);
      row_done(j, usum);
    }
    asm volatile("; mq-full-path-end" ::: "memory");
  } else {
    // ragged and padding workgroups (row0 + RW > rows): addresses clamped to the last real row
    constexpr int nvec = KCOLS >> 2;
    const float s = __builtin_bit_cast(float, s_bits), o = __builtin_bit_cast(float, o_bits);
    const float inv_s = __fdiv_rn(1.0f, s);
    float4 xs[2][V];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t row = row0 + grp * 2 + j;
      const float4* xr = reinterpret_cast<const float4*>(x + (row < rows ? row : rows - 1) * KCOLS);
#pragma unroll
      for (int k = 0; k < V; ++k) xs[j][k] = xr[lane + 256 * k < nvec ? lane + 256 * k : nvec - 1];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      uint32_t usum = 0;
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (lane + 256 * k < nvec) convert(j, k, xs[j][k], s, inv_s, o, usum);
      row_done(j, usum);
    }
  }
  __syncthreads();
  if (HAS_SUM && threadIdx.x < RW && row0 + threadIdx.x < rows)
    row_sum[row0 + threadIdx.x] = (s_part[threadIdx.x][0] + s_part[threadIdx.x][1]) + (s_part[threadIdx.x][2] + s_part[threadIdx.x][3]) - 128 * KCOLS;
  // rows past `rows` are padding of the image: written like the others.  Streaming stores: the image is read next by the GEMM, seven in
  // eight of its workgroups on other XCDs, so this XCD's L2 has no use for the lines; written with the default policy they stay dirty
  // in it until the kernel ends.  Same bytes, same image; this kernel's dispatch is 1.1 us shorter inside the headline step, the step
  // 0.95 us (DESIGN 4.2 "cache policy", NOTES 11.2: sc1 stores gain 0.6 us; streaming x LOADS cost 0.3 us wherever they were tried)
  staged_copy_out<RW, 256 * GRPS, true, STORE_NT>(stage8, q, row0, rows, KCOLS);
}

}  // namespace mq

using namespace mq;

extern "C" {

int mq_version(void) { return MQ_VERSION; }

const char* mq_last_error(void) { return g_err; }

int mq_device_info(int* cu_count, int* max_clock_khz, char* arch_name, size_t arch_name_len) {
  int dev = 0;
  hipDeviceProp_t p;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) {
    set_error("mq_device_info: no HIP device");
    return MQ_EHIP;
  }
  if (cu_count) *cu_count = p.multiProcessorCount;
  if (max_clock_khz) *max_clock_khz = p.clockRate;
  if (arch_name && arch_name_len) snprintf(arch_name, arch_name_len, "%s", p.gcnArchName);
  return MQ_OK;
}

int mq_quantize(const void* x, int dtype, int64_t rows, int64_t cols, const float* scale, const float* offset,
                int64_t n_scale, float qmin, float qmax, int shift, const float* chan_scale, void* q, int q_dtype,
                int32_t* row_sum, mq_stream_t stream) {
  MQ_REQUIRE(rows >= 0 && cols >= 0 && rows < (int64_t)0x7fffffff, "mq_quantize: bad shape %lld x %lld",
             (long long)rows, (long long)cols);
  MQ_REQUIRE(n_scale == 1 || n_scale == rows, "mq_quantize: n_scale=%lld must be 1 or rows=%lld", (long long)n_scale,
             (long long)rows);
  if (rows == 0 || cols == 0) return MQ_OK;      // empty tensor (its data pointer may be NULL)
  MQ_REQUIRE(x && q && scale && offset, "mq_quantize: null pointer");
  MQ_REQUIRE(chan_scale == nullptr || (dtype == MQ_F32 && n_scale == 1),
             "mq_quantize: chan_scale needs float32 activations and a per-tensor grid");
  const bool per_row = (n_scale == rows) && rows > 1 && chan_scale == nullptr;
  const float lo = qmin - (float)shift, hi = qmax - (float)shift;
  hipStream_t st = as_stream(stream);
#define MQ_Q(T, QT, LO, HI)                                                                                          \
  do {                                                                                                               \
    MQ_REQUIRE(lo >= (float)(LO) && hi <= (float)(HI), "mq_quantize: [%g,%g]-%d does not fit the storage type", qmin, \
               qmax, shift);                                                                                         \
    return launch_quantize<T, QT>((const T*)x, (QT*)q, rows, cols, scale, offset, per_row, qmin, qmax, shift,        \
                                  row_sum, chan_scale, st);                                                          \
  } while (0)
#define MQ_QD(T)                                          \
  switch (q_dtype) {                                      \
    case MQ_I8: MQ_Q(T, int8_t, -128, 127);               \
    case MQ_U8: MQ_Q(T, uint8_t, 0, 255);                 \
    case MQ_I16: MQ_Q(T, int16_t, -32768, 32767);         \
    case MQ_U16: MQ_Q(T, uint16_t, 0, 65535);             \
    case MQ_I32: MQ_Q(T, int32_t, -2147483648.0, 2147483520.0); \
    default: break;                                       \
  }
  if (dtype == MQ_F32) { MQ_QD(float) }
  else if (dtype == MQ_F16) { MQ_QD(__half) }
#undef MQ_QD
#undef MQ_Q
  set_error("mq_quantize: dtype %d -> q_dtype %d not supported", dtype, q_dtype);
  return MQ_EUNSUPPORTED;
}

static std::atomic<int> g_tiled8_rows{0};       // tuning hook: rows per workgroup of the staged kernel: 0 = by shape (4 up to 2048 columns), 4 / 8 forced
extern "C" int mq_quantize_tiled_set_rows(int rows) {
  g_tiled8_rows = rows == 4 ? 4 : (rows == 8 ? 8 : 0);
  return 0;
}
static std::atomic<int> g_tiled8{1};            // tuning hook: 0 = the lane-per-fragment kernel for every shape
int mq_quantize_tiled_set_staged(int on) {
  g_tiled8 = on ? 1 : 0;
  return 0;
}

int mq_quantize_tiled(const void* x, int dtype, int64_t rows, int64_t cols, const float* scale, const float* offset,
                      float qmin, float qmax, int shift, const float* chan_scale, int8_t* q_tiled, int32_t* row_sum,
                      mq_stream_t stream) {
  MQ_REQUIRE(rows != 0 ? (x && q_tiled && scale && offset) : true, "mq_quantize_tiled: null pointer");
  MQ_REQUIRE(rows >= 0 && cols > 0 && cols % 128 == 0 && (rows + 15) / 8 < (int64_t)0x7fffffff,
             "mq_quantize_tiled: bad shape %lld x %lld (cols must be a multiple of 128)", (long long)rows, (long long)cols);
  MQ_REQUIRE(qmin - (float)shift >= -128.f && qmax - (float)shift <= 127.f, "mq_quantize_tiled: [%g,%g]-%d does not fit int8",
             qmin, qmax, shift);
  if (rows == 0) return MQ_OK;
  MQ_REQUIRE(aligned(x, 16) && aligned(q_tiled, 16), "mq_quantize_tiled: pointers must be 16-byte aligned");
  MQ_REQUIRE(chan_scale == nullptr || (dtype == MQ_F32 && aligned(chan_scale, 16)),
             "mq_quantize_tiled: chan_scale needs float32 activations and a 16-byte aligned vector");
  const unsigned grid = (unsigned)(((rows + 15) / 16) * 2);      // 8 rows per workgroup, padding rows included
  hipStream_t st = as_stream(stream);
#define MQ_QT(T, KBW)                                                                                                 \
  do {                                                                                                                \
    if (row_sum) quantize_tiled_kernel<T, true, KBW><<<grid, 512, 0, st>>>((const T*)x, q_tiled, rows, cols, scale, offset, qmin, qmax, shift, row_sum); \
    else quantize_tiled_kernel<T, false, KBW><<<grid, 512, 0, st>>>((const T*)x, q_tiled, rows, cols, scale, offset, qmin, qmax, shift, row_sum);       \
  } while (0)
  const int64_t kblocks = cols >> 6;
  if (chan_scale != nullptr) {       // the SmoothQuant form: x / chan_scale[k] in front of the same index arithmetic
    if (row_sum) quantize_tiled_kernel<float, true, 0, true><<<grid, 512, 0, st>>>((const float*)x, q_tiled, rows, cols, scale, offset, qmin, qmax, shift, row_sum, chan_scale);
    else quantize_tiled_kernel<float, false, 0, true><<<grid, 512, 0, st>>>((const float*)x, q_tiled, rows, cols, scale, offset, qmin, qmax, shift, row_sum, chan_scale);
  } else if (dtype == MQ_F32 && cols >= 1024 && cols <= 4096 && cols % 1024 == 0 && rows >= 64 && g_tiled8.load()) {
    MQ_REQUIRE(rows <= (int64_t)0x7fffffff, "mq_quantize_tiled: %lld rows do not fit the staged kernel's 32-bit row count", (long long)rows);
    const int rows_knob = g_tiled8_rows.load();
    const bool four = rows_knob == 4 || (rows_knob == 0 && cols <= 2048);
    const unsigned grid8 = (unsigned)(((rows + 15) / 16) * (four ? 4 : 2));
    const size_t lds = (size_t)cols * (four ? 4 : 8);
#define MQ_QT8(V)                                                                                                                              \
  do {                                                                                                                                         \
    if (four) {                                                                                                                                \
      if (row_sum) quantize_tiled8_kernel<V, true, 2><<<grid8, 512, lds, st>>>((const float*)x, q_tiled, scale, offset, row_sum, (int)rows, shift, qmin, qmax);  \
      else quantize_tiled8_kernel<V, false, 2><<<grid8, 512, lds, st>>>((const float*)x, q_tiled, scale, offset, row_sum, (int)rows, shift, qmin, qmax);        \
    } else if (row_sum) quantize_tiled8_kernel<V, true><<<grid8, 1024, lds, st>>>((const float*)x, q_tiled, scale, offset, row_sum, (int)rows, shift, qmin, qmax);  \
    else quantize_tiled8_kernel<V, false><<<grid8, 1024, lds, st>>>((const float*)x, q_tiled, scale, offset, row_sum, (int)rows, shift, qmin, qmax);        \
  } while (0)
    if (cols == 1024) MQ_QT8(1);
    else if (cols == 2048) MQ_QT8(2);
    else if (cols == 3072) MQ_QT8(3);
    else MQ_QT8(4);
#undef MQ_QT8
  } else if (dtype == MQ_F32) {
    if (kblocks == 32) MQ_QT(float, 2);            // K = 2048: 2 steps of 2 k blocks per wave, all in flight
    else if (kblocks == 16) MQ_QT(float, 1);
    else MQ_QT(float, 0);
  } else if (dtype == MQ_F16) {
    MQ_QT(__half, 0);
  } else {
    set_error("mq_quantize_tiled: dtype %d not supported", dtype);
    return MQ_EUNSUPPORTED;
  }
#undef MQ_QT
  MQ_LAUNCH_CHECK("mq_quantize_tiled");
  return MQ_OK;
}

int mq_linear_epilogue_prepare(const float* a_scale, const float* a_offset, int a_shift, const float* w_scale,
                               const float* w_offset, int64_t n_wscale, int w_shift, const int32_t* w_colsum,
                               int64_t N, int64_t K, float* alpha, int32_t* w_zp, int32_t* col_term,
                               mq_stream_t stream) {
  MQ_REQUIRE(a_scale && a_offset && w_scale && w_offset && w_colsum && alpha && w_zp && col_term,
             "mq_linear_epilogue_prepare: null pointer");
  MQ_REQUIRE(N > 0 && K > 0 && K < (1 << 24), "mq_linear_epilogue_prepare: N=%lld K=%lld", (long long)N, (long long)K);
  MQ_REQUIRE(n_wscale == 1 || n_wscale == N, "mq_linear_epilogue_prepare: n_wscale=%lld must be 1 or N",
             (long long)n_wscale);
  linear_epilogue_prepare_kernel<<<(unsigned)((N + 255) / 256), 256, 0, as_stream(stream)>>>(
      a_scale, a_offset, a_shift, w_scale, w_offset, n_wscale == N && N > 1, w_shift, w_colsum, N, (int)K, alpha, w_zp,
      col_term);
  MQ_LAUNCH_CHECK("mq_linear_epilogue_prepare");
  return MQ_OK;
}

int mq_pack_w4(const uint8_t* nibbles, int64_t N, int64_t K, uint8_t* packed, mq_stream_t stream) {
  MQ_REQUIRE(nibbles && packed, "mq_pack_w4: null pointer");
  MQ_REQUIRE(N > 0 && K > 0 && K % 64 == 0, "mq_pack_w4: K=%lld must be a positive multiple of 64", (long long)K);
  const int64_t total = N * K / 2;
  pack_w4_kernel<<<(unsigned)((total + 255) / 256), 256, 0, as_stream(stream)>>>(nibbles, total, packed);
  MQ_LAUNCH_CHECK("mq_pack_w4");
  return MQ_OK;
}

}  // extern "C"
