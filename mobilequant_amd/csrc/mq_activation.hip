// The activation kernels of the prefill path: QSiLU / QGELU in one pass, the gated FFN's act(w1 x) * w3 x -> w2's integer input image
// (values or 8-bit indices in), the same map as a 256 x 256 table and its lookup.  Every route evaluates ONE gate chain (gate_chain
// below) with the value-form quantizer of mq_quant.h, so the routes agree bit for bit.
#include "mq_common.h"

#pragma clang fp contract(off)

// ---- QSiLU / QGELU.forward in one pass (qmodule.py:739-754, :790-798) -------------------------------------------
// SiLU:  xi = Qin(x);  g = Qmid(sigmoid(xi));  out = Qout(xi * g)       (Qmid: the [0,1] sigmoid grid, qmodule.py:731-734)
// GELU:  xi = Qin(x);  out = Qout(0.5 * xi * (1 + erf(xi / sqrt 2)))
// = 4 (2) launches and 9 (5) passes as composite ops.  exp / erf are the device library's (<= 1-2 ulp), the divide of the
// sigmoid is IEEE: results equal torch's GPU sigmoid / gelu bit for bit and the CPU reference's up to those ulps, i.e.
// after the output quantizer at most one LSB apart on a vanishing fraction of elements.
namespace mq {

// y1 = Qact(act(xi)) of one gate input value xi (qmodule.py:739-753, :790-798):  QSiLU xi * Qmid(sigmoid(xi)),  QGELU the erf form
__device__ __forceinline__ float gate_chain(int act, float xi, const Grid& mid, const Grid& actout) {
  float r;
  if (act == 0) {
    const float gate = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-xi)));
    r = __fmul_rn(xi, mid.fq_value(gate));
  } else {
    r = __fmul_rn(__fmul_rn(0.5f, xi), __fadd_rn(1.0f, erff(__fmul_rn(xi, 0.70710678118654752440f))));
  }
  return actout.fq_value(r);
}

struct ActArgs {
  const float* x;
  float* y;
  int64_t numel;
  int act;   // 0 = SiLU, 1 = GELU (erf)
  const float* s[3];   // in / mid / out scale (nullable)
  const float* o[3];
  float qmin[3], qmax[3];
};

__global__ void __launch_bounds__(256) act_quant_kernel(const ActArgs a) {
  Grid g[3];           // in / mid / out
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = load_grid(a.s[k], a.o[k], a.qmin[k], a.qmax[k]);
  auto f = [&](float v) { return gate_chain(a.act, g[0].fq_value(v), g[1], g[2]); };
  const int64_t nvec = a.numel >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
    float4 v = reinterpret_cast<const float4*>(a.x)[i];
    v.x = f(v.x); v.y = f(v.y); v.z = f(v.z); v.w = f(v.w);
    reinterpret_cast<float4*>(a.y)[i] = v;
  }
  for (int64_t i = (nvec << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.numel; i += stride) a.y[i] = f(a.x[i]);
}


// ---- f1: the gated FFN's  act(w1(x)) * w3(x)  -> integer input image of w2, ONE launch ------------------------------------------
// Reference chain (hf_model.py:1057, qmodule.py:739-753): y1 = Qact(va * Qmid(sigmoid(va))) (QSiLU; QGELU: Qact(gelu(va))), the
// plain fp32 product p = y1 * vb (ElementwiseMul is not quantised), then w2's input quantizer.  va / vb arrive either as fp32 values
// or -- the integer chain -- as the 8-bit output INDICES the w1 / w3 GEMMs wrote (va = (qa - oa) * sa: exactly the fp32 value the
// fake-quant path would hold).  Output: int8 storage (index - shift) of p on w2's input grid + row sums (what mq_quantize would
// produce from p), optionally p itself.  3 B per element instead of 17 for the composite chain.  Wave per row, 16 elements per lane.
struct GatedArgs {
  const void* a;
  const void* b;
  int in_index;                // 0: fp32 values, 1: u8 indices
  int64_t rows, cols;
  int act;
  const float* s[5];           // a grid, b grid, mid (sigmoid) grid, activation output grid, w2 input grid
  const float* o[5];
  float qmin[5], qmax[5];
  int shift;
  int8_t* q;
  int32_t* row_sum;
  float* y;
};

enum { GG_A = 0, GG_B = 1, GG_MID = 2, GG_ACT = 3, GG_OUT = 4 };      // GatedArgs' grids

// Index inputs take only 256 values each: thread t of 256 evaluates the gate chain of index t (and the plain value of b's index t)
// into the two LDS tables -- the arithmetic of the value route on the same operands, so a table read IS that arithmetic's result.
__device__ __forceinline__ void gated_lut_fill(float (*lut)[256], const GatedArgs& g, const Grid (&gr)[4]) {
  lut[0][threadIdx.x] = gate_chain(g.act, dequant((float)threadIdx.x, gr[GG_A].s, gr[GG_A].o), gr[GG_MID], gr[GG_ACT]);
  lut[1][threadIdx.x] = dequant((float)threadIdx.x, gr[GG_B].s, gr[GG_B].o);
}
// the product on w2's input grid -> int8 storage: the value form's index, NaN -> qmin like mq_quantize (integer storage has no NaN)
__device__ __forceinline__ int gated_store(float prod, float so, float iso, float oo, float qmin, float qmax, int shift) {
  return to_storage_nan2qmin(index_value_keepnan(prod, so, iso, oo, qmin, qmax), qmin, shift);
}

template <bool INDEX, bool WRITE_Y>
__global__ void __launch_bounds__(256) gated_act_quant_kernel(const GatedArgs g) {
  Grid gr[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) gr[k] = load_grid(g.s[k], g.o[k], g.qmin[k], g.qmax[k]);
  const Grid go = load_grid(g.s[GG_OUT], g.o[GG_OUT], g.qmin[GG_OUT], g.qmax[GG_OUT]);
  auto gate_of = [&](float xi) { return gate_chain(g.act, xi, gr[GG_MID], gr[GG_ACT]); };
  // index inputs: the whole activation chain (exp, three exact divides) ONCE per index (gated_lut_fill); the per-element work is two
  // table reads, the product and w2's input quantizer.  (45 -> ~10 us at [2048, 5632].)
  __shared__ float lut[2][256];
  if constexpr (INDEX) {
    gated_lut_fill(lut, g, gr);
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t row = wave0; row < g.rows; row += nwaves) {
    int acc = 0;
    for (int64_t c = (int64_t)lane * 16; c < g.cols; c += 1024) {
      float y1[16], vb[16];
      const int64_t at = row * g.cols + c;
      if constexpr (INDEX) {
        const uint4 pa = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(g.a) + at);
        const uint4 pb = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(g.b) + at);
        const uint32_t wa[4] = {pa.x, pa.y, pa.z, pa.w}, wb[4] = {pb.x, pb.y, pb.z, pb.w};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          y1[e] = lut[0][(wa[e >> 2] >> (8 * (e & 3))) & 0xffu];
          vb[e] = lut[1][(wb[e >> 2] >> (8 * (e & 3))) & 0xffu];
        }
      } else {
        const float4* pa = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(g.a) + at);
        const float4* pb = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(g.b) + at);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const float4 x = pa[d], z = pb[d];
          y1[4 * d] = gate_of(x.x); y1[4 * d + 1] = gate_of(x.y); y1[4 * d + 2] = gate_of(x.z); y1[4 * d + 3] = gate_of(x.w);
          vb[4 * d] = z.x; vb[4 * d + 1] = z.y; vb[4 * d + 2] = z.z; vb[4 * d + 3] = z.w;
        }
      }
      float p[16];
      uint32_t w[4];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        uint32_t pk = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float prod = __fmul_rn(y1[4 * d + e], vb[4 * d + e]);
          p[4 * d + e] = prod;
          const int st_v = gated_store(prod, go.s, go.inv_s, go.o, go.qmin, go.qmax, g.shift);
          acc += st_v;
          pk |= ((uint32_t)st_v & 0xffu) << (8 * e);
        }
        w[d] = pk;
      }
      *reinterpret_cast<uint4*>(g.q + at) = make_uint4(w[0], w[1], w[2], w[3]);
      if constexpr (WRITE_Y) {
        float4* py = reinterpret_cast<float4*>(g.y + at);
#pragma unroll
        for (int d = 0; d < 4; ++d) py[d] = make_float4(p[4 * d], p[4 * d + 1], p[4 * d + 2], p[4 * d + 3]);
      }
    }
    if (g.row_sum != nullptr) {
      acc = wave_sum(acc);
      if (lane == 0) g.row_sum[row] = acc;
    }
  }
}

// Index inputs without the fp32 side output (the integer chain of fuse_gated_mlp): a WORKGROUP per row and 8 elements per thread
// and trip, so that [2048, 5632] puts 8 waves on every SIMD instead of 2 -- the kernel is a latency-bound stream (two LDS table reads
// and one exact divide per element), occupancy is what it lacks.  Same tables, same per-element arithmetic as the kernel above.
__global__ void __launch_bounds__(256) gated_index_rows_kernel(const GatedArgs g) {
  __shared__ float lut[2][256];
  __shared__ int s_part[4];
  const float so = g.s[GG_OUT][0], oo = g.o[GG_OUT][0];               // the output grid is required (host-checked)
  const float iso = __fdiv_rn(1.0f, so);
  {
    Grid gr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) gr[k] = load_grid(g.s[k], g.o[k], g.qmin[k], g.qmax[k]);
    gated_lut_fill(lut, g, gr);
  }
  __syncthreads();
  const int64_t row = blockIdx.x;
  const uint8_t* pa = reinterpret_cast<const uint8_t*>(g.a) + row * g.cols;
  const uint8_t* pb = reinterpret_cast<const uint8_t*>(g.b) + row * g.cols;
  int8_t* pq = g.q + row * g.cols;
  int acc = 0;
  for (int64_t c = (int64_t)threadIdx.x * 8; c < g.cols; c += 2048) {
    const uint2 va = *reinterpret_cast<const uint2*>(pa + c), vb = *reinterpret_cast<const uint2*>(pb + c);
    const uint32_t wa[2] = {va.x, va.y}, wb[2] = {vb.x, vb.y};
    uint32_t w[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      uint32_t pk = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float prod = __fmul_rn(lut[0][(wa[d] >> (8 * e)) & 0xffu], lut[1][(wb[d] >> (8 * e)) & 0xffu]);
        const int st_v = gated_store(prod, so, iso, oo, g.qmin[GG_OUT], g.qmax[GG_OUT], g.shift);
        acc += st_v;
        pk |= ((uint32_t)st_v & 0xffu) << (8 * e);
      }
      w[d] = pk;
    }
    *reinterpret_cast<uint2*>(pq + c) = make_uint2(w[0], w[1]);
  }
  if (g.row_sum != nullptr) {
    acc = wave_sum(acc);
    const int total = block_sum4(acc, s_part, (int)(threadIdx.x >> 6));
    if (threadIdx.x == 0) g.row_sum[row] = total;
  }
}

// ---- the same map as a 256 x 256 table --------------------------------------------------------------------------------------------
// With index inputs and static grids, act(a) * b -> w2's input index is a FUNCTION of the two 8-bit indices: 65 536 values, computed
// once per set of grids (mq_gated_table: the per-element arithmetic of the kernels above, evaluated for every (ia, ib) pair -- the
// table IS that arithmetic, so results are bit-identical) and then looked up (mq_gated_lookup): one LDS byte read per element instead
// of two table reads, a multiply and an IEEE divide.  The lookup kernel is a pure stream (2 B in, 1 B out per element).
__global__ void __launch_bounds__(256) gated_table_kernel(const GatedArgs g, int8_t* __restrict__ table) {
  Grid gr[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) gr[k] = load_grid(g.s[k], g.o[k], g.qmin[k], g.qmax[k]);
  const Grid& go = gr[GG_OUT];
  const int ia = blockIdx.x, ib = threadIdx.x;
  const float y1 = gate_chain(g.act, dequant((float)ia, gr[GG_A].s, gr[GG_A].o), gr[GG_MID], gr[GG_ACT]);
  const float prod = __fmul_rn(y1, dequant((float)ib, gr[GG_B].s, gr[GG_B].o));
  table[ia * 256 + ib] = (int8_t)gated_store(prod, go.s, go.inv_s, go.o, go.qmin, go.qmax, g.shift);
}

constexpr int GL_TABLE = 65536;
// 1024 threads = four groups of four waves; a group owns one row at a time (rows strided by 4 * gridDim), requests the whole row up
// front (<= 4 x 8 bytes per lane and operand), then looks up.  Two such workgroups are resident per CU (2 x 64 KiB of LDS): 8 waves
// per SIMD, and at [2048, 5632] every group handles exactly one row -- the kernel is one round of loads, lookups and stores.
// TILED: q is the fragment-blocked image of mq_quantize_tiled (1-KiB blocks of 16 rows x 64 k; a lane's eight bytes stay inside one
// 16-byte fragment chunk, and the four rows of a workgroup's trip -- rows 4 n .. 4 n + 3 -- fill whole 64-byte pieces of a block).
template <bool TILED>
__global__ void __launch_bounds__(1024) gated_lookup_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int64_t rows, int64_t cols,
                                                            const int8_t* __restrict__ table, int8_t* __restrict__ q, int32_t* __restrict__ row_sum) {
  auto dst = [&](int64_t row, int64_t c) -> int8_t* {
    if constexpr (TILED) return q + tiled_image_offset(row, c, cols);
    else return q + row * cols + c;
  };
  extern __shared__ __attribute__((aligned(16))) int8_t lut[];      // [256][256]
  __shared__ int s_sum[4];
  const int grp = threadIdx.x >> 8, tid = threadIdx.x & 255;
  constexpr int MAXIT = 4;                                          // cols <= 8192 on the fast path (host-checked); longer rows loop
  const int64_t row0 = (int64_t)blockIdx.x * 4 + grp;
  uint2 va[MAXIT], vb[MAXIT];
  const bool fast = cols <= 2048 * MAXIT;
  if (fast && row0 < rows) {                                        // first row's operands go out before the table copy
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int64_t c = (int64_t)tid * 8 + 2048 * it;
      if (c < cols) {
        va[it] = *reinterpret_cast<const uint2*>(a + row0 * cols + c);
        vb[it] = *reinterpret_cast<const uint2*>(b + row0 * cols + c);
      }
    }
  }
  for (int i = threadIdx.x; i < GL_TABLE / 16; i += 1024) reinterpret_cast<uint4*>(lut)[i] = reinterpret_cast<const uint4*>(table)[i];
  __syncthreads();
  auto convert = [&](uint2 x, uint2 y, int& acc) {
    const uint32_t wa[2] = {x.x, x.y}, wb[2] = {y.x, y.y};
    uint32_t w[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      uint32_t pk = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int st_v = lut[(((wa[d] >> (8 * e)) & 0xffu) << 8) | ((wb[d] >> (8 * e)) & 0xffu)];
        acc += st_v;
        pk |= ((uint32_t)st_v & 0xffu) << (8 * e);
      }
      w[d] = pk;
    }
    return make_uint2(w[0], w[1]);
  };
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < rows; base += stride) {      // uniform trip count for the whole workgroup
    const int64_t row = base + grp;
    int acc = 0;
    if (row < rows) {
      if (fast) {
        if (base != (int64_t)blockIdx.x * 4) {
#pragma unroll
          for (int it = 0; it < MAXIT; ++it) {
            const int64_t c = (int64_t)tid * 8 + 2048 * it;
            if (c < cols) {
              va[it] = *reinterpret_cast<const uint2*>(a + row * cols + c);
              vb[it] = *reinterpret_cast<const uint2*>(b + row * cols + c);
            }
          }
        }
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
          const int64_t c = (int64_t)tid * 8 + 2048 * it;
          if (c < cols) *reinterpret_cast<uint2*>(dst(row, c)) = convert(va[it], vb[it], acc);
        }
      } else {
        for (int64_t c = (int64_t)tid * 8; c < cols; c += 2048)
          *reinterpret_cast<uint2*>(dst(row, c)) =
              convert(*reinterpret_cast<const uint2*>(a + row * cols + c), *reinterpret_cast<const uint2*>(b + row * cols + c), acc);
      }
    }
    if (row_sum != nullptr) {
      if (tid < 1) s_sum[grp] = 0;
      __syncthreads();
      acc = wave_sum(acc);
      if ((threadIdx.x & 63) == 0) atomicAdd(&s_sum[grp], acc);
      __syncthreads();
      if (tid == 0 && row < rows) row_sum[row] = s_sum[grp];
    }
  }
}

}  // namespace mq

using namespace mq;

extern "C" int mq_gated_table(int act, const float* a_scale, const float* a_offset, const float* b_scale, const float* b_offset,
                              const float* mid_scale, const float* mid_offset, float mid_qmin, float mid_qmax, const float* act_scale,
                              const float* act_offset, float act_qmin, float act_qmax, const float* out_scale, const float* out_offset,
                              float out_qmin, float out_qmax, int q_shift, int8_t* table, mq_stream_t stream) {
  MQ_REQUIRE((act == 0 || act == 1) && a_scale && a_offset && b_scale && b_offset && out_scale && out_offset && table,
             "mq_gated_table: null pointer / bad act (0 SiLU, 1 GELU)");
  MQ_REQUIRE((mid_scale == nullptr) == (mid_offset == nullptr) && (act_scale == nullptr) == (act_offset == nullptr),
             "mq_gated_table: scale/offset must both be set or NULL");
  MQ_REQUIRE(out_qmin - (float)q_shift >= -128.f && out_qmax - (float)q_shift <= 127.f, "mq_gated_table: output grid does not fit int8");
  GatedArgs g{nullptr, nullptr, 1, 0, 0, act, {a_scale, b_scale, mid_scale, act_scale, out_scale}, {a_offset, b_offset, mid_offset, act_offset, out_offset},
              {0.f, 0.f, mid_qmin, act_qmin, out_qmin}, {0.f, 0.f, mid_qmax, act_qmax, out_qmax}, q_shift, nullptr, nullptr, nullptr};
  gated_table_kernel<<<256, 256, 0, as_stream(stream)>>>(g, table);
  MQ_LAUNCH_CHECK("mq_gated_table");
  return MQ_OK;
}

static int gated_lookup_launch(const char* fn, bool tiled, const uint8_t* a, const uint8_t* b, int64_t rows, int64_t cols, const int8_t* table,
                               int8_t* q_out, int32_t* row_sum, mq_stream_t stream) {
  MQ_REQUIRE(rows >= 0 && cols >= 0 && cols % (tiled ? 64 : 8) == 0, "%s: cols %% %d == 0", fn, tiled ? 64 : 8);
  if (rows == 0 || cols == 0) return MQ_OK;
  MQ_REQUIRE(a && b && table && q_out && aligned(a, 8) && aligned(b, 8) && aligned(q_out, tiled ? 16 : 8) && aligned(table, 16),
             "%s: null or misaligned pointer", fn);
  static PerDeviceOnce attr_set[2];
  const int dev = current_device();
  if (!attr_set[tiled].done(dev)) {
    hipError_t e = hipFuncSetAttribute(tiled ? (const void*)gated_lookup_kernel<true> : (const void*)gated_lookup_kernel<false>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, GL_TABLE);
    if (e != hipSuccess) {
      set_error("%s: hipFuncSetAttribute: %s", fn, hipGetErrorString(e));
      return MQ_EHIP;
    }
    attr_set[tiled].mark(dev);
  }
  int64_t blocks = (rows + 3) / 4;                          // four rows per workgroup and trip; two resident workgroups per CU
  if (blocks > 512) blocks = 512;
  if (tiled) gated_lookup_kernel<true><<<(unsigned)blocks, 1024, GL_TABLE, as_stream(stream)>>>(a, b, rows, cols, table, q_out, row_sum);
  else gated_lookup_kernel<false><<<(unsigned)blocks, 1024, GL_TABLE, as_stream(stream)>>>(a, b, rows, cols, table, q_out, row_sum);
  MQ_LAUNCH_CHECK(fn);
  return MQ_OK;
}

extern "C" int mq_gated_lookup(const uint8_t* a, const uint8_t* b, int64_t rows, int64_t cols, const int8_t* table, int8_t* q_out,
                               int32_t* row_sum, mq_stream_t stream) {
  return gated_lookup_launch("mq_gated_lookup", false, a, b, rows, cols, table, q_out, row_sum, stream);
}

extern "C" int mq_gated_lookup_tiled(const uint8_t* a, const uint8_t* b, int64_t rows, int64_t cols, const int8_t* table, int8_t* q_tiled,
                                     int32_t* row_sum, mq_stream_t stream) {
  return gated_lookup_launch("mq_gated_lookup_tiled", true, a, b, rows, cols, table, q_tiled, row_sum, stream);
}

extern "C" int mq_gated_act_quant(const void* a, const void* b, int in_dtype, int64_t rows, int64_t cols, int act,
                                  const float* a_scale, const float* a_offset, const float* b_scale, const float* b_offset,
                                  const float* mid_scale, const float* mid_offset, float mid_qmin, float mid_qmax,
                                  const float* act_scale, const float* act_offset, float act_qmin, float act_qmax,
                                  const float* out_scale, const float* out_offset, float out_qmin, float out_qmax, int q_shift,
                                  int8_t* q_out, int32_t* row_sum, float* y, mq_stream_t stream) {
  MQ_REQUIRE(rows >= 0 && cols >= 0 && cols % 16 == 0 && (act == 0 || act == 1),
             "mq_gated_act_quant: bad arguments (cols %% 16 == 0; act = 0 SiLU, 1 GELU)");
  if (rows == 0 || cols == 0) return MQ_OK;
  MQ_REQUIRE(a && b && q_out && out_scale && out_offset, "mq_gated_act_quant: null pointer (a, b, q_out and the output grid are required)");
  MQ_REQUIRE(in_dtype == MQ_F32 || in_dtype == MQ_U8, "mq_gated_act_quant: inputs are float32 values or uint8 indices");
  MQ_REQUIRE(in_dtype == MQ_F32 || (a_scale && a_offset && b_scale && b_offset), "mq_gated_act_quant: index inputs need their grids");
  MQ_REQUIRE(aligned(a, 16) && aligned(b, 16) && aligned(q_out, 16) && (!y || aligned(y, 16)), "mq_gated_act_quant: pointers must be 16-byte aligned");
  MQ_REQUIRE((mid_scale == nullptr) == (mid_offset == nullptr) && (act_scale == nullptr) == (act_offset == nullptr),
             "mq_gated_act_quant: scale/offset must both be set or NULL");
  MQ_REQUIRE(out_qmin - (float)q_shift >= -128.f && out_qmax - (float)q_shift <= 127.f, "mq_gated_act_quant: output grid does not fit int8");
  const bool idx = in_dtype == MQ_U8;
  GatedArgs g{a, b, idx ? 1 : 0, rows, cols, act,
              {idx ? a_scale : nullptr, idx ? b_scale : nullptr, mid_scale, act_scale, out_scale},
              {idx ? a_offset : nullptr, idx ? b_offset : nullptr, mid_offset, act_offset, out_offset},
              {0.f, 0.f, mid_qmin, act_qmin, out_qmin}, {0.f, 0.f, mid_qmax, act_qmax, out_qmax}, q_shift, q_out, row_sum, y};
  int64_t blocks = (rows + 3) / 4;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipStream_t st = as_stream(stream);
  if (idx && !y && cols % 8 == 0 && rows < (int64_t)0x7fffffff && aligned(a, 8) && aligned(b, 8)) {
    gated_index_rows_kernel<<<(unsigned)rows, 256, 0, st>>>(g);
  } else if (idx) {
    if (y) gated_act_quant_kernel<true, true><<<(unsigned)blocks, 256, 0, st>>>(g);
    else gated_act_quant_kernel<true, false><<<(unsigned)blocks, 256, 0, st>>>(g);
  } else {
    if (y) gated_act_quant_kernel<false, true><<<(unsigned)blocks, 256, 0, st>>>(g);
    else gated_act_quant_kernel<false, false><<<(unsigned)blocks, 256, 0, st>>>(g);
  }
  MQ_LAUNCH_CHECK("mq_gated_act_quant");
  return MQ_OK;
}

extern "C" int mq_act_quant(const float* x, int64_t numel, int act, const float* in_scale, const float* in_offset, float in_qmin,
                            float in_qmax, const float* mid_scale, const float* mid_offset, float mid_qmin, float mid_qmax,
                            const float* out_scale, const float* out_offset, float out_qmin, float out_qmax, float* y,
                            mq_stream_t stream) {
  MQ_REQUIRE(numel >= 0 && (act == 0 || act == 1), "mq_act_quant: bad arguments (act = 0 SiLU, 1 GELU)");
  if (numel == 0) return MQ_OK;
  MQ_REQUIRE(x && y && aligned(x, 16) && aligned(y, 16), "mq_act_quant: x / y must be non-null and 16-byte aligned");
  MQ_REQUIRE((in_scale == nullptr) == (in_offset == nullptr) && (mid_scale == nullptr) == (mid_offset == nullptr) &&
                 (out_scale == nullptr) == (out_offset == nullptr),
             "mq_act_quant: scale/offset must both be set or NULL");
  ActArgs a{x, y, numel, act, {in_scale, mid_scale, out_scale}, {in_offset, mid_offset, out_offset},
            {in_qmin, mid_qmin, out_qmin}, {in_qmax, mid_qmax, out_qmax}};
  int64_t g = ((numel >> 2) + 255) / 256;
  if (g < 1) g = 1;
  if (g > 256 * 8) g = 256 * 8;
  act_quant_kernel<<<(unsigned)g, 256, 0, as_stream(stream)>>>(a);
  MQ_LAUNCH_CHECK("mq_act_quant");
  return MQ_OK;
}