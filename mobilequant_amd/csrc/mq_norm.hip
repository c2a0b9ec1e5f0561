// QRMSNorm.forward (qmodule.py:469-530 around hf_model.py:184-195) in ONE pass over the activations.
//
// Reference op sequence on x [rows, cols] (fp32):
//   xi  = Qin(x)                                 input quantizer (16-bit per-tensor in every recipe), optional
//   r   = rsqrt(mean(xi^2, -1) + eps)            x.pow(2).mean(-1, keepdim=True); torch.rsqrt
//   y   = weight' * (xi * r) (+ bias)            weight' = Qw(weight), fake-quantised once by the caller
//   out = Qout(y)                                8-bit per-tensor activation grid, optional
// = 6 elementwise / reduction launches and ~9 passes over the tensor as composite torch ops.  Here a wave owns a
// row, keeps it in registers (cols <= 4096) or re-reads it (larger), and writes out -- and, when the output grid is
// an 8-bit one, the int8 indices + row sums the consumer linears (q/k/v, w1/w3) feed to the integer GEMM, so their
// activation quantize launches disappear (norm -> int8 -> GEMM chaining).
//
// Numerics: every elementwise op is the reference's (IEEE divide, round-half-even, separate mul/add; 1/sqrt with
// correctly rounded sqrt and divide, which is what the CPU reference computes).  The sum of squares is reduced in
// a different order than torch's (lane-strided partial sums, then a butterfly), so r can differ in the last bit
// and an output that sits within ~1e-7 relative of a rounding boundary can land on the neighbouring grid point.
// What the tests hold (tests/test_gpu_prefill_elementwise.py): given the row scalar -- some fp32 r within the
// derived bound of the float64 one -- every RMSNorm output is the fp32 replay of `emit` bit for bit; a LayerNorm element equals the
// float64 oracle's index unless its pre-rounding value is within the derived fp32 bound of a boundary (< 0.1 % of the elements of an
// 8-bit grid), and is one step away at most there.  Against the reference's frozen outputs: 1 LSB on < 0.1 % of the elements.
#include <hip/hip_fp16.h>

#include "mq_common.h"

namespace mq {

#pragma clang fp contract(off)

struct NormArgs {
  const float* x;
  const float* weight;
  const float* bias;
  float eps;
  const float* in_scale;
  const float* in_offset;
  float in_qmin, in_qmax;
  const float* out_scale;
  const float* out_offset;
  float out_qmin, out_qmax;
  float* y;
  int8_t* q_out;
  int8_t* q_tiled;     // same integer image in the fragment-blocked layout of mq_quantize_tiled (nullable)
  int q_shift;
  int32_t* row_sum;
  int64_t rows;
  int cols;
};

// TPR = threads per row: 64 (a wave owns a row, 4 rows per workgroup) for short rows, 256 (a workgroup owns a row,
// reductions through LDS) for cols >= 1024 -- at M = 2048 rows the wave-per-row mapping leaves only 2 waves per SIMD,
// all in the same phase (load, then ~55 VALU ops per element, then store), so nothing overlaps.
// V = float4 vectors held per thread (cols <= 4 * TPR * V); V == 0: the row is re-read instead of kept.
// LN: LayerNorm (QLayerNorm.forward, qmodule.py:624-640 around F.layer_norm) instead of RMSNorm: mean and biased
// variance of the row, y = (xi * rstd + (-rstd * mean)) * gamma + beta -- the expression of torch's CPU kernel.
template <int V, bool LN, int TPR>
__global__ void __launch_bounds__(256) rmsnorm_quant_kernel(const NormArgs a) {
  __shared__ float s_red[3][4];
  __shared__ int s_redi[4];
  const int lane = TPR == 64 ? (threadIdx.x & 63) : threadIdx.x;   // index of this thread inside its row
  const int wv_id = threadIdx.x >> 6;
  const int64_t row = TPR == 64 ? (int64_t)blockIdx.x * 4 + wv_id : (int64_t)blockIdx.x;
  if (TPR == 64 && row >= a.rows) return;      // TPR == 256: grid == rows, and the block-wide reductions need everyone
  auto row_sum_f = [&](float v, int slot) {
    v = wave_sum_f_readlane(v);
    if constexpr (TPR == 64) return v;
    return block_sum4(v, s_red[slot], wv_id);
  };
  const int cols = a.cols, nvec = cols >> 2;
  const float4* xr = reinterpret_cast<const float4*>(a.x + row * cols);
  const float4* wv = reinterpret_cast<const float4*>(a.weight);
  const float4* bv = reinterpret_cast<const float4*>(a.bias);
  const Grid gi = load_grid(a.in_scale, a.in_offset, a.in_qmin, a.in_qmax), go = load_grid(a.out_scale, a.out_offset, a.out_qmin, a.out_qmax);
  auto qin = [&](float v) { return gi.fq_value(v); };

  constexpr int VV = V > 0 ? V : 1;
  float4 xs[VV];
  float ss = 0.f;
  if constexpr (V > 0) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int i = lane + TPR * k;
      if (i < nvec) {
        float4 v = xr[i];
        v.x = qin(v.x); v.y = qin(v.y); v.z = qin(v.z); v.w = qin(v.w);
        xs[k] = v;
        ss += v.x * v.x;
        ss += v.y * v.y;
        ss += v.z * v.z;
        ss += v.w * v.w;
      }
    }
  } else {
    for (int i = lane; i < nvec; i += TPR) {
      float4 v = xr[i];
      v.x = qin(v.x); v.y = qin(v.y); v.z = qin(v.z); v.w = qin(v.w);
      ss += v.x * v.x;
      ss += v.y * v.y;
      ss += v.z * v.z;
      ss += v.w * v.w;
    }
  }
  float r, shiftv = 0.f;
  if constexpr (LN) {
    // ss holds sum(xi^2) so far; LayerNorm wants sum(xi) and then sum((xi - mean)^2): redo the (register) pass
    float s1 = 0.f;
    if constexpr (V > 0) {
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (lane + TPR * k < nvec) s1 += (xs[k].x + xs[k].y) + (xs[k].z + xs[k].w);
    } else {
      for (int i = lane; i < nvec; i += TPR) {
        float4 v = xr[i];
        s1 += (qin(v.x) + qin(v.y)) + (qin(v.z) + qin(v.w));
      }
    }
    const float mu = __fdiv_rn(row_sum_f(s1, 0), (float)cols);
    float s2 = 0.f;
    auto dev2 = [&](float4 v) {
      const float d0 = v.x - mu, d1 = v.y - mu, d2 = v.z - mu, d3 = v.w - mu;
      s2 += d0 * d0;
      s2 += d1 * d1;
      s2 += d2 * d2;
      s2 += d3 * d3;
    };
    if constexpr (V > 0) {
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (lane + TPR * k < nvec) dev2(xs[k]);
    } else {
      for (int i = lane; i < nvec; i += TPR) {
        float4 v = xr[i];
        v.x = qin(v.x); v.y = qin(v.y); v.z = qin(v.z); v.w = qin(v.w);
        dev2(v);
      }
    }
    const float var = __fdiv_rn(row_sum_f(s2, 1), (float)cols);
    r = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(var, a.eps)));
    shiftv = __fmul_rn(-r, mu);
  } else {
    ss = row_sum_f(ss, 2);
    const float mean = __fdiv_rn(ss, (float)cols);
    r = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(mean, a.eps)));
  }

  int acc = 0;
  auto emit = [&](int i, float4 v) {
    const float4 w = wv[i];
    float y0, y1, y2, y3;
    if constexpr (LN) {
      y0 = __fmul_rn(__fadd_rn(__fmul_rn(v.x, r), shiftv), w.x); y1 = __fmul_rn(__fadd_rn(__fmul_rn(v.y, r), shiftv), w.y);
      y2 = __fmul_rn(__fadd_rn(__fmul_rn(v.z, r), shiftv), w.z); y3 = __fmul_rn(__fadd_rn(__fmul_rn(v.w, r), shiftv), w.w);
    } else {
      y0 = __fmul_rn(w.x, __fmul_rn(v.x, r)); y1 = __fmul_rn(w.y, __fmul_rn(v.y, r));
      y2 = __fmul_rn(w.z, __fmul_rn(v.z, r)); y3 = __fmul_rn(w.w, __fmul_rn(v.w, r));
    }
    if (bv) {
      const float4 b = bv[i];
      y0 = __fadd_rn(y0, b.x); y1 = __fadd_rn(y1, b.y); y2 = __fadd_rn(y2, b.z); y3 = __fadd_rn(y3, b.w);
    }
    if (go.on) {
      auto qout = [&](float y) { return index_value_keepnan(y, go.s, go.inv_s, go.o, go.qmin, go.qmax); };
      const float q0 = qout(y0), q1 = qout(y1), q2 = qout(y2), q3 = qout(y3);
      y0 = dequant(q0, go.s, go.o); y1 = dequant(q1, go.s, go.o); y2 = dequant(q2, go.s, go.o); y3 = dequant(q3, go.s, go.o);
      if (a.q_out || a.q_tiled) {   // NaN has no integer image: saturate to the grid's low end like mq_quantize
        const int s0 = (int)fmaxf(q0, a.out_qmin) - a.q_shift, s1 = (int)fmaxf(q1, a.out_qmin) - a.q_shift;
        const int s2 = (int)fmaxf(q2, a.out_qmin) - a.q_shift, s3 = (int)fmaxf(q3, a.out_qmin) - a.q_shift;
        acc += (s0 + s1) + (s2 + s3);
        const unsigned pk = (unsigned)(s0 & 0xff) | ((unsigned)(s1 & 0xff) << 8) | ((unsigned)(s2 & 0xff) << 16) | ((unsigned)(s3 & 0xff) << 24);
        if (a.q_out) reinterpret_cast<unsigned*>(a.q_out + row * cols)[i] = pk;
        if (a.q_tiled) *reinterpret_cast<unsigned*>(a.q_tiled + tiled_image_offset(row, i << 2, cols)) = pk;   // k = 4 i
      }
    }
    if (a.y) reinterpret_cast<float4*>(a.y + row * cols)[i] = make_float4(y0, y1, y2, y3);
  };
  if constexpr (V > 0) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int i = lane + TPR * k;
      if (i < nvec) emit(i, xs[k]);
    }
  } else {
    for (int i = lane; i < nvec; i += TPR) {
      float4 v = xr[i];
      v.x = qin(v.x); v.y = qin(v.y); v.z = qin(v.z); v.w = qin(v.w);
      emit(i, v);
    }
  }
  if (a.row_sum) {
    acc = wave_sum(acc);
    if constexpr (TPR == 64) {
      if (lane == 0) a.row_sum[row] = acc;
    } else {
      const int total = block_sum4(acc, s_redi, wv_id);
      if (threadIdx.x == 0) a.row_sum[row] = total;
    }
  }
}


// Image-only, fragment-blocked output (the decoder-layer pass: llama.fuse_decoder_layer): the kernel above stores a row's tiled image as
// 16-byte pieces at a 256-byte stride -- 10.5 us at [2048, 2048] against 7.6 us for the row-major image.  Here a workgroup of FOUR
// row groups (256 threads each, the arithmetic of rmsnorm_quant_kernel<V, LN, 256> op for op) owns EIGHT rows, two per group, all
// loads issued up front; the int8 results go to an LDS staging tile in the image's order and leave as 128-byte runs (8 rows x 16 B
// = whole cache lines of a fragment block).
// GRPS: row groups per workgroup (4: eight rows, 1024 threads, one workgroup per CU; 2: four rows, 512 threads, TWO per CU whose load /
// arithmetic / store phases overlap -- mq_norm_tiled_set_rows).
template <int V, bool LN, int GRPS = 4>
__global__ void __launch_bounds__(256 * GRPS) norm_tiled8_kernel(const NormArgs a) {
  constexpr int RW = 2 * GRPS;                                      // rows per workgroup
  extern __shared__ __attribute__((aligned(16))) int8_t stage[];   // [cols / 16 pieces][RW rows][16 B]
  __shared__ float s_red[2][3][GRPS][4];                            // [row of the pair][statistic][group][wave]
  __shared__ int s_redi[2][GRPS][4];
  const int grp = threadIdx.x >> 8, lane = threadIdx.x & 255, wv_id = (threadIdx.x >> 6) & 3;
  const int cols = a.cols, nvec = cols >> 2;
  const int64_t row0 = (int64_t)blockIdx.x * RW;
  const float4* wv = reinterpret_cast<const float4*>(a.weight);
  const float4* bv = reinterpret_cast<const float4*>(a.bias);
  const Grid gi = load_grid(a.in_scale, a.in_offset, a.in_qmin, a.in_qmax);
  const float so = a.out_scale[0], oo = a.out_offset[0];            // the output grid is required here (host-checked)
  const float iso = __fdiv_rn(1.0f, so);
  // The arithmetic runs on register PAIRS (v_pk_mul / v_pk_fma / v_pk_add: mq_common.h): the kernel spent ~480 VALU instructions per
  // wave on 16 elements per thread -- as much time as its memory round trip -- and two thirds of them have a packed form with the
  // same bits.  The row statistics keep their element-by-element association (the sums must be those of rmsnorm_quant_kernel).
  // input quantizer, value form.  A NaN / inf element must still poison its row (the reference's clamp propagates NaN): the clamp is a
  // v_med3 (NaN -> qmin) and `probe` = fma(v, 0, probe) turns NaN for such an element; it is added to the row statistic (+ 0.0 otherwise).
  v2f probe2 = {0.f, 0.f};
  auto qin2 = [&](v2f v) -> v2f {
    if (!gi.on) return v;
    probe2 = __builtin_elementwise_fma(v, splat2(0.f), probe2);
    const v2f t = div_by_scale2(v, gi.s, gi.inv_s);                 // index_image_nan2qmin on a register pair
    v2f q = {rintf(t.x), rintf(t.y)};
    q = q + splat2(gi.o);
    q.x = __builtin_amdgcn_fmed3f(q.x, gi.qmin, gi.qmax);
    q.y = __builtin_amdgcn_fmed3f(q.y, gi.qmin, gi.qmax);
    return (q - splat2(gi.o)) * splat2(gi.s);                       // dequant
  };
  const float ubias = (float)(128 - a.q_shift);                    // image_u8f / image_pack4 (mq_common.h)
  float4 xs[2][V];
#pragma unroll
  for (int j = 0; j < 2; ++j) {                                     // every load of both rows goes out before any arithmetic
    const int64_t row = row0 + grp * 2 + j;
    const float4* xr = reinterpret_cast<const float4*>(a.x + (row < a.rows ? row : a.rows - 1) * cols);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int i = lane + 256 * k;
      xs[j][k] = xr[i < nvec ? i : nvec - 1];
    }
  }
  float4 wreg[V];
#pragma unroll
  for (int k = 0; k < V; ++k) wreg[k] = wv[lane + 256 * k < nvec ? lane + 256 * k : nvec - 1];
  auto group_sum = [&](float v, int j, int slot) {                  // block-wide barrier: all four groups run the same sequence
    return block_sum4(wave_sum_f_readlane(v), s_red[j][slot][grp], wv_id);
  };
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t row = row0 + grp * 2 + j;
    float ss = 0.f;
    probe2 = splat2(0.f);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (lane + 256 * k < nvec) {
        const float4 v = xs[j][k];
        const v2f lo = qin2((v2f){v.x, v.y}), hi = qin2((v2f){v.z, v.w});
        xs[j][k] = make_float4(lo.x, lo.y, hi.x, hi.y);
        const v2f sl = lo * lo, sh = hi * hi;
        ss += sl.x;
        ss += sl.y;
        ss += sh.x;
        ss += sh.y;
      }
    }
    const float probe = probe2.x + probe2.y;                        // 0 or NaN
    float r, shiftv = 0.f;
    if constexpr (LN) {
      float s1 = 0.f;
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (lane + 256 * k < nvec) s1 += (xs[j][k].x + xs[j][k].y) + (xs[j][k].z + xs[j][k].w);
      s1 += probe;
      const float mu = __fdiv_rn(group_sum(s1, j, 0), (float)cols);
      float s2 = 0.f;
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (lane + 256 * k < nvec) {
          const float4 v = xs[j][k];
          const v2f d01 = (v2f){v.x, v.y} - splat2(mu), d23 = (v2f){v.z, v.w} - splat2(mu);
          const v2f q01 = d01 * d01, q23 = d23 * d23;
          s2 += q01.x;
          s2 += q01.y;
          s2 += q23.x;
          s2 += q23.y;
        }
      const float var = __fdiv_rn(group_sum(s2, j, 1), (float)cols);
      r = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(var, a.eps)));
      shiftv = __fmul_rn(-r, mu);
    } else {
      ss = group_sum(ss + probe, j, 2);
      const float mean = __fdiv_rn(ss, (float)cols);
      r = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(mean, a.eps)));
    }
    uint32_t usum = 0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int i = lane + 256 * k;
      if (i < nvec) {
        const float4 v = xs[j][k], w = wreg[k];
        v2f y01 = (v2f){v.x, v.y} * splat2(r), y23 = (v2f){v.z, v.w} * splat2(r);
        if constexpr (LN) {
          y01 = (y01 + splat2(shiftv)) * (v2f){w.x, w.y};
          y23 = (y23 + splat2(shiftv)) * (v2f){w.z, w.w};
        } else {
          y01 = (v2f){w.x, w.y} * y01;
          y23 = (v2f){w.z, w.w} * y23;
        }
        if (bv) {
          const float4 b = bv[i];
          y01 = y01 + (v2f){b.x, b.y};
          y23 = y23 + (v2f){b.z, b.w};
        }
        const v2f u01 = image_u8f2(y01, so, iso, oo, a.out_qmin, a.out_qmax, ubias), u23 = image_u8f2(y23, so, iso, oo, a.out_qmin, a.out_qmax, ubias);
        const uint32_t pk = image_pack4(u01.x, u01.y, u23.x, u23.y, usum);
        // staging: piece (k >> 4) = 16-byte chunk column, then the row of the eight, then the byte:  k = 4 i
        *reinterpret_cast<unsigned*>(stage + (i >> 2) * (RW * 16) + ((grp * 2 + j) << 4) + ((i & 3) << 2)) = pk;
      }
    }
    if (a.row_sum) {
      const int acc = wave_sum((int)usum);
      if ((threadIdx.x & 63) == 0) s_redi[j][grp][wv_id] = acc;
    }
  }
  __syncthreads();                                                  // the staging tile and the row-sum partials are complete
  if (a.row_sum && threadIdx.x < RW) {
    const int g = threadIdx.x >> 1, j = threadIdx.x & 1;
    if (row0 + threadIdx.x < a.rows) a.row_sum[row0 + threadIdx.x] = (s_redi[j][g][0] + s_redi[j][g][1]) + (s_redi[j][g][2] + s_redi[j][g][3]) - 128 * cols;
  }
  staged_copy_out<RW, 256 * GRPS, false>(stage, a.q_tiled, row0, a.rows, cols);
}

}  // namespace mq

using namespace mq;

// rows per workgroup of the image-only tiled norm: 0 = by shape (four rows -- two 512-thread workgroups per CU, whose load / arithmetic /
// store phases overlap -- up to 2048 columns: 6.9 -> 6.2 us at [2048, 2048]; eight beyond, where it is a wash), 4 / 8 force one (A/B timing)
static std::atomic<int> g_norm_tiled_rows{0};
extern "C" int mq_norm_tiled_set_rows(int rows) {
  g_norm_tiled_rows = rows == 4 ? 4 : (rows == 8 ? 8 : 0);
  return 0;
}

static int launch_norm(const char* fn, bool ln, const float* x, int64_t rows, int64_t cols, const float* weight, const float* bias,
                       float eps, const float* in_scale, const float* in_offset, float in_qmin, float in_qmax,
                       const float* out_scale, const float* out_offset, float out_qmin, float out_qmax, float* y,
                       int8_t* q_out, int8_t* q_tiled, int q_shift, int32_t* row_sum, mq_stream_t stream) {
  if (rows == 0) return MQ_OK;                   // empty activation (its data pointers may be NULL)
  MQ_REQUIRE(x && weight && (y || q_out || q_tiled), "%s: null pointer", fn);
  MQ_REQUIRE(!q_tiled || (cols % 64 == 0 && aligned(q_tiled, 16)), "%s: the fragment-blocked output needs cols %% 64 == 0 and a 16-byte aligned buffer", fn);
  MQ_REQUIRE(rows >= 0 && cols > 0 && cols % 4 == 0 && cols <= (1 << 20) && rows < (int64_t)0x7fffffff,
             "%s: bad shape %lld x %lld (cols must be a multiple of 4)", fn, (long long)rows, (long long)cols);
  MQ_REQUIRE((in_scale == nullptr) == (in_offset == nullptr) && (out_scale == nullptr) == (out_offset == nullptr),
             "%s: scale/offset must both be set or NULL", fn);
  MQ_REQUIRE(!(q_out || q_tiled) || out_scale, "%s: integer output needs an output quantizer", fn);
  MQ_REQUIRE(!row_sum || q_out || q_tiled, "%s: row sums are those of the integer output", fn);
  MQ_REQUIRE(!(q_out || q_tiled) || (out_qmin - (float)q_shift >= -128.f && out_qmax - (float)q_shift <= 127.f),
             "%s: [%g,%g]-%d does not fit int8", fn, out_qmin, out_qmax, q_shift);
  MQ_REQUIRE(aligned(x, 16) && aligned(weight, 16) && (!bias || aligned(bias, 16)) && (!y || aligned(y, 16)) &&
                 (!q_out || aligned(q_out, 4)),
             "%s: pointers must be 16-byte aligned", fn);
  if (rows == 0) return MQ_OK;
  NormArgs a{x, weight, bias, eps, in_scale, in_offset, in_qmin, in_qmax, out_scale, out_offset, out_qmin, out_qmax,
             y, q_out, q_tiled, q_shift, row_sum, rows, (int)cols};
  hipStream_t st = as_stream(stream);
  // image-only, fragment-blocked: eight rows per workgroup, stores as whole lines of the image (norm_tiled8_kernel)
  if (q_tiled && !y && !q_out && out_scale && cols >= 1024 && cols <= 4096 && cols % 64 == 0 && rows >= 64) {
    const int rows_knob = g_norm_tiled_rows.load();
    const bool four = rows_knob == 4 || (rows_knob == 0 && cols <= 2048);
    const unsigned grid = four ? (unsigned)((rows + 3) / 4) : (unsigned)((rows + 7) / 8);
    const size_t lds = (size_t)cols * (four ? 4 : 8);
#define MQ_NORM8(V)                                                                   \
    do {                                                                              \
      if (four) {                                                                     \
        if (ln) norm_tiled8_kernel<V, true, 2><<<grid, 512, lds, st>>>(a);            \
        else norm_tiled8_kernel<V, false, 2><<<grid, 512, lds, st>>>(a);              \
      } else if (ln) norm_tiled8_kernel<V, true><<<grid, 1024, lds, st>>>(a);         \
      else norm_tiled8_kernel<V, false><<<grid, 1024, lds, st>>>(a);                  \
    } while (0)
    if (cols <= 1024) MQ_NORM8(1);
    else if (cols <= 2048) MQ_NORM8(2);
    else MQ_NORM8(4);
#undef MQ_NORM8
    MQ_LAUNCH_CHECK(fn);
    return MQ_OK;
  }
#define MQ_NORM(V, TPR)                                                                                   \
  do {                                                                                                    \
    const unsigned grid = (TPR) == 64 ? (unsigned)((rows + 3) / 4) : (unsigned)rows;                      \
    if (ln) rmsnorm_quant_kernel<V, true, TPR><<<grid, 256, 0, st>>>(a);                                  \
    else rmsnorm_quant_kernel<V, false, TPR><<<grid, 256, 0, st>>>(a);                                    \
  } while (0)
  if (cols < 1024) MQ_NORM(4, 64);                      // short rows: a wave per row
  else if (cols <= 1024) MQ_NORM(1, 256);               // a workgroup per row from here on
  else if (cols <= 2048) MQ_NORM(2, 256);
  else if (cols <= 4096) MQ_NORM(4, 256);
  else if (cols <= 8192) MQ_NORM(8, 256);
  else MQ_NORM(0, 256);
#undef MQ_NORM
  MQ_LAUNCH_CHECK(fn);
  return MQ_OK;
}

extern "C" int mq_rmsnorm_quant(const float* x, int64_t rows, int64_t cols, const float* weight, const float* bias, float eps,
                                const float* in_scale, const float* in_offset, float in_qmin, float in_qmax,
                                const float* out_scale, const float* out_offset, float out_qmin, float out_qmax, float* y,
                                int8_t* q_out, int8_t* q_tiled, int q_shift, int32_t* row_sum, mq_stream_t stream) {
  return launch_norm("mq_rmsnorm_quant", false, x, rows, cols, weight, bias, eps, in_scale, in_offset, in_qmin, in_qmax, out_scale,
                     out_offset, out_qmin, out_qmax, y, q_out, q_tiled, q_shift, row_sum, stream);
}

extern "C" int mq_layernorm_quant(const float* x, int64_t rows, int64_t cols, const float* weight, const float* bias, float eps,
                                  const float* in_scale, const float* in_offset, float in_qmin, float in_qmax,
                                  const float* out_scale, const float* out_offset, float out_qmin, float out_qmax, float* y,
                                  int8_t* q_out, int8_t* q_tiled, int q_shift, int32_t* row_sum, mq_stream_t stream) {
  return launch_norm("mq_layernorm_quant", true, x, rows, cols, weight, bias, eps, in_scale, in_offset, in_qmin, in_qmax, out_scale,
                     out_offset, out_qmin, out_qmax, y, q_out, q_tiled, q_shift, row_sum, stream);
}
