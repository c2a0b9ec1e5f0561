// The two launches a weight-only (W4A16) model's decode step is made of (the engine: decode_weight_only.py).
//
// mq_w4a16_decode_gemv: mq_w4a16_stream.h's weight-stream walk (w4_stream_walk, described there) over ONE row image, with the whole-dword
// fetch of s16 / z' (scales and zeros 4-byte aligned: this entry's contract), between a prologue and an epilogue chosen per launch.
//   prologue: the fp16 image of the row is formed from fp32 x -- as it is, behind HFRMSNorm or behind nn.LayerNorm; every workgroup
//             recomputes the norm's statistics (x is one row: K floats out of L2), in the expressions of decode_head_kernel (mq_decode.hip)
//   epilogue: + bias; resid + (sum + bias); or, on an image whose rows interleave the gate and the up linear, act(a_n) * b_n -- a wave
//             owns both rows of a pair (row slots 2 q and 2 q + 1), so the product needs no second launch and no exchange.
// mq_w4a16_decode_attention: RoPE on q and the new k, the two cache writes, scores, softmax and p . v over the fp32 cache, one launch.
//   Grid (heads, nsplit), 256 threads.  A group of head_dim / 4 lanes owns a position (one 16-byte load per lane: a cache row is read
//   as one contiguous run), 256 / (head_dim / 4) positions per pass, four passes' loads in flight.  A split's scores stay in LDS:
//   scores -> block max -> exp and block sum -> p . v, each reduced in a fixed order.  The row at *pos is never read from the cache:
//   every workgroup ropes the new k itself, and workgroup (first head of the kv group, split 0) writes it.  nsplit > 1: (max, sum,
//   partial out) records, an integer ticket per head, the last arrival combines them in split order -- mq_decode_attention.h's protocol
//   (write-through record stores, drained by every wave; agent-scope release on the ticket, agent-scope acquire in the last arrival).
#include "mq_w4a16_stream.h"

namespace mq {

struct W4DecArgs {
  const float* x;
  W4Image g;
  int prologue;
  const float* norm_w;
  const float* norm_b;
  float eps;
  const float* bias;
  const float* resid;
  int act;
  float* out;
};

constexpr int WD_THREADS = 1024, WD_WAVES = 16;
constexpr int WD_RED_BYTES = 64;                                   // 16 wave totals behind the fp16 row
constexpr int WD_MAX_K = 32768;
constexpr size_t WD_MAX_LDS = (size_t)WD_MAX_K * 2 + WD_RED_BYTES;

__device__ __forceinline__ float wd_act(float a, int act) {
  if (act == 0) return __fdiv_rn(a, __fadd_rn(1.0f, expf(-a)));                               // SiLU
  return __fmul_rn(__fmul_rn(a, 0.5f), __fadd_rn(1.0f, erff(__fmul_rn(a, 0.70710678118654752440f))));   // GELU, erf form
}

// The prologue: x -> the row image in LDS as fp16 ([K], unit order, 16 floats of reduction slots behind it), plain or behind a norm whose
// statistics every workgroup recomputes.  Every thread of the workgroup calls it; the caller's barrier completes the image.
__device__ __forceinline__ void wd_stage_row(const W4DecArgs& a, char* smem, const int wave, const int lane) {
  const int K = a.g.K;
  float* red = reinterpret_cast<float*>(smem + (size_t)K * 2);
  const int quads = K >> 2;
  float r = 1.f, sh = 0.f;
  if (a.prologue == MQ_W4A16_PRO_RMSNORM) {
    float ss = 0.f;
    for (int i = threadIdx.x; i < quads; i += WD_THREADS) {
      const float4 f = reinterpret_cast<const float4*>(a.x)[i];
      ss += f.x * f.x;
      ss += f.y * f.y;
      ss += f.z * f.z;
      ss += f.w * f.w;
    }
    const float mean = __fdiv_rn(block_reduce<WD_WAVES, BlockSum>(ss, red, wave, lane), (float)K);
    r = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(mean, a.eps)));
  } else if (a.prologue == MQ_W4A16_PRO_LAYERNORM) {
    float s1 = 0.f;
    for (int i = threadIdx.x; i < quads; i += WD_THREADS) {
      const float4 f = reinterpret_cast<const float4*>(a.x)[i];
      s1 += (f.x + f.y) + (f.z + f.w);
    }
    const float mu = __fdiv_rn(block_reduce<WD_WAVES, BlockSum>(s1, red, wave, lane), (float)K);
    float s2 = 0.f;
    for (int i = threadIdx.x; i < quads; i += WD_THREADS) {
      const float4 f = reinterpret_cast<const float4*>(a.x)[i];
      const float d0 = f.x - mu, d1 = f.y - mu, d2 = f.z - mu, d3 = f.w - mu;
      s2 += d0 * d0;
      s2 += d1 * d1;
      s2 += d2 * d2;
      s2 += d3 * d3;
    }
    const float var = __fdiv_rn(block_reduce<WD_WAVES, BlockSum>(s2, red, wave, lane), (float)K);
    r = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(var, a.eps)));
    sh = __fmul_rn(-r, mu);
  }
  for (int i = threadIdx.x; i < quads; i += WD_THREADS) {
    const float4 f = reinterpret_cast<const float4*>(a.x)[i];
    float v[4] = {f.x, f.y, f.z, f.w};
    if (a.prologue != MQ_W4A16_PRO_PLAIN) {
      float w[4] = {1.f, 1.f, 1.f, 1.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
      if (a.norm_w) {
        const float4 t = reinterpret_cast<const float4*>(a.norm_w)[i];
        w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
      }
      if (a.norm_b) {
        const float4 t = reinterpret_cast<const float4*>(a.norm_b)[i];
        b[0] = t.x; b[1] = t.y; b[2] = t.z; b[3] = t.w;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float y;
        if (a.prologue == MQ_W4A16_PRO_RMSNORM) {
          y = __fmul_rn(v[e], r);                                // x * rsqrt(mean + eps), then weight * y
          if (a.norm_w) y = __fmul_rn(w[e], y);
        } else {
          y = __fadd_rn(__fmul_rn(v[e], r), sh);                 // (x - mu) * r as x r - r mu, then * weight
          if (a.norm_w) y = __fmul_rn(y, w[e]);
        }
        if (a.norm_b) y = __fadd_rn(y, b[e]);
        v[e] = y;
      }
    }
    stage_quad(smem, i << 2, v);
  }
}

template <bool GATED>
__global__ void __launch_bounds__(WD_THREADS) w4a16_decode_gemv_kernel(const W4DecArgs a, const int rows_per_wg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];     // [K] fp16, unit order | 16 floats
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int N = a.g.N;
  const int base = blockIdx.x * rows_per_wg;
  const int row_end = base + rows_per_wg < N ? base + rows_per_wg : N;
  // row of this wave's slot t: plain -- base + wave + 16 t; gated -- the two rows of pair wave + 16 (t >> 1) (rows_per_wg is even)
  auto slot_row = [&](int t) { return GATED ? base + 2 * (wave + WD_WAVES * (t >> 1)) + (t & 1) : base + wave + WD_WAVES * t; };
  const int nslots = GATED ? (((row_end - base) >> 1) > wave ? 2 * ((((row_end - base) >> 1) - wave + WD_WAVES - 1) / WD_WAVES) : 0)
                           : (row_end - base > wave ? (row_end - base - wave + WD_WAVES - 1) / WD_WAVES : 0);

  float p_bias = 0.f, p_resid = 0.f;                              // lane t keeps the bias and the residual of row slot t
  float held = 0.f;                                               // gated: a_n while b_n streams

  w4_stream_walk<8, true, 1>(
      a.g, nslots, slot_row,
      [&] {                                                       // behind the first requests: per-row parameters, the row image
        if constexpr (!GATED) {
          if (lane < nslots) {
            const int row = slot_row(lane);
            if (a.bias) p_bias = a.bias[row];
            if (a.resid) p_resid = a.resid[row];
          }
        }
        wd_stage_row(a, smem, wave, lane);
        __syncthreads();
      },
      smem, 1,
      [&](int t, const float (&sums)[1]) {                        // a completed row: the epilogue
        const int row = slot_row(t);
        const float sum = sums[0];
        if constexpr (GATED) {
          if (!(t & 1)) {
            held = sum;                                            // a_n; b_n is the next slot
          } else if (lane == 0) {
            a.out[row >> 1] = __fmul_rn(wd_act(held, a.act), sum);
          }
        } else {
          const float bias = readlane_f(p_bias, t), resid = readlane_f(p_resid, t);
          if (lane == 0) {
            float f = __fadd_rn(sum, bias);
            if (a.resid) f = __fadd_rn(resid, f);
            a.out[row] = f;
          }
        }
      });
}

static const char* wd_rule(int64_t N, int64_t K, int64_t gs, int epilogue) {
  if (!mq_w4a16_supported(1, N, K, gs)) return "mq_w4a16_supported: N % 16 == 0, K % 64 == 0, group_size a multiple of 32 that divides K";
  if (K > WD_MAX_K) return "K <= 32768";
  if (N > (1ll << 30)) return "N <= 2^30";
  if (epilogue == MQ_W4A16_EPI_GATED && N % 32 != 0) return "gated: N % 32 == 0";
  return nullptr;
}

// ---- attention -----------------------------------------------------------------------------------------------------------------------
struct W4AttnArgs {
  const float* qkv;
  float* k_cache;
  float* v_cache;
  const float* rope_row;
  const int* pos;
  int H, KV, D, T, rot;
  int nsplit;
  float* part;
  unsigned* ticket;
  float* out;
  float sqrt_d;
  int max_chunk;                  // ceil(T / nsplit): the floats of LDS behind the fixed part
};

constexpr int WA_THREADS = 256;
constexpr int WA_MAX_CHUNK = 8192;
constexpr int WA_REC_PAD = 4;                                      // a record: {max, sum, -, -, out[D]}

// x[d] of a head roped with this position's row (cos | sin, rot each): two rounded products, one rounded add
__device__ __forceinline__ float wa_rope(const float* x, int d, const float* rope_row, int rot) {
  const float v = x[d];
  if (d >= rot) return v;
  const int half = rot >> 1;
  const float r = d < half ? -x[d + half] : x[d - half];
  return __fadd_rn(__fmul_rn(v, rope_row[d]), __fmul_rn(r, rope_row[rot + d]));
}

__global__ void __launch_bounds__(WA_THREADS) w4a16_decode_attention_kernel(const W4AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int D = a.D, H = a.H, T = a.T;
  float* s_q = reinterpret_cast<float*>(smem);                    // [D] roped q
  float* s_k = s_q + D;                                            // [D] roped new k
  float* s_v = s_k + D;                                            // [D] new v
  float* s_red = s_v + D;                                          // [16]: 4 wave slots, the ticket
  float* s_part = s_red + 16;                                      // [G][D] = 1024 partial outputs
  float* s_sc = s_part + 1024;                                     // [max_chunk] scores, then probabilities
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.x, split = blockIdx.y, nsplit = a.nsplit;
  const int p = a.pos[0];
  if (p < 0 || p >= T) return;                                     // (uniform over the grid: no ticket is taken)
  const int rep = H / a.KV, g = h / rep;
  const float* qh = a.qkv + (size_t)h * D;
  const float* kn = a.qkv + (size_t)(H + g) * D;
  const float* vn = a.qkv + (size_t)(H + a.KV + g) * D;
  if (tid < D) {
    s_q[tid] = wa_rope(qh, tid, a.rope_row, a.rot);
    const float kr = wa_rope(kn, tid, a.rope_row, a.rot), vv = vn[tid];
    s_k[tid] = kr;
    s_v[tid] = vv;
    if (split == 0 && h == g * rep) {                              // the cache append: one workgroup per kv head
      a.k_cache[((size_t)g * T + p) * D + tid] = kr;
      a.v_cache[((size_t)g * T + p) * D + tid] = vv;
    }
  }
  __syncthreads();

  const int n = p + 1;
  const int chunk = (n + nsplit - 1) / nsplit;                     // <= max_chunk
  const int lo = split * chunk < n ? split * chunk : n;
  const int hi = lo + chunk < n ? lo + chunk : n;
  const int LG = D >> 2;                                           // lanes per position: 8, 16, 32 or 64 (a power of two)
  const int NG = WA_THREADS / LG;                                  // positions per pass
  const int gi = tid / LG, li = tid - gi * LG;
  const float* kc = a.k_cache + (size_t)g * T * D + 4 * li;
  const float* vc = a.v_cache + (size_t)g * T * D + 4 * li;

  // ---- scores ----------------------------------------------------------------------------------------------------------------------
  const float4 q4 = reinterpret_cast<const float4*>(s_q)[li];
  const float4 kn4 = reinterpret_cast<const float4*>(s_k)[li];
  float mx = -INFINITY;
  for (int t0 = lo + gi; t0 < hi; t0 += 4 * NG) {
    float4 kk[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = t0 + u * NG;
      kk[u] = kn4;                                                 // (the row at p; past hi: not used)
      if (t < hi && t != p) kk[u] = *reinterpret_cast<const float4*>(kc + (size_t)t * D);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = t0 + u * NG;
      float d = (q4.x * kk[u].x + q4.y * kk[u].y) + (q4.z * kk[u].z + q4.w * kk[u].w);
      for (int m = LG >> 1; m > 0; m >>= 1) d += __shfl_xor(d, m, 64);
      const float s = __fdiv_rn(d, a.sqrt_d);
      if (t < hi) {
        if (li == 0) s_sc[t - lo] = s;
        mx = fmaxf(mx, s);
      }
    }
  }
  mx = block_reduce<WA_THREADS / 64, BlockMax>(mx, s_red, wave, lane);   // -inf for an empty split (barriers inside: s_sc is written)

  // ---- probabilities -----------------------------------------------------------------------------------------------------------------
  float ps = 0.f;
  for (int i = tid; i < hi - lo; i += WA_THREADS) {
    const float e = expf(s_sc[i] - mx);
    s_sc[i] = e;
    ps += e;
  }
  ps = block_reduce<WA_THREADS / 64, BlockSum>(ps, s_red, wave, lane);

  // ---- p . v -------------------------------------------------------------------------------------------------------------------------
  const float4 vn4 = reinterpret_cast<const float4*>(s_v)[li];
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t0 = lo + gi; t0 < hi; t0 += 4 * NG) {
    float4 vv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = t0 + u * NG;
      vv[u] = vn4;
      if (t < hi && t != p) vv[u] = *reinterpret_cast<const float4*>(vc + (size_t)t * D);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = t0 + u * NG;
      if (t < hi) {
        const float w = s_sc[t - lo];
        o.x += w * vv[u].x;
        o.y += w * vv[u].y;
        o.z += w * vv[u].z;
        o.w += w * vv[u].w;
      }
    }
  }
  reinterpret_cast<float4*>(s_part)[gi * LG + li] = o;
  __syncthreads();
  float od = 0.f;
  if (tid < D) {
    for (int k = 0; k < NG; ++k) od += s_part[k * D + tid];        // position groups in order
  }

  if (nsplit == 1) {
    if (tid < D) a.out[(size_t)h * D + tid] = __fdiv_rn(od, ps);
    return;
  }
  // ---- the split's record, the ticket, the last arrival's combine -------------------------------------------------------------------
  typedef unsigned gu32;
  const int rec = D + WA_REC_PAD;
  gu32* mine = (gu32*)(a.part + ((size_t)h * nsplit + split) * rec);
  if (tid < D) __hip_atomic_store(mine + WA_REC_PAD + tid, __float_as_uint(od), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0) {
    __hip_atomic_store(mine, __float_as_uint(mx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + 1, __float_as_uint(ps), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // every storing wave drains its write-through stores
  __syncthreads();
  unsigned* s_ticket = reinterpret_cast<unsigned*>(s_red + 8);
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *s_ticket = __hip_atomic_fetch_add((gu32*)(a.ticket + h), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (*s_ticket != (unsigned)(nsplit - 1)) return;
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store((gu32*)(a.ticket + h), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
  }
  __syncthreads();
  if (tid < D) {
    const gu32* recs = (const gu32*)(a.part + (size_t)h * nsplit * rec);
    float M = -INFINITY;
    for (int c = 0; c < nsplit; ++c) M = fmaxf(M, __uint_as_float(__hip_atomic_load(recs + (size_t)c * rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
    float tot = 0.f, acc = 0.f;
    for (int c = 0; c < nsplit; ++c) {                             // split order; an empty split: max -inf, weight 0
      const float mc = __uint_as_float(__hip_atomic_load(recs + (size_t)c * rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      const float sc = __uint_as_float(__hip_atomic_load(recs + (size_t)c * rec + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      const float oc = __uint_as_float(__hip_atomic_load(recs + (size_t)c * rec + WA_REC_PAD + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      const float w = expf(mc - M);
      tot += w * sc;
      acc += w * oc;
    }
    a.out[(size_t)h * D + tid] = __fdiv_rn(acc, tot);
  }
}

}  // namespace mq

using namespace mq;

extern "C" int mq_w4a16_decode_supported(int64_t N, int64_t K, int64_t group_size, int epilogue) {
  return wd_rule(N, K, group_size, epilogue) == nullptr;
}

extern "C" int mq_w4a16_decode_gemv(const mq_w4a16_decode_gemv_args* p, mq_stream_t stream) {
  MQ_REQUIRE(p, "mq_w4a16_decode_gemv: null pointer (argument block)");
  MQ_REQUIRE(p->prologue >= MQ_W4A16_PRO_PLAIN && p->prologue <= MQ_W4A16_PRO_LAYERNORM && p->epilogue >= MQ_W4A16_EPI_BIAS &&
                 p->epilogue <= MQ_W4A16_EPI_GATED,
             "mq_w4a16_decode_gemv: unknown prologue %d (0 plain, 1 rmsnorm, 2 layernorm) or epilogue %d (0 bias, 1 resid, 2 gated)", p->prologue,
             p->epilogue);
  MQ_REQUIRE(p->x && p->w_packed && p->scales && p->zeros && p->out, "mq_w4a16_decode_gemv: null pointer (x, w_packed, scales, zeros, out)");
  MQ_REQUIRE(aligned(p->x, 16) && aligned(p->w_packed, 16) && aligned(p->out, 16) && aligned(p->scales, 4) && aligned(p->zeros, 4) &&
                 aligned(p->bias, 16) && aligned(p->resid, 16) && aligned(p->norm_weight, 16) && aligned(p->norm_bias, 16),
             "mq_w4a16_decode_gemv: misaligned pointer (x, w_packed, out, bias, resid, norm_weight, norm_bias: 16 bytes; scales, zeros: 4)");
  MQ_REQUIRE(p->prologue == MQ_W4A16_PRO_PLAIN || p->eps > 0.f, "mq_w4a16_decode_gemv: a norm prologue needs eps > 0 (got %g)", (double)p->eps);
  MQ_REQUIRE(p->epilogue != MQ_W4A16_EPI_RESID || p->resid, "mq_w4a16_decode_gemv: the residual epilogue needs resid");
  MQ_REQUIRE(p->epilogue != MQ_W4A16_EPI_GATED || (!p->bias && (p->act == 0 || p->act == 1)),
             "mq_w4a16_decode_gemv: the gated epilogue takes no bias and act 0 (SiLU) or 1 (GELU) (got act %d)", p->act);
  MQ_REQUIRE(p->out != p->x && p->out != p->resid, "mq_w4a16_decode_gemv: out must not be x or resid (other workgroups still read them)");
  const char* why = wd_rule(p->N, p->K, p->group_size, p->epilogue);
  if (why) {
    set_error("mq_w4a16_decode_gemv: N=%lld K=%lld group_size=%lld is not served (mq_w4a16_decode_supported: %s)", (long long)p->N,
              (long long)p->K, (long long)p->group_size, why);
    return MQ_EUNSUPPORTED;
  }
  W4DecArgs a;
  a.x = p->x;
  a.g = w4_image(p->w_packed, p->scales, p->zeros, p->N, p->K, p->group_size);
  a.prologue = p->prologue;
  a.norm_w = p->norm_weight;
  a.norm_b = p->norm_bias;
  a.eps = p->eps;
  a.bias = p->bias;
  a.resid = p->epilogue == MQ_W4A16_EPI_RESID ? p->resid : nullptr;
  a.act = p->act;
  a.out = p->out;
  const bool gated = p->epilogue == MQ_W4A16_EPI_GATED;
  // one fat workgroup per CU; a wave keeps at most 64 row slots (their bias and residual live one per lane); gated: whole pairs
  int rows_per_wg;
  unsigned grid;
  fat_row_geometry(a.g.N, WD_WAVES * 64, &rows_per_wg, &grid);
  if (gated && (rows_per_wg & 1)) {                                // (the cap is even: rounding up stays below it)
    ++rows_per_wg;
    grid = (unsigned)((a.g.N + rows_per_wg - 1) / rows_per_wg);
  }
  const size_t lds = (size_t)a.g.K * 2 + WD_RED_BYTES;
  static std::atomic<size_t> lds_set[2][kMaxDevices];
  const void* fn = gated ? (const void*)w4a16_decode_gemv_kernel<true> : (const void*)w4a16_decode_gemv_kernel<false>;
  if (const int rc = set_lds(fn, lds_set[gated], lds, "mq_w4a16_decode_gemv", WD_MAX_LDS)) return rc;
  hipStream_t st = as_stream(stream);
  if (gated) w4a16_decode_gemv_kernel<true><<<grid, WD_THREADS, lds, st>>>(a, rows_per_wg);
  else w4a16_decode_gemv_kernel<false><<<grid, WD_THREADS, lds, st>>>(a, rows_per_wg);
  MQ_LAUNCH_CHECK("mq_w4a16_decode_gemv");
  return MQ_OK;
}

extern "C" int mq_w4a16_decode_attention(const mq_w4a16_decode_attention_args* p, mq_stream_t stream) {
  MQ_REQUIRE(p, "mq_w4a16_decode_attention: null pointer (argument block)");
  MQ_REQUIRE(p->qkv && p->k_cache && p->v_cache && p->rope_row && p->pos && p->out,
             "mq_w4a16_decode_attention: null pointer (qkv, k_cache, v_cache, rope_row, pos, out)");
  MQ_REQUIRE(aligned(p->qkv, 16) && aligned(p->k_cache, 16) && aligned(p->v_cache, 16) && aligned(p->out, 16) && aligned(p->part, 16) &&
                 aligned(p->rope_row, 4) && aligned(p->pos, 4) && aligned(p->ticket, 4),
             "mq_w4a16_decode_attention: misaligned pointer (qkv, k_cache, v_cache, out, part: 16 bytes; rope_row, pos, ticket: 4)");
  MQ_REQUIRE(p->heads >= 1 && p->kv_heads >= 1 && p->heads <= 65535, "mq_w4a16_decode_attention: heads=%d kv_heads=%d must be >= 1 (heads <= 65535)",
             p->heads, p->kv_heads);
  MQ_REQUIRE(p->cache_len >= 1 && p->cache_len <= (1 << 24), "mq_w4a16_decode_attention: cache_len=%d outside 1 .. 2^24", p->cache_len);
  const char* why = nullptr;
  if (p->head_dim != 32 && p->head_dim != 64 && p->head_dim != 128 && p->head_dim != 256) why = "head_dim 32, 64, 128 or 256";
  else if (p->heads % p->kv_heads != 0) why = "heads % kv_heads == 0";
  else if (p->rot_dim < 2 || p->rot_dim > p->head_dim || p->rot_dim % 2 != 0) why = "rot_dim even, 2 <= rot_dim <= head_dim";
  else if (p->nsplit < 1 || p->nsplit > 16) why = "1 <= nsplit <= 16";
  else if ((p->cache_len + p->nsplit - 1) / p->nsplit > WA_MAX_CHUNK) why = "ceil(cache_len / nsplit) <= 8192";
  if (why) {
    set_error("mq_w4a16_decode_attention: heads=%d kv_heads=%d head_dim=%d rot_dim=%d cache_len=%d nsplit=%d is not served (%s)", p->heads,
              p->kv_heads, p->head_dim, p->rot_dim, p->cache_len, p->nsplit, why);
    return MQ_EUNSUPPORTED;
  }
  MQ_REQUIRE(p->nsplit == 1 || (p->part && p->ticket), "mq_w4a16_decode_attention: nsplit=%d needs part and ticket", p->nsplit);
  W4AttnArgs a;
  a.qkv = p->qkv;
  a.k_cache = p->k_cache;
  a.v_cache = p->v_cache;
  a.rope_row = p->rope_row;
  a.pos = p->pos;
  a.H = p->heads;
  a.KV = p->kv_heads;
  a.D = p->head_dim;
  a.T = p->cache_len;
  a.rot = p->rot_dim;
  a.nsplit = p->nsplit;
  a.part = p->part;
  a.ticket = p->ticket;
  a.out = p->out;
  a.sqrt_d = (float)sqrt((double)p->head_dim);
  a.max_chunk = (p->cache_len + p->nsplit - 1) / p->nsplit;
  const size_t lds = ((size_t)3 * a.D + 16 + 1024 + a.max_chunk) * sizeof(float);
  constexpr size_t max_lds = ((size_t)3 * 256 + 16 + 1024 + WA_MAX_CHUNK) * sizeof(float);
  static std::atomic<size_t> lds_set[kMaxDevices];
  if (const int rc = set_lds((const void*)w4a16_decode_attention_kernel, lds_set, lds, "mq_w4a16_decode_attention", max_lds)) return rc;
  w4a16_decode_attention_kernel<<<dim3((unsigned)a.H, (unsigned)a.nsplit), WA_THREADS, lds, as_stream(stream)>>>(a);
  MQ_LAUNCH_CHECK("mq_w4a16_decode_attention");
  return MQ_OK;
}
