// The five-launch decode attention, phase by phase: ONE text for decode_attention_kernel<D> (mq_decode.hip: one token of one
// sequence), decode_attention_batch_kernel<D> (mq_decode_batch.hip: one token of each of B sequences) and
// decode_attention_rows_kernel<D, VCH, TABLE> (mq_decode_rows.hip: consecutive positions of one sequence, or table rows over a batch of
// caches).  Their contract -- row b / row j / row r computes the single-sequence launch's bits -- holds because they run THESE expressions
// in THESE reduction orders; a kernel adds only its indexing, where its new keys and values live, and what is truly its own.
// The phases are statement macros (MQ_ATTN_*), expanded in the kernel's own scope, not functions: the kernels then compile to the
// instruction streams of the spelled-out text (loop peeling, register count and block layout depend on the form), and a `return` in a
// phase leaves the kernel.  Each phase lists the names it needs and the names it defines; common to all: D (head_dim), the argument
// block `a`, tid / lane / wv (thread, lane, wave of the 256-thread workgroup), h / c (head, split), H (heads), nsplit.  In order:
//   MQ_ATTN_GEOMETRY, MQ_ATTN_LDS              thread mappings; the static LDS (declared in the kernel: part of the cache bound)
//   MQ_ATTN_KEY_LOADER, MQ_ATTN_VALUE_LOADER   the requests for cached keys and values, the first issued before anything waits
//   MQ_ATTN_GRIDS                              the seven grids from the launch-constants line
//   MQ_ATTN_NEW_TOKEN                          RoPE + the three input quantizers of one new token, its cache append
//   MQ_ATTN_QSUM_REDUCE, MQ_ATTN_CONSTS        the query's index sum; zero points, alpha_qk / alpha_pv, qconst
//   MQ_ATTN_SCORES                             all scores of the head into s_sc, the waves' maxima into s_redf
//   MQ_ATTN_SOFTMAX                            exp / sum, then pv_bmm's input index of THIS split's positions over s_sc
//   MQ_ATTN_SPLIT_BLOCKS, MQ_ATTN_PV_FLAT      exact integer p.v over this split's cached blocks
//   MQ_ATTN_PV_ADD_NEW, MQ_ATTN_FOLD_GROUPS    one new position from LDS; the zero-point fold and the groups' sums to s_acc
//   MQ_ATTN_FINISH                             position groups -> head; the split protocol; pv_bmm's output grid, the consumer's image
// Also the host checks the entries share and the launch of those with a (heads, nsplit, rows) grid.  Compiled under each includer's
// flags, as the prologue in mq_decode_common.h.
#pragma once
#include "mq_decode_common.h"

namespace mq {

#pragma clang fp contract(off)

// One element d of a new token's q / k / v row on its 8-bit attention input grid, as stored (index - 128): RoPE (rotate-half over the
// first rot dimensions: x * cos + rot(x) * sin) then the grid -- MQ_ATTN_NEW_TOKEN's expressions as a function, for the launch
// that builds new rows in a loop (mq_decode_rows.hip).  par: the element's RoPE partner; rot = 0: no rotation (v).
__device__ __forceinline__ int8_t attn_new_elem(float raw, float par, float cs, float sn, int d, int rot, const Grid& g) {
  float x = raw;
  if (d < rot) {
    const float sg = d < (rot >> 1) ? -1.f : 1.f;                  // (-x) * sin == -(x * sin) exactly
    x = __fadd_rn(__fmul_rn(raw, cs), __fmul_rn(sg * par, sn));
  }
  const float i = index_decode_keepnan(x, g.s, g.inv_s, g.o, g.qmin, g.qmax);
  return (int8_t)((i != i ? 0 : (int)i) - 128);
}
// The score of one position from its exact integer dot (q index . k index) and key byte sum: qk_bmm's output grid, then / sqrt(D)
// (hf_model.py:513); sqrt(D) a power of two: the divide is an exact multiply.
template <int D>
__device__ __forceinline__ float attn_score(int dot, int ks, int zq, int qconst, float alpha_qk, const Grid& qo) {
  constexpr bool pow2 = (D == 64 || D == 256);
  const int ti = dot - zq * ks + qconst;
  const float qv = qo.fq(__fmul_rn((float)ti, alpha_qk));
  return pow2 ? __fmul_rn(qv, 1.0f / (D == 64 ? 8.0f : 16.0f)) : __fdiv_rn(qv, __fsqrt_rn((float)D));
}

// D = head_dim (compile time: every index below is a shift).  Scores: LPP lanes per cached position (4; 2 at D = 32), each with CH
// 16-byte chunks of the key row (LPP * CH * 16 = D); 256 / LPP positions per pass, KB passes in flight.  p.v: a thread owns one dword
// (4 dims) of the value rows of G = 1024 / D position groups; a 64-position block gives each thread PPB = D / 16 positions.
#define MQ_ATTN_GEOMETRY(D)                                                                       \
  constexpr int LPP = D >= 64 ? 4 : 2, CH = D >= 64 ? D / 64 : 1, PPP = 256 / LPP, KB = 8 / CH;   \
  constexpr int DQ = D / 4, G = 256 / DQ, PPB = 64 / G, VB = 16;                                  \
  static_assert(PPB * G == 64 && VB % PPB == 0, "block mapping")

// s_sc [cache_len]: scores -> exp -> (p index - zp) as int; the kernel's D-byte rows (its q and its new k / v: the argument);
// s_acc [G][D]: partial p.v sums
#define MQ_ATTN_LDS(...)                                                \
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];      \
  float* s_sc = reinterpret_cast<float*>(smem_raw);                    \
  __shared__ __attribute__((aligned(16))) int8_t __VA_ARGS__;          \
  __shared__ float s_redf[4];                                          \
  __shared__ int s_redq[4];                                            \
  __shared__ long long s_acc[1024];                                    \
  __shared__ unsigned s_ticket

// this lane's chunk ch of a D-byte row in LDS (needs sub)
#define MQ_ATTN_LDS_FRAG(ROW, ch) (*reinterpret_cast<const v4i*>((ROW) + (sub * CH + (ch)) * 16))

// Needs kc (the KV head's keys).  Defines sub, slot, kbuf, load_keys(t0): KB passes of key rows from t0 on, and issues load_keys(0).
// CACHED: whether position t is read from memory (the new ones are appended by this very launch: they come from registers or LDS);
// position 0 stands in elsewhere (always valid memory) and is masked in MQ_ATTN_SCORES.
#define MQ_ATTN_KEY_LOADER(CACHED)                                                                                                   \
  const int sub = tid & (LPP - 1), slot = tid / LPP;                                                                                 \
  v4i kbuf[KB][CH];                                                                                                                  \
  auto load_keys = [&](int t0) {                                                                                                     \
    _Pragma("unroll") for (int u = 0; u < KB; ++u) {                                                                                 \
      const int t = t0 + u * PPP + slot;                                                                                             \
      const int tc = (CACHED) ? t : 0;                                                                                               \
      _Pragma("unroll") for (int ch = 0; ch < CH; ++ch) kbuf[u][ch] = *reinterpret_cast<const v4i*>(kc + (size_t)tc * D + (sub * CH + ch) * 16); \
    }                                                                                                                                \
  };                                                                                                                                 \
  load_keys(0)

// Needs vc (the KV head's values, flat layout).  Defines dq, grp, vbuf, item_pos(i), load_values(i0): thread (dq = dword of 4 dims, grp)
// reads positions 64 b + grp + G j of this split's blocks b = c, c + nsplit, ...; only the NCACHED first positions come from memory.
#define MQ_ATTN_VALUE_LOADER(NCACHED)                                                                                                \
  const int dq = tid & (DQ - 1), grp = tid / DQ;                                                                                     \
  int vbuf[VB];                                                                                                                      \
  auto item_pos = [&](int i) { return 64 * (c + nsplit * (i / PPB)) + grp + G * (i % PPB); }; /* PPB: a power of two (shifts) */      \
  auto load_values = [&](int i0) {                                                                                                   \
    _Pragma("unroll") for (int u = 0; u < VB; ++u) {                                                                                 \
      const int t = item_pos(i0 + u);                                                                                                \
      vbuf[u] = *reinterpret_cast<const int*>(vc + (size_t)(t < (NCACHED) ? t : 0) * D + dq * 4);                                    \
    }                                                                                                                                \
  }

// needs cv (the lane's float of the launch-constants line)
#define MQ_ATTN_GRIDS                                                                                                                          \
  const Grid qa = const_grid(cv, AG_QK_A, a.qk_a), qb = const_grid(cv, AG_QK_B, a.qk_b), qo = const_grid(cv, AG_QK_OUT, a.qk_out);             \
  const Grid pa = const_grid(cv, AG_PV_A, a.pv_a), pb = const_grid(cv, AG_PV_B, a.pv_b), po = const_grid(cv, AG_PV_OUT, a.pv_out);             \
  const Grid oi = const_grid(cv, AG_O_IN, a.o_in)

// One new token at position pos: needs its raw q / k / v elements and RoPE partners (q_raw, q_par, k_raw, k_par, v_raw), cs / sn, rot,
// half, kvh.  x * cos + rot(x) * sin, rot(x)[d] = d < rot/2 ? -x[d + rot/2] : x[d - rot/2]; (-x) * sin == -(x * sin) exactly.  Threads
// d < D leave element d on its grid in s_q8 / s_k8 / s_v8 (index - 128: the new key and value never come back through memory); the KV
// group's first head appends them to the caches K_CACHE / V_CACHE.  Defines qsum_part.
#define MQ_ATTN_NEW_TOKEN(K_CACHE, V_CACHE)                                                                                               \
  int qsum_part = 0;                                                                                                                      \
  if (tid < D) {                                                                                                                          \
    float qv = q_raw, kv = k_raw;                                                                                                         \
    if (tid < rot) {                                                                                                                      \
      const float sg = tid < half ? -1.f : 1.f;                                                                                           \
      qv = __fadd_rn(__fmul_rn(q_raw, cs), __fmul_rn(sg * q_par, sn));                                                                    \
      kv = __fadd_rn(__fmul_rn(k_raw, cs), __fmul_rn(sg * k_par, sn));                                                                    \
    }                                                                                                                                     \
    const float iq = index_decode_keepnan(qv, qa.s, qa.inv_s, qa.o, qa.qmin, qa.qmax), ik = index_decode_keepnan(kv, qb.s, qb.inv_s, qb.o, qb.qmin, qb.qmax);     \
    const float iv = index_decode_keepnan(v_raw, pb.s, pb.inv_s, pb.o, pb.qmin, pb.qmax);                                                             \
    const int sq = (iq != iq ? 0 : (int)iq) - 128, sk = (ik != ik ? 0 : (int)ik) - 128, sv = (iv != iv ? 0 : (int)iv) - 128;              \
    s_q8[tid] = (int8_t)sq;                                                                                                               \
    s_k8[tid] = (int8_t)sk;                                                                                                               \
    s_v8[tid] = (int8_t)sv;                                                                                                               \
    qsum_part = sq;                                                                                                                       \
    if (c == 0 && h % (H / a.kv_heads) == 0) {                                                                                            \
      (K_CACHE)[((size_t)kvh * a.cache_len + pos) * D + tid] = (int8_t)sk;                                                                \
      (V_CACHE)[((size_t)kvh * a.cache_len + pos) * D + tid] = (int8_t)sv;                                                                \
    }                                                                                                                                     \
  }

// the waves' sums of the query indices (qsum_part) to s_redq; ends on the barrier after which they and the new rows in LDS are complete
#define MQ_ATTN_QSUM_REDUCE                 \
  {                                         \
    const int w = wave_sum_dpp(qsum_part);  \
    if (lane == 0) s_redq[wv] = w;          \
  }                                         \
  __syncthreads()

// sum (iq - zq)(ik - zk) = sum sq sk - zk sum sq - zq sum sk + D zq zk: qconst holds the terms without the key
#define MQ_ATTN_CONSTS                                                                                       \
  const int qsum = (s_redq[0] + s_redq[1]) + (s_redq[2] + s_redq[3]);                                        \
  const int zq = (int)qa.o - 128, zk = (int)qb.o - 128, zv = (int)pb.o - 128, zp = (int)pa.o;                \
  const float alpha_qk = __fmul_rn(qa.s, qb.s), alpha_pv = __fmul_rn(pa.s, pb.s);                            \
  const int qconst = D * zq * zk - zk * qsum

// Scores of positions 0 .. T-1 into s_sc.  Needs qf[CH] (this lane's share of the query), kbuf = load_keys(0).  KEY_FRAG: the key
// fragment of position t, chunk ch -- kbuf[u][ch] for a cached one, the kernel's own for a position this launch appends.  Every
// workgroup of a head computes ALL scores (bit-identical statistics in every split, no exchange).  Ends on the barrier after which s_sc
// and the waves' maxima (s_redf) are complete.
#define MQ_ATTN_SCORES(KEY_FRAG)                                                                             \
  const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};                                         \
  float lmax = -INFINITY;                                                                                    \
  for (int t0 = 0; t0 < T; t0 += KB * PPP) {                                                                 \
    if (t0 > 0) load_keys(t0);                                                                               \
    _Pragma("unroll") for (int u = 0; u < KB; ++u) {                                                         \
      if (t0 + u * PPP >= T) break; /* (uniform) the rest of the batch lies beyond the sequence */           \
      const int t = t0 + u * PPP + slot;                                                                     \
      int dot = 0, ks = 0;                                                                                   \
      _Pragma("unroll") for (int ch = 0; ch < CH; ++ch) {                                                    \
        const v4i kf = (KEY_FRAG);                                                                           \
        dot = dot16(kf, qf[ch], dot);                                                                        \
        ks = dot16(kf, ones, ks);                                                                            \
      }                                                                                                      \
      dot = quad_sum<LPP>(dot);                                                                              \
      ks = quad_sum<LPP>(ks);                                                                                \
      if (t < T && sub == 0) {                                                                               \
        const float sc = attn_score<D>(dot, ks, zq, qconst, alpha_qk, qo);                                   \
        s_sc[t] = sc;                                                                                        \
        lmax = fmaxf(lmax, sc);                                                                              \
      }                                                                                                      \
    }                                                                                                        \
  }                                                                                                          \
  lmax = wave_max_f(lmax);                                                                                   \
  if (lane == 0) s_redf[wv] = lmax;                                                                          \
  __syncthreads()

// softmax over s_sc[0 .. T-1] in fp32 (exp(s - max) / sum, the sum in thread / wave order), then pv_bmm's input quantizer once per
// position of THIS split's 64-position blocks: defines s_pi = s_sc as (index - zp) ints.  Ends on the barrier that completes them.
#define MQ_ATTN_SOFTMAX                                                                            \
  const float mx = fmaxf(fmaxf(s_redf[0], s_redf[1]), fmaxf(s_redf[2], s_redf[3]));                \
  __syncthreads();                                                                                 \
  float lsum = 0.f;                                                                                \
  for (int t = tid; t < T; t += 256) {                                                             \
    const float e = expf(s_sc[t] - mx);                                                            \
    s_sc[t] = e;                                                                                   \
    lsum += e;                                                                                     \
  }                                                                                                \
  lsum = wave_sum_f_rowbcast(lsum);                                                                         \
  if (lane == 0) s_redf[wv] = lsum;                                                                \
  __syncthreads();                                                                                 \
  const float tot_e = (s_redf[0] + s_redf[1]) + (s_redf[2] + s_redf[3]);                           \
  int* s_pi = reinterpret_cast<int*>(s_sc);                                                        \
  for (int t = tid; t < T; t += 256) {                                                             \
    if (nsplit == 1 || ((t >> 6) % nsplit) == c) {                                                 \
      const float pr = __fdiv_rn(s_sc[t], tot_e);                                                  \
      const float ip = index_decode_keepnan(pr, pa.s, pa.inv_s, pa.o, pa.qmin, pa.qmax);                       \
      s_pi[t] = (ip != ip ? 0 : (int)ip) - zp;                                                     \
    }                                                                                              \
  }                                                                                                \
  __syncthreads()

// this split's share (my_blocks) of the 64-position blocks that hold the NCACHED first positions
#define MQ_ATTN_SPLIT_BLOCKS(NCACHED)            \
  const int nblk = ((NCACHED) + 63) >> 6;        \
  const int my_blocks = c < nblk ? (nblk - 1 - c) / nsplit + 1 : 0

// p.v over the NCACHED first positions, `items` items of this thread (my_blocks * PPB), flat value layout, into acc[4] / psum (long long):
// exact integers.  sum_t pi[t] (vs[t][d] - zv) = sum_t pi[t] vs[t][d] - zv sum_t pi[t]: v_bfe_i32 + v_mad_i32_i24 per element, one add
// per position; a32 / p32: <= 16 positions x 65535 x 128 < 2^31.  vbuf = load_values(0).  (the sbfe builtin returns unsigned)
#define MQ_ATTN_PV_FLAT(NCACHED)                                                                                     \
  for (int i0 = 0; i0 < items; i0 += VB) {                                                                           \
    if (i0 > 0) load_values(i0);                                                                                     \
    int a32[4] = {0, 0, 0, 0}, p32 = 0;                                                                              \
    _Pragma("unroll") for (int u = 0; u < VB; ++u) {                                                                 \
      const int t = item_pos(i0 + u);                                                                                \
      const bool ok = i0 + u < items && t < (NCACHED);                                                               \
      const int pi = s_pi[ok ? t : 0];                                                                               \
      const int pim = ok ? pi : 0;                                                                                   \
      p32 += pim;                                                                                                    \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) a32[e] += (int)__builtin_amdgcn_sbfe(vbuf[u], 8 * e, 8) * pim;   \
    }                                                                                                                \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) acc[e] += a32[e];                                                  \
    psum += p32;                                                                                                     \
  }

// a position this launch appends (value row S_V in LDS, probability index PI): added by position group 0 of the split that owns its block
#define MQ_ATTN_PV_ADD_NEW(S_V, PI)                                                                                            \
  {                                                                                                                            \
    const int sv4 = *reinterpret_cast<const int*>((S_V) + dq * 4);                                                             \
    const int pi = (PI);                                                                                                       \
    psum += pi;                                                                                                                \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) acc[e] += (long long)((int)__builtin_amdgcn_sbfe(sv4, 8 * e, 8) * pi);       \
  }

// the zero-point fold, then this thread's four sums to s_acc[grp][D]; the kernel's barrier completes them
#define MQ_ATTN_FOLD_GROUPS                                                              \
  _Pragma("unroll") for (int e = 0; e < 4; ++e) acc[e] -= (long long)zv * psum;          \
  _Pragma("unroll") for (int e = 0; e < 4; ++e) s_acc[grp * D + dq * 4 + e] = acc[e]

// From the NGRP x D partial sums in s_acc (complete: the kernel's barrier) to the head's output row: thread d < D adds the groups.
// nsplit == 1: the workgroup finishes the head.  nsplit > 1: exact int64 partial sums go to the launch row's split scratch PART with
// write-through stores, the row's per-head tickets TICKET count the splits, the last one adds the partials (integers: any order is THE
// sum) and finishes (cdna guide G16 R1); the others leave the kernel.  Then pv_bmm's output grid on one rounding of the exact sum (as
// mq_attention.hip) and the index on the consumer linear's input grid (o_proj's int8 image), both at element OUT of out / out_q.
// SPLIT_LOCALS / OUT_LOCALS: declarations a kernel with rows makes for PART, TICKET / OUT -- on the split path / in the epilogue only,
// so that the row arithmetic stays off the other paths; empty for the single-sequence kernel.
// The ticket's RELEASE at agent scope: the partials are already write-through (8-byte agent atomics, drained by the vmcnt
// wait and ordered for the whole workgroup by the barrier), which is what makes this correct on gfx950; the release gives the formal
// release -> acquire edge to the last split's fence as well.  One L2 write-back per split workgroup, on the long-context path only.
// The last split resets the ticket: ready for the next launch.
#define MQ_ATTN_FINISH(NGRP, SPLIT_LOCALS, PART, TICKET, OUT_LOCALS, OUT)                                                                  \
  long long tot = 0;                                                                                                                       \
  if (tid < D) {                                                                                                                           \
    _Pragma("unroll") for (int gq = 0; gq < (NGRP); ++gq) tot += s_acc[gq * D + tid];                                                      \
  }                                                                                                                                        \
  if (nsplit > 1) {                                                                                                                        \
    SPLIT_LOCALS                                                                                                                           \
    if (tid < D) __hip_atomic_store((PART) + ((size_t)c * H + h) * D + tid, (unsigned long long)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                                       \
    __syncthreads();                                                                                                                       \
    if (tid == 0) s_ticket = __hip_atomic_fetch_add((TICKET) + h, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);                           \
    __syncthreads();                                                                                                                       \
    if (s_ticket != (unsigned)(nsplit - 1)) return;                                                                                        \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");                                                                                     \
    if (tid == 0) __hip_atomic_store((TICKET) + h, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                                          \
    if (tid < D) {                                                                                                                         \
      tot = 0;                                                                                                                             \
      for (int cc = 0; cc < nsplit; ++cc)                                                                                                  \
        tot += (long long)__hip_atomic_load((PART) + ((size_t)cc * H + h) * D + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);            \
    }                                                                                                                                      \
  }                                                                                                                                        \
  if (tid < D) {                                                                                                                           \
    OUT_LOCALS                                                                                                                             \
    const float pre = (float)((double)tot * (double)alpha_pv);                                                                             \
    const float y = po.fq(pre);                                                                                                            \
    if (a.out) a.out[OUT] = y;                                                                                                               \
    if (a.out_q) {                                                                                                                         \
      const float qi = index_decode_keepnan(y, oi.s, oi.inv_s, oi.o, oi.qmin, oi.qmax);                                                                \
      a.out_q[OUT] = (int8_t)((qi != qi ? (int)oi.qmin : (int)qi) - 128);                                                                    \
    }                                                                                                                                      \
  }

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// The largest cache_len the five-launch attention serves: LDS per workgroup on gfx950 (160 KiB) = static + 4 B per cached position
// (scores); the static arrays are <= 9008 B (single, batched) / 12592 B (rows: the new rows' keys and values) at head_dim 256, so
// 4 x 32768 fits everywhere and this is the bound.  mobilequant_amd/decode.py mirrors it to choose the chain.
constexpr int kAttnMaxCache = 32768;

// What mq_decode_attention, _batch, _multi and _ragged require of the argument block they share, in two parts (the value layout's
// checks of check_row_run_attention stand between them); `entry` names the caller in the message.
inline int check_five_launch_attention_shape(const char* entry, const mq_decode_attention_args& a) {
  MQ_REQUIRE(a.qkv && a.k_cache && a.v_cache && a.cos && a.sin && a.pos && a.consts && (a.out || a.out_q), "%s: null pointer", entry);
  MQ_REQUIRE(a.heads > 0 && a.kv_heads > 0 && a.heads % a.kv_heads == 0 && (a.head_dim == 32 || a.head_dim == 64 || a.head_dim == 128 || a.head_dim == 256) &&
                 a.cache_len > 0 && a.cache_len <= kAttnMaxCache && a.rot_dim > 0 && a.rot_dim <= a.head_dim && a.rot_dim % 2 == 0,
             "%s: heads=%d kv_heads=%d head_dim=%d (32 / 64 / 128 / 256) cache_len=%d (<= %d) rot_dim=%d", entry, a.heads, a.kv_heads, a.head_dim,
             a.cache_len, kAttnMaxCache, a.rot_dim);
  return MQ_OK;
}
inline int check_five_launch_attention_grids(const char* entry, const mq_decode_attention_args& a) {
  MQ_REQUIRE(a.nsplit >= 1 && a.nsplit <= 16 && (a.nsplit == 1 || (a.part && a.ticket)), "%s: nsplit=%d (1..16; > 1 needs part and ticket)", entry, a.nsplit);
  MQ_REQUIRE(a.qk_a.scale && a.qk_b.scale && a.pv_a.scale && a.pv_b.scale && a.qk_a.qmin == 0.f && a.qk_a.qmax == 255.f && a.qk_b.qmin == 0.f &&
                 a.qk_b.qmax == 255.f && a.pv_b.qmin == 0.f && a.pv_b.qmax == 255.f && a.pv_a.qmin == 0.f && a.pv_a.qmax <= 65535.f,
             "%s: q / k / v need 8-bit unsigned grids, the probabilities an unsigned grid of at most 16 bits", entry);
  MQ_REQUIRE(!a.out_q || (a.o_in.scale && a.o_in.qmin == 0.f && a.o_in.qmax == 255.f), "%s: the int8 output image needs the consumer's 8-bit unsigned grid (o_in)", entry);
  MQ_REQUIRE(aligned(a.k_cache, 16) && aligned(a.v_cache, 16) && aligned(a.consts, 16) && aligned(a.qkv, 4), "%s: caches / consts must be 16-byte aligned", entry);
  return MQ_OK;
}
inline int check_five_launch_attention(const char* entry, const mq_decode_attention_args& a) {
  const int rc = check_five_launch_attention_shape(entry, a);
  return rc != MQ_OK ? rc : check_five_launch_attention_grids(entry, a);
}
// What mq_decode_attention_multi and _ragged (mq_decode_rows.hip) both require: the row count, the shared block (the value layout's
// checks between its two parts; the ragged entry serves the flat layout only and passes 0), no prefetch rows, a stride that covers a row.
inline int check_row_run_attention(const char* entry, const mq_decode_attention_args& a, int rows, int64_t qkv_stride, int v_chunked) {
  MQ_REQUIRE(rows >= 1 && rows <= MQ_DECODE_MAX_BATCH, "%s: rows=%d outside 1..%d", entry, rows, MQ_DECODE_MAX_BATCH);
  int rc = check_five_launch_attention_shape(entry, a);
  if (rc != MQ_OK) return rc;
  MQ_REQUIRE(v_chunked == 0 || v_chunked == 1, "%s: v_chunked=%d (0 or 1)", entry, v_chunked);
  MQ_REQUIRE(!v_chunked || a.cache_len % 16 == 0, "%s: v_chunked needs cache_len %% 16 == 0 (cache_len=%d)", entry, a.cache_len);
  rc = check_five_launch_attention_grids(entry, a);
  if (rc != MQ_OK) return rc;
  MQ_REQUIRE(a.prefetch_wgs == 0, "%s: no prefetch rows (prefetch_wgs must be 0)", entry);
  MQ_REQUIRE(rows == 1 || qkv_stride >= (int64_t)(a.heads + 2 * a.kv_heads) * a.head_dim, "%s: qkv_stride must cover a q | k | v row", entry);
  return MQ_OK;
}

// The launch of the entries with a (heads, nsplit, rows) grid -- mq_decode_attention_batch, _multi, _ragged -- on a checked block:
// 4 bytes of dynamic LDS per cached position (the scores), the kernel's LDS ceiling raised once per kernel and device (the function-local
// cache: one per instantiation).  Kernels: a type whose member template kernel<D> is the entry's kernel at head_dim D.
template <auto Kernel, class Args>
inline int launch_attention_rows_kernel(const char* entry, const Args& args, const mq_decode_attention_args& a, int rows, mq_stream_t stream) {
  static std::atomic<size_t> lds_set[kMaxDevices];
  const size_t lds = (size_t)a.cache_len * sizeof(float);
  const int rc = set_lds(reinterpret_cast<const void*>(Kernel), lds_set, lds, entry);
  if (rc != MQ_OK) return rc;
  Kernel<<<dim3((unsigned)a.heads, (unsigned)a.nsplit, (unsigned)rows), 256, lds, as_stream(stream)>>>(args);
  MQ_LAUNCH_CHECK(entry);
  return MQ_OK;
}
template <class Kernels, class Args>
inline int launch_attention_rows(const char* entry, const Args& args, const mq_decode_attention_args& a, int rows, mq_stream_t stream) {
  switch (a.head_dim) {
    case 32: return launch_attention_rows_kernel<Kernels::template kernel<32>>(entry, args, a, rows, stream);
    case 64: return launch_attention_rows_kernel<Kernels::template kernel<64>>(entry, args, a, rows, stream);
    case 128: return launch_attention_rows_kernel<Kernels::template kernel<128>>(entry, args, a, rows, stream);
    default: return launch_attention_rows_kernel<Kernels::template kernel<256>>(entry, args, a, rows, stream);
  }
}

}  // namespace mq
