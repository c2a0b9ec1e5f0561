// Seeded token selection on the device (mq_sample): greedy, temperature, top-k, top-p (nucleus) and min-p for 1 .. 8 logits rows.
//
// THE RULE (normative).  Per row: fp32 logits l[0..V), temperature >= 0, top_k (0 = off), top_p in (0, 1] (1 = off),
// min_p in [0, 1) (0 = off), seed and stream (u64), n = pos[row] = the number of tokens already in the sequence.
//   0. (mq_sample_penalized only.)  With the row's history h[0..V) (bit 31: in the prompt; bits 0..15: c_i, times generated, saturating),
//      seen_i = (h_i != 0), repetition r, presence a, frequency f and an optional dense bias, each line one correctly rounded fp32
//      operation, no fused multiply-add:  l1 = seen_i ? (l_i > 0 ? l_i / r : l_i * r) : l_i;  t = f * (float)c_i;
//      t = t + (c_i > 0 ? a : 0);  l2 = l1 - t;  l3 = bias ? l2 + bias_i : l2.  l3 stands for l_i below.  A neutral row (r = 1, a = f = 0,
//      no bias) skips the step: the bits of l_i are kept.  r not finite and > 0 is served as 1.
//   1. z_i = l_i / temperature (fp32, correctly rounded divide; -0 counts as +0).  A NaN logit is -inf.  If every logit is -inf or
//      NaN the token is 0.
//   2. Order: z descending, ties by index ascending.  "Prefix" = a prefix in this order.
//   3. K = the first top_k tokens (all if top_k is 0 or >= V).
//   4. w_i = (u64) floor(expf(z_i - z_max) * 2^32): sums of w are exact integers in any order (V <= 2^20: below 2^53).  W_K = sum over
//      K.  P = the shortest prefix of K whose sum is >= ceil((double)top_p * (double)W_K); never empty; top_p == 1: P = K.
//   5. C = the tokens of P with z_i - z_max >= logf(min_p) (fp32); the top token always passes; min_p == 0: C = P.
//   6. (r0..r3) = philox4x32_10(counter {lo32(n), i / 4, lo32(stream), hi32(stream)}, key {lo32(seed), hi32(seed)}),
//      u_i = ((r_(i % 4) >> 9) + 0.5) * 2^-23 (23 random bits: k + 0.5 has at most 24 significant bits, so u_i is exact in fp32 and
//      strictly inside (0, 1); with 24 bits the largest k + 0.5 would round up to u = 1 and g = +inf), g_i = -logf(-logf(u_i)),
//      token = argmax over C of z_i + g_i (one fp32 add), ties to the lowest index: a draw from softmax(z) restricted to C.
//   7. temperature == 0: the lowest index of the maximal logit; no random numbers.  A row whose parameters are out of range
//      (temperature < 0 or not finite, top_k < 0, top_p outside (0, 1], min_p outside [0, 1)) is served as greedy.
// Nothing above depends on an evaluation order: the masses are integers, every random number is a function of (seed, stream, n, i)
// and every maximum is taken under a total order.  So a row's token depends on that row alone, not on its slot or on the launch.
//
// THE KERNELS.  Launch 1 (sample_scan_kernel, grid slices x rows, 256 threads): rows without a filter (and greedy rows) -- each
// workgroup takes a slice of the row, keeps the running best (z + g, index) and writes its partial to scratch.  Launch 2
// (sample_select_kernel, one workgroup of 1024 threads per row): merges the partials of an unfiltered row in slice order; a filtered
// row is selected here by radix, without a sort.  Every token gets the 52-bit key (monotone u32 of z) << 20 | (2^20 - 1 - i): keys
// are distinct and their descending order is the rule's order, so K and P are "key >= cut" and no tie needs a case of its own.  A cut
// is found digit by digit (11 / 11 / 10 / 10 / 10 bits): per level one pass over the row builds (count, u64 mass) per digit in LDS
// with integer atomics among the tokens that share the digits found so far, a block scan from the top digit finds the digit where the
// count reaches top_k (K) or the mass reaches the threshold (P), and the descent goes on inside it; once the digit holds one token a
// single pass reads its key.  The last pass is the Gumbel argmax over key >= cut with the min-p test.  A row of at most 32 768 entries
// is read from memory once and held in LDS as z; longer rows are re-read (from the L2) per pass.
// Optional outputs: kept[row] = |C|; logprob[row] = (z_tok - z_max) - log(W_C 2^-32) with W_C the integer mass of C, evaluated in
// double from fp32 z.  Against the exact restricted log-softmax of z: |error| <= 2^-23 (2 + log V) + V / W_C + ulp_fp32(logprob) --
// each w carries expf's error (1 ulp ASSUMED) and the rounding of z_i - z_max, |d_i| 2^-24 relative, whose p-weighted mean is at
// most 2^-24 log V; flooring drops less than one unit of 2^-32 per token; one rounding of z_tok - z_max and one of the result.  Not
// part of the bit contract.  All results leave through ordinary vector stores.
// Both kernels are templates over a load policy, instantiated four times (sample_scan_kernel<Pol>, sample_select_kernel<Pol>).
// mq_sample_penalized runs them with the Penalty policy: step 0 is applied wherever a logit is loaded -- once for a row held in LDS, on
// every re-read of a longer one -- reading 4 more bytes of history (8 with a bias) per entry; the history is never staged in LDS.  The
// thread that writes a row's token then counts it in the row's history (observe).
//
// SEVERAL ROWS OF ONE SEQUENCE (mq_sample_rows).  T <= 8 logits rows of ONE sequence -- the rows of a multi-token step over
// [t, d_1 .. d_(T-1)] -- under one request, one optional penalty row, one optional dense bias row and one optional history h[0..V); the
// proposals d[0..T-2] (int64) and a base index are read from device memory.  Row j (0-based) is drawn at n_j = *n_base + n_offset + j.
// Step 0 uses for row j the entry
//      c_i(j) = min(65535, c_i + #{m < j : d[m] == i})   (bits 0..15)      seen_i(j) = (h_i != 0) or (c_i(j) > 0)      (bit 31 untouched)
// i.e. the history on which d[0..j-1] were counted one after the other; an absent history is all zeros; a proposal outside [0, V) matches
// no entry.  Everything else is the rule above, unchanged; there is no idle row: every row draws.  The history and the logits are not
// written.  So tok[j] is what mq_sample draws for that row alone at n_j (a neutral request, with or without a history, keeps the bits of
// its logits) and what mq_sample_penalized draws there from a history that has counted d[0..j-1].
// The same two kernels with a third load policy, Rows: a workgroup reads the at most
// seven proposals in front of its row once, wave-uniform, and compares them with the 4-entry block index as the entries are loaded --
// nothing more is staged in LDS and no pass over V is added.
// mq_sample_history_count moves the counts of n ids by +1 or -1 (saturating at 65 535 and at 0, bit 31 kept, ids outside [0, V) ignored)
// with one compare-and-swap loop per id: the result of applying them one by one, in any order.
//
// ROWS OF SEVERAL SEQUENCES (mq_sample_ragged).  R <= 8 logits rows of a ragged step: row r belongs to sequence
// row_seq[r] at cached position row_pos[r], the table mq_decode_attention_ragged reads (device int32), and was stepped with token
// row_tok[r] (device int64).  Runs are that launch's (mq_row_runs.h): a maximal stretch of consecutive rows with equal row_seq whose
// row_pos rise by exactly one.  A row whose row_seq is outside [0, batch) or whose row_pos is outside [0, cache_len) is idle and ends a
// run: its tok, kept and logprob keep their bytes.  A live row r at distance j from its run's first row, with s = row_seq[r], is drawn
// at n = row_pos[r] + n_offset under params[s], with penalty[s], bias[s] and the history row of s (each of the three arrays nullable: no
// penalty row is the neutral one, no history is all zeros, no bias array is no bias), and step 0 uses the entry of mq_sample_rows,
//      c_i(j) = min(65535, c_i + #{m < j : d[m] == i})      seen_i(j) = (h_i != 0) or (c_i(j) > 0)      with d[0 .. j-1] = row_tok[r-j+1 .. r],
// the proposals in front of the row.  The run's first token row_tok[r-j] is no proposal: it is the sequence's last accepted token and
// the history holds it already.  A token outside [0, V) matches no entry; a neutral sequence keeps the bits of its logits, history or
// not; nothing but tok, kept, logprob and scratch is written; there is no observe.  So tok[r] and kept[r] are, bit for bit, what
// mq_sample_rows draws for row j of that run alone (the sequence's request and history, n_base + n_offset = the run's first index,
// those proposals) and what mq_sample / mq_sample_penalized draw for the row alone from the counted history.
// The same two kernels with a fourth load policy, Ragged: the row is the
// workgroup's blockIdx, so the walk back over the table (at most 7 steps), the request lookup and the at most 7 proposals are
// wave-uniform scalar loads; row_seq and row_pos are range-checked before any address is formed from them -- the table is device data,
// and whatever it holds the launch stays inside its buffers.  Behind its constructor the policy IS Rows: no pass over V and no LDS is added.
// mq_sample_history_count_ragged is mq_sample_history_count over (sequence, id) pairs and a [batch][history_stride] block of histories.
#include "mq_common.h"
#include "mq_row_runs.h"

#include <limits.h>

namespace mq {
namespace {

constexpr int SM_SCAN_THREADS = 256;
constexpr int SM_SLICE = 4096;                 // entries per slice of launch 1 (at most SM_MAX_SLICES slices: longer slices above 2^18 entries)
constexpr int SM_MAX_SLICES = 64;
constexpr int SM_THREADS = 1024;               // launch 2: one workgroup per row
constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_BINS = 2048;
constexpr int SM_LDS_ROW = 32768;              // entries of a row held in LDS (128 KiB of the 160)
constexpr int SM_LEVELS = 5;

struct Best {
  float v;
  int i;
};

// (a, ia) ranks above (b, ib): the larger value, then the lower index.  No NaN reaches here.  A total order.
__device__ __forceinline__ bool better(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned r[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__device__ __forceinline__ float uniform_of(unsigned r) { return ((float)(r >> 9) + 0.5f) * 0x1p-23f; }
__device__ __forceinline__ float gumbel_of(unsigned r) { return -logf(-logf(uniform_of(r))); }

struct RowCfg {
  float t, top_p, min_p;
  int top_k;
  unsigned s0, s1, k0, k1, n;
  bool greedy, filtered;
};

__device__ __forceinline__ RowCfg row_cfg(const mq_sample_row& p, int n, int V) {
  RowCfg c;
  c.t = p.temperature; c.top_p = p.top_p; c.min_p = p.min_p; c.top_k = p.top_k;
  c.s0 = (unsigned)p.stream; c.s1 = (unsigned)(p.stream >> 32); c.k0 = (unsigned)p.seed; c.k1 = (unsigned)(p.seed >> 32);
  c.n = (unsigned)n;
  const bool valid = c.t >= 0.f && c.t < __builtin_inff() && c.top_k >= 0 && c.top_p > 0.f && c.top_p <= 1.f && c.min_p >= 0.f && c.min_p < 1.f;
  c.greedy = !valid || c.t == 0.f;
  c.filtered = !c.greedy && ((c.top_k > 0 && c.top_k < V) || c.top_p < 1.f || c.min_p > 0.f);
  return c;
}

// z of rule 1 (greedy rows: the logit itself)
__device__ __forceinline__ float z_of(float l, const RowCfg& c) {
  if (l != l) return -__builtin_inff();
  return (c.greedy ? l : l / c.t) + 0.f;
}

// ---- step 0 of the rule: how a kernel reads a logit -------------------------------------------------------------------------------
// A policy loads entries of a logits row.  NoPenalty is the plain read of mq_sample; Penalty applies step 0 on the way in (mq_sample_penalized),
// so no kernel writes the logits and none makes a pass of its own for it.
struct NoArgs {};

struct NoPenalty {
  typedef NoArgs Args;
  __device__ __forceinline__ NoPenalty(const NoArgs&, int) {}
  __device__ __forceinline__ float4 load4(const float* __restrict__ row, int i) const { return *reinterpret_cast<const float4*>(row + i); }
  __device__ __forceinline__ float load1(const float* __restrict__ row, int i) const { return row[i]; }
  __device__ __forceinline__ void observe(int) const {}
};

struct PenArgs {
  const mq_sample_penalty_row* pen;
  unsigned* hist;
  long long hstride;
  const float* const* bias;
  int observe;
};

// Step 0 on one entry, for the three penalised policies: the request's (r, a, f), its dense bias row and whether the step runs at all.
struct Step0 {
  const float* b;                 // the dense bias row, or nullptr
  float r, a, f;
  bool active;
  // (r, a, f) of pen[i], the request's penalty row; pen == nullptr: of the neutral one
  __device__ __forceinline__ void decode(const mq_sample_penalty_row* pen, int i) {
    r = 1.f; a = 0.f; f = 0.f;
    if (pen) {
      const mq_sample_penalty_row q = pen[i];
      r = (q.repetition > 0.f && q.repetition < __builtin_inff()) ? q.repetition : 1.f;
      a = q.presence; f = q.frequency;
    }
  }
  // the entry is hv with `extra` in-flight occurrences added to its count
  // one correctly rounded fp32 operation per line (the build has no contraction: -ffp-contract=off)
  __device__ __forceinline__ float one(float l, unsigned hv, unsigned extra, float bv) const {
    const unsigned c = min(0xFFFFu, (hv & 0xFFFFu) + extra);
    const float l1 = (hv != 0u || extra != 0u) ? (l > 0.f ? l / r : l * r) : l;
    float t = f * (float)c;
    t = t + (c > 0u ? a : 0.f);
    const float l2 = l1 - t;
    return b ? l2 + bv : l2;
  }
};

struct Penalty : Step0 {
  typedef PenArgs Args;
  unsigned* h;                    // the row's history: bit 31 = in the prompt, bits 0..15 = times generated
  bool count;
  __device__ __forceinline__ Penalty(const PenArgs& pa, int row) {
    __builtin_assume(pa.pen != nullptr);                            // (mq_sample_penalized refuses a null penalty)
    decode(pa.pen, row);
    h = pa.hist + (long long)row * pa.hstride;
    b = pa.bias ? pa.bias[row] : nullptr;
    active = r != 1.f || a != 0.f || f != 0.f || b != nullptr;     // a neutral request keeps the bits of its logits (-0 stays -0), history or not
    count = pa.observe != 0;
  }
  __device__ __forceinline__ float4 load4(const float* __restrict__ row, int i) const {
    const float4 l = *reinterpret_cast<const float4*>(row + i);
    if (!active) return l;                                          // workgroup-uniform
    const uint4 hv = *reinterpret_cast<const uint4*>(h + i);
    const float4 bv = b ? *reinterpret_cast<const float4*>(b + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    return make_float4(one(l.x, hv.x, 0u, bv.x), one(l.y, hv.y, 0u, bv.y), one(l.z, hv.z, 0u, bv.z), one(l.w, hv.w, 0u, bv.w));
  }
  __device__ __forceinline__ float load1(const float* __restrict__ row, int i) const {
    return active ? one(row[i], h[i], 0u, b ? b[i] : 0.f) : row[i];
  }
  // the drawn token's count, saturating at 65 535: one thread, after every read of the row's history in this launch
  __device__ __forceinline__ void observe(int t) const {
    if (!count) return;
    const unsigned v = h[t];
    if ((v & 0xFFFFu) != 0xFFFFu) h[t] = v + 1u;
  }
};

// mq_sample_rows: T rows of ONE sequence.  One request, penalty row, bias row and history for all rows; row j adds the proposals in front
// of it to the history's counts as it reads them.
struct RowsArgs {
  const mq_sample_penalty_row* pen;   // one row, or nullptr (neutral)
  const unsigned* hist;               // the sequence's history, or nullptr (all zeros)
  const float* bias;                  // one dense row, or nullptr
  const long long* prop;              // rows - 1 proposals
  int V;
  int n_offset;
};

constexpr int SM_MAX_PROPOSALS = MQ_DECODE_MAX_BATCH - 1;

struct Rows : Step0 {
  typedef RowsArgs Args;
  const unsigned* h;              // the sequence's history, or nullptr (all zeros)
  int d[SM_MAX_PROPOSALS];        // the proposals in front of this row (wave-uniform), -1: none
  __device__ __forceinline__ Rows() {}                                 // (Ragged fills the fields itself)
  __device__ __forceinline__ Rows(const RowsArgs& ra, int row) {
    decode(ra.pen, 0);
    h = ra.hist;
    b = ra.bias;
    active = r != 1.f || a != 0.f || f != 0.f || b != nullptr;     // a neutral request keeps the bits of its logits (-0 stays -0), history or not
#pragma unroll
    for (int m = 0; m < SM_MAX_PROPOSALS; ++m) {
      d[m] = -1;
      if (active && m < row) {
        const long long t = ra.prop[m];
        if (t >= 0 && t < (long long)ra.V) d[m] = (int)t;
      }
    }
  }
  __device__ __forceinline__ float4 load4(const float* __restrict__ row, int i) const {
    const float4 l = *reinterpret_cast<const float4*>(row + i);
    if (!active) return l;                                          // workgroup-uniform
    const uint4 hv = h ? *reinterpret_cast<const uint4*>(h + i) : make_uint4(0u, 0u, 0u, 0u);
    const float4 bv = b ? *reinterpret_cast<const float4*>(b + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned e0 = 0u, e1 = 0u, e2 = 0u, e3 = 0u;
    const int blk = i >> 2;
    bool hit = false;
#pragma unroll
    for (int m = 0; m < SM_MAX_PROPOSALS; ++m) hit = hit || (d[m] >> 2) == blk;      // (-1 >> 2 = -1: no block)
    if (hit) {
#pragma unroll
      for (int m = 0; m < SM_MAX_PROPOSALS; ++m) {
        e0 += d[m] == i ? 1u : 0u; e1 += d[m] == i + 1 ? 1u : 0u; e2 += d[m] == i + 2 ? 1u : 0u; e3 += d[m] == i + 3 ? 1u : 0u;
      }
    }
    return make_float4(one(l.x, hv.x, e0, bv.x), one(l.y, hv.y, e1, bv.y), one(l.z, hv.z, e2, bv.z), one(l.w, hv.w, e3, bv.w));
  }
  __device__ __forceinline__ float load1(const float* __restrict__ row, int i) const {
    if (!active) return row[i];
    unsigned e = 0u;
#pragma unroll
    for (int m = 0; m < SM_MAX_PROPOSALS; ++m) e += d[m] == i ? 1u : 0u;
    return one(row[i], h ? h[i] : 0u, e, b ? b[i] : 0.f);
  }
  __device__ __forceinline__ void observe(int) const {}               // the caller counts what it keeps (mq_sample_history_count)
};

// mq_sample_ragged: R rows of up to `batch` sequences, named by the row table of mq_decode_attention_ragged.  A live row reads its
// sequence's request, penalty row, bias row and history, and the tokens its run was stepped with behind the run's first row are the
// proposals in front of it; from there on it is a Rows policy.
struct RaggedArgs {
  const int* row_seq;                 // [rows] the row's sequence; outside [0, batch): idle
  const int* row_pos;                 // [rows] the row's cached position; outside [0, cache_len): idle
  const long long* row_tok;           // [rows] the tokens the rows were stepped with
  const mq_sample_penalty_row* pen;   // [batch], or nullptr (every sequence neutral)
  const unsigned* hist;               // [batch][hstride], or nullptr (all zeros)
  long long hstride;
  const float* const* bias;           // [batch] device pointers (each nullptr or a dense row), or nullptr
  int batch, V, n_offset;
};

struct Ragged : Rows {
  // only built for a live row (row_index below has range-checked row_seq[row] and row_pos[row])
  typedef RaggedArgs Args;
  __device__ __forceinline__ Ragged(const RaggedArgs& ga, int row) {
    const int s = ga.row_seq[row];
    decode(ga.pen, s);
    h = ga.hist ? ga.hist + (long long)s * ga.hstride : nullptr;
    b = ga.bias ? ga.bias[s] : nullptr;
    active = r != 1.f || a != 0.f || f != 0.f || b != nullptr;     // a neutral request keeps the bits of its logits (-0 stays -0), history or not
    const int j = active ? run_rows_in_front(ga.row_seq, ga.row_pos, row, s, ga.row_pos[row], SM_MAX_PROPOSALS) : 0;
#pragma unroll
    for (int m = 0; m < SM_MAX_PROPOSALS; ++m) {
      d[m] = -1;
      if (m < j) {                                                  // row_tok[row - j] is the run's first token: no proposal
        const long long t = ga.row_tok[row - j + 1 + m];
        if (t >= 0 && t < (long long)ga.V) d[m] = (int)t;
      }
    }
  }
};

// running best of z + g (greedy: z) over entries [lo, hi) of the row, 4 per thread and step; lo, hi multiples of 4
template <class Pol>
__device__ __forceinline__ Best scan_range(const float* __restrict__ row, int lo, int hi, const RowCfg& c, const Pol& p, int tid, int nthreads) {
  Best b{-__builtin_inff(), INT_MAX};
  for (int i = lo + 4 * tid; i < hi; i += 4 * nthreads) {
    const float4 l = p.load4(row, i);
    const float lv[4] = {l.x, l.y, l.z, l.w};
    unsigned r[4] = {0, 0, 0, 0};
    if (!c.greedy) philox4x32_10(c.n, (unsigned)(i >> 2), c.s0, c.s1, c.k0, c.k1, r);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float s = z_of(lv[e], c);
      if (!c.greedy) s = s + gumbel_of(r[e]);
      if (better(s, i + e, b.v, b.i)) { b.v = s; b.i = i + e; }
    }
  }
  return b;
}

__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(b.v, o);
    const int oi = __shfl_xor(b.i, o);
    if (better(ov, oi, b.v, b.i)) { b.v = ov; b.i = oi; }
  }
  return b;
}

// every thread gets the workgroup's best; red: 2 * waves words of LDS
__device__ __forceinline__ Best block_best(Best b, float* red_v, int* red_i, int tid, int waves) {
  b = wave_best(b);
  __syncthreads();
  if ((tid & 63) == 0) { red_v[tid >> 6] = b.v; red_i[tid >> 6] = b.i; }
  __syncthreads();
  Best o{red_v[0], red_i[0]};
  for (int w = 1; w < waves; ++w)
    if (better(red_v[w], red_i[w], o.v, o.i)) { o.v = red_v[w]; o.i = red_i[w]; }
  return o;
}

__device__ __forceinline__ bool row_idle(const int* pos, int row, int cache_len, int* n) {
  *n = pos[row];
  return *n < 0 || *n >= cache_len;
}

// Which index a row draws at and which request it reads.  mq_sample / mq_sample_penalized: pos[row] with the idle sentinel, params[row].
// mq_sample_rows: *pos + n_offset + row, never idle, the one request.  mq_sample_ragged: row_pos[row] + n_offset with the table's idle rows
// (sequence or position out of range, checked before anything is addressed by them), the request of the row's sequence.
template <class PolArgs>
__device__ __forceinline__ bool row_index(const PolArgs&, const int* pos, int row, int cache_len, int* n) { return row_idle(pos, row, cache_len, n); }
__device__ __forceinline__ bool row_index(const RowsArgs& ra, const int* pos, int row, int, int* n) {
  *n = pos[0] + ra.n_offset + row;
  return false;
}
__device__ __forceinline__ bool row_index(const RaggedArgs& ga, const int*, int row, int cache_len, int* n) {
  const int s = ga.row_seq[row], p = ga.row_pos[row];
  *n = p + ga.n_offset;
  return s < 0 || s >= ga.batch || p < 0 || p >= cache_len;
}
template <class PolArgs>
__device__ __forceinline__ int request_of(const PolArgs&, int row) { return row; }
__device__ __forceinline__ int request_of(const RaggedArgs& ga, int row) { return ga.row_seq[row]; }
__device__ __forceinline__ int request_of(const RowsArgs&, int) { return 0; }

__device__ __forceinline__ void slice_bounds(int V, int S, int s, int* lo, int* hi) {
  const int len = ((V / 4 + S - 1) / S) * 4;
  *lo = min(V, s * len);
  *hi = min(V, *lo + len);
}

template <class Pol, class PolArgs>
__device__ __forceinline__ void sample_scan(const float* __restrict__ logits, long long stride, int V, const int* __restrict__ pos, int cache_len,
                                            const mq_sample_row* __restrict__ params, Best* __restrict__ part, const PolArgs& pa) {
  __shared__ float red_v[SM_SCAN_THREADS / 64];
  __shared__ int red_i[SM_SCAN_THREADS / 64];
  const int row = blockIdx.y, s = blockIdx.x, S = gridDim.x, tid = threadIdx.x;
  int n;
  if (row_index(pa, pos, row, cache_len, &n)) return;                 // workgroup-uniform
  const RowCfg c = row_cfg(params[request_of(pa, row)], n, V);
  if (c.filtered) return;
  const Pol p(pa, row);
  int lo, hi;
  slice_bounds(V, S, s, &lo, &hi);
  const Best b = block_best(scan_range(logits + (long long)row * stride, lo, hi, c, p, tid, SM_SCAN_THREADS), red_v, red_i, tid, SM_SCAN_THREADS / 64);
  if (tid == 0) part[row * SM_MAX_SLICES + s] = b;
}

// pos / cache_len: mq_sample's; mq_sample_rows: n_base / unused; mq_sample_ragged: the table's row_pos / cache_len (row_index)
template <class Pol>
__global__ __launch_bounds__(SM_SCAN_THREADS) void sample_scan_kernel(const float* __restrict__ logits, long long stride, int V, const int* __restrict__ pos,
                                                                      int cache_len, const mq_sample_row* __restrict__ params, Best* __restrict__ part,
                                                                      typename Pol::Args pa) {
  sample_scan<Pol>(logits, stride, V, pos, cache_len, params, part, pa);
}

// ---- launch 2 ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long mass_of(float z, float zmax) {
  const float e = expf(z - zmax) * 0x1p32f;
  return e >= 0.f ? (unsigned long long)floorf(e) : 0ull;            // (a NaN, from z = z_max = +inf, carries no mass)
}

struct Lds {
  float* z;                       // the row as z (rows of at most SM_LDS_ROW entries), else unused
  unsigned long long* hm;         // [SM_BINS] mass per digit
  unsigned* hc;                   // [SM_BINS] count per digit
  unsigned long long* wt;         // [2][SM_WAVES] wave totals of the two scans
  unsigned long long* found;      // [6] digit, count before, mass before, count in, mass in, key
  float* red_v;                   // [SM_WAVES]
  int* red_i;                     // [SM_WAVES]
};

struct RowSrc {
  const float* g;                 // logits row in memory
  const float* z;                 // LDS copy (z), or nullptr
};

template <class Pol>
__device__ __forceinline__ float4 load_z4(const RowSrc& r, int i, const RowCfg& c, const Pol& p) {
  if (r.z) return *reinterpret_cast<const float4*>(r.z + i);
  const float4 l = p.load4(r.g, i);
  return make_float4(z_of(l.x, c), z_of(l.y, c), z_of(l.z, c), z_of(l.w, c));
}

__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, const Lds& L, int tid) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                // the last shuffle has landed: nothing of this wave is in flight at the barrier
  __syncthreads();                                                 // (L.wt may still be read by the previous reduction)
  if ((tid & 63) == 0) L.wt[tid >> 6] = v;
  __syncthreads();
  unsigned long long s = 0;
  for (int w = 0; w < SM_WAVES; ++w) s += L.wt[w];
  return s;
}

// The cut of the shortest prefix (among tokens with key >= lb) whose count (by_mass = false) or mass (true) reaches `need` (>= 1, at most
// the total).  Returns the cut key; *cnt / *mass = the prefix's count and mass (the cut token included).
template <class Pol>
__device__ unsigned long long select_cut(const RowSrc& r, int V, const RowCfg& c, const Pol& p, float zmax, unsigned long long lb, bool by_mass,
                                         unsigned long long need, const Lds& L, int tid, unsigned long long* cnt, unsigned long long* mass) {
  const int SH[SM_LEVELS] = {41, 30, 20, 10, 0}, WD[SM_LEVELS] = {11, 11, 10, 10, 10};
  unsigned long long prefix = 0, acc_c = 0, acc_m = 0;
  const int lane = tid & 63, wave = tid >> 6;
  for (int level = 0; level < SM_LEVELS; ++level) {
    const int sh = SH[level], up = SH[level] + WD[level];
    const unsigned dmask = (1u << WD[level]) - 1u;
    __syncthreads();
    for (int b = tid; b < SM_BINS; b += SM_THREADS) { L.hc[b] = 0u; L.hm[b] = 0ull; }
    if (tid == 0) { L.found[0] = 0; L.found[1] = 0; L.found[2] = 0; L.found[3] = 0; L.found[4] = 0; }
    __syncthreads();
    for (int i = 4 * tid; i < V; i += 4 * SM_THREADS) {
      const float4 z4 = load_z4(r, i, c, p);
      const float zv[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned long long k = sort_key(zv[e], i + e);
        if (k >= lb && (level == 0 || (k >> up) == (prefix >> up))) {
          const unsigned d = (unsigned)(k >> sh) & dmask;
          atomicAdd(&L.hc[d], 1u);
          atomicAdd(&L.hm[d], mass_of(zv[e], zmax));
        }
      }
    }
    __syncthreads();
    // thread t owns digits 2047 - 2t (first in the order) and 2046 - 2t; exclusive scans of count and mass in that order
    const int bh = SM_BINS - 1 - 2 * tid, bl = bh - 1;
    const unsigned long long ch = L.hc[bh], cl = L.hc[bl], mh = L.hm[bh], ml = L.hm[bl];
    unsigned long long sc = ch + cl, sm = mh + ml;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long uc = __shfl_up(sc, o), um = __shfl_up(sm, o);
      if (lane >= o) { sc += uc; sm += um; }
    }
    if (lane == 63) { L.wt[wave] = sc; L.wt[SM_WAVES + wave] = sm; }
    __syncthreads();
    unsigned long long oc = 0, om = 0;
    for (int w = 0; w < wave; ++w) { oc += L.wt[w]; om += L.wt[SM_WAVES + w]; }
    const unsigned long long ec = sc - (ch + cl) + oc, em = sm - (mh + ml) + om;        // before digit bh
    const unsigned long long before = by_mass ? em : ec, vh = by_mass ? mh : ch, vl = by_mass ? ml : cl;
    if (before < need && need <= before + vh) {
      L.found[0] = (unsigned long long)bh; L.found[1] = ec; L.found[2] = em; L.found[3] = ch; L.found[4] = mh;
    } else if (before + vh < need && need <= before + vh + vl) {
      L.found[0] = (unsigned long long)bl; L.found[1] = ec + ch; L.found[2] = em + mh; L.found[3] = cl; L.found[4] = ml;
    }
    __syncthreads();
    const unsigned long long d = L.found[0], in_c = L.found[3], in_m = L.found[4];
    acc_c += L.found[1];
    acc_m += L.found[2];
    need -= by_mass ? L.found[2] : L.found[1];
    prefix |= d << sh;
    if (level == SM_LEVELS - 1 || in_c <= 1) {
      acc_c += in_c;
      acc_m += in_m;
      if (level < SM_LEVELS - 1 && in_c == 1) {                  // the digit holds one token: read its key instead of descending
        __syncthreads();
        for (int i = 4 * tid; i < V; i += 4 * SM_THREADS) {
          const float4 z4 = load_z4(r, i, c, p);
          const float zv[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const unsigned long long k = sort_key(zv[e], i + e);
            if (k >= lb && (k >> sh) == (prefix >> sh)) L.found[5] = k;
          }
        }
        __syncthreads();
        prefix = L.found[5];
      }
      break;
    }
  }
  *cnt = acc_c;
  *mass = acc_m;
  return prefix;
}

template <class Pol, class PolArgs>
__device__ __forceinline__ void sample_select(unsigned char* smem, const float* __restrict__ logits, long long stride, int V, int S, int lds_row,
                                              const int* __restrict__ pos, int cache_len, const mq_sample_row* __restrict__ params,
                                              const Best* __restrict__ part, long long* __restrict__ tok, int* __restrict__ kept,
                                              float* __restrict__ logprob, const PolArgs& pa) {
  const int row = blockIdx.x, tid = threadIdx.x;
  int n;
  if (row_index(pa, pos, row, cache_len, &n)) return;                 // workgroup-uniform: an idle row keeps its token and its history
  const RowCfg c = row_cfg(params[request_of(pa, row)], n, V);
  const Pol p(pa, row);
  Lds L;
  L.z = reinterpret_cast<float*>(smem);
  L.hm = reinterpret_cast<unsigned long long*>(smem + (size_t)lds_row * 4);
  L.found = L.hm + SM_BINS;
  L.wt = L.found + 8;
  L.hc = reinterpret_cast<unsigned*>(L.wt + 2 * SM_WAVES);
  L.red_v = reinterpret_cast<float*>(L.hc + SM_BINS);
  L.red_i = reinterpret_cast<int*>(L.red_v + SM_WAVES);
  RowSrc r{logits + (long long)row * stride, nullptr};
  const float NEG_INF = -__builtin_inff();
  const bool want_mass = logprob != nullptr;

  if (!c.filtered && !want_mass) {                                  // merge launch 1's partials in slice order (one slice: scan here)
    Best b{NEG_INF, INT_MAX};
    if (S > 1) {
      if (tid < S) b = part[row * SM_MAX_SLICES + tid];
      b = block_best(b, L.red_v, L.red_i, tid, SM_WAVES);
    } else {
      b = block_best(scan_range(r.g, 0, V, c, p, tid, SM_THREADS), L.red_v, L.red_i, tid, SM_WAVES);
    }
    if (tid == 0) {
      const int t = b.i == INT_MAX ? 0 : b.i;
      tok[row] = t;
      if (kept) kept[row] = c.greedy ? 1 : V;
      p.observe(t);
    }
    return;
  }

  // stage the row as z; its maximum
  Best zb{NEG_INF, INT_MAX};
  for (int i = 4 * tid; i < V; i += 4 * SM_THREADS) {
    const float4 z4 = load_z4(r, i, c, p);
    if (lds_row) *reinterpret_cast<float4*>(L.z + i) = z4;
    const float zv[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (better(zv[e], i + e, zb.v, zb.i)) { zb.v = zv[e]; zb.i = i + e; }
  }
  if (lds_row) r.z = L.z;
  zb = block_best(zb, L.red_v, L.red_i, tid, SM_WAVES);
  const float zmax = zb.v;
  if (zmax == NEG_INF || c.greedy) {                                  // nothing to draw from (token 0), or greedy with a log-probability asked for
    if (tid == 0) {
      const int t = zmax == NEG_INF ? 0 : zb.i;
      tok[row] = t;
      if (kept) kept[row] = zmax == NEG_INF ? 0 : 1;
      if (logprob) logprob[row] = 0.f;
      p.observe(t);
    }
    return;
  }

  unsigned long long cut = 0, cnt = (unsigned long long)V, wk = 0;
  const bool use_k = c.top_k > 0 && c.top_k < V;
  if (use_k) {
    cut = select_cut(r, V, c, p, zmax, 0ull, false, (unsigned long long)c.top_k, L, tid, &cnt, &wk);
  } else if (c.top_p < 1.f) {
    unsigned long long m = 0;
    for (int i = 4 * tid; i < V; i += 4 * SM_THREADS) {
      const float4 z4 = load_z4(r, i, c, p);
      m += mass_of(z4.x, zmax) + mass_of(z4.y, zmax) + mass_of(z4.z, zmax) + mass_of(z4.w, zmax);
    }
    wk = block_sum_u64(m, L, tid);
  }
  if (c.top_p < 1.f) {
    unsigned long long need = (unsigned long long)ceil((double)c.top_p * (double)wk);
    need = need < 1ull ? 1ull : (need > wk ? wk : need);
    unsigned long long pm;
    cut = select_cut(r, V, c, p, zmax, cut, true, need, L, tid, &cnt, &pm);
  }

  // the draw: argmax of z + g over key >= cut with the min-p test; |C| and its mass on the way
  const float lmin = c.min_p > 0.f ? logf(c.min_p) : NEG_INF;
  Best b{NEG_INF, INT_MAX};
  unsigned long long nkept = 0, wc = 0;
  for (int i = 4 * tid; i < V; i += 4 * SM_THREADS) {
    const float4 z4 = load_z4(r, i, c, p);
    const float zv[4] = {z4.x, z4.y, z4.z, z4.w};
    bool in[4], any = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      in[e] = sort_key(zv[e], i + e) >= cut && (zv[e] - zmax >= lmin || i + e == zb.i);
      any = any || in[e];
    }
    if (!any) continue;
    unsigned rr[4];
    philox4x32_10(c.n, (unsigned)(i >> 2), c.s0, c.s1, c.k0, c.k1, rr);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (in[e]) {
        const float s = zv[e] + gumbel_of(rr[e]);
        if (better(s, i + e, b.v, b.i)) { b.v = s; b.i = i + e; }
        nkept += 1;
        if (want_mass) wc += mass_of(zv[e], zmax);
      }
  }
  b = block_best(b, L.red_v, L.red_i, tid, SM_WAVES);
  if (kept) nkept = block_sum_u64(nkept, L, tid);
  if (want_mass) wc = block_sum_u64(wc, L, tid);
  if (tid == 0) {
    const int t = b.i == INT_MAX ? zb.i : b.i;
    tok[row] = t;
    if (kept) kept[row] = (int)nkept;
    if (logprob) {
      const float zt = r.z ? r.z[t] : z_of(p.load1(r.g, t), c);
      logprob[row] = (float)((double)(zt - zmax) - (log((double)wc) - 32.0 * 0.693147180559945309417));
    }
    p.observe(t);
  }
}

// NoPenalty: mq_sample.  Penalty: step 0 applied as a row is read, the drawn token counted in the row's history at the tail.  Rows: the rows
// of one sequence, each with the proposals in front of it counted as its entries are read.  Ragged: the rows of a ragged step, each under
// its own sequence's request with the proposals of its run counted as it reads.  pos / cache_len: as in sample_scan_kernel.
template <class Pol>
__global__ __launch_bounds__(SM_THREADS) void sample_select_kernel(const float* __restrict__ logits, long long stride, int V, int S, int lds_row,
                                                                   const int* __restrict__ pos, int cache_len,
                                                                   const mq_sample_row* __restrict__ params, const Best* __restrict__ part,
                                                                   long long* __restrict__ tok, int* __restrict__ kept, float* __restrict__ logprob,
                                                                   typename Pol::Args pa) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  sample_select<Pol>(smem, logits, stride, V, S, lds_row, pos, cache_len, params, part, tok, kept, logprob, pa);
}

__global__ void history_clear_kernel(uint4* __restrict__ h, int n4) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n4) h[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ids repeat: the OR is idempotent.  An id outside [0, V) is ignored.
__global__ void history_mark_kernel(unsigned* __restrict__ h, int V, const long long* __restrict__ ids, long long n) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const long long t = ids[j];
  if (t >= 0 && t < V) atomicOr(&h[t], 0x80000000u);
}

// The count (bits 0..15) of a history entry moves by delta = +1 / -1, saturating at 65 535 / at 0; bit 31 stays.  One compare-and-swap loop.
__device__ __forceinline__ void count_entry(unsigned* e, int delta) {
  unsigned old = *e;
  for (;;) {
    const unsigned c = old & 0xFFFFu;
    if (delta > 0 ? c == 0xFFFFu : c == 0u) return;
    const unsigned seen = atomicCAS(e, old, delta > 0 ? old + 1u : old - 1u);
    if (seen == old) return;
    old = seen;
  }
}

// count_entry for every id: repeated ids count repeatedly, and since every id moves its entry the same way the result is that of applying
// them one by one.  An id outside [0, V) is ignored.
__global__ void history_count_kernel(unsigned* __restrict__ h, int V, const long long* __restrict__ ids, long long n, int delta) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const long long t = ids[j];
  if (t < 0 || t >= V) return;
  count_entry(h + t, delta);
}

// history_count_kernel over pairs[j] = (sequence, id) and the histories [batch][hstride]: a pair whose sequence is outside [0, batch) or
// whose id is outside [0, V) is ignored, before anything is addressed by it.
__global__ void history_count_ragged_kernel(unsigned* __restrict__ h, long long hstride, int V, int batch, const long long* __restrict__ pairs,
                                            long long n, int delta) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const long long s = pairs[2 * j], t = pairs[2 * j + 1];
  if (s < 0 || s >= batch || t < 0 || t >= V) return;
  count_entry(h + s * hstride + t, delta);
}

__global__ void sample_uniforms_kernel(unsigned long long seed, unsigned long long stream, unsigned n, long long first, long long count,
                                       float* __restrict__ out) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const long long i = first + j;
  unsigned r[4];
  philox4x32_10(n, (unsigned)(i >> 2), (unsigned)stream, (unsigned)(stream >> 32), (unsigned)seed, (unsigned)(seed >> 32), r);
  out[j] = uniform_of(r[i & 3]);
}

size_t select_lds_bytes(int lds_row) {
  return (size_t)lds_row * 4 + (size_t)SM_BINS * 8 + 8 * 8 + 2 * SM_WAVES * 8 + (size_t)SM_BINS * 4 + 2 * SM_WAVES * 4;
}

// ---- the checks the entries share -------------------------------------------------------------------------------------------------
int check_V(int64_t V, const char* who) {
  MQ_REQUIRE(V >= 4 && V % 4 == 0 && V <= (1 << 20), "%s: V=%lld must be a multiple of 4 in [4, 2^20]", who, (long long)V);
  return MQ_OK;
}

int check_history_stride(int64_t history_stride, int64_t V, const char* who) {
  MQ_REQUIRE(history_stride >= V && history_stride % 4 == 0, "%s: history_stride=%lld must be >= V and a multiple of 4", who, (long long)history_stride);
  return MQ_OK;
}

// the history entries: a history of V entries per row
int check_history(const uint32_t* history, int64_t V, const char* who) {
  MQ_REQUIRE(history != nullptr && aligned(history, 16), "%s: history must be a 16-byte aligned pointer", who);
  return check_V(V, who);
}

// the history entries: n ids (`what`: their name in the message) in device memory
int check_ids(const int64_t* ids, int64_t n, const char* what, const char* who) {
  MQ_REQUIRE(n >= 0 && n <= ((int64_t)1 << 31), "%s: n=%lld outside [0, 2^31]", who, (long long)n);
  MQ_REQUIRE(n == 0 || (ids != nullptr && aligned(ids, 8)), "%s: %s must be an 8-byte aligned pointer when n > 0", who, what);
  return MQ_OK;
}

int check_sample_args(const mq_sample_args* a, const char* who) {
  MQ_REQUIRE(a->logits && a->pos && a->params && a->tok && a->scratch,
             "%s: null pointer (logits, pos, params, tok and scratch are required; kept and logprob are optional)", who);
  MQ_REQUIRE(a->rows >= 1 && a->rows <= MQ_DECODE_MAX_BATCH, "%s: rows=%d outside 1..%d", who, a->rows, MQ_DECODE_MAX_BATCH);
  if (const int rc = check_V(a->V, who)) return rc;
  MQ_REQUIRE(a->logits_stride >= a->V && a->logits_stride % 4 == 0, "%s: logits_stride=%lld must be >= V and a multiple of 4", who,
             (long long)a->logits_stride);
  MQ_REQUIRE(a->cache_len >= 1, "%s: cache_len=%d must be >= 1 (a row with pos outside [0, cache_len) is idle)", who, a->cache_len);
  MQ_REQUIRE(aligned(a->logits, 16) && aligned(a->params, 16) && aligned(a->scratch, 16), "%s: logits, params and scratch must be 16-byte aligned", who);
  MQ_REQUIRE(aligned(a->tok, 8) && aligned(a->pos, 4) && aligned(a->kept, 4) && aligned(a->logprob, 4), "%s: tok must be 8-byte, pos / kept / logprob 4-byte aligned", who);
  MQ_REQUIRE(a->scratch_bytes >= MQ_SAMPLE_SCRATCH_BYTES, "%s: scratch_bytes=%lld below MQ_SAMPLE_SCRATCH_BYTES", who, (long long)a->scratch_bytes);
  static_assert(MQ_SAMPLE_SCRATCH_BYTES >= MQ_DECODE_MAX_BATCH * SM_MAX_SLICES * sizeof(Best), "scratch holds every row's partials");
  static_assert(sizeof(mq_sample_row) == 32, "mq_sample_row is 32 bytes");
  static_assert(sizeof(mq_sample_penalty_row) == 16, "mq_sample_penalty_row is 16 bytes");
  return MQ_OK;
}

// An mq_sample_rows_args / mq_sample_ragged_args as mq_sample's block over the same rows (the shared fields carry the same names): its
// limits and alignments are the entry's.
template <class A>
mq_sample_args as_sample_args(const A* a, const int* pos, int cache_len) {
  mq_sample_args s;
  s.logits = a->logits; s.logits_stride = a->logits_stride; s.V = a->V; s.rows = a->rows;
  s.pos = pos; s.cache_len = cache_len; s.params = a->params; s.tok = a->tok; s.kept = a->kept; s.logprob = a->logprob;
  s.scratch = a->scratch; s.scratch_bytes = a->scratch_bytes;
  return s;
}

// the two launches of an entry under its load policy (mq_sample_rows: a->pos is n_base; mq_sample_ragged: a->pos is row_pos)
template <class Pol>
int launch_sample(const mq_sample_args* a, const typename Pol::Args& pa, const char* who, mq_stream_t stream) {
  const int V = (int)a->V;
  const int S = min(SM_MAX_SLICES, (V + SM_SLICE - 1) / SM_SLICE);
  const int lds_row = V <= SM_LDS_ROW ? V : 0;
  const size_t lds = select_lds_bytes(lds_row);
  const int dev = current_device();
  static PerDeviceOnce once;                                         // (one per instantiation)
  if (!once.done(dev)) {
    MQ_REQUIRE(hipFuncSetAttribute((const void*)sample_select_kernel<Pol>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)select_lds_bytes(SM_LDS_ROW)) == hipSuccess,
               "%s: hipFuncSetAttribute(%zu B LDS) failed", who, select_lds_bytes(SM_LDS_ROW));
    once.mark(dev);
  }
  hipStream_t st = as_stream(stream);
  Best* part = static_cast<Best*>(a->scratch);
  long long* tok = reinterpret_cast<long long*>(a->tok);
  if (S > 1) {
    sample_scan_kernel<Pol><<<dim3((unsigned)S, (unsigned)a->rows), SM_SCAN_THREADS, 0, st>>>(a->logits, (long long)a->logits_stride, V, a->pos, a->cache_len,
                                                                                            a->params, part, pa);
    MQ_LAUNCH_CHECK(who);
  }
  sample_select_kernel<Pol><<<(unsigned)a->rows, SM_THREADS, lds, st>>>(a->logits, (long long)a->logits_stride, V, S, lds_row, a->pos, a->cache_len, a->params,
                                                                       part, tok, a->kept, a->logprob, pa);
  MQ_LAUNCH_CHECK(who);
  return MQ_OK;
}

}  // namespace
}  // namespace mq

using namespace mq;

extern "C" {

int mq_sample(const mq_sample_args* a, mq_stream_t stream) {
  MQ_REQUIRE(a != nullptr, "mq_sample: null argument block");
  if (const int rc = check_sample_args(a, "mq_sample")) return rc;
  return launch_sample<NoPenalty>(a, NoArgs{}, "mq_sample", stream);
}

int mq_sample_penalized(const mq_sample_penalized_args* a, mq_stream_t stream) {
  MQ_REQUIRE(a != nullptr, "mq_sample_penalized: null argument block");
  if (const int rc = check_sample_args(&a->s, "mq_sample_penalized")) return rc;
  MQ_REQUIRE(a->penalty != nullptr && a->history != nullptr, "mq_sample_penalized: null pointer (penalty and history are required; bias is optional)");
  MQ_REQUIRE(aligned(a->penalty, 16) && aligned(a->history, 16) && aligned(a->bias, 8),
             "mq_sample_penalized: penalty and history must be 16-byte aligned, bias 8-byte aligned");
  if (const int rc = check_history_stride(a->history_stride, a->s.V, "mq_sample_penalized")) return rc;
  MQ_REQUIRE(a->observe == 0 || a->observe == 1, "mq_sample_penalized: observe=%d must be 0 or 1", a->observe);
  return launch_sample<Penalty>(&a->s, PenArgs{a->penalty, a->history, (long long)a->history_stride, a->bias, a->observe}, "mq_sample_penalized", stream);
}

int mq_sample_history_prompt(uint32_t* history, int64_t V, const int64_t* ids, int64_t n, int clear, mq_stream_t stream) {
  if (const int rc = check_history(history, V, "mq_sample_history_prompt")) return rc;
  if (const int rc = check_ids(ids, n, "ids", "mq_sample_history_prompt")) return rc;
  MQ_REQUIRE(clear == 0 || clear == 1, "mq_sample_history_prompt: clear=%d must be 0 or 1", clear);
  hipStream_t st = as_stream(stream);
  if (clear) {
    const int n4 = (int)(V / 4);
    history_clear_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, st>>>(reinterpret_cast<uint4*>(history), n4);
    MQ_LAUNCH_CHECK("mq_sample_history_prompt");
  }
  if (n > 0) {
    history_mark_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(history, (int)V, reinterpret_cast<const long long*>(ids), (long long)n);
    MQ_LAUNCH_CHECK("mq_sample_history_prompt");
  }
  return MQ_OK;
}

int mq_sample_rows(const mq_sample_rows_args* a, mq_stream_t stream) {
  MQ_REQUIRE(a != nullptr, "mq_sample_rows: null argument block");
  MQ_REQUIRE(a->n_base != nullptr, "mq_sample_rows: null pointer (n_base is required)");
  const mq_sample_args s = as_sample_args(a, a->n_base, 1);          // (no row is idle: cache_len is unused)
  if (const int rc = check_sample_args(&s, "mq_sample_rows")) return rc;
  MQ_REQUIRE(a->n_offset >= -(1 << 30) && a->n_offset <= (1 << 30), "mq_sample_rows: n_offset=%d outside [-2^30, 2^30]", a->n_offset);
  MQ_REQUIRE(a->rows == 1 || a->proposals != nullptr, "mq_sample_rows: null pointer (proposals holds rows - 1 ids when rows > 1)");
  MQ_REQUIRE(aligned(a->penalty, 16) && aligned(a->history, 16) && aligned(a->bias, 16) && aligned(a->proposals, 8),
             "mq_sample_rows: penalty, history and bias must be 16-byte aligned, proposals 8-byte aligned");
  const RowsArgs ra{a->penalty, a->history, a->bias, reinterpret_cast<const long long*>(a->proposals), (int)a->V, a->n_offset};
  return launch_sample<Rows>(&s, ra, "mq_sample_rows", stream);
}

int mq_sample_ragged(const mq_sample_ragged_args* a, mq_stream_t stream) {
  MQ_REQUIRE(a != nullptr, "mq_sample_ragged: null argument block");
  MQ_REQUIRE(a->row_seq && a->row_pos && a->row_tok, "mq_sample_ragged: null pointer (the row table row_seq / row_pos and row_tok are required)");
  MQ_REQUIRE(a->batch >= 1 && a->batch <= MQ_DECODE_MAX_BATCH, "mq_sample_ragged: batch=%d outside 1..%d", a->batch, MQ_DECODE_MAX_BATCH);
  const mq_sample_args s = as_sample_args(a, a->row_pos, a->cache_len);
  if (const int rc = check_sample_args(&s, "mq_sample_ragged")) return rc;
  MQ_REQUIRE(a->n_offset >= -(1 << 30) && a->n_offset <= (1 << 30), "mq_sample_ragged: n_offset=%d outside [-2^30, 2^30]", a->n_offset);
  MQ_REQUIRE((a->penalty == nullptr && a->history == nullptr) || (a->history_stride >= a->V && a->history_stride % 4 == 0),
             "mq_sample_ragged: history_stride=%lld must be >= V and a multiple of 4 (with a penalty or a history)", (long long)a->history_stride);
  MQ_REQUIRE(aligned(a->row_seq, 4) && aligned(a->row_tok, 8) && aligned(a->penalty, 16) && aligned(a->history, 16) && aligned(a->bias, 8),
             "mq_sample_ragged: penalty and history must be 16-byte aligned, row_tok and bias 8-byte, row_seq 4-byte aligned");
  const RaggedArgs ga{a->row_seq, a->row_pos, reinterpret_cast<const long long*>(a->row_tok), a->penalty, a->history, (long long)a->history_stride,
                      a->bias, a->batch, (int)a->V, a->n_offset};
  return launch_sample<Ragged>(&s, ga, "mq_sample_ragged", stream);
}

int mq_sample_history_count_ragged(uint32_t* history, int64_t history_stride, int64_t V, int batch, const int64_t* pairs, int64_t n, int delta,
                                   mq_stream_t stream) {
  const char* who = "mq_sample_history_count_ragged";
  if (const int rc = check_history(history, V, who)) return rc;
  if (const int rc = check_history_stride(history_stride, V, who)) return rc;
  MQ_REQUIRE(batch >= 1 && batch <= MQ_DECODE_MAX_BATCH, "%s: batch=%d outside 1..%d", who, batch, MQ_DECODE_MAX_BATCH);
  if (const int rc = check_ids(pairs, n, "pairs", who)) return rc;
  MQ_REQUIRE(delta == 1 || delta == -1, "%s: delta=%d must be +1 or -1", who, delta);
  if (n > 0) {
    history_count_ragged_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(history, (long long)history_stride, (int)V, batch,
                                                                                           reinterpret_cast<const long long*>(pairs), (long long)n, delta);
    MQ_LAUNCH_CHECK(who);
  }
  return MQ_OK;
}

int mq_sample_history_count(uint32_t* history, int64_t V, const int64_t* ids, int64_t n, int delta, mq_stream_t stream) {
  if (const int rc = check_history(history, V, "mq_sample_history_count")) return rc;
  if (const int rc = check_ids(ids, n, "ids", "mq_sample_history_count")) return rc;
  MQ_REQUIRE(delta == 1 || delta == -1, "mq_sample_history_count: delta=%d must be +1 or -1", delta);
  if (n > 0) {
    history_count_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(history, (int)V, reinterpret_cast<const long long*>(ids), (long long)n, delta);
    MQ_LAUNCH_CHECK("mq_sample_history_count");
  }
  return MQ_OK;
}

int mq_sample_uniforms(uint64_t seed, uint64_t stream_id, uint32_t n, int64_t first, int64_t count, float* out, mq_stream_t stream) {
  MQ_REQUIRE(out != nullptr, "mq_sample_uniforms: null pointer");
  MQ_REQUIRE(first >= 0 && count >= 1 && count <= (1 << 24) && first + count <= ((int64_t)1 << 34), "mq_sample_uniforms: first=%lld count=%lld outside first >= 0, 1 <= count <= 2^24, first + count <= 2^34",
             (long long)first, (long long)count);
  sample_uniforms_kernel<<<(unsigned)((count + 255) / 256), 256, 0, as_stream(stream)>>>(seed, stream_id, n, (long long)first, (long long)count, out);
  MQ_LAUNCH_CHECK("mq_sample_uniforms");
  return MQ_OK;
}

}  // extern "C"
