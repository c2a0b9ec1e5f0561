// Per-token log-probabilities and top-n alternatives from a raw logits row (mq_logprob_top): what a sampling interface reports as
// `logprobs` / `top_logprobs` with ranks.  A launch of its own behind a selection launch (mq_sample*): it reads the logits row the
// sampler read and the token the sampler wrote.
//
// THE RULE (normative).  Per live row: fp32 logits l[0..V), a chosen token t (int64) and n_top in 0 .. 20.  The logits
// are the RAW row -- no temperature, penalty or bias: the model's distribution.
//   1. l'_i = l_i; a NaN is -inf and -0 counts as +0 (mq_sample's step 1 without the divide).
//   2. Order: l' descending, ties by index ascending (mq_sample's step 2 and its 52-bit key: (monotone u32 of l') << 20 | (2^20 - 1 - i)).
//   3. m = max l'.  m == -inf (every logit -inf or NaN): every lp is -inf, lse is -inf.  Otherwise
//        e_i = (l'_i == m_s) ? 1 : expf(l'_i - m_s)      with m_s the maximum of the SLICE that holds i (below); a slice with m_s = -inf sums to 0
//        S   = the sum of e_i f_s, f_s = (m_s == m) ? 1 : expf(m_s - m), in the fixed order below;   lse = m + logf(S)
//        d_i = (l'_i == m) ? 0 : l'_i - m;     lp_i = d_i - logf(S)        (two fp32 operations, no fma)
//      For a finite m these are (l'_i - m) - logf(S) and expf(l'_i - m): the selects only spell out x - x = 0 and expf(0) = 1.  With a
//      +inf logit they define the result: m = +inf, every finite or -inf entry has e_i = 0 and lp_i = -inf, and the c entries that are
//      +inf share the mass, S = c and lp_i = -logf(c) (0 for a single one).  Ids and rank follow the order as always.
//   4. logprob = lp_t.  rank = 1 + #{i : i is in front of t in the order}.  t outside [0, V): logprob = NaN, rank = 0 (the range is
//      checked before any address is formed from t).
//   5. top_id[k], top_logprob[k], k < n_top: the first n_top tokens of the order and their lp; k >= V: id -1, -inf.  An all -inf row
//      still has the order 0, 1, ... and rank t + 1.  top_logprob[k] carries the bits logprob carries for t = top_id[k]: both are lp_i
//      of step 3, evaluated from l'_i (the key holds its bits), m and logf(S).
// THE ORDER OF THE SUM (a function of V alone).  Slices of 4096 entries: slice s is [4096 s, min(V, 4096 s + 4096)), ns = ceil(V / 4096)
// <= 256.  Inside a slice thread t (of 256) owns the entries lo + 1024 k + 4 t + e, k = 0..3, e = 0..3, and sums its e_i from 0 in the
// order (k, e) (an entry past the slice's end adds +0); the 64 lanes of a wave meet in the xor butterfly a <- a + a[lane ^ o], o = 32, 16,
// 8, 4, 2, 1 (every lane ends with the same bits); the four waves W0..W3 meet as ((W0 + W1) + W2) + W3 = S_s.  The merge: lane j (of 64)
// sums S_s f_s (one rounded product each) from 0 over s = j, j + 64, j + 128, j + 192 (those below ns with m_s > -inf), and the lanes
// meet in the same butterfly.  No floating-point atomics: the bits of S depend on the row's logits and V only -- not on the row count,
// the row's index, its neighbours, logits_stride, the index form, or eager / replayed.  Maxima, counts and the key selection are
// order-free (exact).
//
// The per-slice pass (lp_slice) and the fixed-order row sum (lp_row_stats) live in mq_logprob_slice.h, which mq_beam.hip shares.
// THE KERNELS.  Launch 1 (logprob_slices_kernel, grid ns x rows, 256 threads): a workgroup reads its slice ONCE into registers (16
// entries per thread), writes (m_s, S_s), its count of keys above t's key (l[t]: one uniform load) and its first n_top keys, found by
// n_top rounds of a block arg-max over the thread-local best (the owner of a round's winner removes it and rescans its 16 keys; a DPP
// row reduction per wave and one barrier per round, double-buffered; n_top = 0 runs no round and no pass).  Launch 2 (logprob_merge_kernel, one workgroup per row):
// stages the partials and the at most ns x n_top candidate keys in LDS (44 KiB at most), merges maxima, counts and the sum in the fixed
// order, and picks the first n_top of the candidates as an ns-way merge of the slices' sorted lists (thread s holds list s's head; the
// owner of a round's winner writes that record entry and moves its head on).  ns == 1 (V <= 4096): one launch (logprob_row_kernel)
// runs both bodies.  Every result leaves through ordinary vector stores.  Static LDS only (no launch attribute to set: capturable
// without a warm-up).
//
// WHERE A RECORD GOES.  Three index forms, those of the samplers: (a) pos[rows]: row r is sequence r at n = pos[r], idle when n is
// outside [0, cache_len); (b) n_base: all rows are sequence 0, row j at *n_base + n_offset + j; (c) row_seq / row_pos: row r is sequence
// row_seq[r] at row_pos[r] + n_offset, idle when row_seq[r] is outside [0, batch) or row_pos[r] outside [0, cache_len) -- checked before
// any address is formed from them.  No form: row r at [r][0].  A live row writes its record at [sequence][n] of arrays
// [batch][record_len] ([batch][record_len][n_top] for the alternatives); n outside [0, record_len) writes nothing, an idle row writes
// nothing.  n is read on the device, so a replayed launch lands on the next record.
//
// ERROR BOUND (u = 2^-24, gamma_n = n u / (1 - n u)); the bit contract above is exact, this is the distance to the real-valued
// log-softmax of l'.  ASSUMED: the device expf and logf are within 1 ulp (relative 2 u); not measured here.  A term of S carries: the
// rounding of l'_i - m_s and of m_s - m, u (m_s - l'_i) + u (m - m_s) = u (m - l'_i) in the exponent; two expf, 2 u each; the product,
// u; the additions it passes through, at most 16 + 6 + 3 in its slice and 4 + 6 in the merge, gamma_35.  Weighted by p_i the exponent
// term sums to at most u log V (sum_i p_i (m - l'_i) = log p_max + H(p) <= log V), so relative to S
//     E_S = 1.01 (u log V + 5 u + gamma_35)                      (1.01: the second-order terms)
// logf(S) adds 2 u log S <= 2 u log V (1 <= S <= V); d_i is rounded once, u |l'_i - m| <= u |lp_i|; the final subtraction once, u |lp_i|:
//     |lp^_i - lp_i| <= E_S + 2 u log V + 2 u |lp_i|
// V = 2^20, |lp| = 34 (Gaussian logits of scale 3): 3.2e-6 + 1.7e-6 + 4.1e-6 = 9.0e-6.  tests/test_gpu_logprob.py evaluates the formula per entry.
#include "mq_logprob_slice.h"

#include <limits.h>

namespace mq {
namespace {

struct LpIndex {
  const int* pos;                 // (a)
  const int* n_base;              // (b)
  const int* row_seq;             // (c)
  const int* row_pos;
  int n_offset, batch, cache_len, record_len;
};

struct LpArgs {
  const float* logits;
  long long stride;
  int V, S, n_top;
  const long long* tok;
  LpIndex ix;
  float* logprob;
  int* rank;
  int* top_id;
  float* top_logprob;
  LpPart* part;                   // [rows][LP_MAX_SLICES]
  u64* keys;                      // [rows][LP_MAX_SLICES][LP_MAX_TOP]
};

// The record a row writes, as an element offset into [batch][record_len]; false: the row is idle or its index is outside the record.
// Every table entry is range-checked before it addresses anything.  Workgroup-uniform.
__device__ __forceinline__ bool lp_record(const LpIndex& x, int row, long long* rec) {
  long long seq = row, n = 0;
  if (x.row_seq) {
    const int s = x.row_seq[row], p = x.row_pos[row];
    if (s < 0 || s >= x.batch || p < 0 || p >= x.cache_len) return false;
    seq = s;
    n = (long long)p + x.n_offset;
  } else if (x.n_base) {
    seq = 0;
    n = (long long)x.n_base[0] + x.n_offset + row;
  } else if (x.pos) {
    n = x.pos[row];
    if (n < 0 || n >= x.cache_len) return false;
  }
  if (n < 0 || n >= x.record_len) return false;
  *rec = seq * x.record_len + n;
  return true;
}

// The row's record from its ns partials and candidate lists (both in LDS).
__device__ __forceinline__ void lp_finish(const float* __restrict__ row, int V, int ns, long long t, int n_top, const LpPart* part, const u64* cand,
                                          long long rec, const LpArgs& a, LpRed& R) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float NEG_INF = -__builtin_inff();
  float m, log_s;
  int in_front;
  lp_row_stats(part, ns, R, &m, &log_s, &in_front);                  // (the fixed-order sum: mq_logprob_slice.h)

  if (tid == 0) {
    const bool have_t = t >= 0 && t < (long long)V;
    a.logprob[rec] = have_t ? lp_of(lp_norm(row[t]), m, log_s) : __builtin_nanf("");
    a.rank[rec] = have_t ? 1 + in_front : 0;
  }

  // the first n_top of the candidates: an ns-way merge of the slices' sorted lists, thread s at the head of list s
  int head = 0;
  u64 cur = (tid < ns && n_top > 0) ? cand[tid * LP_MAX_TOP] : 0ull;
  int* top_id = a.top_id + rec * n_top;
  float* top_lp = a.top_logprob + rec * n_top;
  for (int r = 0; r < n_top; ++r) {
    const u64 wb = lp_wave_max_k(cur);
    if (lane == 0) R.k[r & 1][wave] = wb;
    lp_sync();
    u64 g = R.k[r & 1][0];
#pragma unroll
    for (int w = 1; w < LP_WAVES; ++w) g = R.k[r & 1][w] > g ? R.k[r & 1][w] : g;
    if (g == 0ull) {                                                 // fewer than n_top entries (k >= V)
      if (tid == 0) { top_id[r] = -1; top_lp[r] = NEG_INF; }
    } else if (cur == g) {                                           // keys are distinct: one owner
      top_id[r] = sort_key_id(g);
      top_lp[r] = lp_of(sort_key_value(g), m, log_s);
      ++head;
      cur = head < n_top ? cand[tid * LP_MAX_TOP + head] : 0ull;
    }
  }
}

__global__ __launch_bounds__(LP_THREADS) void logprob_slices_kernel(LpArgs a) {
  __shared__ LpRed R;
  const int row = blockIdx.y, s = blockIdx.x;
  long long rec;
  if (!lp_record(a.ix, row, &rec)) return;                           // workgroup-uniform
  const long long o = (long long)row * LP_MAX_SLICES + s;
  lp_slice(a.logits + (long long)row * a.stride, a.V, s, a.tok[row], a.n_top, a.part + o, a.keys + o * LP_MAX_TOP, R);
}

__global__ __launch_bounds__(LP_THREADS) void logprob_merge_kernel(LpArgs a) {
  __shared__ LpRed R;
  __shared__ LpPart part[LP_MAX_SLICES];
  __shared__ u64 cand[LP_MAX_SLICES * LP_MAX_TOP];
  const int row = blockIdx.x, tid = threadIdx.x;
  long long rec;
  if (!lp_record(a.ix, row, &rec)) return;                           // workgroup-uniform
  const long long o = (long long)row * LP_MAX_SLICES;
  if (tid < a.S) {
    part[tid] = a.part[o + tid];
    for (int r = 0; r < a.n_top; ++r) cand[tid * LP_MAX_TOP + r] = a.keys[(o + tid) * LP_MAX_TOP + r];
  }
  lp_sync();
  lp_finish(a.logits + (long long)row * a.stride, a.V, a.S, a.tok[row], a.n_top, part, cand, rec, a, R);
}

// V <= LP_SLICE: both bodies in one launch
__global__ __launch_bounds__(LP_THREADS) void logprob_row_kernel(LpArgs a) {
  __shared__ LpRed R1, R2;
  __shared__ LpPart part[1];
  __shared__ u64 cand[LP_MAX_TOP];
  const int row = blockIdx.x;
  long long rec;
  if (!lp_record(a.ix, row, &rec)) return;                           // workgroup-uniform
  const float* lrow = a.logits + (long long)row * a.stride;
  const long long t = a.tok[row];
  lp_slice(lrow, a.V, 0, t, a.n_top, part, cand, R1);
  lp_sync();
  lp_finish(lrow, a.V, 1, t, a.n_top, part, cand, rec, a, R2);
}

}  // namespace
}  // namespace mq

using namespace mq;

extern "C" {

int mq_logprob_top(const mq_logprob_top_args* a, mq_stream_t stream) {
  MQ_REQUIRE(a != nullptr, "mq_logprob_top: null argument block");
  MQ_REQUIRE(a->logits && a->tok && a->logprob && a->rank,
             "mq_logprob_top: null pointer (logits, tok, logprob and rank are required; top_id / top_logprob go together, with n_top > 0)");
  MQ_REQUIRE(a->rows >= 1 && a->rows <= MQ_DECODE_MAX_BATCH, "mq_logprob_top: rows=%d outside 1..%d", a->rows, MQ_DECODE_MAX_BATCH);
  MQ_REQUIRE(a->V >= 4 && a->V % 4 == 0 && a->V <= (1 << 20), "mq_logprob_top: V=%lld must be a multiple of 4 in [4, 2^20]", (long long)a->V);
  MQ_REQUIRE(a->logits_stride >= a->V && a->logits_stride % 4 == 0, "mq_logprob_top: logits_stride=%lld must be >= V and a multiple of 4",
             (long long)a->logits_stride);
  MQ_REQUIRE(a->n_top >= 0 && a->n_top <= MQ_LOGPROB_MAX_TOP, "mq_logprob_top: n_top=%d outside 0..%d", a->n_top, MQ_LOGPROB_MAX_TOP);
  MQ_REQUIRE((a->top_id != nullptr) == (a->top_logprob != nullptr), "mq_logprob_top: top_id and top_logprob go together (one of them is null)");
  MQ_REQUIRE(a->n_top == 0 || a->top_id != nullptr, "mq_logprob_top: n_top=%d needs top_id and top_logprob", a->n_top);
  MQ_REQUIRE(a->scratch != nullptr, "mq_logprob_top: null pointer (scratch is required)");
  MQ_REQUIRE(a->scratch_bytes >= MQ_LOGPROB_SCRATCH_BYTES, "mq_logprob_top: scratch_bytes=%lld below MQ_LOGPROB_SCRATCH_BYTES", (long long)a->scratch_bytes);
  MQ_REQUIRE((a->row_seq != nullptr) == (a->row_pos != nullptr), "mq_logprob_top: row_seq and row_pos go together (one of them is null)");
  const int forms = (a->pos ? 1 : 0) + (a->n_base ? 1 : 0) + (a->row_seq ? 1 : 0);
  MQ_REQUIRE(forms <= 1, "mq_logprob_top: more than one index form (pass pos, or n_base, or row_seq / row_pos, or none)");
  MQ_REQUIRE(a->batch >= 1 && a->batch <= MQ_DECODE_MAX_BATCH, "mq_logprob_top: batch=%d outside 1..%d", a->batch, MQ_DECODE_MAX_BATCH);
  MQ_REQUIRE(a->n_base || a->row_seq || a->rows <= a->batch, "mq_logprob_top: rows=%d above batch=%d (row r is sequence r)", a->rows, a->batch);
  MQ_REQUIRE(a->record_len >= 1, "mq_logprob_top: record_len=%d must be >= 1", a->record_len);
  MQ_REQUIRE(!(a->pos || a->row_seq) || a->cache_len >= 1, "mq_logprob_top: cache_len=%d must be >= 1 (a row outside [0, cache_len) is idle)", a->cache_len);
  MQ_REQUIRE(a->n_offset >= -(1 << 30) && a->n_offset <= (1 << 30), "mq_logprob_top: n_offset=%d outside [-2^30, 2^30]", a->n_offset);
  MQ_REQUIRE(aligned(a->logits, 16) && aligned(a->scratch, 16), "mq_logprob_top: logits and scratch must be 16-byte aligned");
  MQ_REQUIRE(aligned(a->tok, 8) && aligned(a->pos, 4) && aligned(a->n_base, 4) && aligned(a->row_seq, 4) && aligned(a->row_pos, 4) &&
                 aligned(a->logprob, 4) && aligned(a->rank, 4) && aligned(a->top_id, 4) && aligned(a->top_logprob, 4),
             "mq_logprob_top: tok must be 8-byte, the index tables and the outputs 4-byte aligned");
  LpArgs k;
  k.logits = a->logits;
  k.stride = (long long)a->logits_stride;
  k.V = (int)a->V;
  k.S = (k.V + LP_SLICE - 1) / LP_SLICE;
  k.n_top = a->n_top;
  k.tok = reinterpret_cast<const long long*>(a->tok);
  k.ix = LpIndex{a->pos, a->n_base, a->row_seq, a->row_pos, a->n_offset, a->batch, a->cache_len, a->record_len};
  k.logprob = a->logprob;
  k.rank = a->rank;
  k.top_id = a->top_id;
  k.top_logprob = a->top_logprob;
  k.part = static_cast<LpPart*>(a->scratch);
  k.keys = reinterpret_cast<u64*>(static_cast<char*>(a->scratch) + (size_t)MQ_DECODE_MAX_BATCH * LP_MAX_SLICES * sizeof(LpPart));
  hipStream_t st = as_stream(stream);
  if (k.S == 1) {
    logprob_row_kernel<<<(unsigned)a->rows, LP_THREADS, 0, st>>>(k);
    MQ_LAUNCH_CHECK("mq_logprob_top");
    return MQ_OK;
  }
  logprob_slices_kernel<<<dim3((unsigned)k.S, (unsigned)a->rows), LP_THREADS, 0, st>>>(k);
  MQ_LAUNCH_CHECK("mq_logprob_top");
  logprob_merge_kernel<<<(unsigned)a->rows, LP_THREADS, 0, st>>>(k);
  MQ_LAUNCH_CHECK("mq_logprob_top");
  return MQ_OK;
}

}  // extern "C"
