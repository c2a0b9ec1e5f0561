// The best continuations of a group of beams from their raw logits rows (mq_beam_select): the device half of a beam-search step.  W
// beams of one prompt are W rows of the batched engine's logits; the step needs the group's best K = 2 W (token, beam) pairs by summed
// log-probability.  Instead of reading W rows back (W x 128 KB at V = 32 000) the host reads n_groups x K records.
//
// THE RULE (normative).  logits [rows][logits_stride] fp32, the RAW rows; cum [rows] fp32, the beams' summed
// log-probabilities; group [rows] int32; n_groups; K = n_cand in 1 .. MQ_LOGPROB_MAX_TOP.  All device data.
//   MEMBERSHIP.  Row r belongs to group g = group[r] iff 0 <= g < n_groups (range-checked before any address is formed from it).  Any
//     other value -- -1, n_groups, INT_MIN, INT_MAX -- makes r a member of nothing: its logits and its cum are never read and have no
//     influence, whatever garbage they hold.
//   PER MEMBER ROW.  The order and the log-probabilities lp_i are those of mq_logprob_top's rule (csrc/mq_logprob.hip), steps 1 - 3:
//     l'_i (NaN -> -inf, -0 -> +0), l' descending with ties by index ascending, the same slices and the same fixed order of the sum, the
//     same m, logf(S) and lp_i = d_i - logf(S).  The row's list is the first K entries of that order (min(K, V) of them); lp carries
//     the bits mq_logprob_top writes as top_logprob[k] for that row: both run ONE body (mq_logprob_slice.h).  row_lse[r] = m + logf(S)
//     (-inf for an all -inf row, +inf with a +inf logit).
//   CANDIDATE SCORE.  Candidate (r, k), k-th of row r's list, scores s = cum'_r + lp: ONE fp32 addition (no fma), with cum'_r = cum[r],
//     a NaN cum counting as -inf; -0 counts as +0 (s + 0); a NaN sum (cum = +inf with lp = -inf) counts as -inf.
//   GROUP ORDER.  s descending, ties by r ascending, then by k ascending.  Within a row s is non-increasing along the row's order
//     (fp32 addition is monotone), so the group's first K candidates always lie inside the union of its rows' first-K lists.
//   OUTPUTS.  For g < n_groups and j < K: cand_score / cand_row / cand_token / cand_logprob [n_groups][K] hold the j-th candidate of
//     group g: s, r, the token id and lp.  A group with fewer than K candidates (no member, or V < K with one member) pads with score
//     -inf, row -1, token -1, logprob -inf.  row_lse [rows] is written for member rows only; no input is written.
//   INVARIANCE.  Every output bit of a group is a function of its member rows' logits, their cum, their relative order, K and V only
//     (cand_row names the rows by their indices) -- not of the other groups, of which rows the members occupy beyond their order, of
//     logits_stride, or of eager / replayed execution.  No floating-point atomics; maxima, counts and ranks are exact in any order.
//
// THE KERNELS.  Launch 1 (beam_slices_kernel, grid ns x rows): mq_logprob's per-slice pass (lp_slice: one read of the row, (m_s, S_s),
// the slice's first K keys) for member rows.  Launch 2 (beam_rows_kernel, one workgroup per row): stages a row's partials and ns x K
// candidate keys in LDS (44 KiB at most -- eight rows' lists do not fit at once, hence a workgroup per row), takes m and logf(S) in the
// fixed order (lp_row_stats), writes row_lse and merges the ns sorted lists to the row's K entries (key, lp) in scratch.  V <= 4096:
// launches 1 and 2 are one (beam_row_kernel).  Launch 3 (beam_groups_kernel, one workgroup per group): thread t < 8 x 20 owns entry
// (r, k) = (t / 20, t % 20), scores it, and its rank is the number of entries whose 64-bit key ((monotone u32 of s) << 32 | (255 - t))
// is larger -- 160 LDS reads; the entries of rank < K write themselves.  Every result leaves through ordinary vector stores.  Static
// LDS only, no launch attribute, no host synchronisation: capturable without a warm-up.  Scratch (MQ_BEAM_SCRATCH_BYTES) is owned by
// the call on its stream.
#include "mq_logprob_slice.h"

namespace mq {
namespace {

constexpr int BM_ENTRIES = MQ_DECODE_MAX_BATCH * LP_MAX_TOP;          // 160 scored entries per group at most

struct BeamEntry {
  u64 key;                        // the logit's key (0: the row has no k-th entry)
  float lp;
  int pad;
};

static_assert(MQ_BEAM_SCRATCH_BYTES == MQ_LOGPROB_SCRATCH_BYTES + BM_ENTRIES * sizeof(BeamEntry), "scratch: the slices' partials and keys, then every row's list");
static_assert(BM_ENTRIES <= LP_THREADS && BM_ENTRIES <= 256, "one thread per entry; the entry index fits the key's low byte");

struct BeamArgs {
  const float* logits;
  long long stride;
  int V, S, K, rows, n_groups;
  const float* cum;
  const int* group;
  float* cand_score;
  int* cand_row;
  int* cand_token;
  float* cand_logprob;
  float* row_lse;
  LpPart* part;                   // [rows][LP_MAX_SLICES]
  u64* keys;                      // [rows][LP_MAX_SLICES][LP_MAX_TOP]
  BeamEntry* list;                // [rows][LP_MAX_TOP]
};

// Is the row a member of some group?  (workgroup-uniform; the only use of a group entry besides the comparison in the group kernel)
__device__ __forceinline__ bool beam_member(const BeamArgs& a, int row) {
  const int g = a.group[row];
  return g >= 0 && g < a.n_groups;
}

// A member row's lse and list from its ns partials and candidate lists (both in LDS).
__device__ __forceinline__ void beam_finish(int row, int ns, const LpPart* part, const u64* cand, const BeamArgs& a, LpRed& R) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float m, log_s;
  int in_front;
  lp_row_stats(part, ns, R, &m, &log_s, &in_front);
  if (tid == 0) a.row_lse[row] = m + log_s;                          // (m = -inf: log_s is 0)

  // the first K of the candidates: mq_logprob's ns-way merge of the slices' sorted lists, thread s at the head of list s
  int head = 0;
  u64 cur = tid < ns ? cand[tid * LP_MAX_TOP] : 0ull;
  BeamEntry* list = a.list + (long long)row * LP_MAX_TOP;
  for (int r = 0; r < a.K; ++r) {
    const u64 wb = lp_wave_max_k(cur);
    if (lane == 0) R.k[r & 1][wave] = wb;
    lp_sync();
    u64 g = R.k[r & 1][0];
#pragma unroll
    for (int w = 1; w < LP_WAVES; ++w) g = R.k[r & 1][w] > g ? R.k[r & 1][w] : g;
    if (g == 0ull) {                                                 // fewer than K entries (k >= V)
      if (tid == 0) list[r] = BeamEntry{0ull, -__builtin_inff(), 0};
    } else if (cur == g) {                                           // keys are distinct: one owner
      list[r] = BeamEntry{g, lp_of(sort_key_value(g), m, log_s), 0};
      ++head;
      cur = head < a.K ? cand[tid * LP_MAX_TOP + head] : 0ull;
    }
  }
}

__global__ __launch_bounds__(LP_THREADS) void beam_slices_kernel(BeamArgs a) {
  __shared__ LpRed R;
  const int row = blockIdx.y, s = blockIdx.x;
  if (!beam_member(a, row)) return;                                  // workgroup-uniform
  const long long o = (long long)row * LP_MAX_SLICES + s;
  lp_slice(a.logits + (long long)row * a.stride, a.V, s, -1, a.K, a.part + o, a.keys + o * LP_MAX_TOP, R);
}

__global__ __launch_bounds__(LP_THREADS) void beam_rows_kernel(BeamArgs a) {
  __shared__ LpRed R;
  __shared__ LpPart part[LP_MAX_SLICES];
  __shared__ u64 cand[LP_MAX_SLICES * LP_MAX_TOP];
  const int row = blockIdx.x, tid = threadIdx.x;
  if (!beam_member(a, row)) return;                                  // workgroup-uniform
  const long long o = (long long)row * LP_MAX_SLICES;
  if (tid < a.S) {
    part[tid] = a.part[o + tid];
    for (int r = 0; r < a.K; ++r) cand[tid * LP_MAX_TOP + r] = a.keys[(o + tid) * LP_MAX_TOP + r];
  }
  lp_sync();
  beam_finish(row, a.S, part, cand, a, R);
}

// V <= LP_SLICE: both bodies in one launch
__global__ __launch_bounds__(LP_THREADS) void beam_row_kernel(BeamArgs a) {
  __shared__ LpRed R1, R2;
  __shared__ LpPart part[1];
  __shared__ u64 cand[LP_MAX_TOP];
  const int row = blockIdx.x;
  if (!beam_member(a, row)) return;                                  // workgroup-uniform
  lp_slice(a.logits + (long long)row * a.stride, a.V, 0, -1, a.K, part, cand, R1);
  lp_sync();
  beam_finish(row, 1, part, cand, a, R2);
}

// The group's first K candidates: every entry's rank among the at most 160 scored entries of the group's rows.
__global__ __launch_bounds__(LP_THREADS) void beam_groups_kernel(BeamArgs a) {
  __shared__ u64 sk[BM_ENTRIES];
  const int g = blockIdx.x, t = threadIdx.x;                         // g < n_groups by the grid
  const int r = t / LP_MAX_TOP, k = t % LP_MAX_TOP;
  const float NEG_INF = -__builtin_inff();
  BeamEntry e = BeamEntry{0ull, NEG_INF, 0};
  float s = NEG_INF;
  u64 mine = 0ull;
  if (r < a.rows && k < a.K && a.group[r] == g) {                    // (r, k) in range before anything is read through them
    e = a.list[r * LP_MAX_TOP + k];
    if (e.key != 0ull) {
      float c = a.cum[r];
      c = c != c ? NEG_INF : c;
      s = c + e.lp;
      s = s != s ? NEG_INF : s + 0.f;
      const unsigned u = __float_as_uint(s);
      mine = ((u64)((u & 0x80000000u) ? ~u : (u | 0x80000000u)) << 32) | (u64)(255 - t);     // (never 0)
    }
  }
  if (t < BM_ENTRIES) sk[t] = mine;
  lp_sync();
  int rank = 0, n = 0;
#pragma unroll 8
  for (int j = 0; j < BM_ENTRIES; ++j) {
    const u64 o = sk[j];                                             // (a broadcast read)
    rank += o > mine ? 1 : 0;
    n += o != 0ull ? 1 : 0;
  }
  const long long base = (long long)g * a.K;
  if (mine != 0ull && rank < a.K) {
    a.cand_score[base + rank] = s;
    a.cand_row[base + rank] = r;
    a.cand_token[base + rank] = sort_key_id(e.key);
    a.cand_logprob[base + rank] = e.lp;
  }
  if (t < a.K && t >= n) {                                           // fewer than K candidates: the padding
    a.cand_score[base + t] = NEG_INF;
    a.cand_row[base + t] = -1;
    a.cand_token[base + t] = -1;
    a.cand_logprob[base + t] = NEG_INF;
  }
}

}  // namespace
}  // namespace mq

using namespace mq;

extern "C" {

int mq_beam_select(const mq_beam_select_args* a, mq_stream_t stream) {
  MQ_REQUIRE(a != nullptr, "mq_beam_select: null argument block");
  MQ_REQUIRE(a->logits && a->cum && a->group && a->cand_score && a->cand_row && a->cand_token && a->cand_logprob && a->row_lse,
             "mq_beam_select: null pointer (logits, cum, group, cand_score, cand_row, cand_token, cand_logprob and row_lse are required)");
  MQ_REQUIRE(a->rows >= 1 && a->rows <= MQ_DECODE_MAX_BATCH, "mq_beam_select: rows=%d outside 1..%d", a->rows, MQ_DECODE_MAX_BATCH);
  MQ_REQUIRE(a->V >= 4 && a->V % 4 == 0 && a->V <= (1 << 20), "mq_beam_select: V=%lld must be a multiple of 4 in [4, 2^20]", (long long)a->V);
  MQ_REQUIRE(a->logits_stride >= a->V && a->logits_stride % 4 == 0, "mq_beam_select: logits_stride=%lld must be >= V and a multiple of 4",
             (long long)a->logits_stride);
  MQ_REQUIRE(a->n_groups >= 1 && a->n_groups <= MQ_DECODE_MAX_BATCH, "mq_beam_select: n_groups=%d outside 1..%d", a->n_groups, MQ_DECODE_MAX_BATCH);
  MQ_REQUIRE(a->n_cand >= 1 && a->n_cand <= MQ_LOGPROB_MAX_TOP, "mq_beam_select: n_cand=%d outside 1..%d", a->n_cand, MQ_LOGPROB_MAX_TOP);
  MQ_REQUIRE(a->scratch != nullptr, "mq_beam_select: null pointer (scratch is required)");
  MQ_REQUIRE(a->scratch_bytes >= MQ_BEAM_SCRATCH_BYTES, "mq_beam_select: scratch_bytes=%lld below MQ_BEAM_SCRATCH_BYTES", (long long)a->scratch_bytes);
  MQ_REQUIRE(aligned(a->logits, 16) && aligned(a->scratch, 16), "mq_beam_select: logits and scratch must be 16-byte aligned");
  MQ_REQUIRE(aligned(a->cum, 4) && aligned(a->group, 4) && aligned(a->cand_score, 4) && aligned(a->cand_row, 4) && aligned(a->cand_token, 4) &&
                 aligned(a->cand_logprob, 4) && aligned(a->row_lse, 4),
             "mq_beam_select: cum, group and the outputs must be 4-byte aligned");
  BeamArgs k;
  k.logits = a->logits;
  k.stride = (long long)a->logits_stride;
  k.V = (int)a->V;
  k.S = (k.V + LP_SLICE - 1) / LP_SLICE;
  k.K = a->n_cand;
  k.rows = a->rows;
  k.n_groups = a->n_groups;
  k.cum = a->cum;
  k.group = a->group;
  k.cand_score = a->cand_score;
  k.cand_row = a->cand_row;
  k.cand_token = a->cand_token;
  k.cand_logprob = a->cand_logprob;
  k.row_lse = a->row_lse;
  char* const sc = static_cast<char*>(a->scratch);
  k.part = reinterpret_cast<LpPart*>(sc);
  k.keys = reinterpret_cast<u64*>(sc + (size_t)MQ_DECODE_MAX_BATCH * LP_MAX_SLICES * sizeof(LpPart));
  k.list = reinterpret_cast<BeamEntry*>(sc + (size_t)MQ_LOGPROB_SCRATCH_BYTES);
  hipStream_t st = as_stream(stream);
  if (k.S == 1) {
    beam_row_kernel<<<(unsigned)a->rows, LP_THREADS, 0, st>>>(k);
    MQ_LAUNCH_CHECK("mq_beam_select");
  } else {
    beam_slices_kernel<<<dim3((unsigned)k.S, (unsigned)a->rows), LP_THREADS, 0, st>>>(k);
    MQ_LAUNCH_CHECK("mq_beam_select");
    beam_rows_kernel<<<(unsigned)a->rows, LP_THREADS, 0, st>>>(k);
    MQ_LAUNCH_CHECK("mq_beam_select");
  }
  beam_groups_kernel<<<(unsigned)a->n_groups, LP_THREADS, 0, st>>>(k);
  MQ_LAUNCH_CHECK("mq_beam_select");
  return MQ_OK;
}

}  // extern "C"
