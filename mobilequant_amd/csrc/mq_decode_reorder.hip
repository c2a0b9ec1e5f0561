// Re-order the slots of the batched decode engine's int8 KV caches in place (mq_decode_cache_reorder): the cache half of a beam-search
// step, which assigns "slot d continues old slot parent[d]" for all d AT ONCE -- a permutation with fan-out.  mq_decode_cache_fork
// (mq_decode_fork.hip) refuses exactly that: there a source is never a destination.  Here swaps, cycles, chains and fan-out from a slot
// that is itself overwritten are all served by one launch, with no second buffer.
//
// THE RULE (normative).  caches[c], c < n_caches, is [batch][kv_heads][cache_len][head_dim] int8, contiguous, 16-byte
// aligned; pos [batch] is the engines' position vector (cache_len = idle) and parent [batch] the assignment, both DEVICE data.
//   - Slot d is a LIVE DESTINATION iff, with p = parent[d]:  0 <= p < batch;  p != d;  0 < pos[p] < cache_len.
//   - For a live destination, for every cache c and head h, bytes [0, pos[p] * head_dim) of caches[c][d][h] become those of
//     caches[c][p][h] AS THEY WERE BEFORE THE CALL: a simultaneous assignment.  A source may itself be a live destination: a swap
//     (0 <- 1, 1 <- 0), a cycle, a chain (1 <- 2 <- 3: slot 1 gets old 2, slot 2 gets old 3), a fan-out from a slot that is overwritten.
//   - Nothing else is written: no byte at or past pos[p] of a destination, no byte of a slot that is not a live destination, and pos
//     itself never.  parent[d] == d (the identity) writes nothing.
//   - Every table entry is range-checked before any address is formed from it.  No-ops for the affected slot: an entry -1, batch,
//     INT_MIN or INT_MAX; an idle source; pos[p] == 0.
//   - Both tables are read on the device: one captured launch serves any later table.  No host synchronisation.
//
// WHY NO HAZARD EXISTS.  The grid has NO dimension over slots: (blocks of 16-byte chunks of a head) x (cache, head).  The thread that
// owns chunk i of (cache, head) loads chunk i of every slot that some live destination takes (where i is below that source's live
// length), waits for all of them, and only then stores; no other thread ever touches chunk i of any slot of that (cache, head).  So
// every load sees the bytes from before the call whatever order the workgroups run in: no second buffer, no ordering between
// workgroups.
//
// THE KERNEL.  256 threads, one chunk per thread and round.  The tables arrive through uniform loads into compile-time indexed
// scalars (parent[d], the live chunks of slot s): the (source, destination) double loop is fully unrolled under uniform tests, the eight
// chunk registers are compile-time indexed and every load is unconditional (a lane past a source's live length re-reads that source's
// chunk 0, which is live) -- mq_decode_fork.hip's warning: a run-time indexed array or loads behind a lane condition sent that kernel's
// registers to LDS.  Checked in the ISA: no private segment, no LDS.  Plain 16-byte vector loads and stores (the lines stay in the L2:
// the next step's attention reads them).  The grid's first dimension is sized from cache_len (the positions are device data) and capped
// at RO_MAX_XBLOCKS; past that a workgroup goes round its chunk loop.  No launch attribute: capturable without a warm-up.
#include "mq_common.h"

namespace mq {
namespace {

constexpr int RO_THREADS = 256;
constexpr int RO_MAX_XBLOCKS = 16;                            // 64 KiB of a head per round of the grid: a wave amortises its prologue
constexpr int RO_MAX_CACHES = 1024;
constexpr long long RO_MAX_GRID_Y = 65535;
constexpr int RO_SLOTS = MQ_DECODE_MAX_BATCH;

typedef unsigned ro_chunk __attribute__((ext_vector_type(4)));        // 16 bytes: one global_load / global_store_dwordx4 per lane
static_assert(RO_SLOTS == 8, "the wait between the loads and the stores names eight chunk registers");

struct ReorderArgs {
  int8_t* const* caches;
  int batch, kv_heads, cache_len, head_dim;
  long long head_chunks;                                      // cache_len * head_dim / 16: a head's allocation in 16-byte chunks
  const int* pos;
  const int* parent;
};

__global__ __launch_bounds__(RO_THREADS) void cache_reorder_kernel(ReorderArgs a) {
  // The tables, range-checked: live[s] is 0 unless s < batch and 0 < pos[s] < cache_len; src[d] is -1 unless d is a live destination.
  // Every entry is loaded unconditionally (slot s >= batch through the clamped index batch - 1), and everything up to the first exit
  // is selects, not branches: this prologue runs in EVERY wave of a grid that is sized from cache_len, and a grid of mostly idle
  // workgroups is bound by it.
  int par[RO_SLOTS], at[RO_SLOTS];
  long long live[RO_SLOTS];
#pragma unroll
  for (int s = 0; s < RO_SLOTS; ++s) {
    const int c = s < a.batch ? s : a.batch - 1;
    par[s] = a.parent[c];
    at[s] = a.pos[c];
  }
  long long top = 0;
#pragma unroll
  for (int s = 0; s < RO_SLOTS; ++s) {
    par[s] = s < a.batch ? par[s] : -1;
    const int p = s < a.batch ? at[s] : 0;
    live[s] = (long long)((p > 0 && p < a.cache_len) ? p : 0) * (a.head_dim >> 4);
    top = live[s] > top ? live[s] : top;
  }
  const long long i_first = (long long)blockIdx.x * RO_THREADS;
  if (i_first >= top) return;                                 // past every slot's live chunks: the cheap exit of most of a long cache's grid
  int src[RO_SLOTS];
  unsigned need = 0;                                          // bit s: some live destination takes slot s
  long long most = 0;
#pragma unroll
  for (int d = 0; d < RO_SLOTS; ++d) {
    const int p = par[d];                                     // (-1 for d >= batch)
    long long lv = 0;
#pragma unroll
    for (int s = 0; s < RO_SLOTS; ++s) lv = (s != d && p == s) ? live[s] : lv;      // (p == s: 0 <= p < 8, and live[s] > 0: s < batch)
    src[d] = lv > 0 ? p : -1;
    need |= lv > 0 ? 1u << (p & 7) : 0u;
    most = lv > most ? lv : most;
  }
  if (need == 0 || i_first >= most) return;                   // workgroup-uniform, before any cache is touched

  const int c = (int)blockIdx.y / a.kv_heads, h = (int)blockIdx.y % a.kv_heads;
  ro_chunk* const base = reinterpret_cast<ro_chunk*>(a.caches[c]) + (long long)h * a.head_chunks;
  const long long slot_chunks = (long long)a.kv_heads * a.head_chunks;
  const long long round = (long long)gridDim.x * RO_THREADS;
  for (long long i = i_first + threadIdx.x; i < most; i += round) {
    ro_chunk v[RO_SLOTS];
#pragma unroll
    for (int s = 0; s < RO_SLOTS; ++s) {
      v[s] = ro_chunk{0u, 0u, 0u, 0u};
      if (need >> s & 1u) v[s] = base[(long long)s * slot_chunks + (i < live[s] ? i : 0)];       // uniform test, unconditional load
    }
    // every load of chunk i has landed before its first store.  The chunks pass THROUGH the statement: the compiler then knows them
    // settled and puts no wait of its own in front of a store (vmcnt counts stores too: such a wait would hold every store until the
    // one before it had completed)
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7])
                 :
                 : "memory");
#pragma unroll
    for (int d = 0; d < RO_SLOTS; ++d)
#pragma unroll
      for (int s = 0; s < RO_SLOTS; ++s)
        if (src[d] == s) {                                    // uniform
          if (i < live[s]) base[(long long)d * slot_chunks + i] = v[s];
        }
  }
}

}  // namespace
}  // namespace mq

using namespace mq;

extern "C" {

int mq_decode_cache_reorder(const mq_decode_cache_fork_args* a, mq_stream_t stream) {
  MQ_REQUIRE(a != nullptr, "mq_decode_cache_reorder: null argument block");
  MQ_REQUIRE(a->caches && a->pos && a->parent, "mq_decode_cache_reorder: null pointer (caches, pos and parent are required)");
  MQ_REQUIRE(a->n_caches >= 1 && a->n_caches <= RO_MAX_CACHES, "mq_decode_cache_reorder: n_caches=%d outside 1..%d", a->n_caches, RO_MAX_CACHES);
  MQ_REQUIRE(a->batch >= 1 && a->batch <= MQ_DECODE_MAX_BATCH, "mq_decode_cache_reorder: batch=%d outside 1..%d", a->batch, MQ_DECODE_MAX_BATCH);
  MQ_REQUIRE(a->kv_heads >= 1, "mq_decode_cache_reorder: kv_heads=%d must be >= 1", a->kv_heads);
  MQ_REQUIRE(a->cache_len >= 1, "mq_decode_cache_reorder: cache_len=%d must be >= 1", a->cache_len);
  MQ_REQUIRE(a->head_dim >= 16 && a->head_dim <= 256 && a->head_dim % 16 == 0,
             "mq_decode_cache_reorder: head_dim=%d must be a multiple of 16 in [16, 256]", a->head_dim);
  MQ_REQUIRE((long long)a->n_caches * a->kv_heads <= RO_MAX_GRID_Y, "mq_decode_cache_reorder: n_caches x kv_heads = %lld above %lld (one grid row each)",
             (long long)a->n_caches * a->kv_heads, RO_MAX_GRID_Y);
  MQ_REQUIRE(aligned(a->caches, 8) && aligned(a->pos, 4) && aligned(a->parent, 4),
             "mq_decode_cache_reorder: the pointer table must be 8-byte, pos and parent 4-byte aligned");
  ReorderArgs k;
  k.caches = a->caches;
  k.batch = a->batch;
  k.kv_heads = a->kv_heads;
  k.cache_len = a->cache_len;
  k.head_dim = a->head_dim;
  k.head_chunks = (long long)a->cache_len * (a->head_dim >> 4);
  k.pos = a->pos;
  k.parent = a->parent;
  const long long xb = (k.head_chunks + RO_THREADS - 1) / RO_THREADS;
  const dim3 grid((unsigned)(xb < RO_MAX_XBLOCKS ? xb : RO_MAX_XBLOCKS), (unsigned)(a->n_caches * a->kv_heads));
  cache_reorder_kernel<<<grid, RO_THREADS, 0, as_stream(stream)>>>(k);
  MQ_LAUNCH_CHECK("mq_decode_cache_reorder");
  return MQ_OK;
}

}  // extern "C"
