// Fork cached sequences into other slots of the batched decode engine's int8 KV caches (mq_decode_cache_fork): n samples of one
// prompt from ONE prefill.  One launch copies the live part of every source slot, in every cache (all layers, keys and values), into
// any number of destination slots; a source byte is loaded once, however many destinations take it.
//
// THE RULE (normative).  caches[c], c < n_caches, is [batch][kv_heads][cache_len][head_dim] int8, contiguous, 16-byte
// aligned; pos [batch] is the engines' position vector (cache_len = idle) and parent [batch] the fork table, both DEVICE data.
//   - Slot s is a SOURCE iff parent[s] == s.
//   - Slot d is a LIVE DESTINATION iff, with p = parent[d]:  0 <= p < batch and p != d;  parent[p] == p (a source is never itself
//     overwritten: no in-place hazard exists, whatever order the workgroups run in);  0 <= pos[p] < cache_len.
//   - For a live destination, for every cache c and head h, bytes [0, pos[p] * head_dim) of caches[c][d][h] become those of
//     caches[c][p][h].
//   - Nothing else is written: no byte at or past pos[p] of a destination, no byte of a slot that is not a live destination, and pos
//     itself never.
//   - Every entry of parent is range-checked before any address is formed from it.  No-ops for the affected slot: an entry -1, batch,
//     INT_MIN or INT_MAX; a chain (parent[d] = p, parent[p] = q != p); an idle source; pos[p] == 0.
//   - Both tables are read on the device: one captured launch serves any later table.  No host synchronisation.
//
// THE KERNEL.  Grid (blocks of 16-byte chunks of a head's live bytes) x (cache, head) x (slot), 256 threads.  The workgroups of slot s
// read parent[s], pos[s] and parent[0 .. batch) with uniform loads and leave -- before any cache is touched -- unless s is a source at
// 0 < pos[s] < cache_len with at least one destination; the destinations are a bit mask (no indexed array, no private segment).  The
// only table entry an address is formed from is d itself, d < batch, where parent[d] == s.  A thread then holds FK_UNROLL independent
// 16-byte loads in flight and stores each chunk to every destination with plain 16-byte vector stores (they keep the lines in the L2:
// the next step's attention reads them).  head_dim % 16 == 0 makes every head's live span a whole number of chunks at a 16-byte
// aligned address.  The grid's first dimension is sized from cache_len (the positions are device data) and capped at FK_MAX_XBLOCKS:
// past FK_MAX_XBLOCKS * FK_BLOCK_CHUNKS chunks per head a workgroup goes round its chunk loop.  No LDS, no launch attribute:
// capturable without a warm-up.
#include "mq_common.h"

namespace mq {
namespace {

constexpr int FK_THREADS = 256;
constexpr int FK_UNROLL = 4;                                  // independent 16-byte loads in flight per lane
constexpr int FK_BLOCK_CHUNKS = FK_THREADS * FK_UNROLL;       // 16 KiB of a head per workgroup and round
constexpr int FK_MAX_XBLOCKS = 16;                            // 256 KiB of a head per round of the grid
constexpr int FK_MAX_CACHES = 1024;
constexpr long long FK_MAX_GRID_Y = 65535;

// 16 bytes: one global_load / global_store_dwordx4 per lane.  A native vector, and every load unconditional: hipcc moved an array of
// HIP's uint4 struct behind `if (i < live)` into 16 KiB of LDS (ds_write_b128 behind each load, a vmcnt wait per load); this form keeps
// FK_UNROLL loads in flight in 24 VGPRs with no LDS and no private segment (checked in the ISA).
typedef unsigned fk_chunk __attribute__((ext_vector_type(4)));

struct ForkArgs {
  int8_t* const* caches;
  int batch, kv_heads, cache_len, head_dim;
  long long head_chunks;                                      // cache_len * head_dim / 16: a head's allocation in 16-byte chunks
  const int* pos;
  const int* parent;
};

__global__ __launch_bounds__(FK_THREADS) void cache_fork_kernel(ForkArgs a) {
  const int s = (int)blockIdx.z;                              // < batch by the grid
  if (a.parent[s] != s) return;                               // not a source (workgroup-uniform, like every test below)
  const int p = a.pos[s];
  if (p <= 0 || p >= a.cache_len) return;                     // idle, or nothing cached
  const long long live = (long long)p * (a.head_dim >> 4);    // the head's live 16-byte chunks
  const long long i_first = (long long)blockIdx.x * FK_BLOCK_CHUNKS;
  if (i_first >= live) return;
  unsigned mask = 0;                                          // bit d: slot d takes this source
#pragma unroll
  for (int d = 0; d < MQ_DECODE_MAX_BATCH; ++d)
    if (d < a.batch && d != s && a.parent[d] == s) mask |= 1u << d;
  if (mask == 0) return;

  const int c = (int)blockIdx.y / a.kv_heads, h = (int)blockIdx.y % a.kv_heads;
  fk_chunk* const base = reinterpret_cast<fk_chunk*>(a.caches[c]) + (long long)h * a.head_chunks;
  const long long slot_chunks = (long long)a.kv_heads * a.head_chunks;
  const fk_chunk* const src = base + (long long)s * slot_chunks;
  const long long round = (long long)gridDim.x * FK_BLOCK_CHUNKS;
  for (long long i0 = i_first + threadIdx.x; i0 < live; i0 += round) {
    fk_chunk v[FK_UNROLL];
#pragma unroll
    for (int u = 0; u < FK_UNROLL; ++u) {
      const long long i = i0 + (long long)u * FK_THREADS;
      v[u] = src[i < live ? i : i0];                          // unconditional (chunk i0 is live): the loads stay in registers and in flight together
    }
    for (unsigned m = mask; m != 0; m &= m - 1) {              // uniform: every destination in turn
      fk_chunk* const dst = base + (long long)(__builtin_ctz(m)) * slot_chunks;
#pragma unroll
      for (int u = 0; u < FK_UNROLL; ++u) {
        const long long i = i0 + (long long)u * FK_THREADS;
        if (i < live) dst[i] = v[u];
      }
    }
  }
}

}  // namespace
}  // namespace mq

using namespace mq;

extern "C" {

int mq_decode_cache_fork(const mq_decode_cache_fork_args* a, mq_stream_t stream) {
  MQ_REQUIRE(a != nullptr, "mq_decode_cache_fork: null argument block");
  MQ_REQUIRE(a->caches && a->pos && a->parent, "mq_decode_cache_fork: null pointer (caches, pos and parent are required)");
  MQ_REQUIRE(a->n_caches >= 1 && a->n_caches <= FK_MAX_CACHES, "mq_decode_cache_fork: n_caches=%d outside 1..%d", a->n_caches, FK_MAX_CACHES);
  MQ_REQUIRE(a->batch >= 1 && a->batch <= MQ_DECODE_MAX_BATCH, "mq_decode_cache_fork: batch=%d outside 1..%d", a->batch, MQ_DECODE_MAX_BATCH);
  MQ_REQUIRE(a->kv_heads >= 1, "mq_decode_cache_fork: kv_heads=%d must be >= 1", a->kv_heads);
  MQ_REQUIRE(a->cache_len >= 1, "mq_decode_cache_fork: cache_len=%d must be >= 1", a->cache_len);
  MQ_REQUIRE(a->head_dim >= 16 && a->head_dim <= 256 && a->head_dim % 16 == 0,
             "mq_decode_cache_fork: head_dim=%d must be a multiple of 16 in [16, 256]", a->head_dim);
  MQ_REQUIRE((long long)a->n_caches * a->kv_heads <= FK_MAX_GRID_Y, "mq_decode_cache_fork: n_caches x kv_heads = %lld above %lld (one grid row each)",
             (long long)a->n_caches * a->kv_heads, FK_MAX_GRID_Y);
  MQ_REQUIRE(aligned(a->caches, 8) && aligned(a->pos, 4) && aligned(a->parent, 4),
             "mq_decode_cache_fork: the pointer table must be 8-byte, pos and parent 4-byte aligned");
  ForkArgs k;
  k.caches = a->caches;
  k.batch = a->batch;
  k.kv_heads = a->kv_heads;
  k.cache_len = a->cache_len;
  k.head_dim = a->head_dim;
  k.head_chunks = (long long)a->cache_len * (a->head_dim >> 4);
  k.pos = a->pos;
  k.parent = a->parent;
  const long long xb = (k.head_chunks + FK_BLOCK_CHUNKS - 1) / FK_BLOCK_CHUNKS;
  const dim3 grid((unsigned)(xb < FK_MAX_XBLOCKS ? xb : FK_MAX_XBLOCKS), (unsigned)(a->n_caches * a->kv_heads), (unsigned)a->batch);
  cache_fork_kernel<<<grid, FK_THREADS, 0, as_stream(stream)>>>(k);
  MQ_LAUNCH_CHECK("mq_decode_cache_fork");
  return MQ_OK;
}

}  // extern "C"
