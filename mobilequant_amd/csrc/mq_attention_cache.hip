// The bridge between the two KV cache formats of one attention block: the decode engines keep the cached keys / values
// as int8 indices in [kv_heads][cache_len][D] (values also transposed in 16-position chunks: [kv_heads][cache_len / 16][D][16]); the
// prefill attention (mq_attention.hip) continues a sequence over ITS images -- k_i8, k_rowsum, vt_i8 (keys permuted inside 64-key
// blocks), v_prefix (head_dim 128 / 256) and the fragment-blocked fp16 k_f16 (head_dim 64) -- whose layouts the header states above
// mq_attention_args.  Both hold the same indices (index - 128) on the same grids, so the bridge is data movement plus the three derived
// images, every one of them exact integer arithmetic:
//   mq_attention_cache_import   decode caches, positions 0 .. n - 1   ->  images        (one launch)
//   mq_attention_cache_export   images, rows p0 .. p0 + n - 1          ->  decode caches (one launch; no byte outside those positions)
// Both are bound by HBM traffic: every request is 16 bytes per lane, the value permutation goes through the LDS so that both sides stay
// coalesced.  No host synchronisation, caller's stream: capturable.
#include "mq_common.h"

namespace mq {

__device__ __forceinline__ unsigned cache_pack_h2(float a, float b) { return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(a, b)); }

// key r of a 64-key block sits at kappa(r) of a vT row: r = 16 j + 4 tq + e  <->  kappa = 16 tq + 4 j + e
__device__ __forceinline__ int kappa_of(int r) { return 16 * ((r >> 2) & 3) + 4 * (r >> 4) + (r & 3); }

constexpr int kTileStride = 80;       // bytes per dimension row of the LDS tile [64 dims][64 kappa]: 16-byte aligned rows, 20 dwords apart

__device__ __forceinline__ int byte_sum16(const uint4 w) {
  const unsigned u[4] = {w.x, w.y, w.z, w.w};
  int s = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) s += (int)(int8_t)(u[i] & 0xffu) + (int)(int8_t)((u[i] >> 8) & 0xffu) + (int)(int8_t)((u[i] >> 16) & 0xffu) + (int)(int8_t)(u[i] >> 24);
  return s;
}

// ---- import ---------------------------------------------------------------------------------------------------------------------
// One launch, two kinds of workgroups (256 threads).  nblk = n / 64.
//   [0, KV * nblk): key workgroup (head, block b).  Thread (r = tid >> 2, c = tid & 3) owns row 64 b + r, the 16 columns 64 dc + 16 c of
//     every 64-column slab dc -- the prep kernel's mapping: one 16-byte load, one 16-byte store to k_i8, its share of the row sum, and at
//     head_dim 64 the two 16-byte halves of its fp16 fragment piece.
//   the rest: value workgroup (head, slab dc, run of blocks).  Per block the 64 keys x 64 dimensions are read with one 16-byte load per
//     thread in the cache's own order, scattered into an LDS tile [dim][kappa] and read back as the 16 bytes kappa = 16 c .. of dimension
//     d = tid >> 2: one 16-byte store to vt_i8.  With v_prefix the run is the whole sequence, walked in order with the running column
//     sums in registers (no second launch); without it every block is a workgroup of its own.  The next block's load is in flight
//     while this one goes through the LDS (two tiles: one barrier per block).
template <int D>
__global__ void __launch_bounds__(256) attention_cache_import_kernel(const mq_attention_cache_args a) {
  const int nblk = a.n >> 6, CSB = a.cache_seq >> 6;
  const int tid = threadIdx.x, r = tid >> 2, c = tid & 3;
  const int nk = a.kv_heads * nblk;
  __shared__ __attribute__((aligned(16))) int8_t tile[2][64 * kTileStride];
  if ((int)blockIdx.x < nk) {
    const int h = blockIdx.x / nblk, b = blockIdx.x % nblk;
    const int t = 64 * b + r;
    const int8_t* src = a.k + (size_t)h * a.k_head_stride + (size_t)t * D + 16 * c;
    int8_t* dst = a.k_i8 + ((size_t)h * a.cache_seq + t) * D + 16 * c;
    int sum = 0;
    uint4 w[D / 64];
#pragma unroll
    for (int dc = 0; dc < D / 64; ++dc) w[dc] = *reinterpret_cast<const uint4*>(src + 64 * dc);
#pragma unroll
    for (int dc = 0; dc < D / 64; ++dc) {
      *reinterpret_cast<uint4*>(dst + 64 * dc) = w[dc];
      sum += byte_sum16(w[dc]);
    }
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    const int zq = (int)a.qk_a.offset[0] - 128;          // read at launch: the grids are learnable
    if (c == 0) a.k_rowsum[(size_t)h * a.cache_seq + t] = -zq * sum;
    if constexpr (D == 64) {
      if (a.k_f16 != nullptr) {
        // fp16 of the centred index, the prep kernel's arithmetic (index - offset in fp32, exact for an offset in [-256, 511]; outside
        // that range the image is poisoned with NaN as the prep kernel poisons it: the caller keeps such a cache off the f16 contraction)
        const float zk = a.qk_b.offset[0];
        const unsigned u[4] = {w[0].x, w[0].y, w[0].z, w[0].w};
        unsigned hw[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float i0 = (float)((int)(int8_t)((u[i >> 1] >> (16 * (i & 1))) & 0xffu) + 128);
          const float i1 = (float)((int)(int8_t)((u[i >> 1] >> (16 * (i & 1) + 8)) & 0xffu) + 128);
          hw[i] = cache_pack_h2(__fsub_rn(i0, zk), __fsub_rn(i1, zk));
        }
        if (!(zk >= -256.f && zk <= 511.f)) {
#pragma unroll
          for (int i = 0; i < 8; ++i) hw[i] = 0x7e007e00u;
        }
        uint16_t* hdst = a.k_f16 + (((size_t)h * CSB + b) * 8 + 2 * (r >> 4)) * 512 + ((r & 15) + 16 * c) * 8;
        reinterpret_cast<uint4*>(hdst)[0] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
        reinterpret_cast<uint4*>(hdst + 512)[0] = make_uint4(hw[4], hw[5], hw[6], hw[7]);
      }
    }
    return;
  }
  // value workgroups
  const bool scan = a.v_prefix != nullptr;
  const int runs = scan ? 1 : nblk;                       // block runs per (head, slab)
  int wg = blockIdx.x - nk;
  const int run = wg % runs;
  wg /= runs;
  const int dc = wg % (D / 64), h = wg / (D / 64);
  const int b0 = scan ? 0 : run, b1 = scan ? nblk : run + 1;
  const int8_t* vh = a.v + (size_t)h * a.v_head_stride;
  // load side: plain layout -- thread (r, c): key 64 b + r, dimensions 64 dc + 16 c ..; chunked layout -- thread (j = tid >> 6, d = tid & 63):
  // the 16 positions of chunk 4 b + j for dimension 64 dc + d (a wave reads one contiguous KiB)
  const int lj = tid >> 6, ld = tid & 63;
  auto load = [&](int b) -> uint4 {
    if (a.v_chunked) return *reinterpret_cast<const uint4*>(vh + (((size_t)(4 * b + lj)) * D + 64 * dc + ld) * 16);
    return *reinterpret_cast<const uint4*>(vh + (size_t)(64 * b + r) * D + 64 * dc + 16 * c);
  };
  const int d = tid >> 2;                                 // store side: dimension 64 dc + d, kappa 16 c ..
  const int kap = kappa_of(r);
  int prefix = 0;
  uint4 next = load(b0);
  for (int b = b0; b < b1; ++b) {
    const uint4 cur = next;
    if (b + 1 < b1) next = load(b + 1);
    int8_t* tl = tile[b & 1];
    const unsigned u[4] = {cur.x, cur.y, cur.z, cur.w};
    if (a.v_chunked) {
      // dword tq of the chunk row (positions 4 tq .. + 3 of chunk j) is dword 4 tq + j of the vT row
#pragma unroll
      for (int tq = 0; tq < 4; ++tq) *reinterpret_cast<unsigned*>(tl + ld * kTileStride + 4 * (4 * tq + lj)) = u[tq];
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) tl[(16 * c + i) * kTileStride + kap] = (int8_t)(u[i >> 2] >> (8 * (i & 3)));
    }
    __syncthreads();
    const uint4 o = *reinterpret_cast<const uint4*>(tl + d * kTileStride + 16 * c);
    *reinterpret_cast<uint4*>(a.vt_i8 + (((size_t)h * CSB + b) * D + 64 * dc + d) * 64 + 16 * c) = o;
    if (scan) {
      int cs = byte_sum16(o);
      cs += __shfl_xor(cs, 1, 64);
      cs += __shfl_xor(cs, 2, 64);
      prefix += cs;
      if (c == 0) a.v_prefix[((size_t)h * CSB + b) * D + 64 * dc + d] = prefix;
    }
  }
}

// ---- export ---------------------------------------------------------------------------------------------------------------------
// grid (touched 64-row blocks, kv_heads, 1 + D / 64): z = 0 copies the block's key rows inside [p0, p0 + n), z - 1 = dc un-permutes one
// 64-dimension slab of the block's values through the LDS tile.  A 16-position chunk of the chunked layout that the range covers only
// partly is written byte by byte, so the other positions' bytes keep their values.
template <int D>
__global__ void __launch_bounds__(256) attention_cache_export_kernel(const mq_attention_cache_args a) {
  const int CSB = a.cache_seq >> 6;
  const int tid = threadIdx.x, r = tid >> 2, c = tid & 3;
  const int b = (a.p0 >> 6) + blockIdx.x, h = blockIdx.y;
  const int lo = a.p0, hi = a.p0 + a.n;
  __shared__ __attribute__((aligned(16))) int8_t tile[64 * kTileStride];
  if (blockIdx.z == 0) {
    const int t = 64 * b + r;
    if (t < lo || t >= hi) return;
    const int8_t* src = a.k_i8 + ((size_t)h * a.cache_seq + t) * D + 16 * c;
    int8_t* dst = a.k + (size_t)h * a.k_head_stride + (size_t)t * D + 16 * c;
#pragma unroll
    for (int dc = 0; dc < D / 64; ++dc) *reinterpret_cast<uint4*>(dst + 64 * dc) = *reinterpret_cast<const uint4*>(src + 64 * dc);
    return;
  }
  const int dc = blockIdx.z - 1;
  const int d = tid >> 2;
  *reinterpret_cast<uint4*>(tile + d * kTileStride + 16 * c) =
      *reinterpret_cast<const uint4*>(a.vt_i8 + (((size_t)h * CSB + b) * D + 64 * dc + d) * 64 + 16 * c);
  __syncthreads();
  int8_t* vh = a.v + (size_t)h * a.v_head_stride;
  if (a.v_chunked) {
    const int j = tid >> 6, dd = tid & 63;
    const int t0 = 64 * b + 16 * j;                       // the chunk's first position
    if (t0 + 16 <= lo || t0 >= hi) return;
    const int8_t* row = tile + dd * kTileStride + 4 * j;
    const unsigned u0 = *reinterpret_cast<const unsigned*>(row), u1 = *reinterpret_cast<const unsigned*>(row + 16);
    const unsigned u2 = *reinterpret_cast<const unsigned*>(row + 32), u3 = *reinterpret_cast<const unsigned*>(row + 48);
    int8_t* dst = vh + (((size_t)(4 * b + j)) * D + 64 * dc + dd) * 16;
    if (t0 >= lo && t0 + 16 <= hi) {
      *reinterpret_cast<uint4*>(dst) = make_uint4(u0, u1, u2, u3);
    } else {
      auto put4 = [&](int p, unsigned u) {                // positions t0 + p .. + 3: only those inside [lo, hi)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (t0 + p + e >= lo && t0 + p + e < hi) dst[p + e] = (int8_t)(u >> (8 * e));
      };
      put4(0, u0); put4(4, u1); put4(8, u2); put4(12, u3);
    }
  } else {
    const int t = 64 * b + r;
    if (t < lo || t >= hi) return;
    const int kap = kappa_of(r);
    auto get4 = [&](int i) {                              // dimensions 16 c + i .. + 3 of this key
      unsigned u = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) u |= ((unsigned)(uint8_t)tile[(16 * c + i + e) * kTileStride + kap]) << (8 * e);
      return u;
    };
    *reinterpret_cast<uint4*>(vh + (size_t)t * D + 64 * dc + 16 * c) = make_uint4(get4(0), get4(4), get4(8), get4(12));
  }
}

static int check_cache_args(const mq_attention_cache_args& a, const char* fn, bool import) {
  MQ_REQUIRE(a.head_dim == 64 || a.head_dim == 128 || a.head_dim == 256, "%s: head_dim 64, 128 or 256 (got %d)", fn, a.head_dim);
  MQ_REQUIRE(a.kv_heads > 0 && a.kv_heads <= 65535, "%s: kv_heads = %d outside 1 .. 65535", fn, a.kv_heads);
  MQ_REQUIRE(a.cache_seq > 0 && a.cache_seq % 64 == 0 && a.cache_seq <= 65536, "%s: cache_seq = %d (the images' rows: a multiple of 64, <= 65536)", fn,
             a.cache_seq);
  MQ_REQUIRE(a.cache_len > 0 && (!a.v_chunked || a.cache_len % 16 == 0), "%s: cache_len = %d (positive; a multiple of 16 with v_chunked)", fn, a.cache_len);
  MQ_REQUIRE(a.v_chunked == 0 || a.v_chunked == 1, "%s: v_chunked = %d (0: [kv][cache_len][D], 1: [kv][cache_len / 16][D][16])", fn, a.v_chunked);
  if (import)
    MQ_REQUIRE(a.p0 == 0 && a.n > 0 && a.n % 64 == 0, "%s: positions 0 .. n - 1 with n %% 64 == 0 (got p0=%d n=%d)", fn, a.p0, a.n);
  else
    MQ_REQUIRE(a.p0 >= 0 && a.n > 0, "%s: rows p0 .. p0 + n - 1 with p0 >= 0, n > 0 (got p0=%d n=%d)", fn, a.p0, a.n);
  MQ_REQUIRE((int64_t)a.p0 + a.n <= a.cache_seq && (int64_t)a.p0 + a.n <= a.cache_len,
             "%s: p0 + n = %lld exceeds the images (cache_seq=%d) or the decode caches (cache_len=%d)", fn, (long long)a.p0 + a.n, a.cache_seq, a.cache_len);
  MQ_REQUIRE(a.k != nullptr && a.v != nullptr && a.k_i8 != nullptr && a.vt_i8 != nullptr && (!import || a.k_rowsum != nullptr), "%s: null pointer", fn);
  const int64_t head_bytes = (int64_t)a.cache_len * a.head_dim;
  MQ_REQUIRE(a.k_head_stride >= head_bytes && a.v_head_stride >= head_bytes && a.k_head_stride % 16 == 0 && a.v_head_stride % 16 == 0,
             "%s: head strides must be multiples of 16 bytes and at least cache_len * head_dim = %lld (got k %lld, v %lld)", fn, (long long)head_bytes,
             (long long)a.k_head_stride, (long long)a.v_head_stride);
  MQ_REQUIRE(aligned(a.k, 16) && aligned(a.v, 16) && aligned(a.k_i8, 16) && aligned(a.vt_i8, 16), "%s: pointers must be 16-byte aligned", fn);
  if (import) {
    MQ_REQUIRE(aligned(a.k_rowsum, 4) && a.qk_a.offset != nullptr, "%s: qk_a's offset (the zero point of k_rowsum) is read by pointer: it must be set", fn);
    MQ_REQUIRE(a.head_dim == 64 ? a.v_prefix == nullptr : (a.v_prefix != nullptr && aligned(a.v_prefix, 16)),
               "%s: v_prefix ([kv_heads][cache_seq / 64][head_dim] int32, 16-byte aligned) is required at head_dim 128 / 256 and absent at 64", fn);
    MQ_REQUIRE(a.k_f16 == nullptr || (a.head_dim == 64 && aligned(a.k_f16, 16) && a.qk_b.offset != nullptr),
               "%s: k_f16 is a head_dim 64 image, 16-byte aligned, and needs qk_b's offset", fn);
  }
  return MQ_OK;
}

}  // namespace mq

using namespace mq;

extern "C" int mq_attention_cache_import(const mq_attention_cache_args* args, mq_stream_t stream) {
  MQ_REQUIRE(args != nullptr, "mq_attention_cache_import: null argument block");
  const mq_attention_cache_args a = *args;
  if (int rc = check_cache_args(a, "mq_attention_cache_import", true)) return rc;
  const int nblk = a.n / 64, slabs = a.head_dim / 64;
  const unsigned grid = (unsigned)(a.kv_heads * nblk + a.kv_heads * slabs * (a.v_prefix != nullptr ? 1 : nblk));
  hipStream_t st = as_stream(stream);
  if (a.head_dim == 64) attention_cache_import_kernel<64><<<grid, 256, 0, st>>>(a);
  else if (a.head_dim == 128) attention_cache_import_kernel<128><<<grid, 256, 0, st>>>(a);
  else attention_cache_import_kernel<256><<<grid, 256, 0, st>>>(a);
  MQ_LAUNCH_CHECK("mq_attention_cache_import");
  return MQ_OK;
}

extern "C" int mq_attention_cache_export(const mq_attention_cache_args* args, mq_stream_t stream) {
  MQ_REQUIRE(args != nullptr, "mq_attention_cache_export: null argument block");
  const mq_attention_cache_args a = *args;
  if (int rc = check_cache_args(a, "mq_attention_cache_export", false)) return rc;
  const dim3 grid((unsigned)((a.p0 + a.n - 1) / 64 - a.p0 / 64 + 1), (unsigned)a.kv_heads, (unsigned)(1 + a.head_dim / 64));
  hipStream_t st = as_stream(stream);
  if (a.head_dim == 64) attention_cache_export_kernel<64><<<grid, 256, 0, st>>>(a);
  else if (a.head_dim == 128) attention_cache_export_kernel<128><<<grid, 256, 0, st>>>(a);
  else attention_cache_export_kernel<256><<<grid, 256, 0, st>>>(a);
  MQ_LAUNCH_CHECK("mq_attention_cache_export");
  return MQ_OK;
}
