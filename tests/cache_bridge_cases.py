"""The case table of the cache bridge tests (test_cache_bridge_host.py checks that it is legal and covers what it claims,
test_gpu_cache_bridge.py runs it).  Shapes are small: the largest buffer is about 1 MiB."""
import dataclasses
import functools

import numpy as np

PAD_ROWS = 48          # padded plain layout: [KV, cache_len + 48, D], passed as [:, :cache_len]
PAD_CHUNKS = 3         # padded chunked layout: [KV, cache_len / 16 + 3, D, 16], passed as [:, :cache_len / 16]


@dataclasses.dataclass(frozen=True)
class Geometry:
    D: int
    KV: int
    cache_len: int
    rows: int          # the images' rows (cache_seq)

    @property
    def id(self):
        return f"D{self.D}-kv{self.KV}-len{self.cache_len}-rows{self.rows}"


GEOMETRIES = (Geometry(64, 1, 64, 64),            # the smallest legal case
              Geometry(64, 3, 208, 256), Geometry(128, 2, 208, 256), Geometry(256, 1, 208, 256), Geometry(256, 3, 208, 256),
              Geometry(128, 1, 2176, 2176), Geometry(256, 2, 2176, 2176))    # 34 blocks: the long v_prefix walk, the double buffer


@dataclasses.dataclass(frozen=True)
class Config:
    """A geometry with a value layout and a head stride."""
    geo: Geometry
    chunked: bool
    padded: bool

    @property
    def id(self):
        return f"{self.geo.id}-{'chunked' if self.chunked else 'plain'}-{'padded' if self.padded else 'dense'}"

    def k_alloc(self):
        g = self.geo
        return (g.KV, g.cache_len + (PAD_ROWS if self.padded else 0), g.D)

    def v_alloc(self):
        g = self.geo
        if self.chunked:
            return (g.KV, g.cache_len // 16 + (PAD_CHUNKS if self.padded else 0), g.D, 16)
        return self.k_alloc()

    def head_strides(self):
        """(k, v) head strides in bytes."""
        ka, va = self.k_alloc(), self.v_alloc()
        return int(np.prod(ka[1:])), int(np.prod(va[1:]))


CONFIGS = tuple(Config(g, chunked, padded) for g in GEOMETRIES for chunked in (False, True) for padded in (False, True))

IMPORT_N = (64, 192, 2112)          # one block, fewer blocks than the cache holds, 33 blocks
FILLS = ("random", "min", "max", "one_hot")
ZQ = (0.0, 128.0, 255.0, -382.0)    # qk_a's offset; -382: the out-of-window grid of test_gpu_prefill_attention.py
ZK_EXACT = (-256.0, 0.0, 128.0, 511.0)
ZK_POISONED = (-257.0, 512.0, 1e4)


def import_ns(geo):
    return tuple(n for n in IMPORT_N if n <= geo.cache_len and n <= geo.rows)


def import_cases(geo):
    """(n, fill, zq, zk) of one geometry.  At the largest n every fill meets every zq; at the smaller ones fill and zq go in pairs.  At
    head_dim 64 every fill also meets every zk (at the other head dims zk is not read)."""
    ns = import_ns(geo)
    out = [(ns[-1], f, zq, 0.0) for f in FILLS for zq in ZQ]
    out += [(n, f, zq, 128.0) for n in ns[:-1] for f, zq in zip(FILLS, ZQ)]
    if geo.D == 64:
        out += [(ns[-1], f, 128.0, zk) for f in FILLS for zk in ZK_EXACT + ZK_POISONED if zk != 0.0]
    return out


# ---- export ranges (p0, n) and the chunk / block situations each is listed for -------------------------------------------------
EXPORT_RANGES = {
    208: {(0, 1): {"first_position", "high_end_in_chunk", "inside_one_chunk"},
          (0, 208): {"whole_cache", "three_blocks", "last_chunk", "last_position_unaligned_len"},
          (15, 1): {"low_end_in_chunk", "inside_one_chunk"},
          (15, 2): {"low_end_in_chunk", "high_end_in_chunk", "both_ends_in_chunks"},
          (16, 16): {"chunk_exactly"},
          (17, 30): {"low_end_in_chunk", "high_end_in_chunk", "both_ends_in_chunks"},
          (37, 1): {"strictly_inside_one_chunk", "inside_one_chunk"},
          (63, 2): {"block_boundary", "low_end_in_chunk", "high_end_in_chunk"},
          (60, 100): {"three_blocks", "block_boundary", "low_end_in_chunk"},
          (192, 16): {"last_chunk", "chunk_exactly"},
          (207, 1): {"last_position_unaligned_len", "last_chunk", "low_end_in_chunk"}},
    2176: {(1000, 1111): {"three_blocks", "both_ends_in_chunks", "whole_chunk_between_cut_ends"},
           (2175, 1): {"last_position", "last_chunk", "low_end_in_chunk"}},
    64: {(0, 64): {"whole_cache"}, (17, 30): {"both_ends_in_chunks"}, (63, 1): {"last_position", "low_end_in_chunk"}},
}

# what the ranges of the cache_len = 208 geometries must cover between them
REQUIRED_SITUATIONS = {"low_end_in_chunk", "high_end_in_chunk", "both_ends_in_chunks", "inside_one_chunk", "strictly_inside_one_chunk",
                       "chunk_exactly", "block_boundary", "three_blocks", "last_chunk", "last_position_unaligned_len", "first_position",
                       "whole_cache"}


def situations(p0, n, cache_len):
    """The chunk (16 positions) and block (64 positions) situations the range [p0, p0 + n) of a cache of cache_len positions hits,
    computed from the range alone."""
    lo, hi = p0, p0 + n
    out = set()
    cut_low = cut_high = whole = False
    for t0 in range(lo // 16 * 16, hi, 16):
        below, above = t0 < lo, hi < t0 + 16
        if below and above:
            out.add("strictly_inside_one_chunk")
        cut_low |= below
        cut_high |= above
        whole |= not below and not above
    if cut_low:
        out.add("low_end_in_chunk")
    if cut_high:
        out.add("high_end_in_chunk")
    if cut_low and cut_high and lo // 16 != (hi - 1) // 16:
        out.add("both_ends_in_chunks")
        if whole:
            out.add("whole_chunk_between_cut_ends")
    if lo // 16 == (hi - 1) // 16 and n < 16:
        out.add("inside_one_chunk")
    if lo % 16 == 0 and n == 16:
        out.add("chunk_exactly")
    if lo // 64 != (hi - 1) // 64:
        out.add("block_boundary")
    if (hi - 1) // 64 - lo // 64 >= 2:
        out.add("three_blocks")
    if (hi - 1) // 16 == (cache_len - 1) // 16:
        out.add("last_chunk")
    if hi == cache_len:
        out.add("last_position_unaligned_len" if cache_len % 64 else "last_position")
    if lo == 0:
        out.add("first_position")
    if lo == 0 and hi == cache_len:
        out.add("whole_cache")
    return out


def export_ranges(geo):
    return tuple(EXPORT_RANGES[geo.cache_len])


# ---- data ----------------------------------------------------------------------------------------------------------------------
def _seed(*parts):
    s = 0
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def random_bytes(shape, *seed):
    return np.random.default_rng(_seed(*seed)).integers(-128, 128, size=shape, dtype=np.int8)


@functools.lru_cache(maxsize=None)
def logical_kv(geo, fill):
    """(k, v) [KV, cache_len, D] int8 of one fill, read-only (shared by every test that uses the pair)."""
    shape = (geo.KV, geo.cache_len, geo.D)
    if fill == "random":
        k, v = random_bytes(shape, geo.id, "k"), random_bytes(shape, geo.id, "v")
    elif fill in ("min", "max"):
        k = np.full(shape, -128 if fill == "min" else 127, np.int8)
        v = k.copy()
    elif fill == "one_hot":
        # one 127 per head at a seeded (t, d) inside the first 64 positions (every import n holds it), in zeros
        rng = np.random.default_rng(_seed(geo.id, "one_hot"))
        k, v = np.zeros(shape, np.int8), np.zeros(shape, np.int8)
        for a in (k, v):
            for h in range(geo.KV):
                a[h, rng.integers(0, 64), rng.integers(0, geo.D)] = 127
    else:
        raise ValueError(fill)
    k.setflags(write=False)
    v.setflags(write=False)
    return k, v


IMAGE_NAMES = ("k_i8", "vt_i8", "k_rs", "v_pre", "k_f16")


def _frozen(images):
    for name in IMAGE_NAMES:
        if images[name] is not None:
            images[name].setflags(write=False)
    return images


@functools.lru_cache(maxsize=None)
def reference_images(geo, fill, n, zq, zk):
    """cache_bridge_ref.import_images of one import case over zeros, laid out for the geometry's image rows: computed once, read-only."""
    import cache_bridge_ref as R
    k, v = logical_kv(geo, fill)
    return _frozen(R.import_images(k, v, n, zq, zk, geo.D, geo.D == 64, rows=geo.rows))


@functools.lru_cache(maxsize=None)
def written_by_import(geo, n):
    """Boolean masks over the flat images: the elements an import of n positions writes (those the reference takes from the caches and
    not from the state before)."""
    import cache_bridge_ref as R
    zeros = np.zeros((geo.KV, n, geo.D), np.int8)
    sizes = R.import_images(zeros, zeros, n, 0.0, 0.0, geo.D, geo.D == 64, rows=geo.rows)
    ones = {name: np.ones_like(sizes[name]) for name in IMAGE_NAMES if sizes[name] is not None}
    got = R.import_images(zeros, zeros, n, 0.0, 0.0, geo.D, geo.D == 64, rows=geo.rows, before=ones)
    return {name: got[name] != 1 for name in ones}


def expected_images(geo, fill, n, zq, zk, before):
    """The whole images after the import: the reference where the import writes, `before` (flat arrays) elsewhere."""
    ref, mask = reference_images(geo, fill, n, zq, zk), written_by_import(geo, n)
    return {name: np.where(mask[name], ref[name], before[name].astype(ref[name].dtype)) for name in mask}
