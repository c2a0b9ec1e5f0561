"""Re-ordering the slots of the batched engine's caches in place: mq_decode_cache_reorder against the torch restatement
of its rule (tests/beam_ref.py: a simultaneous assignment, evaluated on clones) -- caches filled with random bytes and compared WHOLE,
so every untouched byte counts.  Every comparison is an equality of bytes."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from beam_ref import reorder_rule  # noqa: E402

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
L = 80
POS = [0, 1, 15, 16, 63, 79, 80, 40]                               # cache_len 80: slot 6 is idle, slot 0 holds nothing
POS_B = [40, 80, 79, 63, 16, 15, 1, 5]                             # the same tables with other slots live
POS_C = [33, 33, 33, 33, 12, 12, 12, 12]                           # two groups of beams, each at one position
IDENT = list(range(8))
TABLES = {
    "identity": IDENT,
    "swap": [0, 2, 1, 3, 4, 5, 6, 7],
    "cycle_3": [0, 1, 3, 4, 2, 5, 6, 7],                           # 2 <- 3 <- 4 <- 2
    "rotation_8": [1, 2, 3, 4, 5, 6, 7, 0],
    "chain": [0, 2, 3, 3, 4, 5, 6, 7],                             # 1 <- 2 <- 3: slot 1 gets old 2, slot 2 gets old 3
    "all_from_1": [1, 1, 1, 1, 1, 1, 1, 1],                        # the source survives
    "all_from_0_and_0_from_5": [5, 0, 0, 0, 0, 0, 0, 0],           # the source is overwritten
    "two_groups": [1, 0, 1, 1, 7, 7, 4, 5],                        # slots 0..3 and 4..7 permuted (with fan-out) independently
    "out_of_range": [-1, 8, INT_MIN, INT_MAX, 5, 4, 6, 7],         # only 4 <-> 5 is live
    "idle_and_empty_sources": [6, 0, 0, 6, 4, 5, 6, 7],            # POS: slot 6 is idle and slot 0 holds nothing
    "mixed_positions": [2, 4, 5, 7, 1, 3, 6, 2],                   # sources of different positions, one taken twice
}
WRITES_NOTHING = {("identity", 0), ("identity", 1), ("identity", 2), ("idle_and_empty_sources", 0),
                  ("all_from_1", 1)}                               # POS_B: slot 1 is idle


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32).to(dev)


def _random_caches(n, B, H, L, D, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-128, 128, (B, H, L, D), generator=g, dtype=torch.int8).to(dev) for _ in range(n)]


def _run_and_compare(caches, pos, parent, L, dev, **kw):
    import mobilequant_amd as mq
    want = reorder_rule(caches, pos, parent, L)
    dpos, dpar = _i32(pos, dev), _i32(parent, dev)
    mq.ops.decode_cache_reorder(caches, dpos, dpar, **kw)
    torch.cuda.synchronize()
    assert dpos.tolist() == pos and dpar.tolist() == parent
    for i, (got, w) in enumerate(zip(caches, want)):
        assert torch.equal(got, w), (i, (got != w).nonzero()[:4].tolist())
    return want


@pytest.mark.parametrize("D", [16, 64, 128, 256])
def test_kernel_assigns_what_the_rule_says_and_nothing_else(dev, D):
    for name, parent in TABLES.items():
        for pi, pos in enumerate((POS, POS_B, POS_C)):
            caches = _random_caches(3, 8, 2, L, D, dev, seed=D)
            before = [c.clone() for c in caches]
            want = _run_and_compare(caches, pos, parent, L, dev)
            changed = any(not torch.equal(w, b) for w, b in zip(want, before))
            assert changed != ((name, pi) in WRITES_NOTHING), (name, pi)      # (the reference itself moves bytes: the comparison is not vacuous)


def test_a_swap_and_a_chain_see_the_bytes_from_before_the_call(dev):
    """Spelt out on the bytes themselves, not through the restated rule."""
    import mobilequant_amd as mq
    caches = _random_caches(2, 4, 2, L, 64, dev, seed=1)
    old = [c.clone() for c in caches]
    mq.ops.decode_cache_reorder(caches, _i32([30, 30, 20, 10], dev), _i32([1, 0, 3, 3], dev))
    torch.cuda.synchronize()
    for c, o in zip(caches, old):
        assert torch.equal(c[0, :, :30], o[1, :, :30]) and torch.equal(c[1, :, :30], o[0, :, :30])       # the swap
        assert torch.equal(c[2, :, :10], o[3, :, :10]) and torch.equal(c[2, :, 10:], o[2, :, 10:])       # 2 <- 3, its tail kept
        assert torch.equal(c[3], o[3]) and torch.equal(c[0, :, 30:], o[0, :, 30:])
    caches = _random_caches(2, 4, 2, L, 64, dev, seed=2)
    old = [c.clone() for c in caches]
    mq.ops.decode_cache_reorder(caches, _i32([5, 9, 40, 79], dev), _i32([0, 2, 3, 3], dev))              # the chain 1 <- 2 <- 3
    torch.cuda.synchronize()
    for c, o in zip(caches, old):
        assert torch.equal(c[1, :, :40], o[2, :, :40]) and torch.equal(c[2, :, :79], o[3, :, :79]) and torch.equal(c[3], o[3]) and torch.equal(c[0], o[0])
        assert torch.equal(c[1, :, 40:], o[1, :, 40:]) and torch.equal(c[2, :, 79:], o[2, :, 79:])


def test_kernel_goes_round_its_chunk_loop(dev):
    """2 MiB per head: more chunks than one round of the grid covers; a swap of two slots at different positions, one of them one
    position short of the cache's end."""
    Lb = 8192
    caches = _random_caches(2, 2, 1, Lb, 256, dev, seed=5)
    old = [c.clone() for c in caches]
    want = _run_and_compare(caches, [Lb - 1, 5000], [1, 0], Lb, dev)
    assert torch.equal(want[0][0, :, :5000], old[0][1, :, :5000]) and torch.equal(want[0][1, :, :Lb - 1], old[0][0, :, :Lb - 1])
    assert torch.equal(want[0][1, :, Lb - 1], old[0][1, :, Lb - 1]) and torch.equal(want[0][0, :, 5000:], old[0][0, :, 5000:])


def test_tables_that_fork_serves_give_forks_bytes(dev):
    import mobilequant_amd as mq
    for parent in ([0, 1, 2, 4, 4, 5, 6, 7], [5, 5, 5, 5, 5, 5, 5, 5], [0, 0, 0, 3, 5, 5, 5, 5]):
        a = _random_caches(3, 8, 2, L, 64, dev, seed=7)
        b = [c.clone() for c in a]
        mq.ops.decode_cache_fork(a, _i32(POS_B, dev), _i32(parent, dev))
        mq.ops.decode_cache_reorder(b, _i32(POS_B, dev), _i32(parent, dev))
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_registered_operator_runs_the_same_launch(dev):
    import mobilequant_amd.torch_ops  # noqa: F401
    caches = _random_caches(3, 8, 2, L, 64, dev, seed=4)
    want = reorder_rule(caches, POS_B, TABLES["rotation_8"], L)
    assert torch.ops.mobilequant_amd.decode_cache_reorder(caches, _i32(POS_B, dev), _i32(TABLES["rotation_8"], dev)) is None
    torch.cuda.synchronize()
    assert all(torch.equal(c, w) for c, w in zip(caches, want))


def test_batch_one_has_no_destination(dev):
    caches = _random_caches(2, 1, 2, 32, 64, dev, seed=6)
    for parent in ([0], [-1], [1], [INT_MAX]):
        before = [c.clone() for c in caches]
        _run_and_compare(caches, [17], parent, 32, dev)
        assert all(torch.equal(c, b) for c, b in zip(caches, before))


def test_one_captured_launch_serves_later_tables(dev):
    import mobilequant_amd as mq
    caches = _random_caches(3, 8, 2, L, 64, dev, seed=9)
    fill = [c.clone() for c in caches]
    table = mq.ops.decode_cache_table(caches)
    dpos, dpar = _i32(POS, dev), _i32(IDENT, dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                      # no warm-up launch in front: there is no launch attribute to set
        mq.ops.decode_cache_reorder(caches, dpos, dpar, table=table)
    for pos, parent in ((POS_C, TABLES["two_groups"]), (POS_B, TABLES["rotation_8"]), (POS, TABLES["out_of_range"])):
        for c, f in zip(caches, fill):
            c.copy_(f)
        dpos.copy_(_i32(pos, dev))
        dpar.copy_(_i32(parent, dev))
        g.replay()
        torch.cuda.synchronize()
        want = reorder_rule(fill, pos, parent, L)
        assert any(not torch.equal(w, f) for w, f in zip(want, fill))
        for got, w in zip(caches, want):
            assert torch.equal(got, w)


def test_op_refusals_on_device_tensors(dev):
    import mobilequant_amd as mq
    caches = _random_caches(2, 2, 1, 8, 16, dev)
    pos, par = _i32([3, 8], dev), _i32([1, 0], dev)
    for bad in (torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="decode_cache_reorder: table|no CPU path"):
            mq.ops.decode_cache_reorder(caches, pos, par, table=bad)
    odd = torch.zeros(2 * 8 * 16 + 8, dtype=torch.int8, device=dev)[8:].view(2, 1, 8, 16)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        mq.ops.decode_cache_reorder([odd], pos, par)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mq.ops.decode_cache_reorder(caches, pos.cpu(), par)
