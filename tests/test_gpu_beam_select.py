"""mq_beam_select (csrc/mq_beam.hip) against the numpy restatement of its rule (tests/beam_ref.py): candidates (row,
token, score bits, log-probability bits) and padding exactly, the log-probability bits against mq_logprob_top's, row_lse within the
log-probability kernel's bound of float64, and the invariances the rule promises.  m and logf(S) of a row are read from
mq_logprob_top's own output (pinned by tests/test_gpu_logprob.py); everything behind them is single fp32 operations."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_ref  # noqa: E402
import logprob_ref  # noqa: E402

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
SPLITS = {"1x8": [0] * 8, "2x4": [0, 0, 0, 0, 1, 1, 1, 1], "4x2": [0, 0, 1, 1, 2, 2, 3, 3], "8x1": list(range(8))}
KS = [1, 2, 16, 20]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _rows(V, seed, rows=8):
    rng = np.random.default_rng(seed)
    l = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    cum = (-rng.random(rows) * 20).astype(np.float32)
    return l, cum


def _lists(dl, K, n_groups, group):
    """Every member row's (ids, lp) by the numpy rule, with m and logf(S) from mq_logprob_top; also that kernel's own top lists."""
    from mobilequant_amd import sampling
    rows = dl.shape[0]
    _, _, top_id, top_lp = sampling.logprob_top(dl, torch.zeros(rows, dtype=torch.int64, device=dl.device), n_top=K)
    top_id, top_lp, l = top_id.cpu().numpy(), top_lp.cpu().numpy(), dl.cpu().numpy()
    lists = []
    for r in range(rows):
        if not beam_ref.member(group[r], n_groups):
            lists.append(None)
            continue
        m = logprob_ref.normalise(l[r])[top_id[r, 0]]
        lists.append(beam_ref.row_list(l[r], m, -top_lp[r, 0], K))
    return lists, top_id, top_lp


def _select(dl, cum, group, n_groups, K, **kw):
    import mobilequant_amd as mq
    dev = dl.device
    dc, dg = torch.tensor(cum, dtype=torch.float32).to(dev), torch.tensor(group, dtype=torch.int32).to(dev)
    keep = (dl.clone(), dc.clone(), dg.clone())
    out = mq.ops.beam_select(dl, dc, dg, n_groups, K, **kw)
    torch.cuda.synchronize()
    for a, b in zip(keep, (dl, dc, dg)):                           # the inputs are unchanged
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    return [t.cpu().numpy() for t in out]


def _check(dl, cum, group, n_groups, K):
    """One launch against the rule.  Returns the outputs."""
    V = dl.shape[1]
    sc, row, tok, lp, lse = _select(dl, cum, group, n_groups, K)
    lists, top_id, top_lp = _lists(dl, K, n_groups, group)
    wsc, wrow, wtok, wlp = beam_ref.select(lists, cum, group, n_groups, K)
    assert np.array_equal(row, wrow) and np.array_equal(tok, wtok), (row, wrow, tok, wtok)
    assert np.array_equal(_bits(sc), _bits(wsc)) and np.array_equal(_bits(lp), _bits(wlp))
    l = dl.cpu().numpy()
    for g in range(n_groups):
        for j in range(K):
            r, t = row[g, j], tok[g, j]
            if r < 0:
                assert t == -1 and sc[g, j] == -np.inf and lp[g, j] == -np.inf
                continue
            k = int(np.nonzero(top_id[r] == t)[0][0])              # the bits mq_logprob_top writes for that token
            assert _bits(lp[g, j]) == _bits(top_lp[r, k])
    for r in range(dl.shape[0]):
        if lists[r] is not None:
            want = beam_ref.lse64(l[r])
            if np.isfinite(want):
                assert abs(float(lse[r]) - want) <= logprob_ref.bound(V, want), (r, lse[r], want)
            else:
                assert lse[r] == want
    return sc, row, tok, lp, lse


@pytest.mark.parametrize("V", [160, 4096, 4100, 32000])
def test_candidates_are_the_rules_in_every_split_of_eight_rows(dev, V):
    l, cum = _rows(V, seed=V)
    l[5] = l[2]                                                    # equal rows: with equal cum the row order decides
    cum[5] = cum[2]
    l[1] = np.round(l[1])                                          # equal logits inside a row: the index decides
    dl = torch.from_numpy(l).to(dev)
    seen = set()
    for name, group in SPLITS.items():
        for K in KS:
            sc, row, tok, lp, _ = _check(dl, cum, group, max(group) + 1, K)
            assert (row >= 0).all()
            seen.add(len(set(row.ravel().tolist())))
    assert max(seen) > 1                                           # candidates of one group come from several rows


def test_first_step_form_ignores_the_rows_that_are_members_of_nothing(dev):
    """The state after a prefill: one member per group, the other rows hold garbage."""
    V, K = 160, 16
    l, cum = _rows(V, seed=1)
    group = [0, -1, 2, INT_MIN, 1, 3, INT_MAX, 4]                  # n_groups = 4: entries -1, INT_MIN, INT_MAX and n_groups are no members
    outs = []
    for fill, cfill in ((np.nan, np.nan), (np.inf, np.inf), (7.0, 0.0)):
        a, c = l.copy(), cum.copy()
        for r in (1, 3, 6, 7):
            a[r], c[r] = fill, cfill
        outs.append(_check(torch.from_numpy(a).to(dev), c, group, 4, K)[:4])
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y)
    assert sorted(set(outs[0][1].ravel().tolist())) == [0, 2, 4, 5]
    # a group without any member is all padding; V < K pads a one-member group
    sc, row, tok, lp, _ = _check(torch.from_numpy(l).to(dev), cum, [1] * 8, 2, 4)
    assert (row[0] == -1).all() and (tok[0] == -1).all() and np.isneginf(sc[0]).all() and (row[1] >= 0).all()
    small = torch.from_numpy(l[:, :8].copy()).to(dev)
    sc, row, tok, lp, _ = _check(small, cum, [0, -1, -1, -1, -1, -1, -1, -1], 1, 20)
    assert (row[0, :8] == 0).all() and (row[0, 8:] == -1).all() and sorted(tok[0, :8].tolist()) == list(range(8))


def test_rows_built_to_break_ties(dev):
    V, K = 160, 20
    l, cum = _rows(V, seed=2)
    l[1] = l[0]
    cum[1] = cum[0]                                                # equal rows, equal cum: the row decides
    l[2] = 1.0                                                     # a constant row: the index decides
    l[3] *= np.float32(0.1)
    l[3, :4] = [5.0, np.float32(5.0) - np.float32(2.0 ** -21), 5.0, 4.0]
    cum[3] = -4096.0                                               # different logits that round to one score
    cum[4] = -np.inf                                               # every score of the row is -inf
    cum[5] = np.nan                                                # counts as -inf
    l[6] = -np.inf                                                 # an all -inf row: every lp -inf
    l[6, 3] = np.nan
    l[7, 11] = np.inf                                              # a +inf logit takes the whole mass
    l[7, 90] = np.inf
    cum[7] = -0.0
    l[0, 5] = -0.0
    l[0, 6] = 0.0
    dl = torch.from_numpy(l).to(dev)
    for name, group in SPLITS.items():
        sc, row, tok, lp, lse = _check(dl, cum, group, max(group) + 1, K)
    assert lse[6] == -np.inf and lse[7] == np.inf                  # (the 8 x 1 split: every row alone in its group)
    assert tok[6].tolist() == list(range(K)) and np.isneginf(sc[6]).all()
    assert tok[7, :2].tolist() == [11, 90] and np.allclose(sc[7, :2], -np.log(2.0), atol=1e-6)
    assert np.isneginf(sc[7, 2:]).all() and np.isneginf(sc[4]).all() and np.isneginf(sc[5]).all()
    assert tok[2].tolist() == list(range(K))
    assert len(set(_bits(sc[3, :3]).tolist())) == 1 and tok[3, :3].tolist() == [0, 2, 1]


def test_a_groups_outputs_do_not_depend_on_anything_else(dev):
    import mobilequant_amd as mq
    V, K = 4100, 16
    l, cum = _rows(V, seed=3)
    dl = torch.from_numpy(l).to(dev)
    group = SPLITS["4x2"]
    base = _check(dl, cum, group, 4, K)
    for g in range(4):
        # alone: the other groups' rows are members of nothing (and hold other bytes)
        a = l.copy()
        alone = [v if v == g else -1 for v in group]
        for r in range(8):
            if alone[r] < 0:
                a[r] = np.nan
        got = _check(torch.from_numpy(a).to(dev), cum, alone, 4, K)
        for x, y in zip(base[:4], got[:4]):
            assert np.array_equal(x[g].view(np.int32), y[g].view(np.int32))
        assert np.array_equal(_bits(base[4][2 * g:2 * g + 2]), _bits(got[4][2 * g:2 * g + 2]))
    # group 1's rows (2, 3) moved to rows (4, 7) as group 0 of a one-group launch: the same records under the new row names
    a, c = np.full_like(l, 3.0), np.zeros_like(cum)
    a[4], a[7], c[4], c[7] = l[2], l[3], cum[2], cum[3]
    got = _check(torch.from_numpy(a).to(dev), c, [-1, -1, -1, -1, 0, 5, 9, 0], 1, K)
    assert np.array_equal(np.where(base[1][1] == 2, 4, 7), got[1][0])
    for i in (0, 2, 3):
        assert np.array_equal(base[i][1].view(np.int32), got[i][0].view(np.int32))
    assert _bits(got[4][4]) == _bits(base[4][2]) and _bits(got[4][7]) == _bits(base[4][3])
    # another logits_stride
    wide = torch.full((8, V + 64), float("nan"), device=dev)
    wide[:, :V] = dl
    got = _check(wide[:, :V], cum, group, 4, K)
    for x, y in zip(base, got):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    # replayed from a graph captured without a warm-up launch, under later inputs
    dc, dg = torch.zeros(8, device=dev), torch.full((8,), -1, dtype=torch.int32, device=dev)
    src = torch.zeros_like(dl)
    out = mq.ops.beam_select(dl, torch.tensor(cum).to(dev), torch.tensor(group, dtype=torch.int32).to(dev), 4, K)   # (the buffers' shapes)
    out = tuple(torch.zeros_like(t) for t in out)
    scratch = torch.empty(mq._lib.MQ_BEAM_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mq.ops.beam_select(src, dc, dg, 4, K, out=out, scratch=scratch)
    src.copy_(dl)
    dc.copy_(torch.tensor(cum))
    dg.copy_(torch.tensor(group, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(base, out):
        assert np.array_equal(x.view(np.int32), y.cpu().numpy().view(np.int32))


def test_registered_operator_runs_the_same_launches(dev):
    import mobilequant_amd.torch_ops  # noqa: F401
    l, cum = _rows(160, seed=4)
    dl = torch.from_numpy(l).to(dev)
    want = _check(dl, cum, SPLITS["2x4"], 2, 8)
    got = torch.ops.mobilequant_amd.beam_select(dl, torch.tensor(cum).to(dev), torch.tensor(SPLITS["2x4"], dtype=torch.int32).to(dev), 2, 8)
    for x, y in zip(want, got):
        assert np.array_equal(x.view(np.int32), y.cpu().numpy().view(np.int32))
