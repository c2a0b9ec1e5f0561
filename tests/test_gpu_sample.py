"""GPU: seeded token selection on the device (csrc/mq_sample.hip, mobilequant_amd/sampling.py).

The oracle is tests/sampling_ref.py: a numpy Philox4x32-10 (pinned to Random123's known answers in tests/test_sample_host.py) and the
selection rule with float64 transcendentals.  The random numbers are compared bit for bit.  A drawn token is compared exactly wherever
the reference's decision is wider than fp32 library functions can move it (a DECIDABLE draw: sampling_ref.analyse); every draw must
land in the reference's candidate set plus its boundary band.  The engines are held to the per-sequence contract with no tolerance:
prompt i of a batch == DecodeEngine.generate on that prompt alone with stream i, in any slot, captured or not."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sampling_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# chi-square quantile 1 - 1e-6 for 1 .. 63 degrees of freedom (scipy.stats.chi2.isf(1e-6, dof))
CHI2_1E6 = [23.928, 27.631, 30.665, 33.377, 35.888, 38.258, 40.522, 42.701, 44.811, 46.863, 48.866, 50.825, 52.747, 54.635, 56.493, 58.324,
            60.131, 61.914, 63.677, 65.421, 67.147, 68.856, 70.55, 72.229, 73.895, 75.547, 77.188, 78.817, 80.436, 82.044, 83.643, 85.232,
            86.812, 88.383, 89.947, 91.502, 93.051, 94.592, 96.126, 97.653, 99.174, 100.689, 102.198, 103.701, 105.198, 106.69, 108.177,
            109.659, 111.136, 112.608, 114.076, 115.539, 116.998, 118.452, 119.902, 121.349, 122.791, 124.23, 125.665, 127.096, 128.524,
            129.949, 131.37]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _sample(dev, logits, pos, params, streams, want_extra=True):
    from mobilequant_amd import ops
    rows = logits.shape[0]
    lg = torch.from_numpy(logits).to(dev)
    tok = torch.full((rows,), -7, dtype=torch.int64, device=dev)
    kept = torch.full((rows,), -7, dtype=torch.int32, device=dev) if want_extra else None
    lp = torch.full((rows,), 7.0, dtype=torch.float32, device=dev) if want_extra else None
    ops.sample(lg, torch.tensor(pos, dtype=torch.int32, device=dev), (params, streams), tok, kept=kept, logprob=lp)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), (kept.cpu().numpy() if want_extra else None), (lp.cpu().numpy() if want_extra else None)


# ---- the random numbers, bit exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,stream,n,first", [
    (0, 0, 0, 0),
    (1, 2, 3, 0),
    (0xDEADBEEFCAFEF00D, 0x8000000000000001, 65535, 0),
    (7, 0xFFFFFFFFFFFFFFFF, 65536, 4 * 65536 - 8),            # i / 4 crosses 2^16 inside the block
    (2 ** 64 - 1, 0xFEDCBA9876543210, 0x7FFFFFFF, 1_000_000),
    (12345, 1 << 63, 70_001, (1 << 20) - 4096),
])
def test_uniforms_are_the_numpy_philox_bit_for_bit(dev, seed, stream, n, first):
    from mobilequant_amd import ops
    count = 4096
    got = ops.sample_uniforms(seed, stream, n, first, count, dev).cpu().numpy()
    want = R.uniforms(seed, stream, n, np.arange(first, first + count))
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got.min() > 0.0 and got.max() < 1.0


# ---- the token against the float64 reference ---------------------------------------------------------------------------------------
FAMILIES = ("gauss1", "gauss4", "neg_inf", "tie_max", "tie_cut")


def _row(rng, V, family):
    l = rng.standard_normal(V).astype(np.float32)
    if family == "gauss4":
        l *= np.float32(4.0)
    elif family == "neg_inf":
        l[rng.random(V) < 0.3] = -np.inf
        l[int(rng.integers(V))] = np.nan                       # a NaN counts as -inf
    elif family == "tie_max":
        idx = rng.choice(V, size=min(1000, V // 2), replace=False)
        l[idx] = l.max() + np.float32(0.5)                     # a 1 000-fold tie at the maximum (half the row at V = 64)
    elif family == "tie_cut":
        order = np.argsort(-l, kind="stable")
        lo, hi = min(20, V // 8), min(80, V // 2)
        l[order[lo:hi]] = l[order[lo]]                         # equal logits on both sides of rank 40 (the top-k cut)
    return l


def _grid(V):
    return list(itertools.product((0.0, 0.7, 1.3), (0, 1, 40, V), (1.0, 0.9, 0.1), (0.0, 0.05)))


@pytest.mark.parametrize("V", [64, 1024, 32000, 256000])
def test_tokens_match_the_float64_reference_wherever_it_is_decidable(dev, V):
    """Rows 1 .. 8 per launch; every row of a launch carries its own request, so each row count sees the whole parameter grid
    (temperature {0, 0.7, 1.3} x top_k {0, 1, 40, V} x top_p {1, 0.9, 0.1} x min_p {0, 0.05}) over the five logits families.
    A configuration, for the 1 % cap on undecidable draws, is a vocabulary size: its 584 draws are pooled over the grid, the
    families and the row counts; the share per family and per parameter combination is printed.  delta = 64 ulp_fp32(max|z| + max|g|)
    and the band of 2^-20 W_K are sampling_ref.analyse's.  Measured on an MI355X: 0 / 3 / 3 / 5 undecidable of 584 draws at V = 64 / 1 024 / 32 000 / 256 000 (0 / 0.51 / 0.51 /
    0.86 %), the Gaussian and -inf families 0 everywhere.  Nearly all of them are the tie at the maximum with top_k = 40 and top_p 0.9 /
    0.1: every tied token weighs exactly 2^32 there and fp32(0.9) * 40 is 36 - 1e-6, so the token of rank 36 sits 2^-25 W_K from the
    threshold -- inside the band by its definition, whatever computes the draw (the device is exact on it: expf(0) = 1)."""
    from mobilequant_amd import SamplingParams
    rng = np.random.default_rng(1000 + V)
    grid = _grid(V)
    stats = {f: [0, 0] for f in FAMILIES}                      # family -> [draws, undecidable]
    by_combo = {}
    draw = 0
    for rows in range(1, 9):
        for start in range(0, len(grid), rows):
            combos = [grid[(start + r) % len(grid)] for r in range(rows)]
            fams = [FAMILIES[(draw + r) % len(FAMILIES)] for r in range(rows)]
            logits = np.stack([_row(rng, V, f) for f in fams])
            pos = [int(rng.integers(0, 100_000)) for _ in range(rows)]
            seeds = [int(rng.integers(0, 2 ** 63)) for _ in range(rows)]
            streams = [int(rng.integers(0, 2 ** 63)) * 2 + 1 for _ in range(rows)]
            params = [SamplingParams(temperature=t, top_k=k, top_p=p, min_p=m, seed=s) for (t, k, p, m), s in zip(combos, seeds)]
            tok, kept, lp = _sample(dev, logits, pos, params, streams)
            plain, _, _ = _sample(dev, logits, pos, params, streams, want_extra=False)      # (unfiltered rows: the sliced launch)
            assert np.array_equal(tok, plain), (V, rows, tok, plain)
            for r in range(rows):
                t, k, p, m = combos[r]
                a = R.analyse(logits[r], t, k, p, m, seeds[r], streams[r], pos[r])
                stats[fams[r]][0] += 1
                c = by_combo.setdefault(combos[r], [0, 0])
                c[0] += 1
                what = (V, rows, r, fams[r], combos[r], int(tok[r]), a["token"])
                assert int(tok[r]) in a["allowed"], what            # never outside the reference's C plus the band
                if a["decidable"]:
                    assert int(tok[r]) == a["token"], what
                else:
                    stats[fams[r]][1] += 1
                    c[1] += 1
                if t > 0:
                    assert a["kept_lo"] <= int(kept[r]) <= a["kept_hi"], what + (int(kept[r]), a["kept_lo"], a["kept_hi"])
                    if a["kept_lo"] == a["kept_hi"] and a["decidable"]:
                        z = (np.where(np.isnan(logits[r]), np.float32(-np.inf), logits[r]) / np.float32(t)).astype(np.float32).astype(np.float64)
                        zc = z[a["C"]]
                        want = z[a["token"]] - (zc.max() + np.log(np.exp(zc - zc.max()).sum()))
                        # the kernel's stated tolerance: 2^-23 (2 + log V) + V / W_C + ulp_fp32(logprob), W_C in units of 2^-32
                        tol = 2.0 ** -23 * (2 + np.log(V)) + V / (np.exp(zc - zc.max()).sum() * 2.0 ** 32) + R.ulp32(want)
                        assert abs(float(lp[r]) - want) <= tol, what + (float(lp[r]), want, tol)
                else:
                    assert int(kept[r]) == 1
            draw += rows
    for f, (n, u) in stats.items():
        print(f"V={V} family={f}: {n} draws, {u} undecidable ({100.0 * u / n:.3f} %)")
    for combo, (n, u) in sorted(by_combo.items()):
        if u:
            print(f"V={V} combo={combo}: {u} of {n} undecidable")
    n_all, u_all = sum(n for n, _ in stats.values()), sum(u for _, u in stats.values())
    print(f"V={V}: {n_all} draws, {u_all} undecidable ({100.0 * u_all / n_all:.3f} %)")
    assert u_all <= 0.01 * n_all, (V, n_all, u_all)


def test_idle_rows_keep_their_token_and_out_of_range_rows_are_greedy(dev):
    import ctypes
    from mobilequant_amd import _lib, ops
    from mobilequant_amd.sampling import ROW_DTYPE
    V = 1024
    rng = np.random.default_rng(5)
    logits = rng.standard_normal((4, V)).astype(np.float32)
    lg = torch.from_numpy(logits).to(dev)
    tok = torch.full((4,), -7, dtype=torch.int64, device=dev)
    pos = torch.tensor([3, 16, -1, 15], dtype=torch.int32, device=dev)         # cache_len 16: rows 1 and 2 are idle
    rows = np.zeros(4, dtype=ROW_DTYPE)
    rows[:] = (0.8, 0, 1.0, 0.0, 1, 2)
    rows[3] = (-1.0, 5, 0.5, 0.0, 1, 2)                                        # temperature < 0: served as greedy
    pr = torch.from_numpy(rows.view(np.uint8).reshape(-1)).to(dev)
    ops.sample(lg, pos, pr, tok, cache_len=16)
    got = tok.cpu().tolist()
    assert got[1] == -7 and got[2] == -7
    assert got[0] == R.analyse(logits[0], 0.8, 0, 1.0, 0.0, 1, 2, 3)["token"]
    assert got[3] == int(np.argmax(logits[3]))
    # all -inf / NaN: token 0
    bad = np.full((1, V), -np.inf, dtype=np.float32)
    bad[0, 5] = np.nan
    from mobilequant_amd import SamplingParams
    for sp in (SamplingParams(), SamplingParams(top_k=10, top_p=0.5), SamplingParams(temperature=0.0)):
        t, _, _ = _sample(dev, bad, [0], [sp], [0])
        assert int(t[0]) == 0


# ---- the distribution ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (8, 0.8)])
def test_draws_follow_the_restricted_softmax(dev, top_k, top_p):
    """V = 64, fixed logits, 200 000 draws (n = 0 .. 24 999 over 8 streams).  Chi-square against the exact restricted softmax in
    float64; threshold = the 1 - 1e-6 quantile for the degrees of freedom.  No token outside C is ever drawn."""
    from mobilequant_amd import SamplingParams, ops
    from mobilequant_amd.sampling import pack_rows
    V, N, T = 64, 25000, 0.9
    rng = np.random.default_rng(77)
    l = (rng.standard_normal(V) * 1.5).astype(np.float32)
    p = R.restricted_softmax(l, T, top_k, top_p, 0.0)
    C = np.flatnonzero(p > 0)
    lg = torch.from_numpy(np.tile(l, (8, 1))).to(dev)
    host = pack_rows([SamplingParams(temperature=T, top_k=top_k, top_p=top_p, seed=99)] * 8, list(range(8)))
    pr = torch.from_numpy(host.view(np.uint8).reshape(-1)).to(dev)
    pos = torch.arange(N, dtype=torch.int32, device=dev).view(N, 1).repeat(1, 8).contiguous()
    toks = torch.full((N, 8), -1, dtype=torch.int64, device=dev)
    for n in range(N):
        ops.sample(lg, pos[n], pr, toks[n])
    torch.cuda.synchronize()
    t = toks.cpu().numpy().reshape(-1)
    counts = np.bincount(t, minlength=V).astype(np.float64)
    assert counts[p == 0].sum() == 0
    exp = p[C] * t.size
    assert exp.min() > 5
    chi2 = float(((counts[C] - exp) ** 2 / exp).sum())
    dof = len(C) - 1
    print(f"top_k={top_k} top_p={top_p}: |C|={len(C)} chi2={chi2:.2f} dof={dof} threshold={CHI2_1E6[dof - 1]}")
    assert chi2 < CHI2_1E6[dof - 1], (chi2, dof)


# ---- the per-sequence contract, bit exact ---------------------------------------------------------------------------------------------
def _flat_model(dev):
    """The batched-decode tests' model with the lm_head scaled down: a flat next-token distribution (160 entries), so that sampled
    continuations of 24 tokens under different seeds or streams collide with probability about 160^-24 << 2^-40."""
    from test_gpu_decode_batch import _model
    m = _model(dev, "llama", 2, 8)
    with torch.no_grad():
        m.lm_head.weight.mul_(0.05)
    return m


def test_batch_generate_is_the_single_engine_per_prompt_in_any_slot_captured_or_not(dev):
    from test_gpu_decode_batch import _prompts
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _flat_model(dev)
    NEW = 24
    prompts = _prompts(m.shape.vocab, [1, 5, 17, 64, 65, 120, 9, 33], seed=12)
    sps = [SamplingParams(temperature=0.9, seed=11), SamplingParams(temperature=0.7, top_k=40, top_p=0.9, seed=11),
           SamplingParams(temperature=1.3, top_p=0.8, min_p=0.02, seed=5), SamplingParams(temperature=0.0),
           SamplingParams(temperature=1.0, top_k=5, seed=2 ** 64 - 1), SamplingParams(temperature=0.8, min_p=0.05, seed=3),
           SamplingParams(temperature=1.1, top_k=40, top_p=0.5, min_p=0.01, seed=4), SamplingParams(temperature=0.6, top_p=0.95, seed=8)]
    single = DecodeEngine(m, cache_len=256)
    want = [single.generate(p, NEW, sampling=sp, stream=i) for i, (p, sp) in enumerate(zip(prompts, sps))]
    assert all(len(o) == len(p) + NEW for o, p in zip(want, prompts))
    assert want == [single.generate(p, NEW, sampling=sp, stream=i) for i, (p, sp) in enumerate(zip(prompts, sps))]      # two runs repeat
    single.capture()
    assert want == [single.generate(p, NEW, sampling=sp, stream=i) for i, (p, sp) in enumerate(zip(prompts, sps))]      # graph == eager
    assert want[0] == single.generate(prompts[0], NEW, sampling=sps[0], stream=0, prefill=False)
    for B in (1, 3, 8):
        for captured in (False, True):
            be = BatchDecodeEngine(m, B, cache_len=256)
            if captured:
                be.capture()
            got = be.generate(prompts[:B], NEW, sampling=sps[:B])
            assert got == want[:B], (B, captured)
            assert got == be.generate(prompts[:B], NEW, sampling=sps[:B])
            if B > 1:                                          # permuted across the slots: the stream, not the slot, names the sequence
                perm = list(np.random.default_rng(B).permutation(B))
                got_p = be.generate([prompts[i] for i in perm], NEW, sampling=[sps[i] for i in perm], streams=[int(i) for i in perm])
                assert got_p == [want[i] for i in perm], (B, captured, perm)
    # one request for every prompt; a sequence leaves at its EOS and the others go on unchanged
    be = BatchDecodeEngine(m, 8, cache_len=256).capture()
    sp = SamplingParams(temperature=0.9, top_k=50, seed=21)
    ref = [single.generate(p, NEW, sampling=sp, stream=i) for i, p in enumerate(prompts)]
    assert be.generate(prompts, NEW, sampling=sp) == ref
    eos = ref[2][len(prompts[2]) + 3]
    assert be.generate(prompts, NEW, sampling=sp, eos_token_id=eos) == [single.generate(p, NEW, sampling=sp, stream=i, eos_token_id=eos)
                                                                        for i, p in enumerate(prompts)]
    # another seed or another stream is another continuation
    a = single.generate(prompts[3], NEW, sampling=sp, stream=3)
    assert a == ref[3]
    assert single.generate(prompts[3], NEW, sampling=SamplingParams(temperature=0.9, top_k=50, seed=22), stream=3) != a
    assert single.generate(prompts[3], NEW, sampling=sp, stream=4) != a
    assert single.generate(prompts[3], NEW, sampling=sp, stream=3 + (1 << 32)) != a


def test_sampled_tokens_are_the_reference_rule_on_the_engines_own_logits(dev):
    """generate(sampling=...) step by step == sampling_ref on the logits the engine holds in front of every draw (where decidable)."""
    from test_gpu_decode_batch import _prompts
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine
    m = _flat_model(dev)
    eng = DecodeEngine(m, cache_len=128).capture()
    prompt = _prompts(m.shape.vocab, [9], seed=4)[0]
    sp = SamplingParams(temperature=0.8, top_k=40, top_p=0.9, seed=77)
    got = eng.generate(prompt, 16, sampling=sp, stream=5)
    eng.reset()
    eng.prefill(prompt)
    seq, undecided = list(prompt), 0
    for _ in range(16):
        a = R.analyse(eng.logits.cpu().numpy(), 0.8, 40, 0.9, 0.0, 77, 5, len(seq))
        nxt = got[len(seq)]
        assert nxt in a["allowed"]
        if a["decidable"]:
            assert nxt == a["token"], (len(seq), nxt, a["token"])
        else:
            undecided += 1
        seq.append(nxt)
        eng.step(nxt)
    assert undecided <= 1


def test_greedy_parity_and_legacy_paths(dev):
    """SamplingParams(temperature=0) == plain generate on tests/golden/generate_case.npz (margins >= 3 % of the logit span: no tie in
    play), in both engines; generate(do_sample=True, generator=...) still is the hand-applied multinomial rule."""
    from conftest import load_npz
    from test_gpu_round2 import _decode_model
    from mobilequant_amd import SamplingParams
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m, _ = _decode_model(dev)
    z = load_npz("generate_case.npz")
    ctx, want = z["context"].tolist(), z["tokens"].tolist()
    new = len(want) - len(ctx)
    greedy = SamplingParams(temperature=0.0)
    eng = DecodeEngine(m, cache_len=64)
    assert eng.generate(ctx, new) == want
    assert eng.generate(ctx, new, sampling=greedy) == want
    eng.capture()
    assert eng.generate(ctx, new, sampling=greedy, stream=9) == want
    for captured in (False, True):
        be = BatchDecodeEngine(m, 2, cache_len=64)
        if captured:
            be.capture()
        assert be.generate([ctx, ctx[:5]], new, sampling=greedy) == be.generate([ctx, ctx[:5]], new)
        assert be.generate([ctx], new, sampling=greedy)[0] == want
    g1 = torch.Generator(device=dev).manual_seed(123)
    got = eng.generate(ctx, 10, do_sample=True, temperature=0.7, generator=g1)
    g2 = torch.Generator(device=dev).manual_seed(123)
    eng.reset()
    eng.prefill(ctx)
    by_hand = list(ctx)
    for _ in range(10):
        nxt = int(torch.multinomial(torch.softmax(eng.logits / 0.7, dim=-1), num_samples=1, generator=g2))
        by_hand.append(nxt)
        eng.step(nxt)
    assert got == by_hand
