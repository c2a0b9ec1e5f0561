"""GPU: token scoring -- the fused lm_head log-softmax (csrc/mq_score.hip, ops.score_head) and mobilequant_amd/scoring.py.

The kernel is held to a float64 reference of the same logits under the error bound its header states (evaluated per row here):
every lse and logprob within the bound, argmax equal to float64's wherever the top two logits are further apart than twice the bound
and the lowest index on exact ties.  Rows are independent of their launch and bit-reproducible; no [M, V] tensor is allocated.  End
to end the API is checked against the model's own logits (three families, W8 / W4, module chain and fused layers), batched scoring
against scoring alone (bit for bit), and the 22-layer fixture's perplexity against the reference's recorded NLL."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BV = 128                               # the kernel's vocabulary tile (partials per row: T = ceil(V / 128))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def gamma(n):
    return n * U / (1 - n * U)


def reference(y, w, b, t, chunk=8192):
    """float64 per-row (lse, logprob, argmax, top-two gap, E = max_v e_v, e_target) of y @ w.T (+ b), vocabulary in chunks.
    e_v = gamma_{K+1} (|b_v| + sum_k |y_k w_vk|) over the finite columns (a -inf bias column is exactly -inf in both)."""
    M, K = y.shape
    V = w.shape[0]
    y64, ay = y.double(), y.double().abs()
    lse = torch.full((M,), -math.inf, dtype=torch.float64, device=y.device)
    top = torch.full((M, 2), -math.inf, dtype=torch.float64, device=y.device)
    arg = torch.zeros(M, dtype=torch.int64, device=y.device)
    E = torch.zeros(M, dtype=torch.float64, device=y.device)
    lt = torch.zeros(M, dtype=torch.float64, device=y.device)
    et = torch.zeros(M, dtype=torch.float64, device=y.device)
    g = gamma(K + 1)
    for v0 in range(0, V, chunk):
        wc = w[v0:v0 + chunk].double()
        lg = y64 @ wc.T
        s = ay @ wc.abs().T
        if b is not None:
            bc = b[v0:v0 + chunk].double()
            lg = lg + bc
            s = s + torch.where(torch.isinf(bc), torch.zeros_like(bc), bc.abs())
        e = g * s
        E = torch.maximum(E, e.max(1).values)
        lse = torch.logaddexp(lse, torch.logsumexp(lg, 1))
        n = lg.shape[1]
        tv, ti = torch.topk(lg, min(2, n), dim=1)       # (ties: topk's order is not the lowest index; argmax is computed apart)
        cmax, carg = lg.max(1)
        first = torch.argmax((lg == cmax[:, None]).to(torch.int8), 1)
        upd = cmax > top[:, 0]
        arg = torch.where(upd, first + v0, arg)
        both = torch.cat([top, tv if n >= 2 else torch.cat([tv, torch.full_like(tv, -math.inf)], 1)], 1)
        top = torch.topk(both, 2, dim=1).values
        inside = (t >= v0) & (t < v0 + n)
        idx = (t - v0).clamp(0, n - 1)[:, None]
        lt = torch.where(inside, lg.gather(1, idx)[:, 0], lt)
        et = torch.where(inside, e.gather(1, idx)[:, 0], et)
    lp = torch.where(t >= 0, lt - lse, torch.zeros_like(lse))
    return dict(lse=lse, lp=lp, arg=arg, gap=top[:, 0] - top[:, 1], E=E, et=et)


def bounds(ref, V):
    T = -(-V // BV)
    lse = ref["lse"]
    b_lse = ref["E"] + 1.01 * (2 * U * math.log(V) + 8 * U + gamma(T + 129)) + 4 * U * math.log(V) + U * lse.abs()
    b_lp = torch.where(ref["lp"] != 0, ref["et"] + b_lse + U * ref["lp"].abs(), torch.zeros_like(b_lse))
    return b_lse, b_lp


def check_against_reference(y, w, b, t, what, nan_rows=(), ties=()):
    """Run ops.score_head and hold every row to the float64 bound; returns the worst error / bound ratio."""
    from mobilequant_amd import ops
    lp, lse, am = ops.score_head(y, w, b, t)
    torch.cuda.synchronize()
    ref = reference(y, w, b, t)
    V = w.shape[0]
    b_lse, b_lp = bounds(ref, V)
    ok = torch.ones(y.shape[0], dtype=torch.bool, device=y.device)
    for r in nan_rows:                                     # a NaN row: lse / logprob NaN, argmax its first NaN (every logit is NaN: 0)
        assert torch.isnan(lse[r]) and (t[r] < 0 or torch.isnan(lp[r])) and int(am[r]) == 0, (what, r)
        ok[r] = False
    ign = (t < 0) & ok
    assert torch.equal(lp[ign], torch.zeros_like(lp[ign])), what
    d_lse = (lse.double() - ref["lse"]).abs()[ok]
    d_lp = (lp.double() - ref["lp"]).abs()[ok]
    assert torch.isfinite(lse[ok]).all(), what
    r_lse = float((d_lse / b_lse[ok]).max())
    bad = d_lp > b_lp[ok]
    assert not bool(bad.any()), (what, float(d_lp[bad].max()), float(b_lp[ok][bad].min()))
    assert r_lse <= 1.0, (what, r_lse)
    r_lp = float((d_lp[b_lp[ok] > 0] / b_lp[ok][b_lp[ok] > 0]).max()) if bool((b_lp[ok] > 0).any()) else 0.0
    # exact ties: the duplicated W rows give bit-identical fp32 logits, but float64 GEMM launches over different vocabulary chunks (or
    # edge tiles) need not round them alike: where float64's argmax is one of them, the answer is the first of them
    gap = ref["gap"][ok]
    am_ok, arg_ok = am[ok], ref["arg"][ok].clone()
    tied = torch.zeros_like(arg_ok, dtype=torch.bool)
    for d in ties:
        tied |= arg_ok == d
    arg_ok[tied] = min(ties) if ties else 0
    decided = (gap > 2 * ref["E"][ok]) | tied
    wrong = decided & (am_ok != arg_ok)
    assert not bool(wrong.any()), (what, int(wrong.sum()), am_ok[wrong][:4].tolist(), arg_ok[wrong][:4].tolist())
    print(f"{what}: worst |error| / bound  lse {r_lse:.4f}  logprob {r_lp:.4f}; argmax decided on {int(decided.sum())} / {int(ok.sum())} "
          f"rows, {int(tied.sum())} exact ties")
    return max(r_lse, r_lp)


def make_case(M, K, V, with_bias, seed, dev, specials=True):
    """y [M, K], W [V, K], bias, targets with: ignored targets, exact ties (W rows duplicated inside and across tiles and made the
    maximum for half the rows), logits of +-1e4, a bias of -inf over a whole tile, one NaN row."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    y = torch.randn(M, K, generator=g)
    w = torch.randn(V, K, generator=g) * (3.0 / math.sqrt(K))
    b = torch.randn(V, generator=g) if with_bias else None
    t = torch.randint(0, V, (M,), generator=g)
    t[::7] = -1
    nan_rows, dup = [], []
    if specials:
        if V >= 3:
            dup = sorted({1, V // 2, V - 1})
            base = y[: (M + 1) // 2].mean(0)                    # aligned with the first half of the rows: their maximum, a 3-way tie
            w[dup] = (base / base.norm() * 6.0).expand(len(dup), K)
            if b is not None:
                b[dup] = 0.0
        if M >= 3:
            y[2] *= 1e4 / 3.0                                   # logits ~ +-1e4: exp(l) overflows fp32 many times over
        if b is not None and V >= 2 * BV:
            b[BV:2 * BV] = -math.inf                            # tile 1 entirely -inf for every row
            t[(t >= BV) & (t < 2 * BV)] = 0
        if M >= 5:
            y[4, K // 2] = float("nan")
            nan_rows = [4]
    return y.to(dev), w.to(dev), (b.to(dev) if b is not None else None), t.to(dev), nan_rows, dup


MS = [1, 63, 300, 2048]
VS = [97, 160, 1003, 32000, 100352, 256000]
CASES = [(M, 2048 if (i + j) % 2 else 128, V, (i + 2 * j) % 3 != 0) for i, M in enumerate(MS) for j, V in enumerate(VS)]


@pytest.mark.parametrize("M,K,V,with_bias", CASES)
def test_score_head_lies_within_its_bound_of_float64(dev, M, K, V, with_bias):
    y, w, b, t, nan_rows, dup = make_case(M, K, V, with_bias, seed=M * 7 + V, dev=dev)
    check_against_reference(y, w, b, t, f"M {M} K {K} V {V} bias {with_bias}", nan_rows, dup)


@pytest.mark.parametrize("K", [128, 2048])
def test_score_head_plain_random_inputs_at_both_depths(dev, K):
    """No special values: every row's lse and logprob bounded, argmax decided almost everywhere."""
    y, w, b, t, _, _ = make_case(300, K, 32000, True, seed=K, dev=dev, specials=False)
    check_against_reference(y, w, b, t, f"plain K {K}")


def test_exact_ties_across_tiles_take_the_lowest_index(dev):
    """Three identical W rows (tile 0, a middle tile, the ragged last tile) maximal for every row: argmax is the first of them;
    a duplicate of the maximum in an EARLIER tile than the first maximum moves argmax there."""
    from mobilequant_amd import ops
    g = torch.Generator(device="cpu").manual_seed(3)
    M, K, V = 300, 256, 1003
    y = torch.randn(M, K, generator=g).abs()
    w = torch.randn(V, K, generator=g) * 0.01
    w[[500, 700, 1002]] = 1.0
    lp, lse, am = ops.score_head(y.to(dev), w.to(dev), None, None)
    assert (am.cpu() == 500).all()
    w[130] = 1.0
    lp, lse, am = ops.score_head(y.to(dev), w.to(dev), None, None)
    assert (am.cpu() == 130).all()
    assert torch.equal(lp, torch.zeros_like(lp))                 # no targets: logprob 0


def test_all_minus_inf_rows_give_minus_inf_lse_and_no_nan_elsewhere(dev):
    from mobilequant_amd import ops
    g = torch.Generator(device="cpu").manual_seed(4)
    M, K, V = 64, 128, 1003
    y = torch.randn(M, K, generator=g)
    w = torch.randn(V, K, generator=g) * 0.1
    b = torch.full((V,), -math.inf)
    b[900:] = 0.0                                               # seven of eight tiles entirely -inf
    t = torch.randint(900, V, (M,), generator=g)
    lp, lse, am = ops.score_head(y.to(dev), w.to(dev), b.to(dev), t.to(dev))
    want = torch.log_softmax((y.double() @ w.double().T + b.double()), -1)
    assert torch.isfinite(lse).all() and torch.isfinite(lp).all()
    assert ((am.cpu() >= 900)).all()
    assert float((lp.double().cpu() - want.gather(1, t[:, None])[:, 0]).abs().max()) < 1e-4


def test_rows_are_independent_of_the_launch_and_reproducible(dev):
    """A row's outputs are bit-identical alone (M = 1), inside M = 2048, at other row offsets, through a strided view, and twice."""
    from mobilequant_amd import ops
    y, w, b, t, _, _ = make_case(2048, 2048, 32000, True, seed=9, dev=dev, specials=False)
    full = ops.score_head(y, w, b, t)
    again = ops.score_head(y, w, b, t)
    for a, c in zip(full, again):
        assert torch.equal(a, c)
    for r in (0, 1, 127, 128, 1000, 2047):
        one = ops.score_head(y[r:r + 1], w, b, t[r:r + 1])
        for a, c in zip(one, full):
            assert torch.equal(a, c[r:r + 1]), r
    for off, n in ((5, 300), (77, 63), (1900, 148)):
        part = ops.score_head(y[off:off + n], w, b, t[off:off + n])
        for a, c in zip(part, full):
            assert torch.equal(a, c[off:off + n]), (off, n)
    wide = torch.zeros(2048, 2048 + 12, device=dev)
    wide[:, 4:4 + 2048] = y
    view = wide[:, 4:4 + 2048]                                   # row stride 2060, 16-byte aligned rows
    assert view.stride(0) == 2060
    for a, c in zip(ops.score_head(view, w, b, t), full):
        assert torch.equal(a, c)


def test_no_logits_tensor_is_allocated(dev):
    """V = 256 000, M = 4 096: the allocator's peak grows by less than 1/16 of M V 4 bytes during score_head."""
    from mobilequant_amd import ops
    M, K, V = 4096, 128, 256000
    g = torch.Generator(device=dev).manual_seed(1)
    y = torch.randn(M, K, device=dev, generator=g)
    w = torch.randn(V, K, device=dev, generator=g) * 0.1
    t = torch.randint(0, V, (M,), device=dev, generator=g)
    ops.score_head(y[:8], w, None, t[:8])                        # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    lp, lse, am = ops.score_head(y, w, None, t)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated(dev) - base
    print(f"score_head M {M} V {V}: peak grew by {grew / 2**20:.1f} MiB; logits would be {M * V * 4 / 2**20:.0f} MiB")
    assert grew < M * V * 4 / 16, grew
    assert torch.isfinite(lp).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
GEOMS = {
    "llama": dict(hidden=256, heads=32, kv_heads=4, head_dim=64, ffn=512, vocab=160),
    "stablelm": dict(hidden=256, heads=4, kv_heads=4, head_dim=64, ffn=512, vocab=96, norm="layernorm", qkv_bias=True, rotary_pct=0.25),
    "gemma": dict(hidden=256, heads=2, kv_heads=1, head_dim=256, ffn=512, vocab=128, hidden_act="gelu", embed_scale=True, eps=1e-6),
}


def _model(dev, geom, wbits, fused, layers=2, max_pos=2048, seed=11):
    """The decode tests' random models (tests/test_gpu_decode_batch.py's recipe) with room for 2 048 positions."""
    import mobilequant_amd as mq
    from mobilequant_amd import llama
    from mobilequant_amd.calibration import get_act_range
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    shape = LlamaShape(layers=layers, max_pos=max_pos, **GEOMS[geom])
    m = LlamaForCausalLM(shape)
    m.reset_parameters(seed=seed, std=0.08)
    m = m.to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(5)
    act = get_act_range(m, [torch.randint(0, shape.vocab, (1, 48), generator=g) for _ in range(2)])
    mq.create_sim_qmodel(m, mq.QuantConfig(bitwidth=wbits, is_per_channel=wbits == 4), mq.QuantConfig(bitwidth=8))
    for n, mod in m.named_modules():                          # ptq/mobilequant.py:175-201
        if isinstance(mod, mq.QLinear):
            if "w2" in n:
                mod.weight_quantizer.qcfg.is_per_channel = True
                mod.output_quantizer.qcfg.bitwidth = 16
            elif "o_proj" in n:
                mod.output_quantizer.qcfg.bitwidth = 16
        elif isinstance(mod, (mq.QRMSNorm, mq.QLayerNorm)):
            mod.input_quantizer.qcfg.bitwidth = 16
            mod.weight_quantizer.qcfg.bitwidth = 16
            mod.weight_quantizer.qcfg.is_symmetric = False
            mod.weight_quantizer.qcfg.is_per_channel = False
        elif isinstance(mod, mq.QMatMul):
            if "qk_bmm" in n:
                mod.output_quantizer.qcfg.bitwidth = 16
            if "pv_bmm" in n:
                mod.input_quantizer.qcfg.bitwidth = 16
    mq.set_scale_and_offset(m, act, "buffer")
    if fused:
        assert llama.fuse_decoder_layer(m) == layers
    return m


def _explicit(m, ids, targets):
    """What scoring must reproduce, from the model's own forward: float64 log_softmax of model(ids) at the targets, its argmax, and
    the head bound (reference() on the final norm's rows, doubled: the library lm_head and the fused head each lie within it)."""
    with torch.no_grad():
        logits = m(ids).double()
        y = m.norm(m.hidden_states(ids))
    B, S, V = logits.shape
    t = targets.reshape(-1)
    lsm = torch.log_softmax(logits.reshape(B * S, V), -1)
    lp = torch.where(t >= 0, lsm.gather(1, t.clamp(min=0)[:, None])[:, 0], torch.zeros(B * S, dtype=torch.float64, device=ids.device))
    ref = reference(y.reshape(B * S, -1), m.lm_head.weight, m.lm_head.bias, t)
    b_lse, b_lp = bounds(ref, V)
    return (lp.view(B, S), torch.logsumexp(logits, -1), logits.argmax(-1), 2 * b_lp.view(B, S), 2 * b_lse.view(B, S),
            ref["gap"].view(B, S), ref["E"].view(B, S))


@pytest.mark.parametrize("fused", [False, True], ids=["module_chain", "fused"])
@pytest.mark.parametrize("wbits", [8, 4])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_scoring_matches_the_models_own_logits(dev, geom, wbits, fused):
    from mobilequant_amd import scoring
    m = _model(dev, geom, wbits, fused)
    V = m.shape.vocab
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(0, V, (3, 192), generator=g).to(dev)
    # token_logprobs: next-token targets, last position without one
    lp, lse, am = scoring.token_logprobs(m, ids)
    want_lp, want_lse, want_am, b_lp, b_lse, gap, E = _explicit(m, ids, torch.cat([ids[:, 1:], torch.full_like(ids[:, :1], -1)], 1))
    body = (slice(None), slice(0, -1))
    assert ((lp.double() - want_lp).abs()[body] <= b_lp[body]).all(), float((lp.double() - want_lp).abs().max())
    assert ((lse.double() - want_lse).abs()[body] <= b_lse[body]).all()
    decided = (gap > 4 * E)[body]
    assert torch.equal(am[body][decided], want_am[body][decided])
    assert (lp[:, -1] == 0).all() and torch.isnan(lse[:, -1]).all() and (am[:, -1] == -1).all()
    # loglikelihood: every request against an explicit forward of its own padded input; batched == alone, bit for bit
    reqs = []
    for n_ctx, n_cont in ((1, 1), (5, 3), (40, 24), (63, 1), (64, 7), (100, 30), (150, 140), (2, 64), (130, 2)):
        reqs.append((torch.randint(0, V, (n_ctx,), generator=g).tolist(), torch.randint(0, V, (n_cont,), generator=g).tolist()))
    ctx = reqs[2][0]                                            # a greedy continuation: the argmax after a 40-token context
    x = torch.zeros(1, 64, dtype=torch.int64)
    x[0, :40] = torch.tensor(ctx)
    tg = torch.full((1, 64), -1, dtype=torch.int64)
    tg[0, 39] = 0
    reqs.append((ctx, [int(scoring.token_logprobs(m, x.to(dev), tg.to(dev))[2][0, 39])]))
    assert scoring.batches_requests(m) == fused                  # the module chain is scored one request per forward
    got = scoring.loglikelihood(m, reqs, max_length=160, batch_size=4)
    alone = [scoring.loglikelihood(m, [r], max_length=160, batch_size=1)[0] for r in reqs]
    assert got == alone, [(a, b) for a, b in zip(got, alone) if a != b]
    for (ctx, cont), (ll, greedy) in zip(reqs, got):
        inp, _, p0 = scoring.request_rows(ctx, cont, 160)
        L = scoring._padded_len(len(inp), m.shape.max_pos)
        x = torch.zeros(1, L, dtype=torch.int64)
        x[0, :len(inp)] = torch.tensor(inp)
        tg = torch.full((1, L), -1, dtype=torch.int64)
        tg[0, p0:p0 + len(cont)] = torch.tensor(cont)
        w_lp, _, w_am, w_b, _, w_gap, w_E = _explicit(m, x.to(dev), tg.to(dev))
        sl = slice(p0, p0 + len(cont))
        assert abs(ll - float(w_lp[0, sl].sum())) <= float(w_b[0, sl].sum()), (ll, float(w_lp[0, sl].sum()))
        if bool((w_gap[0, sl] > 4 * w_E[0, sl]).all()):
            assert greedy == bool((w_am[0, sl].cpu() == torch.tensor(cont)).all())
    assert got[-1][1]


def test_rolling_loglikelihood_is_the_sum_of_explicit_window_forwards(dev):
    """5 000 tokens at max_length 2 048 (three windows, each a full 2 048-token input), fused W8 llama geometry."""
    from mobilequant_amd import scoring
    m = _model(dev, "llama", 8, True)
    g = torch.Generator().manual_seed(8)
    toks = torch.randint(0, m.shape.vocab, (5000,), generator=g).tolist()
    total = scoring.loglikelihood_rolling(m, toks, max_length=2048, prefix_token=0)
    wins = scoring.rolling_windows(toks, 2048, 0)
    assert [len(c) + len(x) - 1 for c, x in wins] == [2048, 2048, 2048] and sum(len(x) for _, x in wins) == 5000
    want, tol = 0.0, 0.0
    for ctx, cont in wins:
        inp, _, p0 = scoring.request_rows(ctx, cont, 2048)
        tg = torch.full((1, len(inp)), -1, dtype=torch.int64)
        tg[0, p0:] = torch.tensor(cont)
        w_lp, _, _, w_b, _, _, _ = _explicit(m, torch.tensor([inp]).to(dev), tg.to(dev))
        want += float(w_lp.sum())
        tol += float(w_b.sum())
    print(f"rolling: {total:.6f} vs explicit {want:.6f} (bound {tol:.3g})")
    assert abs(total - want) <= tol
    ppl = scoring.perplexity(m, [toks], max_length=2048, prefix_token=0)
    assert ppl.tokens == 5000 and ppl.sum_logprob == total and abs(ppl.ppl - math.exp(-total / 5000)) <= 1e-9 * ppl.ppl


@pytest.mark.parametrize("tag", ["w8a8", "w4a8"])
def test_perplexity_within_0_05_of_the_reference_at_22_layers(dev, tag):
    """tests/golden/full_depth_stable_case.npz (the reference's 22-layer model over eight sequences): perplexity() through the fused
    prefill against the perplexity of the reference's recorded NLL, and token_logprobs' argmax against its recorded argmax."""
    from mobilequant_amd import llama, scoring
    from test_gpu_round5 import _stable_model, _stable_reference
    m, z = _stable_model(dev, tag)
    ids_all, ref_nll, ref_arg = _stable_reference(z, tag)
    ref_ppl = float(np.exp(ref_nll.mean()))
    assert llama.fuse_decoder_layer(m) == 22
    S = ids_all.shape[1]
    res = scoring.perplexity(m, [list(map(int, r)) for r in ids_all], max_length=S)
    assert res.tokens == ref_nll.size
    _, _, am = scoring.token_logprobs(m, torch.from_numpy(ids_all).long().to(dev))
    agree = float((am[:, :-1].cpu().numpy() == ref_arg[:, :-1]).mean())
    print(f"[{tag}] perplexity {res.ppl:.5f} vs reference {ref_ppl:.5f} ({res.ppl - ref_ppl:+.5f}) over {res.tokens} tokens; argmax agreement {agree:.4f}")
    assert abs(res.ppl - ref_ppl) <= 0.05
    assert agree >= 0.99
