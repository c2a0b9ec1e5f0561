"""GPU: the W4A16 decode engine -- mq_w4a16_decode_gemv and mq_w4a16_decode_attention (csrc/mq_w4a16_decode.hip) and
WeightOnlyDecodeEngine (decode_weight_only.py) against the float64 oracle of tests/w4a16_decode_ref.py.

GEMV, plain prologue: the exact cases of test_gpu_w4a16.py (integer x, power-of-two scales, random nibbles) equal the oracle bit for bit
under every epilogue (the gated product to the rounding of act(a) * b).  Norm prologues: held to w4a16_ref.bound on rows whose normalised
values all lie clear of an fp16 rounding boundary, so x16 is the oracle's.  Attention: the cache row's bits, every other cache byte,
nothing read above pos, and o within ATTN_TOL.  Engine: logits, prefill + step, cache rows and the device's own module chain within
MODEL_ORDER_FACTOR x MOVEMENT of the oracle; determinism, capture, generate, refusals.

Every tolerance is a multiple of what the REFERENCE arithmetic moves by when it is run in fp32 instead of float64 (w4a16_decode_ref's
emulation), measured on the CPU -- `python tests/test_gpu_w4a16_decode.py` prints the figures below; the code under test is not involved."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import w4a16_decode_ref as D  # noqa: E402
import w4a16_ref as R  # noqa: E402
from w4a16_cases import exact_x  # noqa: E402

pytestmark = pytest.mark.gpu

F16, F32, F64 = np.float16, np.float32, np.float64

MODEL_ORDER_FACTOR = 4.0
ATTN_ORDER_FACTOR = 4.0
# max |o(fp32 emulation of steps 4-6) - o(float64 oracle)| over every attention case of a head_dim (attention_cases below), CPU
ATTN_MOVEMENT = {32: 3.778e-07, 64: 3.145e-07, 128: 3.693e-07, 256: 5.797e-07}
# max |logits(fp32 emulation) - logits(float64 oracle)| over the 24 teacher-forced steps of each model (MODELS below), CPU
MOVEMENT = {"toy": 1.101e-3, "toy96": 1.002e-3, "h256": 1.873e-3, "layernorm": 8.389e-4, "gemma": 5.651e-4}     # at max |logit| 2.79, 3.25, 4.58, 3.19, 3.29
# the smallest top-2 gap of the oracle's logits over the 16 greedy steps of GREEDY_PROMPT on the toy model with 96 tokens, CPU
GREEDY_MIN_GAP = 0.018692             # >= 2 x 4 x 1.002e-3
TOY_CFG = dict(bitwidth=4, group_size=64, is_symmetric=False, is_per_channel=True)
STEPS = 24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- GEMV ------------------------------------------------------------------------------------------------------------------------------
def gemv(dev, x, packed, s16, z16, g, epilogue="bias", n_out=None, **kw):
    from mobilequant_amd import weight_only
    N = packed.shape[0]
    out = torch.full((n_out or (N // 2 if epilogue == "gated" else N),), float("nan"), dtype=torch.float32, device=dev)
    t = {k: (_t(v, dev) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    weight_only.w4a16_decode_gemv(_t(x, dev), _t(packed, dev), _t(s16, dev), _t(z16, dev), out, group_size=g, epilogue=epilogue, **t)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def exact_weights(rng, N, K, g):
    """test_gpu_w4a16.py's: random nibbles, zeros in [-3, 18], scales 2^e with e in [-6, -1] drawn per row and group."""
    gs, G = R.groups(K, g)
    u = rng.integers(0, 16, size=(N, K), dtype=np.uint8)
    z16 = rng.integers(-3, 19, size=(N, G)).astype(F16)
    s16 = (2.0 ** rng.integers(-6, 0, size=(N, G))).astype(F16)
    return u, s16, z16


def gemv_shapes(cus):
    """N x K of 16 x 64, 48 x 128, 256 x 128, 128 x 256 at g 32, 64 and K; more rows than waves in a workgroup; two chunk passes per row;
    group sizes with g / 32 = 3 and 6, the division arm of the group lookup: 2 groups per row, and 3 -- odd, so the half of the scale
    dword a chunk's s16 sits in alternates with the row."""
    out = [(N, K, g) for N, K in ((16, 64), (48, 128), (256, 128), (128, 256)) for g in sorted({32, 64, K})]
    return out + [(16 * cus + 32, 64, 32), (32, 2112, 64), (48, 192, 96), (32, 576, 192)]


def gated_bound(a64, b64, kind):
    """|kernel - oracle| allowed for act(a) * b with a, b exact: fp32 roundings of the chain (exp or erf: 2 ulp each in the device
    library's documentation; the add, the divide or the two products: half an ulp each) -- 4 ulp of the result; the erf form adds the
    absolute error of 1 + erf(a / sqrt 2) where that sum cancels (3 2^-24: erf at +-1, the add, the rounded argument) times |a b| / 2.
    SiLU as the contract writes it, a / (1 + exp(-a)) in fp32, is -0 once exp(-a) leaves the fp32 range (a < -88.7), where the true
    value is at most 88.8 e^-88.7 = 2.7e-37 < 2^-120 in magnitude: that much times |b| is allowed on top (the exact cases reach
    |a| of several hundred)."""
    want = D.gated(a64, b64, kind)
    tol = 4.0 * D.ulp32(want)
    if kind == "gelu":
        tol = tol + 4.0 * 2.0 ** -24 * np.abs(0.5 * a64 * b64)
    else:
        tol = tol + 2.0 ** -120 * np.abs(b64)
    return want, tol


def test_gemv_plain_prologue_is_exact_under_every_epilogue(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for N, K, g in gemv_shapes(cus):
        rng = np.random.default_rng(N * 1009 + K + g)
        u, s16, z16 = exact_weights(rng, N, K, g)
        packed, w16 = R.pack(u), R.w16(u, s16, z16, g)
        x = exact_x(rng, 1, K)[0]
        y64 = R.linear64(x[None], w16)[0][0]
        what = f"N={N} K={K} g={g}"
        assert np.array_equal(y64.astype(F32).astype(F64), y64)                                   # the case IS exact
        bias = (rng.integers(-40, 41, size=N) / 64.0).astype(F32)
        resid = rng.integers(-8, 9, size=N).astype(F32)
        for b in (None, bias):
            want = (y64 + (0 if b is None else b.astype(F64))).astype(F32)
            got = gemv(dev, x, packed, s16, z16, g, bias=b)
            assert np.array_equal(bits(got), bits(want)), (what, "bias", b is not None, np.flatnonzero(bits(got) != bits(want))[:8])
            want = (resid.astype(F64) + y64 + (0 if b is None else b.astype(F64))).astype(F32)
            got = gemv(dev, x, packed, s16, z16, g, epilogue="resid", resid=resid, bias=b)
            assert np.array_equal(bits(got), bits(want)), (what, "resid", b is not None, np.flatnonzero(bits(got) != bits(want))[:8])
        if N % 32 == 0:
            for kind in ("silu", "gelu"):
                want, tol = gated_bound(y64[0::2], y64[1::2], kind)
                got = gemv(dev, x, packed, s16, z16, g, epilogue="gated", act=kind)
                err = np.abs(got.astype(F64) - want)
                assert np.all(err <= tol), (what, kind, float((err / tol).max()), int(np.argmax(err / tol)))


NORM_ROWS = [(128, 0, 1.0), (256, 1, 1.0), (128, 2, 1e-3), (256, 4, 1e-3)]          # K, seed, magnitude (1e-3: eps decides the result)


def norm_case(K, seed, mag, kind):
    rng = np.random.default_rng([K, seed, 0 if kind == "rmsnorm" else 1])
    x = (rng.standard_normal(K) * mag).astype(F32)
    nw = (1.0 + 0.25 * rng.standard_normal(K)).astype(F32)
    nb = (0.1 * rng.standard_normal(K)).astype(F32) if kind == "layernorm" else None
    return x, nw, nb, 1e-5


def norm_case_seed(K, seed, mag, kind):
    """The first seed from `seed` on whose normalised row lies clear of every fp16 rounding boundary (about three in four do)."""
    for s in range(seed, seed + 64):
        x, nw, nb, eps = norm_case(K, s, mag, kind)
        if D.fp16_boundary_distance(D.norm(x, kind, nw, nb, eps)).min() > 8.0:
            return s
    raise AssertionError("no clear seed")


# seeds chosen on the CPU (norm_case_seed; `python tests/test_gpu_w4a16_decode.py` prints them): (K, magnitude, kind) -> seed
NORM_SEEDS = {(128, 1.0, "rmsnorm"): 0, (128, 1.0, "layernorm"): 0, (256, 1.0, "rmsnorm"): 3, (256, 1.0, "layernorm"): 1,
              (128, 1e-3, "rmsnorm"): 2, (128, 1e-3, "layernorm"): 2, (256, 1e-3, "rmsnorm"): 4, (256, 1e-3, "layernorm"): 4}


@pytest.mark.parametrize("kind", ["rmsnorm", "layernorm"])
def test_gemv_norm_prologues_within_the_linear_bound(dev, kind):
    for K, _, mag in NORM_ROWS:
        seed = NORM_SEEDS[(K, mag, kind)]
        x, nw, nb, eps = norm_case(K, seed, mag, kind)
        y64 = D.norm(x, kind, nw, nb, eps)
        assert int((D.fp16_boundary_distance(y64) <= 8.0).sum()) == 0            # x16 is unambiguous: no element near a rounding boundary
        N, g = 48, 64
        rng = np.random.default_rng(K + seed)
        w = rng.standard_normal((N, K)).astype(F32)
        s, o = R.grid_from_minmax(w, False, g)
        u, s16, z16 = R.stored(w, s, o, False, g)
        bias = rng.standard_normal(N).astype(F32)
        want, sumabs = R.linear64(y64[None], R.w16(u, s16, z16, g), bias)
        got = gemv(dev, x, R.pack(u), s16, z16, g, prologue=kind, norm_weight=nw, norm_bias=nb, eps=eps, bias=bias)
        err = np.abs(got.astype(F64) - want[0])
        tol = R.bound(K, sumabs[0], want[0], F32)
        print(f"norm prologue {kind} K={K} mag={mag}: max err / bound = {float((err / tol).max()):.3f}")
        assert np.all(err <= tol), (kind, K, mag, float((err / tol).max()))
        if mag < 1.0:                                                             # eps decides: without it the row would be O(1) after the norm
            assert np.abs(y64).max() < 0.5 * np.abs(D.norm(x, kind, nw, nb, 1e-12)).max()


# ---- attention -------------------------------------------------------------------------------------------------------------------------
T_CACHE, KV_HEADS = 96, 2
ATTN_POS = (0, 1, 31, 32, 33, 63, 64, 65, 95)
ATTN_SPLITS = (1, 2, 7)                                       # 7 divides no pos + 1 of ATTN_POS
ATTN_PARAMS = [(Dh, rep, pct) for Dh in (32, 64, 128, 256) for rep in (1, 2, 8) for pct in (1.0, 0.25)]


def attention_case(Dh, rep, pct, pos):
    """qkv row, caches (positions < pos Gaussian, the rest NaN) and the RoPE row, as numpy fp32."""
    H, KV, rot = KV_HEADS * rep, KV_HEADS, int(pct * Dh)
    rng = np.random.default_rng([Dh, rep, rot, pos])
    qkv = rng.standard_normal((H + 2 * KV) * Dh).astype(F32)
    kc = np.full((KV, T_CACHE, Dh), np.nan, F32)
    vc = np.full((KV, T_CACHE, Dh), np.nan, F32)
    kc[:, :pos] = rng.standard_normal((KV, pos, Dh))
    vc[:, :pos] = rng.standard_normal((KV, pos, Dh))
    inv = 1.0 / (10000.0 ** (np.arange(0, rot, 2, dtype=F32) / F32(rot)))
    ang = np.concatenate([pos * inv, pos * inv]).astype(F32)
    return H, KV, rot, qkv, kc, vc, np.cos(ang).astype(F32), np.sin(ang).astype(F32)


def attention_ref(H, KV, Dh, qkv, kc, vc, cos, sin, pos, dt):
    q = D.rope(qkv[:H * Dh].reshape(H, Dh), cos, sin, dt)
    k = np.concatenate([np.asarray(kc[:, :pos], dt), D.rope(qkv[H * Dh:(H + KV) * Dh].reshape(KV, Dh), cos, sin, dt)[:, None]], axis=1)
    v = np.concatenate([np.asarray(vc[:, :pos], dt), np.asarray(qkv[(H + KV) * Dh:], dt).reshape(KV, 1, Dh)], axis=1)
    return D.attention(q, k, v, dt)


def measure_attention_movement():
    out = {}
    for Dh, rep, pct in ATTN_PARAMS:
        for pos in ATTN_POS:
            H, KV, rot, qkv, kc, vc, cos, sin = attention_case(Dh, rep, pct, pos)
            d = np.abs(attention_ref(H, KV, Dh, qkv, kc, vc, cos, sin, pos, F32).astype(F64) - attention_ref(H, KV, Dh, qkv, kc, vc, cos, sin, pos, F64)).max()
            out[Dh] = max(out.get(Dh, 0.0), float(d))
    return out


@pytest.mark.parametrize("Dh,rep,pct", ATTN_PARAMS)
def test_attention_appends_one_row_and_matches_the_oracle(dev, Dh, rep, pct):
    from mobilequant_amd import weight_only
    from mobilequant_amd.llama import apply_rope
    tol = ATTN_ORDER_FACTOR * ATTN_MOVEMENT[Dh]
    assert tol > 0
    GUARD = 2 * Dh
    worst = 0.0
    for pos in ATTN_POS:
        H, KV, rot, qkv, kc, vc, cos, sin = attention_case(Dh, rep, pct, pos)
        want = attention_ref(H, KV, Dh, qkv, kc, vc, cos, sin, pos, F64)
        k_row = apply_rope(torch.from_numpy(qkv[H * Dh:(H + KV) * Dh].reshape(1, KV, 1, Dh)), torch.from_numpy(cos)[None], torch.from_numpy(sin)[None])
        k_row, v_row = k_row.numpy().reshape(KV, Dh), qkv[(H + KV) * Dh:].reshape(KV, Dh)
        for ns in ATTN_SPLITS:
            bufs = []
            for c in (kc, vc):                                                       # guard rows around each cache
                b = torch.full((c.size + 2 * GUARD,), 12345.0, dtype=torch.float32, device=dev)
                b[GUARD:GUARD + c.size] = _t(c.reshape(-1), dev)
                bufs.append(b)
            out = torch.full((H * Dh,), float("nan"), dtype=torch.float32, device=dev)
            part = torch.full((H * ns * (Dh + 4),), float("nan"), dtype=torch.float32, device=dev) if ns > 1 else None
            ticket = torch.zeros(H, dtype=torch.int32, device=dev) if ns > 1 else None
            weight_only.w4a16_decode_attention(_t(qkv, dev), bufs[0][GUARD:GUARD + kc.size], bufs[1][GUARD:GUARD + vc.size], _t(np.concatenate([cos, sin]), dev),
                                               torch.tensor([pos], dtype=torch.int32, device=dev), out, heads=H, kv_heads=KV, head_dim=Dh, rot_dim=rot,
                                               nsplit=ns, part=part, ticket=ticket)
            torch.cuda.synchronize()
            what = f"D={Dh} rep={rep} rot={rot} pos={pos} nsplit={ns}"
            for b, c, row in ((bufs[0], kc, k_row), (bufs[1], vc, v_row)):
                exp = np.full(c.size + 2 * GUARD, 12345.0, F32)
                e = c.copy()
                e[:, pos] = row                                                      # the one row written, with apply_rope's bits (v: as given)
                exp[GUARD:GUARD + c.size] = e.reshape(-1)
                assert np.array_equal(bits(b.cpu().numpy()), bits(exp)), what     # every other byte untouched, NaN payloads included
            got = out.cpu().numpy().reshape(H, Dh)
            assert np.isfinite(got).all(), what                                      # nothing above pos was read
            if ticket is not None:
                assert not ticket.any(), what                                        # left ready for the next launch
            worst = max(worst, float(np.abs(got.astype(F64) - want).max()))
            assert np.abs(got.astype(F64) - want).max() <= tol, (what, float(np.abs(got.astype(F64) - want).max()), tol)
    print(f"attention D={Dh} rep={rep} pct={pct}: max err {worst:.3e} of {tol:.3e}")


def test_attention_outside_the_cache_does_nothing(dev):
    from mobilequant_amd import weight_only
    H, KV, rot, qkv, kc, vc, cos, sin = attention_case(64, 2, 1.0, 5)
    for pos in (-1, T_CACHE):
        k, v = _t(kc.reshape(-1), dev), _t(vc.reshape(-1), dev)
        out = torch.full((H * 64,), 7.0, dtype=torch.float32, device=dev)
        weight_only.w4a16_decode_attention(_t(qkv, dev), k, v, _t(np.concatenate([cos, sin]), dev), torch.tensor([pos], dtype=torch.int32, device=dev), out,
                                           heads=H, kv_heads=KV, head_dim=64, rot_dim=rot)
        torch.cuda.synchronize()
        assert np.array_equal(bits(k.cpu().numpy()), bits(kc.reshape(-1))) and np.array_equal(bits(v.cpu().numpy()), bits(vc.reshape(-1)))
        assert bool((out == 7.0).all())


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
def model_shape(name):
    from mobilequant_amd.llama import LlamaShape
    if name == "toy":
        return LlamaShape.toy()
    if name == "toy96":                                              # generate: mq_sample takes vocabularies that are multiples of 4
        return LlamaShape.toy(vocab=96)
    if name == "h256":
        return LlamaShape.toy(hidden=256, heads=4, kv_heads=1, head_dim=64, ffn=512)
    if name == "layernorm":
        return LlamaShape.toy(norm="layernorm", qkv_bias=True, rotary_pct=0.25)
    return LlamaShape.toy(heads=2, kv_heads=1, head_dim=256, hidden_act="gelu", embed_scale=True, eps=1e-6)


MODELS = ("toy", "h256", "layernorm", "gemma")
SEEDS = {"toy": 0, "h256": 1, "layernorm": 2, "gemma": 3, "toy96": 0}
GREEDY_PROMPT = (5, 17, 42, 7, 90, 3, 61, 28)
GREEDY_NEW = 16


def float_model(name):
    from mobilequant_amd.llama import LlamaForCausalLM
    m = LlamaForCausalLM(model_shape(name)).eval()
    m.reset_parameters(0.08, seed=SEEDS[name])
    return m


def model_ids(name):
    return np.random.default_rng(100 + SEEDS[name]).integers(0, model_shape(name).vocab, size=STEPS)


class Setup:
    """One model on the device with its oracle results, computed once and shared (read-only)."""

    def __init__(self, name, dev):
        import mobilequant_amd.quantization.qmodule as Q
        from mobilequant_amd import WeightOnlyDecodeEngine
        self.name, self.ids = name, model_ids(name)
        self.model = Q.create_weight_only_qmodel(float_model(name).to(dev), Q.QuantConfig(**TOY_CFG))
        self.chain = D.Chain.from_packed(self.model)
        ref = D.Chain.from_float(float_model(name), TOY_CFG["group_size"])
        # (the device packer made the oracle's weights: MOVEMENT, measured on the oracle's own quantisation, is this chain's)
        self.weights_differ = [(i, key) for i, (a, b) in enumerate(zip(self.chain.layers, ref.layers)) for key in ("q", "k", "v", "o", "w1", "w2", "w3")
                               if not np.array_equal(a[key][0].view(np.uint16), b[key][0].view(np.uint16))]
        self.want, self.want_cache = self.chain.run(self.ids, F64)
        self.tol = MODEL_ORDER_FACTOR * MOVEMENT[name]
        assert self.tol > 0
        self.engine = WeightOnlyDecodeEngine(self.model, cache_len=STEPS)
        self.got = self.teacher_forced(self.engine)

    def teacher_forced(self, eng):
        eng.reset()
        rows = [eng.step(int(t)).clone() for t in self.ids]
        torch.cuda.synchronize()
        return torch.stack(rows).cpu().numpy()


_SETUPS = {}


@pytest.fixture()
def setup(request, dev):
    name = request.param
    if name not in _SETUPS:
        _SETUPS[name] = Setup(name, dev)
    return _SETUPS[name]


by_model = pytest.mark.parametrize("setup", MODELS, indirect=True)


@by_model
def test_engine_logits_match_the_oracle(setup):
    err = np.abs(setup.got.astype(F64) - setup.want).max()
    print(f"{setup.name}: engine max |logit error| {err:.3e} of {setup.tol:.3e} (max |logit| {np.abs(setup.want).max():.2f})")
    assert err <= setup.tol
    assert not setup.weights_differ, setup.weights_differ
    assert setup.engine.launches_per_token <= 5 * len(setup.model.layers) + 2
    assert setup.engine.position() == STEPS


@by_model
def test_engine_cache_and_module_chain_are_the_same_model(setup, dev):
    """The device's own module chain sits inside the bound too, and the engine's cache rows are within it of the chain's."""
    m = setup.model
    cache = m.new_cache(1, STEPS)
    with torch.no_grad():
        rows = [m(torch.tensor([[int(t)]], device=dev), cache=cache, pos=p)[0, 0] for p, t in enumerate(setup.ids)]
    chain_logits = torch.stack(rows).cpu().numpy()
    assert np.abs(chain_logits.astype(F64) - setup.want).max() <= setup.tol
    eng = setup.engine
    setup.teacher_forced(eng)
    for li in range(len(m.layers)):
        for mine, theirs, want in ((eng.cached_keys(li, STEPS), cache[li][0][0], setup.want_cache[li][0]), (eng.cached_values(li, STEPS), cache[li][1][0], setup.want_cache[li][1])):
            assert (mine - theirs).abs().max().item() <= setup.tol
            assert np.abs(mine.cpu().numpy().astype(F64) - want).max() <= setup.tol


@by_model
@pytest.mark.parametrize("n", [1, 7, 23])
def test_prefill_then_step_lands_in_the_bound(setup, n):
    eng = setup.engine
    eng.reset()
    first = eng.prefill(setup.ids[:n]).cpu().numpy()
    assert eng.position() == n and np.abs(first.astype(F64) - setup.want[n - 1]).max() <= setup.tol
    got = eng.step(int(setup.ids[n])).cpu().numpy()
    assert np.abs(got.astype(F64) - setup.want[n]).max() <= setup.tol


@by_model
def test_determinism_capture_and_the_last_position(setup, dev):
    from mobilequant_amd import WeightOnlyDecodeEngine
    eng = setup.engine
    again = setup.teacher_forced(eng)
    assert np.array_equal(bits(again), bits(setup.got))                              # the same steps, the same bits
    with pytest.raises(RuntimeError, match="KV cache is full"):
        eng.step(1)                                                                  # position 23 was the last
    cap = WeightOnlyDecodeEngine(setup.model, cache_len=STEPS).capture()
    replayed = setup.teacher_forced(cap)                                             # ONE graph, positions 0 .. cache_len - 1
    assert np.array_equal(bits(replayed), bits(setup.got))
    with pytest.raises(RuntimeError, match="KV cache is full"):
        cap.step(1)
    for ns in (2, 3):                                                                # split attention: inside the bound, deterministic, capturable
        sp = WeightOnlyDecodeEngine(setup.model, cache_len=STEPS, attn_splits=ns)
        a = setup.teacher_forced(sp)
        assert np.abs(a.astype(F64) - setup.want).max() <= setup.tol
        assert np.array_equal(bits(setup.teacher_forced(sp)), bits(a)) and np.array_equal(bits(setup.teacher_forced(sp.capture())), bits(a))


@pytest.mark.parametrize("setup", ["toy96"], indirect=True)
def test_generate(setup, dev):
    from mobilequant_amd import WeightOnlyDecodeEngine, sampling
    from mobilequant_amd.sampling import SamplingParams
    want, gap = setup.chain.greedy(GREEDY_PROMPT, GREEDY_NEW)
    assert gap >= 2.0 * setup.tol and abs(gap - GREEDY_MIN_GAP) < 1e-6, (gap, setup.tol)   # no step of the oracle is close enough to flip
    eng = WeightOnlyDecodeEngine(setup.model, cache_len=64)
    assert eng.generate(GREEDY_PROMPT, GREEDY_NEW) == want
    assert eng.generate(GREEDY_PROMPT, GREEDY_NEW, eos_token_id=want[len(GREEDY_PROMPT) + 2]) == want[:len(GREEDY_PROMPT) + 3]
    assert eng.generate(GREEDY_PROMPT, GREEDY_NEW, eos_token_id=[want[-1], 1000]) == want[:want.index(want[-1], len(GREEDY_PROMPT)) + 1]
    # sampled: the tokens of mq_sample called by hand on each step's logits with the same (seed, stream, n)
    req, stream = SamplingParams(temperature=0.9, top_k=20, top_p=0.95, seed=1234), 3
    eng.reset()
    eng.prefill(GREEDY_PROMPT)
    by_hand, tok = list(GREEDY_PROMPT), torch.zeros(1, dtype=torch.int64, device=dev)
    for i in range(GREEDY_NEW):
        n = len(by_hand)
        sampling.sample(eng.logits.view(1, -1), torch.tensor([n], dtype=torch.int32, device=dev), ([req], [stream]), tok, cache_len=64)
        by_hand.append(int(tok.item()))
        if i < GREEDY_NEW - 1:
            eng.step(by_hand[-1])
    assert by_hand != want and len(set(by_hand[len(GREEDY_PROMPT):])) > 4
    assert eng.generate(GREEDY_PROMPT, GREEDY_NEW, sampling=req, stream=stream) == by_hand
    assert eng.generate(GREEDY_PROMPT, GREEDY_NEW, sampling=req, stream=stream + 1) != by_hand
    eng.capture()
    assert eng.generate(GREEDY_PROMPT, GREEDY_NEW, sampling=req, stream=stream) == by_hand
    assert eng.generate(GREEDY_PROMPT, GREEDY_NEW) == want
    for bad in (SamplingParams(temperature=0.9, repetition_penalty=1.3), SamplingParams(temperature=0.9, logit_bias={3: 1.0})):
        with pytest.raises(NotImplementedError, match="penalised request"):
            eng.generate(GREEDY_PROMPT, 4, sampling=bad)


def test_refusals_and_coverage(dev):
    import mobilequant_amd.quantization.qmodule as Q
    from mobilequant_amd import WeightOnlyDecodeEngine
    with pytest.raises(ValueError, match=r"layers\.0\.self_attn\.q_proj: Linear is not a WeightOnlyLinear"):
        WeightOnlyDecodeEngine(float_model("toy").to(dev))
    sim = Q.create_sim_qmodel(float_model("toy").to(dev), Q.QuantConfig(bitwidth=4, is_per_channel=True), Q.QuantConfig(bitwidth=8))
    with pytest.raises(ValueError, match="QLinear is not a WeightOnlyLinear"):
        WeightOnlyDecodeEngine(sim)
    m = Q.create_weight_only_qmodel(float_model("toy").to(dev), Q.QuantConfig(**TOY_CFG))
    with pytest.raises(ValueError, match=r"cache_len: 129 outside 1 \.\. max_pos = 128"):
        WeightOnlyDecodeEngine(m, cache_len=129)
    eng = WeightOnlyDecodeEngine(m)
    eng.step(3)
    cov = Q.int8_coverage(m)
    assert len(cov["w4a16_modules"]) == 14 and "layers.1.mlp.w2" in cov["w4a16_modules"]


if __name__ == "__main__":
    print("ATTN_MOVEMENT =", {k: float("%.3e" % v) for k, v in measure_attention_movement().items()})
    mv = {}
    for name in MODELS + ("toy96",):
        chain = D.Chain.from_float(float_model(name), TOY_CFG["group_size"])
        w64, _ = chain.run(model_ids(name), F64)
        w32, _ = chain.run(model_ids(name), F32)
        mv[name] = float("%.3e" % np.abs(w32.astype(F64) - w64).max())
        print(f"  {name}: max |logit| {np.abs(w64).max():.2f}")
    print("MOVEMENT =", mv)
    ids, gap = D.Chain.from_float(float_model("toy96"), TOY_CFG["group_size"]).greedy(GREEDY_PROMPT, GREEDY_NEW)
    print("GREEDY_MIN_GAP = %.6f  (needs >= %.3e); ids %s" % (gap, 2 * MODEL_ORDER_FACTOR * mv["toy96"], ids))
    print("NORM_SEEDS =", {(K, mag, kind): norm_case_seed(K, seed, mag, kind) for K, seed, mag in NORM_ROWS for kind in ("rmsnorm", "layernorm")})
