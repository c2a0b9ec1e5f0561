"""GPU: the batched decode step (csrc/mq_decode_batch.hip, mobilequant_amd/decode_batch.py).

The contract is per sequence: slot b of a BatchDecodeEngine step computes what DecodeEngine computes for that sequence alone, so the
single-sequence engine -- pinned to the module graph and the oracle by the other decode tests -- is the oracle here, and the bar is
bit identity: every step's logits row and, at the end, every slot's key / value cache.  One captured graph serves every mix of slot
positions; prompts of 1 .. 768 tokens put the slots on both sides of the 64-position blocks and of the split threshold (768) at once.
Kernel level: each batched launch against the single-sequence launch it generalises, row by row, in every mode the entries serve,
up to the B * K limits."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

GEOMS = {
    # TinyLlama geometry (head_dim 64, GQA 32 / 4), reduced hidden / ffn / vocab
    "llama": dict(hidden=256, heads=32, kv_heads=4, head_dim=64, ffn=512, vocab=160),
    # StableLM-2: LayerNorm, q|k|v bias, 25 % rotary, MHA
    "stablelm": dict(hidden=256, heads=4, kv_heads=4, head_dim=64, ffn=512, vocab=96, norm="layernorm", qkv_bias=True, rotary_pct=0.25),
    # Gemma: head_dim 256, MQA, GELU, embed scale
    "gemma": dict(hidden=256, heads=2, kv_heads=1, head_dim=256, ffn=512, vocab=128, hidden_act="gelu", embed_scale=True, eps=1e-6),
}
CACHE = 848                                       # 768 + 64 steps fit; a multiple of 16 (the single engine's four-launch chain)
PROMPT_LENS = [1, 7, 63, 64, 65, 300, 767, 768]
STEPS = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(dev, geom, layers, wbits, seed=11):
    """A random model through the reference's surgery and the mixed-precision recipe of the other decode tests."""
    import mobilequant_amd as mq
    from mobilequant_amd.calibration import get_act_range
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    shape = LlamaShape(layers=layers, max_pos=1024, **GEOMS[geom])
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
    return m


def _prompts(vocab, lens, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g).tolist() for n in lens]


def _single_run(eng, prompt, steps):
    """One sequence alone through DecodeEngine, greedy: (tokens fed per step, logits after each of them, final caches)."""
    eng.reset()
    if len(prompt) == 1:
        eng.step(prompt[0])
        feed, logits = [prompt[0]], [eng.logits.clone()]
    else:
        eng.prefill(prompt)
        feed, logits = [], []
    while len(feed) < steps:                                    # feed[k] -> logits[k]
        nxt = int(torch.argmax(eng.logits))
        feed.append(nxt)
        eng.step(nxt)
        logits.append(eng.logits.clone())
    n = eng._host_pos
    caches = [(eng.k_cache[li][:, :n].clone(), eng.cached_values(li, n).clone()) for li in range(len(eng.k_cache))]
    return feed, logits, caches


def _start_slot(be, b, prompt):
    if len(prompt) == 1:
        be.start(b)
    else:
        be.prefill(b, prompt)


def _check_identity(m, prompts, refs, B, capture=True):
    """B slots, prompts[b] in slot b, STEPS steps from ONE captured graph: logits rows and caches equal the single runs."""
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    be = BatchDecodeEngine(m, B, cache_len=CACHE)
    for b in range(B):
        _start_slot(be, b, prompts[b])
    if capture:
        be.capture()
    for k in range(STEPS):
        out = be.step([refs[b][0][k] for b in range(B)])
        for b in range(B):
            want = refs[b][1][k]
            assert torch.equal(out[b], want), (B, b, len(prompts[b]), k, float((out[b] - want).abs().max()))
    for b in range(B):
        for li, (kc, vc) in enumerate(refs[b][2]):
            n = kc.shape[1]
            assert be.position(b) == n
            assert torch.equal(be.cached_keys(b, li), kc) and torch.equal(be.cached_values(b, li), vc), (B, b, li)
    return be


@pytest.mark.parametrize("wbits", [8, 4], ids=["w8a8", "w4a8"])
@pytest.mark.parametrize("geom,layers", [("llama", 1), ("llama", 2), ("stablelm", 2), ("gemma", 1), ("gemma", 2)])
def test_every_slot_is_the_single_engine_bit_for_bit(dev, geom, layers, wbits):
    from mobilequant_amd.decode import DecodeEngine
    m = _model(dev, geom, layers, wbits)
    prompts = _prompts(m.shape.vocab, PROMPT_LENS)
    single = DecodeEngine(m, cache_len=CACHE)
    refs = [_single_run(single, p, STEPS) for p in prompts]
    for B, pick in ((1, [6]), (3, [0, 3, 7]), (8, list(range(8)))):
        _check_identity(m, [prompts[i] for i in pick], [refs[i] for i in pick], B)


@pytest.mark.parametrize("tag", ["w8a8", "w4a8"])
def test_full_size_tinyllama_eight_slots_bit_for_bit(dev, tag):
    """22-layer TinyLlama geometry (hidden 2048, FFN 5632), B = 8, 32 steps from one captured graph, against eight single runs."""
    import dataclasses
    from test_gpu_round5 import _stable_model
    from mobilequant_amd import llama
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m, z = _stable_model(dev, tag)
    cl = 320
    cos, sin = llama.rope_tables(dataclasses.replace(m.shape, max_pos=cl))
    m.cos, m.sin = cos.to(dev), sin.to(dev)
    ids = np.concatenate([z["ids"][None], z["ids_more"]])
    lens = [1, 9, 63, 64, 65, 130, 200, 250]
    prompts = [ids[i % ids.shape[0], :n].tolist() for i, n in enumerate(lens)]
    single = DecodeEngine(m, cache_len=cl)
    steps = 32
    refs = [_single_run(single, p, steps) for p in prompts]
    be = BatchDecodeEngine(m, 8, cache_len=cl)
    for b in range(8):
        _start_slot(be, b, prompts[b])
    be.capture()
    for k in range(steps):
        out = be.step([refs[b][0][k] for b in range(8)])
        for b in range(8):
            assert torch.equal(out[b], refs[b][1][k]), (tag, b, k, float((out[b] - refs[b][1][k]).abs().max()))
    for b in range(8):
        for li in (0, 10, 21):
            kc, vc = refs[b][2][li]
            assert torch.equal(be.cached_keys(b, li), kc) and torch.equal(be.cached_values(b, li), vc), (tag, b, li)


def test_continuous_batching_swaps_a_slot_without_disturbing_the_others(dev):
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _model(dev, "llama", 2, 8)
    V = m.shape.vocab
    prompts = _prompts(V, [40, 100, 70, 20], seed=9)
    newp = _prompts(V, [55], seed=10)[0]
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, V, (30, 4), generator=g).tolist()
    runs = {}
    for swap in (False, True):
        be = BatchDecodeEngine(m, 4, cache_len=160)
        for b in range(4):
            be.prefill(b, prompts[b])
        be.capture()
        rows, idle_k = [], None
        for k in range(30):
            if k == 5:
                be.release(3)                                  # slot 3 goes idle: its bytes and its logits row freeze
                idle_k = ([c[3].clone() for c in be.k_cache], [c[3].clone() for c in be.v_cache], be.logits[3].clone())
            if swap and k == 10:
                be.release(1)
                be.prefill(1, newp)
            out = be.step(toks[k]).clone()
            rows.append(out)
            if idle_k is not None:
                assert torch.equal(out[3], idle_k[2])
                assert all(torch.equal(c[3], c0) for c, c0 in zip(be.k_cache, idle_k[0]))
                assert all(torch.equal(c[3], c0) for c, c0 in zip(be.v_cache, idle_k[1]))
        runs[swap] = (torch.stack(rows), [c.clone() for c in be.k_cache], [c.clone() for c in be.v_cache], be)
    a, b_ = runs[False], runs[True]
    for s in (0, 2):                                           # the other slots do not notice the swap
        assert torch.equal(a[0][:, s], b_[0][:, s]), s
        assert all(torch.equal(x[s], y[s]) for x, y in zip(a[1], b_[1])) and all(torch.equal(x[s], y[s]) for x, y in zip(a[2], b_[2]))
    # slot 1's new sequence is a fresh single-engine run fed the same tokens
    single = DecodeEngine(m, cache_len=160)
    single.reset()
    single.prefill(newp)
    for k in range(10, 30):
        assert torch.equal(b_[0][k, 1], single.step(toks[k][1])), k
    be = b_[3]
    n = be.position(1)
    assert n == len(newp) + 20
    for li in range(2):
        assert torch.equal(be.cached_keys(1, li), single.k_cache[li][:, :n]) and torch.equal(be.cached_values(1, li), single.cached_values(li, n))


def test_a_full_slot_raises_and_release_leaves_the_others_running(dev):
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _model(dev, "llama", 1, 8)
    p0, p1 = _prompts(m.shape.vocab, [30, 60], seed=4)
    be = BatchDecodeEngine(m, 2, cache_len=64)
    be.prefill(0, p0)
    be.prefill(1, p1)
    be.capture()
    single = DecodeEngine(m, cache_len=64, launches=5)
    single.reset()
    single.prefill(p0)
    for k in range(4):
        out = be.step([k + 1, k + 2])
        assert torch.equal(out[0], single.step(k + 1))
    assert be.position(1) == 64
    with pytest.raises(RuntimeError, match="slot 1's KV cache is full"):
        be.step([5, 6])
    frozen = [c[1].clone() for c in be.k_cache + be.v_cache]
    be.release(1)
    for k in range(4, 10):
        out = be.step([k + 1, 0])
        assert torch.equal(out[0], single.step(k + 1)), k
    assert all(torch.equal(c[1], f) for c, f in zip(be.k_cache + be.v_cache, frozen))
    # generate releases a slot that reaches the cache end and keeps serving the other one
    outs = be.generate([p1, p0], max_new_tokens=10)
    assert len(outs[0]) == 65 and len(outs[1]) == len(p0) + 10          # 60 + 4 cached positions, then the fifth token ends it
    assert outs[1] == DecodeEngine(m, cache_len=64, launches=5).generate(p0, 10)


@pytest.mark.parametrize("geom", ["llama", "gemma"])
def test_generate_greedy_is_the_single_engine_per_prompt_and_sampling_is_reproducible(dev, geom):
    from mobilequant_amd.decode import DecodeEngine
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _model(dev, geom, 2, 8)
    prompts = _prompts(m.shape.vocab, [1, 5, 17, 64, 65, 120, 9, 33], seed=12)
    be = BatchDecodeEngine(m, 8, cache_len=256)
    be.capture()
    got = be.generate(prompts, max_new_tokens=24)
    single = DecodeEngine(m, cache_len=256)
    for p, o in zip(prompts, got):
        assert o == single.generate(p, 24), len(p)
    eos = got[2][len(prompts[2]) + 3]                          # a token one sequence meets early: that one stops there
    got_eos = be.generate(prompts, max_new_tokens=24, eos_token_id=eos)
    for p, o in zip(prompts, got_eos):
        assert o == single.generate(p, 24, eos_token_id=eos), len(p)
    s1 = be.generate(prompts, 16, do_sample=True, temperature=0.7, generator=torch.Generator(device=dev).manual_seed(7))
    s2 = be.generate(prompts, 16, do_sample=True, temperature=0.7, generator=torch.Generator(device=dev).manual_seed(7))
    assert s1 == s2 and all(len(o) == len(p) + 16 for o, p in zip(s1, prompts))


# ---- kernel level: each batched launch against the single-sequence launch, row by row --------------------------------------------------
def _call(name, *args):
    from mobilequant_amd import _lib
    _lib.call(name, *args)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _clone_struct(s):
    c = type(s)()
    ctypes.pointer(c)[0] = s
    return c


def _gemv_rows(ba, B, N_out, y_len, x_len, fp32_in, dev, gen, keep):
    """Fresh inputs for ba's rows (x fp32 or xq int8, resid), the batched launch, then B single launches on the same inputs."""
    g = ba.g
    gate = bool(g.gate_q)
    if fp32_in:
        x = (torch.randn(B, x_len, generator=gen) * 3).to(dev)
        g.x, g.xq, ba.x_stride = x.data_ptr(), None, x_len
    else:
        x = torch.randint(-128, 128, (B, x_len), generator=gen, dtype=torch.int8).to(dev)
        g.xq, g.x, ba.x_stride = x.data_ptr(), None, x_len
    keep.append(x)
    res = (torch.randn(B, y_len, generator=gen) * 2).to(dev) if (not gate and g.resid) else None
    outs = {}
    for mode in ("batch", "single"):
        y = torch.full((B, y_len), -7777.0, device=dev)
        gq = torch.full((B, N_out), 85, dtype=torch.int8, device=dev)
        r = res.clone() if res is not None else None
        if r is not None:
            g.resid = r.data_ptr()
            g.y = r.data_ptr()                                  # in place, as the engine's o_proj / w2 launches
        else:
            g.y = y.data_ptr() if (not gate or g.y) else None
        if gate:
            g.gate_q = gq.data_ptr()
        ba.y_stride, ba.gate_stride = y_len, N_out
        if mode == "batch":
            _call("mq_decode_gemv_batch", ctypes.byref(ba), _st())
        else:
            for b in range(B):
                s = _clone_struct(g)
                s.x = (g.x + 4 * b * x_len) if g.x else None
                s.xq = (g.xq + b * x_len) if g.xq else None
                if r is not None:
                    s.resid = s.y = g.resid + 4 * b * y_len
                elif g.y:
                    s.y = g.y + 4 * b * y_len
                if gate:
                    s.gate_q = g.gate_q + b * N_out
                _call("mq_decode_gemv", ctypes.byref(s), _st())
        torch.cuda.synchronize()
        outs[mode] = ((r if r is not None else y).clone(), gq.clone())
    return outs


def _assert_same(outs, what):
    (yb, qb), (ys, qs) = outs["batch"], outs["single"]
    assert torch.equal(yb.view(torch.int32), ys.view(torch.int32)), (what, int((yb.view(torch.int32) != ys.view(torch.int32)).sum()))
    assert torch.equal(qb, qs), (what, int((qb != qs).sum()))


def _random_linear(ba, K, N, w4, gen, dev, keep, norm=None):
    """Replace ba's weights / epilogue vectors with random ones of shape N x K (grids and consts stay the record's)."""
    g = ba.g
    wb = K // 2 if w4 else K
    w = torch.randint(-128, 128, (N, wb), generator=gen, dtype=torch.int8).to(dev)
    alpha = (torch.rand(N, generator=gen) * 1e-3 + 1e-4).to(dev)
    zp = torch.randint(-3, 4, (N,), generator=gen, dtype=torch.int32).to(dev)
    ct = torch.randint(-5000, 5000, (N,), generator=gen, dtype=torch.int32).to(dev)
    keep += [w, alpha, zp, ct]
    g.K, g.N, g.w, g.alpha, g.w_zp, g.col_term, g.bias = K, N, w.data_ptr(), alpha.data_ptr(), zp.data_ptr(), ct.data_ptr(), None
    g.w4 = int(w4)
    NL = N // 2 if g.gate_q else N
    g.seg_end[0], g.seg_end[1] = NL // 3, 2 * NL // 3
    if g.norm_w:
        nw = (torch.rand(K, generator=gen) + 0.5).to(dev)
        keep.append(nw)
        g.norm_w = nw.data_ptr()
        if g.norm_bias:
            nb = torch.randn(K, generator=gen).to(dev) * 0.1
            keep.append(nb)
            g.norm_bias = nb.data_ptr()


def test_gemv_batch_launch_is_the_single_launch_per_row_in_every_mode(dev):
    """Every record the batched engine lowers (norm / layernorm prologues, int8 inputs, q|k|v segments, QSiLU / QGELU gates, residual
    adds, W8 / W4), at B = 1..8, then the same modes at K up to the entries' limits: fp32 prologues at K 4096 / 8192 (the rows the
    prologue re-reads instead of holding), a plain fp32 input, and int8 inputs up to B * K = 128 KiB (Gemma's w2 at K = 16 384)."""
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    gen = torch.Generator().manual_seed(0)
    keep = []
    for geom, wbits in (("llama", 8), ("stablelm", 4), ("gemma", 4), ("gemma", 8)):
        m = _model(dev, geom, 1, wbits)
        s = m.shape
        for B in range(1, 9):
            be = BatchDecodeEngine(m, B, cache_len=64)
            for i, (kind, ba) in enumerate(be.phases):
                if kind != "gemv":
                    continue
                g = ba.g
                gate = bool(g.gate_q)
                n_out = g.N // 2 if gate else g.N
                x_len = g.K
                outs = _gemv_rows(ba, B, n_out, n_out, x_len, bool(g.x), dev, gen, keep)
                _assert_same(outs, (geom, wbits, B, i))
        # the limits: B * K up to 128 KiB of images; fp32 rows at K 4096 / 8192 through the re-read path
        be = BatchDecodeEngine(m, 1, cache_len=64)
        qkv_rec, w13_rec, w2_rec = be.phases[0][1], be.phases[3][1], be.phases[4][1]
        for B, K, rec, w4 in ((8, 4096, qkv_rec, False), (4, 8192, qkv_rec, True), (8, 8192, w13_rec, wbits == 4),
                              (8, 16384, w2_rec, False), (4, 32768, w2_rec, True), (3, 8192, qkv_rec, False)):
            ba = _clone_struct(rec)
            ba.batch = B
            _random_linear(ba, K, 768, w4, gen, dev, keep)
            g = ba.g
            gate = bool(g.gate_q)
            n_out = 384 if gate else 768
            outs = _gemv_rows(ba, B, n_out, n_out, K, not g.xq, dev, gen, keep)
            _assert_same(outs, (geom, "limit", B, K, w4))
        # a plain fp32 input (no norm): the q|k|v record without its norm
        ba = _clone_struct(qkv_rec)
        ba.batch = 5
        ba.g.norm_w, ba.g.norm_bias, ba.g.layernorm = None, None, 0
        _random_linear(ba, 2048, 640, False, gen, dev, keep)
        outs = _gemv_rows(ba, 5, 640, 640, 2048, True, dev, gen, keep)
        _assert_same(outs, (geom, "fp32"))


@pytest.mark.parametrize("geom", ["llama", "stablelm"])
def test_gemv_batch_launch_is_the_single_launch_on_a_partial_last_pass_and_a_ragged_last_workgroup(dev, geom):
    """K = 2304 is 144 16-byte chunks per weight row (288 per w1|w3 pair, 72 / 144 packed): the last 64-chunk pass of a logical row is
    partial in every mode, and 257 logical rows leave the last workgroup short.  The q|k|v, the gated w1|w3 and the int8-input record,
    W8 and W4, at B = 3 and B = 8, row by row against mq_decode_gemv."""
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    gen = torch.Generator().manual_seed(1)
    keep = []
    be = BatchDecodeEngine(_model(dev, geom, 1, 8), 1, cache_len=64)
    K, NL = 2304, 257
    assert be.phases[3][1].g.gate_q and be.phases[4][1].g.xq and not be.phases[0][1].g.gate_q
    for name, rec in (("qkv", be.phases[0][1]), ("w13", be.phases[3][1]), ("w2", be.phases[4][1])):
        for w4 in (False, True):
            for B in (3, 8):
                ba = _clone_struct(rec)
                ba.batch = B
                gate = bool(ba.g.gate_q)
                _random_linear(ba, K, 2 * NL if gate else NL, w4, gen, dev, keep)
                outs = _gemv_rows(ba, B, NL, NL, K, not ba.g.xq, dev, gen, keep)
                _assert_same(outs, (geom, name, w4, B))


@pytest.mark.parametrize("geom", ["llama", "stablelm", "gemma"])
def test_attention_batch_launch_is_the_single_launch_per_sequence(dev, geom):
    """Different positions per sequence -- 0, block edges, the split threshold, cache_len - 1 and the idle sentinel -- in one launch:
    each sequence's output image and appended bytes equal mq_decode_attention's (1 and 4 splits); no other slot's byte moves."""
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _model(dev, geom, 1, 8)
    s = m.shape
    CL = 1600
    from mobilequant_amd import llama
    import dataclasses
    cos, sin = llama.rope_tables(dataclasses.replace(s, max_pos=CL))
    m.cos, m.sin = cos.to(dev), sin.to(dev)
    B = 8
    be = BatchDecodeEngine(m, B, cache_len=CL)
    ab = be.phases[1][1]
    gen = torch.Generator().manual_seed(2)
    positions = [0, 63, 64, 767, 768, 1300, CL - 1, CL]
    for trial in range(2):
        pos_t = torch.tensor(positions if trial == 0 else positions[::-1], dtype=torch.int32, device=dev)
        be.pos.copy_(pos_t)
        be.qkv.copy_(torch.randn(be.qkv.shape, generator=gen).to(dev) * 2)
        kc = torch.randint(-128, 128, be.k_cache[0].shape, generator=gen, dtype=torch.int8).to(dev)
        vc = torch.randint(-128, 128, be.v_cache[0].shape, generator=gen, dtype=torch.int8).to(dev)
        be.k_cache[0].copy_(kc)
        be.v_cache[0].copy_(vc)
        be.attn_q.fill_(85)
        _call("mq_decode_attention_batch", ctypes.byref(ab), _st())
        torch.cuda.synchronize()
        got_q, got_k, got_v = be.attn_q.clone(), be.k_cache[0].clone(), be.v_cache[0].clone()
        for nsplit in (1, 4):
            part = torch.zeros(nsplit, s.heads * s.head_dim, dtype=torch.int64, device=dev)
            ticket = torch.zeros(s.heads, dtype=torch.int32, device=dev)
            for b in range(B):
                a = _clone_struct(ab.a)
                k1, v1 = kc[b].clone(), vc[b].clone()
                oq = torch.full((s.heads * s.head_dim,), 85, dtype=torch.int8, device=dev)
                a.qkv = be.qkv[b].data_ptr()
                a.k_cache, a.v_cache, a.out_q, a.pos = k1.data_ptr(), v1.data_ptr(), oq.data_ptr(), pos_t[b:].data_ptr()
                a.nsplit, a.part, a.ticket = nsplit, part.data_ptr(), ticket.data_ptr()
                _call("mq_decode_attention", ctypes.byref(a), _st())
                torch.cuda.synchronize()
                p = int(pos_t[b])
                assert torch.equal(got_q[b], oq), (geom, b, p, nsplit)
                assert torch.equal(got_k[b], k1) and torch.equal(got_v[b], v1), (geom, b, p)
                if p >= CL:                                   # the idle slot: nothing moved
                    assert torch.equal(got_k[b], kc[b]) and torch.equal(got_v[b], vc[b]) and bool((got_q[b] == 85).all())
                else:                                         # exactly the appended position changed (where its bytes differ)
                    dk = (got_k[b] != kc[b]).any(dim=-1)
                    assert not dk[:, :p].any() and not dk[:, p + 1:].any()


@pytest.mark.parametrize("ln,K,V,B", [(False, 256, 160, 8), (True, 256, 96, 3), (False, 2048, 32000, 8), (True, 2048, 1000, 5),
                                      (False, 4096, 1003, 8), (False, 2048, 256000, 8), (False, 12288, 50, 2), (True, 1000, 77, 7)])
def test_head_batch_launch_is_the_single_head_per_row(dev, ln, K, V, B):
    """Final norm + lm_head for B rows against mq_decode_head per row, bit for bit (Gemma's V = 256 000 included); a row whose slot is
    idle keeps its logits."""
    from mobilequant_amd._lib import MqDecodeHeadBatchArgs
    gen = torch.Generator().manual_seed(K + V)
    x = (torch.randn(B, K, generator=gen) * 2).to(dev)
    nw = (torch.rand(K, generator=gen) + 0.5).to(dev)
    nb = (torch.randn(K, generator=gen) * 0.1).to(dev) if ln else None
    w = torch.randn(V, K, generator=torch.Generator(device=dev).manual_seed(K), device=dev) * 0.05
    bias = (torch.randn(V, generator=gen) * 0.1).to(dev) if ln else None
    cl = 100
    pos = torch.tensor([(7 * b) % cl if b != 1 else cl for b in range(B)], dtype=torch.int32, device=dev)
    logits = torch.full((B, V), -7777.0, device=dev)
    h = MqDecodeHeadBatchArgs()
    h.x, h.x_stride, h.norm_weight, h.norm_bias, h.layernorm, h.eps = x.data_ptr(), K, nw.data_ptr(), nb.data_ptr() if ln else None, int(ln), 1e-5
    h.w, h.bias, h.K, h.V, h.batch, h.logits, h.logits_stride = w.data_ptr(), bias.data_ptr() if ln else None, K, V, B, logits.data_ptr(), V
    h.pos, h.cache_len = pos.data_ptr(), cl
    _call("mq_decode_head_batch", ctypes.byref(h), _st())
    torch.cuda.synchronize()
    for b in range(B):
        one = torch.full((V,), -7777.0, device=dev)
        _call("mq_decode_head", x[b].data_ptr(), nw.data_ptr(), nb.data_ptr() if ln else None, int(ln), ctypes.c_float(1e-5), w.data_ptr(),
              bias.data_ptr() if ln else None, K, V, one.data_ptr(), _st())
        torch.cuda.synchronize()
        if B > 1 and b == 1:
            assert bool((logits[b] == -7777.0).all()), "an idle row was written"
            continue
        assert torch.equal(logits[b].view(torch.int32), one.view(torch.int32)), (ln, K, V, b)
