"""GPU: multi-token decode steps and speculative greedy generation (csrc/mq_decode_rows.hip, DecodeEngine.step_tokens / extend /
rewind / generate(draft=...)).

The single-token path is the oracle and the bar is bit identity.  Kernel: mq_decode_attention_multi against `rows` sequential
mq_decode_attention_batch launches at batch 1 over the same cache (its out_q rows and every cache byte), in both value layouts.
Engine: every step_tokens row against the logits of single step() calls, the caches against theirs.  Speculative generation: the
returned ids against plain greedy generate, token for token, for every kind of draft."""
import ctypes
import dataclasses
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_decode_batch import _model  # noqa: E402
from test_gpu_decode_grouped import _model as _grouped_model  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _clone_struct(s):
    c = type(s)()
    ctypes.pointer(c)[0] = s
    return c


def _long_rope(m, n):
    from mobilequant_amd import llama
    cos, sin = llama.rope_tables(dataclasses.replace(m.shape, max_pos=n))
    m.cos, m.sin = cos.to(m.cos.device), sin.to(m.cos.device)


def _flat_values(eng, vc):
    """A value cache of the engine's layout as [kv_heads, cache_len, head_dim]."""
    if not eng.v_transposed:
        return vc
    kv, ch, D, _ = vc.shape
    return vc.permute(0, 1, 3, 2).reshape(kv, ch * 16, D)


def _to_layout(eng, flat):
    if not eng.v_transposed:
        return flat.clone()
    kv, n, D = flat.shape
    return flat.view(kv, n // 16, 16, D).permute(0, 1, 3, 2).contiguous()


# ---- kernel ---------------------------------------------------------------------------------------------------------------------
def _check_multi_launch(eng, p, R, gen):
    """One mq_decode_attention_multi launch of R rows at position p over random caches / q|k|v rows against R sequential
    mq_decode_attention_batch launches at batch 1 (the reference walks positions p .. p + R - 1, each appending its own)."""
    from mobilequant_amd import _lib
    from mobilequant_amd._lib import MqDecodeAttentionBatchArgs
    if eng._rows is None:
        eng._lower_rows()
    ma = next(a for k, a in eng._rows[0] if k == "attn_multi")          # layer 0
    ma.rows = R
    s, CL, dev = eng.shape, eng.cache_len, eng.dev
    HD = s.heads * s.head_dim
    eng.rqkv.copy_(torch.randn(eng.rqkv.shape, generator=gen).to(dev) * 2)
    kc = torch.randint(-128, 128, eng.k_cache[0].shape, generator=gen, dtype=torch.int8).to(dev)
    vflat = torch.randint(-128, 128, (s.kv_heads, CL, s.head_dim), generator=gen, dtype=torch.int8).to(dev)
    eng.k_cache[0].copy_(kc)
    eng.v_cache[0].copy_(_to_layout(eng, vflat))
    eng.rattn_q.fill_(85)
    eng.pos.fill_(p)
    _lib.call("mq_decode_attention_multi", ctypes.byref(ma), _st())
    torch.cuda.synchronize()
    got_q, got_k, got_v = eng.rattn_q.clone(), eng.k_cache[0].clone(), _flat_values(eng, eng.v_cache[0]).clone()
    # reference: batch-1 launches in sequence, the flat value layout
    k1, v1 = kc.clone(), vflat.clone()
    part = torch.zeros(eng.LONG_SPLITS, HD, dtype=torch.int64, device=dev)
    ticket = torch.zeros(s.heads, dtype=torch.int32, device=dev)
    for j in range(R):
        oq = torch.full((HD,), 85, dtype=torch.int8, device=dev)
        if p + j < CL:
            a = _clone_struct(ma.a)
            pos_t = torch.tensor([p + j], dtype=torch.int32, device=dev)
            a.qkv, a.k_cache, a.v_cache, a.out_q, a.pos = eng.rqkv[j].data_ptr(), k1.data_ptr(), v1.data_ptr(), oq.data_ptr(), pos_t.data_ptr()
            a.part, a.ticket = part.data_ptr(), ticket.data_ptr()
            b = MqDecodeAttentionBatchArgs()
            b.a, b.batch, b.split_from, b.qkv_stride = a, 1, ma.split_from, ma.qkv_stride
            _lib.call("mq_decode_attention_batch", ctypes.byref(b), _st())
            torch.cuda.synchronize()
        assert torch.equal(got_q[j], oq), (p, R, j, eng.v_transposed)
    assert torch.equal(got_k, k1), (p, R, eng.v_transposed)
    assert torch.equal(got_v, v1), (p, R, eng.v_transposed)
    # no row beyond R was written
    assert bool((eng.rattn_q[R:] == 85).all())


@pytest.mark.parametrize("geom", ["llama", "stablelm", "gemma"])
@pytest.mark.parametrize("launches", [5, 4], ids=["flat_values", "chunked_values"])
def test_attention_multi_launch_is_sequential_single_launches(dev, geom, launches):
    """Rows 1..8 at positions on both sides of a 16-position chunk, a 64-position block and the split threshold (768), and rows that
    run past cache_len: the output images and every cache byte equal sequential batch-1 launches."""
    from mobilequant_amd.decode import DecodeEngine
    m = _model(dev, geom, 1, 8)
    CL = 1024
    _long_rope(m, CL)
    eng = DecodeEngine(m, cache_len=CL, launches=launches)
    assert eng.v_transposed == (launches == 4)
    gen = torch.Generator().manual_seed(7)
    for p in (0, 1, 14, 15, 16, 17, 60, 63, 64, 65, 127, 760, 765, 767, 768, 769, CL - 9, CL - 8, CL - 3, CL - 1):
        for R in range(1, 9):
            _check_multi_launch(eng, p, R, gen)


@pytest.mark.parametrize("launches", [5, 4], ids=["flat_values", "chunked_values"])
def test_attention_multi_launch_long_cache(dev, launches):
    from mobilequant_amd.decode import DecodeEngine
    m = _model(dev, "llama", 1, 8)
    CL = 8448
    _long_rope(m, CL)
    eng = DecodeEngine(m, cache_len=CL, launches=launches)
    gen = torch.Generator().manual_seed(8)
    for p, R in ((8190, 8), (8192, 5), (CL - 6, 8), (5000, 3)):
        _check_multi_launch(eng, p, R, gen)


# ---- engine ---------------------------------------------------------------------------------------------------------------------
RECIPES = {"w8a8": lambda dev, geom, layers: _model(dev, geom, layers, 8),
           "w4a8": lambda dev, geom, layers: _model(dev, geom, layers, 4),
           "w4g128": lambda dev, geom, layers: _grouped_model(dev, geom, layers, 4, 128)}


def _steps(eng, prompt, toks):
    """The single-token oracle: prefill, then one step() per token -> ([logits after each token], caches)."""
    eng.reset()
    eng.prefill(prompt)
    out = [eng.step(t).clone() for t in toks]
    return out, _caches(eng)


def _caches(eng):
    n = eng.position()
    return [(eng.k_cache[li][:, :n].clone(), eng.cached_values(li, n).clone()) for li in range(len(eng.k_cache))]


def _same_caches(eng, want, tag):
    for li, (k, v) in enumerate(want):
        n = k.shape[1]
        assert eng.position() == n, tag
        assert torch.equal(eng.k_cache[li][:, :n], k) and torch.equal(eng.cached_values(li, n), v), (tag, li)


@pytest.mark.parametrize("recipe", list(RECIPES))
@pytest.mark.parametrize("launches", [4, 5])
@pytest.mark.parametrize("captured", [False, True], ids=["direct", "graph"])
def test_step_tokens_rows_are_single_steps_bit_for_bit(dev, recipe, launches, captured):
    from mobilequant_amd.decode import DecodeEngine
    m = RECIPES[recipe](dev, "llama", 2)
    CL = 848
    g = torch.Generator().manual_seed(4)
    ref = DecodeEngine(m, cache_len=CL, launches=launches)
    eng = DecodeEngine(m, cache_len=CL, launches=launches)
    assert eng.launches == ref.launches and eng.max_rows == 8
    for plen, chunks in ((9, [1, 3, 8, 7, 2, 8, 5]), (700, [8] * 9 + [6])):
        prompt = torch.randint(0, m.shape.vocab, (plen,), generator=g).tolist()
        toks = torch.randint(0, m.shape.vocab, (sum(chunks),), generator=g).tolist()
        want, caches = _steps(ref, prompt, toks)
        eng.reset()
        eng.prefill(prompt)
        if captured:
            eng.capture()
        i = 0
        for c in chunks:
            rows = eng.step_tokens(toks[i:i + c])
            assert rows.shape == (c, m.shape.vocab)
            for r in range(c):
                assert torch.equal(rows[r], want[i + r]), (recipe, launches, plen, i, r, float((rows[r] - want[i + r]).abs().max()))
            assert torch.equal(eng.logits, want[i + c - 1])
            i += c
        _same_caches(eng, caches, (recipe, launches, plen))
        if captured:
            assert set(eng._row_graphs) == set(chunks)


@pytest.mark.parametrize("geom,recipe", [("stablelm", "w8a8"), ("gemma", "w4a8")])
def test_step_tokens_other_geometries(dev, geom, recipe):
    from mobilequant_amd.decode import DecodeEngine
    m = RECIPES[recipe](dev, geom, 2)
    g = torch.Generator().manual_seed(5)
    for launches in (4, 5):
        ref, eng = DecodeEngine(m, cache_len=160, launches=launches), DecodeEngine(m, cache_len=160, launches=launches)
        prompt = torch.randint(0, m.shape.vocab, (57,), generator=g).tolist()
        toks = torch.randint(0, m.shape.vocab, (20,), generator=g).tolist()
        want, caches = _steps(ref, prompt, toks)
        eng.reset()
        eng.prefill(prompt)
        i = 0
        for c in (8, 4, 8):
            rows = eng.step_tokens(toks[i:i + c])
            for r in range(c):
                assert torch.equal(rows[r], want[i + r]), (geom, launches, i, r)
            i += c
        _same_caches(eng, caches, (geom, launches))


@pytest.mark.parametrize("launches", [4, 5])
def test_extend_is_n_steps(dev, launches):
    from mobilequant_amd.decode import DecodeEngine
    m = _model(dev, "llama", 2, 8)
    g = torch.Generator().manual_seed(6)
    ref, eng = DecodeEngine(m, cache_len=128, launches=launches), DecodeEngine(m, cache_len=128, launches=launches)
    prompt = torch.randint(0, m.shape.vocab, (13,), generator=g).tolist()
    for n in (1, 7, 8, 9, 30):
        toks = torch.randint(0, m.shape.vocab, (n,), generator=g).tolist()
        want, caches = _steps(ref, prompt, toks)
        eng.reset()
        eng.prefill(prompt)
        got = eng.extend(toks)
        assert torch.equal(got, want[-1]), (launches, n)
        _same_caches(eng, caches, (launches, n))
        # the engine goes on with single steps from there
        nxt = int(torch.argmax(want[-1]))
        assert torch.equal(eng.step(nxt), ref.step(nxt))


@pytest.mark.parametrize("launches", [4, 5])
@pytest.mark.parametrize("captured", [False, True], ids=["direct", "graph"])
def test_rewind_forgets_the_dropped_positions(dev, launches, captured):
    """Garbage tokens, rewind, then more steps (multi-token and single): the same bits as an engine that never saw the garbage --
    rewinds into the middle of a 16-position chunk and across a 64-position block included."""
    from mobilequant_amd.decode import DecodeEngine
    m = _model(dev, "llama", 2, 8)
    g = torch.Generator().manual_seed(9)
    ref, eng = DecodeEngine(m, cache_len=256, launches=launches), DecodeEngine(m, cache_len=256, launches=launches)
    prompt = torch.randint(0, m.shape.vocab, (58,), generator=g).tolist()
    toks = torch.randint(0, m.shape.vocab, (24,), generator=g).tolist()
    want, caches = _steps(ref, prompt, toks)
    eng.reset()
    eng.prefill(prompt)
    if captured:
        eng.capture()
    junk = lambda n: torch.randint(0, m.shape.vocab, (n,), generator=g).tolist()      # noqa: E731
    eng.step_tokens(junk(8))                                   # 58 .. 65: across the 64-block, then dropped
    eng.rewind(58)
    rows = eng.step_tokens(toks[:3] + junk(5))                 # 3 kept, 5 dropped (61 .. 65)
    for r in range(3):
        assert torch.equal(rows[r], want[r])
    eng.rewind(61)
    for i in range(3, 10):                                     # single steps over the dropped bytes
        assert torch.equal(eng.step(toks[i]), want[i]), i
    eng.step(junk(1)[0])
    eng.rewind(68)
    rows = eng.step_tokens(toks[10:18])
    for r in range(8):
        assert torch.equal(rows[r], want[10 + r])
    got = eng.extend(toks[18:])
    assert torch.equal(got, want[-1])
    _same_caches(eng, caches, (launches, captured))
    with pytest.raises(ValueError):
        eng.rewind(eng.position() + 1)


def test_step_tokens_limits(dev):
    from mobilequant_amd.decode import DecodeEngine
    m = _model(dev, "llama", 1, 8)
    eng = DecodeEngine(m, cache_len=32)
    eng.reset()
    eng.extend(list(range(28)))
    with pytest.raises(RuntimeError, match="overflow"):
        eng.step_tokens([1] * 5)
    with pytest.raises(ValueError, match="outside 1..8"):
        eng.step_tokens([1] * 9)
    with pytest.raises(ValueError, match="outside 1..8"):
        eng.step_tokens([])
    eng.step_tokens([1] * 4)
    assert eng.position() == 32


# ---- speculative ----------------------------------------------------------------------------------------------------------------
def _always_wrong(ref_ids, vocab):
    def draft(ids, k):
        return [(ref_ids[len(ids) + i] + 1) % vocab if len(ids) + i < len(ref_ids) else 0 for i in range(k)]
    return draft


@pytest.mark.parametrize("launches", [4, 5])
def test_speculative_greedy_is_plain_greedy(dev, launches):
    from mobilequant_amd.decode import DecodeEngine, prompt_lookup_draft
    m = _model(dev, "llama", 2, 8)
    small = _model(dev, "llama", 1, 8, seed=23)
    V = m.shape.vocab
    g = torch.Generator().manual_seed(12)
    CL, N = 160, 40
    eng = DecodeEngine(m, cache_len=CL, launches=launches)
    self_draft = DecodeEngine(m, cache_len=CL, launches=launches)
    small_draft = DecodeEngine(small, cache_len=CL)
    # a prompt that repeats itself, so that prompt lookup has something to find
    base = torch.randint(0, V, (12,), generator=g).tolist()
    ctx = base + base[:7]
    plain = eng.generate(ctx, N)
    assert len(plain) == len(ctx) + N
    eos = plain[len(ctx) + 6]                                   # hit inside an accepted run of the self-draft
    plain_eos = eng.generate(ctx, N, eos_token_id=eos)
    assert len(plain_eos) < len(plain)
    for nd in (1, 3, 7):
        for name, draft in (("self", self_draft), ("small", small_draft), ("wrong", _always_wrong(plain, V)),
                            ("lookup", prompt_lookup_draft(3))):
            got = eng.generate(ctx, N, draft=draft, num_draft=nd)
            assert got == plain, (launches, nd, name)
            st = eng.spec_stats
            assert st["target_steps"] == st["rounds"] and st["accepted"] <= st["proposed"]
            if name == "self":
                assert st["accepted"] == st["proposed"], st
                assert st["target_steps"] == math.ceil((N - 1) / (nd + 1)), (nd, st)
            if name == "wrong":
                assert st["accepted"] == 0 and st["target_steps"] == N - 1, st
            assert eng.generate(ctx, N, eos_token_id=eos, draft=draft, num_draft=nd) == plain_eos, (launches, nd, name, "eos")
            if name == "self":
                assert eng.spec_stats["accepted"] == eng.spec_stats["proposed"]
    # near the cache end: context + new tokens fill the cache exactly
    ctx2 = ctx + plain[len(ctx):len(ctx) + 100]
    n2 = CL - len(ctx2)
    want = eng.generate(ctx2, n2)
    for nd in (1, 3, 7):
        for draft in (self_draft, prompt_lookup_draft(2), _always_wrong(want, V)):
            assert eng.generate(ctx2, n2, draft=draft, num_draft=nd) == want, nd
    # one-token context: the step kernels start the sequence
    assert eng.generate(ctx[:1], 12, draft=self_draft, num_draft=3) == eng.generate(ctx[:1], 12)


def test_speculative_refuses_sampling_and_bad_drafts(dev):
    from mobilequant_amd.decode import DecodeEngine
    m = _model(dev, "llama", 1, 8)
    eng = DecodeEngine(m, cache_len=64)
    with pytest.raises(ValueError, match="greedy"):
        eng.generate([1, 2, 3], 4, do_sample=True, draft=lambda ids, k: [])
    with pytest.raises(ValueError, match="another engine"):
        eng.generate([1, 2, 3], 4, draft=eng)
    other = _model(dev, "stablelm", 1, 8)                       # vocabulary 96 against 160
    with pytest.raises(ValueError, match="vocabulary"):
        eng.generate([1, 2, 3], 4, draft=DecodeEngine(other, cache_len=64))
    with pytest.raises(TypeError):
        eng.generate([1, 2, 3], 4, draft=5)


def _tinyllama_draft(dev, vocab):
    """A 2-layer model of the TinyLlama geometry (hidden 2048, GQA 32 / 4, FFN 5632) through test_gpu_decode_batch._model's recipe."""
    import mobilequant_amd as mq
    from mobilequant_amd.calibration import get_act_range
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    shape = LlamaShape(hidden=2048, layers=2, heads=32, kv_heads=4, head_dim=64, ffn=5632, vocab=vocab, eps=1e-5, max_pos=512)
    m = LlamaForCausalLM(shape)
    m.reset_parameters(seed=31, std=0.02)
    m = m.to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(5)
    act = get_act_range(m, [torch.randint(0, vocab, (1, 48), generator=g) for _ in range(2)])
    mq.create_sim_qmodel(m, mq.QuantConfig(bitwidth=8), mq.QuantConfig(bitwidth=8))
    for n, mod in m.named_modules():
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


def test_full_size_tinyllama_speculative_with_a_two_layer_draft(dev):
    """22-layer TinyLlama geometry target, 2-layer draft of the same vocabulary: 64 new tokens equal plain greedy."""
    from test_gpu_round5 import _stable_model
    from mobilequant_amd.decode import DecodeEngine
    m, z = _stable_model(dev, "w8a8")
    cl = 320
    _long_rope(m, cl)
    eng = DecodeEngine(m, cache_len=cl)
    assert eng.max_rows == 8
    draft = DecodeEngine(_tinyllama_draft(dev, m.shape.vocab), cache_len=cl)
    ctx = np.asarray(z["ids"])[:40].tolist()
    plain = eng.generate(ctx, 64)
    for nd in (3, 7):
        assert eng.generate(ctx, 64, draft=draft, num_draft=nd) == plain, nd
        assert eng.spec_stats["rounds"] >= 1
    # and step_tokens at full size: rows are single steps
    eng.reset()
    eng.prefill(ctx)
    ref = [eng.step(t).clone() for t in plain[40:48]]
    eng.rewind(40)
    rows = eng.step_tokens(plain[40:48])
    for r in range(8):
        assert torch.equal(rows[r], ref[r]), r
