"""DecodeEngine.prefill(append=True) / BatchDecodeEngine.prefill(slot, ids, append=True) and the two kernels under them
(mq_attention_cache_import / mq_attention_cache_export): a live decode sequence is continued with ONE chunked forward
of the model over image caches built from the engine's int8 caches.  Everything here is an equality of integers or of bits: the
images against a torch restatement of the header's formulas and against the prefill's own preparation kernel, the exported bytes
against the images, the appended logits against the model's own chunked forward, the stepped part against step()."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CACHE_LEN = 256
_MODELS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(dev, D, fused=True, kv_heads=2):
    """LlamaShape.toy variant (2 layers, 4 / kv_heads heads; kv_heads = 1 at head_dim 256 is Gemma's MQA geometry) at head_dim D, W8A8,
    calibrated, the attention QMatMuls on fixed grids; fused through fuse_decoder_layer unless fused=False.  Built once per
    (D, fused, kv_heads)."""
    key = (D, fused, kv_heads)
    if key in _MODELS:
        return _MODELS[key]
    import mobilequant_amd as mq
    from mobilequant_amd import llama
    from mobilequant_amd.calibration import get_act_range
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    shape = LlamaShape.toy(hidden=256, layers=2, heads=4, kv_heads=kv_heads, head_dim=D, ffn=512, vocab=97, max_pos=CACHE_LEN)
    m = LlamaForCausalLM(shape)
    m.reset_parameters(seed=3, std=0.08)
    m = m.to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(1)
    act = get_act_range(m, [torch.randint(0, shape.vocab, (1, 32), generator=g)])
    a8 = mq.QuantConfig(bitwidth=8)
    mq.create_sim_qmodel(m, mq.QuantConfig(bitwidth=8), a8)
    for n, mod in m.named_modules():
        if isinstance(mod, mq.QLinear) and ("w2" in n or "o_proj" in n):
            mod.output_quantizer.qcfg.bitwidth = 16
        elif isinstance(mod, (mq.QRMSNorm, mq.QLayerNorm)):
            mod.input_quantizer.qcfg.bitwidth = 16
            mod.weight_quantizer.qcfg.bitwidth = 16
    mq.set_scale_and_offset(m, act, "buffer")
    for layer in m.layers:
        at = layer.self_attn
        for q, bits, lo, hi in ((at.qk_bmm.input_quantizer, 8, -4.0, 4.0), (at.qk_bmm.input2_quantizer, 8, -4.5, 4.5),
                                (at.qk_bmm.output_quantizer, 16, -60.0, 60.0), (at.pv_bmm.input_quantizer, 16, 0.0, 1.0),
                                (at.pv_bmm.input2_quantizer, 8, -4.0, 4.0), (at.pv_bmm.output_quantizer, 8, -1.5, 1.5)):
            q.qcfg.bitwidth = bits
            q.set_scale_offset_from_minmax(torch.tensor(lo), torch.tensor(hi), "buffer", dev)
    if fused:
        assert llama.fuse_decoder_layer(m) == 2
    _MODELS[key] = m
    return m


def _engine_kv_heads(D):
    """The engine tests run head_dim 256 as MQA (one kv head under four query heads); the import tests keep two kv heads there."""
    return 1 if D == 256 else 2


def _ids(m, n=CACHE_LEN, seed=7):
    return torch.randint(0, m.shape.vocab, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def _engine(m, launches):
    from mobilequant_amd.decode import DecodeEngine
    e = DecodeEngine(m, cache_len=CACHE_LEN, launches=launches)
    assert e.launches == launches and e.v_transposed == (launches == 4)
    return e


def _grids(m, li=0):
    qk = m.layers[li].self_attn.qk_bmm
    return {name: (q.scale.detach(), q.offset.detach(), q.qmin, q.qmax) for name, q in (("qk_a", qk.input_quantizer), ("qk_b", qk.input2_quantizer))}


# ---- the header's formulas (include/mobilequant_amd.h above mq_attention_args), in torch ------------------------------------------
def _vt_of(v):
    """v [KV, n, D] int8 -> vT image [KV, n / 64, D, 64]: key t = 64 b + 16 j + 4 tq + e at kappa = 16 tq + 4 j + e."""
    KV, n, D = v.shape
    return v.view(KV, n // 64, 4, 4, 4, D).permute(0, 1, 5, 3, 2, 4).reshape(KV, n // 64, D, 64)


def _v_of(vt):
    """the inverse: vT image [KV, nb, D, 64] -> v [KV, 64 nb, D]."""
    KV, nb, D, _ = vt.shape
    return vt.view(KV, nb, D, 4, 4, 4).permute(0, 1, 4, 3, 5, 2).reshape(KV, nb * 64, D)


def _k_f16_of(k, zk):
    """k [KV, n, 64] int8 -> fp16(ik - zk) in the fragment-blocked order, as [KV, n / 64, 8, 64, 8]."""
    KV, n, D = k.shape
    c = ((k.float() + 128.0) - zk).half()
    return c.view(KV, n // 64, 4, 16, 4, 2, 8).permute(0, 1, 2, 5, 4, 3, 6).reshape(KV, n // 64, 8, 64, 8)


def _image_views(c):
    KV, D, R = c["kv_heads"], c["head_dim"], c["rows"]
    out = {"k_i8": c["k_i8"].view(KV, R, D), "k_rs": c["k_rs"].view(KV, R), "vt_i8": c["vt_i8"].view(KV, R // 64, D, 64)}
    if c["v_pre"] is not None:
        out["v_pre"] = c["v_pre"].view(KV, R // 64, D)
    if c["k_f16"] is not None:
        out["k_f16"] = c["k_f16"].view(torch.int16).view(KV, R // 64, 8, 64, 8)
    return out


def _decoded(c, n):
    """(k, v) [KV, n, D] int8 the image cache holds for positions 0 .. n - 1."""
    iv = _image_views(c)
    return iv["k_i8"][:, :n].clone(), _v_of(iv["vt_i8"])[:, :n].clone()


def _greedy(e, n=4):
    rows = []
    for _ in range(n):
        rows.append(e.step(int(e.logits.argmax())).clone())
    return torch.stack(rows)


# ---- 1 / 2: import ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launches", [4, 5])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_import_matches_the_header_formulas(dev, D, launches):
    from mobilequant_amd import ops
    m = _model(dev, D)
    e = _engine(m, launches)
    e.fill_cache_random(128, seed=11)
    s = m.shape
    c = ops.attention_image_cache(s.kv_heads, D, CACHE_LEN, dev)
    for name in ("k_i8", "vt_i8", "k_rs", "v_pre"):
        if c[name] is not None:
            c[name].fill_(0x33 if c[name].dtype == torch.int8 else 0x33333333)
    if c["k_f16"] is not None:
        c["k_f16"].view(torch.int16).fill_(0x3333)
    g = _grids(m, 1)
    zq, zk = float(g["qk_a"][1]), float(g["qk_b"][1])
    ops.attention_cache_import(c, e.k_cache[1], e.v_cache[1], 128, g, v_chunked=e.v_transposed)
    torch.cuda.synchronize()
    k, v = e.k_cache[1][:, :128], e.cached_values(1, 128).contiguous()
    iv = _image_views(c)
    assert torch.equal(iv["k_i8"][:, :128], k)
    assert torch.equal(iv["k_rs"][:, :128], (-(int(zq) - 128) * k.int().sum(-1)).int())
    assert torch.equal(iv["vt_i8"][:, :2], _vt_of(v))
    if D == 64:
        assert c["k_f16_valid"] is True and ops.attention_f16_offsets_ok(zk)
        assert torch.equal(iv["k_f16"][:, :2], _k_f16_of(k, zk).view(torch.int16))
        assert bool((iv["k_f16"][:, 2:] == 0x3333).all())
    else:
        assert torch.equal(iv["v_pre"][:, :2], v.view(s.kv_heads, 2, 64, D).int().sum(2).cumsum(1).int())
        assert bool((iv["v_pre"][:, 2:] == 0x33333333).all())
    assert bool((iv["k_i8"][:, 128:] == 0x33).all()) and bool((iv["vt_i8"][:, 2:] == 0x33).all()) and bool((iv["k_rs"][:, 128:] == 0x33333333).all())


@pytest.mark.parametrize("D,launches", [(64, 4), (128, 5), (256, 4), (256, 5)])
def test_import_matches_the_prefill_preparation(dev, D, launches):
    """The images the model's own chunk at pos 0 leaves are, byte for byte, what the import makes of the caches prefill() filled."""
    from mobilequant_amd import ops
    m = _model(dev, D)
    ids = _ids(m)
    ref = m.new_image_cache(1, CACHE_LEN)
    with torch.no_grad():
        m(torch.tensor(ids[:128], device=dev).view(1, -1), cache=ref, pos=0)
    e = _engine(m, launches)
    e.prefill(ids[:128])
    for li in range(2):
        c = ops.attention_image_cache(m.shape.kv_heads, D, CACHE_LEN, dev)
        ops.attention_cache_import(c, e.k_cache[li], e.v_cache[li], 128, _grids(m, li), v_chunked=e.v_transposed)
        torch.cuda.synchronize()
        got, want = _image_views(c), _image_views(ref[li].per_sequence[0])
        for name in ("k_i8", "k_rs"):
            assert torch.equal(got[name][:, :128], want[name][:, :128]), (li, name)
        for name in ("vt_i8", "v_pre"):
            if name in got:
                assert torch.equal(got[name][:, :2], want[name][:, :2]), (li, name)
        if D == 64:
            assert ref[li].per_sequence[0]["k_f16_valid"] and c["k_f16_valid"]
            assert torch.equal(got["k_f16"][:, :2], want["k_f16"][:, :2]), li


# ---- 3: export ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_export_writes_the_rows_and_nothing_else(dev, D, chunked):
    from mobilequant_amd import ops
    KV, p0, n = 2, 64, 37
    g = torch.Generator(device=dev).manual_seed(D + chunked)
    c = ops.attention_image_cache(KV, D, CACHE_LEN, dev)
    for name in ("k_i8", "vt_i8"):
        c[name].copy_(torch.randint(-128, 128, c[name].shape, generator=g, device=dev, dtype=torch.int8))
    # the state before is seeded random bytes, not a constant: a stray write of any byte shows
    k = torch.randint(-128, 128, (KV, CACHE_LEN, D), generator=g, device=dev, dtype=torch.int8)
    v = torch.randint(-128, 128, (KV, CACHE_LEN // 16, D, 16) if chunked else (KV, CACHE_LEN, D), generator=g, device=dev, dtype=torch.int8)
    k0, v0 = k.clone(), v.clone()
    ops.attention_cache_export(c, k, v, p0, n, v_chunked=chunked)
    torch.cuda.synchronize()
    want_k, want_v = _decoded(c, CACHE_LEN)
    logical, logical0 = (t.permute(0, 1, 3, 2).reshape(KV, CACHE_LEN, D) if chunked else t for t in (v, v0))
    for got, want, before in ((k, want_k, k0), (logical, want_v, logical0)):
        assert torch.equal(got[:, p0:p0 + n], want[:, p0:p0 + n])
        assert torch.equal(got[:, :p0], before[:, :p0]) and torch.equal(got[:, p0 + n:], before[:, p0 + n:])


# ---- 4 .. 7, 9, 10: the engine --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,launches", [(64, 4), (64, 5), (128, 4), (128, 5), (256, 4), (256, 5)])
def test_aligned_append_is_the_models_chunked_forward(dev, D, launches):
    from mobilequant_amd.decode import DecodeEngine
    m = _model(dev, D, kv_heads=_engine_kv_heads(D))
    ids = _ids(m)
    ref = m.new_image_cache(1, CACHE_LEN)
    with torch.no_grad():
        m(torch.tensor(ids[:64], device=dev).view(1, -1), cache=ref, pos=0, last_logits_only=True)
        want = m(torch.tensor(ids[64:150], device=dev).view(1, -1), cache=ref, pos=64, last_logits_only=True)[0, -1].clone()
    e = _engine(m, launches)
    e.prefill(ids[:64])
    got = e.prefill(ids[64:150], append=True)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and got is e.logits
    assert e.position() == 150 and int(e.pos.item()) == 150
    assert e.append_stats["stepped"] == 0 and e.append_stats["prefilled"] == 86 and e.append_stats["reason"] is None
    e2 = DecodeEngine(m, cache_len=CACHE_LEN, launches=launches)
    for li in range(2):
        k, v = _decoded(ref[li].per_sequence[0], 150)
        assert torch.equal(e.k_cache[li][:, :150], k) and torch.equal(e.cached_values(li, 150), v), li
        e2.k_cache[li][:, :150] = k
        e2.load_cached_values(li, v)
    e2.set_position(150)
    e2.logits.copy_(want)
    assert torch.equal(_greedy(e), _greedy(e2))


@pytest.mark.parametrize("D,launches", [(64, 4), (128, 5), (256, 4)])
def test_unaligned_append_steps_to_the_boundary(dev, D, launches):
    m = _model(dev, D, kv_heads=_engine_kv_heads(D))
    ids = _ids(m)
    a, b = _engine(m, launches), _engine(m, launches)
    for e in (a, b):
        e.prefill(ids[:64])
        e.extend(ids[64:70])
    a.prefill(ids[70:200], append=True)
    assert a.append_stats["stepped"] == 58 and a.append_stats["prefilled"] == 72 and a.append_stats["reason"] is None
    b.extend(ids[70:128])
    b.prefill(ids[128:200], append=True)
    assert b.append_stats["stepped"] == 0 and b.append_stats["prefilled"] == 72
    torch.cuda.synchronize()
    assert a.position() == b.position() == 200 and torch.equal(a.logits, b.logits)
    for li in range(2):
        assert torch.equal(a.k_cache[li][:, :200], b.k_cache[li][:, :200]) and torch.equal(a.cached_values(li), b.cached_values(li))
    # one appended token is step(token)
    a.prefill(ids[200:201], append=True)
    b.step(ids[200])
    assert a.append_stats["stepped"] == 1 and a.append_stats["prefilled"] == 0 and torch.equal(a.logits, b.logits) and a.position() == 201
    # an append that ends at the boundary, or one token past it, is all stepped
    for end in (128, 129):
        a.rewind(70), b.rewind(70)
        a.prefill(ids[70:end], append=True)
        b.extend(ids[70:end])
        assert a.append_stats["stepped"] == end - 70 and a.append_stats["prefilled"] == 0
        assert a.position() == end and torch.equal(a.logits, b.logits)
        for li in range(2):
            assert torch.equal(a.k_cache[li][:, :end], b.k_cache[li][:, :end]) and torch.equal(a.cached_values(li), b.cached_values(li))


def test_captured_engine_appends_like_an_uncaptured_one(dev):
    m = _model(dev, 64)
    ids = _ids(m)
    a, b = _engine(m, 4), _engine(m, 4)
    a.capture()
    for e in (a, b):
        e.prefill(ids[:64])
        e.extend(ids[64:70])
        e.prefill(ids[70:200], append=True)
        assert e.append_stats["stepped"] == 58 and e.append_stats["prefilled"] == 72
    assert a.graph is not None and b.graph is None
    assert torch.equal(a.logits, b.logits)
    assert torch.equal(_greedy(a, 3), _greedy(b, 3))


def test_rewind_then_append_is_a_fresh_engine_at_that_position(dev):
    m = _model(dev, 64)
    ids = _ids(m)
    a, b = _engine(m, 4), _engine(m, 4)
    a.prefill(ids[:64])
    a.extend(ids[150:190])                    # positions 64 .. 103 hold another continuation, then are dropped
    a.rewind(64)
    b.prefill(ids[:64])
    for e in (a, b):
        e.prefill(ids[64:150], append=True)
    assert a.position() == 150 and torch.equal(a.logits, b.logits)
    for li in range(2):
        assert torch.equal(a.k_cache[li][:, :150], b.k_cache[li][:, :150]) and torch.equal(a.cached_values(li), b.cached_values(li))
    assert torch.equal(_greedy(a, 2), _greedy(b, 2))


@pytest.mark.parametrize("D", [64, 128, 256])
def test_batched_engine_appends_on_one_slot(dev, D):
    from mobilequant_amd.decode_batch import BatchDecodeEngine
    m = _model(dev, D, kv_heads=_engine_kv_heads(D))
    ids, ids0, ids2 = _ids(m), _ids(m, 40, seed=8), _ids(m, 90, seed=9)
    be, twin = BatchDecodeEngine(m, 3, cache_len=CACHE_LEN), BatchDecodeEngine(m, 3, cache_len=CACHE_LEN)
    for e in (be, twin):
        e.prefill(0, ids0)
        e.prefill(1, ids[:70])
        e.prefill(2, ids2)
    before = [(be.k_cache[li][[0, 2]].clone(), be.v_cache[li][[0, 2]].clone()) for li in range(2)]
    rows_before = be.logits[[0, 2]].clone()
    got = be.prefill(1, ids[70:200], append=True).clone()
    assert be.append_stats["stepped"] == 58 and be.append_stats["prefilled"] == 72 and be.append_stats["reason"] is None
    single = _engine(m, 5)
    single.prefill(ids[:70])
    single.prefill(ids[70:200], append=True)
    torch.cuda.synchronize()
    assert torch.equal(got, single.logits) and be.position(1) == 200
    for li in range(2):
        assert torch.equal(be.cached_keys(1, li), single.k_cache[li][:, :200]) and torch.equal(be.cached_values(1, li), single.cached_values(li))
        assert torch.equal(be.k_cache[li][[0, 2]], before[li][0]) and torch.equal(be.v_cache[li][[0, 2]], before[li][1])
    assert [be.position(0), be.position(2)] == [40, 90] and be.pos.tolist() == [40, 200, 90] and torch.equal(be.logits[[0, 2]], rows_before)
    toks = [5, 6, 7]
    assert torch.equal(be.step(toks)[[0, 2]], twin.step(toks)[[0, 2]])
    assert torch.equal(be.logits[1], single.step(6))


def test_unfused_model_is_stepped_with_a_reason(dev):
    m = _model(dev, 64, fused=False)
    ids = _ids(m)
    a, b = _engine(m, 4), _engine(m, 4)
    for e in (a, b):
        e.prefill(ids[:64])
    a.prefill(ids[64:100], append=True)
    b.extend(ids[64:100])
    assert a.append_stats["stepped"] == 36 and a.append_stats["prefilled"] == 0 and isinstance(a.append_stats["reason"], str)
    assert a.position() == 100 and torch.equal(a.logits, b.logits)
    for li in range(2):
        assert torch.equal(a.k_cache[li], b.k_cache[li]) and torch.equal(a.v_cache[li], b.v_cache[li])


def test_overflow_raises_before_anything_runs(dev):
    m = _model(dev, 64)
    ids = _ids(m, 300)
    e = _engine(m, 4)
    e.prefill(ids[:70])
    kv = [(e.k_cache[li].clone(), e.v_cache[li].clone()) for li in range(2)]
    logits = e.logits.clone()
    with pytest.raises(RuntimeError, match="overflow"):
        e.prefill(ids[70:70 + CACHE_LEN - 69], append=True)
    assert e.position() == 70 and int(e.pos.item()) == 70 and torch.equal(e.logits, logits)
    for li in range(2):
        assert torch.equal(e.k_cache[li], kv[li][0]) and torch.equal(e.v_cache[li], kv[li][1])
