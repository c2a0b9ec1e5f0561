"""The gated-activation kernels (mq_activation.hip) against each other: every route evaluates one gate chain, so they agree bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    import mobilequant_amd._lib as L
    assert L.device_info()["arch"].startswith("gfx950")
    return torch.device("cuda:0")


@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_gate_chain_routes_agree_bit_for_bit(dev, act):
    """act(a) * b -> w2's int8 input image through every route: the workgroup-per-row kernel on indices, the wave-per-row kernel on
    indices (want_y) and on values (with and without want_y), and the 256 x 256 table with its lookup.  The same expression on the same
    operands: no tolerance, no excluded share.  [5, 2064]: a ragged last wave of the wave-per-row kernel (4 rows per workgroup), more
    than one 1024-element trip of it and more than one 2048-element trip of the row kernel; row 0 starts with all 256 indices in
    order.  va = (ia - oa) * sa as a separate subtract and multiply in torch gives the kernels' dequant bits.  With b = 1 the product
    is the QSiLU / QGELU output itself: mq_act_quant's chain."""
    from mobilequant_amd import ops
    import mobilequant_amd as mq

    def grid(lo, hi):
        q = mq.Quantizer(mq.QuantConfig(bitwidth=8))
        q.set_scale_offset_from_minmax(lo, hi, "buffer", dev)
        return (q.scale.detach(), q.offset.detach(), q.qmin, q.qmax)
    ga, gb, gmid, gact, gout = grid(-3.0, 2.5), grid(-2.0, 3.0), grid(0.0, 1.0), grid(-0.3, 2.5), grid(-4.0, 5.0)
    mid = gmid if act == "silu" else None
    gen = torch.Generator().manual_seed(20240607)
    a_idx = torch.randint(0, 256, (5, 2064), generator=gen, dtype=torch.uint8)
    b_idx = torch.randint(0, 256, (5, 2064), generator=gen, dtype=torch.uint8)
    a_idx[0, :256] = torch.arange(256, dtype=torch.uint8)
    b_idx[0, :256] = torch.arange(256, dtype=torch.uint8)
    a_idx, b_idx = a_idx.to(dev), b_idx.to(dev)
    va = (a_idx.float() - ga[1]) * ga[0]
    vb = (b_idx.float() - gb[1]) * gb[0]
    kw = dict(mid_grid=mid, act_grid=gact, q_shift=128)

    q_row, rs_row = ops.gated_act_quant(a_idx, b_idx, act, gout, a_grid=ga[:2], b_grid=gb[:2], **kw)
    q_wave, rs_wave, y_wave = ops.gated_act_quant(a_idx, b_idx, act, gout, a_grid=ga[:2], b_grid=gb[:2], want_y=True, **kw)
    q_val, rs_val = ops.gated_act_quant(va, vb, act, gout, **kw)
    q_valy, rs_valy, y_val = ops.gated_act_quant(va, vb, act, gout, want_y=True, **kw)
    q_tab, rs_tab = ops.gated_lookup(a_idx, b_idx, ops.gated_table(act, gout, ga[:2], gb[:2], mid_grid=mid, act_grid=gact, q_shift=128))
    for name, q, rs in (("index, wave per row", q_wave, rs_wave), ("values", q_val, rs_val), ("values, want_y", q_valy, rs_valy),
                        ("table lookup", q_tab, rs_tab)):
        assert torch.equal(q, q_row), name
        assert torch.equal(rs, rs_row), name
    assert torch.equal(y_wave, y_val)

    y_one = ops.gated_act_quant(va, torch.ones_like(va), act, gout, want_y=True, **kw)[2]
    assert torch.equal(y_one, ops.act_quant(va, act, in_grid=None, mid_grid=mid, out_grid=gact))
