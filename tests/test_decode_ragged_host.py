"""Ragged decode steps without a GPU: the plan packer of BatchDecodeEngine.step_tokens (decode.plan_rows), the row budget of a batched
speculative round (decode.spec_row_budget), and mq_decode_attention_ragged as a C entry -- declared, exported, mirrored by its ctypes
block, argument blocks outside its limits refused with MQ_EINVAL and a message before any HIP call.  (The barriers and the instantiations of
its kernel, mq_decode_rows.hip: tests/test_decode_rows_host.py.)  Pointers are fake, aligned and never dereferenced."""
import ctypes
import itertools
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000          # a fake, 16-byte aligned device address


# ---- the plan packer ---------------------------------------------------------------------------------------------------------------
def test_plan_rows_orders_slots_and_keeps_their_rows_contiguous():
    from mobilequant_amd.decode import plan_rows
    pos = [5, 700, None, 64]
    plan = plan_rows({3: [30, 31, 32, 33], 0: [7, 8, 9], 1: [11]}, pos, 8, 1024)      # (given out of order)
    assert plan.row_seq == [0, 0, 0, 1, 3, 3, 3, 3]
    assert plan.row_pos == [5, 6, 7, 700, 64, 65, 66, 67]
    assert plan.row_tok == [7, 8, 9, 11, 30, 31, 32, 33]
    assert plan.spans == {0: (0, 3), 1: (3, 1), 3: (4, 4)}
    # one slot, one row; one slot, every row
    assert plan_rows({1: [4]}, pos, 8, 1024) == ([1], [700], [4], {1: (0, 1)})
    p8 = plan_rows({3: range(8)}, pos, 8, 1024)
    assert p8.row_seq == [3] * 8 and p8.row_pos == list(range(64, 72)) and p8.spans == {3: (0, 8)}
    # equal positions on different slots are two runs
    assert plan_rows({0: [1], 1: [2]}, [9, 9], 8, 16).row_pos == [9, 9]
    # a slot that ends exactly at the cache end
    assert plan_rows({0: [1, 2]}, [14], 8, 16).row_pos == [14, 15]


def test_plan_rows_tables_make_one_run_per_slot():
    """What mq_decode_attention_ragged asks of its caller: over random plans every slot's rows are one stretch of consecutive rows at
    consecutive positions, and no slot appears in two stretches."""
    import random
    from mobilequant_amd.decode import plan_rows
    rnd = random.Random(3)
    for _ in range(200):
        B = rnd.randint(1, 8)
        pos = [rnd.randint(0, 90) for _ in range(B)]
        slots = rnd.sample(range(B), rnd.randint(1, B))
        counts = {b: 1 for b in slots}
        for _ in range(rnd.randint(0, 8 - len(slots))):
            counts[rnd.choice(slots)] += 1
        plan = plan_rows({b: [rnd.randint(0, 99) for _ in range(c)] for b, c in counts.items()}, pos, 8, 100)
        assert [k for k, _ in itertools.groupby(plan.row_seq)] == sorted(slots)
        for b, (r0, c) in plan.spans.items():
            assert c == counts[b] and plan.row_seq[r0:r0 + c] == [b] * c and plan.row_pos[r0:r0 + c] == list(range(pos[b], pos[b] + c))
        assert sum(c for _, c in plan.spans.values()) == len(plan.row_tok) <= 8


def test_plan_rows_refusals():
    from mobilequant_amd.decode import plan_rows
    pos = [5, None, 12]
    with pytest.raises(ValueError, match="outside 1..8"):
        plan_rows({}, pos, 8, 16)
    with pytest.raises(ValueError, match="outside 1..8"):
        plan_rows({0: [1] * 5, 2: [1] * 4}, pos, 8, 32)
    with pytest.raises(ValueError, match="outside 1..4"):
        plan_rows({0: [1] * 5}, pos, 4, 32)                          # (an engine whose shape lowered max_rows)
    with pytest.raises(ValueError, match="no tokens"):
        plan_rows({0: [1], 2: []}, pos, 8, 16)
    for bad in (3, -1):
        with pytest.raises(ValueError, match="outside 0..2"):
            plan_rows({bad: [1]}, pos, 8, 16)
    with pytest.raises(RuntimeError, match="idle"):
        plan_rows({1: [1]}, pos, 8, 16)
    with pytest.raises(RuntimeError, match="overflow"):
        plan_rows({2: [1] * 5}, pos, 8, 16)                          # 12 + 5 > 16
    assert plan_rows({2: [1] * 4}, pos, 8, 16).row_pos == [12, 13, 14, 15]


# ---- the speculative row budget ----------------------------------------------------------------------------------------------------
def test_spec_row_budget():
    from mobilequant_amd.decode import spec_row_budget
    big = [100]
    assert spec_row_budget(4, 8, big, big) == [4]                    # one live slot: num_draft binds
    assert spec_row_budget(7, 8, big, big) == [7] and spec_row_budget(9, 8, big, big) == [7]
    assert spec_row_budget(4, 8, big * 2, big * 2) == [3, 3]         # 8 // 2 - 1
    assert spec_row_budget(4, 8, big * 3, big * 3) == [1, 1, 1]      # 8 // 3 - 1
    assert spec_row_budget(4, 8, big * 4, big * 4) == [1] * 4
    for L in (5, 6, 7, 8):
        assert spec_row_budget(4, 8, big * L, big * L) == [0] * L    # eight live slots: plain steps
    assert spec_row_budget(4, 8, [100, 3, 1], [100, 100, 100]) == [1, 1, 0]      # tokens still allowed - 1
    assert spec_row_budget(4, 8, [100, 2], [2, 1]) == [1, 0]         # cache room - 1
    assert spec_row_budget(0, 8, big, big) == [0]
    assert spec_row_budget(4, 4, big * 2, big * 2) == [1, 1]         # a lowered max_rows
    assert spec_row_budget(4, 8, [], []) == []
    with pytest.raises(ValueError):
        spec_row_budget(-1, 8, big, big)
    with pytest.raises(ValueError):
        spec_row_budget(4, 8, [1, 2], [1])


def test_spec_row_budget_never_exceeds_max_rows():
    from mobilequant_amd.decode import spec_row_budget
    for max_rows in range(1, 9):
        for L in range(1, max_rows + 1):
            for nd in (0, 1, 4, 7, 100):
                for allowed, room in (([100] * L, [100] * L), ([1] * L, [100] * L), (list(range(1, L + 1)), list(range(L, 0, -1)))):
                    ks = spec_row_budget(nd, max_rows, allowed, room)
                    assert len(ks) == L and all(0 <= k <= nd for k in ks)
                    assert L + sum(ks) <= max_rows, (max_rows, L, nd, ks)
                    assert all(k + 1 <= max(a, 1) and k + 1 <= max(r, 1) for k, a, r in zip(ks, allowed, room))


# ---- the C entry -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mobilequant_amd import _lib, build
    build.build()
    return _lib.load()


def _grid(on=True, qmax=255.0):
    from mobilequant_amd._lib import MqGrid
    return MqGrid(P, P, 0.0, qmax) if on else MqGrid(None, None, 0.0, 0.0)


def _args(rows=2, batch=4, **kw):
    from mobilequant_amd._lib import MqDecodeAttentionArgs, MqDecodeAttentionRaggedArgs
    a = MqDecodeAttentionArgs()
    a.qkv, a.k_cache, a.v_cache, a.cos, a.sin, a.consts, a.out_q = P, P, P, P, P, P, P      # (a.pos stays null: it is not read)
    a.heads, a.kv_heads, a.head_dim, a.cache_len, a.rot_dim, a.nsplit = 8, 2, 64, 256, 64, 1
    a.qk_a, a.qk_b, a.pv_b, a.o_in = _grid(), _grid(), _grid(), _grid()
    a.pv_a, a.qk_out, a.pv_out = _grid(qmax=65535.0), _grid(qmax=65535.0), _grid()
    for k, v in kw.items():
        setattr(a, k, v)
    m = MqDecodeAttentionRaggedArgs()
    m.a, m.rows, m.batch, m.split_from, m.qkv_stride, m.row_seq, m.row_pos = a, rows, batch, 768, (8 + 4) * 64, P, P
    return m


def _rejects(lib, args, text):
    rc = lib.mq_decode_attention_ragged(ctypes.byref(args), None)
    msg = lib.mq_last_error()
    assert rc == 1, (rc, msg)                                   # MQ_EINVAL
    assert text.encode() in msg, msg


def test_entry_is_declared_exported_and_the_struct_matches_the_header(lib):
    from mobilequant_amd import _lib, ops
    from mobilequant_amd._lib import MqDecodeAttentionArgs, MqDecodeAttentionRaggedArgs
    assert "mq_decode_attention_ragged" in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, "mq_decode_attention_ragged") and callable(ops.decode_attention_ragged)
    hdr = open(os.path.join(ROOT, "include", "mobilequant_amd.h")).read()
    assert re.search(r"int mq_decode_attention_ragged\(const mq_decode_attention_ragged_args\* args, mq_stream_t stream\);", hdr)
    assert lib.mq_version() // 100 == _lib.HEADER_MAJOR
    fields = ("a", "rows", "batch", "split_from", "qkv_stride", "row_seq", "row_pos")
    src = "\n".join(["#include <stddef.h>", "#include <stdio.h>", '#include "mobilequant_amd.h"', "int main(void) {",
                     '  printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(mq_decode_attention_ragged_args), '
                     + ", ".join(f"offsetof(mq_decode_attention_ragged_args, {f})" for f in fields) + ");", "  return 0;", "}"])
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        cc = next((x for x in ("cc", "gcc", "clang") if subprocess.run(["which", x], stdout=subprocess.PIPE).returncode == 0), None)
        if cc is None:
            cc = "/opt/rocm/llvm/bin/clang"
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    F = MqDecodeAttentionRaggedArgs
    assert got == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in fields]
    assert F.rows.offset == ctypes.sizeof(MqDecodeAttentionArgs)


def test_ragged_refuses_a_null_block_and_zero_rows_before_any_launch(lib):
    """Bad argument blocks are rejected by the entry itself (MQ_EINVAL + mq_last_error), before any HIP call: checkable without a GPU."""
    assert lib.mq_decode_attention_ragged(None, None) == 1 and b"mq_decode_attention_ragged: null argument block" in lib.mq_last_error()
    _rejects(lib, _args(rows=0), "rows=0 outside 1..8")


def test_ragged_rejects_argument_blocks_outside_the_limits(lib):
    for r in (9, -1):
        _rejects(lib, _args(rows=r), "rows=%d outside 1..8" % r)
    for b in (0, 9, -1):
        _rejects(lib, _args(batch=b), "batch=%d outside 1..8" % b)
    for name in ("row_seq", "row_pos"):
        m = _args()
        setattr(m, name, None)
        _rejects(lib, m, "null row table")
    _rejects(lib, _args(v_cache=None), "null pointer")
    _rejects(lib, _args(out_q=None), "null pointer")
    _rejects(lib, _args(head_dim=48), "head_dim=48")
    _rejects(lib, _args(cache_len=40000), "cache_len=40000")
    _rejects(lib, _args(cache_len=0), "cache_len=0")
    _rejects(lib, _args(nsplit=4), "needs part and ticket")
    _rejects(lib, _args(nsplit=17, part=P, ticket=P), "nsplit=17")
    _rejects(lib, _args(k_cache=P + 8), "16-byte aligned")
    _rejects(lib, _args(prefetch_wgs=4), "prefetch")
    _rejects(lib, _args(pv_a=_grid(qmax=70000.0)), "at most 16 bits")
    m = _args(rows=3)
    m.qkv_stride = 64
    _rejects(lib, m, "qkv_stride")

