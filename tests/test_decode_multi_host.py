"""The multi-token decode step without a GPU: mq_decode_attention_multi is declared, exported and mirrored by its ctypes block, argument
blocks outside its limits are refused with MQ_EINVAL and a message before any HIP call, and the bookkeeping of a speculative round
(decode.spec_accept) and the prompt-lookup draft behave on synthetic rows.  (The barriers and the instantiations of its kernel,
mq_decode_rows.hip: tests/test_decode_rows_host.py.)  Pointers are fake, aligned and never dereferenced."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000          # a fake, 16-byte aligned device address


@pytest.fixture(scope="module")
def lib():
    from mobilequant_amd import _lib, build
    build.build()
    return _lib.load()


def _grid(on=True, qmax=255.0):
    from mobilequant_amd._lib import MqGrid
    return MqGrid(P, P, 0.0, qmax) if on else MqGrid(None, None, 0.0, 0.0)


def _args(rows=2, v_chunked=0, **kw):
    from mobilequant_amd._lib import MqDecodeAttentionArgs, MqDecodeAttentionMultiArgs
    a = MqDecodeAttentionArgs()
    a.qkv, a.k_cache, a.v_cache, a.cos, a.sin, a.pos, a.consts, a.out_q = P, P, P, P, P, P, P, P
    a.heads, a.kv_heads, a.head_dim, a.cache_len, a.rot_dim, a.nsplit = 8, 2, 64, 256, 64, 1
    a.qk_a, a.qk_b, a.pv_b, a.o_in = _grid(), _grid(), _grid(), _grid()
    a.pv_a, a.qk_out, a.pv_out = _grid(qmax=65535.0), _grid(qmax=65535.0), _grid()
    for k, v in kw.items():
        setattr(a, k, v)
    m = MqDecodeAttentionMultiArgs()
    m.a, m.rows, m.split_from, m.qkv_stride, m.v_chunked = a, rows, 768, (8 + 4) * 64, v_chunked
    return m


def _rejects(lib, args, text):
    rc = lib.mq_decode_attention_multi(ctypes.byref(args), None)
    msg = lib.mq_last_error()
    assert rc == 1, (rc, msg)                                   # MQ_EINVAL
    assert text.encode() in msg, msg


def test_entry_is_declared_exported_and_the_struct_matches_the_header(lib):
    from mobilequant_amd import _lib
    from mobilequant_amd._lib import MqDecodeAttentionArgs, MqDecodeAttentionMultiArgs
    assert "mq_decode_attention_multi" in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, "mq_decode_attention_multi")
    hdr = open(os.path.join(ROOT, "include", "mobilequant_amd.h")).read()
    assert re.search(r"int mq_decode_attention_multi\(const mq_decode_attention_multi_args\* args, mq_stream_t stream\);", hdr)
    assert lib.mq_version() // 100 == _lib.HEADER_MAJOR == 3
    fields = ("a", "rows", "split_from", "qkv_stride", "v_chunked")
    src = "\n".join(["#include <stddef.h>", "#include <stdio.h>", '#include "mobilequant_amd.h"', "int main(void) {",
                     '  printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(mq_decode_attention_multi_args), '
                     + ", ".join(f"offsetof(mq_decode_attention_multi_args, {f})" for f in fields) + ");", "  return 0;", "}"])
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        cc = next((x for x in ("cc", "gcc", "clang") if subprocess.run(["which", x], stdout=subprocess.PIPE).returncode == 0), None)
        if cc is None:
            cc = "/opt/rocm/llvm/bin/clang"
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    F = MqDecodeAttentionMultiArgs
    assert got == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in fields]
    assert F.rows.offset == ctypes.sizeof(MqDecodeAttentionArgs)


def test_rejects_argument_blocks_outside_the_limits(lib):
    assert lib.mq_decode_attention_multi(None, None) == 1 and b"null argument block" in lib.mq_last_error()
    for r in (0, 9, -1):
        _rejects(lib, _args(rows=r), "outside 1..8")
    _rejects(lib, _args(pos=None), "null pointer")
    _rejects(lib, _args(v_cache=None), "null pointer")
    _rejects(lib, _args(out_q=None), "null pointer")
    _rejects(lib, _args(head_dim=48), "head_dim=48")
    _rejects(lib, _args(cache_len=40000), "cache_len=40000")
    _rejects(lib, _args(cache_len=0), "cache_len=0")
    _rejects(lib, _args(v_chunked=1, cache_len=200), "cache_len % 16 == 0")
    _rejects(lib, _args(v_chunked=2), "v_chunked=2")
    _rejects(lib, _args(nsplit=4), "needs part and ticket")
    _rejects(lib, _args(nsplit=17, part=P, ticket=P), "nsplit=17")
    _rejects(lib, _args(k_cache=P + 8), "16-byte aligned")
    _rejects(lib, _args(prefetch_wgs=4), "prefetch")
    _rejects(lib, _args(pv_a=_grid(qmax=70000.0)), "at most 16 bits")
    m = _args(rows=3)
    m.qkv_stride = 64
    _rejects(lib, m, "qkv_stride")


# ---- the bookkeeping of a speculative round ------------------------------------------------------------------------------------
def test_accept_all_proposals_takes_the_bonus_row():
    from mobilequant_amd.decode import spec_accept
    assert spec_accept([4, 5, 6, 7], [4, 5, 6]) == ([4, 5, 6, 7], 3, False)
    assert spec_accept([9], []) == ([9], 0, False)               # no proposals: one token from row 0


def test_accept_none():
    from mobilequant_amd.decode import spec_accept
    assert spec_accept([1, 5, 6, 7], [4, 5, 6]) == ([1], 0, False)


@pytest.mark.parametrize("i", range(5))
def test_mismatch_at_each_index_ends_the_round_with_the_target_token(i):
    from mobilequant_amd.decode import spec_accept
    props = [10, 11, 12, 13, 14]
    rows = props[:i] + [99] + [0] * (5 - i)
    assert spec_accept(rows, props) == (props[:i] + [99], i, False)


def test_eos_inside_the_accepted_run_stops_at_it():
    from mobilequant_amd.decode import spec_accept
    assert spec_accept([4, 2, 6, 7], [4, 2, 6], eos=[2]) == ([4, 2], 2, True)
    assert spec_accept([4, 5, 6, 2], [4, 5, 6], eos={2, 3}) == ([4, 5, 6, 2], 3, True)      # EOS as the bonus token
    assert spec_accept([3, 5], [4], eos=[3]) == ([3], 0, True)                             # EOS as the disagreeing token


def test_budget_and_cache_end_cut_the_round():
    from mobilequant_amd.decode import spec_accept
    assert spec_accept([4, 5, 6, 7], [4, 5, 6], budget=2) == ([4, 5], 2, True)
    assert spec_accept([4, 5, 6, 7], [4, 5, 6], budget=1) == ([4], 1, True)
    assert spec_accept([4, 5, 6, 7], [4, 5, 6], room=3) == ([4, 5, 6], 3, True)
    assert spec_accept([4, 9, 6, 7], [4, 5, 6], budget=2) == ([4, 9], 1, True)             # the mismatch is also the last allowed token
    assert spec_accept([4, 5, 6, 7], [4, 5, 6], budget=4, room=5) == ([4, 5, 6, 7], 3, True)
    assert spec_accept([4, 5, 6, 7], [4, 5, 6], budget=5, room=5) == ([4, 5, 6, 7], 3, False)
    with pytest.raises(ValueError):
        spec_accept([4, 5], [4, 5, 6])


def test_prompt_lookup_draft():
    from mobilequant_amd.decode import prompt_lookup_draft
    d = prompt_lookup_draft(3)
    assert d([1, 2, 3, 4, 5, 9, 1, 2, 3], 4) == [4, 5, 9, 1]
    assert d([1, 2, 3, 4, 5, 9, 1, 2, 3], 1) == [4]
    assert d([1, 2, 3, 7, 1, 2, 3, 8, 1, 2, 3], 2) == [8, 1]        # the latest earlier occurrence
    assert d([1, 2, 3, 4], 3) == []                                  # no earlier occurrence
    assert d([1, 2, 3], 3) == [] and d([5, 5, 5, 5], 0) == []
    assert d([5, 5, 5, 5], 3) == [5]                                 # overlapping occurrence: what follows it
    assert prompt_lookup_draft(1)([7, 8, 7], 2) == [8, 7]
    with pytest.raises(ValueError):
        prompt_lookup_draft(0)
