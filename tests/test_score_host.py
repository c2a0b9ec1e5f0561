"""Host side of token scoring (mobilequant_amd/scoring.py, mq_score_head): lm-eval 0.3 window and request bookkeeping, the C-ABI
argument checks (no GPU: every check fails before any HIP call), and the kernel source against the barrier audit."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _windows(n, max_length, prefix=0):
    from mobilequant_amd.scoring import rolling_windows
    return rolling_windows(list(range(1, n + 1)), max_length, prefix)


def test_rolling_windows_match_the_lm_eval_example():
    assert _windows(10, 4) == [([0], [1, 2, 3, 4]), ([4], [5, 6, 7, 8]), ([6, 7, 8], [9, 10])]


@pytest.mark.parametrize("max_length", [1, 4, 7, 64])
@pytest.mark.parametrize("extra", ["empty", "short", "equal", "one_more", "two_and_three"])
def test_rolling_windows_predict_every_token_once_from_at_most_max_length_tokens(max_length, extra):
    n = {"empty": 0, "short": max(max_length - 1, 1), "equal": max_length, "one_more": max_length + 1,
         "two_and_three": 2 * max_length + 3}[extra]
    toks = list(range(1, n + 1))
    wins = _windows(n, max_length)
    if n == 0:
        assert wins == []
        return
    assert [t for _, c in wins for t in c] == toks                       # every token predicted exactly once, in order
    stream = [0] + toks
    for ctx, cont in wins:
        assert ctx and cont and len(ctx) + len(cont) - 1 <= max_length    # the model input is at most max_length tokens
        start = stream.index(cont[0]) - len(ctx)
        assert stream[start:start + len(ctx) + len(cont)] == ctx + cont   # the context is the tokens right in front
    assert wins[0] == ([0], toks[:min(max_length, n)])
    if n > max_length:                                                    # later windows carry the full max_length input
        assert all(len(c) + len(x) - 1 == max_length for c, x in wins[1:])


def test_request_rows_follow_lm_eval_truncation():
    from mobilequant_amd.scoring import request_rows
    inp, cont, p0 = request_rows([1, 2, 3], [4, 5], 8)
    assert (inp, cont, p0) == ([1, 2, 3, 4], [4, 5], 2)                 # positions 2, 3 predict 4, 5
    inp, cont, p0 = request_rows(list(range(1, 11)), [11, 12], 4)
    assert (inp, cont, p0) == ([8, 9, 10, 11], [11, 12], 2)             # (ctx + cont)[-(4 + 1):][:-1]
    inp, cont, p0 = request_rows([7], [1, 2, 3, 4], 4)
    assert (inp, cont, p0) == ([7, 1, 2, 3], [1, 2, 3, 4], 0)
    for bad in (([], [1]), ([1], []), ([1], [1, 2, 3, 4, 5])):
        with pytest.raises(ValueError):
            request_rows(*bad, 4)


def test_padding_bookkeeping_keeps_every_batch_at_a_multiple_of_64():
    from mobilequant_amd.scoring import PAD_MULTIPLE, _padded_len
    assert PAD_MULTIPLE == 64
    assert [_padded_len(n, 2048) for n in (1, 63, 64, 65, 2047, 2048)] == [64, 64, 64, 128, 2048, 2048]
    assert _padded_len(100, 96) == 96                                     # never past the model's position tables


def test_score_head_argument_checks_fail_before_any_launch():
    from mobilequant_amd import _lib as L
    lib = L.load()
    p = ctypes.c_void_p(0x10000)
    s = ctypes.c_void_p(0x20000)
    need = lib.mq_score_head_scratch_bytes(300, 1003)
    assert need >= 3 * 300 * 8 * 4 + 300 * 4 and need % 256 == 0
    assert lib.mq_score_head_scratch_bytes(4, 0) < 0
    ok = dict(y=p, ld=128, w=p, b=None, t=p, M=300, K=128, V=1003, s=s, nb=need, lp=p, lse=p, am=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mq_score_head(a["y"], a["ld"], a["w"], a["b"], a["t"], a["M"], a["K"], a["V"], a["s"], a["nb"], a["lp"], a["lse"], a["am"], None)
    for name in ("y", "w", "s", "lp", "lse", "am"):
        assert call(**{name: None}) == 1 and b"null pointer" in lib.mq_last_error(), name
    assert call(V=0) == 1 and b"V must be" in lib.mq_last_error()
    assert call(V=-5) == 1
    for K in (0, 2, 130, 1 << 20):
        assert call(K=K) == 1 and b"K must be" in lib.mq_last_error(), K
    assert call(ld=64) == 1 and b"y_stride" in lib.mq_last_error()
    assert call(y=ctypes.c_void_p(0x10004)) == 1 and b"aligned" in lib.mq_last_error()
    assert call(s=ctypes.c_void_p(0x20010)) == 1 and b"aligned" in lib.mq_last_error()
    assert call(nb=need - 1) == 1 and b"scratch_bytes" in lib.mq_last_error()
    assert call(M=-1) == 1
    assert lib.mq_score_head(None, 0, None, None, None, 0, 0, 0, None, 0, None, None, None, None) == 0      # M = 0: a no-op


def test_score_head_wrapper_refuses_host_tensors():
    import torch
    from mobilequant_amd import ops
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        ops.score_head(torch.zeros(4, 8), torch.zeros(16, 8), None, None)


def test_score_kernel_passes_the_barrier_audit(tmp_path):
    """The new source under tools/barrier_audit.py (test_cabi.py's audit covers a fixed list of files): no s_barrier with LDS
    traffic in flight on any path."""
    from mobilequant_amd import build
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    asm = str(tmp_path / "mq_score.s")
    r = subprocess.run([build.HIPCC, *flags, "-w", "--cuda-device-only", "-S", os.path.join(ROOT, "mobilequant_amd", "csrc", "mq_score.hip"),
                        "-o", asm], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "barrier_audit.py"), asm], stdout=subprocess.PIPE, text=True).stdout
    assert "PENDING" not in rep and "possibly in flight 0" in rep, rep
    assert "v_mfma_f32_32x32x2_f32" in open(asm).read()
