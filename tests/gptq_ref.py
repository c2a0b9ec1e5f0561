"""GPTQ rounding (mq_gptq_round) restated in numpy from its contract, the float64 factor of the Hessian, and the case table of the GPU
test with its data generators.  A helper, not a test; numpy only.

Contract (include/mobilequant_amd.h).  For every row of w [N, K] independently, fp32, round to nearest:
    for t = 0 .. K-1:   k = perm[t], g = k // group_size
        q    = oracle.quantize_index(w[k], s[g], o[g], qmin, qmax)         IEEE divide, round_ste, fp32 add, clamp (NaN stays NaN)
        dq   = oracle.dequantize_index(q, s[g], o[g])
        e    = float32(float32(w[k] - dq) / u[t, t])
        loss += float64(e) * float64(e)                                    ascending t
        w[perm[t']] = oracle.fma_f32(-e, u[t, t'], w[perm[t']])            every t' > t: ONE fma each, in ascending t
    index[k] = (qmin if q is NaN else q) - qmin   (uint8),   w_deq[k] = dq
Because every element gets its updates as single fmas in ascending t, the kernel's blocking cannot change a bit: the comparison is
bit for bit, loss included (its float64 products are exact and the additions run in the same order).
"""
import functools
import os
import re

import numpy as np

from oracle import mq_oracle as O

F32, F64 = np.float32, np.float64

# ---- the launch constants of csrc/mq_gptq.hip (compared with the source by tests/test_gptq_host.py) ------------------------------------
STRIP = 64          # rows of a workgroup, one lane each
BLOCK = 32          # walk-order columns of the in-register chain
WAVES = 8           # waves of a workgroup
CHUNK = 16          # trailing walk positions a wave updates together (a last chunk may hold 4, 8 or 12)
TILE = 64           # the transposes' tile
SLICE = WAVES * CHUNK          # trailing columns the workgroup takes in one trip: past BLOCK + SLICE columns a wave makes a second trip
CONSTANTS = dict(GPTQ_STRIP=STRIP, GPTQ_BLOCK=BLOCK, GPTQ_WAVES=WAVES, GPTQ_CHUNK=CHUNK, GPTQ_TILE=TILE)
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mobilequant_amd", "csrc", "mq_gptq.hip")


def source_constants():
    """name -> value of every `constexpr int GPTQ_*` of the kernel source."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (GPTQ_[A-Z]+) = (\d+);", open(SOURCE).read())}


# ---- the contract ------------------------------------------------------------------------------------------------------------------------
def gptq_round(w, scale, offset, qmin, qmax, u, group_size, perm=None):
    """(index uint8 [N, K], w_deq fp32 [N, K], loss float64 [N]) by the contract above.  scale / offset [N, K // group_size]."""
    w = np.array(w, F32)
    N, K = w.shape
    scale, offset, u = np.asarray(scale, F32), np.asarray(offset, F32), np.asarray(u, F32)
    walk = np.arange(K) if perm is None else np.asarray(perm, np.int64)
    index = np.zeros((N, K), np.uint8)
    deq = np.zeros((N, K), F32)
    loss = np.zeros(N, F64)
    with np.errstate(all="ignore"):
        for t in range(K):
            k = int(walk[t])
            g = k // group_size
            q = O.quantize_index(w[:, k], scale[:, g], offset[:, g], qmin, qmax)
            dq = O.dequantize_index(q, scale[:, g], offset[:, g])
            e = ((w[:, k] - dq).astype(F32) / u[t, t]).astype(F32)
            loss += e.astype(F64) * e.astype(F64)
            index[:, k] = (np.where(np.isnan(q), F32(qmin), q) - F32(qmin)).astype(np.uint8)
            deq[:, k] = dq
            if t + 1 < K:
                later = walk[t + 1:]
                w[:, later] = O.fma_f32(-e[:, None], u[t, t + 1:][None, :], w[:, later])
    return index, deq, loss


def rtn(w, scale, offset, qmin, qmax, group_size):
    """(index uint8, w_deq) of round-to-nearest on the same grid."""
    w = np.asarray(w, F32)
    s, o = np.repeat(np.asarray(scale, F32), group_size, axis=1), np.repeat(np.asarray(offset, F32), group_size, axis=1)
    with np.errstate(all="ignore"):
        q = O.quantize_index(w, s, o, qmin, qmax)
        return (np.where(np.isnan(q), F32(qmin), q) - F32(qmin)).astype(np.uint8), O.dequantize_index(q, s, o)


def objective(w_deq, w, H):
    """tr(dW H dW^T) in float64."""
    d = np.asarray(w_deq, F64) - np.asarray(w, F64)
    return float(((d @ np.asarray(H, F64)) * d).sum())


def factor(H, percdamp=0.01, act_order=False, block=None):
    """The float64 factor gptq_factor is held to: (U fp32 [K, K], perm int32 | None, dead bool [K], cond of the damped H).
    block: H is block diagonal with blocks of this size (inputs correlated inside a block only): factored block by block."""
    H = np.array(H, F64)
    K = H.shape[0]
    d = np.diagonal(H).copy()
    dead = d == 0
    H[dead, dead] = 1.0
    perm = None
    if act_order:
        perm = np.argsort(-np.diagonal(H), kind="stable")
        H = H[perm][:, perm]
    H[np.arange(K), np.arange(K)] += percdamp * np.diagonal(H).mean()
    U = np.zeros((K, K), F64)
    cond = 0.0
    step = K if block is None or act_order else block
    for b in range(0, K, step):
        Hb = H[b:b + step, b:b + step]
        Hinv = np.linalg.inv(Hb)
        Hinv = (Hinv + Hinv.T) * 0.5
        U[b:b + step, b:b + step] = np.linalg.cholesky(Hinv).T          # Hinv = L L^T = U^T U with U = L^T upper
        cond = max(cond, float(np.linalg.cond(Hb))) if step <= 1024 else cond
    return U.astype(F32), (None if perm is None else perm.astype(np.int32)), dead, cond


# ---- data ------------------------------------------------------------------------------------------------------------------------------
def make_weight(N, K, seed, dist="t"):
    rng = np.random.default_rng(seed)
    if dist == "gauss":
        return (rng.standard_normal((N, K)) * 0.02).astype(F32)
    return (rng.standard_t(4, size=(N, K)) * 0.02).astype(F32)


def make_hessian(K, seed, tokens=None, block=None):
    """2 X^T X / T float64 of seeded correlated heavy-tailed inputs X [T, K]: Student-t(5) sources mixed by a banded matrix plus a dense
    one, channel scales two decades wide.  block: the inputs are correlated inside blocks of this many channels only -- H is block
    diagonal, assembled from one such matrix per block."""
    if block is not None and block < K:
        H = np.zeros((K, K), F64)
        for b in range(0, K, block):
            H[b:b + block, b:b + block] = make_hessian(block, seed + 1 + b, tokens)
        return H
    rng = np.random.default_rng(seed + 17)
    T = min(tokens or max(2 * K, 256), 2048)
    z = rng.standard_t(5, size=(T, K))
    mix = np.eye(K)
    for d, c in ((1, 0.6), (2, 0.35), (5, 0.2)):
        mix += c * np.eye(K, k=d) + 0.5 * c * np.eye(K, k=-d)
    mix += 0.15 * rng.standard_normal((K, K)) / np.sqrt(K)
    ch = np.exp(rng.uniform(np.log(0.1), np.log(10.0), size=K))
    X = (z @ mix) * ch[None, :]
    return 2.0 * (X.T @ X) / T


def grid_from_minmax(w, bits, sym, group_size, clip=1.0):
    """scale / offset fp32 [N, G] from the groups' min / max times `clip` (clip < 1: a clipped range, the rows saturate the clamp)."""
    N, K = w.shape
    x = np.where(np.isnan(w), F32(0), w).reshape(N, K // group_size, group_size)
    mn, mx = (x.min(axis=2) * F32(clip)).astype(F32), (x.max(axis=2) * F32(clip)).astype(F32)
    s, o, qmin, qmax = O.scale_offset_from_min_max(mn, mx, bits, sym)
    return s, o, qmin, qmax


# ---- the GPU test's cases ------------------------------------------------------------------------------------------------------------------
# Switches of the kernel: N against STRIP (a partly filled strip, one strip, two, three); K against BLOCK (no full block, exactly one,
# one and a short one, several); K - BLOCK against SLICE (waves with no trailing chunk, one trip, a second trip) and CHUNK (a short last
# chunk); group_size against
# BLOCK (below, equal, above, == K); the transposes' TILE (K and G on both sides of it); perm (the chain's columns cross groups).
def _case(N, K, g, bits, sym, perm=False, clip=1.0, dead=False, nan=False, block=None, dist="t"):
    return dict(N=N, K=K, g=K if g == -1 else g, bits=bits, sym=sym, perm=perm, clip=clip, dead=dead, nan=nan, block=block, dist=dist)


CASES = (
    _case(1, 16, 16, 4, False),                         # K < BLOCK: the short chain alone, one lane
    _case(63, 32, 8, 4, True),                          # exactly one block, groups below the block
    _case(64, 36, 4, 3, False, perm=True),              # one block and a short one of 4 columns; the finest group
    _case(65, 64, 32, 4, False, perm=True),             # two strips; group == BLOCK; perm crosses groups inside a block
    _case(130, 64, 16, 2, True),                        # three strips, the last holds 2 rows
    _case(5, 60, 20, 2, False),                         # K - BLOCK = 28: two chunks, the second of 12 columns; six waves have none
    _case(3, 64, -1, 8, True, perm=True),               # group_size == K; two full chunks
    _case(7, 68, 68, 8, False),                         # a last chunk of 4 columns; K past the TILE
    _case(64, 128, 64, 4, False, clip=0.6),             # group above the block; rows saturate the clamp
    _case(9, 160, 32, 4, True, perm=True, clip=0.7),    # K - BLOCK == SLICE: every wave one chunk
    _case(4, 164, 4, 4, False, perm=True),              # K - BLOCK = SLICE + 4: wave 0 makes a second trip, for a chunk of 4 columns
    _case(6, 256, 128, 3, False, perm=True, dead=True),   # a dead column (zero Hessian diagonal, zeroed weight column)
    _case(5, 136, 8, 4, False, nan=True),               # one NaN row between clean rows; a last chunk of 8 columns
    _case(5, 96, 32, 4, True, perm=True, nan=True),
    _case(2, 272, 4, 3, True),                          # G = 68 groups: the grid's transpose past one tile
    _case(3, 1024, 128, 4, False, perm=True),           # the largest K of the table
    _case(2, 4096, 128, 4, False, block=1024),          # wide: inputs correlated inside blocks of 1024 channels
)


def case_id(c):
    return (f"{c['N']}x{c['K']}-g{c['g']}-w{c['bits']}{'s' if c['sym'] else 'a'}" + ("-perm" if c["perm"] else "")
            + (f"-clip{c['clip']}" if c["clip"] != 1.0 else "") + ("-dead" if c["dead"] else "") + ("-nan" if c["nan"] else ""))


def case_seed(c):
    return 100 * c["K"] + 7 * c["N"] + c["bits"] + (3 if c["sym"] else 0)


def case_inputs(c):
    """dict(w, scale, offset, qmin, qmax, u, perm, H, dead) of a case, numpy; w already has its dead columns zeroed."""
    seed = case_seed(c)
    N, K, g = c["N"], c["K"], c["g"]
    w = make_weight(N, K, seed, c["dist"])
    H = make_hessian(K, seed, block=c["block"])
    if c["dead"]:
        k = K // 3
        H[k, :] = 0.0
        H[:, k] = 0.0
    u, perm, dead, _ = factor(H, 0.01, c["perm"], block=c["block"])
    w[:, dead] = 0.0
    if c["nan"]:
        w[N // 2, K // 4] = np.nan
    s, o, qmin, qmax = grid_from_minmax(w, c["bits"], c["sym"], g, c["clip"])
    return dict(w=w, scale=s, offset=o, qmin=qmin, qmax=qmax, u=u, perm=perm, H=H, dead=dead)


@functools.lru_cache(maxsize=None)
def _inputs(i):
    d = case_inputs(CASES[i])
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def inputs(i):
    """The inputs of CASES[i]: computed once per process, shared, read-only."""
    return _inputs(i)


@functools.lru_cache(maxsize=None)
def _reference(i):
    d = inputs(i)
    out = gptq_round(d["w"], d["scale"], d["offset"], d["qmin"], d["qmax"], d["u"], CASES[i]["g"], d["perm"])
    for v in out:
        v.setflags(write=False)
    return out


def reference(i):
    """(index, w_deq, loss) of CASES[i] by the contract: computed once per process, shared, read-only."""
    return _reference(i)


# ---- the model-level tests' toy (torch imported on use) --------------------------------------------------------------------------------
TOY_CFG = dict(bitwidth=4, group_size=64, is_symmetric=False, is_per_channel=True)
TOY_LINEARS = 14


def toy_model(seed=0):
    """The two-block hidden-128 toy LM of the W4A16 test, float, on the CPU."""
    from mobilequant_amd.llama import LlamaForCausalLM, LlamaShape
    m = LlamaForCausalLM(LlamaShape.toy()).eval()
    m.reset_parameters(0.08, seed=seed)
    return m


def toy_calib_ids():
    """Calibration batches: 4 x [2, 64] token ids (512 tokens: more than any linear has input channels)."""
    import torch
    rng = np.random.default_rng(11)
    return [torch.from_numpy(rng.integers(0, 97, size=(2, 64))) for _ in range(4)]
