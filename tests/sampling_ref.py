"""CPU reference of the selection rule of csrc/mq_sample.hip: a numpy Philox4x32-10 and the rule with every
transcendental in float64.  The device's expf / logf are not numpy's, so `analyse` also says whether a draw is DECIDABLE (the winner's
margin and the nucleus boundary are wider than what fp32 library functions can move) and which tokens form the boundary band."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 words -> 4 uint32 arrays.  Random123's philox4x32-10: ten rounds of
    (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0) with (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2, the key bumped by (W0, W1) between rounds."""
    c = [np.asarray(x, dtype=np.uint64) & U32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & U32, p1 >> np.uint64(32), p1 & U32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(W0)) & U32, (k1 + np.uint64(W1)) & U32
    return [x.astype(np.uint32) for x in c]


def uniforms(seed, stream, n, idx):
    """u_i of the rule (fp32, exact) for vocabulary entries idx at (seed, stream, n)."""
    idx = np.asarray(idx, dtype=np.int64)
    r = philox4x32_10([np.asarray(n, dtype=np.int64) & 0xFFFFFFFF, idx >> 2, int(stream) & 0xFFFFFFFF, (int(stream) >> 32) & 0xFFFFFFFF],
                      [int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF])
    r = np.stack(r, axis=-1)
    pick = np.take_along_axis(r, (idx & 3)[..., None], axis=-1)[..., 0]
    u = ((pick >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert u.dtype == np.float32
    return u


def gumbel64(u):
    return -np.log(-np.log(u.astype(np.float64)))


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def candidate_order(z):
    """indices by z descending, ties by index ascending (z fp32, -0 == +0)."""
    return np.argsort(-z.astype(np.float64), kind="stable")


def analyse(logits, temperature, top_k, top_p, min_p, seed, stream, n):
    """The rule on one row.  Returns a dict: token, C (sorted indices), decidable, band (indices that may fall on either side on the
    device), kept_lo / kept_hi (|C without the band|, |C with it|)."""
    l = np.asarray(logits, dtype=np.float32)
    V = l.shape[0]
    lz = np.where(np.isnan(l), np.float32(-np.inf), l)
    if temperature == 0:
        tok = int(np.argmax(lz)) if np.any(lz > -np.inf) else 0
        return dict(token=tok, C=np.array([tok]), decidable=True, band=np.array([], dtype=np.int64), kept_lo=1, kept_hi=1, allowed=np.array([tok]))
    with np.errstate(over="ignore"):
        z = (lz / np.float32(temperature)).astype(np.float32) + np.float32(0.0)
    zmax = z.max()
    if zmax == -np.inf:
        return dict(token=0, C=np.array([0]), decidable=True, band=np.array([], dtype=np.int64), kept_lo=0, kept_hi=0, allowed=np.array([0]))
    order = candidate_order(z)
    k = V if (top_k == 0 or top_k >= V) else int(top_k)
    K = order[:k]
    d32 = (z - zmax).astype(np.float32)                                # fp32 subtract, as the rule
    w = np.floor(np.exp(d32.astype(np.float64)) * 2.0 ** 32)           # exact integers in float64 (<= 2^32)
    wK = w[K]
    WK = float(wK.sum())                                               # < 2^53: exact
    cum_before = np.concatenate(([0.0], np.cumsum(wK)[:-1]))
    band = np.zeros(V, dtype=bool)
    if np.float32(top_p) < 1:
        thr = float(np.ceil(float(np.float32(top_p)) * WK))
        npfx = int(np.searchsorted(cum_before + wK, thr, side="left")) + 1       # shortest prefix with sum >= thr
        P = K[:npfx]
        near = np.abs(cum_before - thr) <= 2.0 ** -20 * WK                       # cumulative mass before the token within 2^-20 W_K of the threshold
        band[K[near]] = True
    else:
        P = K
    u = uniforms(seed, stream, n, np.arange(V))
    g = gumbel64(u)
    finite = z > -np.inf
    delta = 64 * ulp32(float(np.abs(z[finite]).max()) + float(np.abs(g).max()))
    if np.float32(min_p) > 0:
        lm = float(np.log(np.float64(np.float32(min_p))))
        passes = (d32.astype(np.float64) >= lm)
        passes[order[0]] = True
        inP = np.zeros(V, dtype=bool)
        inP[P] = True
        C = np.flatnonzero(inP & passes)
        band |= np.abs(d32.astype(np.float64) - lm) <= delta
        band[order[0]] = False
    else:
        C = np.sort(P)
    inC = np.zeros(V, dtype=bool)
    inC[C] = True
    inK = np.zeros(V, dtype=bool)
    inK[K] = True
    band &= inK                                                         # a token outside the top-k set is never a candidate
    score = z.astype(np.float64) + g
    sc = np.where(inC, score, -np.inf)
    tok = int(np.argmax(sc))
    rest = sc.copy()
    rest[tok] = -np.inf
    # the runner-up among C plus the band (a band token may be admitted on the device)
    alt = np.where(inC | band, score, -np.inf)
    alt[tok] = -np.inf
    runner = int(np.argmax(alt))
    margin = sc[tok] - alt[runner]
    decidable = bool(margin > delta) and not band[tok] and not (np.isfinite(alt[runner]) and band[runner])
    allowed = np.flatnonzero(inC | band)
    return dict(token=tok, C=C, decidable=decidable, band=np.flatnonzero(band), kept_lo=int((inC & ~band).sum()),
                kept_hi=int((inC | band).sum()), allowed=allowed, margin=float(margin), delta=delta)


def restricted_softmax(logits, temperature, top_k, top_p, min_p):
    """Exact probabilities (float64) of the rule's draw: softmax(z) over C, 0 elsewhere."""
    a = analyse(logits, temperature, top_k, top_p, min_p, 0, 0, 0)
    z = (np.asarray(logits, dtype=np.float32) / np.float32(temperature)).astype(np.float32).astype(np.float64)
    p = np.zeros(len(z))
    e = np.exp(z[a["C"]] - z.max())
    p[a["C"]] = e / e.sum()
    return p
