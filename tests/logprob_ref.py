"""The rule of mq_logprob_top (csrc/mq_logprob.hip's header) in numpy: the order exactly, the log-probabilities in
float64, and the kernel header's error bound evaluated for a row."""
import numpy as np

SLICE = 4096            # entries per slice of launch 1 (LP_SLICE): what one workgroup holds on chip
MAX_TOP = 20
U = 2.0 ** -24


def normalise(l):
    """Step 1: fp32 logits with NaN -> -inf and -0 -> +0."""
    l = np.asarray(l, dtype=np.float32).copy()
    l[np.isnan(l)] = -np.inf
    return l + np.float32(0)


def order(l):
    """Step 2: the indices of l' descending, ties by index ascending."""
    lp = normalise(l)
    return np.lexsort((np.arange(lp.size), -lp.astype(np.float64)))


def log_softmax64(l):
    """Step 3 in float64.  An all -inf row: every entry -inf.  A +inf logit: the c entries that are +inf share the mass (-log c each),
    every other entry is -inf."""
    x = normalise(l).astype(np.float64)
    m = x.max()
    if m == -np.inf:
        return np.full(x.size, -np.inf)
    if m == np.inf:
        top = x == np.inf
        return np.where(top, -np.log(float(top.sum())), -np.inf)
    with np.errstate(divide="ignore"):
        return (x - m) - np.log(np.exp(x - m).sum())


def logprob_ref(l, t, n_top):
    """(logprob float64, rank int, top_id int32 [n_top], top_logprob float64 [n_top]) of one row."""
    l = np.asarray(l, dtype=np.float32)
    V = l.size
    o = order(l)
    lp = log_softmax64(l)
    k = min(int(n_top), V)
    top_id = np.full(int(n_top), -1, dtype=np.int32)
    top_lp = np.full(int(n_top), -np.inf)
    top_id[:k], top_lp[:k] = o[:k], lp[o[:k]]
    if not 0 <= int(t) < V:
        return np.nan, 0, top_id, top_lp
    place = np.empty(V, dtype=np.int64)
    place[o] = np.arange(V)
    return lp[int(t)], int(place[int(t)]) + 1, top_id, top_lp


def bound(V, lp):
    """The kernel header's bound on |lp^ - lp| (expf and logf ASSUMED within 1 ulp): E_S + 2 u log V + 2 u |lp|, with
    E_S = 1.01 (u log V + 5 u + gamma_35)."""
    g35 = 35 * U / (1 - 35 * U)
    e_s = 1.01 * (U * np.log(V) + 5 * U + g35)
    return e_s + 2 * U * np.log(V) + 2 * U * np.abs(np.asarray(lp, dtype=np.float64))
