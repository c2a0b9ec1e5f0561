"""The three rules of beam search restated for the tests: mq_beam_select's rule in numpy (exact), the simultaneous
cache assignment of mq_decode_cache_reorder with torch indexing on clones, and generate_beam's host rule over a logits callback."""
import numpy as np

import logprob_ref

NEG_INF = np.float32(-np.inf)


# ---- rule A: the group's best candidates -----------------------------------------------------------------------------------------------
def row_list(l, m, log_s, K):
    """A member row's list by steps 1 - 3 of mq_logprob_top's rule, given the row's m and logf(S) (read from mq_logprob_top's own
    output for that row: m = l'[top_id[0]], logf(S) = -top_logprob[0]; that kernel is pinned by tests/test_gpu_logprob.py).  Everything
    here is one IEEE fp32 operation per value: d_i = (l'_i == m) ? 0 : l'_i - m and lp_i = d_i - logf(S).
    An all -inf (or NaN) row has m = -inf: every lp is -inf and the order is 0, 1, ...  A +inf logit makes m = +inf: the entries that
    are +inf have d = 0 and lp = -logf(c), every other entry has d = -inf and lp = -inf.  Returns (token ids, lp fp32), min(K, V) each."""
    lp_ = logprob_ref.normalise(l)
    o = logprob_ref.order(l)[:K]
    x = lp_[o]
    m, log_s = np.float32(m), np.float32(log_s)
    if m == NEG_INF:
        return o.astype(np.int32), np.full(o.size, NEG_INF, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        d = np.where(x == m, np.float32(0), x - m).astype(np.float32)
        lp = (d - log_s).astype(np.float32)
    return o.astype(np.int32), lp


def score(cum, lp):
    """A candidate's score: ONE fp32 addition; a NaN cum counts as -inf, -0 as +0, a NaN sum (cum = +inf, lp = -inf) as -inf."""
    c = np.float32(cum)
    c = NEG_INF if np.isnan(c) else c
    with np.errstate(invalid="ignore"):
        s = np.float32(c + np.float32(lp))
    return NEG_INF if np.isnan(s) else np.float32(s + np.float32(0))


def select(lists, cum, group, n_groups, K):
    """lists[r]: row r's (ids, lp) from row_list, or None for a row that is a member of nothing.  Returns (score fp32, row, token,
    logprob fp32) arrays [n_groups][K]: per group s descending, ties by r ascending, then by k ascending; padded with -inf, -1, -1, -inf."""
    sc = np.full((n_groups, K), NEG_INF, dtype=np.float32)
    row = np.full((n_groups, K), -1, dtype=np.int32)
    tok = np.full((n_groups, K), -1, dtype=np.int32)
    lpo = np.full((n_groups, K), NEG_INF, dtype=np.float32)
    for g in range(n_groups):
        cands = []
        for r, lst in enumerate(lists):
            if lst is None or int(group[r]) != g:
                continue
            for k, (t, lp) in enumerate(zip(*lst)):
                cands.append((-float(score(cum[r], lp)), r, k, int(t), np.float32(lp)))
        cands.sort(key=lambda c: c[:3])
        for j, (ns, r, k, t, lp) in enumerate(cands[:K]):
            sc[g, j], row[g, j], tok[g, j], lpo[g, j] = np.float32(-ns), r, t, lp
    return sc, row, tok, lpo


def member(g, n_groups):
    return 0 <= int(g) < n_groups


def lse64(l):
    """m + log(S) of a row in float64 (-inf for an all -inf row, +inf with a +inf logit)."""
    x = logprob_ref.normalise(l).astype(np.float64)
    m = x.max()
    if not np.isfinite(m):
        return m
    return m + np.log(np.exp(x - m).sum())


# ---- rule B: the simultaneous assignment over the slots --------------------------------------------------------------------------------
def reorder_rule(caches, pos, parent, L):
    """Slot d takes [0, pos[p]) of every head from p = parent[d] AS IT WAS BEFORE THE CALL iff 0 <= p < batch, p != d and 0 < pos[p] < L.
    Everything else keeps its bytes.  caches: torch tensors [B, H, L, D]; returns new tensors."""
    out = [c.clone() for c in caches]
    B = len(pos)
    for d in range(B):
        p = parent[d]
        if not 0 <= p < B or p == d or not 0 < pos[p] < L:
            continue
        for o, c in zip(out, caches):                              # (c: the bytes from before the call, whatever o has become)
            o[d, :, :pos[p]] = c[p, :, :pos[p]]
    return out


# ---- the host rule ---------------------------------------------------------------------------------------------------------------------
class _Finished:
    def __init__(self, W):
        self.W, self.items, self.n = W, [], 0

    def add(self, ids, s, sc):
        self.items.append((sc, self.n, list(ids), s))
        self.n += 1
        worst = max(range(len(self.items)), key=lambda i: (-self.items[i][0], self.items[i][1]))
        if len(self.items) > self.W:                               # drops the worst; on equal scores the earlier entry stays
            del self.items[worst]

    def ranked(self):
        return sorted(self.items, key=lambda e: (-e[0], e[1]))


def beam_search(lister, prompt, max_new_tokens, W, eos=(), length_penalty=1.0, early_stopping=True, num_return_sequences=1):
    """generate_beam's host rule for ONE prompt.  lister(ids, K) -> (token ids, lp fp32) is the first-K list (rule A's row_list) of
    the logits row behind the sequence ids: the only thing the rule knows about the model.  K = max(2, 1 + |eos|) W.
    L = the new tokens of a hypothesis once the current token is appended.  Per step the candidates of the live beams (beam b's k-th
    entry scores cum_b + lp: one fp32 addition) are ordered by score descending, beam ascending, k ascending, and the first K are
    walked: an EOS at j >= W is skipped; an EOS at j < W finishes (ids + EOS, s) with score s / L ** length_penalty; any other becomes
    a next beam until W are taken.  The finished list keeps the best W (the earlier entry stays on equal scores).  Done iff W are
    finished and (early_stopping or worst finished score >= best candidate score / L ** length_penalty).  At max_new_tokens the live
    beams of a prompt that is not done are added in beam order.
    Returns (sequences, scores, sum_logprobs, parents) with parents[step] = the parent beam of each next beam."""
    eos = set(int(t) for t in eos)
    K = max(2, 1 + len(eos)) * W
    prompt = [int(t) for t in prompt]
    beams = [([], np.float32(0))]
    fin = _Finished(W)
    parents = []
    for step in range(max_new_tokens):
        L = step + 1
        norm = float(L) ** float(length_penalty)
        cands = []
        for b, (ids, cum) in enumerate(beams):
            toks, lps = lister(prompt + ids, K)
            for k, (t, lp) in enumerate(zip(toks, lps)):
                cands.append((-float(score(cum, lp)), b, k, int(t)))
        cands.sort(key=lambda c: c[:3])
        cands = cands[:K]
        nxt = []
        for j, (ns, b, k, t) in enumerate(cands):
            s = np.float32(-ns)
            if t in eos:
                if j < W:
                    fin.add(beams[b][0] + [t], float(s), float(s) / norm)
                continue
            nxt.append((b, t, s))
            if len(nxt) == W:
                break
        done = len(fin.items) >= W and (early_stopping or min(e[0] for e in fin.items) >= -cands[0][0] / norm)
        if not done and L == max_new_tokens:
            for b, t, s in nxt:
                fin.add(beams[b][0] + [t], float(s), float(s) / norm)
            done = True
        if done:
            break
        assert len(nxt) == W
        parents.append([b for b, _, _ in nxt])
        beams = [(beams[b][0] + [t], s) for b, t, s in nxt]
    best = fin.ranked()[:num_return_sequences]
    return [prompt + e[2] for e in best], [e[0] for e in best], [e[3] for e in best], parents
