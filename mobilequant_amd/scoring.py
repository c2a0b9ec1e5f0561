"""Token scoring for llama.LlamaForCausalLM: per-token log-probabilities, lm-eval-style loglikelihoods and rolling-window perplexity.

The reference evaluates its simulated-quant model with lm-eval 0.3 (eval/harness_eval.py: `loglikelihood_rolling` for wikitext) and
eval/simple_eval.py (the argmax of the last position).  Here the model's trunk and final norm run as in forward(), and the fp32
lm_head is fused with its log-softmax (ops.score_head, csrc/mq_score.hip): the [tokens, vocab] logits are never materialised.

    token_logprobs(model, ids)                     -> (logprob, lse, argmax), each [B, S]
    loglikelihood(model, [(ctx, cont), ...])       -> [(sum log p(cont | ctx), is_greedy), ...]   (lm-eval 0.3 _loglikelihood_tokens)
    loglikelihood_rolling(model, ids)              -> sum log p over disjoint windows              (lm-eval 0.3 loglikelihood_rolling)
    perplexity(model, streams)                     -> Perplexity(ppl, sum_logprob, tokens)         (token level)

Token ids are plain lists of ints (or 1-D tensors); tokenizers and datasets stay with the caller.  Nothing here adds modules, buffers
or state to the model.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import ops

PAD_MULTIPLE = 64       # every scoring batch is right-padded to a multiple of this many positions (see loglikelihood)


def _plain_head(head) -> bool:
    w = getattr(head, "weight", None)
    return (type(head) is nn.Linear and w is not None and w.dtype == torch.float32 and w.is_cuda and w.shape[1] % 4 == 0
            and (head.bias is None or head.bias.dtype == torch.float32))


def _head(model, y: torch.Tensor, t: torch.Tensor):
    """(logprob, lse, argmax) of rows y [N, hidden] for targets t [N]: the fused kernel on a plain fp32 nn.Linear lm_head, the
    module's own logits and torch otherwise (a quantized or patched head)."""
    head = model.lm_head
    if _plain_head(head):
        return ops.score_head(y, head.weight, head.bias, t)
    logits = head(y).float()
    lse = torch.logsumexp(logits, -1)
    keep = t >= 0
    lp = torch.where(keep, logits.gather(1, t.clamp(min=0)[:, None])[:, 0] - lse, torch.zeros_like(lse))
    return lp, lse, torch.argmax(logits, -1)


@torch.no_grad()
def token_logprobs(model, ids: torch.Tensor, targets: Optional[torch.Tensor] = None):
    """ids [B, S] -> (logprob, lse, argmax), each [B, S]: log p(targets[b, s] | ids[b, :s + 1]), the log-sum-exp of the logits and
    their argmax (lowest index among ties) at every position.  targets default to the next token, the last position has none; a
    target < 0 means none.  Positions without a target are not run through the head: logprob 0, lse NaN, argmax -1 there."""
    if ids.dim() != 2:
        raise ValueError("token_logprobs: ids must be [B, S]")
    dev = model.embed_tokens.weight.device
    ids = ids.to(dev)
    B, S = ids.shape
    if targets is None:
        targets = torch.full((B, S), -1, dtype=torch.int64, device=dev)
        targets[:, :-1] = ids[:, 1:]
    else:
        targets = targets.to(device=dev, dtype=torch.int64)
        if targets.shape != ids.shape:
            raise ValueError("token_logprobs: targets must have the shape of ids")
    V = model.shape.vocab
    if bool((targets >= V).any()):
        raise ValueError(f"token_logprobs: a target lies outside the vocabulary [0, {V})")
    from .quantization import qmodule as Q
    y = Q._materialize(model.norm(model.hidden_states(ids)))
    y = y.reshape(B * S, -1)
    t = targets.reshape(-1)
    rows = torch.nonzero(t >= 0)[:, 0]
    logprob = torch.zeros(B * S, dtype=torch.float32, device=dev)
    lse = torch.full((B * S,), float("nan"), dtype=torch.float32, device=dev)
    amax = torch.full((B * S,), -1, dtype=torch.int64, device=dev)
    if rows.numel():
        lp, ls, am = _head(model, y.index_select(0, rows).contiguous(), t.index_select(0, rows))
        logprob[rows], lse[rows], amax[rows] = lp, ls, am
    return logprob.view(B, S), lse.view(B, S), amax.view(B, S)


def _ids(seq) -> List[int]:
    return seq.tolist() if isinstance(seq, torch.Tensor) else [int(v) for v in seq]


def request_rows(context: Sequence[int], continuation: Sequence[int], max_length: int) -> Tuple[List[int], List[int], int]:
    """lm-eval 0.3 _loglikelihood_tokens for one request: (inp, targets of the scored positions, first scored position).
    inp = (context + continuation)[-(max_length + 1):][:-1]; its last len(continuation) positions predict the continuation."""
    ctx, cont = _ids(context), _ids(continuation)
    if not cont:
        raise ValueError("loglikelihood: empty continuation")
    if not ctx:
        raise ValueError("loglikelihood: empty context (lm-eval passes the end-of-text token as the context of such a request)")
    if len(cont) > max_length:
        raise ValueError(f"loglikelihood: continuation of {len(cont)} tokens is longer than max_length {max_length}")
    whole = (ctx + cont)[-(max_length + 1):]
    inp = whole[:-1]
    return inp, cont, len(inp) - len(cont)


def batches_requests(model) -> bool:
    """True when every decoder layer runs fused (llama.fuse_decoder_layer): a row of that trunk does not depend on the other
    sequences of its batch.  The module chain's linears and matmuls do not promise that (their library kernels are chosen by the
    batch's shape), so there loglikelihood runs one request per forward."""
    return all("_mq_plain_forward" in layer.__dict__ and getattr(layer, "fused_mode", "auto") != "off" for layer in model.layers)


def _padded_len(n: int, limit: int) -> int:
    return min(-(-n // PAD_MULTIPLE) * PAD_MULTIPLE, limit)


@torch.no_grad()
def loglikelihood(model, requests, max_length: int = 2048, batch_size: int = 8) -> List[Tuple[float, bool]]:
    """requests: [(context_ids, continuation_ids), ...] -> [(sum log p(continuation | context), is_greedy), ...] in request order,
    with lm-eval 0.3 semantics (request_rows).  Requests are sorted by length and scored batch_size at a time, right-padded to a
    common length that is a multiple of 64 positions: under the causal mask padding never reaches a real position, and every batch
    takes the same trunk kernels (no M <= 8 decode-shaped launch), so a request's result does not depend on its batch mates.  A
    model whose layers are not all fused is scored one request per forward (batches_requests)."""
    dev = model.embed_tokens.weight.device
    if not batches_requests(model):
        batch_size = 1
    rows = [request_rows(c, x, max_length) for c, x in requests]
    order = sorted(range(len(rows)), key=lambda i: -len(rows[i][0]))
    out: List[Optional[Tuple[float, bool]]] = [None] * len(rows)
    for s in range(0, len(order), batch_size):
        chunk = order[s:s + batch_size]
        longest = max(len(rows[i][0]) for i in chunk)
        if longest > model.shape.max_pos:
            raise ValueError(f"loglikelihood: an input of {longest} tokens exceeds the model's max_pos {model.shape.max_pos}")
        L = _padded_len(longest, model.shape.max_pos)
        ids = torch.zeros(len(chunk), L, dtype=torch.int64)
        tg = torch.full((len(chunk), L), -1, dtype=torch.int64)
        for b, i in enumerate(chunk):
            inp, cont, p0 = rows[i]
            ids[b, :len(inp)] = torch.tensor(inp)
            tg[b, p0:p0 + len(cont)] = torch.tensor(cont)
        lp, _, am = token_logprobs(model, ids.to(dev), tg.to(dev))
        lp, am = lp.double().cpu(), am.cpu()
        for b, i in enumerate(chunk):
            inp, cont, p0 = rows[i]
            sl = slice(p0, p0 + len(cont))
            out[i] = (float(lp[b, sl].sum()), bool((am[b, sl] == torch.tensor(cont)).all()))
    return out


def rolling_windows(tokens: Sequence[int], max_length: int, prefix_token: int) -> List[Tuple[List[int], List[int]]]:
    """lm-eval 0.3 get_rolling_token_windows(context_len=1) + make_disjoint_window: (context, continuation) pairs that predict every
    token exactly once, the first from prefix_token, each window seeing at most max_length tokens."""
    toks = _ids(tokens)
    if max_length < 1:
        raise ValueError("rolling_windows: max_length must be >= 1")
    if not toks:
        return []
    pred_len = max_length                          # max_seq_len - context_len + 1
    first = min(max_length, len(toks))
    wins = [([prefix_token] + toks[:first - 1], toks[:first])]
    done = first
    while done < len(toks):
        n = min(len(toks) - done, pred_len)
        end = done + n
        wins.append((toks[max(end - max_length - 1, 0):end - 1], toks[end - n:end]))
        done += n
    return [(a[:len(a) - (len(b) - 1)], b) for a, b in wins]


@torch.no_grad()
def loglikelihood_rolling(model, ids, max_length: int = 2048, prefix_token: Optional[int] = None, batch_size: int = 8) -> float:
    """sum log p of every token of one stream, over disjoint windows of at most max_length tokens (rolling_windows).  prefix_token:
    the token the first window is conditioned on (lm-eval passes the end-of-text token); None: the stream's own first token is that
    context and is not predicted."""
    toks = _ids(ids)
    if prefix_token is None:
        if not toks:
            return 0.0
        prefix_token, toks = toks[0], toks[1:]
    wins = rolling_windows(toks, max_length, prefix_token)
    return float(sum(s for s, _ in loglikelihood(model, wins, max_length, batch_size)))


class Perplexity(NamedTuple):
    ppl: float
    sum_logprob: float
    tokens: int


@torch.no_grad()
def perplexity(model, streams, max_length: int = 2048, prefix_token: Optional[int] = None, batch_size: int = 8) -> Perplexity:
    """Token-level perplexity exp(-sum log p / N) over streams (each scored by loglikelihood_rolling; N = predicted tokens).  All
    streams' windows are batched together.  Word- and byte-level perplexity need the text: the caller divides sum_logprob itself."""
    wins: List[Tuple[List[int], List[int]]] = []
    for s in streams:
        toks = _ids(s)
        p = prefix_token
        if p is None:
            if not toks:
                continue
            p, toks = toks[0], toks[1:]
        wins += rolling_windows(toks, max_length, p)
    n = sum(len(c) for _, c in wins)
    total = float(sum(s for s, _ in loglikelihood(model, wins, max_length, batch_size))) if wins else 0.0
    return Perplexity(float(torch.exp(torch.tensor(-total / n, dtype=torch.float64))) if n else float("nan"), total, n)
