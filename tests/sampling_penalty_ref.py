"""CPU reference of step 0 of the selection rule (csrc/mq_sample.hip): repetition, presence and frequency penalties and
a logit bias from the sequence's own token history, in numpy fp32.  Every line of `transform` is ONE np.float32 operation (numpy has no
fused multiply-add), in the rule's order.  Its result goes to tests/sampling_ref.py as the row's logits."""
import numpy as np

PROMPT_BIT = np.uint32(1 << 31)
COUNT_MASK = np.uint32(0xFFFF)


def transform(logits, history, repetition=1.0, presence=0.0, frequency=0.0, bias=None):
    """l3 of step 0 for one row: logits fp32 [V], history uint32 [V] (bit 31: in the prompt, bits 0..15: times generated), bias None or
    fp32 [V].  A repetition that is not finite and > 0 counts as 1.  The neutral request returns the logits' own bits."""
    l = np.asarray(logits, dtype=np.float32)
    h = np.asarray(history, dtype=np.uint32)
    r, a, f = np.float32(repetition), np.float32(presence), np.float32(frequency)
    if not (r > 0 and r < np.inf):
        r = np.float32(1.0)
    if r == 1 and a == 0 and f == 0 and bias is None:
        return l.copy()
    c = h & COUNT_MASK
    with np.errstate(all="ignore"):
        l1 = np.where(h != 0, np.where(l > 0, l / r, l * r), l)
        t = f * c.astype(np.float32)
        t = t + np.where(c > 0, a, np.float32(0.0))
        l2 = l1 - t
        l3 = l2 + np.asarray(bias, dtype=np.float32) if bias is not None else l2
    assert l3.dtype == np.float32
    return l3


def observe(history, token):
    """The drawn token's count rises by one, saturating at 65 535; in place."""
    if (history[token] & COUNT_MASK) != COUNT_MASK:
        history[token] += np.uint32(1)


def prompt_history(V, ids, history=None):
    """A history with bit 31 set for every id (on top of `history`, or of a cleared one)."""
    h = np.zeros(V, dtype=np.uint32) if history is None else history
    for i in ids:
        h[int(i)] |= PROMPT_BIT
    return h


def dense_bias(V, logit_bias):
    """SamplingParams.logit_bias (pairs or mapping) as the dense fp32 row the kernel reads; None stays None."""
    if logit_bias is None:
        return None
    b = np.zeros(V, dtype=np.float32)
    for t, v in (logit_bias.items() if hasattr(logit_bias, "items") else logit_bias):
        b[int(t)] = np.float32(v)
    return b
