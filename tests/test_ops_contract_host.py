"""CPU: ops_contract_cases.py held to mobilequant_amd/ops.py -- every public wrapper has an entry (or stands in the exempt or predicate
list, or is a re-export of another module's function), every entry's operand list covers the wrapper's signature, and every valid call of the table builds, addresses
real arguments and has the element counts the table states.  A wrapper added without an entry, an entry that loses an operand, or a
case whose sizes drift from its operands fails here, without a GPU."""
import inspect
import os
import sys
import typing

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ops_contract_cases as C  # noqa: E402
from mobilequant_amd import ops  # noqa: E402

PUBLIC = sorted(n for n, f in vars(ops).items() if inspect.isfunction(f) and not n.startswith("_"))


def test_the_table_names_every_public_wrapper_once():
    groups = {"WRAPPERS": [w.name for w in C.WRAPPERS], "EXEMPT": list(C.EXEMPT), "PREDICATES": list(C.PREDICATES), "REEXPORTED": list(C.REEXPORTED)}
    listed = [n for names in groups.values() for n in names]
    assert len(listed) == len(set(listed)), "a name stands in two lists: %r" % sorted(n for n in set(listed) if listed.count(n) > 1)
    assert sorted(listed) == PUBLIC, "without an entry: %r; no such wrapper: %r" % (sorted(set(PUBLIC) - set(listed)), sorted(set(listed) - set(PUBLIC)))
    assert set(C.EXEMPT) == {"decode_gemv_grouped", "decode_attention_multi", "decode_attention_ragged", "decode_cache_table", "decode_cache_fork",
                             "decode_cache_reorder", "beam_select"}, "the exemptions are the struct pass-throughs and the cache / beam wrappers, no others"
    # a re-export is exempt only while it IS one: a function that ops.py defines itself needs an entry
    for name in C.REEXPORTED:
        assert getattr(ops, name).__module__ != ops.__name__, "%s is defined in ops.py: it needs an entry" % name
    for name in set(PUBLIC) - set(C.REEXPORTED):
        assert getattr(ops, name).__module__ == ops.__name__, "%s is re-exported from %s" % (name, getattr(ops, name).__module__)


def _takes_tensor(annotation):
    if annotation is torch.Tensor:
        return True
    return any(_takes_tensor(a) for a in typing.get_args(annotation))


@pytest.mark.parametrize("w", C.WRAPPERS, ids=lambda w: w.name)
def test_operands_cover_the_signature(w):
    """Every parameter is an operand root (tensors, grid tuples and dicts included) or a declared scalar, never both; a parameter annotated
    as a tensor is an operand; paths are unique."""
    hints = typing.get_type_hints(getattr(ops, w.name))
    params = list(inspect.signature(getattr(ops, w.name)).parameters)
    roots = {o.path[0] for o in w.operands}
    assert roots.isdisjoint(w.scalars), (w.name, roots & set(w.scalars))
    assert sorted(roots | set(w.scalars)) == sorted(params), "%s: not in the table: %r; not in the signature: %r" % (
        w.name, sorted(set(params) - roots - set(w.scalars)), sorted((roots | set(w.scalars)) - set(params)))
    for p in params:
        if _takes_tensor(hints.get(p)):
            assert p in roots, "%s: %s is annotated as a tensor and listed as a scalar" % (w.name, p)
    assert len({o.path for o in w.operands}) == len(w.operands)
    for o in w.operands:
        assert o.kind in ("conv", "layout", "raw", "inplace", "out") and o.dtype and all(d in C.NP for d in o.dtype), (w.name, o)


@pytest.mark.parametrize("w", C.WRAPPERS, ids=lambda w: w.name)
def test_cases_build_and_match_their_operands(w):
    """Every case passes only parameters of the signature; every operand is passed by at least one case; an operand's array has a
    documented dtype and the element count its expression gives; scale and offset of every grid differ (a pointer mix-up shows)."""
    params = set(inspect.signature(getattr(ops, w.name)).parameters)
    assert w.cases and len({c.id for c in w.cases}) == len(w.cases)
    seen = set()
    for c in w.cases:
        b = c.build()
        assert set(b.args) <= params, (w.name, c.id, set(b.args) - params)
        arrays = {}
        for o in w.operands:
            try:
                v = C.lookup(b.args, o.path)
            except (KeyError, IndexError, TypeError):
                continue
            if v is None:
                continue
            assert isinstance(v, np.ndarray), (w.name, c.id, o.path, type(v))
            seen.add(o.path)
            arrays[o.path] = v
            assert v.dtype in [np.dtype(C.NP[d]) for d in o.dtype], (w.name, c.id, o.path, v.dtype)
            if o.numel is not None:
                assert v.size == C.sizes_numel(o.numel, b.sizes), (w.name, c.id, o.path, v.size, o.numel, b.sizes)
        # no array of the call is left out of the operand list
        def walk(v, path):
            if isinstance(v, np.ndarray):
                assert path in arrays, "%s %s: the array at %r is no operand of the table" % (w.name, c.id, path)
            elif isinstance(v, dict):
                for k, x in v.items():
                    walk(x, path + (k,))
            elif isinstance(v, (tuple, list)):
                for k, x in enumerate(v):
                    walk(x, path + (k,))
        walk(b.args, ())
        for ps, po in C.grid_pairs(w):
            if ps in arrays and po in arrays and arrays[ps].size == arrays[po].size:
                assert not np.array_equal(arrays[ps].astype(np.float64), arrays[po].astype(np.float64)), (w.name, c.id, ps, po, "scale equals offset")
    assert seen == {o.path for o in w.operands}, "%s: no case passes %r" % (w.name, sorted({o.path for o in w.operands} - seen))


def test_gemm_case_shapes_come_from_the_dispatch_predicates():
    import gemm_cases as G
    M, N, K = C.FR128
    assert G.fr128_shape(M, N, K) and not G.tiled_supported(M, N, K)
    assert not any(G.fr128_shape(M, n, k) for n in range(64, N, 16) for k in (K,)) and not G.fr128_shape(M, N, K - 256)
