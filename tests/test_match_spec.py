"""The match-model leaf's spec rules (include/w3hip.h, W3_HIST_MATCH) through w3_spec_validate and the Python mirror: no device needed."""
import ctypes as C

import pytest

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L


def _spec(*nodes):
    s = L.ModelSpec()
    s.n_nodes = len(nodes)
    for i, (kind, bits, align, max_bits, extra) in enumerate(nodes):
        nd = L.Node()
        nd.kind, nd.bits, nd.align, nd.max_bits = kind, bits, align, max_bits
        for k, v in extra.items():
            setattr(nd, k, v)
        s.nodes[i] = nd
    return L.load().w3_spec_validate(C.byref(s))


def M(m=4, log_slots=16, bits=11, align=3, **extra):
    return (L.W3_NODE_ORDERN, bits, align, m, dict(history=L.W3_HIST_MATCH, log_cells=log_slots, **extra))


O0, O1 = (L.W3_NODE_ORDERN, 11, 3, 0, {}), (L.W3_NODE_ORDERN, 19, 3, 0, {})
SL = (L.W3_NODE_SLOT_STATE, 2, 0, 0, {"log_cells": 10})
BO2, APM0, APM1 = (L.W3_NODE_BEST_OF_TWO, 0, 0, 0, {}), (L.W3_NODE_APM, 0, 0, 7, {}), (L.W3_NODE_APM, 0, 1, 6, {})


def MIX(n):
    return (L.W3_NODE_MIX, n, L.W3_MIX_ORDER0, 14, {})


def test_the_leaf_is_an_ordern_leaf_like_any_other():
    assert L.W3_HIST_MATCH == 4
    assert _spec(M()) == 0
    for m in (2, 3, 4):
        for log_slots in (8, 12, 20):
            assert _spec(M(m, log_slots)) == 0
    assert _spec(O0, M(), BO2) == 0 and _spec(M(), O0, BO2, O1, BO2) == 0             # under BestOfTwo
    assert _spec(O0, O1, M(), MIX(3)) == 0 and _spec(M(), SL, MIX(2), APM0, APM1) == 0  # under a MIX, APM stages behind
    assert _spec(M(), APM0, APM1) == 0
    assert _spec(M(frozen=1)) == 0 and _spec(O0, M(frozen=1), BO2) == 0                # frozen


def test_values_outside_the_definition_are_invalid():
    for m in (0, 1, 5, 8, 255):
        assert _spec(M(m)) == L.W3_E_INVALID, m
    for log_slots in (0, 7, 21, 24, 255):
        assert _spec(M(4, log_slots)) == L.W3_E_INVALID, log_slots
    assert _spec(M(1, 7)) == L.W3_E_INVALID
    assert _spec((L.W3_NODE_ORDERN, 11, 3, 4, {"history": 5, "log_cells": 16})) == L.W3_E_INVALID   # no such history


def test_valid_shapes_that_are_not_built_are_unsupported():
    for bits, align in ((12, 3), (10, 3), (19, 3), (11, 2), (11, 0), (11, 4)):
        assert _spec(M(bits=bits, align=align)) == L.W3_E_UNSUPPORTED, (bits, align)
    assert _spec(M(), M(), BO2) == L.W3_E_UNSUPPORTED                    # a second match leaf
    assert _spec(M(2, 8), O0, M(4, 16), MIX(3)) == L.W3_E_UNSUPPORTED
    assert _spec(M(), M(frozen=1), BO2) == L.W3_E_UNSUPPORTED
    # out-of-range values come first: a spec that is both is invalid
    assert _spec(M(5, 16, bits=12)) == L.W3_E_INVALID


def test_the_python_mirror():
    s = w3.MatchModel().spec()
    nd = s.nodes[0]
    assert (s.n_nodes, nd.kind, nd.bits, nd.align, nd.history, nd.max_bits, nd.log_cells, nd.frozen) == (1, L.W3_NODE_ORDERN, 11, 3, L.W3_HIST_MATCH, 4, 16, 0)
    nd = w3.OrderNEntropy(11, 3, w3.MatchHistory(2, 8)).spec().nodes[0]
    assert (nd.max_bits, nd.log_cells) == (2, 8)
    s = w3.order012_match_mix().spec()
    assert s.n_nodes == 5 and s.nodes[3].history == L.W3_HIST_MATCH and s.nodes[4].kind == L.W3_NODE_MIX and s.nodes[4].bits == 4
    s = w3.full_cm_match_mix().spec()
    assert s.n_nodes == 11 and s.nodes[7].history == L.W3_HIST_MATCH and s.nodes[8].bits == 8 and s.nodes[3].log_cells == 14
    assert w3.full_cm_match_mix(log_cells=8).spec().nodes[3].log_cells == 8
    assert w3.FrozenModel(w3.MatchModel()).spec().nodes[0].frozen == 1
    for model, code in ((w3.MatchModel(5, 16), L.W3_E_INVALID), (w3.MatchModel(4, 21), L.W3_E_INVALID),
                        (w3.OrderNEntropy(19, 3, w3.MatchHistory()), L.W3_E_UNSUPPORTED),
                        (w3.BestOfTwoModel(w3.MatchModel(), w3.MatchModel()), L.W3_E_UNSUPPORTED)):
        with pytest.raises(w3.W3Error) as e:
            model.spec()
        assert e.value.code == code
    # the sixteen-lane decoder does not take the leaf
    assert w3.Context.decode_spec_covers(w3.order012_mix()) and not w3.Context.decode_spec_covers(w3.order012_match_mix())
    assert not w3.Context.decode_spec_covers(w3.MatchModel()) and not w3.Context.decode_spec_covers(w3.full_cm_match_mix())
    assert "match_ms" in [f for f, _ in L.Timing._fields_]
    assert L.load().w3_abi_version() == 8 and C.sizeof(L.Node) == 24
