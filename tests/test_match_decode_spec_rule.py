"""Which kernel family decodes a model with a match-model leaf (include/w3hip.h "which kernels decode"): w3_decode_spec_covers keeps
answering for default options — the lane kernels — and w3_decode_spec_covers_variant / Context.decode_spec_covers(model, variant=...)
answers under the variant bits: with decode_match_spec (W3_OPT_VARIANT bit 4096) the sixteen-lane decoder takes such a model wherever
the rest of it is covered.  Host only: no device."""
import pytest

import weath3rb0i_amd as w3
from weath3rb0i_amd import _lib as L

BIT = ("decode_match_spec",)


def covers(model, variant=()):
    return w3.Context.decode_spec_covers(model, variant=variant)


def _tree_leaf_in_the_middle():
    return w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.MatchModel(3, 12)), w3.Order1())


WITH_LEAF = {
    "MatchModel": w3.MatchModel,
    "order012_match_mix": w3.order012_match_mix,
    "full_cm_match_mix": w3.full_cm_match_mix,
    "tree_leaf_in_the_middle": _tree_leaf_in_the_middle,
}


def test_the_bit_and_the_export_exist():
    assert L.W3_VAR_DECODE_MATCH_SPEC == 4096
    assert w3.Context.variant_bits(BIT) == 4096 and w3.Context.variant_bits(BIT + ("decode_lane",)) == 4096 | 1024
    assert L.load().w3_abi_version() == 8   # an additive export


@pytest.mark.parametrize("name", sorted(WITH_LEAF))
def test_a_model_with_the_leaf_is_covered_only_under_the_bit(name):
    m = WITH_LEAF[name]
    assert covers(m()) is False
    assert covers(m(), variant=BIT) is True
    assert covers(m(), variant=BIT + ("decode_lane",)) is False      # decode_lane still wins
    assert covers(m(), variant=("aoh_decode_spec",)) is False        # another family's bit changes nothing


def test_what_the_rest_of_the_spec_refuses_stays_refused_under_the_bit():
    one = w3.order012_match_mix(select=w3.LogisticMixer.ONE)
    align1 = w3.BestOfTwoModel(w3.OrderN(12, 1), w3.MatchModel())
    align2 = w3.BestOfTwoModel(w3.OrderN(12, 2), w3.MatchModel())
    three = w3.APM(w3.APM(w3.APM(w3.MatchModel(), w3.APM.ORDER0, 7), w3.APM.ORDER1, 6), w3.APM.ORDER0, 5)
    two = w3.APM(w3.APM(w3.MatchModel(), w3.APM.ORDER0, 7), w3.APM.ORDER1, 6)
    frozen = w3.BestOfTwoModel(w3.Order0(), w3.FrozenModel(w3.MatchModel()))   # (a frozen match leaf: no MatchState is ever formed)
    for m in (one, align1, three, frozen):
        assert covers(m) is False and covers(m, variant=BIT) is False
    for m in (align2, two):
        assert covers(m) is False and covers(m, variant=BIT) is True


def test_models_without_the_leaf_answer_the_same_with_and_without_the_bit():
    models = [w3.Order0(), w3.order012_mix(), w3.full_cm_mix(), w3.full_cm(), w3.order012_mix(select=w3.LogisticMixer.ONE),
              w3.BestOfTwoModel(w3.OrderN(12, 1), w3.Order1()), w3.BestOfTwoModel(w3.Order0(), w3.OrderN(27, 3)),
              w3.APM(w3.APM(w3.APM(w3.Order0(), w3.APM.ORDER0, 7), w3.APM.ORDER1, 6), w3.APM.ORDER0, 5)]
    for m in models:
        assert covers(m) == covers(m, variant=BIT)
        assert covers(m, variant=("decode_lane",)) is False
    assert covers(models[1]) is True and covers(models[4]) is False and covers(models[5]) is False
