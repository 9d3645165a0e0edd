"""tests/setops_model.py on three hand-written pairs with literal expected results: a stored 0, a wrap at 2^32 and its saturating
twin. The GPU tests compare kmi_index_compare / kmi_index_combine with this model, so the model is checked on its own first."""
from tests import index_model as M
from tests import oracle as orc
from tests import setops_model as SM


def _model(pairs, saturating=False):
    m = M.CountModel(31, orc.DNA, orc.SINGLE, saturating=saturating)
    m.d = {(key,): c for key, c in pairs.items()}
    return m


def _d(model):
    return {key[0]: c for key, c in model.d.items()}


def test_plain_pair():
    a, b = _model({1: 5, 2: 3, 3: 7, 4: 1}), _model({2: 4, 3: 2, 5: 9})
    o = SM.overlap(a, b)
    assert [o[w] for w in SM.WORDS] == [4, 3, 2, 16, 15, 10, 6, 5]
    assert o["jaccard"] == 2 / 5 and o["containment_a"] == 0.5 and o["containment_b"] == 2 / 3 and o["weighted_jaccard"] == 5 / 26
    assert _d(SM.combined(a, b, "union_add")) == {1: 5, 2: 7, 3: 9, 4: 1, 5: 9}
    assert _d(SM.combined(a, b, "union_max")) == {1: 5, 2: 4, 3: 7, 4: 1, 5: 9}
    assert _d(SM.combined(a, b, "intersect_min")) == {2: 3, 3: 2}
    assert _d(SM.combined(a, b, "intersect_add")) == {2: 7, 3: 9}
    assert _d(SM.combined(a, b, "intersect_left")) == {2: 3, 3: 7}
    assert _d(SM.combined(a, b, "subtract_keys")) == {1: 5, 4: 1}
    assert _d(SM.combined(a, b, "subtract_counts")) == {1: 5, 3: 5, 4: 1}
    assert _d(a) == {1: 5, 2: 3, 3: 7, 4: 1} and _d(b) == {2: 4, 3: 2, 5: 9}   # the operands are not touched


def test_stored_zero_is_present():
    a, b = _model({10: 0, 11: 6, 12: 2}), _model({10: 3, 11: 0, 13: 0})
    o = SM.overlap(a, b)
    assert [o[w] for w in SM.WORDS] == [3, 3, 2, 8, 3, 6, 3, 0]
    assert o["weighted_jaccard"] == 0.0 and o["jaccard"] == 0.5
    assert _d(SM.combined(a, b, "union_add")) == {10: 3, 11: 6, 12: 2, 13: 0}
    assert _d(SM.combined(a, b, "union_max")) == {10: 3, 11: 6, 12: 2, 13: 0}
    assert _d(SM.combined(a, b, "intersect_min")) == {10: 0, 11: 0}
    assert _d(SM.combined(a, b, "intersect_left")) == {10: 0, 11: 6}
    assert _d(SM.combined(a, b, "subtract_keys")) == {12: 2}            # 11 is in b although its count there is 0
    assert _d(SM.combined(a, b, "subtract_counts")) == {11: 6, 12: 2}   # 11 stays: 6 > 0; 10 leaves: 0 > 3 fails
    empty = _model({})
    assert [SM.overlap(empty, b)[w] for w in SM.WORDS] == [0, 3, 0, 0, 3, 0, 0, 0] and SM.overlap(empty, empty)["jaccard"] == 0.0
    assert _d(SM.combined(a, empty, "subtract_counts")) == {11: 6, 12: 2}   # a's own stored 0 leaves against an empty b
    assert _d(SM.combined(a, empty, "intersect_min")) == {} and _d(SM.combined(empty, b, "union_max")) == {10: 3, 11: 0, 13: 0}


def test_wrap_and_its_saturating_twin():
    pa, pb = {20: 4_000_000_000, 21: 7}, {20: 1_000_000_000, 21: 4_294_967_295}
    a, b = _model(pa), _model(pb)
    assert _d(SM.combined(a, b, "union_add")) == {20: 705_032_704, 21: 6}
    assert _d(SM.combined(a, b, "intersect_add")) == {20: 705_032_704, 21: 6}
    sat = _model(pa, saturating=True)
    assert _d(SM.combined(sat, b, "union_add")) == {20: 4_294_967_295, 21: 4_294_967_295}
    assert _d(SM.combined(sat, b, "intersect_add")) == {20: 4_294_967_295, 21: 4_294_967_295}
    assert SM.combined(sat, b, "union_add").saturating
    o = SM.overlap(a, b)   # the sums are 64-bit, never clamped
    assert o["sum_a"] == 4_000_000_007 and o["sum_b"] == 5_294_967_295 and o["sum_min_shared"] == 1_000_000_007
    assert _d(SM.combined(a, b, "subtract_counts")) == {20: 3_000_000_000} and _d(SM.combined(a, b, "union_max")) == {20: 4_000_000_000, 21: 4_294_967_295}
