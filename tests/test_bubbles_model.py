"""The plain-Python model of bubble popping (tests/bubbles_model.py; the definition is in include/kmerind_hip.h) on the cleaning
pipeline's input, on hand-made bubbles and on random small graphs. No GPU: the GPU tests compare the library with this model."""
import numpy as np
import pytest

from tests import bubbles_model as B
from tests import dbg_clean_model as D
from tests import unitig_model as M


def _summary(nodes, t=1):
    u = M.unitigs_from_strings(nodes, t)
    return len(u), D.n50([len(s) for s, _, _ in u])


def _pruned(reads, k, t=1, exists=False):
    return D.prune(M.graph_of_reads(reads, k, exists), t, exists)[0]


@pytest.mark.parametrize("k", [21, 31, 33])
def test_the_pipeline_input(k):
    """29 unitigs as pruned, 19 after the tip rounds, and one round of popping leaves the genome"""
    genome, reads = D.pipeline_reads(k)
    pruned = _pruned(reads, k)
    assert _summary(pruned)[0] == 29
    tipped = B.clean_tips(pruned)
    assert _summary(tipped) == (19, 259)
    out, s = B.pop(tipped, 1, 2 * k)
    assert s == dict(n_nodes=len(tipped), n_unitigs=19, n_branches=12, n_bubbles=6, n_popped=6, n_nodes_removed=6 * k, n_counters_cleared=12,
                     reserved=0)
    assert _summary(out) == (1, 1500) and M.unitigs_from_strings(out)[0][0] in (genome, M.revcomp(genome))
    # the survivors keep their order and, the twelve junction counters apart, their rows
    assert list(out) == [v for v in tipped if v in out]
    assert sum(1 for v in out for j in range(9) if out[v][j] != tipped[v][j]) == 12
    # a following pruning clears nothing, and a second round finds nothing
    p2, ps = D.prune(out, 1)
    assert p2 == out and ps["n_set_before"] == ps["n_set_after"]
    again, s2 = B.pop(out, 1, 2 * k)
    assert again == out and (s2["n_unitigs"], s2["n_branches"], s2["n_bubbles"], s2["n_popped"]) == (1, 0, 0, 0)


@pytest.mark.parametrize("k", [21, 65])
def test_substitution_and_deletion_around_the_limit(k):
    nodes = _pruned(B.substitution_reads(k, 1), k)
    out, s = B.pop(nodes, 1, k)
    assert (s["n_unitigs"], s["n_branches"], s["n_bubbles"], s["n_popped"], s["n_nodes_removed"], s["n_counters_cleared"]) == (4, 2, 1, 1, k, 2)
    assert _summary(out)[0] == 1
    out, s = B.pop(nodes, 1, k - 1)
    assert out == nodes and (s["n_bubbles"], s["n_popped"]) == (1, 0)
    # a light deletion branch of k - 1 nodes leaves although its heavier sibling has k > M nodes
    nodes = _pruned(B.deletion_reads(k, 1, 2, 1), k)
    out, s = B.pop(nodes, 1, k - 1)
    assert (s["n_bubbles"], s["n_popped"], s["n_nodes_removed"]) == (1, 1, k - 1) and _summary(out)[0] == 1
    # a heavy one leaves the lighter sibling of k nodes alone with M = k - 1, and pops it with M = k
    nodes = _pruned(B.deletion_reads(k, 1, 1, 2), k)
    out, s = B.pop(nodes, 1, k - 1)
    assert out == nodes and (s["n_bubbles"], s["n_popped"]) == (1, 0)
    out, s = B.pop(nodes, 1, k)
    assert (s["n_popped"], s["n_nodes_removed"]) == (1, k) and _summary(out)[0] == 1


def test_ties():
    k = 21
    for seed in range(6):
        trace = []
        out, s = B.pop(_pruned(B.three_way_reads(k, seed), k), 1, k, trace=trace)
        assert (s["n_branches"], s["n_bubbles"], s["n_popped"], s["n_nodes_removed"]) == (3, 1, 2, 2 * k) and _summary(out)[0] == 1
        assert sorted((x[1][:2], x[3]) for x in trace) == [((1, 1), True), ((2, 2), True), ((3, 3), False)]
        # equal weights: the smaller base at the smaller junction node stays
        trace = []
        out, s = B.pop(_pruned(B.substitution_reads(k, seed, 1, 1), k), 1, k, trace=trace)
        assert (s["n_bubbles"], s["n_popped"]) == (1, 1)
        (kept,), (lost,) = [x for x in trace if not x[3]], [x for x in trace if x[3]]
        assert kept[1][:2] == lost[1][:2] == (1, 1)
        assert kept[0][0][2] == lost[0][0][2] < kept[0][1][2] == lost[0][1][2]   # the same junction nodes, the smaller first
        assert kept[0][0][3] & 4 == lost[0][0][3] & 4 and kept[0][0][3] < lost[0][0][3]


def test_cycles_and_hairpins_are_no_branches():
    k = 21
    rng = np.random.default_rng(3)
    ring = B.rand_seq(rng, 30)
    half = B.rand_seq(rng, k + 4)
    nodes = _pruned([B.rand_seq(rng, k + 2), ring + ring + ring[:k], half + M.revcomp(half), "A" * (k + 3)], k)
    out, s = B.pop(nodes, 1, 64)
    assert out == nodes and (s["n_branches"], s["n_bubbles"], s["n_popped"]) == (0, 0, 0)


def test_random_small_graphs():
    """the key orders every bubble (asserted inside the model), so every bubble keeps exactly one greatest branch; junction nodes
    survive; pruned stays pruned at odd k; a second round on a one-bubble input finds nothing"""
    rng = np.random.default_rng(2025)
    bubbles = popped = 0
    for i in range(360):
        k, t, exists = (3, 5, 7)[i % 3], 1 + (i // 3) % 2, bool((i // 6) % 2)
        m = (1, k - 1, k, 2 * k)[(i // 12) % 4]
        raw = M.graph_of_reads(B.fuzz_reads(rng, k), k, exists)
        pruned, _ = D.prune(raw, t, exists)
        for nodes, is_pruned in ((pruned, True), (raw, False)):
            trace = []
            out, s = B.pop(nodes, t, m, exists, trace)
            bubbles += s["n_bubbles"]
            popped += s["n_popped"]
            assert s["n_nodes"] - s["n_nodes_removed"] == len(out) and s["n_counters_cleared"] == 2 * s["n_popped"] and s["reserved"] == 0
            assert s["n_unitigs"] == len(M.unitigs_from_strings(nodes, t)) and 2 * s["n_bubbles"] <= s["n_branches"]
            families = {}
            for js, key, n, gone in trace:
                assert all(w in out for _, _, w, _ in js), i                      # junction nodes survive
                assert gone == all(v not in out for v, _, _, _ in js) and (not gone or n <= m)
                families.setdefault(frozenset((w, j >> 2) for _, _, w, j in js), []).append((key, gone))
            assert len(families) == s["n_bubbles"]
            for fam in families.values():
                assert len(fam) >= 2 and not max(fam)[1]                          # the greatest stays
            if is_pruned:
                again, ps = D.prune(out, t, exists)
                assert again == out and ps["n_set_before"] == ps["n_set_after"], i
    assert bubbles > 100 and popped > 50   # (the properties cannot pass empty)
    for seed in range(10):
        for k in (21, 33):
            out, s = B.pop(_pruned(B.substitution_reads(k, seed), k), 1, k)
            again, s2 = B.pop(out, 1, k)
            assert (s["n_branches"], s["n_bubbles"], s["n_popped"]) == (2, 1, 1)
            assert again == out and (s2["n_unitigs"], s2["n_branches"], s2["n_bubbles"], s2["n_popped"]) == (1, 0, 0, 0)
