"""The plain-Python model of tip clipping (tests/tips_model.py; the definition is in include/kmerind_hip.h) on the cleaning
pipeline's input, on hand-made junctions and on random small graphs. No GPU: the GPU tests compare the library with this model."""
import numpy as np
import pytest

from tests import dbg_clean_model as D
from tests import tips_model as T
from tests import unitig_model as M


def _summary(nodes, t=1):
    u = M.unitigs_from_strings(nodes, t)
    return len(u), D.n50([len(s) for s, _, _ in u])


# k, M -> nodes, unitigs (N50) before, candidates, clipped, nodes removed, counters cleared, unitigs (N50) after
@pytest.mark.parametrize("k,m,nodes,before,cand,clipped,removed,cleared,after",
                         [(21, 42, 1636, (29, 105), 5, 5, 30, 5, (19, 259)), (31, 62, 1686, (29, 115), 5, 5, 30, 5, (19, 259))])
def test_the_pipeline_input(k, m, nodes, before, cand, clipped, removed, cleared, after):
    genome, reads = D.pipeline_reads(k)
    pruned, _ = D.prune(M.graph_of_reads(reads, k), 1)
    assert len(pruned) == nodes and _summary(pruned) == before
    out, s = T.clip(pruned, 1, m)
    assert s == dict(n_nodes=nodes, n_unitigs=before[0], n_candidates=cand, n_tips_clipped=clipped, n_islands=0, n_islands_removed=0,
                     n_nodes_removed=removed, n_counters_cleared=cleared)
    assert len(out) == nodes - removed and _summary(out) == after
    # the survivors keep their order and, the five junction counters apart, their rows
    assert list(out) == [v for v in pruned if v in out]
    assert sum(1 for v in out for j in range(9) if out[v][j] != pruned[v][j]) == cleared
    # a second round clips nothing and gives the map back; the result is still pruned (the six mid-read errors stay as bubbles)
    again, s2 = T.clip(out, 1, m)
    assert again == out and (s2["n_candidates"], s2["n_tips_clipped"], s2["n_nodes_removed"]) == (0, 0, 0) and s2["n_unitigs"] == after[0]
    p2, ps = D.prune(out, 1)
    assert p2 == out and ps["n_set_before"] == ps["n_set_after"]


def _pruned(reads, k, t=1):
    return D.prune(M.graph_of_reads(reads, k), t)[0]


@pytest.mark.parametrize("k", [21, 65])
def test_tip_length_around_the_limit(k):
    for n, gone in ((1, True), (4, True), (5, False)):
        nodes = _pruned(T.tip_reads(k, 1, n), k)
        out, s = T.clip(nodes, 1, 4)
        assert (s["n_candidates"], s["n_tips_clipped"], s["n_nodes_removed"], s["n_counters_cleared"]) == ((1, 1, n, 1) if gone else (0, 0, 0, 0))
        assert (out == nodes) == (not gone)
        if gone:   # the genome is one unitig again
            assert _summary(out)[0] == 1


def test_competing_tips():
    k = 21
    # (branches, candidates, clipped lengths): a real continuation of 12 nodes beats tips of every weight up to its own
    for branches, cand, clipped in (([(0, 12, 3), (1, 3, 2), (2, 2, 1)], 2, [2, 3]), ([(0, 12, 1), (1, 3, 1), (2, 2, 1)], 2, [2, 3]),
                                    ([(0, 12, 1), (1, 3, 2)], 1, []),          # a tip heavier than the continuation stays
                                    ([(1, 3, 2), (2, 2, 1)], 2, [2]),          # only tips: the heavier one stays
                                    ([(2, 3, 1), (1, 2, 2)], 2, [3])):
        nodes = _pruned(T.junction_reads(k, 5, branches), k)
        trace = []
        out, s = T.clip(nodes, 1, 6, trace=trace)
        assert s["n_candidates"] == cand and sorted(x[4] for x in trace if x[5]) == clipped, branches
        assert s["n_nodes_removed"] == sum(clipped) and s["n_counters_cleared"] == len(clipped)
    # two tips of equal weight and nothing else: the one whose junction counter has the smaller base stays
    for seed in range(6):
        nodes = _pruned(T.junction_reads(k, seed, [(1, 3, 1), (2, 2, 1)]), k)
        trace = []
        out, s = T.clip(nodes, 1, 6, trace=trace)
        assert s["n_candidates"] == 2 and s["n_tips_clipped"] == 1
        (kept,), (lost,) = [x for x in trace if not x[5]], [x for x in trace if x[5]]
        assert kept[2] == lost[2] and kept[3] & 4 == lost[3] & 4 and kept[3] < lost[3]


def test_islands_cycles_and_hairpins():
    k = 21
    rng = np.random.default_rng(3)
    island = T.rand_seq(rng, k + 2)                 # three nodes, both ends dead
    ring = T.rand_seq(rng, 30)
    cycle = ring + ring + ring[:k]               # 30 nodes in a cycle
    half = T.rand_seq(rng, k + 4)
    hairpin = half + M.revcomp(half)             # the middle node's out counter leads to its own reverse complement
    nodes = _pruned([island, cycle, hairpin, "A" * (k + 3)], k)
    comps = T.components(M.Graph(nodes, 1))
    assert sorted(len(s) for s, c in comps if c) == [30]
    out, s = T.clip(nodes, 1, 64)
    assert out == nodes and (s["n_candidates"], s["n_islands"], s["n_islands_removed"], s["n_nodes_removed"]) == (0, 1, 0, 0)
    out, s = T.clip(nodes, 1, 64, T.CLIP_ISLANDS)
    assert (s["n_islands"], s["n_islands_removed"], s["n_nodes_removed"]) == (1, 1, 3) and set(nodes) - set(out) == set(M.canonical(island[i:i + k]) for i in range(3))
    out, s = T.clip(nodes, 1, 2, T.CLIP_ISLANDS)   # an island longer than the limit stays
    assert out == nodes and s["n_islands"] == 0


def _random_graph(rng, k, exists):
    g = T.rand_seq(rng, int(rng.integers(k + 2, 40)))
    reads = []
    for _ in range(int(rng.integers(2, 12))):
        p = int(rng.integers(0, len(g) - k))
        r = list(g[p:p + int(rng.integers(k + 1, k + 12))])
        if rng.random() < 0.5:
            i = int(rng.integers(0, len(r)))
            r[i] = T.other_base(r[i], int(rng.integers(1, 4)))
        r = "".join(r)
        reads.append(M.revcomp(r) if rng.random() < 0.5 else r)
    return M.graph_of_reads(reads, k, exists)


def test_random_small_graphs():
    """pruned stays pruned (odd k: no node is its own reverse complement); an end with two or more branches never loses them all"""
    rng = np.random.default_rng(2024)
    clipped = islands = 0
    for i in range(360):
        k, t, exists = (3, 5, 7)[i % 3], 1 + (i // 3) % 2, bool((i // 6) % 2)
        m = (1, 2, k, 2 * k)[(i // 12) % 4]
        raw = _random_graph(rng, k, exists)
        pruned, _ = D.prune(raw, t, exists)
        for nodes, is_pruned in ((pruned, True), (raw, False)):
            out, s = T.clip(nodes, t, m, T.CLIP_ISLANDS if i % 5 == 0 else 0, exists)
            clipped += s["n_tips_clipped"]
            islands += s["n_islands_removed"]
            assert s["n_nodes"] - s["n_nodes_removed"] == len(out) and s["n_counters_cleared"] == s["n_tips_clipped"] <= s["n_candidates"]
            assert s["n_unitigs"] == len(M.unitigs_from_strings(nodes, t))
            before, after = M.Graph(nodes, t), M.Graph(out, t)
            for v in nodes:
                for end in ("out", "in"):
                    if before.degree(v, end) >= 2:
                        assert v in out and after.degree(v, end) >= 1, (i, v, end)
            if is_pruned:
                again, ps = D.prune(out, t, exists)
                assert again == out and ps["n_set_before"] == ps["n_set_after"], i
    assert clipped > 100 and islands > 0   # (the properties cannot pass empty)
