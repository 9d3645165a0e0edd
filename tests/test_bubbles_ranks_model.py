"""The protocol of kmi_dbg_pop_bubbles_dist_host, restated in plain Python over simulated ranks (tests/bubbles_ranks_model.py),
against the model of the definition (tests/bubbles_model.pop on the whole map): for every placement of the nodes the union
afterwards, and the total stats, are the one-rank result, and the local stats add up to the totals. No GPU, no library."""
import zlib

import numpy as np
import pytest

from tests import bubbles_model as B
from tests import bubbles_ranks_model as R
from tests import dbg_clean_model as D
from tests import unitig_model as M
from tests.test_gpu_dbg_bubbles import _fuzz_case

WORLDS = (1, 2, 3, 7)


def _placements(nodes, p):
    """a seeded hash, every node on its own rank modulo p, all nodes on one rank"""
    order = {v: i for i, v in enumerate(sorted(nodes))}
    return [lambda v: zlib.crc32(v.encode() + b"/17") % p, lambda v: order[v] % p, lambda v: p - 1]


def _check(nodes, t, m, exists=False):
    want, stats = B.pop(nodes, t, m, exists)
    staged = R.stages(nodes, t, exists)
    for p in WORLDS:
        for owner in _placements(nodes, p):
            got, total, local, exchanges = R.pop(nodes, t, m, p, owner, exists, staged)
            assert got == want, (p, stats, total)
            assert total == stats, (p, stats, total)
            assert len(local) == p and all(sum(x[f] for x in local) == total[f] for f in B.STATS)
            held = [sum(1 for v in nodes if owner(v) == r) for r in range(p)]
            assert [x["n_nodes"] for x in local] == held and exchanges == 9
    return want, stats


def _graph(reads, k, t=1, exists=False, prune=True, tips=False):
    nodes = M.graph_of_reads(reads, k, exists)
    if prune:
        nodes, _ = D.prune(nodes, t, exists)
    return B.clean_tips(nodes, t, exists=exists) if tips else nodes


@pytest.mark.parametrize("seed,k,n_sets", [(5, 5, 200), (4, 4, 80)])
def test_fuzz_streams(seed, k, n_sets):
    """the read sets and the parameter schedule of tests/test_gpu_dbg_bubbles.py: 200 sets at k = 5, and the 80 at k = 4, which have
    nodes that are their own reverse complement"""
    rng = np.random.default_rng(seed)
    popped = bubbles = pal = 0
    for i in range(n_sets):
        reads, t, exists, prune, m = _fuzz_case(rng, k, i)
        nodes = _graph(reads, k, t, exists, prune)
        want, s = _check(nodes, t, m, exists)
        popped, bubbles, pal = popped + s["n_popped"], bubbles + s["n_bubbles"], pal + sum(1 for v in nodes if v == M.revcomp(v))
    assert popped > 0 and bubbles >= popped and (k != 4 or pal > 0)   # (the comparison cannot pass empty)


def test_the_pipeline_input_after_the_tip_rounds():
    k = 21
    genome, reads = D.pipeline_reads(k)
    for exists in (False, True):
        want, s = _check(_graph(reads, k, exists=exists, tips=True), 1, 2 * k, exists)
        assert (s["n_unitigs"], s["n_branches"], s["n_bubbles"], s["n_popped"], s["n_nodes_removed"], s["n_counters_cleared"]) == (19, 12, 6, 6, 6 * k, 12)
        assert len(M.unitigs_from_strings(want)) == 1


def test_limits_unequal_lengths_ties_and_orientations():
    k = 21
    for m, popped in ((k, 1), (k - 1, 0)):
        assert _check(_graph(B.substitution_reads(k, 1), k), 1, m)[1]["n_popped"] == popped
    for (main, variant), m, popped in (((2, 1), k - 1, 1), ((1, 2), k - 1, 0), ((1, 2), k, 1)):
        assert _check(_graph(B.deletion_reads(k, 1, main, variant), k), 1, m)[1]["n_popped"] == popped
    for seed in (5, 6):
        s = _check(_graph(B.three_way_reads(k, seed), k), 1, k)[1]
        assert (s["n_branches"], s["n_bubbles"], s["n_popped"]) == (3, 1, 2)
        assert _check(_graph(B.substitution_reads(k, seed, 1, 1), k), 1, k)[1]["n_popped"] == 1
    for seed in range(4):
        for rc in (False, True):
            reads = B.substitution_reads(k, seed)
            assert _check(_graph([M.revcomp(r) for r in reads] if rc else reads, k), 1, 2 * k)[1]["n_popped"] == 1
    s = _check(_graph(B.substitution_reads(65, 65), 65), 1, 130)[1]
    assert (s["n_unitigs"], s["n_branches"], s["n_bubbles"], s["n_popped"], s["n_nodes_removed"], s["n_counters_cleared"]) == (4, 2, 1, 1, 65, 2)


def test_cycles_hairpins_an_island_a_homopolymer_and_nothing():
    k = 21
    rng = np.random.default_rng(3)
    ring = B.rand_seq(rng, 30)
    half = B.rand_seq(rng, k + 4)
    nodes = _graph([B.rand_seq(rng, k + 2), ring + ring + ring[:k], half + M.revcomp(half), "A" * (k + 3)], k)
    want, s = _check(nodes, 1, 64)
    assert want == nodes and (s["n_branches"], s["n_bubbles"], s["n_popped"]) == (0, 0, 0)
    want, s = _check({}, 1, 42)
    assert want == {} and s == dict.fromkeys(B.STATS, 0)
