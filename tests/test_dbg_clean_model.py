"""The plain-Python model of node-map cleaning (tests/dbg_clean_model.py) on cases small enough to check on paper, and on the
pipeline construction the GPU tests assert against it. No GPU, no library."""
import pytest

from tests import dbg_clean_model as D
from tests import unitig_model as M

A, C, G, T = 0, 1, 2, 3


def _node(out=(), inn=(), occ=1):
    c = [0] * 9
    for b, v in out:
        c[b] = v
    for b, v in inn:
        c[4 + b] = v
    c[8] = occ
    return c


def _cleared(before, after):
    return sorted((v, j) for v in before for j in range(8) if before[v][j] and not after[v][j])


def test_a_two_node_path_is_kept_whole():
    # AACG -> ACGG: AACG (canonical) has out G; ACGG (canonical: rc = CCGT) has in A
    nodes = {"AACG": _node(out=[(G, 1)]), "ACGG": _node(inn=[(A, 1)])}
    assert all(M.canonical(v) == v for v in nodes)
    out, s = D.prune(nodes, 1)
    assert out == nodes
    assert s == dict(n_nodes=2, n_set_before=2, n_weak=0, n_absent=0, n_unreciprocated=0, n_set_after=2, n_isolated=0, n_requests=0)


def test_a_counter_to_a_kmer_that_is_no_node_is_absent():
    nodes = {"AACG": _node(out=[(G, 1), (T, 1)]), "ACGG": _node(inn=[(A, 1)])}   # AACG -> ACGT is no node
    out, s = D.prune(nodes, 1)
    assert _cleared(nodes, out) == [("AACG", T)]
    assert (s["n_absent"], s["n_unreciprocated"], s["n_weak"], s["n_set_after"], s["n_isolated"]) == (1, 0, 0, 2, 0)


def test_a_one_sided_counter_is_unreciprocated():
    nodes = {"AACG": _node(out=[(G, 1)]), "ACGG": _node()}   # ACGG is a node but has no in A
    out, s = D.prune(nodes, 1)
    assert _cleared(nodes, out) == [("AACG", G)]
    assert (s["n_absent"], s["n_unreciprocated"], s["n_set_after"], s["n_isolated"]) == (0, 1, 0, 2)
    # the neighbour stored reverse-complemented: AAGT -> AGTT = rc(AACT); the reciprocal is (AACT, out, comp(A) = T)
    nodes = {"AAGT": _node(out=[(T, 1)]), "AACT": _node(out=[(T, 1)])}
    assert D.neighbour("AAGT", T) == ("AACT", T, False)
    assert D.prune(nodes, 1)[0] == nodes
    nodes["AACT"] = _node(out=[(G, 1)])   # AACT -> ACTG = rc(CAGT) is no node
    out, s = D.prune(nodes, 1)
    assert _cleared(nodes, out) == [("AACT", G), ("AAGT", T)] and (s["n_absent"], s["n_unreciprocated"]) == (1, 1)


def test_threshold_two_against_counters_one_and_two():
    nodes = {"AACG": _node(out=[(G, 2)]), "ACGG": _node(inn=[(A, 1)])}
    out, s = D.prune(nodes, 2)
    # ACGG's in A = 1 is weak; AACG's out G = 2 passes rule 1 and 2 and fails rule 3 against the map as it was
    assert _cleared(nodes, out) == [("AACG", G), ("ACGG", 4 + A)]
    assert (s["n_weak"], s["n_absent"], s["n_unreciprocated"], s["n_set_after"], s["n_isolated"]) == (1, 0, 1, 0, 2)
    nodes["ACGG"] = _node(inn=[(A, 2)])
    assert D.prune(nodes, 2)[0] == nodes


def test_the_palindrome_exemption_at_k_4():
    # v = ACGT is its own reverse complement. Read forward, CACGT puts the adjacency into ACGT's in C; read on the other strand
    # (ACGTG) the same adjacency lands in out G. CACG is canonical (rc = CGTG) and holds out T either way.
    assert M.revcomp("ACGT") == "ACGT"
    nodes = {"ACGT": _node(out=[(G, 1)]), "CACG": _node(out=[(T, 1)])}
    # palindromic v: (ACGT, out, G) -> x = CGTG, w = CACG stored as rc(x): the formula's reciprocal would be (CACG, out, comp(A) = T)
    assert D.neighbour("ACGT", G) == ("CACG", T, True)
    # palindromic w: (CACG, out, T) -> x = ACGT = w: the formula's reciprocal is (ACGT, in, C), which is 0 here
    assert D.neighbour("CACG", T) == ("ACGT", 4 + C, True)
    out, s = D.prune(nodes, 1)
    assert out == nodes and s["n_unreciprocated"] == 0 and s["n_set_after"] == 2
    # rules 1 and 2 still apply to a palindrome's counters
    nodes["ACGT"][T] = 1   # ACGT -> CGTT = rc(AACG): no node
    out, s = D.prune(nodes, 1)
    assert _cleared(nodes, out) == [("ACGT", T)] and s["n_absent"] == 1
    out, s = D.prune(nodes, 2)
    assert s["n_weak"] == 3 and s["n_set_after"] == 0


def test_a_hairpin_and_a_self_loop_are_kept():
    k = 5
    # poly-A: AAAAA -> AAAAA, out A and in A are each other's reciprocal
    nodes = M.graph_of_reads(["A" * (2 * k)], k)
    assert list(nodes) == ["AAAAA"] and nodes["AAAAA"][A] == k and nodes["AAAAA"][4 + A] == k
    out, s = D.prune(nodes, 1)
    assert out == nodes and s["n_set_after"] == 2
    # ACAC...: ACACA <-> CACAC = rc(GTGTG); every counter has its reciprocal
    nodes = M.graph_of_reads(["AC" * k], k)
    assert sorted(nodes) == ["ACACA", "CACAC"]
    out, s = D.prune(nodes, 1)
    assert out == nodes and s["n_set_after"] == s["n_set_before"] == 4
    # a hairpin: AAATT -> AATTT = rc(AAATT); the counter (AAATT, out, T) is its own reciprocal
    nodes = M.graph_of_reads(["AAATTT"], k)
    assert list(nodes) == ["AAATT"] and nodes["AAATT"][:8] == [0, 0, 0, 2, 0, 0, 0, 0]   # (both windows land in out T)
    assert D.neighbour("AAATT", T) == ("AAATT", T, False)
    out, s = D.prune(nodes, 1)
    assert out == nodes and s["n_set_before"] == 1 and s["n_set_after"] == 1


@pytest.mark.parametrize("k,built,retained,absent", [(15, 29, 18, 17), (21, 29, 18, 17), (22, 29, 18, 17), (31, 29, 18, 17), (32, 29, 18, 17),
                                                     (33, 29, 18, 17), (63, 17, 6, 5)])
def test_the_pipeline_construction_ends_as_one_unitig(k, built, retained, absent):
    genome, reads = D.pipeline_reads(k)
    nodes = M.graph_of_reads(reads, k)
    assert len(M.unitigs_from_strings(nodes)) == built
    kept = D.retain(nodes, 2, 2**32 - 1)
    assert len(kept) == len(genome) - k + 1
    assert len(M.unitigs_from_strings(kept)) == retained
    pruned, s = D.prune(kept, 1)
    assert (s["n_weak"], s["n_absent"], s["n_unreciprocated"]) == (0, absent, 0)
    assert M.unitigs_from_strings(pruned) == [(min(genome, M.revcomp(genome)), sum(c[8] for c in kept.values()), False)]


@pytest.mark.parametrize("t", [1, 2, 3])
def test_idempotence_and_the_stats_identity(t):
    k = 11
    _, reads = D.pipeline_reads(k)
    reads = reads[:60] + [r[:40] + "N" + r[41:] for r in reads[60:70]] + reads[-11:]
    nodes = M.graph_of_reads(reads, k)
    once, s = D.prune(nodes, t)
    assert s["n_set_after"] == s["n_set_before"] - s["n_weak"] - s["n_absent"] - s["n_unreciprocated"]
    assert s["n_set_after"] == sum(1 for c in once.values() for j in range(8) if c[j])
    assert s["n_isolated"] == sum(1 for c in once.values() if not any(c[:8]))
    assert (s["n_absent"] if t == 1 else s["n_weak"]) > 0 and s["n_nodes"] == len(nodes) == len(once)
    assert [c[8] for c in once.values()] == [c[8] for c in nodes.values()] and list(once) == list(nodes)
    twice, s2 = D.prune(once, t)
    assert twice == once
    assert (s2["n_weak"], s2["n_absent"], s2["n_unreciprocated"]) == (0, 0, 0) and s2["n_set_before"] == s["n_set_after"]
    # after prune(t) the compaction does not depend on the threshold 1..t
    for u in range(1, t + 1):
        assert M.unitigs_from_strings(once, u) == M.unitigs_from_strings(once, t)


def test_spectrum_and_retain():
    nodes = {"AACG": _node(occ=1), "ACGG": _node(occ=3), "AAGT": _node(occ=3), "AACT": _node(occ=9)}
    hist, tot = D.spectrum(nodes, 4)
    assert hist == [0, 1, 0, 3] and tot == dict(n_entries=4, sum_counts=16, min_count=1, max_count=9)
    assert D.spectrum({}, 2) == ([0, 0], dict(n_entries=0, sum_counts=0, min_count=0, max_count=0))
    assert list(D.retain(nodes, 2, 5)) == ["ACGG", "AAGT"] and D.retain(nodes, 0, 2**32 - 1) == nodes and D.retain(nodes, 10, 10) == {}
