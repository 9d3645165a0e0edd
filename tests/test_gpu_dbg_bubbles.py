"""Popping the bubbles of a de Bruijn node map on the GPU (DeBruijnNodes.pop_bubbles / kmi_dbg_pop_bubbles) against the plain-Python
model (tests/bubbles_model.py). The model's input is never the GPU's map: it is tests/unitig_model.graph_of_reads on the reads, put
through the models of the pruning and of the tip rounds where the GPU map went through them, and the GPU's export is compared with
it before the call. After the call: the same keys in the same order, the rows word for word, all eight stats; n_unitigs also
against kmi_dbg_compact on a twin map."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

from tests import bubbles_model as B
from tests import dbg_clean_model as D
from tests import unitig_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import kmerind_amd as K
    c = K.Context(0)
    yield c
    c.close()


def _build(ctx, reads, k, exists=False, prune=None, tips=False):
    import kmerind_amd as K
    g = K.DeBruijnNodes(ctx, K.make_config(k), exists_only=exists)
    g.build(D.fastq(reads))
    if prune:
        g.prune_edges(prune)
    while tips:   # the tip rounds of the cleaning pipeline
        clipped = g.clip_tips(prune)["n_tips_clipped"]
        g.prune_edges(prune)
        tips = clipped > 0
    return g


def _export(g, k):
    keys, cnt = g.to_vector()
    return keys, cnt, (M.decode_keys(keys, k) if keys.shape[0] else [])   # (every node may have left)


def _check(ctx, reads, k, t=1, m=None, exists=False, prune=True, tips=False, trace=None):
    """builds the map (pruned with t when asked, then through the tip rounds when asked), pops once and compares everything with
    the model -> (g, nodes before, after, stats)"""
    m = 2 * k if m is None else m
    nodes = M.graph_of_reads(reads, k, exists)
    if prune:
        nodes, _ = D.prune(nodes, t, exists)
    if tips:
        nodes = B.clean_tips(nodes, t, exists=exists)
    g = _build(ctx, reads, k, exists, t if prune else None, tips)
    keys0, cnt0, strs0 = _export(g, k)
    assert D.nodes_of(keys0, cnt0, k) == nodes, "the map before the call is not the model's input"
    want, stats = B.pop(nodes, t, m, exists, trace)
    got = g.pop_bubbles(t, m)
    print(k, t, m, exists, got)
    assert got == stats
    keys1, cnt1, strs1 = _export(g, k)
    stay = np.array([s in want for s in strs0], dtype=bool)
    assert keys1.shape == keys0[stay].shape and (keys1 == keys0[stay]).all()       # the same keys in the same order
    assert strs1 == [s for s in strs0 if s in want]
    assert cnt1.tolist() == [want[s] for s in strs1]                               # word for word, counts[8] among them
    twin = _build(ctx, reads, k, exists, t if prune else None, tips)
    assert len(twin.unitigs(t)[2]) == stats["n_unitigs"]
    twin.close()
    return g, nodes, want, stats


# ---- one to four key words
@pytest.mark.parametrize("k", [21, 33])
def test_the_pipeline_input_after_the_tip_rounds(ctx, k):
    genome, reads = D.pipeline_reads(k)
    g, nodes, want, s = _check(ctx, reads, k, tips=True)
    assert s == dict(n_nodes=len(nodes), n_unitigs=19, n_branches=12, n_bubbles=6, n_popped=6, n_nodes_removed=6 * k, n_counters_cleared=12,
                     reserved=0)
    # one unitig is left, the genome; a following pruning clears nothing, a second round finds nothing and leaves the map
    from kmerind_amd.core import split_unitigs
    off, bases, occ, circ = g.unitigs(1)
    (u,) = split_unitigs(off, bases)
    assert u.decode() in (genome, M.revcomp(genome)) and not circ[0]
    before = g.to_vector()
    p = g.prune_edges(1)
    assert p["n_set_before"] == p["n_set_after"]
    again = g.pop_bubbles(1)
    assert again == dict(n_nodes=len(want), n_unitigs=1, n_branches=0, n_bubbles=0, n_popped=0, n_nodes_removed=0, n_counters_cleared=0, reserved=0)
    after = g.to_vector()
    assert (before[0] == after[0]).all() and (before[1] == after[1]).all()
    g.close()


@pytest.mark.parametrize("k", [65, 97])
def test_one_substitution_in_three_and_four_key_words(ctx, k):
    g, nodes, want, s = _check(ctx, B.substitution_reads(k, k), k)
    assert (s["n_unitigs"], s["n_branches"], s["n_bubbles"], s["n_popped"], s["n_nodes_removed"], s["n_counters_cleared"]) == (4, 2, 1, 1, k, 2)
    assert g.n_words == (2 * k + 63) // 64 and len(M.unitigs_from_strings(want)) == 1
    g.close()


# ---- fuzz
def _fuzz_case(rng, k, i):
    """set i of a run: (reads, t, exists, pruned, M)"""
    return B.fuzz_reads(rng, k), 1 + i % 2, bool((i // 2) % 2), (i // 4) % 2 == 0, (1, k - 1, k, 2 * k)[(i // 8) % 4]


def _model_alone(seed, k, n_sets):
    """what the model pops over a run, and the palindromic nodes it meets: the seeds below were picked on the CPU with this"""
    rng = np.random.default_rng(seed)
    popped = bubbles = pal = 0
    for i in range(n_sets):
        reads, t, exists, prune, m = _fuzz_case(rng, k, i)
        nodes = M.graph_of_reads(reads, k, exists)
        if prune:
            nodes, _ = D.prune(nodes, t, exists)
        s = B.pop(nodes, t, m, exists)[1]
        popped, bubbles, pal = popped + s["n_popped"], bubbles + s["n_bubbles"], pal + sum(1 for v in nodes if v == M.revcomp(v))
    return popped, bubbles, pal


@pytest.mark.parametrize("part", range(4))
def test_fuzz_k5(ctx, part):
    """200 random read sets at k = 5 in four parts, both node kinds, t = 1 and 2, pruned and as built, M = 1, k - 1, k, 2 k; the
    pruned ones stay pruned"""
    if part == 0:
        popped, bubbles, _ = _model_alone(5, 5, 200)
        assert popped >= 20 and bubbles >= popped   # (the comparison cannot pass empty)
    rng = np.random.default_rng(5)
    for i in range(200):
        reads, t, exists, prune, m = _fuzz_case(rng, 5, i)
        if i // 50 != part:
            continue
        g, nodes, want, s = _check(ctx, reads, 5, t, m, exists, prune)
        if prune:
            p = g.prune_edges(t)
            assert p["n_set_before"] == p["n_set_after"], i
        g.close()


def test_palindromic_nodes_k4(ctx):
    """k = 4, 80 sets: nodes that are their own reverse complement link to nothing and exempt their neighbours' counters from the
    pruning's rule 3; exact against the model (pruned-stays-pruned is not a property of even k)"""
    popped, _, pal = _model_alone(4, 4, 80)
    assert pal > 0 and popped > 0
    rng = np.random.default_rng(4)
    got = 0
    for i in range(80):
        reads, t, exists, prune, m = _fuzz_case(rng, 4, i)
        g, nodes, want, s = _check(ctx, reads, 4, t, m, exists, prune)
        got += s["n_popped"]
        g.close()
    assert got == popped


# ---- hand-made shapes
def test_substitution_around_the_limit(ctx):
    k = 21
    g, nodes, want, s = _check(ctx, B.substitution_reads(k, 1), k, m=k)   # 2 : 1
    assert (s["n_bubbles"], s["n_popped"], s["n_nodes_removed"]) == (1, 1, k) and len(M.unitigs_from_strings(want)) == 1
    g.close()
    g, nodes, want, s = _check(ctx, B.substitution_reads(k, 1), k, m=k - 1)
    assert want == nodes and (s["n_bubbles"], s["n_popped"], s["n_nodes_removed"]) == (1, 0, 0)
    g.close()


def test_deletion_branches_of_unequal_length(ctx):
    k = 21
    # a light deletion branch of k - 1 nodes is popped with M = k - 1 although its heavier sibling has k > M nodes
    g, nodes, want, s = _check(ctx, B.deletion_reads(k, 1, 2, 1), k, m=k - 1)
    assert (s["n_bubbles"], s["n_popped"], s["n_nodes_removed"]) == (1, 1, k - 1) and len(M.unitigs_from_strings(want)) == 1
    g.close()
    # a heavy one leaves the lighter sibling of k nodes alone with M = k - 1; with M = k the sibling is popped
    g, nodes, want, s = _check(ctx, B.deletion_reads(k, 1, 1, 2), k, m=k - 1)
    assert want == nodes and (s["n_bubbles"], s["n_popped"]) == (1, 0)
    g.close()
    g, nodes, want, s = _check(ctx, B.deletion_reads(k, 1, 1, 2), k, m=k)
    assert (s["n_bubbles"], s["n_popped"], s["n_nodes_removed"]) == (1, 1, k) and len(M.unitigs_from_strings(want)) == 1
    g.close()


def test_ties(ctx):
    k = 21
    for seed in (5, 6):
        trace = []
        g, nodes, want, s = _check(ctx, B.three_way_reads(k, seed), k, m=k, trace=trace)   # 3 : 2 : 1
        assert (s["n_branches"], s["n_bubbles"], s["n_popped"], s["n_nodes_removed"]) == (3, 1, 2, 2 * k)
        assert sorted((x[1][:2], x[3]) for x in trace) == [((1, 1), True), ((2, 2), True), ((3, 3), False)]
        g.close()
        trace = []
        g, nodes, want, s = _check(ctx, B.substitution_reads(k, seed, 1, 1), k, m=k, trace=trace)   # 1 : 1
        (kept,), (lost,) = [x for x in trace if not x[3]], [x for x in trace if x[3]]
        assert kept[1][:2] == lost[1][:2] == (1, 1) and s["n_popped"] == 1
        # the same two junction nodes, the smaller first; there the smaller base stays
        assert kept[0][0][2] == lost[0][0][2] < kept[0][1][2] == lost[0][1][2] and kept[0][0][3] < lost[0][0][3]
        assert kept[0][0][0] in want and lost[0][0][0] not in want
        g.close()


def test_orientations(ctx):
    """the same bubble read from either strand, over seeds until the popped branch has had its junction end at the smaller and at
    the greater junction node on an out end and on an in end of their stored k-mers"""
    seen = set()
    for seed in range(8):
        for rc in (False, True):
            reads = B.substitution_reads(21, seed)
            if rc:
                reads = [M.revcomp(r) for r in reads]
            trace = []
            g, nodes, want, s = _check(ctx, reads, 21, trace=trace)
            (lost,) = [x for x in trace if x[3]]
            assert s["n_popped"] == 1 and lost[2] == 21
            seen.update((i, lost[0][i][3] >> 2) for i in range(2))
            g.close()
        if len(seen) == 4:
            break
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_edge_exists_map(ctx):
    """every key ties on value: the base at the smaller junction node decides every bubble"""
    genome, reads = D.pipeline_reads(21)
    trace = []
    g, nodes, want, s = _check(ctx, reads, 21, exists=True, tips=True, trace=trace)
    assert (s["n_bubbles"], s["n_popped"]) == (6, 6) and all(x[1][:2] == (1, 1) for x in trace)
    g.close()


def test_cycles_and_hairpins_are_no_branches(ctx):
    k = 21
    rng = np.random.default_rng(3)
    ring = B.rand_seq(rng, 30)
    half = B.rand_seq(rng, k + 4)
    reads = [B.rand_seq(rng, k + 2), ring + ring + ring[:k], half + M.revcomp(half), "A" * (k + 3)]
    g, nodes, want, s = _check(ctx, reads, k, m=64)
    assert want == nodes and (s["n_branches"], s["n_bubbles"], s["n_popped"], s["n_nodes_removed"]) == (0, 0, 0, 0)
    g.close()


def test_nothing_leaves(ctx):
    import kmerind_amd as K
    g = K.DeBruijnNodes(ctx, K.make_config(21))
    assert g.pop_bubbles() == dict.fromkeys(B.STATS, 0) and g.local_size() == 0
    g.close()
    g, nodes, want, s = _check(ctx, ["ACGGTCAGGTTCAAGGCTTAGGCATCAGGA"], 21)   # one path of ten nodes
    assert want == nodes and (s["n_nodes_removed"], s["n_unitigs"], s["n_branches"]) == (0, 1, 0)
    g.close()


# ---- refusals, and the compaction's result
def _unitigs_readable(g):
    from kmerind_amd import _lib as L
    return L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0)


def test_refusals_leave_the_map_and_the_unitigs(ctx):
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    k = 21
    reads = B.substitution_reads(k, 2)
    st = L.DbgPopStats()
    g = _build(ctx, reads, k, prune=1)
    before = g.to_vector()
    g.unitigs()
    for t, m, flags in ((0, 42, 0), (1, 0, 0), (1, 42, 1), (1, 42, 0x80000000)):
        st.n_nodes = 7
        assert L.lib.kmi_dbg_pop_bubbles(g.h, t, m, flags, C.byref(st)) == L.ERR_INVALID, (t, m, flags)
        assert [getattr(st, f) for f in B.STATS] == [0] * 8
        after = g.to_vector()
        assert (before[0] == after[0]).all() and (before[1] == after[1]).all() and _unitigs_readable(g) == L.OK
    # a call that succeeds drops the unitigs until the next compaction, whether it pops (first) or not (second); stats may be NULL
    assert L.lib.kmi_dbg_pop_bubbles(g.h, 1, 42, 0, None) == L.OK and g.local_size() == before[0].shape[0] - k
    assert _unitigs_readable(g) == L.ERR_INVALID
    g.unitigs()
    assert _unitigs_readable(g) == L.OK and g.pop_bubbles()["n_popped"] == 0 and _unitigs_readable(g) == L.ERR_INVALID
    g.unitigs()
    assert _unitigs_readable(g) == L.OK
    g.close()
    g5 = K.DeBruijnNodes(ctx, K.make_config(k, "DNA5"))
    g5.build(D.fastq(reads))
    before = g5.to_vector()
    assert L.lib.kmi_dbg_pop_bubbles(g5.h, 1, 42, 0, C.byref(st)) == L.ERR_INVALID
    after = g5.to_vector()
    assert (before[0] == after[0]).all() and (before[1] == after[1]).all()
    g5.close()


class _Comm:
    def __init__(self, h):
        self.h = h


def test_one_rank_communicator_build_is_a_whole_map(monkeypatch):
    """a build over a one-rank communicator under KMI_FORCE_DIST=1 goes through the code of several ranks but leaves the whole map
    with the one rank: the call takes it, and gives the model's result"""
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    reads = B.substitution_reads(21, 3)
    nodes, _ = D.prune(M.graph_of_reads(reads, 21), 1)
    want, stats = B.pop(nodes, 1, 42)
    monkeypatch.setenv("KMI_FORCE_DIST", "1")
    ctx = K.Context(0, rank=0, nranks=1)
    h = C.c_void_p()
    ctx.check(L.lib.kmi_comm_create(ctx.h, None, C.byref(h)))
    g = None
    try:
        g = K.DeBruijnNodes(ctx, K.make_config(21))
        g.build_dist(D.fastq(reads), _Comm(h))
        g.prune_edges(1, comm=_Comm(h))
        assert g.pop_bubbles() == stats and stats["n_popped"] == 1
        assert D.nodes_of(*g.to_vector(), 21) == want
    finally:
        if g is not None:
            g.close()
        L.lib.kmi_comm_destroy(h)
        ctx.close()


def _share_worker(rank, world, port, data, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        try:
            g = K.DeBruijnNodes(ctx, K.make_config(21))
            g.build_dist(data if rank == 0 else b"", comm)
            before = g.to_vector()
            g.unitigs(comm=comm)
            st = L.DbgPopStats()
            status = L.lib.kmi_dbg_pop_bubbles(g.h, 1, 42, 0, C.byref(st))
            after = g.to_vector()
            ret[rank] = dict(status=status, stats=[getattr(st, f) for f in B.STATS], nodes=int(before[0].shape[0]),
                             same=bool((before[0] == after[0]).all() and (before[1] == after[1]).all()),
                             unitigs=L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0))
            g.close()
        finally:
            comm.close()
            ctx.close()
    finally:
        dist.destroy_process_group()


def test_a_rank_s_share_is_refused():
    """two processes share the GPU over a gloo group: each holds its share of the build, and the one-rank call refuses it"""
    import torch.multiprocessing as mp
    from kmerind_amd import _lib as L
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ret = mp.Manager().dict()
    reads = B.substitution_reads(21, 2)
    mp.spawn(_share_worker, args=(2, port, D.fastq(reads), ret), nprocs=2, join=True)
    assert sum(ret[r]["nodes"] for r in range(2)) == len(M.graph_of_reads(reads, 21))
    for r in range(2):
        assert ret[r]["status"] == L.ERR_INVALID and ret[r]["stats"] == [0] * 8 and ret[r]["same"] and ret[r]["unitigs"] == L.OK, ret[r]
