"""Clipping the tips of a de Bruijn node map on the GPU (DeBruijnNodes.clip_tips / kmi_dbg_clip_tips) against the plain-Python
model (tests/tips_model.py). The model's input is never the GPU's map: it is tests/unitig_model.graph_of_reads on the reads, put
through the model of the pruning where the GPU map is pruned, and the GPU's export is compared with it before the call. After the
call: the same keys in the same order, the rows word for word, all eight stats; n_unitigs also against kmi_dbg_compact on a twin
map."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

from tests import dbg_clean_model as D
from tests import tips_model as T
from tests import unitig_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import kmerind_amd as K
    c = K.Context(0)
    yield c
    c.close()


def _build(ctx, reads, k, exists=False, prune=None):
    import kmerind_amd as K
    g = K.DeBruijnNodes(ctx, K.make_config(k), exists_only=exists)
    g.build(D.fastq(reads))
    if prune:
        g.prune_edges(prune)
    return g


def _export(g, k):
    keys, cnt = g.to_vector()
    return keys, cnt, (M.decode_keys(keys, k) if keys.shape[0] else [])   # (every node may have left)


def _check(ctx, reads, k, t=1, m=None, islands=False, exists=False, prune=True, trace=None):
    """builds the map (pruned with t when asked), clips once and compares everything with the model -> (g, nodes before, after, stats)"""
    m = 2 * k if m is None else m
    nodes = M.graph_of_reads(reads, k, exists)
    if prune:
        nodes, _ = D.prune(nodes, t, exists)
    g = _build(ctx, reads, k, exists, t if prune else None)
    keys0, cnt0, strs0 = _export(g, k)
    assert D.nodes_of(keys0, cnt0, k) == nodes, "the map before the call is not the model's input"
    want, stats = T.clip(nodes, t, m, T.CLIP_ISLANDS if islands else 0, exists, trace)
    got = g.clip_tips(t, m, islands)
    print(k, t, m, islands, exists, got)
    assert got == stats
    keys1, cnt1, strs1 = _export(g, k)
    stay = np.array([s in want for s in strs0], dtype=bool)
    assert keys1.shape == keys0[stay].shape and (keys1 == keys0[stay]).all()       # the same keys in the same order
    assert strs1 == [s for s in strs0 if s in want]
    assert cnt1.tolist() == [want[s] for s in strs1]                               # word for word, counts[8] among them
    twin = _build(ctx, reads, k, exists, t if prune else None)
    assert len(twin.unitigs(t)[2]) == stats["n_unitigs"]
    twin.close()
    return g, nodes, want, stats


# ---- one to four key words
@pytest.mark.parametrize("k,cand,removed", [(21, 5, 30), (33, 5, 30)])
def test_the_pipeline_input(ctx, k, cand, removed):
    genome, reads = D.pipeline_reads(k)
    g, nodes, want, s = _check(ctx, reads, k)
    assert (s["n_candidates"], s["n_tips_clipped"], s["n_nodes_removed"], s["n_counters_cleared"]) == (cand, cand, removed, cand)
    # the unitigs afterwards are the model's; a second round clips nothing and leaves the map; it is still pruned
    from kmerind_amd.core import split_unitigs
    off, bases, occ, circ = g.unitigs(1)
    assert sorted((x.decode(), int(o), bool(c)) for x, o, c in zip(split_unitigs(off, bases), occ, circ)) == M.unitigs_from_strings(want)
    assert len(occ) < s["n_unitigs"]
    before = g.to_vector()
    again = g.clip_tips(1)
    assert (again["n_candidates"], again["n_tips_clipped"], again["n_nodes_removed"], again["n_nodes"]) == (0, 0, 0, len(want))
    p = g.prune_edges(1)
    assert p["n_set_before"] == p["n_set_after"]
    after = g.to_vector()
    assert (before[0] == after[0]).all() and (before[1] == after[1]).all()
    g.close()


@pytest.mark.parametrize("k", [65, 97])
def test_one_junction_with_one_tip(ctx, k):
    g, nodes, want, s = _check(ctx, T.tip_reads(k, k, 6), k)
    # (the genome's own stretch behind the junction is short enough to be a candidate too; it is the heavier branch and stays)
    assert (s["n_unitigs"], s["n_candidates"], s["n_tips_clipped"], s["n_nodes_removed"], s["n_counters_cleared"]) == (3, 2, 1, 6, 1)
    assert g.n_words == (2 * k + 63) // 64 and len(M.unitigs_from_strings(want)) == 1
    g.close()


# ---- fuzz
def _random_reads(rng, k):
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
    return reads


def test_fuzz_k5(ctx):
    """100 random read sets at k = 5, both node kinds, t = 1 and 2, pruned and as built; the pruned ones stay pruned"""
    rng = np.random.default_rng(5)
    clipped = islands = 0
    for i in range(100):
        reads = _random_reads(rng, 5)
        t, exists, prune = 1 + i % 2, bool((i // 2) % 2), (i // 4) % 2 == 0
        g, nodes, want, s = _check(ctx, reads, 5, t, (1, 2, 5, 10)[(i // 8) % 4], i % 3 == 0, exists, prune)
        clipped += s["n_tips_clipped"]
        islands += s["n_islands_removed"]
        if prune:
            p = g.prune_edges(t)
            assert p["n_set_before"] == p["n_set_after"], i
        g.close()
    assert clipped > 20 and islands > 0   # (the comparison cannot pass empty)


def test_palindromic_nodes_k4(ctx):
    """k = 4: nodes that are their own reverse complement link to nothing and exempt their neighbours' counters from the pruning's
    rule 3; exact against the model (pruned-stays-pruned is not a property of even k)"""
    rng = np.random.default_rng(4)
    pal = clipped = 0
    for i in range(40):
        reads = _random_reads(rng, 4) + ["ACGTT", "GAATTCA"][:i % 3]
        g, nodes, want, s = _check(ctx, reads, 4, 1 + i % 2, (1, 3, 8)[i % 3], i % 4 == 0, False, i % 2 == 0)
        pal += sum(1 for v in nodes if v == M.revcomp(v))
        clipped += s["n_tips_clipped"]
        g.close()
    assert pal > 0 and clipped > 0


# ---- hand-made shapes
def test_tip_length_around_the_limit(ctx):
    for n, gone in ((1, True), (4, True), (5, False)):
        g, nodes, want, s = _check(ctx, T.tip_reads(21, 1, n), 21, m=4)
        assert (s["n_candidates"], s["n_tips_clipped"], s["n_nodes_removed"]) == ((1, 1, n) if gone else (0, 0, 0))
        g.close()


def test_orientations(ctx):
    """the same tip read from either strand, over seeds that put the tip's attached end and the junction end on an out end and on
    an in end of their stored k-mers"""
    seen = set()
    for seed in range(6):
        for rc in (False, True):
            reads = T.tip_reads(21, seed, 3)
            if rc:
                reads = [M.revcomp(r) for r in reads]
            trace = []
            g, nodes, want, s = _check(ctx, reads, 21, trace=trace)
            (tip,) = [x for x in trace if x[5]]   # (the genome's own stretch behind the junction is a candidate too, and stays)
            assert s["n_tips_clipped"] == 1 and tip[4] == 3
            seen.add(("tip", tip[1] >> 2))
            seen.add(("junction", tip[3] >> 2))
            g.close()
    assert seen == {("tip", 0), ("tip", 1), ("junction", 0), ("junction", 1)}


@pytest.mark.parametrize("branches,clipped", [([(0, 12, 3), (1, 3, 2), (2, 2, 1)], [2, 3]),   # unequal tips beside a continuation
                                               ([(0, 12, 1), (1, 3, 1), (2, 2, 1)], [2, 3]),   # all equal: the continuation stays
                                               ([(0, 12, 1), (1, 3, 2)], []),                  # a tip heavier than the continuation
                                               ([(1, 3, 2), (2, 2, 1)], [2]),                  # two tips alone: the heavier stays
                                               ([(2, 3, 1), (1, 2, 1)], None)])                # ... of equal weight: the smaller base
def test_competing_tips(ctx, branches, clipped):
    for seed in (5, 6):
        trace = []
        g, nodes, want, s = _check(ctx, T.junction_reads(21, seed, branches), 21, m=6, trace=trace)
        assert s["n_candidates"] == len(branches) - (branches[0][1] > 6)
        if clipped is None:
            (kept,), (lost,) = [x for x in trace if not x[5]], [x for x in trace if x[5]]
            assert kept[2] == lost[2] and kept[3] < lost[3] and s["n_tips_clipped"] == 1
        else:
            assert sorted(x[4] for x in trace if x[5]) == clipped
        junction = trace[0][2]
        assert junction in want and sum(1 for c in want[junction][:8] if c) >= 2   # the junction keeps a branch and its trunk
        g.close()


def test_islands_cycles_and_hairpins(ctx):
    k = 21
    rng = np.random.default_rng(3)
    ring = T.rand_seq(rng, 30)
    half = T.rand_seq(rng, k + 4)
    reads = [T.rand_seq(rng, k + 2), ring + ring + ring[:k], half + M.revcomp(half), "A" * (k + 3)]
    g, nodes, want, s = _check(ctx, reads, k, m=64)
    assert want == nodes and (s["n_candidates"], s["n_islands"], s["n_islands_removed"], s["n_nodes_removed"]) == (0, 1, 0, 0)
    assert any(c for _, c in T.components(M.Graph(nodes, 1)))
    g.close()
    g, nodes, want, s = _check(ctx, reads, k, m=64, islands=True)
    assert (s["n_islands"], s["n_islands_removed"], s["n_nodes_removed"]) == (1, 1, 3)
    g.close()


def test_edge_exists_map_and_weak_counters(ctx):
    genome, reads = D.pipeline_reads(21)
    g, nodes, want, s = _check(ctx, reads, 21, exists=True)
    assert s["n_tips_clipped"] > 0
    g.close()
    # t = 2 on the map as built: the substituted reads' counters are 1, so their nodes are islands and short chains under t = 2
    for islands in (False, True):
        g, nodes, want, s = _check(ctx, reads, 21, t=2, prune=False, islands=islands)
        assert any(0 < c < 2 for row in nodes.values() for c in row[:8]) and s["n_islands"] > 0
        g.close()


def test_nothing_leaves(ctx):
    import kmerind_amd as K
    g = K.DeBruijnNodes(ctx, K.make_config(21))
    assert g.clip_tips() == dict.fromkeys(T.STATS, 0) and g.local_size() == 0
    g.close()
    g, nodes, want, s = _check(ctx, ["ACGGTCAGGTTCAAGGCTTAGGCATCAGGA"], 21)   # one path of ten nodes: an island, which stays
    assert want == nodes and (s["n_nodes_removed"], s["n_unitigs"], s["n_islands"]) == (0, 1, 1)
    g.close()


# ---- refusals, and the compaction's result
def _unitigs_readable(g):
    from kmerind_amd import _lib as L
    return L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0)


def test_refusals_leave_the_map_and_the_unitigs(ctx):
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    reads = T.tip_reads(21, 2, 3)
    st = L.DbgClipStats()
    g = _build(ctx, reads, 21, prune=1)
    before = g.to_vector()
    g.unitigs()
    for t, m, flags in ((0, 42, 0), (1, 0, 0), (1, 42, 2), (1, 42, 0x80000001)):
        assert L.lib.kmi_dbg_clip_tips(g.h, t, m, flags, C.byref(st)) == L.ERR_INVALID, (t, m, flags)
        assert [getattr(st, f) for f in T.STATS] == [0] * 8
        after = g.to_vector()
        assert (before[0] == after[0]).all() and (before[1] == after[1]).all() and _unitigs_readable(g) == L.OK
    # a call that succeeds drops the unitigs until the next compaction, whether it clips (first) or not (second); stats may be NULL
    assert L.lib.kmi_dbg_clip_tips(g.h, 1, 42, 0, None) == L.OK and g.local_size() == before[0].shape[0] - 3
    assert _unitigs_readable(g) == L.ERR_INVALID
    g.unitigs()
    assert _unitigs_readable(g) == L.OK and g.clip_tips()["n_tips_clipped"] == 0 and _unitigs_readable(g) == L.ERR_INVALID
    g.unitigs()
    assert _unitigs_readable(g) == L.OK
    g.close()
    g5 = K.DeBruijnNodes(ctx, K.make_config(21, "DNA5"))
    g5.build(D.fastq(reads))
    before = g5.to_vector()
    assert L.lib.kmi_dbg_clip_tips(g5.h, 1, 42, 0, C.byref(st)) == L.ERR_INVALID
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
    reads = T.tip_reads(21, 3, 3)
    nodes, _ = D.prune(M.graph_of_reads(reads, 21), 1)
    want, stats = T.clip(nodes, 1, 42)
    monkeypatch.setenv("KMI_FORCE_DIST", "1")
    ctx = K.Context(0, rank=0, nranks=1)
    h = C.c_void_p()
    ctx.check(L.lib.kmi_comm_create(ctx.h, None, C.byref(h)))
    g = None
    try:
        g = K.DeBruijnNodes(ctx, K.make_config(21))
        g.build_dist(D.fastq(reads), _Comm(h))
        g.prune_edges(1, comm=_Comm(h))
        assert g.clip_tips() == stats and stats["n_tips_clipped"] == 1
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
            st = L.DbgClipStats()
            status = L.lib.kmi_dbg_clip_tips(g.h, 1, 42, 0, C.byref(st))
            after = g.to_vector()
            ret[rank] = dict(status=status, stats=[getattr(st, f) for f in T.STATS], nodes=int(before[0].shape[0]),
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
    mp.spawn(_share_worker, args=(2, port, D.fastq(T.tip_reads(21, 2, 3)), ret), nprocs=2, join=True)
    assert sum(ret[r]["nodes"] for r in range(2)) == len(M.graph_of_reads(T.tip_reads(21, 2, 3), 21))
    for r in range(2):
        assert ret[r]["status"] == L.ERR_INVALID and ret[r]["stats"] == [0] * 8 and ret[r]["same"] and ret[r]["unitigs"] == L.OK, ret[r]
