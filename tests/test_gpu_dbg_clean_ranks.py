"""Cleaning a de Bruijn node map held over ranks (kmi_dbg_spectrum_dist_host, kmi_dbg_retain_counts on every rank's share,
kmi_dbg_prune_edges_dist_host). The expected value is always the plain-Python model (tests/dbg_clean_model.py) on the ORACLE's whole
node map: the union of the ranks' maps must be the model's map, the totals the model's stats on every rank. Two and four processes
share the GPU over a gloo group (kmerind_amd/transport.py), started as tests/test_gpu_unitigs_ranks.py starts them; nodes are placed by
KeyToRank of the canonical k-mer, so nearly every counter's neighbour lives on another rank."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

from tests import dbg_clean_model as D
from tests import oracle as orc
from tests import unitig_model as M

pytestmark = pytest.mark.gpu
MAX = 2**32 - 1


def _genome(rng, n):
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, n)])


def _branching_reads(seed, k, n_reads=400):
    """reads of a genome with a repeat of 3k inserted twice, SNP variants, a poly-A stretch of 2k and a few N, both strands"""
    rng = np.random.default_rng(seed)
    g = _genome(rng, 2000)
    rep = g[300:300 + 3 * k]
    g = g[:800] + rep + g[800:1400] + rep + g[1400:] + "A" * (2 * k) + _genome(rng, 200)
    snp = list(g)
    for p in rng.integers(0, len(g), 8):
        snp[p] = "ACGT"[("ACGT".index(snp[p]) + 1) % 4]
    snp = "".join(snp)
    reads = []
    for i in range(n_reads):
        src = snp if i % 5 == 0 else g
        p = int(rng.integers(0, len(src) - 140))
        r = src[p:p + int(rng.integers(max(k + 2, 60), 140))]
        if i % 40 == 7:
            r = r[:30] + "N" + r[31:]
        reads.append(M.revcomp(r) if rng.random() < 0.5 else r)
    # counters that no neighbour reciprocates: u is read once; a second read stops at an N, which sets all four out counters of the
    # k-mer in front of it -- the true base then stands at 2 against its neighbour's 1 (unreciprocated at t = 2); a third read holds
    # the neighbour behind another base x with another k-mer in front of it (unreciprocated at t = 1)
    u = _genome(rng, 200)
    x = "ACGT"[("ACGT".index(u[100]) + 1) % 4]
    z = "ACGT"[("ACGT".index(u[100 - k]) + 1) % 4]
    reads += [u, u[:100] + "N", z + u[101 - k:100] + x + _genome(rng, 30)]
    return D.fastq(reads)


def _record_shares(data, world):
    """contiguous shares of whole four-line records, one per rank"""
    lines = data.rstrip(b"\n").split(b"\n")
    n_rec = len(lines) // 4
    cuts = [n_rec * r // world * 4 for r in range(world + 1)]
    return [b"".join(ln + b"\n" for ln in lines[cuts[r]:cuts[r + 1]]) for r in range(world)]


def _oracle_nodes(data, k):
    s = orc.kspec(k)
    om = orc.DbgMap(s)
    om.insert(*orc.dbg_parse(s, data))
    return D.nodes_of(*om.export(canonical=True), k)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _units(g, comm, t=1):
    from kmerind_amd.core import split_unitigs
    off, bases, occ, circ = g.unitigs(t, comm=comm)
    return [(s.decode(), int(o), bool(c)) for s, o, c in zip(split_unitigs(off, bases), occ, circ)], tuple(g.unitig_totals)


def _job(K, L, ctx, comm, rank, world, job):
    k = job["k"]
    out = {}
    st_l, st_t, n = L.DbgPruneStats(), L.DbgPruneStats(), C.c_uint64()
    # 1. branching reads: spectrum, then prune at every t on a fresh build
    for t in job["ts"]:
        g = K.DeBruijnNodes(ctx, K.make_config(k))
        g.build_dist(job["parts"][rank], comm)
        if t == job["ts"][0]:
            hist, totals = g.spectrum(64, comm=comm)
            out["spectrum"] = (hist.tolist(), totals)
            # the contract: t = 0 is refused on every rank with nothing left waiting; the one-rank form refuses a share
            before = g.to_vector()
            out["t0"] = L.lib.kmi_dbg_prune_edges_dist_host(g.h, comm.h, 0, C.byref(st_l), C.byref(st_t))
            out["plain"] = L.lib.kmi_dbg_prune_edges(g.h, 1, C.byref(st_l))
            after = g.to_vector()
            out["unchanged"] = bool((before[0] == after[0]).all() and (before[1] == after[1]).all())
            g.unitigs(comm=comm)
        local = g.prune_edges(t, comm=comm)
        out[("prune", t)] = dict(local=local, total=dict(g.prune_totals), map=g.to_vector(),
                                 export=L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0), sent=ctx.debug_counter(13))
        again = g.prune_edges(t, comm=comm)
        out[("again", t)] = dict(total=dict(g.prune_totals), same=bool((g.to_vector()[1] == out[("prune", t)]["map"][1]).all()), local=again)
        out[("units", t)] = [_units(g, comm, u) for u in range(1, t + 1)]
        g.close()
    # 2. the pipeline: retain on every rank's share, prune over the ranks, compact over the ranks
    if job.get("pipeline") is not None:
        g = K.DeBruijnNodes(ctx, K.make_config(k))
        g.build_dist(job["pipeline"][rank], comm)
        built = _units(g, comm)[1][0]
        erased = g.retain_counts(2)
        kept = _units(g, comm)[1][0]
        g.prune_edges(1, comm=comm)
        out["pipeline"] = dict(built=built, erased=erased, kept=kept, stats=dict(g.prune_totals), units=_units(g, comm), size=g.local_size())
        g.close()
    return out


def _job_nothing(K, L, ctx, comm, rank, world, job):
    g = K.DeBruijnNodes(ctx, K.make_config(job["k"]))
    g.build_dist(job["parts"][rank], comm)
    local = g.prune_edges(1, comm=comm)
    out = dict(local=local, total=dict(g.prune_totals), map=g.to_vector(), spectrum=g.spectrum(4, comm=comm)[0].tolist())
    g.clear()
    g.prune_edges(1, comm=comm)
    out["empty"] = dict(g.prune_totals)
    g.close()
    return out


_JOBS = {"clean": _job, "nothing": _job_nothing}


def _worker(rank, world, port, job, ret):
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
            ret[rank] = _JOBS[job["kind"]](K, L, ctx, comm, rank, world, job)
        finally:
            comm.close()
            ctx.close()
    finally:
        dist.destroy_process_group()


def _run(world, job):
    import torch.multiprocessing as mp
    assert world in (2, 4)
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), job, ret), nprocs=world, join=True)
    return [ret[r] for r in range(world)]


def _union(res, key, k):
    nodes = {}
    for r in res:
        part = D.nodes_of(*r[key]["map"], k)
        assert not set(part) & set(nodes), "a node on two ranks"
        nodes.update(part)
    return nodes


def _with_requests(stats):
    """the model's stats as the sum over ranks shows them: every counter >= t is one request"""
    return dict(stats, n_requests=stats["n_set_before"] - stats["n_weak"])


@pytest.mark.parametrize("k,world", [(21, 2), (32, 2), (63, 2), (32, 4)])
def test_clean_over_ranks_against_the_model(k, world):
    from kmerind_amd import _lib as L
    data = _branching_reads(k, k)
    nodes = _oracle_nodes(data, k)
    genome, reads = D.pipeline_reads(k)
    pipe = D.fastq(reads)
    ts = [1, 2]
    res = _run(world, dict(kind="clean", k=k, parts=_record_shares(data, world), ts=ts, pipeline=_record_shares(pipe, world)))
    seen = dict.fromkeys(D.STATS, 0)
    for r in res:
        assert r["spectrum"] == D.spectrum(nodes, 64)
        assert r["t0"] == L.ERR_INVALID and r["plain"] == L.ERR_INVALID and r["unchanged"]
    for t in ts:
        want, stats = D.prune(nodes, t)
        key = ("prune", t)
        assert _union(res, key, k) == want, t
        for f in D.STATS:
            seen[f] += stats[f]
            assert sum(r[key]["local"][f] for r in res) == _with_requests(stats)[f], (t, f)
        for r in res:
            assert r[key]["total"] == _with_requests(stats), (t, r[key]["total"])
            assert r[key]["local"]["n_requests"] > 0 and r[key]["local"]["n_nodes"] == r[key]["map"][0].shape[0] > 0
            assert r[key]["export"] == L.ERR_INVALID   # the unitigs of the compaction before it are dropped
            assert r[key]["sent"] >= r[key]["local"]["n_requests"] * (r[key]["map"][0].shape[1] + 1) * 8
            # a second call clears nothing anywhere
            a = r[("again", t)]
            assert a["same"] and (a["total"]["n_weak"], a["total"]["n_absent"], a["total"]["n_unreciprocated"]) == (0, 0, 0)
            assert a["total"]["n_set_before"] == a["total"]["n_set_after"] == stats["n_set_after"]
        exp = M.unitigs_from_strings(want, t)
        for u in range(t):
            assert sorted(x for r in res for x in r[("units", t)][u][0]) == exp, (t, u)
            assert all(r[("units", t)][u][1] == (len(exp), sum(len(s) for s, _, _ in exp)) for r in res)
    assert seen["n_weak"] > 0 and seen["n_absent"] > 0 and seen["n_unreciprocated"] > 0   # (the comparison cannot pass empty)
    # the pipeline
    pn = _oracle_nodes(pipe, k)
    kept = D.retain(pn, 2, MAX)
    pruned, pstats = D.prune(kept, 1)
    assert sum(r["pipeline"]["erased"] for r in res) == len(pn) - len(kept) and sum(r["pipeline"]["size"] for r in res) == len(kept)
    one = [(min(genome, M.revcomp(genome)), sum(c[8] for c in kept.values()), False)]
    assert M.unitigs_from_strings(pruned) == one
    for r in res:
        p = r["pipeline"]
        assert (p["built"], p["kept"]) == (len(M.unitigs_from_strings(pn)), len(M.unitigs_from_strings(kept)))
        assert p["stats"] == _with_requests(pstats) and p["units"][1] == (1, len(genome))
    assert sorted(x for r in res for x in r["pipeline"]["units"][0]) == one


def test_a_world_in_which_ranks_own_no_node():
    read = "ACCGATTGCAGGTTACGGATCA"   # two nodes at k = 21
    nodes = M.graph_of_reads([read], 21)
    want, stats = D.prune(nodes, 1)
    res = _run(4, dict(kind="nothing", k=21, parts=[D.fastq([read]), b"", b"", b""]))
    assert sorted(r["local"]["n_nodes"] for r in res)[:2] == [0, 0] and sum(r["local"]["n_nodes"] for r in res) == 2
    got = {}
    for r in res:
        got.update(D.nodes_of(*r["map"], 21))
        assert r["total"] == dict(stats, n_requests=stats["n_set_before"]) and r["empty"] == dict.fromkeys(D.STATS, 0)
        assert r["spectrum"] == [0, 2, 0, 0]
    assert got == want and stats["n_set_after"] == 2


class _Comm:
    def __init__(self, h):
        self.h = h


def test_one_rank_forced_distributed_gives_the_one_rank_result(monkeypatch):
    """the code of several ranks with the rank as its own peer: the arrays and the stats of kmi_dbg_prune_edges on the same map
    (n_requests apart: the forced form does send its requests, to itself)"""
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    k = 32
    data = _branching_reads(k, k)
    want, stats = D.prune(_oracle_nodes(data, k), 1)
    monkeypatch.setenv("KMI_FORCE_DIST", "1")
    ctx = K.Context(0, rank=0, nranks=1)
    h = C.c_void_p()
    ctx.check(L.lib.kmi_comm_create(ctx.h, None, C.byref(h)))
    g = g1 = None
    try:
        g = K.DeBruijnNodes(ctx, K.make_config(k))
        g.build(data)
        g1 = K.DeBruijnNodes(ctx, K.make_config(k))
        keys0, cnt0 = g.to_vector()
        local = g.prune_edges(1, comm=_Comm(h))
        assert local == g.prune_totals == dict(stats, n_requests=stats["n_set_before"] - stats["n_weak"]) and local["n_requests"] > 0
        assert ctx.debug_counter(13) == local["n_requests"] * (g.n_words + 1 + 1) * 8   # requests out, answers back
        keys1, cnt1 = g.to_vector()
        assert (keys1 == keys0).all() and D.nodes_of(keys1, cnt1, k) == want
        # the one-rank call on a second build of the same input: the same map, the same stats
        g1.build(data)
        assert g1.prune_edges(1) == stats and D.nodes_of(*g1.to_vector(), k) == want
        hist, totals = g.spectrum(16, comm=_Comm(h))
        assert (hist.tolist(), totals) == D.spectrum(want, 16)
    finally:
        for x in (g, g1):
            if x is not None:
                x.close()
        L.lib.kmi_comm_destroy(h)
        ctx.close()
