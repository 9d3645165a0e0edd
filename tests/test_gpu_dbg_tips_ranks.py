"""Clipping the tips of a de Bruijn node map held over ranks (DeBruijnNodes.clip_tips(comm=...) / kmi_dbg_clip_tips_dist_host).
The expected value is always the plain-Python model (tests/tips_model.clip) on the model's WHOLE map: unitig_model.graph_of_reads
on the reads, put through dbg_clean_model.prune where the map is pruned. Every comparison first asserts that the union of the ranks'
maps before the call is the model's input with no node on two ranks, so a build problem cannot pass for a clipping problem. After
the call: the union is the model's map, each rank's keys are its old keys minus the leavers in order, the totals are the model's
stats on every rank, the ranks' local stats add up to them field by field, and n_unitigs equals kmi_dbg_compact_dist_host's total
on a twin build. Two and four processes share the GPU over a gloo group, started as tests/test_gpu_dbg_clean_ranks.py starts them;
several read sets share one spawn."""
import ctypes as C
import os
import socket
import subprocess
import tempfile

import numpy as np
import pytest

from tests import dbg_clean_model as D
from tests import tips_model as T
from tests import unitig_model as M
from tests.test_gpu_dbg_tips import _random_reads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX_BYTES, EX_SENT = 15, 14   # kmi_ctx_debug_counter: bytes and exchanges of the context's last kmi_dbg_clip_tips_dist_host


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _record_shares(reads, world):
    """contiguous shares of whole reads as FASTQ, one per rank (a rank without reads gets no bytes)"""
    cuts = [len(reads) * r // world for r in range(world + 1)]
    return [D.fastq(reads[cuts[r]:cuts[r + 1]]) if cuts[r + 1] > cuts[r] else b"" for r in range(world)]


def _case(reads, k, world, t=1, m=None, islands=False, exists=False, prune=True, parts=None, **more):
    return dict(reads=reads, k=k, t=t, m=2 * k if m is None else m, islands=islands, exists=exists, prune=prune,
                parts=_record_shares(reads, world) if parts is None else parts, **more)


def _units(K, g, comm, t):
    from kmerind_amd.core import split_unitigs
    off, bases, occ, circ = g.unitigs(t, comm=comm)
    return [(s.decode(), int(o), bool(c)) for s, o, c in zip(split_unitigs(off, bases), occ, circ)]


def _same(a, b):
    return bool(a[0].shape == b[0].shape and (a[0] == b[0]).all() and (a[1] == b[1]).all())


def _one_case(K, L, ctx, comm, rank, c):
    def build():
        g = K.DeBruijnNodes(ctx, K.make_config(c["k"]), exists_only=c["exists"])
        g.build_dist(c["parts"][rank], comm)
        if c["prune"]:
            g.prune_edges(c["t"], comm=comm)
        return g
    g = build()
    out = dict(before=g.to_vector())
    out["local"] = g.clip_tips(c["t"], c["m"], c["islands"], comm=comm)
    out["total"] = dict(g.clip_totals)
    out["after"] = g.to_vector()
    out["export"] = L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0)
    out["sent"] = (ctx.debug_counter(EX_SENT), ctx.debug_counter(EX_BYTES))
    if c.get("rounds"):   # still pruned; a second round clips nothing and leaves the arrays; the unitigs afterwards
        g.prune_edges(c["t"], comm=comm)
        out["pruned_again"] = dict(g.prune_totals)
        out["after_prune"] = _same(out["after"], g.to_vector())
        g.clip_tips(c["t"], c["m"], c["islands"], comm=comm)
        out["second"] = dict(g.clip_totals)
        out["second_same"] = _same(out["after"], g.to_vector())
        out["units"] = _units(K, g, comm, c["t"])
    g.close()
    twin = build()
    twin.unitigs(c["t"], comm=comm)
    out["twin_unitigs"] = twin.unitig_totals[0]
    twin.close()
    return out


def _job_cases(K, L, ctx, comm, rank, world, job):
    return [_one_case(K, L, ctx, comm, rank, c) for c in job["cases"]]


def _job_contract(K, L, ctx, comm, rank, world, job):
    """refusals on every rank, then what a successful call does to the compaction's result, then the one-rank call on a share"""
    g = K.DeBruijnNodes(ctx, K.make_config(job["k"]))
    g.build_dist(job["parts"][rank], comm)
    g.prune_edges(1, comm=comm)
    before = g.to_vector()
    g.unitigs(comm=comm)
    sl, st = L.DbgClipStats(), L.DbgClipStats()
    out = dict(refused=[])
    for t, m, flags in ((0, 42, 0), (1, 0, 0), (1, 42, 2)):
        status = L.lib.kmi_dbg_clip_tips_dist_host(g.h, comm.h, t, m, flags, C.byref(sl), C.byref(st))
        out["refused"].append(dict(status=status, stats=[getattr(x, f) for x in (sl, st) for f in T.STATS], same=_same(before, g.to_vector()),
                                   unitigs=L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0)))
    out["plain"] = L.lib.kmi_dbg_clip_tips(g.h, 1, 42, 0, C.byref(sl))
    out["plain_same"] = _same(before, g.to_vector())
    out["ok"] = L.lib.kmi_dbg_clip_tips_dist_host(g.h, comm.h, 1, 42, 0, None, None)   # (both outputs may be NULL)
    out["removed"] = before[0].shape[0] - g.local_size()
    out["unitigs_after"] = L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0)
    g.close()
    return out


_JOBS = {"cases": _job_cases, "contract": _job_contract}


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


def _model(c, trace=None):
    nodes = M.graph_of_reads(c["reads"], c["k"], c["exists"])
    if c["prune"]:
        nodes, _ = D.prune(nodes, c["t"], c["exists"])
    want, stats = T.clip(nodes, c["t"], c["m"], T.CLIP_ISLANDS if c["islands"] else 0, c["exists"], trace)
    return nodes, want, stats


def _compare(c, per_rank, trace=None):
    """one case against the model -> (nodes before, after, stats, owner: node -> rank before the call)"""
    from kmerind_amd import _lib as L
    k = c["k"]
    nodes, want, stats = _model(c, trace)
    owner, after = {}, {}
    for r, res in enumerate(per_rank):
        part = D.nodes_of(*res["before"], k)
        assert not set(part) & set(owner), "a node on two ranks"
        owner.update(dict.fromkeys(part, r))
        assert all(part[v] == nodes.get(v) for v in part), "the map before the call is not the model's input"
    assert set(owner) == set(nodes), "the union of the maps before the call is not the model's input"
    print(k, c["t"], c["m"], c["islands"], c["exists"], c["prune"], stats, [res["local"] for res in per_rank])
    for r, res in enumerate(per_rank):
        keys0, keys1 = res["before"][0], res["after"][0]
        strs0 = M.decode_keys(keys0, k) if keys0.shape[0] else []
        stay = np.array([s in want for s in strs0], dtype=bool)
        assert keys1.shape == keys0[stay].shape and (keys1 == keys0[stay]).all(), r      # its old keys minus the leavers, in order
        part = D.nodes_of(*res["after"], k)
        assert list(part) == [s for s in strs0 if s in want]
        assert all(part[v] == want[v] for v in part), r                                   # word for word, counts[8] among them
        after.update(part)
        assert res["total"] == stats, (r, res["total"], stats)
        assert res["local"]["n_nodes"] == keys0.shape[0] and res["local"]["n_nodes_removed"] == keys0.shape[0] - keys1.shape[0]
        assert res["export"] == L.ERR_INVALID and res["twin_unitigs"] == stats["n_unitigs"]
    assert after == want
    for f in T.STATS:
        assert sum(res["local"][f] for res in per_rank) == stats[f], f
    return nodes, want, stats, owner


# ---- 1. the pipeline input, one and two key words, two and four ranks
@pytest.mark.parametrize("k,world", [(21, 2), (33, 2), (21, 4)])
def test_the_pipeline_input_over_ranks(k, world):
    genome, reads = D.pipeline_reads(k)
    c = _case(reads, k, world, rounds=True)
    (res,) = zip(*_run(world, dict(kind="cases", cases=[c])))
    nodes, want, s, owner = _compare(c, res)
    assert (s["n_unitigs"], s["n_candidates"], s["n_tips_clipped"], s["n_nodes_removed"], s["n_counters_cleared"]) == (29, 5, 5, 30, 5)
    exp = M.unitigs_from_strings(want)
    for r in res:
        p = r["pruned_again"]
        assert (p["n_weak"], p["n_absent"], p["n_unreciprocated"]) == (0, 0, 0) and r["after_prune"]   # prune_edges(1) clears nothing
        z = r["second"]
        assert (z["n_candidates"], z["n_tips_clipped"], z["n_nodes_removed"], z["n_counters_cleared"], z["n_nodes"]) == (0, 0, 0, 0, len(want))
        assert r["second_same"] and z["n_unitigs"] == len(exp) < s["n_unitigs"]
        assert r["sent"][0] > 0 and r["sent"][1] > 0
    assert sorted(x for r in res for x in r["units"]) == exp


# ---- 2. three key words
def test_three_key_words_over_two_ranks():
    c = _case(T.tip_reads(65, 65, 6), 65, 2)
    (res,) = zip(*_run(2, dict(kind="cases", cases=[c])))
    nodes, want, s, owner = _compare(c, res)
    assert (s["n_unitigs"], s["n_candidates"], s["n_tips_clipped"], s["n_nodes_removed"], s["n_counters_cleared"]) == (3, 2, 1, 6, 1)
    assert res[0]["before"][0].shape[1] == 3 and len(M.unitigs_from_strings(want)) == 1


# ---- 3. competing tips and the length limit, in one spawn
_BRANCHES = [([(0, 12, 3), (1, 3, 2), (2, 2, 1)], [2, 3]),   # unequal tips beside a continuation
             ([(0, 12, 1), (1, 3, 1), (2, 2, 1)], [2, 3]),   # all equal: the continuation stays
             ([(0, 12, 1), (1, 3, 2)], []),                  # a tip heavier than the continuation
             ([(1, 3, 2), (2, 2, 1)], [2]),                  # two tips alone: the heavier stays
             ([(2, 3, 1), (1, 2, 1)], None)]                 # ... of equal weight: the smaller base


def test_competing_tips_and_the_length_limit_over_two_ranks():
    cases, meta = [], []
    for branches, clipped in _BRANCHES:
        for seed in (5, 6):
            cases.append(_case(T.junction_reads(21, seed, branches), 21, 2, m=6))
            meta.append((branches, clipped))
    limit = ((1, True), (4, True), (5, False))
    cases += [_case(T.tip_reads(21, 1, n), 21, 2, m=4) for n, _ in limit]
    res = list(zip(*_run(2, dict(kind="cases", cases=cases))))
    for c, (branches, clipped), per_rank in zip(cases, meta, res):
        trace = []
        nodes, want, s, owner = _compare(c, per_rank, trace)
        assert s["n_candidates"] == len(branches) - (branches[0][1] > 6)
        if clipped is None:
            (kept,), (lost,) = [x for x in trace if not x[5]], [x for x in trace if x[5]]
            assert kept[2] == lost[2] and kept[3] < lost[3] and s["n_tips_clipped"] == 1
        else:
            assert sorted(x[4] for x in trace if x[5]) == clipped
        junction = trace[0][2]
        assert junction in want and sum(1 for x in want[junction][:8] if x) >= 2   # the junction keeps a branch and its trunk
    s0 = _model(cases[0])[2]
    assert (s0["n_candidates"], s0["n_tips_clipped"], s0["n_nodes_removed"]) == (2, 2, 5)
    for c, (n, gone), per_rank in zip(cases[len(meta):], limit, res[len(meta):]):
        nodes, want, s, owner = _compare(c, per_rank)
        assert (s["n_candidates"], s["n_tips_clipped"], s["n_nodes_removed"]) == ((1, 1, n) if gone else (0, 0, 0))


# ---- 4. fuzz
FUZZ_SETS = 48
FUZZ_EMPTY_RANK = 143   # the first set of the same stream that leaves one of two ranks without a node (4 nodes, all on rank 0)


def _fuzz_cases(world, extra=()):
    """sets 0 .. FUZZ_SETS - 1 of the generator's stream, then those named in `extra`"""
    rng = np.random.default_rng(5)
    cases = []
    for i in range(max((FUZZ_SETS - 1,) + tuple(extra)) + 1):
        reads = _random_reads(rng, 5)   # (every set is drawn, kept or not: the stream is test_fuzz_k5's)
        if i >= FUZZ_SETS and i not in extra:
            continue
        t, exists, prune = 1 + i % 2, bool((i // 2) % 2), (i // 4) % 2 == 0
        cases.append(_case(reads, 5, world, t, (1, 2, 5, 10)[(i // 8) % 4], i % 3 == 0, exists, prune))
    return cases


@pytest.mark.parametrize("world", [2, 4])
def test_fuzz_k5_over_ranks(world):
    """the first 48 read sets of test_gpu_dbg_tips.py::test_fuzz_k5 with its parameter schedule: 40 clipped tips out of 53
    candidates, 143 islands removed, 225 nodes removed, 40 counters cleared, over 984 nodes (the model, on the CPU). Over two ranks
    the three situations that one-rank code gets wrong, or never meets, must all have occurred. Two of them do within the 48 sets
    (20 clipped tips with a node on another rank than their junction node; 8 times a rank cleared a counter while none of its nodes
    left). No rank of two is left without a node by any of the 48 -- their smallest maps have 4 nodes -- so the two-rank run goes on to
    set 143 of the same stream, the first that does, checked like the others but kept out of the sums above."""
    cases = _fuzz_cases(world, (FUZZ_EMPTY_RANK,) if world == 2 else ())
    res = list(zip(*_run(world, dict(kind="cases", cases=cases))))
    sums = dict.fromkeys(T.STATS, 0)
    far_junction = cleared_without_leaver = empty_rank = 0
    for i, (c, per_rank) in enumerate(zip(cases, res)):
        trace = []
        nodes, want, s, owner = _compare(c, per_rank, trace)
        for f in T.STATS:
            sums[f] += s[f] if i < FUZZ_SETS else 0
        far_junction += sum(1 for v0, _, w, _, _, clipped in trace if clipped and owner[v0] != owner[w])
        cleared_without_leaver += sum(1 for r in per_rank if r["local"]["n_counters_cleared"] > 0 and r["local"]["n_nodes_removed"] == 0)
        empty_rank += sum(1 for r in per_rank if r["local"]["n_nodes"] == 0 and nodes)
    print(world, sums, far_junction, cleared_without_leaver, empty_rank)
    assert sums["n_tips_clipped"] >= 40 and sums["n_islands_removed"] > 0   # (the comparison cannot pass empty)
    assert (sums["n_nodes"], sums["n_candidates"], sums["n_tips_clipped"], sums["n_islands_removed"], sums["n_nodes_removed"],
            sums["n_counters_cleared"]) == (984, 53, 40, 143, 225, 40)
    if world == 2:
        assert far_junction > 0 and cleared_without_leaver > 0 and empty_rank > 0


# ---- 5. islands, cycles, hairpins; an EDGE_EXISTS map
def test_islands_cycles_hairpins_and_an_edge_exists_map_over_two_ranks():
    k = 21
    rng = np.random.default_rng(3)
    ring = T.rand_seq(rng, 30)
    half = T.rand_seq(rng, k + 4)
    reads = [T.rand_seq(rng, k + 2), ring + ring + ring[:k], half + M.revcomp(half), "A" * (k + 3)]
    genome, pipe = D.pipeline_reads(k)
    cases = [_case(reads, k, 2, m=64), _case(reads, k, 2, m=64, islands=True), _case(pipe, k, 2, exists=True)]
    res = list(zip(*_run(2, dict(kind="cases", cases=cases))))
    nodes, want, s, owner = _compare(cases[0], res[0])
    assert want == nodes and (s["n_candidates"], s["n_islands"], s["n_islands_removed"], s["n_nodes_removed"]) == (0, 1, 0, 0)
    assert any(cyc for _, cyc in T.components(M.Graph(nodes, 1)))
    nodes, want, s, owner = _compare(cases[1], res[1])
    assert (s["n_islands"], s["n_islands_removed"], s["n_nodes_removed"]) == (1, 1, 3)
    nodes, want, s, owner = _compare(cases[2], res[2])
    assert s["n_tips_clipped"] > 0


# ---- 6. ranks that own nothing
def test_empty_shares_and_an_empty_world():
    reads = T.tip_reads(21, 2, 3)
    cases = [_case(reads, 21, 4, parts=[D.fastq(reads), b"", b"", b""]), _case([], 21, 4, parts=[b""] * 4)]
    res = list(zip(*_run(4, dict(kind="cases", cases=cases))))
    nodes, want, s, owner = _compare(cases[0], res[0])
    assert s["n_tips_clipped"] == 1 and s["n_nodes_removed"] == 3
    nodes, want, s, owner = _compare(cases[1], res[1])
    assert not nodes and s == dict.fromkeys(T.STATS, 0)
    assert all(r["local"] == s and r["total"] == s and r["before"][0].shape[0] == 0 for r in res[1])


# ---- 7. the code of several ranks on one rank
class _Comm:
    def __init__(self, h):
        self.h = h


def test_one_rank_forced_distributed_gives_the_one_rank_result(monkeypatch):
    """the rank as its own peer: the arrays and all eight stats of kmi_dbg_clip_tips on a second build of the same input. Two builds
    need not place a bucket's nodes in the same order, so the two maps are compared row for row in key order, and the forced call's
    own order against its own map before the call"""
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    k = 21
    genome, reads = D.pipeline_reads(k)
    nodes, _ = D.prune(M.graph_of_reads(reads, k), 1)
    want, stats = T.clip(nodes, 1, 2 * k)
    monkeypatch.setenv("KMI_FORCE_DIST", "1")
    ctx = K.Context(0, rank=0, nranks=1)
    h = C.c_void_p()
    ctx.check(L.lib.kmi_comm_create(ctx.h, None, C.byref(h)))
    g = g1 = None
    try:
        g = K.DeBruijnNodes(ctx, K.make_config(k))
        g.build(D.fastq(reads))
        g.prune_edges(1)
        keys0, cnt0 = g.to_vector()
        strs0 = M.decode_keys(keys0, k)
        assert D.nodes_of(keys0, cnt0, k) == nodes, "the map before the call is not the model's input"
        local = g.clip_tips(1, comm=_Comm(h))
        assert local == g.clip_totals == stats and stats["n_tips_clipped"] == 5
        assert ctx.debug_counter(EX_BYTES) > 0 and ctx.debug_counter(EX_SENT) > 0
        g1 = K.DeBruijnNodes(ctx, K.make_config(k))
        g1.build(D.fastq(reads))
        g1.prune_edges(1)
        assert g1.clip_tips(1) == stats
        keys1, cnt1 = g.to_vector()
        stay = np.array([x in want for x in strs0], dtype=bool)
        assert keys1.shape == keys0[stay].shape and (keys1 == keys0[stay]).all() and D.nodes_of(keys1, cnt1, k) == want

        def by_key(v):
            order = np.lexsort(v[0].T)
            return v[0][order], v[1][order]
        assert _same(by_key((keys1, cnt1)), by_key(g1.to_vector()))
    finally:
        for x in (g, g1):
            if x is not None:
                x.close()
        L.lib.kmi_comm_destroy(h)
        ctx.close()


# ---- 8. the contract
def test_contract_over_two_ranks():
    from kmerind_amd import _lib as L
    reads = T.tip_reads(21, 2, 3)
    res = _run(2, dict(kind="contract", k=21, parts=_record_shares(reads, 2)))
    for r in res:
        for x in r["refused"]:
            assert x["status"] == L.ERR_INVALID and x["stats"] == [0] * 16 and x["same"] and x["unitigs"] == L.OK, x
        assert r["plain"] == L.ERR_INVALID and r["plain_same"]
        assert r["ok"] == L.OK and r["unitigs_after"] == L.ERR_INVALID   # dropped on every rank, whether it lost a node or not
    assert sum(r["removed"] for r in res) == 3


# ---- 9. the facade's example
def _read_fasta(path):
    out = []
    for rec in open(path).read().split(">")[1:]:
        head, seq = rec.split("\n", 1)
        out.append(seq.replace("\n", ""))
    return out


def test_facade_example_through_the_collective_code():
    """examples/de_bruijn_tips_ranks under KMI_FORCE_DIST=1 leaves the unitigs that examples/de_bruijn_tips leaves on the same file
    (the cleaning pipeline's input with min_count = 1, so that the five end-of-read errors are there to clip): its summary (rounds,
    nodes, unitigs, N50) and, sequence by sequence, the one-rank pipeline of the Python layer and the model's unitigs"""
    import kmerind_amd as K
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "de_bruijn_tips_ranks", "de_bruijn_tips"], stdout=subprocess.DEVNULL)
    genome, reads = D.pipeline_reads(31)
    data = D.fastq(reads)
    with tempfile.TemporaryDirectory() as d:
        path, out = os.path.join(d, "reads.fastq"), os.path.join(d, "ranks.fasta")
        with open(path, "wb") as f:
            f.write(data)
        p = subprocess.run([os.path.join(ROOT, "examples", "de_bruijn_tips_ranks"), path, out, "1"], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, KMI_FORCE_DIST="1"))
        assert p.returncode == 0, p.stderr
        got = _read_fasta(out)
        q = subprocess.run([os.path.join(ROOT, "examples", "de_bruijn_tips"), path, "1"], capture_output=True, text=True, timeout=300)
        assert q.returncode == 0, q.stderr
    one = dict(ln.split("\t") for ln in q.stdout.strip().split("\n") if "\t" in ln)
    steps = [ln.split() for ln in p.stdout.strip().split("\n") if ln.startswith("rank 0 of 1 ")]
    assert [x[4] for x in steps] == ["build", "retain_counts", "prune_edges"] + ["clip_tips"] * int(one["rounds"]) + ["unitigs"]
    last = dict(zip(steps[-1][4::2], steps[-1][5::2]))
    assert (last["rounds"], last["nodes"], last["unitigs"], last["total_unitigs"]) == (one["rounds"], one["nodes_final"], one["unitigs_final"],
                                                                                     one["unitigs_final"])
    assert (one["rounds"], one["unitigs_final"]) == ("2", "19")
    assert len(got) == int(one["unitigs_final"]) and D.n50([len(x) for x in got]) == int(one["n50_final"])
    ctx = K.Context(0)
    g = K.DeBruijnNodes(ctx, K.make_config(31))
    try:
        g.build(data)
        g.retain_counts(int(one["threshold"]))
        g.prune_edges(1)
        while g.clip_tips(1, 62)["n_tips_clipped"]:
            g.prune_edges(1)
        g.prune_edges(1)
        assert sorted(got) == sorted(x.decode() for x in g.unitig_sequences(1))
        cur, _ = D.prune(M.graph_of_reads(reads, 31), 1)
        for _ in range(2):
            cur, _ = T.clip(cur, 1, 62)
            cur, _ = D.prune(cur, 1)
        assert sorted(got) == [x for x, _, _ in M.unitigs_from_strings(cur)]
    finally:
        g.close()
        ctx.close()
