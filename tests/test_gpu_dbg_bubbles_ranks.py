"""Popping the bubbles of a de Bruijn node map held over ranks (DeBruijnNodes.pop_bubbles(comm=...) / kmi_dbg_pop_bubbles_dist_host).
The expected value is always the plain-Python model (tests/bubbles_model.pop) on the model's WHOLE map: unitig_model.graph_of_reads
on the reads, put through dbg_clean_model.prune and bubbles_model.clean_tips where the GPU map went through them. Every comparison
first asserts that the union of the ranks' maps before the call is the model's input with no node on two ranks. After the call:
each rank's keys are its old keys minus the leavers in order, the rows are the model's word for word, the totals are the model's
stats on every rank, the ranks' local stats add up to them field by field, and n_unitigs equals kmi_dbg_compact_dist_host's total
on a twin build. Two and four processes share the GPU over a gloo group, started as tests/test_gpu_dbg_tips_ranks.py starts them;
several read sets share one spawn."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import bubbles_model as B
from tests import dbg_clean_model as D
from tests import unitig_model as M
from tests.test_gpu_dbg_bubbles import _fuzz_case
from tests.test_gpu_dbg_tips_ranks import _Comm, _free_port, _read_fasta, _record_shares, _same, _units

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX_BYTES, EX_SENT = 17, 16   # kmi_ctx_debug_counter: bytes and exchanges of the context's last kmi_dbg_pop_bubbles_dist_host
COUNTS = ("n_unitigs", "n_branches", "n_bubbles", "n_popped", "n_nodes_removed", "n_counters_cleared")


def _case(reads, k, world, t=1, m=None, exists=False, prune=True, tips=False, parts=None, **more):
    return dict(reads=reads, k=k, t=t, m=2 * k if m is None else m, exists=exists, prune=prune, tips=tips,
                parts=_record_shares(reads, world) if parts is None else parts, **more)


def _one_case(K, L, ctx, comm, rank, c):
    def build():
        g = K.DeBruijnNodes(ctx, K.make_config(c["k"]), exists_only=c["exists"])
        g.build_dist(c["parts"][rank], comm)
        if c["prune"]:
            g.prune_edges(c["t"], comm=comm)
        tips = c["tips"]
        while tips:   # the tip rounds of the cleaning pipeline, over ranks
            g.clip_tips(c["t"], comm=comm)
            tips = g.clip_totals["n_tips_clipped"] > 0
            g.prune_edges(c["t"], comm=comm)
        return g
    g = build()
    out = dict(before=g.to_vector())
    out["local"] = g.pop_bubbles(c["t"], c["m"], comm=comm)
    out["total"] = dict(g.pop_totals)
    out["after"] = g.to_vector()
    out["export"] = L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0)
    out["sent"] = (ctx.debug_counter(EX_SENT), ctx.debug_counter(EX_BYTES))
    if c.get("rounds"):   # still pruned; a second round pops nothing and leaves the arrays; the unitigs afterwards
        g.prune_edges(c["t"], comm=comm)
        out["pruned_again"] = dict(g.prune_totals)
        out["after_prune"] = _same(out["after"], g.to_vector())
        g.pop_bubbles(c["t"], c["m"], comm=comm)
        out["second"] = dict(g.pop_totals)
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
    """refusals on every rank, then the one-rank call on a share, then what a successful call does to the compaction's result"""
    g = K.DeBruijnNodes(ctx, K.make_config(job["k"]))
    g.build_dist(job["parts"][rank], comm)
    g.prune_edges(1, comm=comm)
    before = g.to_vector()
    g.unitigs(comm=comm)
    sl, st = L.DbgPopStats(), L.DbgPopStats()
    out = dict(refused=[])
    for t, m, flags in ((0, 42, 0), (1, 0, 0), (1, 42, 1)):
        status = L.lib.kmi_dbg_pop_bubbles_dist_host(g.h, comm.h, t, m, flags, C.byref(sl), C.byref(st))
        out["refused"].append(dict(status=status, stats=[getattr(x, f) for x in (sl, st) for f in B.STATS], same=_same(before, g.to_vector()),
                                   unitigs=L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0)))
    out["plain"] = L.lib.kmi_dbg_pop_bubbles(g.h, 1, 42, 0, C.byref(sl))
    out["plain_same"] = _same(before, g.to_vector())
    out["ok"] = L.lib.kmi_dbg_pop_bubbles_dist_host(g.h, comm.h, 1, 42, 0, None, None)   # (both outputs may be NULL)
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
    if c["tips"]:
        nodes = B.clean_tips(nodes, c["t"], exists=c["exists"])
    want, stats = B.pop(nodes, c["t"], c["m"], c["exists"], trace)
    return nodes, want, stats


def _compare(c, per_rank, trace=None):
    """one case against the model -> (nodes before, after, stats, owner: node -> rank before the call)"""
    from kmerind_amd import _lib as L
    k = c["k"]
    nodes, want, stats = _model(c, trace)
    owner, after = {}, {}
    for r, res in enumerate(per_rank):
        part = D.nodes_of(*res["before"], k) if res["before"][0].shape[0] else {}
        assert not set(part) & set(owner), "a node on two ranks"
        owner.update(dict.fromkeys(part, r))
        assert all(part[v] == nodes.get(v) for v in part), "the map before the call is not the model's input"
    assert set(owner) == set(nodes), "the union of the maps before the call is not the model's input"
    print(k, c["t"], c["m"], c["exists"], c["prune"], stats, [res["local"] for res in per_rank])
    for r, res in enumerate(per_rank):
        keys0, keys1 = res["before"][0], res["after"][0]
        strs0 = M.decode_keys(keys0, k) if keys0.shape[0] else []
        stay = np.array([s in want for s in strs0], dtype=bool)
        assert keys1.shape == keys0[stay].shape and (keys1 == keys0[stay]).all(), r      # its old keys minus the leavers, in order
        part = D.nodes_of(*res["after"], k) if keys1.shape[0] else {}
        assert list(part) == [s for s in strs0 if s in want]
        assert all(part[v] == want[v] for v in part), r                                   # word for word, counts[8] among them
        after.update(part)
        assert res["total"] == stats, (r, res["total"], stats)
        loc = res["local"]
        assert loc["n_nodes"] == keys0.shape[0] and loc["n_nodes_removed"] == keys0.shape[0] - keys1.shape[0]
        assert loc["n_counters_cleared"] == sum(1 for v in part for a, b in zip(nodes[v][:8], part[v][:8]) if a != b)
        assert res["export"] == L.ERR_INVALID and res["twin_unitigs"] == stats["n_unitigs"]
    assert after == want
    for f in B.STATS:
        assert sum(res["local"][f] for res in per_rank) == stats[f], f
    return nodes, want, stats, owner


def _counts(s):
    return tuple(s[f] for f in COUNTS)


# ---- 1. the pipeline input after the tip rounds over ranks, one and two key words, two and four ranks
@pytest.mark.parametrize("k,world", [(21, 2), (33, 2), (21, 4)])
def test_the_pipeline_input_after_the_tip_rounds_over_ranks(k, world):
    genome, reads = D.pipeline_reads(k)
    c = _case(reads, k, world, tips=True, rounds=True)
    (res,) = zip(*_run(world, dict(kind="cases", cases=[c])))
    nodes, want, s, owner = _compare(c, res)
    assert _counts(s) == (19, 12, 6, 6, 6 * k, 12)
    for r in res:
        p = r["pruned_again"]
        assert p["n_set_before"] == p["n_set_after"] and r["after_prune"]   # prune_edges(1) clears nothing
        z = r["second"]
        assert _counts(z) == (1, 0, 0, 0, 0, 0) and z["n_nodes"] == len(want) and r["second_same"]
        assert r["sent"][0] > 0 and r["sent"][1] > 0
    (u,) = [x for r in res for x in r["units"]]
    assert u[0] in (genome, M.revcomp(genome)) and not u[2]


# ---- 2. three key words
def test_three_key_words_over_two_ranks():
    c = _case(B.substitution_reads(65, 65), 65, 2)
    (res,) = zip(*_run(2, dict(kind="cases", cases=[c])))
    nodes, want, s, owner = _compare(c, res)
    assert _counts(s) == (4, 2, 1, 1, 65, 2)
    assert res[0]["before"][0].shape[1] == 3 and len(M.unitigs_from_strings(want)) == 1


# ---- 3. limits, unequal lengths, ties and orientations, in one spawn
def test_limits_unequal_lengths_ties_and_orientations_over_two_ranks():
    k = 21
    cases, checks = [], []

    def add(reads, m, check):
        cases.append(_case(reads, k, 2, m=m))
        checks.append(check)

    def popped(bubbles, n_popped, removed, whole):
        def check(nodes, want, s, trace):
            assert (s["n_bubbles"], s["n_popped"], s["n_nodes_removed"]) == (bubbles, n_popped, removed)
            assert (want == nodes) == (n_popped == 0) and (len(M.unitigs_from_strings(want)) == 1) == whole
        return check
    add(B.substitution_reads(k, 1), k, popped(1, 1, k, True))
    add(B.substitution_reads(k, 1), k - 1, popped(1, 0, 0, False))
    # a light deletion branch of k - 1 nodes is popped with M = k - 1 although its heavier sibling has k > M nodes; a heavy one leaves
    # the lighter sibling of k nodes alone with M = k - 1; with M = k the sibling is popped
    add(B.deletion_reads(k, 1, 2, 1), k - 1, popped(1, 1, k - 1, True))
    add(B.deletion_reads(k, 1, 1, 2), k - 1, popped(1, 0, 0, False))
    add(B.deletion_reads(k, 1, 1, 2), k, popped(1, 1, k, True))

    def three_way(nodes, want, s, trace):
        assert (s["n_branches"], s["n_bubbles"], s["n_popped"], s["n_nodes_removed"]) == (3, 1, 2, 2 * k)
        assert sorted((x[1][:2], x[3]) for x in trace) == [((1, 1), True), ((2, 2), True), ((3, 3), False)]

    def tie(nodes, want, s, trace):
        (kept,), (lost,) = [x for x in trace if not x[3]], [x for x in trace if x[3]]
        assert kept[1][:2] == lost[1][:2] == (1, 1) and s["n_popped"] == 1
        # the same two junction nodes, the smaller first; there the smaller base stays
        assert kept[0][0][2] == lost[0][0][2] < kept[0][1][2] == lost[0][1][2] and kept[0][0][3] < lost[0][0][3]
        assert kept[0][0][0] in want and lost[0][0][0] not in want
    for seed in (5, 6):
        add(B.three_way_reads(k, seed), k, three_way)
        add(B.substitution_reads(k, seed, 1, 1), k, tie)
    seen = set()

    def strand(nodes, want, s, trace):
        (lost,) = [x for x in trace if x[3]]
        assert s["n_popped"] == 1 and lost[2] == k
        seen.update((i, lost[0][i][3] >> 2) for i in range(2))
    for seed in range(4):   # the same bubble read from either strand, as test_gpu_dbg_bubbles.py::test_orientations does
        for rc in (False, True):
            reads = B.substitution_reads(k, seed)
            add([M.revcomp(r) for r in reads] if rc else reads, 2 * k, strand)
    res = list(zip(*_run(2, dict(kind="cases", cases=cases))))
    for c, check, per_rank in zip(cases, checks, res):
        trace = []
        nodes, want, s, owner = _compare(c, per_rank, trace)
        check(nodes, want, s, trace)
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ---- 4. fuzz
FUZZ_SETS = 48
FUZZ_EXTRA = ()   # later sets of the same stream for a situation that the first 48 miss over two ranks: none is needed (4, 10, 6, 2)


def _fuzz_cases(world, extra=()):
    """sets 0 .. FUZZ_SETS - 1 of the generator's stream, then those named in `extra`"""
    rng = np.random.default_rng(5)
    cases = []
    for i in range(max((FUZZ_SETS - 1,) + tuple(extra)) + 1):
        reads, t, exists, prune, m = _fuzz_case(rng, 5, i)   # (every set is drawn, kept or not: the stream is test_fuzz_k5's)
        if i < FUZZ_SETS or i in extra:
            cases.append(_case(reads, 5, world, t, m, exists, prune))
    return cases


@pytest.mark.parametrize("world", [2, 4])
def test_fuzz_k5_over_ranks(world):
    """the first 48 read sets of test_gpu_dbg_bubbles.py::test_fuzz_k5 with its parameter schedule; the model's sums over them are
    asserted, so the comparison cannot pass empty. Over two ranks the situations that one-rank code never meets must each have
    occurred: a popped branch whose two junction nodes are on different ranks; a popped branch and the sibling that outweighs it
    whose attached nodes at a shared junction are on different ranks; a popped branch with a node on another rank than both its
    junction nodes; a rank that cleared a counter while none of its nodes left. They are counted from the model's trace and the
    observed owners."""
    cases = _fuzz_cases(world, FUZZ_EXTRA if world == 2 else ())
    res = list(zip(*_run(world, dict(kind="cases", cases=cases))))
    sums = dict.fromkeys(B.STATS, 0)
    far_junctions = split_siblings = far_node = cleared_without_leaver = 0
    for i, (c, per_rank) in enumerate(zip(cases, res)):
        trace = []
        nodes, want, s, owner = _compare(c, per_rank, trace)
        for f in B.STATS:
            sums[f] += s[f] if i < FUZZ_SETS else 0
        families = {}
        for x in trace:
            families.setdefault(frozenset((w, j >> 2) for _, _, w, j in x[0]), []).append(x)
        for js, key, n_nodes, popped in trace:
            if not popped:
                continue
            far_junctions += owner[js[0][2]] != owner[js[1][2]]
            far_node += any(owner[v] not in (owner[js[0][2]], owner[js[1][2]]) for v, _, _, _ in js)
            greater = [y for y in families[frozenset((w, j >> 2) for _, _, w, j in js)] if y[1] > key]
            split_siblings += any(owner[y[0][e][0]] != owner[js[e][0]] for y in greater for e in range(2))
        cleared_without_leaver += sum(1 for r in per_rank if r["local"]["n_counters_cleared"] > 0 and r["local"]["n_nodes_removed"] == 0)
    print(world, sums, far_junctions, split_siblings, far_node, cleared_without_leaver)
    assert tuple(sums[f] for f in B.STATS[:7]) == (1738, 825, 137, 24, 13, 49, 26)
    if world == 2:
        assert far_junctions > 0 and split_siblings > 0 and far_node > 0 and cleared_without_leaver > 0


# ---- 5. cycles, hairpins, an island and a homopolymer; an EDGE_EXISTS map
def test_cycles_hairpins_and_an_edge_exists_map_over_two_ranks():
    k = 21
    rng = np.random.default_rng(3)
    ring = B.rand_seq(rng, 30)
    half = B.rand_seq(rng, k + 4)
    reads = [B.rand_seq(rng, k + 2), ring + ring + ring[:k], half + M.revcomp(half), "A" * (k + 3)]
    genome, pipe = D.pipeline_reads(k)
    cases = [_case(reads, k, 2, m=64), _case(pipe, k, 2, exists=True, tips=True)]
    res = list(zip(*_run(2, dict(kind="cases", cases=cases))))
    nodes, want, s, owner = _compare(cases[0], res[0])
    assert want == nodes and (s["n_branches"], s["n_bubbles"], s["n_popped"], s["n_nodes_removed"]) == (0, 0, 0, 0)
    assert all(_same(r["before"], r["after"]) for r in res[0])
    trace = []
    nodes, want, s, owner = _compare(cases[1], res[1], trace)
    assert (s["n_bubbles"], s["n_popped"]) == (6, 6) and all(x[1][:2] == (1, 1) for x in trace)   # every key ties on value


# ---- 6. ranks that own nothing
EMPTY_RANK_SEED = 18   # bubbles_model.substitution_reads(5, seed): the first seed whose map leaves one rank of four without a node (8, 5, 4, 0)


def test_empty_shares_and_an_empty_world():
    """all reads on rank 0 (the nodes still spread by hash); a map of about a dozen nodes that leaves a rank of four with no node at
    all (substitution_reads(5, EMPTY_RANK_SEED)); an empty world"""
    reads, small = B.substitution_reads(21, 2), B.substitution_reads(5, EMPTY_RANK_SEED)
    cases = [_case(reads, 21, 4, parts=[D.fastq(reads), b"", b"", b""]), _case(small, 5, 4, parts=[D.fastq(small), b"", b"", b""]),
             _case([], 21, 4, parts=[b""] * 4)]
    res = list(zip(*_run(4, dict(kind="cases", cases=cases))))
    nodes, want, s, owner = _compare(cases[0], res[0])
    assert s["n_popped"] == 1 and s["n_nodes_removed"] == 21
    nodes, want, s, owner = _compare(cases[1], res[1])
    print(sorted(r["local"]["n_nodes"] for r in res[1]), s)
    assert nodes and min(r["local"]["n_nodes"] for r in res[1]) == 0
    nodes, want, s, owner = _compare(cases[2], res[2])
    assert not nodes and s == dict.fromkeys(B.STATS, 0)
    assert all(r["local"] == s and r["total"] == s and r["before"][0].shape[0] == 0 for r in res[2])


# ---- 7. the code of several ranks on one rank
def test_one_rank_forced_distributed_gives_the_one_rank_result(monkeypatch):
    """the rank as its own peer: the arrays and all eight stats of kmi_dbg_pop_bubbles on a second build of the same input. Two builds
    need not place a bucket's nodes in the same order, so the two maps are compared row for row in key order, and the forced call's
    own order against its own map before the call"""
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    k = 21
    genome, reads = D.pipeline_reads(k)
    nodes = B.clean_tips(D.prune(M.graph_of_reads(reads, k), 1)[0])
    want, stats = B.pop(nodes, 1, 2 * k)
    monkeypatch.setenv("KMI_FORCE_DIST", "1")
    ctx = K.Context(0, rank=0, nranks=1)
    h = C.c_void_p()
    ctx.check(L.lib.kmi_comm_create(ctx.h, None, C.byref(h)))
    g = g1 = None

    def build():
        x = K.DeBruijnNodes(ctx, K.make_config(k))
        x.build(D.fastq(reads))
        x.prune_edges(1)
        while x.clip_tips(1)["n_tips_clipped"]:
            x.prune_edges(1)
        x.prune_edges(1)
        return x
    try:
        g = build()
        keys0, cnt0 = g.to_vector()
        strs0 = M.decode_keys(keys0, k)
        assert D.nodes_of(keys0, cnt0, k) == nodes, "the map before the call is not the model's input"
        local = g.pop_bubbles(1, comm=_Comm(h))
        assert local == g.pop_totals == stats and stats["n_popped"] == 6
        assert ctx.debug_counter(EX_BYTES) > 0 and ctx.debug_counter(EX_SENT) > 0
        g1 = build()
        assert g1.pop_bubbles(1) == stats
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
    reads = B.substitution_reads(21, 2)
    res = _run(2, dict(kind="contract", k=21, parts=_record_shares(reads, 2)))
    for r in res:
        for x in r["refused"]:
            assert x["status"] == L.ERR_INVALID and x["stats"] == [0] * 16 and x["same"] and x["unitigs"] == L.OK, x
        assert r["plain"] == L.ERR_INVALID and r["plain_same"]
        assert r["ok"] == L.OK and r["unitigs_after"] == L.ERR_INVALID   # dropped on every rank, whether it lost a node or not
    assert sum(r["removed"] for r in res) == 21


# ---- 9. the facade's example
def test_facade_example_through_the_collective_code():
    """examples/de_bruijn_bubbles_ranks under KMI_FORCE_DIST=1 leaves the unitigs that examples/de_bruijn_bubbles leaves on the same
    file (the cleaning pipeline's input with min_count = 1): one unitig, the genome; its sequences one by one against the one-rank
    pipeline of the Python layer and the model's"""
    import kmerind_amd as K
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "de_bruijn_bubbles_ranks", "de_bruijn_bubbles"], stdout=subprocess.DEVNULL)
    genome, reads = D.pipeline_reads(31)
    data = D.fastq(reads)
    with tempfile.TemporaryDirectory() as d:
        path, out = os.path.join(d, "reads.fastq"), os.path.join(d, "ranks.fasta")
        with open(path, "wb") as f:
            f.write(data)
        p = subprocess.run([os.path.join(ROOT, "examples", "de_bruijn_bubbles_ranks"), path, out, "1"], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, KMI_FORCE_DIST="1"))
        assert p.returncode == 0, p.stderr
        got = _read_fasta(out)
        q = subprocess.run([os.path.join(ROOT, "examples", "de_bruijn_bubbles"), path, "1"], capture_output=True, text=True, timeout=300)
        assert q.returncode == 0, q.stderr
    one = dict(ln.split("\t") for ln in q.stdout.strip().split("\n") if "\t" in ln)
    steps = [ln.split() for ln in p.stdout.strip().split("\n") if ln.startswith("rank 0 of 1 ")]
    names = [x[4] for x in steps]
    assert names[:3] == ["build", "retain_counts", "prune_edges"] and names[-1] == "unitigs" and set(names[3:-1]) == {"clip_tips", "pop_bubbles"}
    last = dict(zip(steps[-1][4::2], steps[-1][5::2]))
    assert (last["passes"], last["nodes"], last["unitigs"], last["total_unitigs"]) == (one["passes"], one["nodes_final"], one["unitigs_final"],
                                                                                     one["unitigs_final"])
    pops = [dict(zip(x[5::2], x[6::2])) for x in steps if x[4] == "pop_bubbles"]   # (name value pairs behind the step's name)
    assert [(x["pass"], x["round"], x["total_popped"]) for x in pops] == [("1", "1", "6"), ("1", "2", "0"), ("2", "1", "0")]
    assert (one["passes"], one["unitigs_final"]) == ("2", "1") and got in ([genome], [M.revcomp(genome)])
    ctx = K.Context(0)
    g = K.DeBruijnNodes(ctx, K.make_config(31))
    try:
        g.build(data)
        g.retain_counts(1)
        g.prune_edges(1)
        while True:
            while g.clip_tips(1, 62)["n_tips_clipped"]:
                g.prune_edges(1)
            g.prune_edges(1)
            popped = 0
            while True:
                n = g.pop_bubbles(1, 62)["n_popped"]
                g.prune_edges(1)
                popped += n
                if not n:
                    break
            if not popped:
                break
        assert sorted(got) == sorted(x.decode() for x in g.unitig_sequences(1))
        cur = B.clean_tips(D.prune(M.graph_of_reads(reads, 31), 1)[0], 1, 62)
        cur, _ = B.pop(cur, 1, 62)
        cur, _ = D.prune(cur, 1)
        assert sorted(got) == [x for x, _, _ in M.unitigs_from_strings(cur)]
    finally:
        g.close()
        ctx.close()
