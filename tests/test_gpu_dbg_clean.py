"""Cleaning a de Bruijn node map on the GPU (DeBruijnNodes.spectrum / retain_counts / prune_edges) against the plain-Python model
(tests/dbg_clean_model.py). The model's input is always the oracle's node map, never the GPU's; the unitigs afterwards are checked
against tests/unitig_model.py on the model's map."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import dbg_clean_model as D
from tests import oracle as orc
from tests import unitig_model as M

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "data")
MAX = 2**32 - 1
KS = [15, 21, 32, 33, 63, 96]   # below the super-k-mer path, one word full, two words, three words


@pytest.fixture(scope="module")
def ctx():
    import kmerind_amd as K
    c = K.Context(0)
    yield c
    c.close()


def _genome(rng, n):
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, n)])


@functools.lru_cache(maxsize=None)
def _synthetic_reads(seed, k, n_reads=500):
    """branching reads: a genome with repeats longer than k, SNP variants, a poly-A stretch, both strands"""
    rng = np.random.default_rng(seed)
    g = _genome(rng, 2400)
    rep = g[400:400 + 3 * k]
    g = g[:1000] + rep + g[1000:1600] + rep + g[1600:] + "A" * (2 * k) + _genome(rng, 300)
    snp = list(g)
    for p in rng.integers(0, len(g), 8):
        snp[p] = "ACGT"[("ACGT".index(snp[p]) + 1) % 4]
    snp = "".join(snp)
    reads = []
    for i in range(n_reads):
        src = snp if i % 5 == 0 else g
        p = int(rng.integers(0, len(src) - 130))
        r = src[p:p + int(rng.integers(max(k + 2, 60), 130))]
        reads.append(M.revcomp(r) if rng.random() < 0.5 else r)
    return D.fastq(reads)


def _golden(name):
    return open(os.path.join(GOLD, name), "rb").read()


def _oracle_export(tuples, k, exists=False):
    om = orc.DbgMap(orc.kspec(k), exists_only=exists)
    om.insert(*tuples)
    return om.export(canonical=True)


def _oracle_nodes(tuples, k, exists=False):
    return D.nodes_of(*_oracle_export(tuples, k, exists), k)


def _parse(data, k):
    return orc.dbg_parse(orc.kspec(k), data)


def _gpu_nodes(g, k):
    keys, cnt = g.to_vector()
    nodes = D.nodes_of(keys, cnt, k)
    assert len(nodes) == keys.shape[0]
    return nodes


def _gpu_unitigs(g, t=1):
    from kmerind_amd.core import split_unitigs
    off, bases, occ, circ = g.unitigs(t)
    return sorted((s.decode(), int(o), bool(c)) for s, o, c in zip(split_unitigs(off, bases), occ, circ))


def _keys_of(nodes, n_words):
    return np.array([M.encode_kmer(v, n_words) for v in nodes], dtype=np.uint64).reshape(-1, n_words)


# ---- spectrum
@pytest.mark.parametrize("name,k", [("test.debruijn.small.fastq", 21), ("test.debruijn.small.fastq", 31), ("natural.withN.fastq", 21)])
def test_spectrum_of_golden_fastq(ctx, name, k):
    import kmerind_amd as K
    data = _golden(name)
    occ = _oracle_export(_parse(data, k), k)[1][:, 8].astype(np.int64)
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    g.build(data)
    for n_bins in (2, 256, 65536):
        hist, totals = g.spectrum(n_bins)
        exp = np.bincount(np.minimum(occ, n_bins - 1), minlength=n_bins)
        assert hist.dtype == np.uint64 and (hist == exp).all(), n_bins
        assert totals == dict(n_entries=occ.size, sum_counts=int(occ.sum()), min_count=int(occ.min()), max_count=int(occ.max()))
        assert (hist.tolist(), totals) == D.spectrum(_oracle_nodes(_parse(data, k), k), n_bins)
    g.close()


def test_spectrum_edge_cases(ctx):
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    g = K.DeBruijnNodes(ctx, K.make_config(21))
    hist, totals = g.spectrum(16)
    assert not hist.any() and totals == dict(n_entries=0, sum_counts=0, min_count=0, max_count=0)
    h = np.zeros(4, np.uint64)
    for n_bins in (0, 1, L.SPECTRUM_MAX_BINS + 1):
        assert L.lib.kmi_dbg_spectrum_host(g.h, n_bins, h.ctypes.data_as(C.c_void_p), None) == L.ERR_INVALID
    assert L.lib.kmi_dbg_spectrum_host(g.h, 4, None, None) == L.ERR_INVALID
    g.close()
    ge = K.DeBruijnNodes(ctx, K.make_config(21), exists_only=True)
    ge.build(_golden("test.debruijn.tiny.fastq"))
    assert L.lib.kmi_dbg_spectrum_host(ge.h, 4, h.ctypes.data_as(C.c_void_p), None) == L.ERR_INVALID
    ge.close()


# ---- retain
@pytest.mark.parametrize("k", KS)
def test_retain_counts_against_the_model(ctx, k):
    import kmerind_amd as K
    data = _synthetic_reads(k, k)
    tuples = _parse(data, k)
    nodes = _oracle_nodes(tuples, k)
    more = _parse(_synthetic_reads(k + 1000, k, 60), k)
    extra = _oracle_nodes(more, k)
    assert sum(1 for c in nodes.values() if c[8] == 1) > 0 and sum(1 for c in nodes.values() if 3 <= c[8] <= 5) > 0
    for lo, hi in [(2, MAX), (1, 1), (3, 5), (0, MAX), (MAX, MAX)]:
        g = K.DeBruijnNodes(ctx, K.make_config(k))
        g.build(data)
        keys0, cnt0 = g.to_vector()
        want = D.retain(nodes, lo, hi)
        g.unitigs()
        assert g.retain_counts(lo, hi) == len(nodes) - len(want), (lo, hi)
        assert g.local_size() == len(want)
        keys1, cnt1 = g.to_vector()
        mask = (cnt0[:, 8] >= lo) & (cnt0[:, 8] <= hi)
        assert (keys1 == keys0[mask]).all() and (cnt1 == cnt0[mask]).all(), (lo, hi)   # old order, bit for bit
        assert _gpu_nodes(g, k) == want, (lo, hi)
        if (lo, hi) == (0, MAX):
            assert len(want) == len(nodes)
        if (lo, hi) == (MAX, MAX):
            assert len(want) == 0
        if (lo, hi) in ((2, MAX), (MAX, MAX)):   # afterwards the map works as any map does
            q = _keys_of(list(nodes)[::5], g.n_words)
            fk, fv = g.find(q)
            found = D.nodes_of(fk, fv, k)
            assert found == {v: want[v] for v in list(nodes)[::5] if v in want}
            assert _gpu_unitigs(g) == M.unitigs_from_strings(want)
            victims = list(want)[::3]
            assert g.erase(_keys_of(victims, g.n_words)) == len(victims) if victims else True
            left = {v: c for v, c in want.items() if v not in set(victims)}
            g.insert(*more)
            merged = {v: list(c) for v, c in left.items()}
            for v, c in extra.items():
                merged[v] = [a + b for a, b in zip(merged.get(v, [0] * 9), c)]
            assert _gpu_nodes(g, k) == merged, (lo, hi)
            assert _gpu_unitigs(g) == M.unitigs_from_strings(merged)
        g.close()


def test_retain_more_nodes_in_a_bucket_than_one_tile(ctx):
    """10 M distinct nodes: every fine bucket holds more entries than one tile of the row compaction (256)"""
    import kmerind_amd as K
    rng = np.random.default_rng(11)
    keys = np.unique(rng.integers(0, 1 << 62, 10_000_000, dtype=np.uint64))
    twice = keys[keys % np.uint64(3) == 0]
    kmers = np.concatenate([keys, twice]).reshape(-1, 1)
    edges = ((kmers[:, 0] >> np.uint64(7)) & np.uint64(0xFF)).astype(np.uint8)
    g = K.DeBruijnNodes(ctx, K.make_config(31))
    g.insert(kmers, edges)
    keys0, cnt0 = g.to_vector()
    assert keys0.shape[0] > 9_900_000 and set(np.unique(cnt0[:, 8]).tolist()) >= {1, 2}
    mask = cnt0[:, 8] == 2
    assert g.retain_counts(2, 2) == int((~mask).sum())
    assert ctx.debug_counter(9) > 256
    keys1, cnt1 = g.to_vector()
    assert keys1.shape[0] == int(mask.sum()) and (keys1 == keys0[mask]).all() and (cnt1 == cnt0[mask]).all()
    g.close()


# ---- prune
def _one_sided(k):
    """records as the parser emits them, with the in nibble of every third and the out nibble of every fifth edge byte cleared: a
    counter then exists on one side only"""
    kmers, edges = _parse(_synthetic_reads(k + 7, k, 80), k)
    edges = edges.copy()
    edges[::3] &= 0x0F
    edges[::5] &= 0xF0
    return kmers, edges


def _palindromes(k):
    rng = np.random.default_rng(k)
    reads = []
    for _ in range(6):
        s = _genome(rng, k // 2)
        left, right = _genome(rng, 40), _genome(rng, 40)
        r = left + s + M.revcomp(s) + right
        reads += [r, M.revcomp(r), left + s + M.revcomp(s), M.revcomp(right) + s + M.revcomp(s)]
    return D.fastq(reads)


def _repeats(k):
    return D.fastq(["A" * (2 * k), "AC" * k, "T" * (2 * k), "GA" * k + "C", "ACG" * k])


# name -> (k list, what to insert, edits on the GPU map and on the model alike, EDGE_EXISTS)
PRUNE_CASES = {
    "synthetic": (KS + [22], lambda k: _parse(_synthetic_reads(k, k), k), None, False),
    "withN": ([21], lambda k: _parse(_golden("natural.withN.fastq"), k), None, False),
    "erased": ([21, 32], lambda k: _parse(_synthetic_reads(k, k), k), "erase", False),
    "retained": ([21, 33], lambda k: _parse(_synthetic_reads(k, k), k), "retain", False),
    "one_sided": ([21, 22, 63], _one_sided, None, False),
    "palindromes": ([22, 32], lambda k: _parse(_palindromes(k), k), None, False),
    "repeats": ([15, 22, 33], lambda k: _parse(_repeats(k), k), None, False),
    "exists": ([31], lambda k: _parse(_golden("test.debruijn.small.fastq"), k), None, True),
}
PRUNE_PARAMS = [(name, k, t) for name, (ks, _, _, ex) in PRUNE_CASES.items() for k in ks for t in ((1,) if ex else (1, 2, 3))]


@functools.lru_cache(maxsize=None)
def _prune_model_input(name, k):
    _, make, edit, exists = PRUNE_CASES[name]
    nodes = _oracle_nodes(make(k), k, exists)
    if edit == "erase":
        gone = set(list(nodes)[::7])
        nodes = {v: c for v, c in nodes.items() if v not in gone}
    elif edit == "retain":
        nodes = D.retain(nodes, 2, MAX)
    return nodes


def _prune_gpu_input(ctx, name, k):
    import kmerind_amd as K
    _, make, edit, exists = PRUNE_CASES[name]
    g = K.DeBruijnNodes(ctx, K.make_config(k), exists_only=exists)
    g.insert(*make(k))
    if edit == "erase":
        victims = list(_oracle_nodes(make(k), k, exists))[::7]
        assert g.erase(_keys_of(victims, g.n_words)) == len(victims)
    elif edit == "retain":
        g.retain_counts(2)
    return g


def test_the_prune_cases_hold_every_class():
    """the model's inputs hold counters of each of the three classes, so the comparisons below cannot pass empty"""
    seen = dict.fromkeys(D.STATS, 0)
    exempt = 0
    for name, k, t in PRUNE_PARAMS:
        nodes = _prune_model_input(name, k)
        _, s = D.prune(nodes, t, PRUNE_CASES[name][3])
        for f in D.STATS:
            seen[f] += s[f]
        exempt += sum(1 for v in nodes for j in range(8) if nodes[v][j] >= t and D.neighbour(v, j)[2])
    assert seen["n_weak"] > 0 and seen["n_absent"] > 0 and seen["n_unreciprocated"] > 0 and seen["n_isolated"] > 0 and seen["n_set_after"] > 0
    assert exempt > 0   # (palindromic nodes or neighbours: rule 3's exemption is exercised)
    for name in ("withN", "erased", "retained", "one_sided"):
        k = PRUNE_CASES[name][0][0]
        s = D.prune(_prune_model_input(name, k), 1)[1]
        assert s["n_absent"] + s["n_unreciprocated"] > 0, name


@pytest.mark.parametrize("name,k,t", PRUNE_PARAMS)
def test_prune_edges_against_the_model(ctx, name, k, t):
    exists = PRUNE_CASES[name][3]
    nodes = _prune_model_input(name, k)
    want, stats = D.prune(nodes, t, exists)
    g = _prune_gpu_input(ctx, name, k)
    assert _gpu_nodes(g, k) == nodes
    got = g.prune_edges(t)
    print(name, k, t, got)
    assert got == stats and g.prune_totals == stats
    assert _gpu_nodes(g, k) == want
    keys1, cnt1 = g.to_vector()
    # a second call clears nothing and leaves the map bit-identical
    again = g.prune_edges(t)
    assert (again["n_weak"], again["n_absent"], again["n_unreciprocated"]) == (0, 0, 0)
    assert again["n_set_before"] == again["n_set_after"] == stats["n_set_after"] and again["n_isolated"] == stats["n_isolated"]
    keys2, cnt2 = g.to_vector()
    assert (keys2 == keys1).all() and (cnt2 == cnt1).all()
    # the unitigs of the pruned map, the same for every threshold 1..t
    exp = M.unitigs_from_strings(want, t)
    for u in range(1, t + 1):
        assert _gpu_unitigs(g, u) == exp, u
    g.close()


def test_prune_an_empty_map(ctx):
    import kmerind_amd as K
    g = K.DeBruijnNodes(ctx, K.make_config(21))
    assert g.prune_edges(1) == dict.fromkeys(D.STATS, 0)
    assert g.retain_counts(2) == 0 and g.local_size() == 0
    g.close()


# ---- the pipeline: spectrum -> retain -> prune -> unitigs
@pytest.mark.parametrize("k,built,retained,absent", [(15, 29, 18, 17), (21, 29, 18, 17), (22, 29, 18, 17), (31, 29, 18, 17), (32, 29, 18, 17),
                                                     (33, 29, 18, 17), (63, 17, 6, 5)])
def test_the_pipeline_mends_the_unitigs(ctx, k, built, retained, absent):
    import kmerind_amd as K
    genome, reads = D.pipeline_reads(k)
    data = D.fastq(reads)
    nodes = _oracle_nodes(_parse(data, k), k)
    kept = D.retain(nodes, 2, MAX)
    pruned, stats = D.prune(kept, 1)
    assert (len(M.unitigs_from_strings(nodes)), len(M.unitigs_from_strings(kept)), stats["n_absent"]) == (built, retained, absent)
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    g.build(data)
    assert len(_gpu_unitigs(g)) == built
    hist, _ = g.spectrum(8)
    assert hist.tolist() == D.spectrum(nodes, 8)[0] and hist[1] > 0
    assert g.retain_counts(2) == len(nodes) - len(kept) == int(hist[1])
    assert len(_gpu_unitigs(g)) == retained
    assert g.prune_edges(1) == stats
    got = _gpu_unitigs(g)
    assert len(got) == 1 and got[0][0] == min(genome, M.revcomp(genome)) and got == M.unitigs_from_strings(pruned)
    g.close()


# ---- refusals, each leaving the map as it was
def test_refusals_leave_the_map_unchanged(ctx):
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    data = _golden("test.debruijn.tiny.fastq")
    n, st = C.c_uint64(), L.DbgPruneStats()

    def same(g, before):
        keys, cnt = g.to_vector()
        return (keys == before[0]).all() and (cnt == before[1]).all()
    g = K.DeBruijnNodes(ctx, K.make_config(21))
    g.build(data)
    before = g.to_vector()
    g.unitigs()
    assert L.lib.kmi_dbg_prune_edges(g.h, 0, C.byref(st)) == L.ERR_INVALID and same(g, before)
    assert L.lib.kmi_dbg_retain_counts(g.h, 3, 2, C.byref(n)) == L.ERR_INVALID and same(g, before)
    assert L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0) == L.OK   # a call that fails leaves the unitigs too
    # each of the three mutating calls drops the unitigs of an earlier compaction
    for call in (lambda: g.retain_counts(0), lambda: g.prune_edges(1), lambda: g.retain_counts(2)):
        g.unitigs()
        assert L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0) == L.OK
        call()
        assert L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0) == L.ERR_INVALID
    g.close()
    g5 = K.DeBruijnNodes(ctx, K.make_config(21, "DNA5"))
    g5.build(data)
    before = g5.to_vector()
    assert L.lib.kmi_dbg_prune_edges(g5.h, 1, C.byref(st)) == L.ERR_INVALID and same(g5, before)
    assert g5.retain_counts(0) == 0 and same(g5, before)   # (the filter takes every alphabet)
    g5.close()
    ge = K.DeBruijnNodes(ctx, K.make_config(21), exists_only=True)
    ge.build(data)
    before = ge.to_vector()
    assert L.lib.kmi_dbg_retain_counts(ge.h, 0, 1, C.byref(n)) == L.ERR_INVALID and same(ge, before)
    h = np.zeros(4, np.uint64)
    assert L.lib.kmi_dbg_spectrum_host(ge.h, 4, h.ctypes.data_as(C.c_void_p), None) == L.ERR_INVALID and same(ge, before)
    ge.close()
