"""kmi_index_compare / kmi_index_combine against tests/setops_model.py: pairs of built indexes (one to two words, 2- and 3-bit
alphabets, dense and sparse), the two layouts crossed, buckets of several passes and of more than one compaction tile, the sentinel
key and stored zeros, the two reducers, and the edges. After every combine the result is used further (spectrum, built into again,
erased from) and b is shown not to have moved."""
import numpy as np
import pytest

from tests import index_model as M
from tests import oracle as orc
from tests import setops_model as SM
from tests import spectrum_cases as S

pytestmark = pytest.mark.gpu
CALLS = SM.OPS + ("compare",)
SHAPES = [(17, "DNA", "dense"), (17, "DNA", "sparse"), (31, "DNA", "dense"), (31, "DNA", "sparse"), (32, "DNA", "dense"), (32, "DNA", "sparse"),
          (63, "DNA", "dense"), (21, "DNA5", "dense")]
_B_CASES = {}


@pytest.fixture(scope="module")
def ctxs():
    out = S.make_contexts()
    yield out
    for c in out.values():
        c.close()


def _b_case(k, alphabet):
    """(FASTQ bytes, model) of the second sample of a shape: reads drawn with another seed over a genome whose first half is the
    first half of the genome behind S.reads_case's background reads. Shared, read-only."""
    key = (k, alphabet)
    if key not in _B_CASES:
        # (reads_case draws the adversarial reads and then the background genome from this generator)
        rng = np.random.default_rng(7000 + 10 * k + len(alphabet) + len("canonical"))
        M.adversarial_reads(rng, k)
        genome_a = M.random_seq(rng, 20_000)
        rng_b = np.random.default_rng(9100 + k)
        genome_b = genome_a[:10_000] + M.random_seq(rng_b, 10_000)
        data = M.fastq(M.background(rng_b, 300, genome=genome_b), tag=b"s")
        model = M.CountModel(k, S.ALPHA[alphabet], orc.CANONICAL)
        model.insert(orc.extract(orc.kspec(k, S.ALPHA[alphabet]), data, orc.FASTQ)["kmers"])
        _B_CASES[key] = (data, model)
    return _B_CASES[key]


def _assert_overlap(got, want, where=""):
    assert {w: got[w] for w in SM.WORDS} == {w: want[w] for w in SM.WORDS}, where
    for name in ("jaccard", "containment_a", "containment_b", "weighted_jaccard"):
        assert got[name] == want[name], (where, name)


def _insert_counts(model, base):
    """the model after the reads of `base` were built into it once more"""
    for key, c in base.d.items():
        model.d[key] = model._add(model.d.get(key, 0), c)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("k,alphabet,form", SHAPES)
def test_built_pairs(ctxs, k, alphabet, form, call):
    import kmerind_amd as K
    ctx = ctxs[form]
    a, ma, q = S.built_index(ctx, k, alphabet, "canonical")
    data_a = S.reads_case(k, alphabet, "canonical")[0]
    data_b, mb = _b_case(k, alphabet)
    # no op can pass degenerately
    shared = [key for key in ma.d if key in mb.d]
    assert shared and any(key not in mb.d for key in ma.d) and any(key not in ma.d for key in mb.d)
    assert any(ma.d[key] < mb.d[key] for key in shared) and any(ma.d[key] > mb.d[key] for key in shared)
    b = K.CountIndex(ctx, K.make_config(k, alphabet, strand="canonical"))
    S.build_device(ctx, b, data_b)
    qq = np.concatenate([q, mb.export()[0][::3]])
    if call == "compare":
        _assert_overlap(a.compare(b), SM.overlap(ma, mb))
        assert ctx.debug_counter(10) == 1
        _assert_overlap(b.compare(a), SM.overlap(mb, ma), "the other way round")
        assert M.state_difference(a, ma, qq) is None
    else:
        base = ma.copy()
        want = SM.combined(ma, mb, call)
        assert a.combine(b, call) == want.size() == a.local_size()
        assert ctx.debug_counter(10) == 1
        assert M.state_difference(a, want, qq) is None
        S.assert_spectrum(a.spectrum(4096), S.model_spectrum(want, 4096), "spectrum of the result")
        # the index goes on working: the same reads again, an erase
        S.build_device(ctx, a, data_a)
        _insert_counts(want, base)
        assert M.state_difference(a, want, qq) is None
        gone = want.export()[0][::7]
        assert a.erase(gone) == want.erase(gone) == gone.shape[0]
        assert M.state_difference(a, want, qq) is None
    assert M.state_difference(b, mb, qq) is None   # b's entries did not move
    a.close()
    b.close()


@pytest.mark.parametrize("call", ["compare", "union_add", "intersect_min", "subtract_counts"])
@pytest.mark.parametrize("a_from", ["fastq", "pairs"])
def test_layouts_crossed(ctxs, a_from, call):
    """one operand built from FASTQ on the device (minimizer layout, sparse under KMI_SPARSE_MIN=1), the other filled by
    insert_pairs (placement layout)"""
    import kmerind_amd as K
    ctx = ctxs["sparse"]
    k = 31
    built, m_built, q = S.built_index(ctx, k, "DNA", "canonical")
    m_pairs = _b_case(k, "DNA")[1].copy()
    filled = K.CountIndex(ctx, K.make_config(k, "DNA", strand="canonical"))
    pk, pc = m_pairs.export()
    filled.insert_pairs(pk, pc)
    a, ma, b, mb = (built, m_built, filled, m_pairs) if a_from == "fastq" else (filled, m_pairs, built, m_built)
    qq = np.concatenate([q, pk[::3]])
    if call == "compare":
        _assert_overlap(a.compare(b), SM.overlap(ma, mb))
        assert M.state_difference(a, ma, qq) is None
    else:
        want = SM.combined(ma, mb, call)
        assert a.combine(b, call) == want.size()
        assert M.state_difference(a, want, qq) is None
        _assert_overlap(a.compare(b), SM.overlap(want, mb), "the result against b")
    assert M.state_difference(b, mb, qq) is None
    a.close()
    b.close()


def _np_pairs(idx):
    gk, gc = idx.to_vector()
    order = np.argsort(gk[:, 0], kind="stable")
    return gk[order, 0], gc[order]


def test_several_passes():
    """KMI_LOOKUP_CAP=64 leaves a table 48 entries per pass; 3,000,000 unique keys are about 92 per fine bucket. The keys are
    unique, so numpy on the sorted key arrays is the model."""
    import kmerind_amd as K
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("KMI_LOOKUP_CAP", "64")
        ctx = K.Context(0)
    rng = np.random.default_rng(4242)
    pool = np.unique(rng.integers(0, 1 << 62, 4_600_000, dtype=np.uint64))[:4_500_000]
    pool = pool[rng.permutation(pool.size)]
    ka, kb = np.sort(pool[:3_000_000]), np.sort(pool[1_500_000:])
    ca = (np.uint64(1) + ka % np.uint64(9)).astype(np.uint32)
    cb = (np.uint64(1) + (kb >> np.uint64(7)) % np.uint64(9)).astype(np.uint32)
    cfg = K.make_config(31, "DNA", strand="single")
    b = K.CountIndex(ctx, cfg)
    b.insert_pairs(kb.reshape(-1, 1), cb)
    in_b = np.isin(ka, kb, assume_unique=True)
    cb_of_a = np.zeros(ka.size, dtype=np.uint32)
    cb_of_a[in_b] = cb[np.searchsorted(kb, ka[in_b])]
    assert int(in_b.sum()) == 1_500_000

    a = K.CountIndex(ctx, cfg)
    a.insert_pairs(ka.reshape(-1, 1), ca)
    got = a.compare(b)
    assert ctx.debug_counter(10) >= 2
    want = {"n_a": ka.size, "n_b": kb.size, "n_shared": int(in_b.sum()), "sum_a": int(ca.sum(dtype=np.uint64)), "sum_b": int(cb.sum(dtype=np.uint64)),
            "sum_a_shared": int(ca[in_b].sum(dtype=np.uint64)), "sum_b_shared": int(cb_of_a[in_b].sum(dtype=np.uint64)),
            "sum_min_shared": int(np.minimum(ca, cb_of_a)[in_b].sum(dtype=np.uint64))}
    assert {w: got[w] for w in SM.WORDS} == want

    assert a.combine(b, "subtract_counts") == int((ca > cb_of_a).sum())
    assert ctx.debug_counter(10) >= 2
    gk, gc = _np_pairs(a)
    keep = ca > cb_of_a
    assert (gk == ka[keep]).all() and (gc == (ca - cb_of_a)[keep]).all()
    a.close()

    a = K.CountIndex(ctx, cfg)
    a.insert_pairs(ka.reshape(-1, 1), ca)
    assert a.combine(b, "intersect_min") == int(in_b.sum())
    assert ctx.debug_counter(10) >= 2
    gk, gc = _np_pairs(a)
    assert (gk == ka[in_b]).all() and (gc == np.minimum(ca, cb_of_a)[in_b]).all()
    bk, bc = _np_pairs(b)
    assert (bk == kb).all() and (bc == cb).all()
    a.close()
    b.close()
    ctx.close()


def test_buckets_beyond_one_compaction_tile(ctxs):
    """10,000,000 unique keys are about 305 per fine bucket against the compaction's 256 threads; b holds every third of them.
    A union into an empty index makes the second copy of a on the device."""
    import kmerind_amd as K
    ctx = ctxs["dense"]
    rng = np.random.default_rng(1234)
    keys = np.unique(rng.integers(0, 1 << 62, 10_000_000, dtype=np.uint64))
    counts = (np.uint64(1) + keys % np.uint64(3)).astype(np.uint32)
    cfg = K.make_config(31, "DNA", strand="single")
    a = K.CountIndex(ctx, cfg)
    a.insert_pairs(keys.reshape(-1, 1), counts)
    b = K.CountIndex(ctx, cfg)
    b.insert_pairs(keys[::3].reshape(-1, 1), np.full(keys[::3].size, 2))
    a2 = K.CountIndex(ctx, cfg)
    assert a2.combine(a, "union_max") == keys.size
    in_b = np.zeros(keys.size, dtype=bool)
    in_b[::3] = True
    assert a.combine(b, "subtract_keys") == int((~in_b).sum())
    gk, gc = _np_pairs(a)
    assert (gk == keys[~in_b]).all() and (gc == counts[~in_b]).all()
    assert a2.combine(b, "intersect_left") == int(in_b.sum())
    gk, gc = _np_pairs(a2)
    assert (gk == keys[in_b]).all() and (gc == counts[in_b]).all()
    assert b.local_size() == int(in_b.sum())
    for i in (a, a2, b):
        i.close()


SENTINEL = 0xFFFFFFFFFFFFFFFF


def _filled(ctx, cfg, model, pairs, zeros=()):
    """an index and its model filled by insert_pairs; the keys in `zeros` are then set to 0 by update_pairs(assign)"""
    import kmerind_amd as K
    idx = K.CountIndex(ctx, cfg)
    keys = np.array(list(pairs), dtype=np.uint64).reshape(-1, 1)
    vals = np.array(list(pairs.values()), dtype=np.uint64)
    if keys.shape[0]:
        idx.insert_pairs(keys, vals)
        model.insert_pairs(keys, vals)
    if zeros:
        z = np.array(list(zeros), dtype=np.uint64).reshape(-1, 1)
        assert idx.update_pairs(z, np.zeros(z.shape[0]), op="assign") == model.update_pairs(z, np.zeros(z.shape[0]), "assign") == z.shape[0]
    return idx


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("sentinel_in", ["a", "b", "both"])
def test_sentinel_key_and_stored_zeros(ctxs, sentinel_in, call):
    """k = 32 single strand: the all-ones key is a k-mer (and the LDS table's empty marker). Key 7 is stored with count 0 in b and
    with 5 in a; key 8 with 0 in a and 3 in b; key 9 with 0 in a alone."""
    import kmerind_amd as K
    ctx = ctxs["dense"]
    cfg = K.make_config(32, "DNA", strand="single")
    pa = {1: 4, 2: 9, 7: 5, 8: 1, 9: 1, 100: 2}
    pb = {2: 3, 3: 6, 7: 1, 8: 3, 100: 8}
    if sentinel_in in ("a", "both"):
        pa[SENTINEL] = 11
    if sentinel_in in ("b", "both"):
        pb[SENTINEL] = 4
    ma, mb = M.CountModel(32, orc.DNA, orc.SINGLE), M.CountModel(32, orc.DNA, orc.SINGLE)
    a, b = _filled(ctx, cfg, ma, pa, zeros=(8, 9)), _filled(ctx, cfg, mb, pb, zeros=(7,))
    assert ma.d[(8,)] == 0 and ma.d[(9,)] == 0 and mb.d[(7,)] == 0
    q = np.array(sorted(set(pa) | set(pb) | {55}), dtype=np.uint64).reshape(-1, 1)
    if call == "compare":
        got = a.compare(b)
        _assert_overlap(got, SM.overlap(ma, mb))
        assert got["n_shared"] == 4 + (sentinel_in == "both")   # 2, 7, 8, 100: the stored zeros count as shared
    else:
        want = SM.combined(ma, mb, call)
        assert a.combine(b, call) == want.size()
        assert M.state_difference(a, want, q) is None
        got = {key[0]: c for key, c in zip(*[x.tolist() for x in a.to_vector()])}
        assert got == {key[0]: c for key, c in want.d.items()}
        if call == "subtract_keys":
            assert 7 not in got and 8 not in got and got[9] == 0 and ((SENTINEL in got) == (sentinel_in == "a"))
        if call == "subtract_counts":
            assert got[7] == 5 and 8 not in got and 9 not in got
            assert got.get(SENTINEL) == {"a": 11, "b": None, "both": 7}[sentinel_in]
        if call in ("intersect_min", "intersect_left", "intersect_add"):
            assert 7 in got and 8 in got and ((SENTINEL in got) == (sentinel_in == "both"))
        if call in ("union_add", "union_max"):
            assert got[SENTINEL] == {"a": 11, "b": 4, "both": 15 if call == "union_add" else 11}[sentinel_in] and got[9] == 0
    assert M.state_difference(b, mb, q) is None
    a.close()
    b.close()


@pytest.mark.parametrize("saturating", [False, True])
def test_reducers(ctxs, saturating):
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    ctx = ctxs["dense"]
    cfg = K.make_config(31, "DNA", strand="single")
    pa, pb = {5: 4_000_000_000, 6: 4_000_000_000, 7: 3}, {5: 1_000_000_000, 6: 4_000_000_000, 8: 4_000_000_000}
    for call in ("union_add", "intersect_add"):
        ma, mb = M.CountModel(31, orc.DNA, orc.SINGLE, saturating=saturating), M.CountModel(31, orc.DNA, orc.SINGLE)
        a, b = _filled(ctx, cfg, ma, pa), _filled(ctx, cfg, mb, pb)
        if saturating:
            ctx.check(L.lib.kmi_index_set_saturating(a.h, 1))
        got = a.compare(b)
        _assert_overlap(got, SM.overlap(ma, mb))
        assert got["sum_a"] == 8_000_000_003 and got["sum_b"] == 9_000_000_000 and got["sum_min_shared"] == 5_000_000_000   # never clamped
        want = SM.combined(ma, mb, call)
        assert a.combine(b, call) == want.size()
        got = {key[0]: c for key, c in zip(*[x.tolist() for x in a.to_vector()])}
        assert got == {key[0]: c for key, c in want.d.items()}
        assert got[5] == (4_294_967_295 if saturating else 705_032_704)
        assert got[6] == (4_294_967_295 if saturating else 3_705_032_704)
        a.close()
        b.close()


def _lookup_pair(a, b, q):
    return a.lookup(q).copy(), b.lookup(q).copy()


def test_edges(ctxs):
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    ctx = ctxs["sparse"]
    k = 31
    cfg = K.make_config(k, "DNA", strand="canonical")
    a, ma, q = S.built_index(ctx, k, "DNA", "canonical")

    def refused(fn):
        with pytest.raises(L.KmiError) as e:
            fn()
        assert e.value.status == L.ERR_INVALID

    # compare(a, a); the profile names
    ctx.profile(True)
    ctx.profile_reset()
    got = a.compare(a)
    names = {p["name"] for p in ctx.profile_get() if p["launches"]}
    assert got["n_shared"] == got["n_a"] == got["n_b"] == ma.size() and got["jaccard"] == 1.0 and got["sum_min_shared"] == got["sum_a"]
    assert "bucket_join" in names and "bucket_merge" not in names
    # one operand empty / never filled / both
    never = K.CountIndex(ctx, cfg)
    emptied = K.CountIndex(ctx, cfg)
    emptied.insert(np.arange(10, dtype=np.uint64).reshape(-1, 1))
    assert emptied.retain_counts(2) == 10
    none = M.CountModel(k, orc.DNA, orc.CANONICAL)
    for e, other in ((never, emptied), (emptied, never)):
        _assert_overlap(a.compare(e), SM.overlap(ma, none))
        _assert_overlap(e.compare(a), SM.overlap(none, ma))
        _assert_overlap(e.compare(other), SM.overlap(none, none))
        assert ctx.debug_counter(10) == 0
        for op in ("union_add", "union_max", "subtract_keys", "subtract_counts"):
            assert a.combine(e, op) == ma.size()
        for op in ("intersect_min", "intersect_add", "intersect_left", "subtract_keys", "subtract_counts"):
            assert e.combine(a, op) == 0 and e.local_size() == 0
        assert e.combine(other, "union_add") == 0 and e.combine(other, "intersect_min") == 0
    assert M.state_difference(a, ma, q) is None
    # a union into an empty index copies; an intersection with an empty one empties, and the index goes on working
    ctx.profile_reset()
    assert never.combine(a, "union_add") == ma.size()
    names = {p["name"] for p in ctx.profile_get() if p["launches"]}
    assert "bucket_merge" in names and "bucket_join" not in names
    assert M.state_difference(never, ma, q) is None
    ctx.profile_reset()
    assert never.combine(emptied, "intersect_left") == 0 and never.local_size() == 0
    names = {p["name"] for p in ctx.profile_get() if p["launches"]}
    assert "bucket_join" in names
    ctx.profile_reset()
    assert never.combine(a, "union_max") == ma.size() and never.combine(a, "subtract_keys") == 0
    names = {p["name"] for p in ctx.profile_get() if p["launches"]}
    ctx.profile(False)
    assert "bucket_join" in names and "bucket_merge" in names
    never.insert(np.arange(5, dtype=np.uint64).reshape(-1, 1))
    assert never.local_size() == 5
    # refusals: both indexes answer as before
    b = K.CountIndex(ctx, cfg)
    S.build_device(ctx, b, _b_case(k, "DNA")[0])
    mb = _b_case(k, "DNA")[1]
    before = _lookup_pair(a, b, q)
    refused(lambda: a.combine(a, "union_add"))
    refused(lambda: a.combine(b, 7))
    with pytest.raises(ValueError):
        a.combine(b, "xor")
    others = [K.CountIndex(ctx, K.make_config(29, "DNA", strand="canonical")), K.CountIndex(ctx, K.make_config(k, "DNA5", strand="canonical")),
              K.CountIndex(ctx, K.make_config(k, "DNA", strand="single")), K.PositionIndex(ctx, K.make_config(k, "DNA", index_kind="position"))]
    ctx2 = ctxs["dense"]
    others.append(K.CountIndex(ctx2, cfg))
    for o in others:
        refused(lambda: a.compare(o))
        refused(lambda: o.compare(a))
        refused(lambda: a.combine(o, "intersect_min"))
        refused(lambda: o.combine(a, "union_add"))
        assert o.local_size() == 0
    after = _lookup_pair(a, b, q)
    assert (before[0] == after[0]).all() and (before[1] == after[1]).all()
    assert M.state_difference(a, ma, q) is None and M.state_difference(b, mb, q) is None
    for i in others + [a, b, never, emptied]:
        i.close()
