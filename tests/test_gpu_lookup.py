"""kmi_index_lookup_*: the count of every query, in query order, against tests/read_profile_model.py -- every k-mer shape a count
index takes, both layouts (a device build of one-word DNA k-mers leaves the minimizer layout), dense and sparse, duplicates, both
strands, absent keys, the key that equals the table's empty marker, and buckets that need several passes."""
import numpy as np
import pytest

from tests import index_model as M
from tests import oracle as orc
from tests import read_profile_model as RP

pytestmark = pytest.mark.gpu

STRAND = {"single": orc.SINGLE, "canonical": orc.CANONICAL}
ALPHA = {"DNA": orc.DNA, "DNA5": orc.DNA5, "DNA16": orc.DNA16}


@pytest.fixture(scope="module")
def ctxs():
    """dense: the default; sparse: KMI_SPARSE_MIN=1 leaves every super-k-mer build sparse; small: a lookup table of 64 home slots"""
    import kmerind_amd as K
    out = {}
    for name, env in (("dense", {}), ("sparse", {"KMI_SPARSE_MIN": "1"}), ("small", {"KMI_LOOKUP_CAP": "64"})):
        with pytest.MonkeyPatch.context() as mp:
            for key, v in env.items():
                mp.setenv(key, v)
            out[name] = K.Context(0)
    yield out
    for c in out.values():
        c.close()


def _build_device(ctx, idx, data):
    buf = np.frombuffer(data, dtype=np.uint8)
    d = ctx.alloc(buf.size + 64)
    try:
        ctx.to_device(d, buf)
        idx.build_device(d, buf.size)
    finally:
        ctx.free(d)


def _lookup_device(ctx, idx, q):
    q = np.ascontiguousarray(q, dtype=np.uint64)
    n = q.shape[0]
    dq, dc = ctx.alloc(max(q.nbytes, 8)), ctx.alloc(4 * max(n, 1))
    try:
        ctx.to_device(dq, q)
        idx.lookup_device(dq, n, dc)
        out = np.zeros(n, dtype=np.uint32)
        ctx.to_host(out, dc)
        return out
    finally:
        ctx.free(dq)
        ctx.free(dc)


def _probes(s, alphabet, stored, rng):
    if alphabet == "DNA":
        return M.probes(s, stored, rng)
    # (M.probes' one-base variants flip 2-bit codes: the other alphabets get the rest of its query set)
    pick = stored[rng.integers(0, stored.shape[0], min(1500, stored.shape[0]))]
    return np.concatenate([pick, orc.revcomp(s, pick[: pick.shape[0] // 2]), orc.kmers_from_string(s, M.random_seq(rng, 300 + s.k - 1)),
                           orc.kmers_from_string(s, b"A" * s.k), orc.kmers_from_string(s, b"T" * s.k)])


def _case(ctx, k, alphabet, strand, seed, extra_reads=()):
    """(index built on the device, model, shuffled probes with every probe twice)"""
    import kmerind_amd as K
    rng = np.random.default_rng(seed)
    s = orc.kspec(k, ALPHA[alphabet])
    data = M.fastq(M.adversarial_reads(rng, k) + M.background(rng, 300) + list(extra_reads))
    model = M.CountModel(k, ALPHA[alphabet], STRAND[strand])
    model.insert(orc.extract(s, data, orc.FASTQ)["kmers"])
    idx = K.CountIndex(ctx, K.make_config(k, alphabet, strand=strand))
    _build_device(ctx, idx, data)
    q = _probes(s, alphabet, model.export()[0], rng)
    q = np.concatenate([q, q])
    return idx, model, q[rng.permutation(q.shape[0])]


def _assert_equal(got, want, where):
    assert got.dtype == np.uint32 and got.shape == want.shape, where
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d of %d differ; first at query %d: got %d, expected %d" % (where, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("form", ["dense", "sparse"])
@pytest.mark.parametrize("strand", ["single", "canonical"])
@pytest.mark.parametrize("k", [17, 21, 28, 31, 32])
def test_lookup_matches_the_model(ctxs, k, strand, form):
    ctx = ctxs[form]
    # (the k = 32 single-strand all-T key is all ones: the table's empty marker)
    extra = M.poly_reads(b"T", 3) if (k == 32 and strand == "single") else ()
    idx, model, q = _case(ctx, k, "DNA", strand, 500 + k, extra)
    want = RP.lookup(model, q)
    assert (want > 0).any() and (want == 0).any()
    if k == 32 and strand == "single":
        assert want[(q == np.uint64(0xFFFFFFFFFFFFFFFF)).all(axis=1)].min() >= 3 * 119
    ctx.profile(True)
    ctx.profile_reset()
    _assert_equal(_lookup_device(ctx, idx, q), want, "k=%d %s %s device" % (k, strand, form))
    assert any(p["name"] == "bucket_lookup" and p["launches"] for p in ctx.profile_get())
    ctx.profile(False)
    _assert_equal(idx.lookup(q), want, "k=%d %s %s host" % (k, strand, form))
    idx.close()


@pytest.mark.parametrize("k,alphabet", [(15, "DNA"), (33, "DNA"), (63, "DNA"), (21, "DNA5"), (16, "DNA16")])
def test_lookup_off_the_superkmer_path(ctxs, k, alphabet):
    idx, model, q = _case(ctxs["dense"], k, alphabet, "canonical", 600 + k)
    want = RP.lookup(model, q)
    assert (want > 0).any() and (want == 0).any()
    _assert_equal(idx.lookup(q), want, "k=%d %s" % (k, alphabet))
    _assert_equal(_lookup_device(ctxs["dense"], idx, q), want, "k=%d %s device" % (k, alphabet))
    idx.close()


def test_buckets_larger_than_the_table_take_several_passes(ctxs):
    """3e6 random keys are about 92 per bucket; 64 home slots hold 48 a pass"""
    import kmerind_amd as K
    rng = np.random.default_rng(77)
    keys = np.unique(rng.integers(0, 1 << 62, 3_000_000, dtype=np.uint64))
    counts = (keys % np.uint64(7) + np.uint64(1)).astype(np.uint32)
    stored = keys[rng.integers(0, keys.size, 300_000)]
    absent = rng.integers(0, 1 << 62, 50_000, dtype=np.uint64)
    q = np.concatenate([stored, absent])
    q = q[rng.permutation(q.size)]
    want = np.where(np.isin(q, keys), q % np.uint64(7) + np.uint64(1), np.uint64(0)).astype(np.uint32)
    got = {}
    for name in ("small", "dense"):
        ctx = ctxs[name]
        idx = K.CountIndex(ctx, K.make_config(31, "DNA", strand="single"))
        idx.insert_pairs(keys.reshape(-1, 1), counts)
        got[name] = idx.lookup(q.reshape(-1, 1))
        _assert_equal(got[name], want, name)
        if name == "small":
            assert ctx.debug_counter(8) >= 2
        else:
            assert ctx.debug_counter(8) == 1
        idx.close()
    assert (got["small"] == got["dense"]).all()


def test_lookup_edge_cases(ctxs):
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    ctx = ctxs["sparse"]
    empty = K.CountIndex(ctx, K.make_config(31, "DNA"))
    q = np.arange(1000, dtype=np.uint64).reshape(-1, 1)
    assert (empty.lookup(q) == 0).all() and empty.lookup(q).shape == (1000,)
    assert empty.lookup(q[:0]).shape == (0,)
    empty.close()
    idx, model, q = _case(ctx, 31, "DNA", "canonical", 901)
    assert idx.lookup(q[:0]).shape == (0,)
    idx.lookup_device(0, 0, 0)   # nq = 0: no buffer is touched
    want = RP.lookup(model, q)
    _assert_equal(idx.lookup(q), want, "sparse, before to_vector")
    before = idx.to_vector()
    _assert_equal(idx.lookup(q), want, "dense, after to_vector")
    after = idx.to_vector()
    assert (before[0] == after[0]).all() and (before[1] == after[1]).all()
    assert M.first_difference(*after, *model.export()) is None
    idx.close()
    pos = K.PositionIndex(ctx, K.make_config(21, "DNA", index_kind="position"))
    with pytest.raises(L.KmiError) as e:
        pos.lookup(q[:4])
    assert e.value.status == L.ERR_INVALID
    with pytest.raises(L.KmiError) as e:
        pos.profile_reads(b"@a\nACGT\n+\nIIII\n")
    assert e.value.status == L.ERR_INVALID
    pos.close()
