"""kmi_index_retain_counts: keep lo <= count <= hi on the device, against tests/index_model.CountModel with the out-of-range keys
erased -- the built indexes of test_gpu_spectrum.py (both layouts, dense and sparse, one to two words, 2- and 3-bit alphabets),
buckets of more entries than one tile of the compaction, bucket shapes chosen on purpose, and the edges. After every filter the
index is used further: built into again, erased from, looked up, exported."""
import numpy as np
import pytest

from tests import index_model as M
from tests import read_profile_model as RP
from tests import spectrum_cases as S

pytestmark = pytest.mark.gpu
U32 = 2**32 - 1
RANGES = {"from2": (2, U32), "singletons": (1, 1), "middle": (3, 3000), "all": (0, U32), "none": (4_000_000_000, U32)}


@pytest.fixture(scope="module")
def ctxs():
    out = S.make_contexts()
    yield out
    for c in out.values():
        c.close()


def _filtered(model, lo, hi):
    m = model.copy()
    m.d = {key: c for key, c in model.d.items() if lo <= c <= hi}
    return m


def _insert_counts(model, base):
    """the model after the reads of `base` were built into it once more"""
    for key, c in base.d.items():
        model.d[key] = model._add(model.d.get(key, 0), c)


@pytest.mark.parametrize("which", sorted(RANGES))
@pytest.mark.parametrize("k,alphabet,form", [(17, "DNA", "dense"), (17, "DNA", "sparse"), (31, "DNA", "dense"), (31, "DNA", "sparse"),
                                               (32, "DNA", "dense"), (32, "DNA", "sparse"), (63, "DNA", "dense"), (21, "DNA5", "dense")])
def test_retain_counts_of_built_indexes(ctxs, k, alphabet, form, which):
    ctx = ctxs[form]
    lo, hi = RANGES[which]
    idx, base, q = S.built_index(ctx, k, alphabet, "canonical")
    data = S.reads_case(k, alphabet, "canonical")[0]
    want = _filtered(base, lo, hi)
    assert (want.size() == base.size()) == (which == "all") and (want.size() == 0) == (which == "none")
    ctx.profile(True)
    ctx.profile_reset()
    n_erased = idx.retain_counts(lo, hi)
    names = {p["name"] for p in ctx.profile_get() if p["launches"]}
    ctx.profile(False)
    assert "bucket_retain_count" in names and ("bucket_retain_compact" in names) == (which not in ("all", "none"))
    assert n_erased == base.size() - want.size()
    assert ctx.debug_counter(9) >= 1
    assert (idx.lookup(q) == RP.lookup(want, q)).all()
    hist, totals = idx.spectrum(4096)
    S.assert_spectrum((hist, totals), S.model_spectrum(want, 4096), "spectrum of the result")
    assert not hist[:min(lo, 4095)].any() and (hi >= 4095 or not hist[hi + 1:].any())
    assert M.state_difference(idx, want, q) is None
    if which == "none":
        assert idx.local_size() == 0 and idx.count(q)[1].sum() == 0 and idx.find(q)[0].shape[0] == 0
        assert idx.retain_counts(1) == 0   # nothing to filter
    # the index goes on working: the same reads again (survivors add up, erased keys come back with their fresh count), an erase
    S.build_device(ctx, idx, data)
    _insert_counts(want, base)
    assert want.size() == base.size()
    assert M.state_difference(idx, want, q) is None
    gone = want.export()[0][::7]
    assert idx.erase(gone) == want.erase(gone) == gone.shape[0]
    assert M.state_difference(idx, want, q) is None
    S.assert_spectrum(idx.spectrum(64), S.model_spectrum(want, 64), "spectrum after build and erase")
    idx.close()


def test_buckets_beyond_one_tile(ctxs):
    """bucket_retain_compact_kernel's tile is 256 entries (one per thread). 10,000,000 unique keys are about 305 per fine bucket, so
    every bucket takes two tiles and the second starts behind the first one's survivors; count = 1 + key % 3 alternates survivors
    and losers inside every bucket. The keys are unique, so numpy on (keys, counts) is the model."""
    import kmerind_amd as K
    ctx = ctxs["dense"]
    rng = np.random.default_rng(1234)
    keys = np.unique(rng.integers(0, 1 << 62, 10_000_000, dtype=np.uint64))
    counts = (np.uint64(1) + keys % np.uint64(3)).astype(np.uint32)
    idx = K.CountIndex(ctx, K.make_config(31, "DNA", strand="single"))
    idx.insert_pairs(keys.reshape(-1, 1), counts)
    keep = counts == 2
    assert idx.retain_counts(2, 2) == int((~keep).sum())
    fullest = ctx.debug_counter(9)
    print("fullest bucket:", fullest)
    assert fullest > 256
    gk, gc = idx.to_vector()
    assert gk.shape[0] == int(keep.sum()) == idx.local_size()
    assert (gc == 2).all() and (np.sort(gk[:, 0]) == keys[keep]).all()
    sel = keys[rng.integers(0, keys.size, 100_000)]
    assert (idx.lookup(sel.reshape(-1, 1)) == np.where(sel % np.uint64(3) == 1, 2, 0)).all()
    idx.close()


@pytest.mark.parametrize("mirror", [False, True])
def test_bucket_shapes_on_purpose(ctxs, mirror):
    """to_vector() gives the stored (bucket) order. Losers: the first and the last entry of the array and a run of 2,000 consecutive
    entries (several whole buckets lose everything, their neighbours a head or a tail) -- or, mirrored, only that run survives."""
    import kmerind_amd as K
    ctx = ctxs["dense"]
    rng = np.random.default_rng(555)
    keys = np.unique(rng.integers(0, 1 << 62, 200_000, dtype=np.uint64)).reshape(-1, 1)
    idx = K.CountIndex(ctx, K.make_config(31, "DNA", strand="single"))
    idx.insert_pairs(keys, np.full(keys.shape[0], 5))
    stored = idx.to_vector()[0]
    n = stored.shape[0]
    marked = np.zeros(n, dtype=bool)
    marked[0] = marked[n - 1] = True
    marked[70_001:72_001] = True
    outside = ~marked if mirror else marked
    assert idx.update_pairs(stored[outside], np.full(int(outside.sum()), 1), op="assign") == int(outside.sum())
    k2, c2 = idx.to_vector()
    assert (k2 == stored).all() and (c2 == np.where(outside, 1, 5)).all()   # (the update left the order alone: the shapes are as meant)
    assert idx.retain_counts(2) == int(outside.sum())
    gk, gc = idx.to_vector()
    assert (gc == 5).all() and gk.shape == stored[~outside].shape and (gk == stored[~outside]).all()   # stable: the old order
    assert (idx.lookup(stored) == np.where(outside, 0, 5)).all()
    idx.close()


def test_retain_counts_edge_cases(ctxs):
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    ctx = ctxs["sparse"]
    idx, model, q = S.built_index(ctx, 31, "DNA", "canonical")
    with pytest.raises(L.KmiError) as e:
        idx.retain_counts(3, 2)
    assert e.value.status == L.ERR_INVALID
    assert (idx.lookup(q) == RP.lookup(model, q)).all()
    assert M.state_difference(idx, model, q) is None
    idx.close()
    empty = K.CountIndex(ctx, K.make_config(31, "DNA"))
    assert empty.retain_counts(2) == 0 and empty.local_size() == 0
    empty.insert(np.arange(10, dtype=np.uint64).reshape(-1, 1))
    assert empty.retain_counts(2) == 10 and empty.local_size() == 0
    empty.insert(np.arange(5, dtype=np.uint64).reshape(-1, 1))
    assert empty.local_size() == 5
    empty.close()
    pos = K.PositionIndex(ctx, K.make_config(21, "DNA", index_kind="position"))
    with pytest.raises(L.KmiError) as e:
        pos.retain_counts(2)
    assert e.value.status == L.ERR_INVALID
    pos.close()
