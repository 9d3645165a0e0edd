"""kmi_index_spectrum_*: hist[min(count, n_bins - 1)] per stored entry and the totals, against numpy on tests/index_model.CountModel
-- every k-mer shape a count index takes, both layouts, dense and sparse (whose leftover slots must not be counted), every bin
boundary (the hot bins, the LDS-resident prefix, the clamp), one hot bin, and the edges."""
import numpy as np
import pytest

from tests import index_model as M
from tests import read_profile_model as RP
from tests import spectrum_cases as S

pytestmark = pytest.mark.gpu
N_BINS = (2, 3, 64, 257, 4096)


@pytest.fixture(scope="module")
def ctxs():
    out = S.make_contexts()
    yield out
    for c in out.values():
        c.close()


def _check_built(ctx, k, alphabet, strand, form):
    idx, model, q = S.built_index(ctx, k, alphabet, strand)
    where = "k=%d %s %s %s" % (k, alphabet, strand, form)
    counts = model.export()[1]
    assert counts.max() >= 3000 and (counts == 1).any()   # the crowded read's k-mers, and singletons
    ctx.profile(True)
    ctx.profile_reset()
    for n_bins in N_BINS:
        want = S.model_spectrum(model, n_bins)
        got = S.spectrum_device(ctx, idx, n_bins)
        print(where, n_bins, "device", got[1], got[0][:8])
        S.assert_spectrum(got, want, where + " n_bins=%d device" % n_bins)
        assert int(got[0].sum()) == idx.local_size() == model.size()
    assert any(p["name"] == "count_spectrum" and p["launches"] == len(N_BINS) for p in ctx.profile_get())
    ctx.profile(False)
    for n_bins in N_BINS:
        S.assert_spectrum(idx.spectrum(n_bins), S.model_spectrum(model, n_bins), where + " n_bins=%d host" % n_bins)
    if form == "sparse":   # the index has not been made dense on the way
        got, want = idx.lookup(q), RP.lookup(model, q)
        assert (got == want).all(), where + ": lookup after spectrum"
    assert M.state_difference(idx, model, q) is None
    S.assert_spectrum(idx.spectrum(64), S.model_spectrum(model, 64), where + " after to_vector")
    idx.close()


@pytest.mark.parametrize("form", ["dense", "sparse"])
@pytest.mark.parametrize("strand", ["single", "canonical"])
@pytest.mark.parametrize("k", [17, 21, 28, 31, 32])
def test_spectrum_of_built_indexes(ctxs, k, strand, form):
    _check_built(ctxs[form], k, "DNA", strand, form)


@pytest.mark.parametrize("k,alphabet", [(15, "DNA"), (33, "DNA"), (63, "DNA"), (21, "DNA5"), (16, "DNA16")])
def test_spectrum_off_the_superkmer_path(ctxs, k, alphabet):
    _check_built(ctxs["dense"], k, alphabet, "canonical", "dense")


def test_every_bin_boundary(ctxs):
    """3,000,000 unique keys with counts[i] = i % 70001: every count 0 .. 70000 about 43 times, so the register-counted bins, the
    LDS-resident prefix and the clamp are all straddled; three keys of 2^32 - 1 make sum_counts need its 64 bits. The keys are
    unique and go in as pairs, so the stored map is (keys, counts) itself: numpy on those arrays is the model."""
    import kmerind_amd as K
    ctx = ctxs["dense"]
    rng = np.random.default_rng(4242)
    keys = np.unique(rng.integers(0, 1 << 62, 3_000_500, dtype=np.uint64))[:3_000_003]
    keys = keys[rng.permutation(keys.size)]
    counts = (np.arange(keys.size, dtype=np.uint64) % np.uint64(70001)).astype(np.uint32)
    counts[-3:] = 0xFFFFFFFF
    idx = K.CountIndex(ctx, K.make_config(31, "DNA", strand="single"))
    idx.insert_pairs(keys.reshape(-1, 1), counts)
    assert idx.local_size() == keys.size
    for n_bins in (2, 65, 1024, 65536):
        want = S.spectrum_of_counts(counts, n_bins)
        assert want[1]["sum_counts"] == int(counts.astype(object).sum()) > 1 << 36
        S.assert_spectrum(S.spectrum_device(ctx, idx, n_bins), want, "n_bins=%d device" % n_bins)
        S.assert_spectrum(idx.spectrum(n_bins), want, "n_bins=%d host" % n_bins)
    # one more stored 0
    at = int(np.nonzero(counts == 7)[0][0])
    assert idx.update_pairs(keys[at:at + 1].reshape(-1, 1), [0], op="assign") == 1
    counts[at] = 0
    S.assert_spectrum(idx.spectrum(1024), S.spectrum_of_counts(counts, 1024), "after assign 0")
    idx.close()


def test_a_stored_zero_is_counted_in_bin_zero(ctxs):
    import kmerind_amd as K
    ctx = ctxs["dense"]
    keys = (np.arange(1000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(2)).reshape(-1, 1)
    idx = K.CountIndex(ctx, K.make_config(31, "DNA", strand="single"))
    idx.insert_pairs(keys, np.full(1000, 5))
    assert idx.spectrum(16)[0][0] == 0
    assert idx.update_pairs(keys[17:18], [0], op="assign") == 1
    hist, totals = idx.spectrum(16)
    assert hist[0] == 1 and hist[5] == 999 and hist.sum() == 1000
    assert totals == {"n_entries": 1000, "sum_counts": 999 * 5, "min_count": 0, "max_count": 5}
    idx.close()


def test_one_hot_bin(ctxs):
    import kmerind_amd as K
    ctx = ctxs["dense"]
    rng = np.random.default_rng(99)
    keys = np.unique(rng.integers(0, 1 << 62, 2_000_300, dtype=np.uint64))[:2_000_000].reshape(-1, 1)
    n = keys.shape[0]
    for count, n_bins, hot in ((1, 256, 1), (5, 4, 3)):
        idx = K.CountIndex(ctx, K.make_config(31, "DNA", strand="single"))
        idx.insert_pairs(keys, np.full(n, count))
        for hist, totals in (S.spectrum_device(ctx, idx, n_bins), idx.spectrum(n_bins)):
            assert hist[hot] == n and hist.sum() == n
            assert totals == {"n_entries": n, "sum_counts": n * count, "min_count": count, "max_count": count}
        idx.close()


def test_spectrum_edge_cases(ctxs):
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    ctx = ctxs["sparse"]
    empty = K.CountIndex(ctx, K.make_config(31, "DNA"))
    zero = {"n_entries": 0, "sum_counts": 0, "min_count": 0, "max_count": 0}
    for got in (empty.spectrum(64), S.spectrum_device(ctx, empty, 64)):   # (both overwrite a buffer of ones)
        assert (got[0] == 0).all() and got[0].shape == (64,) and got[1] == zero
    for bad in (0, 1, 65537):
        with pytest.raises(L.KmiError) as e:
            empty.spectrum(bad)
        assert e.value.status == L.ERR_INVALID
    hist, totals = empty.spectrum(65536)
    assert hist.shape == (65536,) and not hist.any()
    # filled, emptied again: arrays exist, no entry does
    empty.insert(np.arange(10, dtype=np.uint64).reshape(-1, 1))
    assert empty.spectrum(4)[0].tolist() == [0, 10, 0, 0]
    empty.erase(np.arange(10, dtype=np.uint64).reshape(-1, 1))
    assert empty.local_size() == 0 and not empty.spectrum(4)[0].any() and empty.spectrum(4)[1] == zero
    empty.close()
    pos = K.PositionIndex(ctx, K.make_config(21, "DNA", index_kind="position"))
    with pytest.raises(L.KmiError) as e:
        pos.spectrum(16)
    assert e.value.status == L.ERR_INVALID
    with pytest.raises(L.KmiError) as e:
        pos.retain_counts(2)
    assert e.value.status == L.ERR_INVALID
    pos.close()
