"""CPU-side guards of what test_gpu_position_sequences.py rests on: the hot keys of tests/multimap_cases.py are distinct valid keys
of one placement bucket and outnumber every query table, and the oracle's multimap answers the hot and heavy inputs the way the
GPU tests expect -- within a time that lets them use it after every step."""
import time

import numpy as np
import pytest

from tests import multimap_cases as MC
from tests import oracle as orc
from tests.test_gpu_index import place_hash_np

SHAPES = sorted({(k, a) for k, a, _ in MC.PASS_SHAPES + MC.HEAVY_SHAPES})


def test_more_hot_query_keys_than_any_query_table_has_slots():
    assert MC.N_HOT_Q > max(MC.QUERY_CAP.values())
    assert MC.N_HOT >= MC.N_HOT_Q + 500                      # hot keys that are stored, share every pass and are not queried
    assert {orc.kspec(k, MC.ALPHA[a]).n_words for k, a, _ in MC.PASS_SHAPES} == {1, 2, 3}
    assert set(MC.QUERY_CAP) == {1, 2, 3, 4}
    assert MC.N_HEAVY > 100 * 512


@pytest.mark.parametrize("k,alpha", SHAPES)
def test_hot_keys_are_distinct_valid_keys_of_one_bucket(k, alpha):
    s = orc.kspec(k, MC.ALPHA[alpha])
    hot = MC.hot_keys(k, alpha, MC.N_HOT)
    assert hot.shape == (MC.N_HOT, s.n_words) and hot.dtype == np.uint64
    assert np.unique(hot, axis=0).shape[0] == MC.N_HOT
    pad = MC.pad_bits(s)
    if pad:
        assert (hot[:, -1] >> np.uint64(64 - pad) == 0).all()
    assert (place_hash_np(hot) >> np.uint64(17) == MC.BUCKET).all()
    other = MC.hot_keys(k, alpha, 100, bucket=32767)
    assert (place_hash_np(other) >> np.uint64(17) == 32767).all()
    if (k, alpha) == (32, "DNA"):
        assert not (hot[:, 0] == np.uint64(MC.EMPTY_MARKER)).any()
        assert orc.kmers_from_string(s, b"T" * 32).tolist() == [[MC.EMPTY_MARKER]]
        assert orc.canonical(s, np.array([[MC.EMPTY_MARKER]], dtype=np.uint64)).tolist() == [[0]]


def test_read_sets_repeat_keys_and_hold_short_reads():
    rng = np.random.default_rng(1)
    seqs = MC.reads(rng, 200, 31)
    assert min(map(len, seqs)) < 31 and max(map(len, seqs)) <= 150
    s = orc.kspec(31)
    for vw in (1, 2):
        kmers, vals = MC.tuples_of(s, MC.fastq(rng, seqs), vw)
        assert vals.shape == (kmers.shape[0], vw) and np.unique(vals[:, 0]).size == kmers.shape[0]
        assert np.unique(orc.canonical(s, kmers), axis=0).shape[0] < kmers.shape[0] // 2     # keys repeat across reads
        if vw == 2:
            assert (vals[:, 1] >> np.uint64(32) == 0).all() and np.unique(vals[:, 1]).size > 100
    fk, fv = MC.tuples_of(s, MC.fasta(seqs), 1, fmt=orc.FASTA)
    assert fk.shape[0] == kmers.shape[0]
    s32 = orc.kspec(32)
    pk, _ = MC.tuples_of(s32, MC.poly_fastq(rng, 32), 2)
    assert int((pk[:, 0] == np.uint64(MC.EMPTY_MARKER)).sum()) == 40 * (150 - 32 + 1)


def test_oracle_steps_on_the_hot_and_heavy_inputs():
    """count: one row per distinct query key, the heavy key's is n; erase returns the tuples removed and the export holds none of
    the erased keys afterwards. All shapes and value widths together in under 2 s: cheap enough to run after every GPU step."""
    spent = [0.0]

    def timed(fn, *args):
        t0 = time.perf_counter()
        out = fn(*args)
        spent[0] += time.perf_counter() - t0
        return out
    for k, alpha in SHAPES:
        s = orc.kspec(k, MC.ALPHA[alpha])
        for vw in (1, 2):
            rng = np.random.default_rng(k + vw)
            hot = MC.hot_keys(k, alpha, MC.N_HOT)
            kmers, vals = MC.hot_tuples(rng, hot, vw, s)
            heavy = hot[:1] if k != 32 else np.array([[MC.EMPTY_MARKER]], dtype=np.uint64)
            hk, hv = MC.heavy_tuples(heavy, vw=vw)
            assert np.unique(np.concatenate([vals[:, 0], hv[:, 0]])).size == kmers.shape[0] + MC.N_HEAVY
            om = orc.MultiMap(s, orc.SINGLE, vw=vw)
            timed(om.insert, kmers, vals)
            timed(om.insert, hk, hv)
            assert om.size() == kmers.shape[0] + MC.N_HEAVY
            q = np.concatenate([MC.pass_queries(rng, hot, s), heavy])
            n_distinct = np.unique(q, axis=0).shape[0]
            ck, cc = timed(om.count, q)
            assert ck.shape[0] == n_distinct and np.unique(ck, axis=0).shape[0] == n_distinct
            row = (ck == heavy).all(axis=1)
            n_heavy = MC.N_HEAVY + int((kmers == heavy).all(axis=1).sum())
            assert int(row.sum()) == 1 and int(cc[row][0]) == n_heavy
            assert int((cc == 0).sum()) >= 990                                # the absent keys
            fk, fv = timed(om.find, q)
            assert fk.shape[0] == int(cc.sum()) and fv.shape == (fk.shape[0], vw)
            before = om.size()
            n = timed(om.erase, q)
            assert n == int(cc.sum()) and om.size() == before - n
            ek, ev = timed(om.export)
            gone = {tuple(r) for r in q.tolist()}
            assert not any(tuple(r) in gone for r in ek.tolist())
            assert timed(om.erase, q) == 0 and timed(om.find, q)[0].shape[0] == 0
    print("oracle steps: %.2f s" % spent[0])
    assert spent[0] < 2.0
