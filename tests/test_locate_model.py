"""tests/locate_model.py on hand-written cases: what the GPU tests of kmi_index_locate_* / kmi_index_seed_reads_* compare against."""
import numpy as np

from tests import index_model as M
from tests import locate_model as LM
from tests import oracle as orc

K = 5
S = orc.kspec(K, orc.DNA)


def km(text):
    return orc.kmers_from_string(S, text)


def test_duplicate_query_and_cap():
    m = LM.LocateModel(S, orc.SINGLE)
    # ACGTA three times (values 10, 11, 12), CGTAC once (20), GGGGG twice (30, 31)
    m.insert(np.concatenate([km(b"ACGTA")] * 3 + [km(b"CGTAC")] + [km(b"GGGGG")] * 2), [10, 11, 12, 20, 30, 31])
    assert m.size() == 6 and m.multiplicities().tolist() == [1, 2, 3]
    q = np.concatenate([km(b"ACGTA"), km(b"TTTTT"), km(b"GGGGG"), km(b"ACGTA"), km(b"CGTAC")])
    occ, off, per = m.locate(q)
    assert occ.tolist() == [3, 0, 2, 3, 1]
    assert off.tolist() == [0, 3, 3, 5, 8, 9]
    assert per == [[(10,), (11,), (12,)], [], [(30,), (31,)], [(10,), (11,), (12,)], [(20,)]]   # a key asked twice is answered twice
    # max_occ at occ: listed
    occ3, off3, per3 = m.locate(q, max_occ=3)
    assert occ3.tolist() == occ.tolist() and off3.tolist() == off.tolist() and per3 == per
    # max_occ at occ - 1: the key is not listed at all, occ stays the true multiplicity
    occ2, off2, per2 = m.locate(q, max_occ=2)
    assert occ2.tolist() == [3, 0, 2, 3, 1]
    assert off2.tolist() == [0, 0, 0, 2, 2, 3]
    assert per2 == [[], [], [(30,), (31,)], [], [(20,)]]
    occ1, off1, per1 = m.locate(q, max_occ=1)
    assert off1.tolist() == [0, 0, 0, 0, 0, 1] and per1 == [[], [], [], [], [(20,)]]
    # no queries
    occ0, off0, per0 = m.locate(np.zeros((0, 1), dtype=np.uint64))
    assert occ0.shape == (0,) and off0.tolist() == [0] and per0 == []


def test_both_strands():
    single, canon = LM.LocateModel(S, orc.SINGLE), LM.LocateModel(S, orc.CANONICAL)
    fwd, rev = km(b"AACCG"), km(b"CGGTT")          # reverse complements of each other
    assert (orc.revcomp(S, fwd) == rev).all()
    for m in (single, canon):
        m.insert(np.concatenate([fwd, rev, fwd]), [1, 2, 3])
    q = np.concatenate([fwd, rev])
    assert single.locate(q)[0].tolist() == [2, 1] and single.locate(q)[2] == [[(1,), (3,)], [(2,)]]
    occ, off, per = canon.locate(q)                # one key under the canonical model, whichever strand asks
    assert occ.tolist() == [3, 3] and off.tolist() == [0, 3, 6] and per == [[(1,), (2,), (3,)]] * 2


def test_two_value_words_sort_as_rows():
    m = LM.LocateModel(S, orc.SINGLE, vw=2)
    m.insert(np.concatenate([km(b"ACGTA")] * 2), [[7, 1], [5, 9]])
    assert m.locate(km(b"ACGTA"))[2] == [[(5, 9), (7, 1)]]
    assert LM.values_difference(np.array([[7, 1], [5, 9]], dtype=np.uint64), np.array([0, 2], dtype=np.uint64), [[(5, 9), (7, 1)]]) is None
    assert LM.values_difference(np.array([[7, 1], [5, 8]], dtype=np.uint64), np.array([0, 2], dtype=np.uint64), [[(5, 9), (7, 1)]]) is not None
    assert LM.values_difference(np.zeros((1, 2), dtype=np.uint64), np.array([0, 2], dtype=np.uint64), [[(5, 9), (7, 1)]]) is not None


def test_seed_reads_rows():
    ref = b"AACCGGATCTC"                            # windows: AACCG ACCGG CCGGA CGGAT GGATC GATCT ATCTC, no two of them one key
    m = LM.LocateModel(S, orc.CANONICAL)
    m.build(M.fasta([ref]), orc.FASTA)
    assert m.size() == 7 and m.multiplicities().tolist() == [1] * 7
    reads = [b"ACCGGAT",                            # three windows of the reference
             b"ACG",                                # shorter than k: a row without windows
             M.revcomp_text(b"GGATCTC"),            # the other strand: three windows
             b"TTTTTTT",                            # three windows, none in the index
             b"AACCGAACCG"]                         # AACCG ACCGA CCGAA CGAAC GAACC AACCG: the first and the last are the same key
    data = M.fastq(reads)
    rows, occ, off, per = m.seed_reads(data)
    assert rows["n_kmers"].tolist() == [3, 0, 3, 3, 6]
    assert rows["first_kmer"].tolist() == [0, 3, 3, 6, 9]
    assert rows["n_listed"].tolist() == [3, 0, 3, 0, 2]
    assert rows["n_hits"].tolist() == [3, 0, 3, 0, 2]
    assert occ.tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    assert off.tolist() == list(np.cumsum([0] + occ.tolist()))
    assert per[9] == per[14] and len(per[9]) == 1
    recs = orc.records(data, orc.FASTQ)
    assert rows["seq_offset"].tolist() == [r.seq_begin for r in recs]
    for r, row in zip(reads, rows):
        assert data[int(row["seq_offset"]):int(row["seq_offset"]) + len(r)] == r
    # a second copy of the reference: every stored key twice; max_occ = 1 then lists nothing, occ keeps the multiplicity
    m.build(M.fasta([ref]), orc.FASTA)
    rows2, occ2, off2, per2 = m.seed_reads(data, max_occ=1)
    assert occ2.tolist() == [2 * c for c in occ.tolist()]
    assert not off2.any() and not rows2["n_listed"].any() and not rows2["n_hits"].any() and all(p == [] for p in per2)
    assert rows2["first_kmer"].tolist() == rows["first_kmer"].tolist() and rows2["n_kmers"].tolist() == rows["n_kmers"].tolist()
    rows3 = m.seed_reads(data, max_occ=2)[0]
    assert rows3["n_hits"].tolist() == [6, 0, 6, 0, 4] and rows3["n_listed"].tolist() == [3, 0, 3, 0, 2]


def test_difference_reports():
    want = (np.array([1, 0], dtype=np.uint32), np.array([0, 1, 1], dtype=np.uint64), [[(4,)], []])
    good = (want[0].copy(), want[1].copy(), np.array([[4]], dtype=np.uint64))
    assert LM.difference(good, want) is None
    assert "occ[1]" in LM.difference((np.array([1, 2], dtype=np.uint32), good[1], good[2]), want)
    assert "offsets[2]" in LM.difference((good[0], np.array([0, 1, 2], dtype=np.uint64), good[2]), want)
    assert "query 0" in LM.difference((good[0], good[1], np.array([[5]], dtype=np.uint64)), want)
