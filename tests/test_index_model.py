"""The reference model of tests/index_model.py against the oracle (CPU): what the operation-sequence GPU tests expect is only as
good as this agreement. Also checks that the adversarial inputs hold what they are made for."""
import numpy as np
import pytest

from tests import index_model as M
from tests import oracle as orc


def _same(a, b):
    assert M.first_difference(a[0], a[1], b[0], b[1]) is None, M.first_difference(a[0], a[1], b[0], b[1])


@pytest.mark.parametrize("k", [21, 32, 40])
@pytest.mark.parametrize("strand", [orc.SINGLE, orc.CANONICAL])
def test_count_model_follows_the_oracle(k, strand):
    """random insert / erase / count / find sequences: the model and orc.CountMap give the same answers"""
    rng = np.random.default_rng(k * 10 + strand)
    s = orc.kspec(k)
    model, om = M.CountModel(k, strand=strand), orc.CountMap(s, strand)
    for step in range(8):
        data = M.fastq(M.background(rng, 40 + 20 * step, genome_len=3000) + M.adversarial_reads(rng, k)[: 4 + step])
        kmers = orc.extract(s, data, orc.FASTQ)["kmers"]
        if step % 3 == 2:
            q = np.concatenate([kmers[::3], orc.revcomp(s, kmers[1::5])])
            assert model.erase(q) == om.erase(q)
        else:
            model.insert(kmers)
            om.insert(kmers)
        assert model.size() == om.size()
        _same(model.export(), om.export())
        q = M.probes(s, model.export()[0], rng, n_stored=400, n_absent=50)
        _same(model.count(q), om.count(q))
        _same(model.find(q), om.find(q))
        have = {tuple(r) for r in om.export()[0].tolist()}
        tq = q if strand == orc.SINGLE else orc.canonical(s, q)
        assert (model.exists(q) == np.array([tuple(r) in have for r in tq.tolist()], dtype=np.uint8)).all()


@pytest.mark.parametrize("saturating", [False, True])
@pytest.mark.parametrize("strand", [orc.SINGLE, orc.CANONICAL])
def test_count_model_pairs_and_updates(saturating, strand):
    """insert_pairs is insert repeated count times (mod 2^32, or stopping at 2^32 - 1); update_pairs touches stored keys only,
    in input order"""
    k = 31
    rng = np.random.default_rng(7 + saturating + 2 * strand)
    s = orc.kspec(k)
    kmers = orc.extract(s, M.fastq(M.background(rng, 60, genome_len=2000)), orc.FASTQ)["kmers"]
    model, om = M.CountModel(k, strand=strand, saturating=saturating), orc.CountMap(s, strand)
    c = rng.integers(1, 4, kmers.shape[0])
    model.insert_pairs(kmers, c)
    om.insert(np.repeat(kmers, c, axis=0))
    _same(model.export(), om.export())
    # counts at the ceiling: wrap or stop
    top = kmers[:5]
    model.insert_pairs(top, np.full(5, M.MASK32 - 1))
    model.insert_pairs(top, np.full(5, 3))
    ref = M.CountModel(k, strand=strand)
    ref.insert_pairs(kmers, c)
    for key in ref.count(top)[0].tolist():
        want = min(ref.d[tuple(key)] + M.MASK32 + 2, M.MASK32) if saturating else (ref.d[tuple(key)] + 1) & M.MASK32
        assert model.d[tuple(key)] == want
    # update: absent keys are not counted, assign keeps the last pair of a key
    absent = orc.kmers_from_string(s, M.random_seq(rng, 200))
    absent = absent[~model.exists(absent).astype(bool)]
    q = np.concatenate([kmers[:10], kmers[:10], absent])
    v = np.arange(q.shape[0], dtype=np.uint64) + 1
    before = dict(model.d)
    assert model.update_pairs(q, v, "assign") == 20
    for i, key in enumerate(model.transform(kmers[:10]).tolist()):
        assert model.d[tuple(key)] == 11 + i
    assert model.size() == len(before)
    model.d = dict(before)
    assert model.update_pairs(q, v, "max") == 20
    assert model.update_pairs(q, np.zeros_like(v), "min") == 20
    assert all(model.d[tuple(key)] == 0 for key in model.transform(kmers[:10]).tolist())
    model.d = dict(before)
    model.update_pairs(q[:10], np.full(10, M.MASK32), "add")   # add wraps, saturating index or not
    assert all(model.d[tuple(key)] == (before[tuple(key)] - 1) & M.MASK32 for key in model.transform(kmers[:10]).tolist())


@pytest.mark.parametrize("k", [21, 31])
def test_node_model_follows_the_oracle(k):
    """builds and tuple inserts are orc.DbgMap's; erase leaves the map the oracle builds from the surviving nodes' tuples"""
    rng = np.random.default_rng(k)
    s = orc.kspec(k)
    model = M.NodeModel(k)
    d1 = M.fastq(M.background(rng, 80, genome_len=3000) + M.poly_reads(b"A", 20))
    d2 = M.fasta(M.background(rng, 40, genome_len=3000))
    model.build(d1)
    model.build(d2, orc.FASTA)
    om = orc.DbgMap(s)
    om.insert(*orc.dbg_parse(s, d1))
    om.insert(*orc.dbg_parse(s, d2, orc.FASTA))
    assert model.size() == om.size()
    assert M.first_difference_rows(*model.export(), *om.export(canonical=True)) is None
    keys = om.export(canonical=True)[0]
    victims = keys[rng.permutation(keys.shape[0])[: keys.shape[0] // 4]]
    q = np.concatenate([victims, orc.revcomp(s, victims[:10]), orc.kmers_from_string(s, M.random_seq(rng, 100))])
    gone = {tuple(r) for r in victims.tolist()}
    assert model.erase(q) == len(gone)
    survivors = np.array([tuple(r) not in gone for r in orc.canonical(s, np.concatenate(
        [orc.dbg_parse(s, d1)[0], orc.dbg_parse(s, d2, orc.FASTA)[0]])).tolist()])
    om2 = orc.DbgMap(s)
    km = np.concatenate([orc.dbg_parse(s, d1)[0], orc.dbg_parse(s, d2, orc.FASTA)[0]])
    ed = np.concatenate([orc.dbg_parse(s, d1)[1], orc.dbg_parse(s, d2, orc.FASTA)[1]])
    om2.insert(km[survivors], ed[survivors])
    assert M.first_difference_rows(*model.export(), *om2.export(canonical=True)) is None
    ck, cc = model.count(q)
    assert int(cc.sum()) == 0 or set(map(tuple, ck[cc == 1].tolist())) <= {tuple(r) for r in om2.export(canonical=True)[0].tolist()}
    assert model.find(victims)[0].shape[0] == 0
    assert model.erase(victims) == 0


@pytest.mark.parametrize("k", list(range(17, 33)))
def test_adversarial_reads_hold_what_they_claim(k):
    rng = np.random.default_rng(k)
    reads = M.adversarial_reads(rng, k)
    data = M.fastq(reads)
    recs = orc.records(data, orc.FASTQ)
    assert len(recs) == len(reads)
    lengths = [r.seq_end - r.seq_begin for r in recs]
    assert lengths == [len(r) for r in reads]
    nmax = M.sk_nmax_of(k)
    assert {k, k + nmax - 1, k + nmax} <= set(lengths)
    assert reads[0] == b"A" * 150 and reads[1] == b"T" * 150
    for p in range(1, 9):   # periodic reads
        assert any(len(r) >= 150 and r[p:] == r[:-p] and len(set(r)) > 1 or (p == 1 and len(set(r)) == 1) for r in reads)
    m = k - M.sk_window_of(k) + 1
    for mm in {m - m % 2, 12, 14, 16}:   # palindromic m-mers (even m) are present
        assert any(r[i:i + mm] == M.revcomp_text(r[i:i + mm]) for r in reads for i in range(len(r) - mm + 1)), mm
    assert any(r[len(r) // 2:] == M.revcomp_text(r[: len(r) // 2]) and len(set(r)) > 2 for r in reads)   # read + its revcomp
    fa = orc.records(M.fasta(reads), orc.FASTA)
    assert len(fa) == len(reads)
    assert len(data) < 300_000
    s = orc.kspec(k)
    assert orc.extract(s, M.fasta(reads), orc.FASTA)["kmers"].shape[0] == orc.extract(s, data, orc.FASTQ)["kmers"].shape[0]


def test_other_generators():
    rng = np.random.default_rng(5)
    k = 31
    crowded = M.crowded_reads(rng, 3000)
    assert len(crowded) == 3000 and len(set(crowded)) == 1
    reads = M.background(rng, 200)
    withn = M.with_n_runs(rng, reads, k)
    assert sum(b"N" in r for r in withn) >= 50 and all(len(a) == len(b) for a, b in zip(reads, withn))
    s = orc.kspec(k)
    split = orc.extract(s, M.fastq(withn), orc.FASTQ, seq_filter=orc.SEQ_N_SPLIT)["kmers"].shape[0]
    plain = orc.extract(s, M.fastq(withn), orc.FASTQ)["kmers"].shape[0]
    assert split < plain
    stored = orc.extract(s, M.fastq(reads), orc.FASTQ)["kmers"]
    q = M.probes(s, stored, rng)
    have = {tuple(r) for r in stored.tolist()}
    assert sum(tuple(r) in have for r in q.tolist()) >= 1500                 # stored keys
    assert (q == orc.kmers_from_string(s, b"T" * k)).all(axis=1).any() and (q == 0).all(axis=1).any()
    var = M.one_base_variants(s, stored[:10], [0, k - 1])
    assert all(bin(int(a) ^ int(b)).count("1") in (1, 2) for a, b in zip(var[:10, 0], stored[:10, 0]))
