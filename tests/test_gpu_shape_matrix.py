"""Every kernel family once per (n_words, bits) instantiation that the other modules never run -- <4,2> (DNA k = 97..128), <4,3>
(DNA5 k = 65..85), <4,4> (DNA16 k = 49..64) -- or run for extraction and a count build alone -- <2,4> <3,4> (DNA16 k = 17..48,
test_gpu_filters.py) -- and at the two 3-bit edges k = 43 and k = 64, exact against tests/oracle.py
and the plain models over it. Families b and c also run one shape of each of the other seven instantiations, so that their ids
name all twelve. The inputs are reads over the alphabet's own letters (N in DNA5, the fifteen IUPAC letters and lower case in
DNA16) of ragged lengths that include k - 1, k, k + 1 and 2k, as FASTQ and FASTA, LF and CRLF.

Where the record of a kernel is wider than four words the partition takes its plain fine scatter (partition_impl, RW >= 5):
  RW = 5: four-word k-mers with one value word -- insert_pairs / update_pairs / lookup (test_value_carrying_records), the
          position index and kmi_route_tuples_dev (test_position_indexes), de Bruijn records (test_de_bruijn_nodes);
          three-word k-mers with two value words -- position + quality at (48, DNA16) and (64, DNA5)
  RW = 6: four-word k-mers with two value words -- position + quality at (128, DNA), (85, DNA5), (64, DNA16)
test_one_fine_bucket_fuller_than_a_tagged_table reaches the multi-pass reduce of TabCfg<4> and the chunk loops of
bucket_update_kernel and dbg_accumulate_kernel at two and four words."""
import functools

import numpy as np
import pytest

from tests import index_model as M
from tests import oracle as orc
from tests import read_profile_model as RP
from tests import setops_model as SM
from tests import spectrum_cases as S
from tests import unitig_model as UM
from tests.shape_cases import ALPHA, BITS, NEW, OLD, REDUCED, n_words
from tests.test_gpu_debruijn import _nodes, check_erase_nodes, check_nodes_build_insert_find
from tests.test_gpu_filters import FILTERS, _check_extract
from tests.test_gpu_index import (STRAND, _keys_in_one_placement_bucket, _same_map, check_extract_route, check_route,
                                  check_split_and_merge_replay, check_update_with_device_updaters, place_hash_np)
from tests.test_gpu_kmer_ops import _random_kmers
from tests.test_gpu_position_index import check_build_insert_query, check_extract_route_records, check_route_tuples
from tests.test_gpu_quality import check_position_quality_index, check_quality_bit_exact
from tests.test_gpu_setops import _assert_overlap
from tests.test_gpu_unitigs import _gpu as _gpu_unitigs

pytestmark = pytest.mark.gpu

RNA = [(100, "RNA")]
ALL = OLD + NEW + RNA          # families b and c: every (n_words, bits) pair
LETTERS = {"DNA": b"ACGT", "RNA": b"ACGU", "DNA5": b"ACGT", "DNA16": b"ACGTRYKMSWBDHVN"}
N_RATE = {"DNA": 0.003, "RNA": 0.003, "DNA5": 0.01, "DNA16": 0.0}      # (N is one of DNA16's letters)
LOWER_RATE = {"DNA": 0.0, "RNA": 0.0, "DNA5": 0.02, "DNA16": 0.1}


def _id(shape):
    k, alpha = shape
    return "k%d-%s-%dx%d" % (k, alpha, n_words(k, alpha), BITS[alpha])


def _shapes(shapes):
    return pytest.mark.parametrize("k,alpha", shapes, ids=[_id(x) for x in shapes])


@pytest.fixture(scope="module")
def ctx():
    import kmerind_amd as K
    c = K.Context(0)
    yield c
    c.close()


# ---- inputs: computed once per shape, never changed
def _sample_reads(rng, genome, k, alpha, n_reads):
    """reads of both batches come from one genome, so that k-mers repeat within and across them"""
    lens = rng.integers(max(1, k - 1), k + 90, n_reads)
    lens[:8] = [k - 1, k, k + 1, 2 * k] * 2
    out = []
    for ln in lens.tolist():
        p = int(rng.integers(0, genome.size - ln + 1))
        r = genome[p:p + ln].copy()
        if N_RATE[alpha]:
            r[rng.random(ln) < N_RATE[alpha]] = ord("N")
        if LOWER_RATE[alpha]:
            low = rng.random(ln) < LOWER_RATE[alpha]
            r[low] |= 0x20
        out.append(r.tobytes())
    return out


def _fastq(rng, reads, eol):
    return b"".join(b"@r%d" % i + eol + r + eol + b"+" + eol + bytes(rng.integers(33, 74, len(r), dtype=np.uint8).tolist()) + eol
                    for i, r in enumerate(reads))


def _fasta(reads, eol, width):
    out = []
    for i, r in enumerate(reads):
        out.append(b">r%d some text" % i + eol)
        out.extend(r[j:j + width] + eol for j in range(0, len(r), width))
    return b"".join(out)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(k, alpha):
    c = Case()
    rng = np.random.default_rng(1000 * k + BITS[alpha])
    letters = np.frombuffer(LETTERS[alpha], dtype=np.uint8)
    # (DNA16: four letters in five are A, C, G or T, the rest is spread over the eleven others, N among them at under 2 %)
    weights = np.full(letters.size, 1.0 / letters.size) if alpha != "DNA16" else np.array([0.2] * 4 + [0.2 / 11] * 11)
    genome = rng.choice(letters, size=2000, p=weights)
    other = rng.choice(letters, size=1200, p=weights)       # an unrelated genome: keys that only one of two samples holds
    c.s = orc.kspec(k, ALPHA[alpha])
    c.reads, c.reads2 = _sample_reads(rng, genome, k, alpha, 1000), _sample_reads(rng, genome, k, alpha, 400)
    c.other = _sample_reads(rng, other, k, alpha, 120)
    c.width = 37 if k % 37 else 41                   # FASTA line width: no divisor of k
    assert k % c.width
    c.fastq = {eol: _fastq(rng, c.reads, eol) for eol in (b"\n", b"\r\n")}
    c.fasta = {eol: _fasta(c.reads, eol, c.width) for eol in (b"\n", b"\r\n")}
    c.fastq2 = _fastq(rng, c.reads2, b"\n")
    c.kmers = orc.extract(c.s, c.fastq[b"\n"], orc.FASTQ)["kmers"]
    c.kmers2 = orc.extract(c.s, c.fastq2, orc.FASTQ)["kmers"]
    assert np.unique(c.kmers, axis=0).shape[0] * 4 < 3 * c.kmers.shape[0]    # k-mers repeat (those without an N many times)
    c.absent = orc.kmers_from_string(c.s, letters[rng.integers(0, letters.size, 300 + k)].tobytes())
    return c


def _queries(c, rng, n=3000):
    """present k-mers (with repeats), some under the other strand, absent ones, duplicates; shuffled"""
    present = c.kmers[rng.integers(0, c.kmers.shape[0], size=n)]
    q = np.concatenate([present, orc.revcomp(c.s, present[: n // 5]), c.absent, present[:100]])
    return q[rng.permutation(q.shape[0])]


def _transformed(s, strand, kmers):
    return kmers if strand == "single" else orc.canonical(s, kmers)


def _rows(a):
    return [tuple(r) for r in np.asarray(a).tolist()]


# ---- b. extraction
@_shapes(ALL)
def test_extraction_fastq_and_fasta_under_every_filter(ctx, k, alpha):
    """k-mers in file order with their position ids, FASTQ and FASTA (lines of a width that is no divisor of k), LF and CRLF, under
    the three sequence filters; k-mers alone off a count configuration; (k-mer, id, quality) bit for bit where valid_config
    takes the combination (no filter with qualities)"""
    import kmerind_amd as K
    c = _case(k, alpha)
    for eol in (b"\n", b"\r\n"):
        for fmt, data in (("fastq", c.fastq[eol]), ("fasta", c.fasta[eol])):
            for flt in FILTERS:
                got, ex = _check_extract(ctx, data, fmt, k, alpha, flt)
                assert ex["kmers"].shape[0] > 0
                if fmt == "fastq" or flt == "n_filter":
                    assert got["n_seqs"] == ex["n_seqs"], (fmt, flt)
            _check_extract(ctx, data, fmt, k, alpha, "all", with_ids=False)
        check_quality_bit_exact(ctx, c.s, K.make_config(k, alpha, index_kind="posqual"), c.fastq[eol])
    if N_RATE[alpha]:      # the filters had something to do
        n = {flt: orc.extract(c.s, c.fastq[b"\n"], orc.FASTQ, seq_filter=FILTERS[flt])["kmers"].shape[0] for flt in FILTERS}
        assert n["n_filter"] < n["all"]


# ---- c. count index
@pytest.mark.parametrize("strand", ["single", "canonical", "bimolecule"])
@_shapes(ALL)
def test_count_index_build_insert_query_erase(ctx, k, alpha, strand):
    """build (single: FASTQ with LF, canonical: FASTQ with CRLF, bimolecule: FASTA), a second insert into the filled buckets,
    to_vector, count / find / exists, erase, insert of transformed keys: orc.CountMap throughout"""
    import kmerind_amd as K
    c = _case(k, alpha)
    s = c.s
    fmt, data = {"single": ("fastq", c.fastq[b"\n"]), "canonical": ("fastq", c.fastq[b"\r\n"]), "bimolecule": ("fasta", c.fasta[b"\n"])}[strand]
    ex = c.kmers if fmt == "fastq" else orc.extract(s, data, orc.FASTA)["kmers"]
    om = orc.CountMap(s, STRAND[strand])
    om.insert(ex)
    idx = K.CountIndex(ctx, K.make_config(k, alpha, strand=strand, seq_format=fmt))
    idx.build(data)
    _same_map(idx, om)
    om.insert(c.kmers2)
    idx.insert(c.kmers2)
    _same_map(idx, om)
    rng = np.random.default_rng(k)
    q = _queries(c, rng)
    for fn in ("count", "find"):
        gk, gv = getattr(idx, fn)(q)
        ok, ov = getattr(om, fn)(q)
        a, b = orc.sorted_pairs(gk, gv), orc.sorted_pairs(ok, ov.astype(np.uint64))
        assert a[0].shape == b[0].shape and (a[0] == b[0]).all() and (a[1] == b[1]).all(), fn
    stored = set(_rows(om.export()[0]))
    want = np.array([t in stored for t in _rows(_transformed(s, strand, q))], dtype=np.uint8)
    assert want.any() and not want.all() and (idx.exists(q) == want).all()
    er = q[::2]
    assert idx.erase(er) == om.erase(er) > 0
    _same_map(idx, om)
    gk, gv = idx.count(q)
    ok, ov = om.count(q)
    a, b = orc.sorted_pairs(gk, gv), orc.sorted_pairs(ok, ov)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    tk = _transformed(s, strand, c.kmers2)               # routed keys after an exchange: transformed already
    d = ctx.alloc(tk.nbytes)
    ctx.to_device(d, tk)
    idx.insert_device(d, tk.shape[0], transformed=True)
    ctx.free(d)
    om.insert(c.kmers2)
    _same_map(idx, om)
    idx.close()


# ---- d. value-carrying records
@pytest.mark.parametrize("strand", ["single", "canonical"])
@_shapes(REDUCED + [(97, "DNA")])
def test_value_carrying_records(ctx, k, alpha, strand):
    """weighted insert_pairs, lookup in query order, profile_reads: records of n_words + 1 words (five at four-word k-mers) against
    index_model.CountModel and read_profile_model"""
    import kmerind_amd as K
    c = _case(k, alpha)
    s = c.s
    rng = np.random.default_rng(2 * k)
    model = M.CountModel(k, ALPHA[alpha], STRAND[strand])
    idx = K.CountIndex(ctx, K.make_config(k, alpha, strand=strand))
    idx.build(c.fastq[b"\n"])
    model.insert(c.kmers)
    q = _queries(c, rng)
    pick = rng.integers(0, c.kmers2.shape[0], 4000)
    pk = np.concatenate([c.kmers2[pick], orc.revcomp(s, c.kmers2[pick[:400]]), c.absent[:50]])
    pw = rng.integers(0, 1000, pk.shape[0]).astype(np.uint64)
    pw[:3] = np.uint64(0xFFFFFFFF)                        # wraps like uint32_t addition
    idx.insert_pairs(pk, pw)
    model.insert_pairs(pk, pw)
    assert M.state_difference(idx, model, q) is None
    empty, m2 = K.CountIndex(ctx, K.make_config(k, alpha, strand=strand)), M.CountModel(k, ALPHA[alpha], STRAND[strand])
    empty.insert_pairs(pk, pw)                            # pairs into an empty index
    m2.insert_pairs(pk, pw)
    assert M.first_difference(*empty.to_vector(), *m2.export()) is None
    empty.close()
    want = RP.lookup(model, q)
    assert (want > 0).any() and (want == 0).any()
    got = idx.lookup(q)
    assert got.dtype == np.uint32 and (got == want).all()
    d = RP.first_row_difference(idx.profile_reads(c.fastq2, solid=2), RP.profile(c.fastq2, s, model, 2))
    assert d is None, d
    idx.close()


@_shapes(REDUCED + [(97, "DNA")])
def test_update_pairs_with_every_updater(ctx, k, alpha):
    """add, max, min, assign, add in sequence; absent keys and keys under the other strand among the pairs"""
    import kmerind_amd as K
    c = _case(k, alpha)
    for strand in ("canonical", "single"):
        check_update_with_device_updaters(ctx, c.s, K.make_config(k, alpha, strand=strand), strand, c.fastq[b"\n"], c.absent, seed=k)


# ---- e. spectrum and filter
@_shapes(REDUCED)
def test_spectrum_and_retain_counts(ctx, k, alpha):
    import kmerind_amd as K
    c = _case(k, alpha)
    model = M.CountModel(k, ALPHA[alpha], orc.CANONICAL)
    model.insert(c.kmers)
    top = int(model.export()[1].max())
    assert top > 8
    q = _queries(c, np.random.default_rng(3 * k))
    for lo, hi in ((3, 2**32 - 1), (0, top // 2), (top + 1, 2**32 - 1)):          # a lower bound, an upper bound, an empty range
        idx = K.CountIndex(ctx, K.make_config(k, alpha, strand="canonical"))
        idx.build(c.fastq[b"\n"])
        for n_bins in (2, 256, top + 1):
            S.assert_spectrum(idx.spectrum(n_bins), S.model_spectrum(model, n_bins), "n_bins=%d" % n_bins)
            S.assert_spectrum(S.spectrum_device(ctx, idx, n_bins), S.model_spectrum(model, n_bins), "n_bins=%d device" % n_bins)
        want = model.copy()
        want.d = {key: v for key, v in model.d.items() if lo <= v <= hi}
        assert idx.retain_counts(lo, hi) == model.size() - want.size() > 0
        assert M.state_difference(idx, want, q) is None
        S.assert_spectrum(idx.spectrum(256), S.model_spectrum(want, 256), "after retain_counts(%d, %d)" % (lo, hi))
        if want.size() == 0:
            assert lo == top + 1
        idx.close()


# ---- f. set operations
@pytest.mark.parametrize("call", SM.OPS + ("compare",))
@_shapes(REDUCED)
def test_set_operations(ctx, k, alpha, call):
    """a = the first 650 reads, b = the reads from 350 on with the second batch: overlapping halves of the input; each with
    its own half of the reads of an unrelated genome"""
    import kmerind_amd as K
    c = _case(k, alpha)
    rng = np.random.default_rng(5 * k)
    data_a = _fastq(rng, c.reads[:650] + c.other[:60], b"\n")
    data_b = _fastq(rng, c.reads[350:] + c.reads2 + c.other[60:], b"\r\n")
    cfg = K.make_config(k, alpha, strand="canonical")
    ma, mb = M.CountModel(k, ALPHA[alpha], orc.CANONICAL), M.CountModel(k, ALPHA[alpha], orc.CANONICAL)
    ma.insert(orc.extract(c.s, data_a, orc.FASTQ)["kmers"])
    mb.insert(orc.extract(c.s, data_b, orc.FASTQ)["kmers"])
    shared = [key for key in ma.d if key in mb.d]          # no op can pass degenerately
    assert shared and any(key not in mb.d for key in ma.d) and any(key not in ma.d for key in mb.d)
    assert any(ma.d[key] < mb.d[key] for key in shared) and any(ma.d[key] > mb.d[key] for key in shared)
    a, b = K.CountIndex(ctx, cfg), K.CountIndex(ctx, cfg)
    a.build(data_a)
    b.build(data_b)
    q = _queries(c, rng)
    if call == "compare":
        _assert_overlap(a.compare(b), SM.overlap(ma, mb))
        _assert_overlap(b.compare(a), SM.overlap(mb, ma), "the other way round")
        assert M.state_difference(a, ma, q) is None
    else:
        want = SM.combined(ma, mb, call)
        assert a.combine(b, call) == want.size() == a.local_size()
        assert M.state_difference(a, want, q) is None
        a.insert(c.kmers2)                                  # the result goes on working
        want.insert(c.kmers2)
        assert M.state_difference(a, want, q) is None
    assert M.state_difference(b, mb, q) is None             # b's entries did not move
    a.close()
    b.close()


# ---- g. position and position + quality indexes
@_shapes(REDUCED + [(64, "DNA5")])
def test_position_indexes(ctx, k, alpha):
    """records of n_words + 1 (position) and n_words + 2 (position + quality) words: five and six of them at the three- and
    four-word shapes"""
    import kmerind_amd as K
    c = _case(k, alpha)
    strand = {(85, "DNA5"): "bimolecule", (32, "DNA16"): "single", (64, "DNA5"): "single"}.get((k, alpha), "canonical")
    cfg = K.make_config(k, alpha, strand=strand, index_kind="position")
    check_build_insert_query(ctx, c.s, cfg, strand, c.fastq[b"\r\n"], c.fastq2, c.absent, seed=k)
    cfg_c = K.make_config(k, alpha, strand="canonical", index_kind="position")
    cfg_q = K.make_config(k, alpha, strand="canonical", index_kind="posqual")
    check_position_quality_index(ctx, c.s, cfg_q, c.fastq[b"\n"])
    if n_words(k, alpha) == 4:
        check_route_tuples(ctx, c.s, cfg_c, c.fastq[b"\n"], 3)
        for kind, cf in (("position", cfg_c), ("posqual", cfg_q)):
            check_extract_route_records(ctx, c.s, cf, kind, c.fastq[b"\n"], 3, 7_000_000, len(c.reads))


# ---- h. routing and the replayed multi-rank build
@_shapes(REDUCED)
def test_routing_and_replayed_multi_rank_build(ctx, k, alpha):
    import kmerind_amd as K
    c = _case(k, alpha)
    for strand, dh, p in (("canonical", "murmur", 3), ("single", "farm", 2), ("bimolecule", "identity", 5)):
        cfg = K.make_config(k, alpha, strand=strand, dist_hash=dh)
        dist_hash = {"murmur": orc.MURMUR, "farm": orc.FARM, "identity": orc.IDENTITY}[dh]
        check_route(ctx, c.s, cfg, strand, dist_hash, c.kmers2, (1, 2, 3, 8))
        data = np.frombuffer(c.fastq[b"\n"], dtype=np.uint8)
        ex, segs = check_extract_route(ctx, c.s, cfg, strand, dist_hash, data, p, len(c.reads))
        assert sum(seg.shape[0] for seg in segs) == ex.shape[0] == c.kmers.shape[0]
    rng = np.random.default_rng(7 * k)
    p = 3
    parts = {(rnd, r): np.frombuffer(_fastq(rng, (c.reads if rnd == 0 else c.reads2)[r::p], b"\n"), dtype=np.uint8)
             for rnd in range(2) for r in range(p)}
    check_split_and_merge_replay(ctx, c.s, K.make_config(k, alpha, strand="canonical"), "canonical", orc.MURMUR, p,
                                 lambda rnd, r: parts[(rnd, r)])


# ---- i. de Bruijn nodes and unitigs
@_shapes(REDUCED)
def test_de_bruijn_nodes(ctx, k, alpha):
    """parser tuples bit for bit, build, insert(tuples), find, count, erase: the edge nibbles of multi-word DNA16 k-mers too"""
    import kmerind_amd as K
    c = _case(k, alpha)
    cfg = K.make_config(k, alpha)
    check_nodes_build_insert_find(ctx, c.s, cfg, c.fastq[b"\r\n"], c.fastq2, c.absent, seed=k)
    check_erase_nodes(ctx, c.s, cfg, c.fastq[b"\n"], c.fastq2, c.absent, seed=k)


@pytest.mark.parametrize("k", [97, 128])
def test_unitigs_of_four_word_nodes(ctx, k):
    """kmi_dbg_compact takes 2-bit alphabets only (test_gpu_unitigs.py::test_refusals): the DNA shapes"""
    import kmerind_amd as K
    c = _case(k, "DNA")
    data = c.fastq[b"\n"] + c.fastq2
    om = orc.DbgMap(c.s)
    om.insert(*orc.dbg_parse(c.s, data))
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    g.build(data)
    for t in (1, 2):
        exp = UM.unitigs(*om.export(canonical=True), k, t)
        assert len(exp) > 3 and _gpu_unitigs(g, t) == exp, t
    g.close()


# ---- j. one fine bucket fuller than a tagged table
N_HOT = 6000              # distinct keys of index a in the chosen bucket
TAB_LIMIT = {4: 2784, 2: 4608}      # TabCfg<NW>::LIMIT = CAP * 3 / 4 of CAP = 3712 (four words) and 6144 (two words)
DBG_ROWS = 1536           # DbgCfg<NW>::ROWS = 2048 * 3 / 4 for every NW > 1: rows per chunk of bucket_update / dbg_accumulate
BUCKET = 4242


@_shapes([(128, "DNA"), (85, "DNA5"), (32, "DNA16")])
def test_one_fine_bucket_fuller_than_a_tagged_table(k, alpha):
    """N_HOT = 6000 distinct multi-word keys in ONE fine bucket, each one to three times, among 20 000 random keys: more than two
    tables of TabCfg<4>::LIMIT = 2784 (four words: (128, DNA), (85, DNA5)), more than one of TabCfg<2>::LIMIT = 4608 ((32, DNA16)),
    and four chunks of DbgCfg::ROWS = 1536. So the reduce, the lookup and the join run in passes (debug counters 8 and 10 say
    so) and bucket_update_kernel and dbg_accumulate_kernel walk the bucket in chunks. Single strand; every step against a
    dict mirror (index_model.CountModel, orc.DbgMap)."""
    import kmerind_amd as K
    nw = n_words(k, alpha)
    assert N_HOT > 2 * TAB_LIMIT[4] and N_HOT > TAB_LIMIT[2] and N_HOT > 3 * DBG_ROWS
    ctx = K.Context(0)
    s = orc.kspec(k, ALPHA[alpha])
    pad = nw * 64 - s.n_bits
    # the words above word 0 are the same for every hot key; the top 16 bits of the last one are zero (so are the pad bits)
    later = (0xFEDCBA9876543210, 0x0123456789ABCDEF, 0x0000123456789ABC)[-(nw - 1):]
    cand = _keys_in_one_placement_bucket(N_HOT * 3 // 2, BUCKET, later_words=later)
    assert cand.shape == (N_HOT * 3 // 2, nw) and np.unique(cand, axis=0).shape[0] == cand.shape[0]
    assert (place_hash_np(cand) >> np.uint64(17) == BUCKET).all() and (cand[:, -1] >> np.uint64(64 - max(pad, 1)) == 0).all()
    hot_a, hot_b = cand[:N_HOT], cand[N_HOT // 2:]          # b shares half of a's hot keys and brings as many of its own
    rng = np.random.default_rng(k)
    cfg = K.make_config(k, alpha, strand="single")
    ma, mb = M.CountModel(k, ALPHA[alpha], orc.SINGLE), M.CountModel(k, ALPHA[alpha], orc.SINGLE)

    def batch(hot, seed):
        keys = np.concatenate([np.repeat(hot, rng.integers(1, 4, size=hot.shape[0]), axis=0), _random_kmers(s, 20_000, seed)])
        return keys[rng.permutation(keys.shape[0])]

    a = K.CountIndex(ctx, cfg)
    for rnd in range(2):                                   # the second insert merges into the full bucket
        keys = batch(hot_a, 10 + rnd)
        a.insert(keys)
        ma.insert(keys)
        assert M.first_difference(*a.to_vector(), *ma.export()) is None, rnd
    # the hot keys really share a bucket: the per-bucket counts of a one-rank split
    n, nb = a.local_size(), K.core.num_buckets()
    dk, dc, db = ctx.alloc(n * nw * 8 + 64), ctx.alloc(n * 4 + 64), ctx.alloc(nb * 4)
    a.split_by_rank_device(1, dk, dc, n, db)
    per_bucket = np.zeros(nb, np.uint32)
    ctx.to_host(per_bucket, db)
    ctx.free(dk); ctx.free(dc); ctx.free(db)
    assert int(per_bucket.sum()) == n and int(per_bucket[BUCKET]) >= N_HOT and int(np.delete(per_bucket, BUCKET).max()) < 200
    # lookup in query order
    absent = _random_kmers(s, 1000, 99)
    q = np.concatenate([hot_a[::2], hot_b[N_HOT // 2::2], absent, hot_a[:500]])
    q = q[rng.permutation(q.shape[0])]
    want = RP.lookup(ma, q)
    assert (want > 0).any() and (want == 0).any()
    assert (a.lookup(q) == want).all()
    assert ctx.debug_counter(8) >= 2                        # N_HOT entries > TAB_LIMIT of the bucket's table: passes
    # update_pairs: the bucket's entries go through the table in chunks of DBG_ROWS
    for op in ("add", "assign"):
        v = rng.integers(0, 50, size=q.shape[0]).astype(np.uint32)
        assert a.update_pairs(q, v, op) == ma.update_pairs(q, v, op) > N_HOT // 2
        assert M.first_difference(*a.to_vector(), *ma.export()) is None, op
    # compare and combine with an index that shares half the hot keys
    b = K.CountIndex(ctx, cfg)
    keys = batch(hot_b, 20)
    b.insert(keys)
    mb.insert(keys)
    _assert_overlap(a.compare(b), SM.overlap(ma, mb))
    assert ctx.debug_counter(10) >= 2                       # b's N_HOT entries of the bucket > TAB_LIMIT: the join runs in passes
    assert SM.overlap(ma, mb)["n_shared"] == N_HOT // 2
    c2 = K.CountIndex(ctx, cfg)
    c2.combine(a, "union_add")                              # a copy of a for the combine
    want = SM.combined(ma, mb, "intersect_min")
    assert c2.combine(b, "intersect_min") == want.size() == N_HOT // 2
    assert ctx.debug_counter(10) >= 2
    assert M.first_difference(*c2.to_vector(), *want.export()) is None
    assert M.first_difference(*b.to_vector(), *mb.export()) is None
    c2.close()
    b.close()
    # find / count / erase of a third of the hot keys and absent ones
    q = np.concatenate([hot_a[::3], absent, hot_a[:90:3]])
    for fn in ("find", "count"):
        assert M.first_difference(*getattr(a, fn)(q), *getattr(ma, fn)(q)) is None, fn
    assert a.erase(q) == ma.erase(q) == hot_a[::3].shape[0]
    assert M.first_difference(*a.to_vector(), *ma.export()) is None
    a.close()
    # de Bruijn nodes of the same keys with random edge nibbles: the ones that are their own smaller strand stay in the bucket
    hot = hot_a[(orc.canonical(s, hot_a) == hot_a).all(axis=1)]
    assert hot.shape[0] > 3 * DBG_ROWS
    om = orc.DbgMap(s)
    g = K.DeBruijnNodes(ctx, K.make_config(k, alpha))
    for rnd in range(2):
        sel = hot if rnd == 0 else hot[::2]
        keys = np.concatenate([np.repeat(sel, 3, axis=0), _random_kmers(s, 20_000, 30 + rnd)])
        keys = keys[rng.permutation(keys.shape[0])]
        edges = rng.integers(0, 256, size=keys.shape[0]).astype(np.uint8)
        om.insert(keys, edges)
        g.insert(keys, edges)
        assert g.local_size() == om.size()
        assert (_nodes(*g.to_vector()) == _nodes(*om.export(canonical=True))).all()
    fk, fc = g.find(hot[::5])
    assert fk.shape[0] == hot[::5].shape[0] and (_nodes(fk, fc) == _nodes(*om.find(hot[::5], canonical=True))).all()
    g.close()
    ctx.close()
