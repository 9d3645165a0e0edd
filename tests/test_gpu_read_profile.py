"""kmi_index_profile_reads_*: one row per FASTQ record, straight from the bytes, against tests/read_profile_model.py (the oracle's
parser and a CountModel): files profiled against their own index, reads of one genome against the index of another batch of it,
reads with and without k-mers, batches, unaligned buffers, capacities, malformed input, and the example program."""
import os
import subprocess

import numpy as np
import pytest

from tests import index_model as M
from tests import oracle as orc
from tests import read_profile_model as RP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
STRAND = {"single": orc.SINGLE, "canonical": orc.CANONICAL}
ALPHA = {"DNA": orc.DNA, "DNA5": orc.DNA5}


@pytest.fixture(scope="module")
def ctx():
    import kmerind_amd as K
    c = K.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_small_batches():
    import kmerind_amd as K
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("KMI_PROFILE_BATCH", "4096")
        c = K.Context(0)
    yield c
    c.close()


def _profile_device(ctx, idx, data, solid=2, capacity=None, shift=0):
    """rows through kmi_index_profile_reads_dev; shift: the bytes start that far into their device buffer"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n_rec = len(orc.records(data, orc.FASTQ))
    cap = n_rec if capacity is None else capacity
    d, o = ctx.alloc(buf.size + 64 + shift), ctx.alloc(40 * (cap + 1))
    try:
        staged = np.concatenate([np.zeros(shift, dtype=np.uint8), buf])
        ctx.to_device(d, staged)
        guard = np.full(cap + 1, 0xAB, dtype=np.uint8).repeat(40).view(RP.ROW)
        ctx.to_device(o, guard)
        err = None
        try:
            n = idx.profile_reads_device(d + shift, buf.size, o, cap, solid)
        except Exception as e:   # (the guard row is checked for a refused call too)
            err, n = e, 0
        out = np.zeros(cap + 1, dtype=RP.ROW)
        ctx.to_host(out, o)
        assert out[cap] == guard[cap], "a row was written past the capacity"
        if err is not None:
            err.rows = out[:cap]
            raise err
        return out[:n]
    finally:
        ctx.free(d)
        ctx.free(o)


def _index_of(ctx, data, k, alphabet="DNA", strand="canonical"):
    import kmerind_amd as K
    s = orc.kspec(k, ALPHA[alphabet])
    model = M.CountModel(k, ALPHA[alphabet], STRAND[strand])
    model.insert(orc.extract(s, data, orc.FASTQ)["kmers"])
    idx = K.CountIndex(ctx, K.make_config(k, alphabet, strand=strand))
    idx.build(data)
    return idx, model, s


def _assert_rows(got, want, where):
    d = RP.first_row_difference(got, want)
    assert d is None, "%s: %s" % (where, d)


@pytest.mark.parametrize("k", [21, 31])
@pytest.mark.parametrize("fname", ["test.small.fastq", "natural.withN.fastq", "test.medium.fastq"])
def test_files_against_their_own_index(ctx, fname, k):
    data = open(os.path.join(DATA, fname), "rb").read()
    idx, model, s = _index_of(ctx, data, k)
    want = RP.profile(data, s, model, 2)
    ctx.profile(True)
    ctx.profile_reset()
    got = _profile_device(ctx, idx, data)
    names = {p["name"] for p in ctx.profile_get() if p["launches"]}
    ctx.profile(False)
    assert {"bucket_lookup", "read_profile_reduce"} <= names, sorted(names)
    _assert_rows(got, want, "%s k=%d device" % (fname, k))
    _assert_rows(idx.profile_reads(data), want, "%s k=%d host" % (fname, k))
    counts = model.export()[1].astype(np.uint64)
    assert int(got["sum_counts"].sum()) == int((counts * counts).sum())
    assert (got["n_present"] == got["n_kmers"]).all()
    idx.close()


def _substituted(rng, read):
    p = int(rng.integers(0, len(read)))
    return read[:p] + bytes([b"ACGT"[(b"ACGT".index(read[p]) + 1 + int(rng.integers(0, 3))) % 4]]) + read[p + 1:]


@pytest.mark.parametrize("k,alphabet,strand", [(17, "DNA", "canonical"), (31, "DNA", "canonical"), (32, "DNA", "canonical"), (31, "DNA", "single"),
                                               (63, "DNA", "canonical"), (21, "DNA5", "canonical")])
def test_reads_against_another_batch_of_the_same_genome(ctx, k, alphabet, strand):
    rng = np.random.default_rng(300 + k)
    genome, other = M.random_seq(rng, 20_000), M.random_seq(rng, 20_000)
    a = M.fastq(M.background(rng, 300, genome=genome))
    b = M.fastq([_substituted(rng, r) for r in M.background(rng, 150, genome=genome)] + M.background(rng, 150, genome=other) +
                M.adversarial_reads(rng, k), tag=b"q")
    idx, model, s = _index_of(ctx, a, k, alphabet, strand)
    for solid in (1, 2, 5):
        want = RP.profile(b, s, model, solid)
        if solid == 2:
            assert ((want["n_present"] > 0) & (want["n_present"] < want["n_kmers"])).any()
            assert ((want["n_present"] == 0) & (want["n_kmers"] > 0)).any() and (want["n_kmers"] == 0).any()
        _assert_rows(_profile_device(ctx, idx, b, solid), want, "k=%d %s %s solid=%d" % (k, alphabet, strand, solid))
    idx.close()


def test_reads_without_kmers_and_cut_records_get_their_rows(ctx):
    k = 21
    rng = np.random.default_rng(9)
    genome = M.random_seq(rng, 5_000)
    idx, model, s = _index_of(ctx, M.fastq(M.background(rng, 100, genome=genome)), k)
    seqs = [genome[10:10 + k - 1], genome[40:40 + k], genome[90:90 + k + 1], genome[200:350], b"AC", genome[400:400 + k + 5]]
    whole = M.fastq(seqs)
    for what, data in (("trailing newline", whole), ("no trailing newline", whole[:-1]), ("CRLF", whole.replace(b"\n", b"\r\n")),
                       ("last record is its header", whole + b"@empty\n"), ("last record lacks its quality line", whole + b"@cut\n" + genome[500:560] + b"\n+\n"),
                       ("one short read", M.fastq([b"ACGT"]))):
        recs = orc.records(data, orc.FASTQ)
        want = RP.profile(data, s, model, 2)
        got = _profile_device(ctx, idx, data)
        _assert_rows(got, want, what)
        assert got.shape[0] == len(recs) and [int(x) for x in got["seq_offset"]] == [r.seq_begin for r in recs], what
        _assert_rows(idx.profile_reads(data), want, what + ", host")
    lens = RP.profile(whole, s, model, 2)["n_kmers"].tolist()
    assert lens == [0, 1, 2, 150 - k + 1, 0, 6]
    idx.close()


def test_batches_do_not_change_the_rows(ctx, ctx_small_batches):
    k = 31
    rng = np.random.default_rng(31)
    genome = M.random_seq(rng, 30_000)
    a = M.fastq(M.background(rng, 300, genome=genome))
    reads = M.background(rng, 560, genome=genome) + M.adversarial_reads(rng, k) + [M.random_seq(rng, 9_000)]   # (one record larger than a batch)
    b = M.fastq([reads[i] for i in rng.permutation(len(reads))])
    assert len(b) > 40 * 4096
    idx, model, s = _index_of(ctx, a, k)
    want = RP.profile(b, s, model, 2)
    default = _profile_device(ctx, idx, b)
    _assert_rows(default, want, "default batch")
    idx2, _, _ = _index_of(ctx_small_batches, a, k)
    _assert_rows(_profile_device(ctx_small_batches, idx2, b), default, "4096-byte batches, device")
    _assert_rows(idx2.profile_reads(b), default, "4096-byte batches, host")
    _assert_rows(_profile_device(ctx_small_batches, idx2, b, shift=1), default, "4096-byte batches, odd address")
    _assert_rows(_profile_device(ctx, idx, b, shift=1), default, "odd address")
    idx.close()
    idx2.close()


def test_arguments_and_errors(ctx):
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    k = 21
    rng = np.random.default_rng(5)
    data = M.fastq(M.background(rng, 40, genome_len=3_000))
    idx, model, s = _index_of(ctx, data, k)
    want = RP.profile(data, s, model, 2)
    # capacity too small: the record count comes back, the rows that fit are written, none behind them
    with pytest.raises(L.KmiError) as e:
        _profile_device(ctx, idx, data, capacity=7)
    assert e.value.status == L.ERR_OVERFLOW and e.value.n_reads == 40
    _assert_rows(e.value.rows, want[:7], "the rows that fit")
    assert idx.profile_reads(b"").shape == (0,)
    assert idx.profile_reads_device(0, 0, 0, 0) == 0
    # an empty index answers 0 everywhere
    empty = K.CountIndex(ctx, K.make_config(k, "DNA"))
    got = empty.profile_reads(data)
    assert (got["n_kmers"] == want["n_kmers"]).all() and (got["seq_offset"] == want["seq_offset"]).all()
    assert not got["n_present"].any() and not got["sum_counts"].any() and not got["highest"].any()
    empty.close()
    for bad, word in ((data[:-30], "truncated record"), (data.replace(b"\n+\n", b"\n-\n", 1), "missing +"), (b"x" + data[1:], "missing @")):
        with pytest.raises(ValueError):
            orc.records(bad, orc.FASTQ)
        with pytest.raises(L.KmiError) as e:
            idx.profile_reads(bad)
        assert e.value.status == L.ERR_PARSE and word in str(e.value), (word, str(e.value))
        with pytest.raises(L.KmiError) as e:
            _profile_device_unchecked(ctx, idx, bad)
        assert e.value.status == L.ERR_PARSE
    with pytest.raises(L.KmiError) as e:
        idx.profile_reads(data, solid=0)
    assert e.value.status == L.ERR_INVALID
    _assert_rows(idx.profile_reads(data), want, "after the refused calls")
    idx.close()
    fa = K.CountIndex(ctx, K.make_config(k, "DNA", seq_format="fasta"))
    with pytest.raises(L.KmiError) as e:
        fa.profile_reads(data)
    assert e.value.status == L.ERR_INVALID
    fa.close()


def _profile_device_unchecked(ctx, idx, data):
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    d, o = ctx.alloc(buf.size + 64), ctx.alloc(40 * 64)
    try:
        ctx.to_device(d, buf)
        return idx.profile_reads_device(d, buf.size, o, 64)
    finally:
        ctx.free(d)
        ctx.free(o)


def test_example_program_prints_the_rows():
    """examples/read_profile: index of one FASTQ, profile of a second, one TSV line per read; and Index::lookup of a sequence's k-mers"""
    exe = os.path.join(ROOT, "examples", "read_profile")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    path = os.path.join(DATA, "test.small.fastq")
    data = open(path, "rb").read()
    seq = data[orc.records(data, orc.FASTQ)[1].seq_begin:][:30]
    seq = seq[:25] + (b"A" if seq[25:26] != b"A" else b"C") + seq[26:] + seq[:21]   # present k-mers, a substitution, a repeat
    out = subprocess.run([exe, path, path, "2", seq.decode()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    s = orc.kspec(21)
    model = M.CountModel(21)
    model.insert(orc.extract(s, data, orc.FASTQ)["kmers"])
    want = RP.profile(data, s, model, 2)
    lines = [ln for ln in out.stdout.splitlines() if ln and not ln.startswith("#")]
    got = [tuple(int(x) for x in ln.split("\t")) for ln in lines]
    assert got == [(int(r["seq_offset"]), int(r["n_kmers"]), int(r["n_present"]), int(r["n_solid"]), int(r["lowest"]), int(r["highest"]),
                    int(r["sum_counts"])) for r in want]
    looked = [ln for ln in out.stdout.splitlines() if ln.startswith("#lookup")]
    counts = RP.lookup(model, orc.kmers_from_string(s, seq))
    assert (counts > 0).any() and (counts == 0).any()
    assert len(looked) == 1 and [int(x) for x in looked[0].split("\t")[1:]] == counts.tolist()
