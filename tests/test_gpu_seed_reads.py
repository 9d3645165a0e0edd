"""kmi_index_seed_reads_*: locate for every window of every read of a FASTQ buffer, and one row per read, against
tests/locate_model.py -- FASTA- and FASTQ-built indexes, reads shorter than k, batches, the sizing call, every capacity one short,
malformed input, agreement with locate() of the same k-mers, and the example program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import index_model as M
from tests import locate_model as LM
from tests import multimap_cases as MC
from tests import oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
GUARD = 64                              # words of a pattern behind every device buffer
PATTERN = 0xA5A5A5A5DEADBEEF
PATTERN32 = 0xDEADBEEF
K = 21


@pytest.fixture(scope="module")
def ctx():
    import kmerind_amd as K_
    c = K_.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_small_batches():
    import kmerind_amd as K_
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("KMI_PROFILE_BATCH", "4096")
        c = K_.Context(0)
    yield c
    c.close()


def seed_raw(ctx, idx, data, max_occ, cap_reads, cap_kmers, cap_hits, sizing=False, shift=0):
    """kmi_index_seed_reads_dev into device buffers of exactly the capacities, each followed by GUARD words of a pattern ->
    (status, (n_reads, n_kmers, n_hits), rows, occ, offsets, values, guards intact)"""
    from kmerind_amd import _lib as L
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    vw = idx.value_words
    h = [np.full(4 * cap_reads + GUARD, PATTERN, dtype=np.uint64),          # rows: 32 bytes each
         np.full(cap_kmers + GUARD, PATTERN32, dtype=np.uint32),
         np.full(cap_kmers + 1 + GUARD, PATTERN, dtype=np.uint64),
         np.full(cap_hits * vw + GUARD, PATTERN, dtype=np.uint64)]
    d_in = ctx.alloc(buf.size + 64 + shift)
    d = [ctx.alloc(a.nbytes) for a in h]
    try:
        ctx.to_device(d_in, np.concatenate([np.zeros(shift, dtype=np.uint8), buf]))
        for p, a in zip(d, h):
            ctx.to_device(p, a)
        nr, nk, nh = C.c_uint64(1), C.c_uint64(2), C.c_uint64(3)
        ptrs = [None] * 4 if sizing else [C.c_void_p(p) for p in d]
        st = L.lib.kmi_index_seed_reads_dev(idx.h, C.c_void_p(d_in + shift), buf.size, max_occ, ptrs[0], 0 if sizing else cap_reads, ptrs[1],
                                            ptrs[2], 0 if sizing else cap_kmers, ptrs[3], 0 if sizing else cap_hits, C.byref(nr), C.byref(nk),
                                            C.byref(nh))
        for p, a in zip(d, h):
            ctx.to_host(a, p)
    finally:
        ctx.free(d_in)
        for p in d:
            ctx.free(p)
    intact = bool((h[0][4 * cap_reads:] == np.uint64(PATTERN)).all() and (h[1][cap_kmers:] == PATTERN32).all() and
                  (h[2][cap_kmers + 1:] == np.uint64(PATTERN)).all() and (h[3][cap_hits * vw:] == np.uint64(PATTERN)).all())
    if sizing:
        intact = intact and all((a == a[-1]).all() for a in h)
    return (st, (nr.value, nk.value, nh.value), h[0][:4 * cap_reads].view(LM.ROW), h[1][:cap_kmers], h[2][:cap_kmers + 1],
            h[3][:cap_hits * vw].reshape(cap_hits, vw), intact)


def seed_device(ctx, idx, data, max_occ=LM.LOCATE_ALL, shift=0):
    """the sizing call, then the call into buffers of exactly the sizes it gave"""
    from kmerind_amd import _lib as L
    st, totals, *_, intact = seed_raw(ctx, idx, data, max_occ, 0, 0, 0, sizing=True, shift=shift)
    assert st == L.OK and intact
    st, totals2, rows, occ, off, values, intact = seed_raw(ctx, idx, data, max_occ, *totals, shift=shift)
    assert st == L.OK and intact and totals2 == totals
    return rows, occ, off, values


def assert_seeds(got, want, where):
    d = LM.first_row_difference(got[0], want[0]) or LM.difference(got[1:], want[1:])
    assert d is None, "%s: %s" % (where, d)


def reference_and_reads(which):
    """(reference bytes, its format, reads as FASTQ): the golden files, or the 3000-base genome of multimap_cases in FASTA records
    that overlap by 60 bases (so some keys are stored twice) / as FASTQ reads, with reads of both strands, three reads shorter than
    k and five random reads the reference does not hold"""
    rng = np.random.default_rng(len(which))
    if which.startswith("natural"):
        reads = open(os.path.join(DATA, "natural.fastq"), "rb").read()
        if which == "natural-fasta":
            return open(os.path.join(DATA, "natural.fasta"), "rb").read(), "fasta", reads
        return reads, "fastq", reads
    reads = MC.fastq(rng, MC.reads(rng, 120, K) + [M.random_seq(rng, 100) for _ in range(5)])
    if which == "genome-fasta":
        return MC.fasta([MC.GENOME[i:i + 560] for i in range(0, len(MC.GENOME), 500)]), "fasta", reads
    return MC.fastq(rng, MC.reads(rng, 100, K), tag=b"ref"), "fastq", reads


def index_of(ctx, ref, fmt, kind="position", k=K):
    import kmerind_amd as K_
    s = orc.kspec(k, orc.DNA)
    idx = K_.PositionIndex(ctx, K_.make_config(k, "DNA", strand="canonical", index_kind=kind, seq_format=fmt))
    idx.build(ref)
    model = LM.LocateModel(s, orc.CANONICAL, MC.VW[kind])
    model.build(ref, orc.FASTQ if fmt == "fastq" else orc.FASTA)
    assert idx.local_size() == model.size() > 0
    return idx, model


@pytest.mark.parametrize("which", ["natural-fasta", "natural-fastq", "genome-fasta", "genome-fastq"])
def test_seed_reads_matches_the_model(ctx, which):
    ref, fmt, reads = reference_and_reads(which)
    idx, model = index_of(ctx, ref, fmt)
    want = model.seed_reads(reads)
    assert int(want[2][-1]) > 0
    if which.startswith("genome"):
        assert int((want[0]["n_kmers"] == 0).sum()) == 3              # the reads shorter than k have their rows
        assert int((want[1] == 0).sum()) >= 5 * (100 - K + 1)         # and the random reads' windows are absent
    assert_seeds(seed_device(ctx, idx, reads), want, "device form")
    assert_seeds(seed_device(ctx, idx, reads, shift=3), want, "device form, unaligned bytes")
    assert_seeds(idx.seed_reads(reads), want, "host form")
    cap = int(np.median(want[1][want[1] > 0]))
    capped = model.seed_reads(reads, cap)
    assert 0 < int(capped[2][-1]) < int(want[2][-1]) and int((capped[1] == cap).sum()) > 0
    assert_seeds(seed_device(ctx, idx, reads, cap), capped, "device form, max_occ %d" % cap)
    assert_seeds(idx.seed_reads(reads, cap), capped, "host form, max_occ %d" % cap)
    idx.close()


def test_seed_reads_against_a_position_quality_index(ctx):
    ref, fmt, reads = reference_and_reads("genome-fastq")
    idx, model = index_of(ctx, ref, fmt, kind="posqual")
    want = model.seed_reads(reads)
    assert_seeds(seed_device(ctx, idx, reads), want, "device form")
    assert_seeds(idx.seed_reads(reads), want, "host form")
    idx.close()


def test_batches_do_not_change_the_arrays(ctx, ctx_small_batches):
    ref, fmt, reads = reference_and_reads("genome-fasta")
    assert len(reads) > 3 * 4096
    got = []
    for c in (ctx, ctx_small_batches):
        idx, model = index_of(c, ref, fmt)
        got.append((seed_device(c, idx, reads, 4), idx.seed_reads(reads, 4)))
        idx.close()
    want = model.seed_reads(reads, 4)
    for (dev, host), where in zip(got, ("one batch", "batches of 4096 bytes")):
        assert_seeds(dev, want, where + ", device form")
        assert_seeds(host, want, where + ", host form")
    for a, b in zip(got[0][0][:3], got[1][0][:3]):
        assert (a == b).all()


def test_sizing_call_and_short_capacities(ctx, ctx_small_batches):
    from kmerind_amd import _lib as L
    ref, fmt, reads = reference_and_reads("genome-fasta")
    for c in (ctx, ctx_small_batches):
        idx, model = index_of(c, ref, fmt)
        want = model.seed_reads(reads)
        totals = (want[0].shape[0], want[1].shape[0], int(want[2][-1]))
        st, got, *_, intact = seed_raw(c, idx, reads, LM.LOCATE_ALL, 0, 0, 0, sizing=True)
        assert st == L.OK and got == totals and intact
        for short in range(3):
            caps = [t - (i == short) for i, t in enumerate(totals)]
            st, got, *_, intact = seed_raw(c, idx, reads, LM.LOCATE_ALL, *caps)
            assert st == L.ERR_OVERFLOW and got == totals, "capacity %d one short" % short
            assert intact, "capacity %d one short: written past a capacity" % short
        st, got, rows, occ, off, values, intact = seed_raw(c, idx, reads, LM.LOCATE_ALL, *totals)
        assert st == L.OK and got == totals and intact
        assert_seeds((rows, occ, off, values), want, "exact capacities")
        # max_occ = 0, and a count index
        st, *_ = seed_raw(c, idx, reads, 0, *totals)
        assert st == L.ERR_INVALID
        idx.close()


def test_count_index_and_malformed_input(ctx):
    import kmerind_amd as K_
    from kmerind_amd import _lib as L
    ref, fmt, reads = reference_and_reads("genome-fastq")
    cidx = K_.CountIndex(ctx, K_.make_config(K, "DNA", strand="canonical"))
    cidx.build(ref)
    cidx.value_words = 1
    st, *_ = seed_raw(ctx, cidx, reads, LM.LOCATE_ALL, 1000, 1000, 1000)
    assert st == L.ERR_INVALID
    cidx.close()
    idx, model = index_of(ctx, ref, fmt)
    bad = reads[:2000] + b"@broken\nACGTACGTACGTACGTACGTACGTACGT\n+\nIIII\n" + reads[:400]
    with pytest.raises(L.KmiError) as e:
        idx.seed_reads(bad)
    assert e.value.status == L.ERR_PARSE
    st, *_ = seed_raw(ctx, idx, bad, LM.LOCATE_ALL, 1000, 100000, 1000000)
    assert st == L.ERR_PARSE
    # no bytes at all
    rows, occ, off, values = idx.seed_reads(b"")
    assert rows.shape == (0,) and occ.shape == (0,) and off.tolist() == [0] and values.shape == (0, 1)
    assert_seeds(idx.seed_reads(reads), model.seed_reads(reads), "after the refused calls")
    idx.close()


def test_seed_reads_is_locate_of_the_reads_kmers(ctx):
    import kmerind_amd as K_
    ref, fmt, reads = reference_and_reads("natural-fasta")
    idx, _ = index_of(ctx, ref, fmt)
    kmers, n_seqs = ctx.read_file(K_.make_config(K, "DNA", strand="canonical"), reads)
    for max_occ in (None, 3):
        rows, occ, off, values = idx.seed_reads(reads, max_occ)
        occ2, off2, values2 = idx.locate(kmers, max_occ)
        assert rows.shape[0] == n_seqs and int(rows["n_kmers"].sum()) == kmers.shape[0] == occ.shape[0]
        assert (occ == occ2).all() and (off == off2).all()
        per_query = [sorted(tuple(r) for r in values2[int(off2[i]):int(off2[i + 1])].tolist()) for i in range(occ2.shape[0])]
        assert LM.values_difference(values, off, per_query) is None
        assert (rows["first_kmer"] == np.concatenate([[0], np.cumsum(rows["n_kmers"])[:-1]]).astype(np.uint64)).all()
        assert (rows["n_hits"] == off[(rows["first_kmer"] + rows["n_kmers"]).astype(np.int64)] - off[rows["first_kmer"].astype(np.int64)]).all()
    idx.close()


@pytest.mark.parametrize("ref_name,max_occ", [("test.fasta", None), ("natural.fasta", None), ("natural.fasta", 1)])
def test_example_program_prints_the_rows(ref_name, max_occ):
    """examples/seed_reads: a position index of a FASTA file, the seeds of a FASTQ file, one TSV line per read"""
    exe = os.path.join(ROOT, "examples", "seed_reads")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    ref, reads = os.path.join(DATA, ref_name), os.path.join(DATA, "natural.fastq")
    out = subprocess.run([exe, ref, reads] + ([str(max_occ)] if max_occ else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    model = LM.LocateModel(orc.kspec(K, orc.DNA), orc.CANONICAL)
    model.build(open(ref, "rb").read(), orc.FASTA)
    rows, occ, off, _ = model.seed_reads(open(reads, "rb").read(), LM.LOCATE_ALL if max_occ is None else max_occ)
    assert lines[0] == "#seq_offset\tn_kmers\tn_listed\tn_hits"
    assert [tuple(int(x) for x in ln.split("\t")) for ln in lines[1:-1]] == \
        [(int(r["seq_offset"]), int(r["n_kmers"]), int(r["n_listed"]), int(r["n_hits"])) for r in rows]
    assert lines[-1] == "#total\t%d\t%d\t%d" % (rows.shape[0], occ.shape[0], int(off[-1]))
