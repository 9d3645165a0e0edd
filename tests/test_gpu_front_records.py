"""The line phase of the one-pass FASTQ front end (kmi_front.h): a line pass takes one RECORD per lane -- the two marker bytes, the
length rule, the runs -- and runs when 64 complete records wait or the range ends; the ring keeps line ENDS alone for a text whose
EOL bytes all stand alone (LF), and (start, end) pairs for any other, the range beginning again as soon as it meets one.

Every build is compared with the oracle's CountMap, and the profile says which front end took it. An input the path must decline
is built a second time in a context made with KMI_FRONT=general, and the two outcomes (index, or error) must be the same.

Ranges: a context made with KMI_FRONT_MIN_RANGE=4096 cuts the input into ranges of one 4 KB step, so records, '+' lines and quality
ends fall on range boundaries at every offset; the default context keeps an input below 64 KB in one range."""
import os

import numpy as np
import pytest

from tests import oracle as orc

pytestmark = pytest.mark.gpu


def _ctx_with(env):
    """a context made under these environment settings (they are read when the context is made)"""
    import kmerind_amd as K
    old = {n: os.environ.get(n) for n in env}
    os.environ.update(env)
    try:
        return K.Context(0)
    finally:
        for n, v in old.items():
            if v is None:
                del os.environ[n]
            else:
                os.environ[n] = v


@pytest.fixture(scope="module")
def contexts():
    made = {"one-range": _ctx_with({}), "4k-ranges": _ctx_with({"KMI_FRONT_MIN_RANGE": "4096"}),
            "general": _ctx_with({"KMI_FRONT": "general"})}
    yield made
    for c in made.values():
        c.close()


def _rand_read(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def _header(i, s):
    """at least 160 bytes per record (a step keeps 128 lines), half a read's length (item capacity), and a length that walks
    through every remainder mod 64 from record to record"""
    return b"r%d %s" % (i, b"x" * (max(150 - 2 * len(s), len(s) // 2) + (i * 37) % 64))


def _fastq(reads, header=_header, qual=lambda i, s: b"I" * len(s), eol=b"\n", plus=lambda i: b"+"):
    return b"".join(b"@" + header(i, s) + eol + s + eol + plus(i) + eol + qual(i, s) + eol for i, s in enumerate(reads))


def _outcome(ctx, k, data, strand="canonical"):
    """(front end that took the build, ("ok", keys, counts) or ("error", text))"""
    import kmerind_amd as K
    from kmerind_amd._lib import KmiError
    idx = K.CountIndex(ctx, K.make_config(k, "DNA", strand=strand))
    ctx.profile(True)
    ctx.profile_reset()
    try:
        idx.build(data)
        res = ("ok",) + tuple(orc.sorted_pairs(*idx.to_vector()))
    except KmiError as e:
        res = ("error", str(e))
    launches = {p["name"]: p["launches"] for p in ctx.profile_get()}
    ctx.profile(False)
    idx.close()
    if launches.get("sk_front", 0) == 0:
        took = "none"
    else:
        took = "front" if launches.get("fastq_scan_tiles", 0) == 0 and launches.get("sk_scatter", 0) > 0 else "general"
    return took, res


def _same(a, b):
    if a[0] != b[0]:
        return False
    if a[0] == "error":
        return a[1] == b[1]
    return a[1].shape == b[1].shape and bool((a[1] == b[1]).all()) and bool((a[2] == b[2]).all())


def _oracle(k, data, model=orc.CANONICAL):
    s = orc.kspec(k, orc.DNA)
    om = orc.CountMap(s, model)
    om.insert(orc.extract(s, data, orc.FASTQ)["kmers"])
    return ("ok",) + tuple(orc.sorted_pairs(*om.export()))


def _check(ctx, k, data, what="", expected=None):
    """the one-pass front end took the build, and the index is the oracle's"""
    took, got = _outcome(ctx, k, data)
    print(what, "k", k, len(data), "bytes: front end", took, got[0])
    assert took == "front", (what, k, took)
    if expected is None:
        expected = _oracle(k, data)
    assert _same(got, expected), (what, k)
    return expected


LENGTHS = [31, 32, 63, 64, 65, 150, 251]


# ------------------------------------------------------------------------------------------------------------------ read lengths
@pytest.mark.parametrize("ranges", ["one-range", "4k-ranges"])
@pytest.mark.parametrize("k", [17, 21, 28, 31])
def test_ragged_read_lengths(contexts, k, ranges):
    """600 reads whose lengths cycle through 31 .. 251 out of step with the lanes (a read shorter than k yields no run, one of
    251 bases two runs and more), headers of every length mod 64: several line passes of 64 records and a last, partial one"""
    rng = np.random.default_rng(1200 + k)
    n = 160 if ranges == "one-range" else 600       # (one range: below 64 KB)
    reads = [_rand_read(rng, LENGTHS[(i * 3 + i // 7) % 7]) for i in range(n)]
    data = _fastq(reads)
    assert ranges != "one-range" or len(data) < 65536
    _check(contexts[ranges], k, data, "ragged " + ranges)


@pytest.mark.parametrize("ranges", ["one-range", "4k-ranges"])
def test_every_read_length_alone(contexts, ranges):
    """130 reads of one length per file: two full passes and one of two records"""
    rng = np.random.default_rng(1300)
    for n in LENGTHS:
        _check(contexts[ranges], 31, _fastq([_rand_read(rng, n) for _ in range(130)]), "length %d" % n)


# ------------------------------------------------------------------------------------------- how many records a range holds
@pytest.mark.parametrize("n_records", [1, 2, 63, 64, 65, 127, 128, 129])
def test_records_in_one_range(contexts, n_records):
    """the edges of the full-wavefront pass: one range (the file is below 64 KB) of exactly this many records"""
    rng = np.random.default_rng(1400 + n_records)
    data = _fastq([_rand_read(rng, 100 + (i % 30)) for i in range(n_records)])
    assert len(data) < 65536
    _check(contexts["one-range"], 31, data, "%d records" % n_records)
    _check(contexts["one-range"], 31, data[:-1], "%d records, no final newline" % n_records)


def test_ranges_without_a_line_and_with_one_record(contexts):
    """records of about 9 KB (a header of 5000 bytes, a read of 2000 bases) under ranges of 4 KB: a range lies inside a header or
    a read and owns no line, or owns a '+' line and a quality line, or one whole record's lines"""
    rng = np.random.default_rng(1500)
    reads = [_rand_read(rng, 2000 + 3 * i) for i in range(40)]
    data = _fastq(reads, header=lambda i, s: b"r%d %s" % (i, b"x" * (5000 + 61 * i)))
    _check(contexts["4k-ranges"], 31, data, "long records")
    # and records of just under 4 KB: most ranges own one record's '@' line
    reads = [_rand_read(rng, 1200 + (i % 5)) for i in range(60)]
    data = _fastq(reads, header=lambda i, s: b"r%d %s" % (i, b"x" * (1600 + (i * 13) % 64)))
    _check(contexts["4k-ranges"], 31, data, "one record per range")


@pytest.mark.parametrize("k", [21, 31])
def test_record_parts_at_every_offset_of_a_step(contexts, k):
    """records of 256 + d bytes, d = 0 .. 63 in turn: record starts, '+' lines and quality ends walk through every offset mod 64,
    across the 4096-byte steps and the range boundaries of both contexts"""
    rng = np.random.default_rng(1600 + k)
    reads = [_rand_read(rng, 70) for _ in range(520)]
    data = _fastq(reads, header=lambda i, s: b"r%04d %s" % (i, b"x" * (104 + i % 64)))
    exp = _check(contexts["4k-ranges"], k, data, "offsets")
    _check(contexts["one-range"], k, data, "offsets", exp)


# -------------------------------------------------------------------------------------------------------------------- line ends
@pytest.mark.parametrize("ranges", ["one-range", "4k-ranges"])
def test_line_end_forms(contexts, ranges):
    rng = np.random.default_rng(1700)
    reads = [_rand_read(rng, LENGTHS[i % 7]) for i in range(330)]
    ctx = contexts[ranges]
    lf = _fastq(reads)
    exp = _check(ctx, 31, lf, "LF")
    _check(ctx, 31, lf[:-1], "LF, no final newline", exp)
    _check(ctx, 31, lf + b"\n\n", "LF, blank lines behind the last record", exp)
    crlf = _fastq(reads, eol=b"\r\n")
    _check(ctx, 31, crlf, "CRLF", exp)
    _check(ctx, 31, crlf[:-2], "CRLF, no final newline", exp)
    # LF records, then CRLF records: a range that has queued and walked batches of runs begins again with (start, end) pairs
    mixed = _fastq(reads[:200]) + _fastq(reads[200:], eol=b"\r\n", header=lambda i, s: _header(i + 200, s))
    _check(ctx, 31, mixed, "LF then CRLF", exp)
    # a '+' line that repeats the header
    _check(ctx, 31, _fastq(reads, plus=lambda i: b"+r%d" % i), "'+' lines with text", exp)


def test_a_last_record_cut_short(contexts):
    """the file ends inside its last record (behind the sequence line, inside the quality line): whatever the general front end
    makes of it, the default build makes the same"""
    rng = np.random.default_rng(1800)
    reads = [_rand_read(rng, 100 + i % 9) for i in range(150)]
    whole = _fastq(reads)
    last = len(_fastq(reads[:-1]))
    for cut in (last + len(_header(149, reads[149])) + 2 + len(reads[149]) + 1, len(whole) - 40):
        data = whole[:cut]
        for ranges in ("one-range", "4k-ranges"):
            took, got = _outcome(contexts[ranges], 31, data)
            _, ref = _outcome(contexts["general"], 31, data)
            print("cut at", cut - last, ranges, "front end", took, got[0], ref[0])
            assert _same(got, ref), (cut, ranges, got[:2], ref[:2])


# ------------------------------------------------------------------------------------------------- inputs the path must decline
def _declined_inputs():
    rng = np.random.default_rng(1900)
    reads = [_rand_read(rng, 100 + i % 11) for i in range(200)]
    lines = _fastq(reads).split(b"\n")           # 800 lines and a last empty string
    def edit(at, fn, also=None):
        out = list(lines)
        out[at] = fn(out[at])
        if also is not None:
            out[also] = fn(out[also])
        return b"\n".join(out)
    cases = {
        "a header without its '@'": edit(4 * 130, lambda s: b">" + s[1:]),
        "a '+' line without its '+'": edit(4 * 70 + 2, lambda s: b"-"),
        "a quality line one short": edit(4 * 90 + 3, lambda s: s[:-1]),
        "a quality line one long": edit(4 * 190 + 3, lambda s: s + b"I"),
        "an empty sequence and quality line": edit(4 * 100 + 1, lambda s: b"", also=4 * 100 + 3),
        "lines of a few bytes": _fastq(reads) + b"@a\nAC\n+\nII\n" * 300,
    }
    return cases


@pytest.mark.parametrize("ranges", ["one-range", "4k-ranges"])
def test_declined_inputs_go_to_the_general_front_end(contexts, ranges):
    for what, data in _declined_inputs().items():
        took, got = _outcome(contexts[ranges], 31, data)
        _, ref = _outcome(contexts["general"], 31, data)
        print(what, ranges, "front end", took, got[0], ref[0])
        assert took == "general", (what, ranges, took)
        assert _same(got, ref), (what, ranges, got[:2], ref[:2])


def test_an_ambiguous_first_line_goes_to_the_general_front_end(contexts):
    """quality lines that begin with '@' beside '+' lines, and a sequence line that begins with '+' (a byte that is no base counts
    as A): among a range's first six lines two can be taken for a header, and the range does not guess"""
    rng = np.random.default_rng(2000)
    reads = [b"+" + _rand_read(rng, 99) for _ in range(200)]
    data = _fastq(reads, qual=lambda i, s: b"@" + b"I" * (len(s) - 1))
    took, got = _outcome(contexts["4k-ranges"], 31, data)
    _, ref = _outcome(contexts["general"], 31, data)
    print("ambiguous: front end", took, got[0], ref[0])
    assert took == "general", took
    assert _same(got, ref)
    # in one range nothing is inferred: the file begins with '@'
    one = _fastq(reads[:100], qual=lambda i, s: b"@" + b"I" * (len(s) - 1))
    assert len(one) < 65536
    _check(contexts["one-range"], 31, one, "'@'-led quality lines in one range")


def test_blank_lines_between_records(contexts):
    """a blank line is no line (a line is a run of bytes that are no EOL): the records keep their roles, and the ring keeps pairs"""
    rng = np.random.default_rng(2100)
    reads = [_rand_read(rng, 100 + i % 13) for i in range(300)]
    recs = [_fastq([s], header=lambda _, s, i=i: _header(i, s)) for i, s in enumerate(reads)]
    data = b"".join(r + (b"\n" if i % 50 == 49 else b"") for i, r in enumerate(recs))
    for ranges in ("one-range", "4k-ranges"):
        took, got = _outcome(contexts[ranges], 31, data)
        _, ref = _outcome(contexts["general"], 31, data)
        print("blank lines", ranges, "front end", took, got[0], ref[0])
        assert _same(got, ref), ranges


# ----------------------------------------------------------------------------------------------------------- de Bruijn edge records
def test_edge_records_of_a_small_input(contexts):
    """sk_front_kernel<W, true>: the node map of 300 ragged reads (both contexts), against the oracle's"""
    import kmerind_amd as K
    rng = np.random.default_rng(2200)
    reads = [_rand_read(rng, LENGTHS[(i * 5 + i // 3) % 7]) for i in range(300)]
    data = _fastq(reads)
    k = 31
    s = orc.kspec(k)
    om = orc.DbgMap(s)
    om.insert(*orc.dbg_parse(s, data))
    ek, ec = om.export(canonical=True)
    exp = orc.sorted_rows(ek, ec.astype(np.uint64))
    for ranges in ("one-range", "4k-ranges"):
        c = contexts[ranges]
        g = K.DeBruijnNodes(c, K.make_config(k))
        c.profile(True)
        c.profile_reset()
        g.build(data)
        names = {p["name"] for p in c.profile_get() if p["launches"]}
        c.profile(False)
        gk, gc = g.to_vector()
        g.close()
        assert {"sk_front", "sk_reduce", "sk_edges_accumulate"} <= names and "dbg_accumulate" not in names, (ranges, names)
        got = orc.sorted_rows(gk, gc.astype(np.uint64))
        assert got.shape == exp.shape and bool((got == exp).all()), ranges
