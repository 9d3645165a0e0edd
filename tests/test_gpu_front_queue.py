"""The one-pass FASTQ front end (kmi_front.h) with its byte ranges handed out from a queue, its EOL test by table lookup and its
pack without a validity select (kmi_front_bytes.h), against the oracle's CountMap for both strand models. Every build asserts
from the profile which front end took it.

Queue: a context made with KMI_FRONT_MIN_RANGE=4096 cuts a 1.5 MB input into a few hundred ranges; KMI_FRONT_MAX_WAVES=8 launches
the front kernel with 8 wavefronts, so every one of them takes dozens of ranges from the queue word. The same input goes through
a context without the cap (as many wavefronts as ranges or as are resident).

Pack: a lane packs its run's bytes sixteen at a time without asking whether they are bases; the bytes of the groups that lie
wholly inside the run's nb bases (nb = the read's length, for a read of one run) and, under a byte mask, the nb % 16 bytes of the
last group are compared with A C G T on the side, and a wavefront in which any lane saw another byte packs its batch of 64 runs
again with the exact routine (another byte counts as A). What lies behind a read -- EOL, '+', the quality line -- must neither
raise that flag nor reach a record."""
import os

import numpy as np
import pytest

from tests import oracle as orc

pytestmark = pytest.mark.gpu

STRANDS = {"canonical": orc.CANONICAL, "single": orc.SINGLE}


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
def ctx():
    c = _ctx_with({})
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_small_ranges():
    c = _ctx_with({"KMI_FRONT_MIN_RANGE": "4096"})
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_eight_waves():
    c = _ctx_with({"KMI_FRONT_MIN_RANGE": "4096", "KMI_FRONT_MAX_WAVES": "8"})
    yield c
    c.close()


def _rand_read(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def _pad(i, s):
    """header padding as in test_gpu_front_items: records of at least 160 bytes, and half a read's length (item capacity)"""
    return b"r%d %s" % (i, b"x" * max(150 - 2 * len(s), len(s) // 2))


def _fastq(reads, header=_pad, qual=lambda i, s: b"I" * len(s), eol=b"\n"):
    return b"".join(b"@" + header(i, s) + eol + s + eol + b"+" + eol + qual(i, s) + eol for i, s in enumerate(reads))


def _front_end_of(ctx, idx, data):
    """builds idx from data; "front" if the one-pass front end took it, "general" if it handed the input over"""
    ctx.profile(True)
    ctx.profile_reset()
    idx.build(data)
    launches = {p["name"]: p["launches"] for p in ctx.profile_get()}
    ctx.profile(False)
    assert launches.get("sk_front", 0) > 0, launches              # it is always tried
    if launches.get("fastq_scan_tiles", 0) == 0:
        assert launches.get("sk_scatter", 0) > 0, launches
        return "front"
    return "general"


def _check(ctx, k, data, expect="front", kmers=None):
    """both strand models against the oracle; `expect`: the front end that has to have taken the build"""
    import kmerind_amd as K
    s = orc.kspec(k, orc.DNA)
    if kmers is None:
        kmers = orc.extract(s, data, orc.FASTQ)["kmers"]
    for strand, model in STRANDS.items():
        idx = K.CountIndex(ctx, K.make_config(k, "DNA", strand=strand))
        took = _front_end_of(ctx, idx, data)
        print("k", k, strand, "front end:", took)
        om = orc.CountMap(s, model)
        om.insert(kmers)
        a, b = orc.sorted_pairs(*idx.to_vector()), orc.sorted_pairs(*om.export())
        idx.close()
        assert a[0].shape == b[0].shape, (k, strand)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), (k, strand)
        assert took == expect, (k, strand, took)
    return kmers


# ---------------------------------------------------------------------------------------------------------------- the queue
@pytest.fixture(scope="module")
def mixed_input():
    """1.5 MB of reads of 25 .. 300 bases (no run, one run, several runs: the ranges hold different numbers of runs), and the
    oracle's k-mers of it, extracted once per k"""
    rng = np.random.default_rng(8100)
    reads = []
    size = 0
    while size < 1_500_000:
        n = int(rng.integers(25, 301))
        reads.append(_rand_read(rng, n))
        size += 2 * n + 160
    return {"data": _fastq(reads), "kmers": {}}


@pytest.mark.parametrize("k", [31, 21])
def test_few_wavefronts_take_many_ranges_from_the_queue(ctx_eight_waves, ctx_small_ranges, mixed_input, k):
    data = mixed_input["data"]
    assert len(data) // 4096 >= 300                      # a few hundred ranges through 8 wavefronts
    kmers = _check(ctx_eight_waves, k, data, kmers=mixed_input["kmers"].get(k))
    mixed_input["kmers"][k] = kmers
    _check(ctx_small_ranges, k, data, kmers=kmers)        # the cap unset: a wavefront per range, the queue hands out nothing


# ------------------------------------------------------------------------------------------------------- the pack, the EOL test
K_PACK = [31, 21]


@pytest.mark.parametrize("k", K_PACK)
def test_read_lengths_of_every_remainder_in_one_batch(ctx, k):
    """64 reads per batch whose lengths (the run's nb = L + k - 1 bases) cycle through every remainder mod 4 and mod 16: the last
    group of a lane holds 1 .. 15 bases or none, and the bytes behind them are the EOL, '+', and a quality line made of A C G T"""
    rng = np.random.default_rng(8200 + k)
    reads = [_rand_read(rng, 96 + (i % 36)) for i in range(128)] + [_rand_read(rng, k + (i % 20)) for i in range(64)]
    _check(ctx, k, _fastq(reads, qual=lambda i, s: (b"ACGT" * 100)[i % 4:i % 4 + len(s)]))


@pytest.mark.parametrize("k", K_PACK)
def test_bytes_that_are_no_bases_take_the_exact_routine(ctx, k):
    """three batches of 64 reads: the first and the third are A C G T only, the second holds reads with an N, lower-case bases and
    a byte above 0x7F -- at a read's first base, in its middle, and in each of its last four bases (the masked last group)"""
    rng = np.random.default_rng(8300 + k)
    reads = [_rand_read(rng, 100 + (i % 7)) for i in range(192)]
    def put(i, at, b):
        r = bytearray(reads[i]); r[at] = b; reads[i] = bytes(r)
    put(64 + 3, 0, ord("N"))
    put(64 + 9, 50, ord("N"))
    for j in range(4):
        put(64 + 20 + j, len(reads[64 + 20 + j]) - 1 - j, ord("N"))
        put(64 + 30 + j, len(reads[64 + 30 + j]) - 1 - j, 0xC1)      # 'A' | 0x80
    put(64 + 40, 17, 0x80 | ord("G"))
    reads[64 + 50] = reads[64 + 50].lower()
    reads[64 + 51] = reads[64 + 51][:40] + reads[64 + 51][40:60].lower() + reads[64 + 51][60:]
    reads[64 + 63] = b"N" * 101
    _check(ctx, k, _fastq(reads))


@pytest.mark.parametrize("k", K_PACK)
def test_a_byte_that_is_no_base_right_behind_clean_reads(ctx, k):
    """reads of A C G T whose quality lines begin with 'N', '!' and bytes above 0x7F: what lies behind a run's end is not looked at"""
    rng = np.random.default_rng(8400 + k)
    reads = [_rand_read(rng, 97 + (i % 17)) for i in range(128)]
    q = [b"N", b"!", b"\xc1", b"~"]
    _check(ctx, k, _fastq(reads, qual=lambda i, s: (q[i % 4] * len(s))))


@pytest.mark.parametrize("k", K_PACK)
def test_control_bytes_in_headers_are_ordinary_bytes(ctx, k):
    """0x09, 0x0B, 0x0C (white space that is no line end) and 0x02, 0x05, 0x0E, 0x01, 0x06 (bytes that share their low bits with
    '\\n' or '\\r', or are an entry of the EOL table themselves) inside headers: a byte taken for an EOL there would cut the header
    into two lines"""
    rng = np.random.default_rng(8500 + k)
    reads = [_rand_read(rng, 100 + (i % 5)) for i in range(128)]
    ctl = [0x09, 0x0B, 0x0C, 0x02, 0x05, 0x0E, 0x01, 0x06, 0x1A, 0x1D, 0x2A, 0x8A, 0x8D]
    def header(i, s):
        c = bytes([ctl[i % len(ctl)]])
        return b"r%d %s%s%s" % (i, c, b"x" * 140, c * 3)
    _check(ctx, k, _fastq(reads, header=header))


@pytest.mark.parametrize("k", K_PACK)
def test_crlf_line_ends(ctx, k):
    rng = np.random.default_rng(8600 + k)
    reads = [_rand_read(rng, 98 + (i % 9)) for i in range(128)]
    _check(ctx, k, _fastq(reads, eol=b"\r\n"))
