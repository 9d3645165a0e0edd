"""The item pass of the one-pass FASTQ front end (kmi_front.h: entries -> items, one forward pass, and the top-down tail for
super-k-mers longer than nmax windows) and the record assembly of its scatter pass (sk_assemble_row), against the oracle's
CountMap. Every build here must have been taken by the one-pass front end: a build that went to the general path tests nothing
of this and fails.

k = 17, 21, 28, 31, 32 are the minimizer shapes W = 7, 11, 13, 19, 19 with nmax = 32, 31, 24, 21, 20 windows per item. An all-A
(or all-T) m-mer has the smallest order hash there is (its canonical form is 0), so every window that holds one has the same
minimizer: a stretch of S such bases inside a read makes one super-k-mer of S - m + W windows, at a read's first or last base
one of S - m + 1 (m = k - W + 1)."""
import numpy as np
import pytest

from tests import oracle as orc

pytestmark = pytest.mark.gpu

KS = [17, 21, 28, 31, 32]
W_OF = {17: 7, 21: 11, 28: 13, 31: 19, 32: 19}
NMAX = {17: 32, 21: 31, 28: 24, 31: 21, 32: 20}
STRANDS = {"canonical": orc.CANONICAL, "single": orc.SINGLE}
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def ctx():
    import kmerind_amd as K
    c = K.Context(0)
    yield c
    c.close()


def _rand_read(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def _fastq(reads):
    """The header is padded: to records of at least 160 bytes (the one-pass front end keeps 128 line starts per 4 KB step and hands
    a text of shorter lines to the general path), and by half a read's length (a byte range has room for one item per 8 bytes; W = 7
    makes one per four bases)."""
    return b"".join(b"@r%d %s\n%s\n+\n%s\n" % (i, b"x" * max(150 - 2 * len(s), len(s) // 2), s, b"I" * len(s)) for i, s in enumerate(reads))


def _build_checked(ctx, k, strand, data):
    """the count index of `data`, built by the one-pass front end (asserted from the profile)"""
    import kmerind_amd as K
    idx = K.CountIndex(ctx, K.make_config(k, "DNA", strand=strand))
    ctx.profile(True)
    ctx.profile_reset()
    idx.build(data)
    launches = {p["name"]: p["launches"] for p in ctx.profile_get()}
    ctx.profile(False)
    assert launches.get("sk_front", 0) > 0 and launches.get("sk_scatter", 0) > 0, launches
    assert launches.get("fastq_scan_tiles", 0) == 0, launches
    return idx


def _check(ctx, k, reads):
    """both strand models against the oracle (one extraction); returns the canonical build's sorted (keys, counts)"""
    data = _fastq(reads)
    s = orc.kspec(k, orc.DNA)
    kmers = orc.extract(s, data, orc.FASTQ)["kmers"]
    got = None
    for strand, model in STRANDS.items():
        idx = _build_checked(ctx, k, strand, data)
        om = orc.CountMap(s, model)
        om.insert(kmers)
        a, b = orc.sorted_pairs(*idx.to_vector()), orc.sorted_pairs(*om.export())
        idx.close()
        assert a[0].shape == b[0].shape, (k, strand)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), (k, strand)
        if strand == "canonical":
            got = a
    return got


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_read_length_sweep(ctx, k, half):
    """128 reads (two batches of 64 lanes) at each length from k - 1 to k + 2 W + 2: no window, one window, and every fill of the
    walk's last block, so the entries behind a lane's last window (w0 >= L) come in every number. Lower and upper half of the
    lengths are a file each."""
    rng = np.random.default_rng(7000 + k)
    lengths = list(range(k - 1, k + 2 * W_OF[k] + 3))
    cut = len(lengths) // 2
    reads = [_rand_read(rng, n) for n in (lengths[:cut], lengths[cut:])[half] for _ in range(128)]
    _check(ctx, k, reads)


@pytest.mark.parametrize("k", KS)
def test_reads_of_150_and_300_bases(ctx, k):
    """a 300-base read is several runs (a run is cut every sk_segment_of(W) windows), a 150-base one is too for W < 19"""
    rng = np.random.default_rng(7100 + k)
    _check(ctx, k, [_rand_read(rng, 150) for _ in range(128)] + [_rand_read(rng, 300) for _ in range(128)])


@pytest.mark.parametrize("k", KS)
def test_reads_of_one_repeated_base(ctx, k):
    """every run is ONE super-k-mer: ceil(windows / nmax) items from one entry, in all 64 lanes"""
    _check(ctx, k, [b"ACGT"[i % 4:i % 4 + 1] * (100 + i) for i in range(64)])


@pytest.mark.parametrize("k", KS)
def test_reads_of_an_eight_base_repeat(ctx, k):
    """the m-mers repeat every eight positions, so every window of a run has the same minimizer hash"""
    rng = np.random.default_rng(7200 + k)
    _check(ctx, k, [(_rand_read(rng, 8) * 20)[:150 - (i % 9)] for i in range(64)])


@pytest.mark.parametrize("k", KS)
def test_one_long_lane_among_ordinary_ones(ctx, k):
    """three batches of 64 single-run reads (k + 40 bases: 41 windows, more than nmax and fewer than a run's segment), the poly-A
    read in lane 0 of the first, lane 31 of the second and lane 63 of the third: the forward loop leaves at entry 0 for the whole
    batch, and 63 lanes go through the tail with ordinary entries"""
    rng = np.random.default_rng(7300 + k)
    reads = [_rand_read(rng, k + 40) for _ in range(192)]
    for at in (0, 64 + 31, 128 + 63):
        reads[at] = b"A" * (k + 40)
    _check(ctx, k, reads)


@pytest.mark.parametrize("where", ["start", "middle", "end"])
@pytest.mark.parametrize("k", KS)
def test_poly_a_stretch_inside_ordinary_reads(ctx, k, where):
    """150-base reads that carry a poly-A stretch at their start, in their middle or at their end, between ordinary reads: of
    nmax + 5 bases, and of nmax + m + 4 bases, which is a super-k-mer of more than nmax windows also where the read begins or
    ends with it. The forward loop then leaves at a first, a middle or a last entry and the tail starts there."""
    rng = np.random.default_rng(7400 + k)
    m = k - W_OF[k] + 1
    reads = []
    for i in range(192):
        r = _rand_read(rng, 150)
        if i % 5 == 2:
            s = NMAX[k] + 5 if i % 2 else NMAX[k] + m + 4
            at = {"start": 0, "middle": 40 + i % 30, "end": 150 - s}[where]
            r = r[:at] + b"A" * s + r[at + s:]
        reads.append(r)
    _check(ctx, k, reads)


@pytest.mark.parametrize("k", KS)
def test_reads_and_their_reverse_complements(ctx, k):
    """the same reads and their reverse complements in one file: every canonical count doubles and the keys stay (the record of a
    super-k-mer and of its mirror image is the same one, whichever of the two sk_assemble_row was given)"""
    rng = np.random.default_rng(7500 + k)
    reads = [_rand_read(rng, int(n)) for n in rng.integers(k, 200, size=300)]
    reads += [b"A" * 120, b"ACCGGTTA" * 15]
    once = _check(ctx, k, reads)
    both = _check(ctx, k, reads + [r.translate(_COMP)[::-1] for r in reads])
    assert once[0].shape == both[0].shape and (once[0] == both[0]).all()
    assert (both[1] == 2 * once[1]).all()
