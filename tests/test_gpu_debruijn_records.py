"""The de Bruijn node build through super-k-mer EDGE records -- sk_front_kernel<W, true>, the `edges` branch of sk_scatter and
sk_edges_accumulate_kernel (kmi_debruijn.h) -- on the inputs where records go wrong: reads of one base, tandem repeats with k-mers
that equal their reverse complement, read lengths around the run cuts, one-base stretches cut into maximal pieces, reads with
their reverse complements, the last reads of the buffer, and one fine bucket of several table chunks. Every build is a
DeBruijnNodes.build of FASTQ bytes into an empty graph and goes through _check: the build took the edge-record path (a build that
went to the tuple path tests nothing of this and fails), its nodes are the oracle's DbgMap node for node and counter for counter,
and two sums hold that need no oracle.

The constants per k, from the rules of the code:
  W    = sk_window_of(k): 7 for k = 17 .. 20, 11 for 21 and 22, 13 for 23 .. 28, 19 for 29 .. 32 (m = k - W + 1)
  NMAX = sk_nmax_of(k) - kSkEdgeWindows = min(52 - k, 32) - 3 windows (k-mers) per edge record: 29 at k <= 20 (48 bases), 17 at k = 32
  SEG  = FrCfg<W>::SEG: a read is cut into runs of 44, 64, 80, 127 windows for W = 7, 11, 13, 19
An all-A (or all-T) m-mer has the smallest order hash there is, so a stretch of one base is one super-k-mer, cut into pieces of
NMAX windows; sk_edges_accumulate walks a record in units of two k-mers: 15 units for a record of 29."""
import functools

import numpy as np
import pytest

from tests import oracle as orc
from tests import unitig_model as M
from tests.test_gpu_front_items import _COMP, _fastq, _rand_read
from tests.test_gpu_reduce_records import _crowd

pytestmark = pytest.mark.gpu

KS = [17, 20, 21, 22, 28, 29, 31, 32]
W_OF = {17: 7, 20: 7, 21: 11, 22: 11, 28: 13, 29: 19, 31: 19, 32: 19}
NMAX = {17: 29, 20: 29, 21: 28, 22: 27, 28: 21, 29: 20, 31: 18, 32: 17}
SEG = {7: 44, 11: 64, 13: 80, 19: 127}
ROWS = 4608                 # DbgCfg<1>::ROWS: nodes per table fill of sk_edges_accumulate
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def test_constants_restate_the_rules():
    for k in KS:
        assert W_OF[k] == (19 if k >= 29 else 13 if k >= 23 else 11 if k >= 21 else 7)
        assert NMAX[k] == min(52 - k, 32) - 3 and k + NMAX[k] - 1 <= 48
    assert NMAX[20] == 29 and (NMAX[20] + 1) // 2 == 15


@pytest.fixture(scope="module")
def ctx():
    import kmerind_amd as K
    c = K.Context(0)
    yield c
    c.close()


def _nodes(keys, counts):
    return orc.sorted_rows(keys, counts.astype(np.uint64))


def _revcomp(r):
    return r.translate(_COMP)[::-1]


@functools.lru_cache(maxsize=None)
def _oracle(k, data):
    """the oracle's node map of FASTQ bytes, sorted rows (key, out A C G T, in A C G T, occurrences); computed once per input"""
    s = orc.kspec(k)
    om = orc.DbgMap(s)
    om.insert(*orc.dbg_parse(s, data))
    rows = _nodes(*om.export(canonical=True))
    rows.setflags(write=False)
    return rows


def _assert_sums(rows, k, data, what):
    """occurrences sum to the k-mers of the input; every k-mer has two neighbours but the first and the last of its read"""
    lengths = [len(s) for s in data.split(b"\n")[1::4]]
    n_kmers = sum(n - k + 1 for n in lengths if n >= k)
    n_reads = sum(1 for n in lengths if n >= k)
    assert int(rows[:, 9].sum()) == n_kmers, (what, k)
    assert int(rows[:, 1:9].sum()) == 2 * (n_kmers - n_reads), (what, k)


def _check(c, k, data, what="", keep=False):
    """build `data` into an empty graph in context c: the path, the oracle's map, the two sums. Returns the graph's sorted rows
    (and the graph, if it is to be kept)."""
    import kmerind_amd as K
    data = bytes(data)
    g = K.DeBruijnNodes(c, K.make_config(k))
    c.profile(True)
    c.profile_reset()
    g.build(data)
    names = {p["name"] for p in c.profile_get() if p["launches"]}
    c.profile(False)
    assert {"sk_front", "sk_reduce", "sk_edges_accumulate"} <= names and "dbg_accumulate" not in names, (what, k, names)
    exp = _oracle(k, data)
    _assert_sums(exp, k, data, what)
    got = _nodes(*g.to_vector())
    assert got.shape == exp.shape, (what, k, got.shape, exp.shape)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (what, k, "%d of %d nodes differ; the first: got %s, expected %s" % (bad.size, exp.shape[0], got[bad[0]].tolist(), exp[bad[0]].tolist()))
    _assert_sums(got, k, data, what)
    if keep:
        return got, g
    g.close()
    return got


# ------------------------------------------------------------------------------------------------------------------ the inputs
def one_base_reads(which):
    """80 reads of 100 + i bases of every base of `which`: every record is a maximal piece, all of a base in one fine bucket"""
    return [which[j:j + 1] * (100 + i) for j in range(len(which)) for i in range(80)]


UNITS = ["AC", "AT", "ACGT", "AACCGGTT", "TTGGCCAA", "random"]
PALINDROMIC = {"AT", "ACGT", "AACCGGTT", "all"}     # at even k these hold a k-mer that is its own reverse complement


def tandem_reads(k, which):
    """64 reads per unit of 150 - (i mod 9) bases that start at phase i mod len(unit); "all": every unit in one file"""
    if which == "all":
        return [r for u in UNITS for r in tandem_reads(k, u)]
    unit = _rand_read(np.random.default_rng(7200 + k), 8) if which == "random" else which.encode()
    return [(unit * (160 // len(unit) + 2))[i % len(unit):][:150 - (i % 9)] for i in range(64)]


def sweep_reads(k, part):
    """part 0 / 1: 128 random reads at each length from k - 1 to k + 2 W + 2, lower and upper half of the lengths. "runs": 64 reads
    at each of S - 1, S, S + 1, 2 S, 2 S + 1 windows -- the last length of one run, the first of two and of three runs"""
    rng = np.random.default_rng(7000 + k)
    if part == "runs":
        s = SEG[W_OF[k]]
        return [_rand_read(rng, n) for n in (k + s - 2, k + s - 1, k + s, k + 2 * s - 1, k + 2 * s) for _ in range(64)]
    lengths = list(range(k - 1, k + 2 * W_OF[k] + 3))
    cut = len(lengths) // 2
    return [_rand_read(rng, n) for n in (lengths[:cut], lengths[cut:])[part] for _ in range(128)]


def stretch_reads(k, where, base):
    """150-base reads, every fifth with a stretch of `base` at its start, in its middle or at its end: of NMAX + 5 bases, and of
    NMAX + m + 4 bases, which is more than NMAX windows also where the read begins or ends with it"""
    rng = np.random.default_rng(7400 + k)
    m = k - W_OF[k] + 1
    reads = []
    for i in range(192):
        r = _rand_read(rng, 150)
        if i % 5 == 2:
            s = NMAX[k] + 5 if i % 2 else NMAX[k] + m + 4
            at = {"start": 0, "middle": 40 + i % 30, "end": 150 - s}[where]
            r = r[:at] + base * s + r[at + s:]
        reads.append(r)
    return reads


def strand_reads(k):
    rng = np.random.default_rng(7500 + k)
    return [_rand_read(rng, int(n)) for n in rng.integers(k, 200, size=300)] + [b"A" * 120, b"ACCGGTTA" * 15]


def tail_reads(k):
    """the first half of the length sweep, its last three reads of k, k + 1 and k + 5 bases; 20 reads in lower and mixed case, the
    last three among them"""
    rng = np.random.default_rng(7600 + k)
    reads = sweep_reads(k, 0)
    reads[-3:] = [_rand_read(rng, k), _rand_read(rng, k + 1), _rand_read(rng, k + 5)]
    n = len(reads)
    for j, i in enumerate(list(range(n - 10, n)) + list(range(n // 2, n // 2 + 10))):
        r = reads[i]
        reads[i] = r.lower() if j % 2 else bytes(c | 0x20 if (p * 7 + j) % 3 == 0 else c for p, c in enumerate(r))
    return reads


def crowd_fastq(k, copies):
    """1100 reads of W - 1 random bases, the canonical m-mer of smallest order hash, W - 1 random bases (W k-mers a read, every one
    with that minimizer -- asserted in _crowd on the reads themselves), each `copies` times in a shuffled order"""
    return _crowd(k, 1100, 4000 + k, w=W_OF[k], copies=copies, fastq=lambda codes: _fastq([BASES[row].tobytes() for row in codes]))


# ----------------------------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("which", [b"A", b"C", b"G", b"T", b"ACGT"])
@pytest.mark.parametrize("k", KS)
def test_reads_of_one_base(ctx, k, which):
    """whole batches of 64 maximal records in one fine bucket: at k <= 20 that is 64 x 15 unit marks per wavefront (the marks of a
    wavefront once held 64 x 10). The node is its own neighbour on both sides."""
    got = _check(ctx, k, _fastq(one_base_reads(which)), which)
    assert got.shape[0] == (len(which) + 1) // 2          # A and T, C and G are one node each
    for row in got.tolist():
        out, inn = row[1:5], row[5:9]
        assert sum(1 for c in out if c) == 1 and [c > 0 for c in out] == [c > 0 for c in inn] and sum(out) == sum(inn)


@pytest.mark.parametrize("base", [b"A", b"T"])
@pytest.mark.parametrize("k", [17, 21, 28])
def test_one_node_past_16_bits(ctx, k, base):
    """700 reads of 150 bases of A, and of T: two counters of one node pass 65535 (the carries of `add`)"""
    got = _check(ctx, k, _fastq([base * 150] * 700), base)
    assert got.shape[0] == 1 and int(got[0, 9]) == 700 * (151 - k) > 65536
    assert sorted(got[0, 1:9].tolist()) == [0] * 6 + [700 * (150 - k)] * 2


@pytest.mark.parametrize("which", UNITS + ["all"])
@pytest.mark.parametrize("k", KS)
def test_tandem_repeats(ctx, k, which):
    """records that repeat with period 2, 4 and 8; at even k the units AT, ACGT and AACCGGTT hold k-mers that equal their own
    reverse complement (rev_a = rc < fw decides a tie), and whole records equal theirs (sk_assemble_row's `flipped` does). Such a
    k-mer takes its edges as the read has them, also where its record travels reverse-complemented (kRecFlipShift): without that bit
    the node TATA..TA of the AT file at k = 20 had out T 4052 and in A 4016 where the oracle has 4036 and 4032 -- the 16 reads that
    end with it in a turned record."""
    data = _fastq(tandem_reads(k, which))
    if k % 2 == 0 and which in PALINDROMIC:
        keys = np.ascontiguousarray(_oracle(k, data)[:, :1])
        assert (orc.revcomp(orc.kspec(k), keys) == keys).any(), "no palindromic node in this file"
    _check(ctx, k, data, which)


@pytest.mark.parametrize("part", [0, 1, "runs"])
@pytest.mark.parametrize("k", KS)
def test_read_length_sweep(ctx, k, part):
    """no window, one window, every fill of the walk's last block; and reads of two and three runs: at a run cut the read goes on,
    so the outside base there is a base (s_runx), at the read's ends it is none"""
    _check(ctx, k, _fastq(sweep_reads(k, part)), part)


@pytest.mark.parametrize("base", [b"A", b"T"])
@pytest.mark.parametrize("where", ["start", "middle", "end"])
@pytest.mark.parametrize("k", KS)
def test_one_base_stretch_inside_ordinary_reads(ctx, k, where, base):
    """a super-k-mer of more than NMAX windows is cut into pieces whose outside bases come from the run's row; a stretch of T is
    stored reverse-complemented, so its pieces swap sides and complement"""
    _check(ctx, k, _fastq(stretch_reads(k, where, base)), (where, base))


@pytest.mark.parametrize("k", KS)
def test_reads_and_their_reverse_complements(ctx, k):
    """the same reads, and with every read's reverse complement appended: the keys stay and occurrences double. A k-mer x with the
    base l before and r behind it adds in[l] and out[r] to its node if x is the smaller strand. In the reverse complement of the
    read the k-mer is rc(x) between comp(r) and comp(l); it is kept as x, its edges change sides and are complemented, which is
    in[l] and out[r] again (likewise if rc(x) is the smaller strand): all eight edge counters double. Only a node with x = rc(x)
    (the ACCGGTTA repeat holds some at even k) is kept as it comes both times: the second read adds in[comp(r)] and out[comp(l)], so
    out[b] becomes out[b] + in[comp(b)] and in[b] becomes in[b] + out[comp(b)]. That needs no oracle. The records of the second half
    of the file are the mirror images of the first half's: `flipped` and rev_a take their other value for each."""
    reads = strand_reads(k)
    once = _check(ctx, k, _fastq(reads), "once")
    both = _check(ctx, k, _fastq(reads + [_revcomp(r) for r in reads]), "both")
    _assert_mirrored(k, once, both)


def _assert_mirrored(k, once, both):
    assert once.shape == both.shape and (once[:, 0] == both[:, 0]).all()
    assert (both[:, 9] == 2 * once[:, 9]).all()
    keys = np.ascontiguousarray(once[:, :1])
    pal = (orc.revcomp(orc.kspec(k), keys) == keys)[:, 0]
    assert pal.any() == (k % 2 == 0)
    assert (both[~pal, 1:9] == 2 * once[~pal, 1:9]).all()
    for b in range(4):
        assert (both[pal, 1 + b] == once[pal, 1 + b] + once[pal, 5 + (3 - b)]).all(), ("out", b)
        assert (both[pal, 5 + b] == once[pal, 5 + b] + once[pal, 1 + (3 - b)]).all(), ("in", b)


@pytest.mark.parametrize("order", ["as-written", "reversed"])
@pytest.mark.parametrize("final_newline", [True, False])
@pytest.mark.parametrize("k", KS)
def test_the_end_of_the_buffer(ctx, k, final_newline, order):
    """the last reads have no room for 16-byte loads and are packed byte by byte; the byte behind the last run of a file without
    a final newline reads as an end of line; lower- and mixed-case bases"""
    reads = tail_reads(k)
    data = _fastq(reads if order == "as-written" else reads[::-1])
    _check(ctx, k, data if final_newline else data[:-1], (final_newline, order))


@pytest.mark.parametrize("copies", [1, 3])
@pytest.mark.parametrize("k", [31, 21])
def test_bucket_of_several_table_chunks(k, copies):
    """about 20 900 (k = 31) and 12 100 (k = 21) nodes in ONE fine bucket among the ordinary buckets of 2000 reads: the bucket is
    walked in table fills of 4608 nodes, every record is read again per fill and the k-mers of other fills are skipped. With every
    crowd read three times the counts are threefold."""
    import kmerind_amd as K
    crowd = crowd_fastq(k, copies)
    alone = _oracle(k, crowd)
    assert alone.shape[0] > 2 * ROWS, alone.shape
    assert (alone[:, 9] % copies == 0).all()
    data = bytes(K.synth_fastq(seed=7 * k, genome_len=30_000, n_reads=2_000)) + crowd
    c = K.Context(0)
    try:
        _check(c, k, data, copies)
    finally:
        c.close()


@pytest.mark.parametrize("which", ["tandem", "one-base"])
@pytest.mark.parametrize("k", [21, 22, 28, 31])
def test_unitigs_of_low_complexity_graphs(ctx, k, which):
    """self-loops and short cycles through palindromic nodes: the compaction against the model on the oracle's map"""
    from kmerind_amd.core import split_unitigs
    data = _fastq(tandem_reads(k, "all") if which == "tandem" else one_base_reads(b"ACGT"))
    _, g = _check(ctx, k, data, which, keep=True)
    exp_rows = _oracle(k, data)
    exp = M.unitigs(np.ascontiguousarray(exp_rows[:, :1]), exp_rows[:, 1:], k)
    off, bases, occ, circ = g.unitigs()
    assert off.shape[0] == occ.shape[0] + 1 and int(off[-1]) == bases.shape[0]
    got = sorted((s.decode(), int(o), bool(cy)) for s, o, cy in zip(split_unitigs(off, bases), occ, circ))
    g.close()
    assert got == exp
