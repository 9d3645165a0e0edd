"""sk_reduce, phase A: identical records counted in the record table T1 -- copies of one record that arrive in the same step, T1
past its fill limit and past the overflow list, the record whose first word equals the empty marker, the carried level and
duplication hints of a second build, and the path without T1. Every build is compared with the CPU oracle's map, exactly."""
import numpy as np
import pytest

from tests.test_gpu_reduce_tail import W, _build_and_compare, _fastq, _minimizers, _smallest_mmer

pytestmark = pytest.mark.gpu


def _context():
    import kmerind_amd as K
    return K.Context(0)   # a fresh one per test: no hint of an earlier build decides whether T1 is used


@pytest.mark.parametrize("copies", [1, 2, 63, 64, 65, 130, 300])
@pytest.mark.parametrize("n_reads", [1, 3])
def test_copies_of_a_record_in_the_same_step(copies, n_reads):
    """1 .. 300 copies of one 150-bp read, and of three different reads: every record of a bucket has that many copies, which
    sit side by side in the bucket. Lanes of one wavefront (up to 64 copies), and of different wavefronts (more), go for the same
    slot of T1 in the same step: one claims it, the others are counted with it, wait in the overflow list or sit in T1 a second
    time -- the counts must be the oracle's whichever happens."""
    import kmerind_amd as K
    one = K.synth_fastq(seed=5, genome_len=5_000, n_reads=n_reads)
    assert one.shape[0] == n_reads * 315   # 150-bp reads
    c = _context()
    _build_and_compare(c, 31, "canonical", [np.concatenate([one] * copies)])
    c.close()


def _crowd(k, n, seed, w=W, copies=2, fastq=_fastq):
    """n distinct reads of 18 random bases, the m-mer of smallest order hash, 18 random bases, each present twice in a shuffled order
    (some twins side by side, most apart): one record of 19 k-mers per read, all in ONE fine bucket. (w: for another window width,
    w - 1 bases on either side and w k-mers per read; copies: how often each read is present; fastq: the writer of the file)"""
    m = k - w + 1
    mm = _smallest_mmer(m)
    rng = np.random.default_rng(seed)
    fixed = np.array([(mm >> (2 * (m - 1 - j))) & 3 for j in range(m)], dtype=np.uint8)
    codes = np.concatenate([rng.integers(0, 4, (n, w - 1), dtype=np.uint8), np.broadcast_to(fixed, (n, m)), rng.integers(0, 4, (n, w - 1), dtype=np.uint8)], axis=1)
    assert np.unique(codes, axis=0).shape[0] == n
    mins = _minimizers(codes, k, w)
    assert mins.shape == (n, w) and (mins == np.uint64(mm)).all()
    return fastq(codes[rng.permutation(np.repeat(np.arange(n), copies))])


@pytest.mark.parametrize("k,strand", [(31, "canonical"), (32, "single")])
@pytest.mark.parametrize("n", [1000, 1200, 1700])
def test_record_table_past_its_limit_and_past_the_list(k, strand, n):
    """One fine bucket of 2 n records, n distinct ones that T1 must count 2, among the ordinary buckets of 2000 reads of a
    30 kbp genome. T1 takes records up to L1 = 1152 (of 1536 home slots: a load of 0.75, so full first windows and claims in the
    second window occur by themselves) and the overflow list 448 more: n = 1000 stays below L1, 1200 goes past L1 and stays
    inside the list, 1700 goes past the list, so that phase A expands records directly. The n = 1200 case builds a second batch
    into the same index and context: that build starts from the level and duplication hints the first one left, so T1 is used
    in every pass of the crowded bucket."""
    import kmerind_amd as K
    crowd = _crowd(k, n, 1000 * k + n)
    batches = [np.concatenate([K.synth_fastq(seed=7 * k, genome_len=30_000, n_reads=2_000), crowd])]
    if n == 1200:
        batches.append(np.concatenate([K.synth_fastq(seed=9 * k, genome_len=30_000, n_reads=2_000), crowd]))
    c = _context()
    _build_and_compare(c, k, strand, batches)
    c.close()


@pytest.mark.parametrize("k,strand", [(32, "single"), (31, "canonical")])
def test_record_whose_first_word_is_the_empty_marker(k, strand):
    """100 reads of T only and 100 of A only: super-k-mer records of one base, among them the one whose first word is all ones,
    T1's empty marker -- it bypasses T1 (at k = 32 single strand its k-mer is the k-mer table's empty marker as well)."""
    def reads(base):
        return np.frombuffer((b"@x\n" + base * 150 + b"\n+\n" + b"I" * 150 + b"\n") * 100, dtype=np.uint8)
    c = _context()
    _build_and_compare(c, k, strand, [np.concatenate([reads(b"T"), reads(b"A")])])
    c.close()


def test_second_build_without_the_record_table():
    """3000 reads of a 3 Mbp genome hold next to no k-mer twice: the second build of them in one context carries a
    low-duplication hint and counts no records in T1 (phase A expands every record directly)."""
    import kmerind_amd as K
    data = K.synth_fastq(seed=31, genome_len=3_000_000, n_reads=3_000)
    c = _context()
    _build_and_compare(c, 31, "canonical", [data, data])
    c.close()
