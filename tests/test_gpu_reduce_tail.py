"""sk_reduce around the end of a bucket: the queue tickets taken two buckets ahead, the hand-over of the next bucket's range and
first records, and the emit sweep -- on inputs that put one fine bucket through many passes between ordinary ones, and on inputs
where almost every ticket is an empty bucket. Every build is compared with the CPU oracle's map, as the other index tests are."""
import itertools

import numpy as np
import pytest

from tests import oracle as orc
from tests.test_gpu_index import STRAND, _same_map

pytestmark = pytest.mark.gpu

W = 19                      # windows per k-mer for k = 29 .. 32: the minimizer is the smallest of W canonical (k - 18)-mers
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
_MULT = 0x9E3779B1


def _order_hash(c):
    """the order among canonical m-mers (restated from the build): a bijection on 32 bits"""
    h = (np.asarray(c, dtype=np.uint64) * np.uint64(_MULT)) & np.uint64(0xFFFFFFFF)
    return h ^ (h >> np.uint64(15))


def _order_hash_inverse(h):
    h ^= (h >> 15) ^ (h >> 30)
    return (h * pow(_MULT, -1, 1 << 32)) & 0xFFFFFFFF


def _revcomp_codes(c, m):
    r = 0
    for _ in range(m):
        r = (r << 2) | (3 - (c & 3))
        c >>= 2
    return r


def _smallest_mmer(m):
    """the canonical m-mer with the smallest order hash: hash values in rising order, the first whose m-mer exists and is canonical"""
    for h in itertools.count():
        c = _order_hash_inverse(h)
        assert int(_order_hash(c)) == h
        if c < (1 << (2 * m)) and c <= _revcomp_codes(c, m):
            return c


def _minimizers(codes, k, w=W):
    """codes: (reads, length) base codes; the canonical m-mer of smallest order hash of every k-mer -> (reads, k-mers); w: the
    windows per k-mer of that k (sk_window_of)"""
    m = k - w + 1
    n, length = codes.shape
    npos = length - m + 1
    f = np.zeros((n, npos), dtype=np.uint64)
    r = np.zeros((n, npos), dtype=np.uint64)
    for j in range(m):
        f = (f << np.uint64(2)) | codes[:, j:j + npos].astype(np.uint64)
        r |= (np.uint64(3) - codes[:, j:j + npos].astype(np.uint64)) << np.uint64(2 * j)
    canon = np.minimum(f, r)
    hashes = _order_hash(canon)
    nk = length - k + 1
    best = np.stack([hashes[:, p:p + nk] for p in range(w)]).argmin(axis=0)        # (the hash is a bijection: no ties between m-mers)
    return np.take_along_axis(canon, best + np.arange(nk)[None, :], axis=1)


def _fastq(codes):
    out = []
    for i, row in enumerate(codes):
        s = BASES[row].tobytes()
        out.append(b"@c%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n")
    return np.frombuffer(b"".join(out), dtype=np.uint8)


def _build_and_compare(c, k, strand, batches):
    """one index, the batches built into it one after the other (the second starts from the first one's level hint); sk_reduce ran"""
    import kmerind_amd as K
    s = orc.kspec(k, orc.DNA)
    idx = K.CountIndex(c, K.make_config(k, "DNA", strand=strand))
    om = orc.CountMap(s, STRAND[strand])
    for data in batches:
        c.profile(True)
        c.profile_reset()
        idx.build(data)
        names = {p["name"] for p in c.profile_get() if p["launches"]}
        c.profile(False)
        assert "sk_reduce" in names, names
        om.insert(orc.extract(s, data, orc.FASTQ)["kmers"])
        _same_map(idx, om)
    idx.close()


@pytest.mark.parametrize("k,strand", [(31, "canonical"), (32, "single")])
def test_one_bucket_of_many_passes_between_ordinary_ones(k, strand):
    """About 1100 reads of 18 random bases, one fixed m-mer M, 18 random bases (m = k - 18: 13 at k = 31, 49 bases, 19 k-mers a
    read): M is the canonical m-mer of smallest order hash, so it is the minimizer of every one of the about 20 000 distinct
    k-mers -- asserted below on the reads themselves. They all land in ONE fine bucket, far past the k-mer table, and the
    records' sub-bucket bits cannot split it: the pass stack, lost passes, the emit of full tables and the hand-over to the next
    bucket behind a bucket of many passes all run, among the ordinary buckets of 2000 reads of a 30 kbp genome. k = 32 single
    strand adds 40 reads of T only (the key that equals the table's empty marker). Built twice in one context: the second
    build starts from the level hint the first one left."""
    import kmerind_amd as K
    m = k - W + 1
    mm = _smallest_mmer(m)
    rng = np.random.default_rng(100 + k)
    n = 1100
    fixed = np.array([(mm >> (2 * (m - 1 - j))) & 3 for j in range(m)], dtype=np.uint8)
    codes = np.concatenate([rng.integers(0, 4, (n, 18), dtype=np.uint8), np.broadcast_to(fixed, (n, m)), rng.integers(0, 4, (n, 18), dtype=np.uint8)], axis=1)
    mins = _minimizers(codes, k)
    assert mins.shape == (n, 19) and (mins == np.uint64(mm)).all()
    crowd = _fastq(codes)
    parts = [K.synth_fastq(seed=7 * k, genome_len=30_000, n_reads=2_000), crowd]
    if k == 32:
        parts.append(np.frombuffer((b"@x\n" + b"T" * 150 + b"\n+\n" + b"I" * 150 + b"\n") * 40, dtype=np.uint8))
    first = np.concatenate(parts)
    second = np.concatenate([K.synth_fastq(seed=9 * k, genome_len=30_000, n_reads=500), _fastq(codes[: n // 2])])
    c = K.Context(0)
    _build_and_compare(c, k, strand, [first, second])
    c.close()


@pytest.mark.parametrize("copies", [1, 2, 65])
@pytest.mark.parametrize("n_reads", [1, 2])
def test_almost_every_ticket_is_an_empty_bucket(copies, n_reads):
    """1, 2 and 65 copies of one read and of two different reads: a handful of buckets hold records (65 copies: more than 64
    identical records in one), every other ticket is an empty bucket that only hands the queue on. The build must end -- no
    workgroup is left waiting for a ticket -- and give the oracle's map."""
    import kmerind_amd as K
    one = K.synth_fastq(seed=3, genome_len=5_000, n_reads=n_reads)
    data = np.concatenate([one] * copies)
    c = K.Context(0)
    _build_and_compare(c, 31, "canonical", [data])
    c.close()
