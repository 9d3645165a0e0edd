"""Seeded inputs for the position / position + quality index tests (test_gpu_position_sequences.py): hot keys that fill one
placement bucket past the query table, a heavy key, and small FASTQ / FASTA read sets whose keys repeat. Test side only, no GPU
needed; test_multimap_cases.py checks on the CPU what the GPU tests take for granted."""
import numpy as np

from tests import index_model as M
from tests import oracle as orc
from tests.test_gpu_index import _keys_in_one_placement_bucket

ALPHA = {"DNA": orc.DNA, "DNA5": orc.DNA5}
VW = {"position": 1, "posqual": 2}

# QTabCfg<NW>::CAP of kmerind_amd/csrc/kmi_index.hip, by key words: the home slots of bucket_query_kernel's LDS table of a
# bucket's distinct query keys (6656 for one word, TabCfg<NW>::CAP for more). The table takes LIMIT = CAP * 3 / 4 of them per pass.
QUERY_CAP = {1: 6656, 2: 6144, 3: 4608, 4: 3712}
N_HOT = 16_000      # distinct hot keys stored in the one bucket
N_HOT_Q = 8_000     # distinct hot keys queried: more than every QUERY_CAP, so no table holds them in one pass
# (In practice the kernel takes far more passes than N_HOT_Q / LIMIT: the generated keys' hashes count up in their low 17 bits,
# which pick the home slot, so the homes crowd into the table's first few hundred slots and a pass is given up on its probe
# length, kMaxProbe, until a pass holds a few hundred keys -- some tens of passes. Counting alone already forces two.)
BUCKET = 777        # the placement bucket of the hot keys (of kmi_index_num_buckets() = 32768)
N_FILLER = 20_000   # random k-mers mixed in
N_HEAVY = 150_000   # values of the heavy key: far above a workgroup's 512 lanes
# the words above word 0 of every multi-word hot key; the top 16 bits of the last one are zero (so are the pad bits)
_LATER = (0xFEDCBA9876543210, 0x0123456789ABCDEF, 0x0000123456789ABC)

# (k, alphabet, index kind) of the query-pass tests: one-, two- and three-word keys with one and two value words
PASS_SHAPES = [(31, "DNA", "position"), (31, "DNA", "posqual"), (63, "DNA", "position"), (63, "DNA5", "posqual")]
# (k, alphabet, index kind) of the heavy-key tests; at k = 32 the heavy key is the table's empty marker
HEAVY_SHAPES = [(31, "DNA", "position"), (32, "DNA", "posqual")]
EMPTY_MARKER = 0xFFFFFFFFFFFFFFFF    # kEmptyKey: the all-T 32-mer


def pad_bits(s):
    return s.n_words * 64 - s.n_bits


def hot_keys(k, alpha, n, bucket=BUCKET):
    """n distinct valid keys of the shape (k, alpha), as (n, n_words), that the placement hash files in `bucket`"""
    s = orc.kspec(k, ALPHA[alpha])
    later = _LATER[len(_LATER) - (s.n_words - 1):]
    keys = _keys_in_one_placement_bucket(n, bucket, later_words=later)
    return np.ascontiguousarray(keys, dtype=np.uint64).reshape(n, s.n_words)


def random_kmers(s, rng, n):
    """n valid k-mers of a random A C G T string"""
    return orc.kmers_from_string(s, M.random_seq(rng, n + s.k - 1))


def distinct_values(rng, n, vw, first=0):
    """(n, vw) value words: word 0 a distinct 64-bit id (the low half counts up from `first` in random order, the high half is
    random), word 1 (vw == 2) a random uint32 bit pattern in the low half"""
    v = np.zeros((n, vw), dtype=np.uint64)
    v[:, 0] = (rng.permutation(n).astype(np.uint64) + np.uint64(first)) | (rng.integers(0, 1 << 32, n, dtype=np.uint64) << np.uint64(32))
    if vw == 2:
        v[:, 1] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    return v


def hot_tuples(rng, keys, vw, s, n_filler=N_FILLER):
    """(kmers, values): every hot key one to three times and n_filler random k-mers, shuffled; values as distinct_values"""
    reps = rng.integers(1, 4, size=keys.shape[0])
    kmers = np.concatenate([np.repeat(keys, reps, axis=0), random_kmers(s, rng, n_filler)])
    order = rng.permutation(kmers.shape[0])
    return np.ascontiguousarray(kmers[order]), distinct_values(rng, kmers.shape[0], vw)


def heavy_tuples(key, n=N_HEAVY, vw=1, seed=0):
    """(kmers, values): one key n times with n distinct values (their ids start at 2^31: none meets an id of hot_tuples)"""
    key = np.asarray(key, dtype=np.uint64).reshape(1, -1)
    return np.ascontiguousarray(np.repeat(key, n, axis=0)), distinct_values(np.random.default_rng(seed), n, vw, first=1 << 31)


def pass_queries(rng, hot, s):
    """N_HOT_Q of the hot keys, 1000 absent random k-mers and 500 of the queried hot keys a second time, shuffled"""
    q = np.concatenate([hot[:N_HOT_Q], random_kmers(s, rng, 1000), hot[:500]])
    return np.ascontiguousarray(q[rng.permutation(q.shape[0])])


# ---- small read sets for the operation sequences
GENOME = M.random_seq(np.random.default_rng(777), 3_000)


def reads(rng, n, k, lo=60, hi=150):
    """n reads of lo .. hi bases from both strands of the 3000-base GENOME (keys repeat across reads and across calls), and a
    few reads shorter than k"""
    out = []
    for _ in range(n):
        ln = int(rng.integers(lo, hi + 1))
        p = int(rng.integers(0, len(GENOME) - ln + 1))
        r = GENOME[p:p + ln]
        out.append(M.revcomp_text(r) if rng.integers(0, 2) else r)
    out += [M.random_seq(rng, int(rng.integers(1, k))) for _ in range(3)]
    return out


def fastq(rng, seqs, tag=b"r"):
    """FASTQ records with random quality characters '!' .. 'I' (a position + quality index reads them)"""
    out = []
    for i, sq in enumerate(seqs):
        q = rng.integers(33, 74, size=len(sq), dtype=np.uint8)
        out.append(b"@%s%d\n%s\n+\n%s\n" % (tag, i, sq, bytes(q.tolist())))
    return b"".join(out)


def fasta(seqs, tag=b"s"):
    return M.fasta(seqs, tag=tag, line=60)


def poly_fastq(rng, k, n_reads=150, n_poly=40):
    """ordinary reads, 40 poly-T and 3 poly-A reads: at k = 32 on a single strand poly-T is the key EMPTY_MARKER, under the
    canonical strand model it becomes the all-zero key"""
    return fastq(rng, reads(rng, n_reads, k) + M.poly_reads(b"T", n_poly) + M.poly_reads(b"A", 3))


def tuples_of(s, data, vw, fmt=orc.FASTQ, file_offset=0):
    """the reference parser's (kmers, values) of a buffer: ids, and for vw == 2 the quality float's bits in word 1"""
    ex = orc.extract(s, data, fmt, file_offset=file_offset, want_ids=True, want_quals=(vw == 2))
    vals = np.zeros((ex["kmers"].shape[0], vw), dtype=np.uint64)
    vals[:, 0] = ex["ids"]
    if vw == 2:
        vals[:, 1] = ex["quals"].view(np.uint32)
    return ex["kmers"], vals
