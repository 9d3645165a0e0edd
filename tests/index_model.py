"""Plain reference model of a count index and of a de Bruijn node map, and seeded adversarial inputs, for the operation-sequence
tests (test_gpu_index_sequences.py, test_gpu_minimizer_queries.py). The models restate the oracle's map semantics in Python dicts
so that operations the oracle has no entry point for (insert_pairs, update_pairs, saturating counts, node erase) have an expected
value; test_index_model.py checks them against the oracle (tests/oracle.py). Test-side only, no GPU needed."""
from collections import Counter

import numpy as np

from tests import oracle as orc

MASK32 = 0xFFFFFFFF


def sk_window_of(k):
    """the super-k-mer window W by k (kmi_minimizer.h); the minimizer length is m = k - W + 1"""
    return 19 if k >= 29 else (13 if k >= 23 else (11 if k >= 21 else (7 if k >= 17 else 0)))


def sk_nmax_of(k):
    """k-mers of the longest super-k-mer record (kmi_minimizer.h): a read of k + nmax - 1 bases is one record at most"""
    return min(52 - k, 32)


def _rows(a, nw):
    return [tuple(r) for r in np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, nw).tolist()]


def _arr(keys, nw):
    return np.array(keys, dtype=np.uint64).reshape(-1, nw)


class CountModel:
    """counting_unordered_map restated: keys canonical (strand=orc.CANONICAL) or as given (orc.SINGLE), one u32 count per key;
    saturating = counts stop at 2^32 - 1 instead of wrapping (kmi_index_set_saturating)"""

    def __init__(self, k, alphabet=orc.DNA, strand=orc.CANONICAL, saturating=False):
        assert strand in (orc.SINGLE, orc.CANONICAL)
        self.k, self.strand, self.saturating = k, strand, saturating
        self.s = orc.kspec(k, alphabet)
        self.nw = self.s.n_words
        self.d = {}

    def copy(self):
        m = CountModel.__new__(CountModel)
        m.__dict__.update(self.__dict__)
        m.d = dict(self.d)
        return m

    def transform(self, kmers):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, self.nw)
        return kmers if self.strand == orc.SINGLE else orc.canonical(self.s, kmers)

    def _add(self, a, b):
        return min(a + b, MASK32) if self.saturating else (a + b) & MASK32

    def insert(self, kmers):
        for key, n in Counter(_rows(self.transform(kmers), self.nw)).items():
            self.d[key] = self._add(self.d.get(key, 0), n)

    def insert_pairs(self, kmers, counts):
        """every pair's count (mod 2^32) is added; a new key starts at 0"""
        for key, c in zip(_rows(self.transform(kmers), self.nw), np.asarray(counts, dtype=np.uint64).tolist()):
            self.d[key] = self._add(self.d.get(key, 0), int(c) & MASK32)

    def update_pairs(self, kmers, values, op):
        """update(pairs, op): stored keys only, pairs of one key in input order (assign keeps the last); add wraps -> pairs applied"""
        hit = 0
        for key, v in zip(_rows(self.transform(kmers), self.nw), np.asarray(values, dtype=np.uint64).tolist()):
            if key not in self.d:
                continue
            hit += 1
            v = int(v) & MASK32
            c = self.d[key]
            self.d[key] = {"add": (c + v) & MASK32, "max": max(c, v), "min": min(c, v), "assign": v}[op]
        return hit

    def erase(self, kmers):
        n = 0
        for key in _rows(self.transform(kmers), self.nw):
            if self.d.pop(key, None) is not None:
                n += 1
        return n

    def clear(self):
        self.d = {}

    def size(self):
        return len(self.d)

    def export(self):
        keys = list(self.d)
        return _arr(keys, self.nw), np.array([self.d[t] for t in keys], dtype=np.uint32)

    def count(self, q):
        """one row per distinct transformed query: 0 or 1"""
        u = list(dict.fromkeys(_rows(self.transform(q), self.nw)))
        return _arr(u, self.nw), np.array([int(t in self.d) for t in u], dtype=np.uint64)

    def find(self, q):
        """one row per distinct transformed query that is stored: its count"""
        u = [t for t in dict.fromkeys(_rows(self.transform(q), self.nw)) if t in self.d]
        return _arr(u, self.nw), np.array([self.d[t] for t in u], dtype=np.uint64)

    def exists(self, q):
        return np.array([t in self.d for t in _rows(self.transform(q), self.nw)], dtype=np.uint8)


class NodeModel:
    """de Bruijn node map: every parsed (k-mer, edge byte) tuple goes into an orc.DbgMap; erase drops the erased nodes' tuples and
    rebuilds it. Nodes are compared under orc.canonical."""

    def __init__(self, k, alphabet=orc.DNA):
        self.k = k
        self.s = orc.kspec(k, alphabet)
        self.nw = self.s.n_words
        self.clear()

    def clear(self):
        self.kmers = np.zeros((0, self.nw), dtype=np.uint64)
        self.edges = np.zeros(0, dtype=np.uint8)
        self.om = orc.DbgMap(self.s)

    def build(self, data, fmt=orc.FASTQ):
        self.insert(*orc.dbg_parse(self.s, data, fmt))

    def insert(self, kmers, edges):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, self.nw)
        edges = np.ascontiguousarray(edges, dtype=np.uint8)
        self.kmers = np.concatenate([self.kmers, kmers])
        self.edges = np.concatenate([self.edges, edges])
        self.om.insert(kmers, edges)

    def _stored(self):
        return set(_rows(self.om.export(canonical=True)[0], self.nw))

    def erase(self, q):
        gone = set(_rows(orc.canonical(self.s, q), self.nw)) & self._stored()
        if gone:
            keep = np.array([t not in gone for t in _rows(orc.canonical(self.s, self.kmers), self.nw)], dtype=bool)
            kmers, edges = self.kmers[keep], self.edges[keep]
            self.clear()
            self.insert(kmers, edges)
        return len(gone)

    def size(self):
        return self.om.size()

    def export(self):
        return self.om.export(canonical=True)

    def find(self, q):
        return self.om.find(q, canonical=True)

    def count(self, q):
        have = self._stored()
        u = list(dict.fromkeys(_rows(orc.canonical(self.s, q), self.nw)))
        return _arr(u, self.nw), np.array([int(t in have) for t in u], dtype=np.uint64)


# ---- inputs
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp_text(seq):
    return seq.translate(_COMP)[::-1]


def random_seq(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])


def fastq(seqs, tag=b"r"):
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag, i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def fasta(seqs, tag=b"r", line=70):
    out = []
    for i, s in enumerate(seqs):
        out.append(b">%s%d\n" % (tag, i))
        out.extend(s[j:j + line] + b"\n" for j in range(0, len(s), line))
    return b"".join(out)


def background(rng, n_reads, read_len=150, genome_len=20_000, genome=None):
    """reads drawn from both strands of one random genome (about n_reads * read_len / genome_len coverage); pass `genome` to
    draw several batches from the same one"""
    g = genome if genome is not None else random_seq(rng, genome_len)
    genome_len = len(g)
    out = []
    for _ in range(n_reads):
        p = int(rng.integers(0, genome_len - read_len + 1))
        r = g[p:p + read_len]
        out.append(revcomp_text(r) if rng.integers(0, 2) else r)
    return out


def palindrome(rng, m):
    """an m-mer equal to its own reverse complement (m even)"""
    h = random_seq(rng, m // 2)
    return h + revcomp_text(h)


def adversarial_reads(rng, k, read_len=150):
    """reads where a minimizer walk can go wrong, all of A C G T: single-base and periodic runs (periods 1 - 8), a read followed
    by its own reverse complement, palindromic m-mers (even m), and the record-split lengths k, k + nmax - 1, k + nmax"""
    out = [b"A" * read_len, b"T" * read_len, b"C" * read_len, b"G" * (k + 3)]
    for p in range(1, 9):
        u = random_seq(rng, p)
        if p > 1 and len(set(u)) == 1:
            u = u[:-1] + (b"C" if u[:1] != b"C" else b"G")
        out.append((u * (read_len // p + 1))[:read_len])
    for _ in range(3):
        r = random_seq(rng, read_len // 2)
        out.append(r + revcomp_text(r))
    m = k - sk_window_of(k) + 1 if sk_window_of(k) else 12
    for mm in sorted({m - (m % 2), 12, 14, 16}):
        pal = palindrome(rng, mm)
        for _ in range(3):
            out.append(random_seq(rng, int(rng.integers(0, k))) + pal + random_seq(rng, int(rng.integers(0, k))) + pal + random_seq(rng, 5))
        out.append(pal * (read_len // mm))
    nmax = sk_nmax_of(k)
    for n in (k, k + nmax - 1, k + nmax, k + 2 * nmax, k - 1):
        out.extend(random_seq(rng, n) for _ in range(2))
    return out


def with_n_runs(rng, seqs, k):
    """N runs of 1 - k bases inside some reads (cut points of the n_split filter; an A inside a plain 2-bit k-mer)"""
    out = []
    for i, s in enumerate(seqs):
        if i % 3 == 0 and len(s) > 2 * k:
            p = int(rng.integers(1, len(s) - k))
            n = int(rng.integers(1, k + 1))
            s = s[:p] + b"N" * n + s[p + n:]
        out.append(s)
    return out


def crowded_reads(rng, copies=3000, read_len=150):
    """one read copied `copies` times: its few minimizer buckets take every copy's records (a fine bucket outgrows its room)"""
    return [random_seq(rng, read_len)] * copies


def poly_reads(base, n, read_len=150):
    return [base * read_len] * n


# ---- probes
def one_base_variants(s, keys, positions):
    """keys with the base at each position (0 = first base) replaced by another base (one-word 2-bit k-mers only)"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    out = []
    for i, p in enumerate(positions):
        sh = np.uint64(2 * (s.k - 1 - p))
        out.append(keys ^ (np.uint64(1 + (i % 3)) << sh))
    return np.concatenate(out).reshape(-1, 1) if out else np.zeros((0, 1), dtype=np.uint64)


def probes(s, stored, rng, n_stored=1500, n_absent=300):
    """a query set for a stored key set: stored keys, their reverse complements, random keys, one-base variants of stored keys
    in the first and the last m-mer (same or a neighbouring minimizer, another key), and the all-A and all-T k-mers"""
    stored = np.ascontiguousarray(stored, dtype=np.uint64).reshape(-1, s.n_words)
    pick = stored[rng.integers(0, stored.shape[0], min(n_stored, stored.shape[0]))] if stored.shape[0] else stored
    parts = [pick, orc.revcomp(s, pick[: pick.shape[0] // 2]), orc.kmers_from_string(s, random_seq(rng, n_absent + s.k - 1))]
    if s.n_words == 1 and pick.shape[0]:
        w = sk_window_of(s.k)
        m = s.k - w + 1 if w else s.k // 2
        parts.append(one_base_variants(s, pick[: min(300, pick.shape[0])], [0, m - 1, s.k - m, s.k - 1]))
    parts += [orc.kmers_from_string(s, b"A" * s.k), orc.kmers_from_string(s, b"T" * s.k)]
    return np.concatenate(parts)


# ---- comparisons
def first_difference(got_keys, got_vals, want_keys, want_vals):
    """None when the two (key, value) multisets are equal, else a line naming the first key whose value differs"""
    if len(got_vals) == 0 or len(want_vals) == 0:
        return None if len(got_vals) == len(want_vals) else "%d rows vs %d expected" % (len(got_vals), len(want_vals))
    a = orc.sorted_rows(got_keys, np.asarray(got_vals, dtype=np.uint64).reshape(-1, 1))
    b = orc.sorted_rows(want_keys, np.asarray(want_vals, dtype=np.uint64).reshape(-1, 1))
    if a.shape == b.shape and (a == b).all():
        return None
    g = {tuple(r[:-1]): r[-1] for r in a.tolist()}
    w = {tuple(r[:-1]): r[-1] for r in b.tolist()}
    for key in sorted(set(g) | set(w)):
        if g.get(key) != w.get(key):
            return "%d rows vs %d expected; first differing key %s: got %s, expected %s" % (
                a.shape[0], b.shape[0], "/".join("%016x" % x for x in key), g.get(key), w.get(key))
    return "%d rows vs %d expected (repeated keys)" % (a.shape[0], b.shape[0])


def first_difference_rows(got_keys, got_rows, want_keys, want_rows):
    """the same for multi-column values (de Bruijn nodes: nine counters)"""
    if len(got_rows) == 0 or len(want_rows) == 0:
        return None if len(got_rows) == len(want_rows) else "%d nodes vs %d expected" % (len(got_rows), len(want_rows))
    a = orc.sorted_rows(got_keys, np.asarray(got_rows).astype(np.uint64))
    b = orc.sorted_rows(want_keys, np.asarray(want_rows).astype(np.uint64))
    if a.shape == b.shape and (a == b).all():
        return None
    nw = np.asarray(got_keys).reshape(len(got_rows), -1).shape[1] if len(got_rows) else np.asarray(want_keys).reshape(len(want_rows), -1).shape[1]
    g = {tuple(r[:nw]): tuple(r[nw:]) for r in a.tolist()}
    w = {tuple(r[:nw]): tuple(r[nw:]) for r in b.tolist()}
    for key in sorted(set(g) | set(w)):
        if g.get(key) != w.get(key):
            return "%d nodes vs %d expected; first differing key %s: got %s, expected %s" % (
                a.shape[0], b.shape[0], "/".join("%016x" % x for x in key), g.get(key), w.get(key))
    return "%d nodes vs %d expected" % (a.shape[0], b.shape[0])


def state_difference(idx, model, q, full=True):
    """None when a count index (kmerind_amd.CountIndex) holds what the model holds -- local_size, count / find / exists on the
    query set q, and (full) to_vector, which makes a sparse index dense -- else a line naming the first thing that differs"""
    if idx.local_size() != model.size():
        return "local_size %d, expected %d" % (idx.local_size(), model.size())
    checks = [("count", idx.count, model.count), ("find", idx.find, model.find)]
    if full:
        checks.append(("to_vector", lambda _: idx.to_vector(), lambda _: model.export()))
    for what, got_fn, want_fn in checks:
        got, want = got_fn(q), want_fn(q)
        d = first_difference(got[0], got[1], want[0], want[1])
        if d:
            return "%s: %s" % (what, d)
    ge, we = idx.exists(q), model.exists(q)
    if not (ge == we).all():
        i = int(np.nonzero(ge != we)[0][0])
        return "exists: query %d (%s) got %d, expected %d" % (i, "/".join("%016x" % x for x in q[i].tolist()), ge[i], we[i])
    return None


def node_state_difference(g, model, q):
    """the same for a de Bruijn node map (kmerind_amd.DeBruijnNodes): local_size, to_vector, find and count on q"""
    if g.local_size() != model.size():
        return "local_size %d, expected %d" % (g.local_size(), model.size())
    d = first_difference_rows(*g.to_vector(), *model.export())
    if d:
        return "to_vector: " + d
    d = first_difference_rows(*g.find(q), *model.find(q))
    if d:
        return "find: " + d
    d = first_difference(*g.count(q), *model.count(q))
    return "count: " + d if d else None
