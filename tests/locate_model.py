"""Dictionary model of the position indexes' queries in the caller's order (kmi_index_locate_*, kmi_index_seed_reads_*) over
tests/oracle.py's parser and strand transform and the tuples of tests/multimap_cases.py. Nothing here comes from the GPU.
Test-side only."""
import numpy as np

from tests import multimap_cases as MC
from tests import oracle as orc

LOCATE_ALL = 0xFFFFFFFF
# kmi_read_seeds (include/kmerind_hip.h), field for field
ROW = np.dtype([("seq_offset", np.uint64), ("first_kmer", np.uint64), ("n_kmers", np.uint32), ("n_listed", np.uint32),
                ("n_hits", np.uint64)])


def _rows(a, nw):
    return [tuple(r) for r in np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, nw).tolist()]


class LocateModel:
    """key (after the strand transform) -> list of value rows, every inserted tuple kept"""

    def __init__(self, s, strand=orc.CANONICAL, vw=1):
        self.s, self.strand, self.vw, self.d = s, strand, vw, {}

    def transform(self, kmers):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, self.s.n_words)
        return kmers if self.strand == orc.SINGLE else orc.canonical(self.s, kmers)

    def insert(self, kmers, values):
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, self.vw)
        for key, v in zip(_rows(self.transform(kmers), self.s.n_words), values.tolist()):
            self.d.setdefault(key, []).append(tuple(v))

    def build(self, data, fmt=orc.FASTQ, file_offset=0):
        self.insert(*MC.tuples_of(self.s, data, self.vw, fmt, file_offset))

    def size(self):
        return sum(len(v) for v in self.d.values())

    def multiplicities(self):
        return np.array(sorted(len(v) for v in self.d.values()), dtype=np.int64)

    def locate(self, q, max_occ=LOCATE_ALL):
        """(occ, offsets, per_query): occ[i] the true multiplicity of transform(q[i]); offsets the exclusive scan of the listed
        counts (occ where occ <= max_occ, else 0); per_query[i] the sorted value rows of query i, empty when it is not listed"""
        keys = _rows(self.transform(q), self.s.n_words)
        occ = np.array([len(self.d.get(key, ())) for key in keys], dtype=np.uint32)
        listed = np.where(occ.astype(np.uint64) <= np.uint64(max_occ), occ, 0).astype(np.uint64)
        offsets = np.zeros(len(keys) + 1, dtype=np.uint64)
        np.cumsum(listed, out=offsets[1:])
        per_query = [sorted(self.d[key]) if n else [] for key, n in zip(keys, listed.tolist())]
        return occ, offsets, per_query

    def seed_reads(self, data, max_occ=LOCATE_ALL):
        """(rows, occ, offsets, per_query) of a FASTQ buffer: the windows are the oracle's tuples, the reads its records; a tuple's
        id names its record (ShortSequenceKmerId: record offset << 16 | offset inside the record)"""
        recs = orc.records(data, orc.FASTQ)
        ex = orc.extract(self.s, data, orc.FASTQ, want_ids=True)
        occ, offsets, per_query = self.locate(ex["kmers"], max_occ)
        windows = dict(zip(*(a.tolist() for a in np.unique(ex["ids"] >> np.uint64(16), return_counts=True))))
        rows = np.zeros(len(recs), dtype=ROW)
        first = 0
        for i, r in enumerate(recs):
            n = windows.get(int(r.record_offset), 0)
            o = occ[first:first + n]
            rows[i] = (r.seq_begin, first, n, int(((o > 0) & (o.astype(np.uint64) <= np.uint64(max_occ))).sum()),
                       int(offsets[first + n] - offsets[first]))
            first += n
        assert first == occ.shape[0]   # the tuples come record by record, in file order
        return rows, occ, offsets, per_query


def values_difference(got_values, offsets, per_query):
    """None when values[offsets[i]:offsets[i + 1]], sorted, are the model's rows of every query i; else a line about the first
    query that differs"""
    got_values = np.asarray(got_values)
    if got_values.shape[0] != int(offsets[-1]):
        return "%d value rows, expected %d" % (got_values.shape[0], int(offsets[-1]))
    for i, want in enumerate(per_query):
        got = sorted(tuple(r) for r in got_values[int(offsets[i]):int(offsets[i + 1])].tolist())
        if got != want:
            return "query %d: got %d rows %s..., expected %d rows %s..." % (i, len(got), got[:2], len(want), want[:2])
    return None


def difference(got, want):
    """got = (occ, offsets, values) of the GPU, want = (occ, offsets, per_query) of the model: occ and offsets exactly, values per
    query as sorted rows"""
    for name, a, b in (("occ", got[0], want[0]), ("offsets", got[1], want[1])):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return "%s: %d words, expected %d" % (name, a.shape[0], b.shape[0])
        if (a != b).any():
            i = int(np.nonzero(a != b)[0][0])
            return "%s[%d]: got %d, expected %d" % (name, i, int(a[i]), int(b[i]))
    return values_difference(got[2], want[1], want[2])


def first_row_difference(got, want):
    """None when the two row arrays are equal, else a line naming the first row that differs"""
    if got.shape != want.shape:
        return "%d rows, expected %d" % (got.shape[0], want.shape[0])
    for i in range(want.shape[0]):
        if got[i] != want[i]:
            return "row %d: got %s, expected %s (fields %s)" % (i, got[i], want[i], ROW.names)
    return None
