"""Plain numpy model of the queries in the caller's order (kmi_index_lookup_*, kmi_index_profile_reads_*) over tests/oracle.py and
tests/index_model.py. Everything here comes from the oracle's parser and from a CountModel; nothing from the GPU. Test-side only."""
import numpy as np

from tests import oracle as orc

# kmi_read_profile (include/kmerind_hip.h), field for field
ROW = np.dtype([("seq_offset", np.uint64), ("sum_counts", np.uint64), ("n_kmers", np.uint32), ("n_present", np.uint32),
                ("n_solid", np.uint32), ("lowest", np.uint32), ("highest", np.uint32), ("reserved", np.uint32)])


def _rows(a, nw):
    return [tuple(r) for r in np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, nw).tolist()]


def lookup(model, q):
    """counts[i] = the model's count of transform(q[i]), 0 when absent: one answer per query, in query order"""
    keys, counts = model.export()
    d = dict(zip(_rows(keys, model.nw), counts.tolist()))
    return np.array([d.get(t, 0) for t in _rows(model.transform(q), model.nw)], dtype=np.uint32)


def profile(data, s, model, solid):
    """one ROW per FASTQ record of `data`, in file order: the read's k-mers are the oracle's tuples whose id names the record
    (ShortSequenceKmerId: record offset << 16 | offset inside the record)"""
    recs = orc.records(data, orc.FASTQ)
    ex = orc.extract(s, data, orc.FASTQ, want_ids=True)
    counts = lookup(model, ex["kmers"]).astype(np.uint64)
    rec_of = ex["ids"] >> np.uint64(16)
    out = np.zeros(len(recs), dtype=ROW)
    for i, r in enumerate(recs):
        c = counts[rec_of == np.uint64(r.record_offset)]
        out[i]["seq_offset"] = r.seq_begin
        out[i]["n_kmers"] = c.size
        if c.size:
            out[i]["sum_counts"] = int(c.sum())
            out[i]["n_present"] = int((c > 0).sum())
            out[i]["n_solid"] = int((c >= solid).sum())
            out[i]["lowest"] = int(c.min())
            out[i]["highest"] = int(c.max())
    return out


def first_row_difference(got, want):
    """None when the two row arrays are equal, else a line naming the first row that differs"""
    if got.shape != want.shape:
        return "%d rows, expected %d" % (got.shape[0], want.shape[0])
    for i in range(want.shape[0]):
        if got[i] != want[i]:
            return "row %d: got %s, expected %s (fields %s)" % (i, got[i], want[i], ROW.names)
    return None
