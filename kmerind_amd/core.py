"""Host-side mirror of the reference's operator interface for the k-mer index path.

Names follow the reference: CountIndex.insert / count / find / erase / size / local_size /
build (bliss::index::kmer::Index, src/index/kmer_index.hpp:98-394) and
KmerFileHelper.read_file (src/io/kmer_file_helper.hpp:550-633) -> Context.read_file."""
import ctypes as C
import os

import numpy as np

from . import _lib as L

lib = L.lib


def make_config(k, alphabet="DNA", strand="canonical", dist_hash="murmur", store_hash="murmur",
                index_kind="count", seq_format="fastq", farm_ndebug=False, seq_filter="all", dist_trans="model"):
    alpha = {"DNA": L.ALPHA_DNA, "DNA5": L.ALPHA_DNA5, "DNA6": L.ALPHA_DNA5,
             "RNA": L.ALPHA_RNA, "RNA5": L.ALPHA_RNA5, "RNA6": L.ALPHA_RNA5, "DNA16": L.ALPHA_DNA16}[alphabet]
    st = {"single": L.STRAND_SINGLE, "canonical": L.STRAND_CANONICAL, "bimolecule": L.STRAND_BIMOLECULE}[strand]
    hs = {"murmur": L.HASH_MURMUR, "farm": L.HASH_FARM, "identity": L.HASH_IDENTITY, "std": L.HASH_STD}
    kind = {"count": L.INDEX_COUNT, "position": L.INDEX_POSITION, "posqual": L.INDEX_POSQUAL}[index_kind]
    fmt = {"fastq": L.FMT_FASTQ, "fasta": L.FMT_FASTA}[seq_format]
    flt = {"all": L.SEQ_ALL, "n_filter": L.SEQ_N_FILTER, "n_split": L.SEQ_N_SPLIT}[seq_filter]
    dt = {"model": L.DIST_MODEL, "lex_less": L.DIST_LEX, "xor_rev_comp": L.DIST_XOR}[dist_trans]
    return L.Config(k, alpha, st, hs[dist_hash], hs[store_hash], kind, fmt, int(bool(farm_ndebug)), flt, dt)


def _u64(a, n_words=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if n_words is not None:
        a = a.reshape(-1, n_words)
    return a


class Context:
    """One GPU = one rank (stands where the reference takes an mxx::comm)."""

    def __init__(self, device=0, rank=0, nranks=1, stream=None):
        h = C.c_void_p()
        st = lib.kmi_ctx_create(device, rank, nranks, C.c_void_p(stream or 0), C.byref(h))
        if st != L.OK:
            raise L.KmiError(st, "kmi_ctx_create failed (no usable HIP device? there is no CPU fallback)")
        self.h = h
        self.rank, self.nranks, self.device = rank, nranks, device
        self.stream = int(stream or 0)

    def close(self):
        if getattr(self, "h", None):
            lib.kmi_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, st):
        if st != L.OK:
            raise L.KmiError(st, (lib.kmi_last_error(self.h) or b"").decode())

    @staticmethod
    def shape(cfg):
        nw, nb, nby = C.c_uint32(), C.c_uint32(), C.c_uint32()
        if lib.kmi_kmer_shape(C.byref(cfg), C.byref(nw), C.byref(nb), C.byref(nby)) != L.OK:
            raise ValueError("invalid k-mer configuration")
        return nw.value, nb.value, nby.value

    # ---- device memory helpers (raw pointers; bench.py may pass torch data_ptr() instead)
    def alloc(self, nbytes):
        p = C.c_void_p()
        self.check(lib.kmi_device_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def free(self, dptr):
        self.check(lib.kmi_device_free(self.h, C.c_void_p(dptr)))

    def to_device(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self.check(lib.kmi_copy_to_device(self.h, C.c_void_p(dptr), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def to_host(self, arr, dptr):
        self.check(lib.kmi_copy_to_host(self.h, arr.ctypes.data_as(C.c_void_p), C.c_void_p(dptr), arr.nbytes))

    def synchronize(self):
        self.check(lib.kmi_synchronize(self.h))

    # ---- array-level k-mer ops
    def _array_op(self, fn, cfg, kmers, out_dtype, per_key, *extra):
        nw = self.shape(cfg)[0]
        kmers = _u64(kmers, nw)
        n = kmers.shape[0]
        out = np.zeros((n, nw) if per_key else n, dtype=out_dtype)
        self.check(fn(self.h, C.byref(cfg), *extra[:2], kmers.ctypes.data_as(C.c_void_p), n, *extra[2:],
                      out.ctypes.data_as(C.c_void_p)))
        return out

    def revcomp(self, cfg, kmers):
        return self._array_op(lib.kmi_revcomp_host, cfg, kmers, np.uint64, True)

    def canonical(self, cfg, kmers):
        return self._array_op(lib.kmi_canonical_host, cfg, kmers, np.uint64, True)

    def hash(self, cfg, which, prefix, kmers):
        which = {"murmur": L.HASH_MURMUR, "farm": L.HASH_FARM, "identity": L.HASH_IDENTITY, "std": L.HASH_STD}.get(which, which)
        return self._array_op(lib.kmi_hash_host, cfg, kmers, np.uint64, False, which, int(prefix))

    def key_to_rank(self, cfg, kmers, nranks):
        nw = self.shape(cfg)[0]
        kmers = _u64(kmers, nw)
        out = np.zeros(kmers.shape[0], dtype=np.uint32)
        self.check(lib.kmi_key_to_rank_host(self.h, C.byref(cfg), kmers.ctypes.data_as(C.c_void_p), kmers.shape[0],
                                            nranks, out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- KmerFileHelper::read_file_* equivalent on an in-memory, record-aligned partition
    def read_file(self, cfg, data, file_offset=0, with_ids=False, with_quals=False, fasta_block=None):
        """returns (kmers[n, n_words], n_seqs) in file order, as parsed (no strand transform);
        with_ids (position index kinds): (kmers, ids, n_seqs), ids = Short/LongSequenceKmerId words.
        fasta_block = (rank, nranks): `data` is a WHOLE FASTA file and the tuples of that rank's block of an equal split come back
        (kmi_extract_fasta_block_host: what read_file_* does on one rank of several)"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else \
            np.ascontiguousarray(data, dtype=np.uint8)
        t = L.Tuples()
        if fasta_block is not None:
            self.check(lib.kmi_extract_fasta_block_host(self.h, C.byref(cfg), buf.ctypes.data_as(C.c_void_p), buf.size,
                                                        int(fasta_block[0]), int(fasta_block[1]), C.byref(t)))
        else:
            self.check(lib.kmi_extract_host(self.h, C.byref(cfg), buf.ctypes.data_as(C.c_void_p), buf.size, file_offset,
                                            C.byref(t)))
        nw = self.shape(cfg)[0]
        n = t.n_tuples
        kmers = np.ctypeslib.as_array(t.kmers, shape=(n * nw,)).copy().reshape(n, nw) if n else \
            np.zeros((0, nw), dtype=np.uint64)
        nseq = t.n_seqs
        ids = None
        if with_ids:
            if not t.ids:
                lib.kmi_tuples_free(C.byref(t))
                raise ValueError("ids need a position index kind in the config")
            ids = np.ctypeslib.as_array(t.ids, shape=(n,)).copy() if n else np.zeros(0, dtype=np.uint64)
        if with_quals and not with_ids:
            with_ids = True
        quals = None
        if with_quals:
            if not t.quals:
                lib.kmi_tuples_free(C.byref(t))
                raise ValueError("qualities need index_kind='posqual'")
            quals = np.ctypeslib.as_array(t.quals, shape=(n,)).copy() if n else np.zeros(0, dtype=np.float32)
        lib.kmi_tuples_free(C.byref(t))
        if with_quals:
            return kmers, ids, quals, nseq
        if with_ids:
            return kmers, ids, nseq
        return kmers, nseq

    def set_fasta_partition(self, part=None):
        """what FASTAParser::init_parser learns from the neighbouring ranks, for the next FASTA extract / build calls
        (a dict from kmerind_amd.fileio.partition_fasta); None = whole file"""
        if part is None:
            self.check(lib.kmi_ctx_set_fasta_partition(self.h, None))
            return
        fp = L.FastaPartition(part["valid_bytes"], part["start_state"], part["at_line_start"], part["records_before"],
                              part["index_shift"], 0)
        self.check(lib.kmi_ctx_set_fasta_partition(self.h, C.byref(fp)))

    def debug_counter(self, which):
        """kmi_ctx_debug_counter: the counters the library keeps for its tests and for diagnosis"""
        v = C.c_uint64()
        self.check(lib.kmi_ctx_debug_counter(self.h, which, C.byref(v)))
        return v.value

    # ---- profiling
    def profile(self, on=True):
        self.check(lib.kmi_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self.check(lib.kmi_profile_reset(self.h))

    def profile_get(self):
        arr = (L.KernelTime * 64)()
        n = C.c_size_t()
        self.check(lib.kmi_profile_get(self.h, arr, 64, C.byref(n)))
        return [{"name": arr[i].name.decode(), "total_ms": arr[i].total_ms, "launches": arr[i].launches,
                 "units": arr[i].units} for i in range(min(n.value, 64))]


# kmi_read_profile (kmerind_hip.h), field for field: 40 bytes per read
READ_PROFILE_DTYPE = np.dtype([("seq_offset", np.uint64), ("sum_counts", np.uint64), ("n_kmers", np.uint32), ("n_present", np.uint32),
                               ("n_solid", np.uint32), ("lowest", np.uint32), ("highest", np.uint32), ("reserved", np.uint32)])
assert READ_PROFILE_DTYPE.itemsize == 40
# kmi_read_seeds (kmerind_hip.h), field for field: 32 bytes per read
READ_SEEDS_DTYPE = np.dtype([("seq_offset", np.uint64), ("first_kmer", np.uint64), ("n_kmers", np.uint32), ("n_listed", np.uint32),
                             ("n_hits", np.uint64)])
assert READ_SEEDS_DTYPE.itemsize == 32


def num_buckets():
    return int(lib.kmi_index_num_buckets())


class CountIndex:
    """bliss::index::kmer::CountIndex<counting map> on one rank (kmer_index.hpp:409-410)."""

    def __init__(self, ctx, cfg):
        self.ctx, self.cfg = ctx, cfg
        self.n_words = ctx.shape(cfg)[0]
        h = C.c_void_p()
        ctx.check(lib.kmi_index_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):   # (a context that is gone took the device blocks with it: nothing to hand back through it)
                lib.kmi_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def insert(self, kmers):
        kmers = _u64(kmers, self.n_words)
        self.ctx.check(lib.kmi_index_insert_host(self.h, kmers.ctypes.data_as(C.c_void_p), kmers.shape[0]))

    def insert_pairs(self, kmers, counts):
        """Index::insert(vector<pair<Kmer, count>>): every pair's count is added (distributed_unordered_map.hpp:1603-1618)"""
        kmers = _u64(kmers, self.n_words)
        rec = np.zeros((kmers.shape[0], self.n_words + 1), dtype=np.uint64)
        rec[:, :self.n_words] = kmers
        rec[:, self.n_words] = np.asarray(counts, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
        self.ctx.check(lib.kmi_index_insert_pairs_host(self.h, rec.ctypes.data_as(C.c_void_p), rec.shape[0]))

    def update_pairs(self, kmers, values, op="add"):
        """update(pairs, op) with a device-side updater (add / max / min / assign): stored keys only -> number of pairs applied"""
        kmers = _u64(kmers, self.n_words)
        rec = np.zeros((kmers.shape[0], self.n_words + 1), dtype=np.uint64)
        rec[:, :self.n_words] = kmers
        rec[:, self.n_words] = np.asarray(values, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
        n = C.c_uint64()
        code = {"add": 0, "max": 1, "min": 2, "assign": 3}[op]
        self.ctx.check(lib.kmi_index_update_pairs_host(self.h, rec.ctypes.data_as(C.c_void_p), rec.shape[0], code, C.byref(n)))
        return n.value

    def insert_device(self, dptr, n, transformed=False):
        """transformed=True: the keys already went through the InputTransform (routed keys after the exchange)"""
        fn = lib.kmi_index_insert_transformed_dev if transformed else lib.kmi_index_insert_dev
        self.ctx.check(fn(self.h, C.c_void_p(dptr), n))

    def build(self, data, file_offset=0):
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else \
            np.ascontiguousarray(data, dtype=np.uint8)
        self.ctx.check(lib.kmi_index_build_host(self.h, buf.ctypes.data_as(C.c_void_p), buf.size, file_offset))

    def build_device(self, dptr, nbytes, file_offset=0):
        self.ctx.check(lib.kmi_index_build_dev(self.h, C.c_void_p(dptr), nbytes, file_offset))

    def clear(self):
        self.ctx.check(lib.kmi_index_clear(self.h))

    def local_size(self):
        n = C.c_uint64()
        self.ctx.check(lib.kmi_index_local_size(self.h, C.byref(n)))
        return n.value

    size = local_size  # single-rank view; kmerind_amd.dist adds the all-reduce

    def owner_ranks(self):
        """1, or the rank count of the build through exchanged super-k-mers that filled this index (kmi_index_sk_consume_dev)"""
        n = C.c_uint32()
        self.ctx.check(lib.kmi_index_owner_ranks(self.h, C.byref(n)))
        return n.value

    # combine-first distributed insert (kmerind_hip.h): split the entries by destination rank / merge received parts
    def split_by_rank_device(self, nranks, keys_dptr, counts_dptr, capacity, bucket_counts_dptr):
        """-> send counts per rank (numpy uint64). Device buffers: keys [capacity * n_words] u64, counts [capacity] u32,
        bucket counts [nranks * num_buckets()] u32."""
        sc = np.zeros(nranks, dtype=np.uint64)
        self.ctx.check(lib.kmi_index_split_by_rank_dev(self.h, nranks, C.c_void_p(keys_dptr), C.c_void_p(counts_dptr), capacity,
                                                       C.c_void_p(bucket_counts_dptr), sc.ctypes.data_as(C.c_void_p)))
        return sc

    def merge_parts_device(self, nparts, keys_dptr, counts_dptr, bucket_counts_dptr):
        self.ctx.check(lib.kmi_index_merge_parts_dev(self.h, nparts, C.c_void_p(keys_dptr), C.c_void_p(counts_dptr),
                                                     C.c_void_p(bucket_counts_dptr)))

    def to_vector(self):
        n = self.local_size()
        keys = np.zeros((n, self.n_words), dtype=np.uint64)
        counts = np.zeros(n, dtype=np.uint32)
        got = C.c_uint64()
        self.ctx.check(lib.kmi_index_export_host(self.h, keys.ctypes.data_as(C.c_void_p),
                                                 counts.ctypes.data_as(C.c_void_p), n, C.byref(got)))
        return keys[:got.value], counts[:got.value]

    def _query(self, fn, q):
        q = _u64(q, self.n_words)
        r = L.Results()
        self.ctx.check(fn(self.h, q.ctypes.data_as(C.c_void_p), q.shape[0], C.byref(r)))
        n = r.n
        if n:
            keys = np.ctypeslib.as_array(r.keys, shape=(n * self.n_words,)).copy().reshape(n, self.n_words)
            vals = np.ctypeslib.as_array(r.values, shape=(n,)).copy()
        else:
            keys = np.zeros((0, self.n_words), dtype=np.uint64)
            vals = np.zeros(0, dtype=np.uint64)
        lib.kmi_results_free(C.byref(r))
        return keys, vals

    def count(self, q):
        return self._query(lib.kmi_index_count_host, q)

    def find(self, q):
        return self._query(lib.kmi_index_find_host, q)

    def exists(self, q):
        """densehash exists() (distributed_densehash_map.hpp:1465-1560): one byte per input key, in input order"""
        q = _u64(q, self.n_words)
        keys, cnt = self.count(q)
        tq = q if self.cfg.strand == L.STRAND_SINGLE else self.ctx.canonical(self.cfg, q)
        have = {tuple(k) for k, c in zip(keys.tolist(), np.asarray(cnt).reshape(len(keys), -1)[:, 0].tolist()) if c}
        return np.fromiter((tuple(k) in have for k in tq.tolist()), dtype=np.uint8, count=tq.shape[0])

    def erase(self, q):
        q = _u64(q, self.n_words)
        n = C.c_uint64()
        self.ctx.check(lib.kmi_index_erase_host(self.h, q.ctypes.data_as(C.c_void_p), q.shape[0], C.byref(n)))
        return n.value

    # ---- queries in the caller's order (no reference counterpart; a position index refuses them)
    def _over(self, comm):
        """the leading arguments of a query: the index, and the communicator of its collective form (anything with a kmi_comm
        handle `h`)"""
        return (self.h,) if comm is None else (self.h, comm.h)

    def lookup(self, q, comm=None):
        """counts[i] = the count stored for the transformed q[i], 0 when absent: one answer per query, in query order. With a
        communicator the answers come from the entries of all ranks: collective, every rank with its own queries."""
        q = _u64(q, self.n_words)
        out = np.zeros(q.shape[0], dtype=np.uint32)
        fn = lib.kmi_index_lookup_host if comm is None else lib.kmi_index_lookup_dist_host
        self.ctx.check(fn(*self._over(comm), q.ctypes.data_as(C.c_void_p), q.shape[0], out.ctypes.data_as(C.c_void_p)))
        return out

    def lookup_device(self, q_dptr, n, out_dptr, comm=None):
        """q_dptr: n k-mers of n_words u64 on the device; out_dptr: n u32 counts"""
        fn = lib.kmi_index_lookup_dev if comm is None else lib.kmi_index_lookup_dist_dev
        self.ctx.check(fn(*self._over(comm), C.c_void_p(q_dptr), n, C.c_void_p(out_dptr)))

    def profile_reads(self, data, solid=2, comm=None):
        """one row (READ_PROFILE_DTYPE) per FASTQ record of `data`, in file order: how many of the read's k-mers the index
        holds, how many of them at least `solid` times, and the lowest / highest / summed count. With a communicator the counts
        come from the entries of all ranks: collective, every rank with its own record-aligned share (a sizing call, then the
        filling call, on every rank)."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else \
            np.ascontiguousarray(data, dtype=np.uint8)
        n = C.c_uint64()
        if comm is not None:
            head = (self.h, comm.h, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, solid)
            st = lib.kmi_index_profile_reads_dist_host(*head, None, 0, C.byref(n))
            if not (st == L.ERR_OVERFLOW and n.value > 0):   # (rows and no room for them: what the sizing call is for)
                self.ctx.check(st)
            out = np.zeros(n.value, dtype=READ_PROFILE_DTYPE)
            self.ctx.check(lib.kmi_index_profile_reads_dist_host(*head, out.ctypes.data_as(C.c_void_p) if n.value else None, n.value, C.byref(n)))
            return out
        cap = int(np.count_nonzero((buf == 10) | (buf == 13))) // 4 + 2   # (every record but the last ends four lines)
        while True:
            out = np.zeros(cap, dtype=READ_PROFILE_DTYPE)
            st = lib.kmi_index_profile_reads_host(self.h, buf.ctypes.data_as(C.c_void_p), buf.size, solid,
                                                  out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
            if st == L.ERR_OVERFLOW and n.value > cap:
                cap = n.value
                continue
            self.ctx.check(st)
            return out[:n.value].copy()

    def profile_reads_device(self, dptr, nbytes, out_dptr, capacity, solid=2, comm=None):
        """dptr: FASTQ bytes on the device; out_dptr: room for `capacity` rows of 40 bytes -> number of records"""
        n = C.c_uint64()
        fn = lib.kmi_index_profile_reads_dev if comm is None else lib.kmi_index_profile_reads_dist_dev
        st = fn(*self._over(comm), C.c_void_p(dptr) if dptr else None, nbytes, solid, C.c_void_p(out_dptr) if out_dptr else None, capacity,
                C.byref(n))
        if st != L.OK:
            err = L.KmiError(st, (lib.kmi_last_error(self.ctx.h) or b"").decode())
            err.n_reads = n.value
            raise err
        return n.value

    # ---- the count spectrum and the filter by count (kmi_index_spectrum_* / kmi_index_retain_counts)
    @staticmethod
    def _totals(t):
        return {"n_entries": t.n_entries, "sum_counts": t.sum_counts, "min_count": t.min_count, "max_count": t.max_count}

    def spectrum(self, n_bins=256):
        """(hist, totals): hist[min(count, n_bins - 1)] counts the stored entries (np.uint64[n_bins]); totals is a dict of
        n_entries, sum_counts, min_count, max_count"""
        hist = np.ones(max(int(n_bins), 0), dtype=np.uint64)
        t = L.SpectrumTotals()
        self.ctx.check(lib.kmi_index_spectrum_host(self.h, n_bins, hist.ctypes.data_as(C.c_void_p), C.byref(t)))
        return hist, self._totals(t)

    def spectrum_device(self, hist_dptr, n_bins):
        """hist_dptr: room for n_bins u64 on the device (cleared by the call) -> totals"""
        t = L.SpectrumTotals()
        self.ctx.check(lib.kmi_index_spectrum_dev(self.h, n_bins, C.c_void_p(hist_dptr), C.byref(t)))
        return self._totals(t)

    def retain_counts(self, lo, hi=2**32 - 1):
        """keeps the entries with lo <= count <= hi, on the device -> number of entries erased"""
        n = C.c_uint64()
        self.ctx.check(lib.kmi_index_retain_counts(self.h, lo, hi, C.byref(n)))
        return n.value

    # ---- two count indexes compared and combined on the device (kmi_index_compare* / kmi_index_combine)
    @staticmethod
    def _overlap(o):
        d = {name: int(getattr(o, name)) for name, _ in L.IndexOverlap._fields_}

        def ratio(num, den):
            return num / den if den else 0.0
        d["jaccard"] = ratio(d["n_shared"], d["n_a"] + d["n_b"] - d["n_shared"])
        d["containment_a"] = ratio(d["n_shared"], d["n_a"])
        d["containment_b"] = ratio(d["n_shared"], d["n_b"])
        d["weighted_jaccard"] = ratio(d["sum_min_shared"], d["sum_a"] + d["sum_b"] - d["sum_min_shared"])
        return d

    def compare(self, other, comm=None):
        """the overlap of this index (a) and `other` (b): a dict of the eight words of kmi_index_overlap plus jaccard,
        containment_a, containment_b and weighted_jaccard as floats (0.0 where the denominator is 0). With a communicator
        (anything with a kmi_comm handle `h`) the words are summed over the ranks: collective."""
        o = L.IndexOverlap()
        if comm is None:
            self.ctx.check(lib.kmi_index_compare(self.h, other.h, C.byref(o)))
        else:
            self.ctx.check(lib.kmi_index_compare_dist_host(self.h, other.h, comm.h, C.byref(o)))
        return self._overlap(o)

    def combine(self, other, op):
        """this index := this index (op) other, on the device; op is one of union_add, union_max, intersect_min, intersect_add,
        intersect_left, subtract_keys, subtract_counts -> the new size"""
        if isinstance(op, str):
            if op not in L.COMBINE_OPS:
                raise ValueError("combine: unknown op %r" % (op,))
            op = L.COMBINE_OPS[op]
        n = C.c_uint64()
        self.ctx.check(lib.kmi_index_combine(self.h, other.h, op, C.byref(n)))
        return n.value


class PositionIndex(CountIndex):
    """bliss::index::kmer::PositionIndex<unordered_multimap> on one rank (kmer_index.hpp:402-403):
    every (k-mer, ShortSequenceKmerId) tuple is kept."""

    def __init__(self, ctx, cfg):
        if cfg.index_kind == L.INDEX_COUNT:
            raise ValueError("PositionIndex needs index_kind='position'")
        super().__init__(ctx, cfg)
        self.value_words = 1 if cfg.index_kind == L.INDEX_POSITION else 2

    def insert(self, kmers, values):
        kmers = _u64(kmers, self.n_words)
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(kmers.shape[0], self.value_words)
        self.ctx.check(lib.kmi_index_insert_tuples_host(self.h, kmers.ctypes.data_as(C.c_void_p),
                                                        values.ctypes.data_as(C.c_void_p), kmers.shape[0]))

    def to_vector(self):
        n = self.local_size()
        keys = np.zeros((n, self.n_words), dtype=np.uint64)
        vals = np.zeros((n, self.value_words), dtype=np.uint64)
        got = C.c_uint64()
        self.ctx.check(lib.kmi_index_export_tuples_host(self.h, keys.ctypes.data_as(C.c_void_p),
                                                        vals.ctypes.data_as(C.c_void_p), n, C.byref(got)))
        return keys[:got.value], vals[:got.value]

    def _query(self, fn, q):
        q = _u64(q, self.n_words)
        r = L.Results()
        self.ctx.check(fn(self.h, q.ctypes.data_as(C.c_void_p), q.shape[0], C.byref(r)))
        n, vw = r.n, self.value_words
        if n:
            keys = np.ctypeslib.as_array(r.keys, shape=(n * self.n_words,)).copy().reshape(n, self.n_words)
            vals = np.ctypeslib.as_array(r.values, shape=(n * vw,)).copy().reshape(n, vw)
        else:
            keys = np.zeros((0, self.n_words), dtype=np.uint64)
            vals = np.zeros((0, vw), dtype=np.uint64)
        lib.kmi_results_free(C.byref(r))
        return keys, vals

    def count(self, q):
        keys, vals = self._query(lib.kmi_index_count_host, q)
        return keys, vals[:, 0]

    # ---- queries in the caller's order (kmi_index_locate_* / kmi_index_seed_reads_*; no reference counterpart)
    def _raise(self, st, **totals):
        err = L.KmiError(st, (lib.kmi_last_error(self.ctx.h) or b"").decode())
        for name, v in totals.items():
            setattr(err, name, v)
        raise err

    def locate(self, q, max_occ=None, comm=None):
        """(occ, offsets, values): occ[i] = entries under the transformed q[i]; values[offsets[i]:offsets[i + 1]] = their value
        rows (shape (n_hits, value_words)) when occ[i] <= max_occ, nothing otherwise. One answer per query, in query order. With a
        communicator the answers come from the entries of all ranks: collective, every rank with its own queries (a sizing call,
        then the filling call, on every rank)."""
        q = _u64(q, self.n_words)
        nq = q.shape[0]
        max_occ = L.LOCATE_ALL if max_occ is None else int(max_occ)
        occ = np.zeros(nq, dtype=np.uint32)
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        n = C.c_uint64()
        fn = lib.kmi_index_locate_host if comm is None else lib.kmi_index_locate_dist_host
        args = (*self._over(comm), q.ctypes.data_as(C.c_void_p), nq, max_occ, occ.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p))
        self.ctx.check(fn(*args, None, 0, C.byref(n)))   # the sizing call
        values = np.zeros((n.value, self.value_words), dtype=np.uint64)
        if n.value or comm is not None:   # (over ranks the filling call is every rank's, also a rank's without a hit)
            self.ctx.check(fn(*args, values.ctypes.data_as(C.c_void_p) if n.value else None, n.value, C.byref(n)))
        return occ, offsets, values

    def locate_device(self, q_dptr, n, occ_dptr, offsets_dptr, values_dptr=0, capacity=0, max_occ=None, comm=None):
        """q_dptr: n k-mers on the device; occ_dptr: n u32; offsets_dptr: n + 1 u64; values_dptr: room for `capacity` hits of
        value_words u64 (0 with capacity 0: the sizing call) -> number of listed hits"""
        max_occ = L.LOCATE_ALL if max_occ is None else int(max_occ)
        hits = C.c_uint64()
        fn = lib.kmi_index_locate_dev if comm is None else lib.kmi_index_locate_dist_dev
        st = fn(*self._over(comm), C.c_void_p(q_dptr), n, max_occ, C.c_void_p(occ_dptr), C.c_void_p(offsets_dptr),
                C.c_void_p(values_dptr) if values_dptr else None, capacity, C.byref(hits))
        if st != L.OK:
            self._raise(st, n_hits=hits.value)
        return hits.value

    def seed_reads(self, data, max_occ=None, comm=None):
        """(rows, occ, offsets, values): one row (READ_SEEDS_DTYPE) per FASTQ record of `data`, in file order; window j of read r
        is query rows[r]['first_kmer'] + j of the locate() arrays over all windows of the buffer. With a communicator the hits
        come from the entries of all ranks: collective, every rank with its own record-aligned share."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else \
            np.ascontiguousarray(data, dtype=np.uint8)
        max_occ = L.LOCATE_ALL if max_occ is None else int(max_occ)
        nr, nk, nh = C.c_uint64(), C.c_uint64(), C.c_uint64()
        tail = (C.byref(nr), C.byref(nk), C.byref(nh))
        fn = lib.kmi_index_seed_reads_host if comm is None else lib.kmi_index_seed_reads_dist_host
        head = (*self._over(comm), buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, max_occ)
        self.ctx.check(fn(*head, None, 0, None, None, 0, None, 0, *tail))   # the sizing call
        rows = np.zeros(nr.value, dtype=READ_SEEDS_DTYPE)
        occ = np.zeros(nk.value, dtype=np.uint32)
        offsets = np.zeros(nk.value + 1, dtype=np.uint64)
        values = np.zeros((nh.value, self.value_words), dtype=np.uint64)

        def ptr(a):
            return a.ctypes.data_as(C.c_void_p) if a.size else None
        self.ctx.check(fn(*head, ptr(rows), rows.size, ptr(occ), offsets.ctypes.data_as(C.c_void_p), occ.size, ptr(values), values.shape[0], *tail))
        return rows, occ, offsets, values

    def seed_reads_device(self, dptr, nbytes, rows_dptr=0, cap_reads=0, occ_dptr=0, offsets_dptr=0, cap_kmers=0, values_dptr=0, cap_hits=0,
                          max_occ=None, comm=None):
        """dptr: FASTQ bytes on the device; rows_dptr: room for cap_reads rows of 32 bytes; occ_dptr: cap_kmers u32; offsets_dptr:
        cap_kmers + 1 u64; values_dptr: cap_hits hits of value_words u64 (all 0: the sizing call) -> (n_reads, n_kmers, n_hits)"""
        max_occ = L.LOCATE_ALL if max_occ is None else int(max_occ)
        nr, nk, nh = C.c_uint64(), C.c_uint64(), C.c_uint64()

        def ptr(p):
            return C.c_void_p(p) if p else None
        fn = lib.kmi_index_seed_reads_dev if comm is None else lib.kmi_index_seed_reads_dist_dev
        st = fn(*self._over(comm), ptr(dptr), nbytes, max_occ, ptr(rows_dptr), cap_reads, ptr(occ_dptr), ptr(offsets_dptr), cap_kmers,
                ptr(values_dptr), cap_hits, C.byref(nr), C.byref(nk), C.byref(nh))
        if st != L.OK:
            self._raise(st, n_reads=nr.value, n_kmers=nk.value, n_hits=nh.value)
        return nr.value, nk.value, nh.value


class DeBruijnNodes:
    """de_bruijn_engine<NodeMap> on one rank (test/test/debruijn/de_bruijn_construct_engine.hpp:241-245): nodes =
    (k-mer, [out A C G T, in A C G T, occurrences]); exists_only = node::edge_exists (0 / 1 per edge, no occurrence count).
    Every node is kept under its lexicographically smaller strand (include/kmerind_hip.h)."""

    def __init__(self, ctx, cfg, exists_only=False):
        self.ctx, self.cfg = ctx, cfg
        self.n_words = ctx.shape(cfg)[0]
        h = C.c_void_p()
        ctx.check(lib.kmi_dbg_create(ctx.h, C.byref(cfg), 1 if exists_only else 0, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):   # (a context that is gone took the device blocks with it: destroying the graph would reach into it)
                lib.kmi_dbg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def parse(self, data):
        """de_bruijn_parser over a FASTQ buffer -> (k-mers as parsed, edge bytes)"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        d = self.ctx.alloc(buf.size + 64)
        try:
            self.ctx.to_device(d, buf)
            n = C.c_uint64()
            self.ctx.check(lib.kmi_dbg_parse_dev(self.ctx.h, C.byref(self.cfg), C.c_void_p(d), buf.size, None, 0, C.byref(n)))
            rec = np.zeros((n.value, self.n_words + 1), dtype=np.uint64)
            if n.value:
                dr = self.ctx.alloc(rec.nbytes)
                try:
                    self.ctx.check(lib.kmi_dbg_parse_dev(self.ctx.h, C.byref(self.cfg), C.c_void_p(d), buf.size, C.c_void_p(dr), n.value, C.byref(n)))
                    self.ctx.to_host(rec, dr)
                finally:
                    self.ctx.free(dr)
        finally:
            self.ctx.free(d)
        return rec[:, :self.n_words].copy(), rec[:, self.n_words].astype(np.uint8)

    def build(self, data):
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        self.ctx.check(lib.kmi_dbg_build_host(self.h, buf.ctypes.data_as(C.c_void_p), buf.size))

    def build_device(self, dptr, nbytes):
        self.ctx.check(lib.kmi_dbg_build_dev(self.h, C.c_void_p(dptr), nbytes))

    def build_dist(self, data, comm):
        """Collective build over the ranks of `comm` (transport.GroupComm, or anything with the kmi_comm handle in `.h`): `data` is
        this rank's record-aligned share of the input; every node goes to the rank KeyToRank gives its canonical k-mer
        (kmi_dbg_build_dist_host). A rank with nothing passes b""."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        self.ctx.check(lib.kmi_dbg_build_dist_host(self.h, comm.h, buf.ctypes.data_as(C.c_void_p), buf.size))

    def insert(self, kmers, edges):
        """insert(vector<pair<Kmer, uint8_t>>): tuples as the parser emits them, either strand"""
        kmers = _u64(kmers, self.n_words)
        rec = np.zeros((kmers.shape[0], self.n_words + 1), dtype=np.uint64)
        rec[:, :self.n_words] = kmers
        rec[:, self.n_words] = np.asarray(edges, dtype=np.uint64) & np.uint64(0xFF)
        self.ctx.check(lib.kmi_dbg_insert_host(self.h, rec.ctypes.data_as(C.c_void_p), rec.shape[0]))

    def clear(self):
        self.ctx.check(lib.kmi_dbg_clear(self.h))

    def erase(self, q):
        """erase(keys): the nodes of these k-mers (either strand) leave the map; returns how many did"""
        q = _u64(q, self.n_words)
        n = C.c_uint64()
        self.ctx.check(lib.kmi_dbg_erase_host(self.h, q.ctypes.data_as(C.c_void_p), q.shape[0], C.byref(n)))
        return n.value

    def local_size(self):
        n = C.c_uint64()
        self.ctx.check(lib.kmi_dbg_local_size(self.h, C.byref(n)))
        return n.value

    size = local_size

    def to_vector(self):
        n = self.local_size()
        keys = np.zeros((n, self.n_words), dtype=np.uint64)
        counts = np.zeros((n, 9), dtype=np.uint32)
        got = C.c_uint64()
        self.ctx.check(lib.kmi_dbg_export_host(self.h, keys.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), n, C.byref(got)))
        return keys[:got.value], counts[:got.value]

    def find(self, q):
        q = _u64(q, self.n_words)
        r = L.Results()
        self.ctx.check(lib.kmi_dbg_find_host(self.h, q.ctypes.data_as(C.c_void_p), q.shape[0], C.byref(r)))
        n = r.n
        if n:
            keys = np.ctypeslib.as_array(r.keys, shape=(n * self.n_words,)).copy().reshape(n, self.n_words)
            vals = np.ctypeslib.as_array(r.values, shape=(n * 5,)).copy().view(np.uint32).reshape(n, 10)[:, :9].copy()
        else:
            keys = np.zeros((0, self.n_words), dtype=np.uint64)
            vals = np.zeros((0, 9), dtype=np.uint32)
        lib.kmi_results_free(C.byref(r))
        return keys, vals

    def count(self, q):
        q = _u64(q, self.n_words)
        r = L.Results()
        self.ctx.check(lib.kmi_dbg_count_host(self.h, q.ctypes.data_as(C.c_void_p), q.shape[0], C.byref(r)))
        n = r.n
        keys = np.ctypeslib.as_array(r.keys, shape=(n * self.n_words,)).copy().reshape(n, self.n_words) if n else np.zeros((0, self.n_words), np.uint64)
        vals = np.ctypeslib.as_array(r.values, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
        lib.kmi_results_free(C.byref(r))
        return keys, vals

    def unitigs(self, min_edge_count=1, comm=None):
        """Compacts the map on the device (kmi_dbg_compact; the definition is in include/kmerind_hip.h) ->
        (offsets: uint64[n + 1], bases: uint8[offsets[-1]] (ASCII letters), occurrences: uint64[n], circular: bool[n]).
        Unitig i is bases[offsets[i]:offsets[i + 1]]. With `comm` (transport.GroupComm, or anything with the kmi_comm handle in
        `.h`) the call is collective (kmi_dbg_compact_dist_host): the graph is the union of the ranks' maps and the arrays are the
        unitigs this rank holds; the counts over all ranks are left in `self.unitig_totals` as (unitigs, bases)."""
        nu, nb = C.c_uint64(), C.c_uint64()
        if comm is not None:
            tu, tb = C.c_uint64(), C.c_uint64()
            self.ctx.check(lib.kmi_dbg_compact_dist_host(self.h, comm.h, int(min_edge_count), C.byref(nu), C.byref(nb), C.byref(tu), C.byref(tb)))
            self.unitig_totals = (tu.value, tb.value)
        else:
            self.ctx.check(lib.kmi_dbg_compact(self.h, int(min_edge_count), C.byref(nu), C.byref(nb)))
            self.unitig_totals = (nu.value, nb.value)
        offsets = np.zeros(nu.value + 1, dtype=np.uint64)
        bases = np.zeros(max(nb.value, 1), dtype=np.uint8)
        occ = np.zeros(max(nu.value, 1), dtype=np.uint64)
        circ = np.zeros(max(nu.value, 1), dtype=np.uint8)
        self.ctx.check(lib.kmi_dbg_unitigs_export_host(self.h, offsets.ctypes.data_as(C.c_void_p), bases.ctypes.data_as(C.c_void_p),
                                                       occ.ctypes.data_as(C.c_void_p), circ.ctypes.data_as(C.c_void_p),
                                                       nu.value, nb.value))
        return offsets, bases[:nb.value], occ[:nu.value], circ[:nu.value].astype(bool)

    # ---- cleaning the map on the device (kmi_dbg_spectrum_* / kmi_dbg_retain_counts / kmi_dbg_prune_edges* / kmi_dbg_clip_tips / kmi_dbg_pop_bubbles)
    def spectrum(self, n_bins=256, comm=None):
        """(hist, totals) of the nodes' occurrence counts (counts[8]): hist[min(count, n_bins - 1)] counts the nodes
        (np.uint64[n_bins]); totals is a dict of n_entries, sum_counts, min_count, max_count. With `comm` the call is collective and
        both are summed over the ranks (kmi_dbg_spectrum_dist_host)."""
        hist = np.ones(max(int(n_bins), 0), dtype=np.uint64)
        t = L.SpectrumTotals()
        if comm is not None:
            self.ctx.check(lib.kmi_dbg_spectrum_dist_host(self.h, comm.h, n_bins, hist.ctypes.data_as(C.c_void_p), C.byref(t)))
        else:
            self.ctx.check(lib.kmi_dbg_spectrum_host(self.h, n_bins, hist.ctypes.data_as(C.c_void_p), C.byref(t)))
        return hist, {"n_entries": t.n_entries, "sum_counts": t.sum_counts, "min_count": t.min_count, "max_count": t.max_count}

    def retain_counts(self, lo, hi=2**32 - 1):
        """keeps the nodes with lo <= occurrences <= hi, on the device; the rest leave with their edge counters (their neighbours'
        counters stay: prune_edges) -> number of nodes erased. Local on every rank of a map held over ranks."""
        n = C.c_uint64()
        self.ctx.check(lib.kmi_dbg_retain_counts(self.h, lo, hi, C.byref(n)))
        return n.value

    def prune_edges(self, min_edge_count=1, comm=None):
        """Clears every edge counter that is below min_edge_count, leads to a k-mer that is not a node, or is not reciprocated by
        its neighbour (kmi_dbg_prune_edges; the definition is in include/kmerind_hip.h) -> dict of the kmi_dbg_prune_stats words.
        With `comm` the call is collective over the union of the ranks' maps (kmi_dbg_prune_edges_dist_host): the dict is this
        rank's and the sums over the ranks are left in `self.prune_totals`."""
        names = [f for f, _ in L.DbgPruneStats._fields_]
        s = L.DbgPruneStats()
        if comm is not None:
            tot = L.DbgPruneStats()
            self.ctx.check(lib.kmi_dbg_prune_edges_dist_host(self.h, comm.h, int(min_edge_count), C.byref(s), C.byref(tot)))
            self.prune_totals = {f: getattr(tot, f) for f in names}
        else:
            self.ctx.check(lib.kmi_dbg_prune_edges(self.h, int(min_edge_count), C.byref(s)))
            self.prune_totals = {f: getattr(s, f) for f in names}
        return {f: getattr(s, f) for f in names}

    def clip_tips(self, min_edge_count=1, max_tip_nodes=None, islands=False, comm=None):
        """One round of tip clipping (kmi_dbg_clip_tips; the definition is in include/kmerind_hip.h): dead-end unitigs of at most
        max_tip_nodes nodes (None: 2 k) that hang off a junction with a greater branch leave the map, and their junction counters
        are cleared; islands=True also removes the short unitigs without any neighbour -> dict of the kmi_dbg_clip_stats words.
        Without `comm` a map that holds a rank's share of a build over ranks is refused. With `comm` the call is collective over
        the union of the ranks' maps (kmi_dbg_clip_tips_dist_host): the dict is this rank's and the sums over the ranks are left in
        `self.clip_totals`."""
        m = 2 * int(self.cfg.k) if max_tip_nodes is None else int(max_tip_nodes)
        names = [f for f, _ in L.DbgClipStats._fields_]
        flags = L.DBG_CLIP_ISLANDS if islands else 0
        s = L.DbgClipStats()
        if comm is not None:
            tot = L.DbgClipStats()
            self.ctx.check(lib.kmi_dbg_clip_tips_dist_host(self.h, comm.h, int(min_edge_count), m, flags, C.byref(s), C.byref(tot)))
            self.clip_totals = {f: getattr(tot, f) for f in names}
        else:
            self.ctx.check(lib.kmi_dbg_clip_tips(self.h, int(min_edge_count), m, flags, C.byref(s)))
            self.clip_totals = {f: getattr(s, f) for f in names}
        return {f: getattr(s, f) for f in names}

    def pop_bubbles(self, min_edge_count=1, max_bubble_nodes=None, comm=None):
        """One round of bubble popping (kmi_dbg_pop_bubbles; the definition is in include/kmerind_hip.h): of the unitigs that run
        between the same two junction ends, those of at most max_bubble_nodes nodes (None: 2 k) that have a greater sibling leave
        the map, and both their junction counters are cleared -> dict of the kmi_dbg_pop_stats words. Without `comm` a map that
        holds a rank's share of a build over ranks is refused. With `comm` the call is collective over the union of the ranks'
        maps (kmi_dbg_pop_bubbles_dist_host): the dict is this rank's and the sums over the ranks are left in `self.pop_totals`."""
        m = 2 * int(self.cfg.k) if max_bubble_nodes is None else int(max_bubble_nodes)
        names = [f for f, _ in L.DbgPopStats._fields_]
        s = L.DbgPopStats()
        if comm is not None:
            tot = L.DbgPopStats()
            self.ctx.check(lib.kmi_dbg_pop_bubbles_dist_host(self.h, comm.h, int(min_edge_count), m, 0, C.byref(s), C.byref(tot)))
            self.pop_totals = {f: getattr(tot, f) for f in names}
        else:
            self.ctx.check(lib.kmi_dbg_pop_bubbles(self.h, int(min_edge_count), m, 0, C.byref(s)))
            self.pop_totals = {f: getattr(s, f) for f in names}
        return {f: getattr(s, f) for f in names}

    def unitig_sequences(self, min_edge_count=1, comm=None):
        """the sequences of unitigs() as a list of bytes, in unitig order"""
        return split_unitigs(*self.unitigs(min_edge_count, comm)[:2])


def split_unitigs(offsets, bases):
    """(offsets, bases) of DeBruijnNodes.unitigs() -> list of bytes"""
    raw = np.ascontiguousarray(bases, dtype=np.uint8).tobytes()
    return [raw[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def synth_fastq(seed, genome_len, n_reads, read_len=150, first_read=0, threads=None):
    """SURVEY.md 8(d) synthetic FASTQ as a numpy uint8 array (host)."""
    nbytes = lib.kmi_synth_fastq_bytes(n_reads, read_len)
    out = np.empty(nbytes, dtype=np.uint8)
    threads = threads or min(16, os.cpu_count() or 1)
    st = lib.kmi_synth_fastq(seed, genome_len, read_len, first_read, n_reads, out.ctypes.data_as(C.c_void_p), nbytes,
                             threads)
    if st != L.OK:
        raise ValueError("kmi_synth_fastq: bad arguments")
    return out
