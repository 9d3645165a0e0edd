"""The position and position + quality indexes (multimaps: bucket_query_kernel<NW, 1> and <NW, 2>, mm_build_vw / mm_insert_vw, the
multimap branch of erase) where they had no cover: (a) one bucket with more distinct query keys than the query table has slots,
so count / find / erase run in passes; (b) a key with 150 000 values, which at k = 32 is the table's empty marker; (c) the
device entry points of a multimap find into buffers of exactly the hit count; (d) operation sequences, scripted and seeded.
The reference is tests/oracle.py's MultiMap throughout, the inputs come from tests/multimap_cases.py (checked on the CPU by
test_multimap_cases.py), and every comparison is exact: integers, float bit patterns as integers, multisets as sorted rows."""
import ctypes as C

import numpy as np
import pytest

from tests import index_model as M
from tests import multimap_cases as MC
from tests import oracle as orc

pytestmark = pytest.mark.gpu

STRAND = {"single": orc.SINGLE, "canonical": orc.CANONICAL}
GUARD = 64                              # words behind a device result buffer that a query must leave alone
PATTERN = 0xA5A5A5A5DEADBEEF


@pytest.fixture(scope="module")
def ctx():
    import kmerind_amd as K
    c = K.Context(0)
    yield c
    c.close()


# ---- comparisons
def difference(got, want):
    """None when two (keys, values) multisets are equal, else a line about the first row that differs"""
    (gk, gv), (wk, wv) = got, want
    if len(gk) != len(wk):
        return "%d rows, expected %d" % (len(gk), len(wk))
    if len(gk) == 0:
        return None
    a, b = orc.sorted_rows(gk, gv), orc.sorted_rows(wk, wv)
    if a.shape == b.shape and (a == b).all():
        return None
    if a.shape != b.shape:
        return "rows of %d words, expected %d" % (a.shape[1], b.shape[1])
    i = int(np.nonzero((a != b).any(axis=1))[0][0])
    return "%d rows; sorted row %d: got %s, expected %s" % (a.shape[0], i, ["%x" % x for x in a[i].tolist()], ["%x" % x for x in b[i].tolist()])


def state_difference(idx, ref, vw):
    """None when the index holds exactly the reference's tuples: local_size and the row multiset of to_vector (value word 1 of a
    position + quality index as the full 64-bit word, whose high half is zero)"""
    if idx.local_size() != ref.size():
        return "local_size %d, expected %d" % (idx.local_size(), ref.size())
    gk, gv = idx.to_vector()
    d = difference((gk, gv), ref.export())
    if d:
        return "to_vector: " + d
    if vw == 2 and gv.shape[0] and int((gv[:, 1] >> np.uint64(32)).max()):
        return "to_vector: a quality word with bits in its high half"
    return None


def find_hits(ctx, idx, q):
    """kmi_index_find_hits_dev of host keys"""
    from kmerind_amd import _lib as L
    q = np.ascontiguousarray(q, dtype=np.uint64).reshape(-1, idx.n_words)
    dq = ctx.alloc(max(q.nbytes, 8))
    try:
        ctx.to_device(dq, q)
        n = C.c_uint64(12345)
        ctx.check(L.lib.kmi_index_find_hits_dev(idx.h, C.c_void_p(dq), q.shape[0], C.byref(n)))
    finally:
        ctx.free(dq)
    return n.value


def query_difference(ctx, idx, ref, q):
    """None when count(q) and find(q) answer as the reference does. The find is sized first (kmi_index_find_hits_dev against the
    reference's row count): a find whose sizing pass and output pass disagree writes past its result buffer, and this way it shows
    as a failed comparison before that find runs."""
    d = difference(idx.count(q), ref.count(q))
    if d:
        return "count: " + d
    want = ref.find(q)
    hits = find_hits(ctx, idx, q)
    if hits != want[0].shape[0]:
        return "find_hits: %d, expected %d" % (hits, want[0].shape[0])
    d = difference(idx.find(q), want)
    return "find: " + d if d else None


def make_index(ctx, k, alpha, strand, kind):
    import kmerind_amd as K
    s = orc.kspec(k, MC.ALPHA[alpha])
    vw = MC.VW[kind]
    return s, vw, K.PositionIndex(ctx, K.make_config(k, alpha, strand=strand, index_kind=kind)), orc.MultiMap(s, STRAND[strand], vw=vw)


# ---- (c) device entry points (called from (a) on its index before the erase)
def device_query(ctx, idx, fn, q, n_records, vw):
    """fn = kmi_index_find_dev / kmi_index_count_dev into device buffers of exactly n_records records (n_words key words and vw
    value words each), each followed by GUARD words of PATTERN -> (n_out, keys, values, key guard, value guard)"""
    nw = idx.n_words
    hk = np.full(n_records * nw + GUARD, PATTERN, dtype=np.uint64)
    hv = np.full(n_records * vw + GUARD, PATTERN, dtype=np.uint64)
    dq, dk, dv = ctx.alloc(q.nbytes), ctx.alloc(hk.nbytes), ctx.alloc(hv.nbytes)
    try:
        ctx.to_device(dq, q)
        ctx.to_device(dk, hk)
        ctx.to_device(dv, hv)
        n = C.c_uint64(0)
        ctx.check(fn(idx.h, C.c_void_p(dq), q.shape[0], C.c_void_p(dk), C.c_void_p(dv), C.byref(n)))
        ctx.to_host(hk, dk)
        ctx.to_host(hv, dv)
    finally:
        ctx.free(dq); ctx.free(dk); ctx.free(dv)
    return n.value, hk[:n_records * nw].reshape(n_records, nw), hv[:n_records * vw].reshape(n_records, vw), hk[n_records * nw:], hv[n_records * vw:]


def check_device_entry_points(ctx, idx, ref, q, vw):
    from kmerind_amd import _lib as L
    want_k, want_v = ref.find(q)
    hits = find_hits(ctx, idx, q)
    assert hits == want_k.shape[0] > q.shape[0]
    n, gk, gv, guard_k, guard_v = device_query(ctx, idx, L.lib.kmi_index_find_dev, q, hits, vw)
    assert n == hits
    assert difference((gk, gv), (want_k, want_v)) is None
    assert (guard_k == np.uint64(PATTERN)).all() and (guard_v == np.uint64(PATTERN)).all()
    # count into buffers of nq records: one row per distinct key, the multiplicity in value word 0 (a record of a position +
    # quality index has two value words; what the second holds for a count is not specified)
    nq = q.shape[0]
    want_k, want_c = ref.count(q)
    n, gk, gv, guard_k, guard_v = device_query(ctx, idx, L.lib.kmi_index_count_dev, q, nq, vw)
    assert n == want_k.shape[0] < nq
    assert difference((gk[:n], gv[:n, 0]), (want_k, want_c)) is None
    assert (gk[n:] == np.uint64(PATTERN)).all() and (gv[n:] == np.uint64(PATTERN)).all()
    assert (guard_k == np.uint64(PATTERN)).all() and (guard_v == np.uint64(PATTERN)).all()


def orc_find_rows(s, data, q):
    """rows the reference's find returns from a canonical position index built from `data`"""
    om = orc.MultiMap(s, orc.CANONICAL)
    om.insert(*MC.tuples_of(s, data, 1))
    return om.find(q)[0].shape[0]


def test_find_hits_dev_on_a_cleared_index_and_on_a_count_index(ctx):
    import kmerind_amd as K
    s, vw, idx, ref = make_index(ctx, 31, "DNA", "canonical", "position")
    rng = np.random.default_rng(4)
    data = MC.fastq(rng, MC.reads(rng, 150, 31))
    q = MC.tuples_of(s, data, 1)[0][:3000]
    idx.build(data)
    assert find_hits(ctx, idx, q) == orc_find_rows(s, data, q) > 3000
    idx.clear()
    assert find_hits(ctx, idx, q) == 0
    idx.close()
    cidx = K.CountIndex(ctx, K.make_config(31, "DNA", strand="canonical"))
    assert find_hits(ctx, cidx, q) == 3000             # a count index: nq, before and after it holds anything
    cidx.build(data)
    assert find_hits(ctx, cidx, q) == 3000
    cidx.close()


# ---- (a) query passes on a multimap
@pytest.mark.parametrize("k,alpha,kind", MC.PASS_SHAPES)
def test_query_passes_on_a_multimap(ctx, k, alpha, kind):
    """N_HOT = 16 000 distinct keys of ONE placement bucket, each one to three times, among 20 000 random k-mers, inserted in two
    calls (the second concatenates). The query holds N_HOT_Q = 8 000 of the hot keys -- more than QTabCfg<NW>::CAP home slots for
    every NW -- so bucket_query_kernel splits the bucket's queries and entries into passes in every mode: the sizing pass and the
    find must take the same passes, count must sum a key's entries within its pass, erase must keep the hot keys that were not
    queried, which went through every pass beside erased ones. Single strand: the hot keys reach the placement hash unchanged."""
    s, vw, idx, ref = make_index(ctx, k, alpha, "single", kind)
    assert MC.N_HOT_Q > MC.QUERY_CAP[s.n_words]
    rng = np.random.default_rng(100 * k + vw)
    hot = MC.hot_keys(k, alpha, MC.N_HOT)
    kmers, vals = MC.hot_tuples(rng, hot, vw, s)
    half = kmers.shape[0] // 2
    for part in (slice(0, half), slice(half, None)):                     # 1. two inserts
        idx.insert(kmers[part], vals[part])
        ref.insert(kmers[part], vals[part])
        assert state_difference(idx, ref, vw) is None
    q = MC.pass_queries(rng, hot, s)                                     # 2.
    n_distinct = np.unique(q, axis=0).shape[0]
    assert q.shape[0] == MC.N_HOT_Q + 1500 and n_distinct > MC.N_HOT_Q
    ck, cc = idx.count(q)                                                # 3. one row per distinct key, zeros for the absent ones
    assert ck.shape[0] == n_distinct and int((cc == 0).sum()) == n_distinct - MC.N_HOT_Q and int(cc.max()) <= 3
    assert difference((ck, cc), ref.count(q)) is None
    assert query_difference(ctx, idx, ref, q) is None                    # 4. (and the count again)
    check_device_entry_points(ctx, idx, ref, q, vw)                      # (c)
    erased = ref.find(q)
    before = ref.size()
    n_gpu, n_ref = idx.erase(q), ref.erase(q)                            # 5.
    assert n_gpu == n_ref == erased[0].shape[0] == int(cc.sum())
    assert ref.size() == before - n_ref >= MC.N_HOT - MC.N_HOT_Q + MC.N_FILLER
    assert state_difference(idx, ref, vw) is None
    fk, fv = idx.find(q)                                                 # 6.
    assert fk.shape[0] == 0 and fv.shape[0] == 0
    ck, cc = idx.count(q)
    assert ck.shape[0] == n_distinct and not cc.any()
    assert difference((ck, cc), ref.count(q)) is None
    assert idx.erase(q) == 0 and state_difference(idx, ref, vw) is None
    idx.insert(erased[0][::2], erased[1][::2])                           # 7.
    ref.insert(erased[0][::2], erased[1][::2])
    assert state_difference(idx, ref, vw) is None
    assert query_difference(ctx, idx, ref, q) is None
    idx.close()


# ---- (b) a heavy key, and the key that equals the table's empty marker
@pytest.mark.parametrize("k,alpha,kind", MC.HEAVY_SHAPES)
def test_heavy_key(ctx, k, alpha, kind):
    """one key with N_HEAVY = 150 000 values: every lane of every wavefront of its bucket hits. k = 31: it is one of the hot keys,
    in the bucket whose queries need passes. k = 32: it is 0xFFFFFFFFFFFFFFFF, the all-T 32-mer, which the query table cannot
    hold as a key (kEmptyKey marks its free slots) and answers from a slot of its own; it also comes in through the build, from
    40 poly-T reads among ordinary ones."""
    s, vw, idx, ref = make_index(ctx, k, alpha, "single", kind)
    rng = np.random.default_rng(100 * k + vw + 1)
    hot = MC.hot_keys(k, alpha, MC.N_HOT)
    heavy = hot[:1] if k != 32 else np.array([[MC.EMPTY_MARKER]], dtype=np.uint64)
    n_heavy = MC.N_HEAVY
    if k == 32:
        data = MC.poly_fastq(rng, k)
        idx.build(data)
        ref.insert(*MC.tuples_of(s, data, vw))
        assert state_difference(idx, ref, vw) is None
        n_heavy += 40 * (150 - k + 1)
    kmers, vals = MC.hot_tuples(rng, hot, vw, s)
    hk, hv = MC.heavy_tuples(heavy, vw=vw)
    for a, b in ((kmers, vals), (hk, hv)):
        idx.insert(a, b)
        ref.insert(a, b)
        assert state_difference(idx, ref, vw) is None
    n_heavy += int((kmers == heavy).all(axis=1).sum())
    q = np.concatenate([MC.pass_queries(rng, hot, s), heavy, heavy])
    ck, cc = idx.count(q)
    assert cc[(ck == heavy).all(axis=1)].tolist() == [n_heavy]
    assert query_difference(ctx, idx, ref, q) is None
    assert query_difference(ctx, idx, ref, heavy) is None
    fk, fv = idx.find(heavy)
    assert fk.shape[0] == n_heavy and (fk == heavy).all() and np.unique(fv[:, 0]).size == n_heavy
    absent = MC.random_kmers(s, rng, 1000)                               # only absent keys
    assert ref.find(absent)[0].shape[0] == 0
    fk, fv = idx.find(absent)
    ck, cc = idx.count(absent)
    assert fk.shape[0] == 0 and ck.shape[0] == np.unique(absent, axis=0).shape[0] and not cc.any()
    assert find_hits(ctx, idx, absent) == 0
    before = ref.size()
    n_gpu, n_ref = idx.erase(heavy), ref.erase(heavy)
    assert n_gpu == n_ref == n_heavy and ref.size() == before - n_heavy
    assert state_difference(idx, ref, vw) is None
    assert idx.erase(heavy) == 0 and state_difference(idx, ref, vw) is None   # a second erase finds nothing
    assert query_difference(ctx, idx, ref, q) is None
    idx.close()


@pytest.mark.parametrize("strand", ["single", "canonical"])
def test_poly_t_reads_through_the_build_at_k_32(ctx, strand):
    """the build from the parse at k = 32 with 40 poly-T reads: on a single strand their k-mer is the empty marker, under the
    canonical strand model it becomes the all-zero key (which the three poly-A reads have too); queried through either spelling"""
    s, vw, idx, ref = make_index(ctx, 32, "DNA", strand, "posqual")
    rng = np.random.default_rng(32)
    data = MC.poly_fastq(rng, 32)
    kmers, vals = MC.tuples_of(s, data, vw)
    idx.build(data)
    ref.insert(kmers, vals)
    assert state_difference(idx, ref, vw) is None
    all_t, all_a = orc.kmers_from_string(s, b"T" * 32), orc.kmers_from_string(s, b"A" * 32)
    assert all_t.tolist() == [[MC.EMPTY_MARKER]] and all_a.tolist() == [[0]]
    n_t, n_a = 40 * 119, 3 * 119
    for q in (all_t, all_a, np.concatenate([all_t, all_a, kmers[::5], MC.random_kmers(s, rng, 200), all_t])):
        assert query_difference(ctx, idx, ref, q) is None
    ck, cc = idx.count(np.concatenate([all_t, all_a]))
    got = dict(zip(ck[:, 0].tolist(), cc.tolist()))
    assert got == ({MC.EMPTY_MARKER: n_t, 0: n_a} if strand == "single" else {0: n_t + n_a})
    n_gpu, n_ref = idx.erase(all_t), ref.erase(all_t)
    assert n_gpu == n_ref == (n_t if strand == "single" else n_t + n_a)
    assert state_difference(idx, ref, vw) is None
    assert idx.erase(all_t) == 0 and query_difference(ctx, idx, ref, np.concatenate([all_t, all_a, kmers[:500]])) is None
    idx.build(data, file_offset=1 << 33)                                 # and back in, beside what is left
    ref.insert(*MC.tuples_of(s, data, vw, file_offset=1 << 33))
    assert state_difference(idx, ref, vw) is None
    idx.close()


# ---- (d) operation sequences
class Log:
    """the operations so far, for failure messages"""

    def __init__(self, name):
        self.name, self.ops = name, []

    def __str__(self):
        return "%s, operations: %s" % (self.name, " -> ".join(self.ops))


class PosSeq:
    """a PositionIndex and its orc.MultiMap, driven step by step; the whole state is compared after every step"""

    def __init__(self, ctx, k, alpha, strand, kind, log):
        from kmerind_amd import _lib as L
        self.L, self.ctx, self.k, self.strand, self.kind, self.log = L, ctx, k, strand, kind, log
        self.s, self.vw, self.idx, self.ref = make_index(ctx, k, alpha, strand, kind)
        self.rng = np.random.default_rng(k + self.vw)

    def close(self):
        self.idx.close()

    def step(self, op, *args):
        self.log.ops.append(op)
        ret = getattr(self, "_" + op)(*args)
        if ret is not None:
            assert ret[0] == ret[1], "%s returned %s, expected %s (%s)" % (op, ret[0], ret[1], self.log)
        self.check()

    def check(self):
        d = state_difference(self.idx, self.ref, self.vw)
        if d is None:      # (to_vector alone cannot see a tuple filed in the wrong bucket)
            d = query_difference(self.ctx, self.idx, self.ref, M.probes(self.s, self.ref.export()[0], self.rng, n_stored=300, n_absent=60))
        assert d is None, "k=%d %s %s: %s (%s)" % (self.k, self.strand, self.kind, d, self.log)

    def tuples(self, data, fmt=orc.FASTQ, file_offset=0):
        return MC.tuples_of(self.s, data, self.vw, fmt, file_offset)

    def _build(self, data, file_offset=0):
        self.idx.build(data, file_offset=file_offset)
        self.ref.insert(*self.tuples(data, file_offset=file_offset))

    def _build_device(self, data):
        buf = np.frombuffer(data, dtype=np.uint8)
        d = self.ctx.alloc(buf.size + 64)
        try:
            self.ctx.to_device(d, buf)
            self.idx.build_device(d, buf.size)
        finally:
            self.ctx.free(d)
        self.ref.insert(*self.tuples(data))

    def _build_fasta(self, data):
        L = self.L
        self.ctx.check(L.lib.kmi_index_set_seq_format(self.idx.h, L.FMT_FASTA))
        try:
            self.idx.build(data)
        finally:
            self.ctx.check(L.lib.kmi_index_set_seq_format(self.idx.h, L.FMT_FASTQ))
        self.ref.insert(*self.tuples(data, fmt=orc.FASTA))

    def _insert(self, kmers, vals):
        self.idx.insert(kmers, vals)
        self.ref.insert(kmers, vals)

    def _erase(self, q):
        return self.idx.erase(q), self.ref.erase(q)

    def _erase_all(self):
        """every key of to_vector(); afterwards the index has_data with no entry"""
        keys = self.idx.to_vector()[0]
        n = self.ref.size()
        got = self.idx.erase(keys) if keys.shape[0] else 0
        want = self.ref.erase(keys) if keys.shape[0] else 0
        assert want == n and self.ref.size() == 0
        return got, want

    def _clear(self):
        self.idx.clear()
        self.ref = orc.MultiMap(self.s, STRAND[self.strand], vw=self.vw)

    def _queries(self, q):
        d = query_difference(self.ctx, self.idx, self.ref, q)
        assert d is None, "%s (%s)" % (d, self.log)

    def assert_empty(self, q):
        """no entry: local_size 0, an empty to_vector, find returns nothing and count a zero per distinct key, as a fresh index"""
        gk, gv = self.idx.to_vector()
        assert self.idx.local_size() == 0 and gk.shape == (0, self.s.n_words) and gv.shape == (0, self.vw), self.log
        fk, fv = self.idx.find(q)
        ck, cc = self.idx.count(q)
        assert fk.shape[0] == 0 and fv.shape[0] == 0 and not cc.any(), self.log
        import kmerind_amd as K
        fresh = K.PositionIndex(self.ctx, self.idx.cfg)
        try:
            assert difference((ck, cc), fresh.count(q)) is None and fresh.find(q)[0].shape[0] == 0, self.log
        finally:
            fresh.close()
        assert find_hits(self.ctx, self.idx, q) == 0, self.log

    # inputs drawn for this index
    def fastq(self, n, poly=False):
        seqs = MC.reads(self.rng, n, self.k)
        if poly:
            seqs += M.poly_reads(b"A", 5) + M.poly_reads(b"T", 4)
        return MC.fastq(self.rng, seqs)

    def query_keys(self, n):
        """stored keys (either strand, some twice) and keys that are not stored"""
        keys = self.ref.export()[0]
        st = keys[self.rng.integers(0, keys.shape[0], n)] if keys.shape[0] else keys
        return np.concatenate([st, orc.revcomp(self.s, st[: n // 3]), MC.random_kmers(self.s, self.rng, n // 4 + 1)])


def row_build_erase_all_build(c):
    """an index that has_data with 0 entries takes the fresh branch of mm_build_vw"""
    c.step("build", c.fastq(200, poly=True))
    q = c.query_keys(500)
    c.step("erase_all")
    c.assert_empty(q)
    c.step("build", c.fastq(250))
    c.step("build", c.fastq(100))


def row_build_erase_all_insert(c):
    """... and of mm_insert_vw"""
    c.step("build", c.fastq(200))
    q = c.query_keys(500)
    c.step("erase_all")
    c.assert_empty(q)
    c.step("insert", *c.tuples(c.fastq(120), file_offset=1 << 30))
    c.step("insert", *c.tuples(c.fastq(60), file_offset=1 << 31))


def row_insert_build_erase_halves(c):
    """tuples, a build that concatenates, erase of half the distinct keys, a build at another file offset, erase of the rest"""
    c.step("insert", *c.tuples(c.fastq(100), file_offset=1 << 34))
    c.step("build", c.fastq(200, poly=True))
    keys = np.unique(c.ref.export()[0], axis=0)
    c.step("erase", keys[::2])
    c.step("build", c.fastq(200), 1 << 33)
    c.step("erase", keys[1::2])
    c.step("erase", np.unique(c.ref.export()[0], axis=0)[::2])


def row_build_clear_erase_build(c):
    c.step("build", c.fastq(200))
    q = c.query_keys(400)
    c.step("clear")
    assert c.idx.erase(q) == 0
    c.step("erase", q)
    c.assert_empty(q)
    c.step("build", c.fastq(150, poly=True))


def row_never_filled(c):
    """erase, find and count on an index that never held anything"""
    q = MC.random_kmers(c.s, c.rng, 300)
    c.check()
    c.assert_empty(q)
    c.step("erase", q)
    c.assert_empty(q)
    c.step("queries", q)
    c.step("erase_all")


def row_fastq_then_fasta(c):
    """a FASTQ build, then a FASTA build of other reads and some of the same, erase keys of both. A position + quality index
    reads FASTQ only: there kmi_index_set_seq_format(FASTA) gives KMI_ERR_INVALID and changes nothing."""
    L = c.L
    seqs = MC.reads(c.rng, 200, c.k)
    c.step("build", MC.fastq(c.rng, seqs))
    seqs2 = MC.reads(c.rng, 150, c.k) + seqs[:20] + M.poly_reads(b"T", 2)
    if c.kind == "posqual":
        import kmerind_amd as K
        assert L.lib.kmi_index_set_seq_format(c.idx.h, L.FMT_FASTA) == L.ERR_INVALID
        c.check()
        with pytest.raises(L.KmiError):                    # (nor is such an index created)
            K.PositionIndex(c.ctx, K.make_config(c.k, "DNA", strand=c.strand, index_kind="posqual", seq_format="fasta"))
        c.step("build", MC.fastq(c.rng, seqs2))            # (still a FASTQ index)
    else:
        c.step("build_fasta", MC.fasta(seqs2))
        c.step("build", MC.fastq(c.rng, seqs2[:50]))       # (and a FASTQ index again)
    c.step("erase", c.query_keys(900))


def row_host_and_device_builds(c):
    c.step("build", c.fastq(150))
    c.step("build_device", c.fastq(300, poly=True))
    c.step("build", c.fastq(200))
    c.step("build_device", c.fastq(100))


def row_kmer_and_its_reverse_complement(c):
    """queries that hold a k-mer and its reverse complement: under the canonical strand model they are one key -- one count row,
    the entries once from find, counted once by erase; on a single strand they are two keys"""
    c.step("build", c.fastq(200))
    st = c.ref.export()[0][::9]
    q = np.concatenate([st, orc.revcomp(c.s, st), st[:10]])
    ck, cc = c.idx.count(q)
    n_keys = np.unique(orc.canonical(c.s, q) if c.strand == "canonical" else q, axis=0).shape[0]
    assert ck.shape[0] == n_keys and np.unique(ck, axis=0).shape[0] == n_keys, c.log
    if c.strand == "canonical":
        assert n_keys == np.unique(st, axis=0).shape[0]
        fk, fv = c.idx.find(q)
        assert difference((fk, fv), c.idx.find(st)) is None and fk.shape[0] == int(cc.sum()), c.log
    c.step("queries", q)
    n = c.ref.find(q)[0].shape[0]
    c.step("erase", q)
    assert c.idx.local_size() == c.ref.size() and n > 0
    c.step("queries", q)


def row_values_verbatim(c):
    """inserted value words come back bit for bit: ids of all ones and with the top bit set; on a position + quality index
    float bit patterns with the sign bit set (-0.0, -1.0, a negative NaN) and of all ones in the low half of word 1"""
    c.step("build", c.fastq(100))
    kmers = c.tuples(c.fastq(40))[0][:2000]
    n = kmers.shape[0]
    vals = np.zeros((n, c.vw), dtype=np.uint64)
    vals[:, 0] = np.array([0xFFFFFFFFFFFFFFFF, 1 << 63, 0, 0x8000000000000001], dtype=np.uint64)[np.arange(n) % 4] - np.arange(n, dtype=np.uint64) // np.uint64(4) * np.uint64(2)
    if c.vw == 2:
        vals[:, 1] = np.array([0x80000000, 0xFFFFFFFF, 0xBF800000, 0xFFC00001, 0x7F800000], dtype=np.uint64)[np.arange(n) % 5]
    c.step("insert", kmers, vals)
    fk, fv = c.idx.find(kmers[:4])
    assert {tuple(r) for r in vals[:4].tolist()} <= {tuple(r) for r in fv.tolist()}, c.log
    c.step("erase", kmers[::2])
    c.step("insert", kmers[::2], vals[::2])


ROWS = [row_build_erase_all_build, row_build_erase_all_insert, row_insert_build_erase_halves, row_build_clear_erase_build,
        row_never_filled, row_fastq_then_fasta, row_host_and_device_builds, row_kmer_and_its_reverse_complement, row_values_verbatim]
BASE = [(31, "DNA", "canonical", "position"), (21, "DNA", "single", "posqual")]
WIDE = (63, "DNA5", "canonical", "position")
TRANSITIONS = [(row, cfg) for row in ROWS for cfg in BASE] + [(row_build_erase_all_build, WIDE)]


@pytest.mark.parametrize("row,cfg", TRANSITIONS, ids=["%s-%d-%s-%s-%s" % ((r.__name__[4:],) + c) for r, c in TRANSITIONS])
def test_transition(ctx, row, cfg):
    c = PosSeq(ctx, *cfg, Log(row.__name__))
    try:
        row(c)
    finally:
        c.close()


OPS = ["build", "build_offset", "insert", "erase", "erase_all", "clear", "count", "find"]


def _random_op(c, rng, op):
    n = int(rng.integers(150, 401))
    if op == "build":
        c.step("build", c.fastq(n, poly=bool(rng.integers(0, 2))))
    elif op == "build_offset":
        c.step("build", c.fastq(n), int(rng.integers(1, 1 << 15)) << 20)
    elif op == "insert":
        c.step("insert", *c.tuples(c.fastq(n // 2), file_offset=int(rng.integers(1, 1 << 15)) << 20))
    elif op == "erase":
        c.step("erase", c.query_keys(1500))
    elif op in ("erase_all", "clear"):
        c.step(op)
    else:    # count and find: on more keys than the probes of the state check
        c.step("queries", c.query_keys(3000))


@pytest.mark.parametrize("cfg", BASE, ids=["%d-%s-%s-%s" % c for c in BASE])
@pytest.mark.parametrize("seed", range(8))
def test_random_sequence(ctx, cfg, seed):
    """12 operations on one index, inputs of 150 to 400 reads of one small genome (keys repeat from step to step); the first
    operation fills the index, the rest are drawn"""
    rng = np.random.default_rng(1000 * cfg[0] + seed)
    c = PosSeq(ctx, *cfg, Log("seed %d" % seed))
    c.rng = rng
    try:
        for i in range(12):
            op = ["build", "insert"][int(rng.integers(0, 2))] if i == 0 else OPS[int(rng.integers(0, len(OPS)))]
            _random_op(c, rng, op)
    finally:
        c.close()
