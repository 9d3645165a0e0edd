"""What the C ABI's older entry points answer when they REFUSE a call: the status, the text left in the context's last error, and
what stands in the out-parameters afterwards. Called through kmerind_amd._lib on a tiny count index and a tiny position index
(k = 21, a dozen k-mers), a de Bruijn node map and a one-rank communicator. Every case is refused on the host before a kernel
runs (or, for n == 0, is done before one would); none of them reaches the device with a bad pointer.

The last error is set to a marker text before every call, so a refusal that sets no text (a null handle or out-parameter) is
pinned as well: the marker is still there afterwards."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K21 = 21
NULL_BUFFER = "null buffer"
NRANKS = "nranks must be in 1..256"
OTHER_CTX = "the communicator belongs to another context"
TAKES_TUPLES = "a position index takes (k-mer, value) tuples: kmi_index_insert_tuples_*"
PAIRS_COUNT = "(k-mer, count) pairs go into a count index"
NEEDS_POSITION = "insert_tuples needs a position index"
UPDATE_COUNTING = "update() is a member of the counting maps"
UNKNOWN_UPDATER = "unknown updater"
EXPORT_SMALL = "export: capacity too small"
MARKER = "owner ranks: 1, 2, 4 or 8"


class _Env:
    def __init__(self):
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        self.K, self.L, self.lib = K, L, L.lib
        self.ctx = K.Context(0)
        self.other = K.Context(0)
        self.cfg = K.make_config(K21, "DNA", strand="canonical")
        self.pcfg = K.make_config(K21, "DNA", strand="canonical", index_kind="position")
        rng = np.random.default_rng(7)
        self.kmers = np.ascontiguousarray(rng.integers(0, 1 << (2 * K21), (12, 1), dtype=np.uint64))
        self.values = np.ascontiguousarray(np.arange(12, dtype=np.uint64).reshape(12, 1))
        self.pairs = np.ascontiguousarray(np.concatenate([self.kmers, np.full((12, 1), 2, np.uint64)], axis=1))
        self.count = K.CountIndex(self.ctx, self.cfg)
        self.count.insert(self.kmers)
        self.pos = K.PositionIndex(self.ctx, self.pcfg)
        self.pos.insert(self.kmers, self.values)
        self.graph = K.DeBruijnNodes(self.ctx, K.make_config(K21))
        self.comm, self.other_comm = C.c_void_p(), C.c_void_p()
        self.ctx.check(self.lib.kmi_comm_create(self.ctx.h, None, C.byref(self.comm)))
        self.other.check(self.lib.kmi_comm_create(self.other.h, None, C.byref(self.other_comm)))
        self.bytes = np.frombuffer(b"@r\nACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIII\n", dtype=np.uint8).copy()

    def close(self):
        self.lib.kmi_comm_destroy(self.comm)
        self.lib.kmi_comm_destroy(self.other_comm)
        self.graph.close()
        self.pos.close()
        self.count.close()
        self.ctx.close()
        self.other.close()

    def last(self):
        return (self.lib.kmi_last_error(self.ctx.h) or b"").decode()

    def call(self, name, *args):
        """(status, last error) of one call; the last error holds MARKER going in"""
        assert self.lib.kmi_index_set_owner_ranks(self.count.h, 3) == self.L.ERR_INVALID and self.last() == MARKER
        st = getattr(self.lib, name)(*args)
        return st, self.last()

    def refused(self, text, name, *args, status=None):
        """status (ERR_INVALID unless given) and the text; text None: the entry sets none"""
        st, msg = self.call(name, *args)
        want = self.L.ERR_INVALID if status is None else status
        assert (st, msg) == (want, MARKER if text is None else text), (name, st, msg)

    def ok(self, name, *args):
        st, msg = self.call(name, *args)
        assert st == self.L.OK, (name, st, msg)


@pytest.fixture(scope="module")
def env():
    e = _Env()
    yield e
    e.close()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _dirty_results(L):
    r = L.Results()
    r.n = 7
    r.keys = C.cast(C.c_void_p(8), C.POINTER(C.c_uint64))
    r.values = C.cast(C.c_void_p(8), C.POINTER(C.c_uint64))
    return r


def _zeroed(r):
    return r.n == 0 and not r.keys and not r.values


class _Outs:
    """one kmi_results, one u64 and one int for the entries' out-parameters"""

    def __init__(self, L):
        self.r, self.u64, self.need_more = L.Results(), C.c_uint64(), C.c_int()

    def dirty(self):
        self.r.n, self.u64.value, self.need_more.value = 7, 99, 5
        self.r.keys = self.r.values = C.cast(C.c_void_p(8), C.POINTER(C.c_uint64))

    def check_zero(self, name, args):
        """those of the three that the call was given are zero"""
        for o in (a._obj for a in args if hasattr(a, "_obj")):
            assert (_zeroed(o) if o is self.r else o.value == 0), name


def _host_buffer_calls(e, kmers, values, pairs, data, n, nb, outs, out32):
    """(name, args) of every entry that takes a host buffer and is rewritten, with the given buffers (None = null) and lengths"""
    count, pos, g, comm = e.count.h, e.pos.h, e.graph.h, e.comm
    r, u64, need_more = outs.r, outs.u64, outs.need_more
    return [
        ("kmi_index_insert_host", (count, kmers, n)),
        ("kmi_index_insert_pairs_host", (count, pairs, n)),
        ("kmi_index_insert_tuples_host", (pos, kmers, values, n)),
        ("kmi_index_build_host", (count, data, nb, 0)),
        ("kmi_index_count_host", (count, kmers, n, C.byref(r))),
        ("kmi_index_find_host", (count, kmers, n, C.byref(r))),
        ("kmi_index_erase_host", (count, kmers, n, C.byref(u64))),
        ("kmi_index_update_pairs_host", (count, pairs, n, 0, C.byref(u64))),
        ("kmi_index_lookup_host", (count, kmers, n, out32)),
        ("kmi_dbg_build_host", (g, data, nb)),
        ("kmi_dbg_insert_host", (g, pairs, n)),
        ("kmi_dbg_find_host", (g, kmers, n, C.byref(r))),
        ("kmi_dbg_erase_host", (g, kmers, n, C.byref(u64))),
        ("kmi_index_insert_dist_host", (count, comm, kmers, n)),
        ("kmi_index_insert_tuples_dist_host", (pos, comm, kmers, values, n)),
        ("kmi_index_insert_pairs_dist_host", (count, comm, pairs, n)),
        ("kmi_index_update_pairs_dist_host", (count, comm, pairs, n, 0, C.byref(u64))),
        ("kmi_index_build_dist_host", (count, comm, data, nb, 0)),
        ("kmi_index_build_range_dist_host", (count, comm, data, nb, 0, nb, 1, C.byref(need_more))),
        ("kmi_index_count_dist_host", (count, comm, kmers, n, C.byref(r))),
        ("kmi_index_find_dist_host", (count, comm, kmers, n, C.byref(r))),
        ("kmi_index_erase_dist_host", (count, comm, kmers, n, C.byref(u64))),
        ("kmi_index_lookup_dist_host", (count, comm, kmers, n, out32)),
        ("kmi_dbg_build_dist_host", (g, comm, data, nb)),
        ("kmi_dbg_build_range_dist_host", (g, comm, data, nb, 0, nb, 1, C.byref(need_more))),
        ("kmi_dbg_find_dist_host", (g, comm, kmers, n, C.byref(r))),
        ("kmi_dbg_erase_dist_host", (g, comm, kmers, n, C.byref(u64))),
    ]


def test_null_host_buffer_with_items_is_refused(env):
    e, L = env, env.L
    out32 = _p(np.zeros(4, np.uint32))
    outs = _Outs(L)
    for name, args in _host_buffer_calls(e, None, None, None, None, 3, 40, outs, out32):
        outs.dirty()
        e.refused(NULL_BUFFER, name, *args)
        outs.check_zero(name, args)   # (what the entry has for out-parameters is zero after the refusal)
    # one of two buffers null
    e.refused(NULL_BUFFER, "kmi_index_insert_tuples_host", e.pos.h, _p(e.kmers), None, 3)
    e.refused(NULL_BUFFER, "kmi_index_insert_tuples_dist_host", e.pos.h, e.comm, None, _p(e.values), 3)
    e.refused(NULL_BUFFER, "kmi_index_lookup_host", e.count.h, _p(e.kmers), 3, None)
    e.refused(NULL_BUFFER, "kmi_index_lookup_dist_host", e.count.h, e.comm, _p(e.kmers), 3, None)
    # the entries whose results come back in a kmi_results want one
    for name in ("kmi_index_count_host", "kmi_index_find_host"):
        e.refused(None, name, e.count.h, _p(e.kmers), 3, None)
    for name in ("kmi_index_count_dist_host", "kmi_index_find_dist_host", "kmi_index_route_pairs_dist_host"):
        e.refused(None, name, e.count.h, e.comm, _p(e.pairs), 3, None)
    r = _dirty_results(L)
    e.refused(NULL_BUFFER, "kmi_index_route_pairs_dist_host", e.count.h, e.comm, None, 3, C.byref(r))
    assert _zeroed(r)


def test_nothing_to_do_with_a_null_buffer_is_ok(env):
    e, L = env, env.L
    before = e.count.local_size(), e.pos.local_size()
    outs = _Outs(L)
    for name, args in _host_buffer_calls(e, None, None, None, None, 0, 0, outs, None):
        outs.dirty()
        e.ok(name, *args)
        outs.check_zero(name, args)
    r = _dirty_results(L)
    e.ok("kmi_index_route_pairs_dist_host", e.count.h, e.comm, None, 0, C.byref(r))
    assert _zeroed(r)
    assert (e.count.local_size(), e.pos.local_size()) == before


def test_wrong_index_kind_and_unknown_updater(env):
    e = env
    count, pos, comm = e.count.h, e.pos.h, e.comm
    km, va, pa = _p(e.kmers), _p(e.values), _p(e.pairs)
    dev = C.c_void_p(256)   # a device pointer nobody reads: the kind is refused first
    for name in ("kmi_index_insert_host", "kmi_index_insert_dev", "kmi_index_insert_transformed_dev"):
        e.refused(TAKES_TUPLES, name, pos, dev if name.endswith("_dev") else km, 12)
    e.refused("a position index takes (k-mer, value) tuples: kmi_index_insert_tuples_dist_host", "kmi_index_insert_dist_host", pos, comm, km, 12)
    e.refused(PAIRS_COUNT, "kmi_index_insert_pairs_host", pos, pa, 12)
    e.refused(PAIRS_COUNT, "kmi_index_insert_pairs_dev", pos, dev, 12)
    e.refused(PAIRS_COUNT, "kmi_index_insert_pairs_dist_host", pos, comm, pa, 12)
    e.refused(NEEDS_POSITION, "kmi_index_insert_tuples_host", count, km, va, 12)
    e.refused(NEEDS_POSITION, "kmi_index_insert_tuples_dev", count, dev, 12)
    e.refused(NEEDS_POSITION, "kmi_index_insert_tuples_dist_host", count, comm, km, va, 12)
    r = _dirty_results(e.L)
    e.refused("(k-mer, value) pairs of a counting map", "kmi_index_route_pairs_dist_host", pos, comm, pa, 12, C.byref(r))
    assert _zeroed(r)
    # update(): the kind, then the updater, then the buffer -- and n_updated is zero after each
    for name, head in (("kmi_index_update_pairs_host", ()), ("kmi_index_update_pairs_dev", ()), ("kmi_index_update_pairs_dist_host", (comm,))):
        buf = dev if name.endswith("_dev") else pa
        for idx, op, rec, text in ((pos, 99, None, UPDATE_COUNTING), (pos, 0, buf, UPDATE_COUNTING), (count, 99, None, UNKNOWN_UPDATER),
                                   (count, 4, buf, UNKNOWN_UPDATER)):
            n = C.c_uint64(99)
            e.refused(text, name, idx, *head, rec, 12, op, C.byref(n))
            assert n.value == 0, (name, text)
        e.refused(None, name, count, *head, buf, 12, 0, None)
    # the queries in the caller's order
    n_hits = C.c_uint64(99)
    occ, off = _p(np.zeros(12, np.uint32)), _p(np.zeros(13, np.uint64))
    e.refused("lookup() is a member of the count index", "kmi_index_lookup_host", pos, km, 12, occ)
    e.refused("lookup() is a member of the count index", "kmi_index_lookup_dev", pos, dev, 12, dev)
    e.refused("lookup() is a member of the count index", "kmi_index_lookup_dist_host", pos, comm, km, 12, occ)
    for name, head in (("kmi_index_locate_host", ()), ("kmi_index_locate_dist_host", (comm,))):
        n_hits.value = 99
        e.refused("locate() is a member of the position indexes", name, count, *head, km, 12, 4, occ, off, None, 0, C.byref(n_hits))
        assert n_hits.value == 0
        n_hits.value = 99
        e.refused("max_occ is at least 1", name, pos, *head, km, 12, 0, occ, off, None, 0, C.byref(n_hits))
        assert n_hits.value == 0
        n_hits.value = 99
        e.refused(NULL_BUFFER, name, pos, *head, None, 12, 4, occ, off, None, 0, C.byref(n_hits))
        assert n_hits.value == 0
        e.refused(None, name, pos, *head, km, 12, 4, occ, off, None, 0, None)


def test_route_entries_refuse_rank_counts_outside_1_to_256(env):
    e, K, L = env, env.K, env.L
    ctx, dev = e.ctx.h, C.c_void_p(256)
    sc = np.full(300, 7, np.uint64)
    nt, ns = C.c_uint64(99), C.c_uint64(99)
    cfg, pcfg = C.byref(e.cfg), C.byref(e.pcfg)

    def calls(c, pc, nranks, counts, n):
        return [("kmi_route_dev", (ctx, c, dev, n, nranks, dev, counts)),
                ("kmi_route_tuples_dev", (ctx, pc, dev, n, nranks, 1, dev, counts)),
                ("kmi_extract_route_dev", (ctx, c, dev, n, nranks, dev, 0, C.byref(nt), C.byref(ns), counts)),
                ("kmi_extract_route_records_dev", (ctx, pc, dev, n, 0, nranks, dev, 0, C.byref(nt), C.byref(ns), counts))]

    for nranks in (0, 257):
        for name, args in calls(cfg, pcfg, nranks, _p(sc), 12):
            e.refused(NRANKS, name, *args)
    for name, args in calls(cfg, pcfg, 4, None, 12):
        e.refused(NRANKS, name, *args)
    assert (sc == 7).all() and nt.value == 99 and ns.value == 99   # (refused before anything is written)
    # the configuration is looked at first, the rank count second, the entry's own rules third
    bad = K.make_config(K21)
    bad.k = 0
    for name, args in calls(C.byref(bad), C.byref(bad), 0, _p(sc), 12):
        e.refused("bad kmi_config", name, *args)
    fasta = K.make_config(K21, seq_format="fasta")
    e.refused(NRANKS, "kmi_extract_route_dev", ctx, C.byref(fasta), dev, 12, 0, dev, 0, C.byref(nt), C.byref(ns), _p(sc))
    e.refused("extract_route: FASTQ only (use kmi_extract_dev + kmi_route_dev)", "kmi_extract_route_dev", ctx, C.byref(fasta), dev, 12, 4, dev, 0,
              C.byref(nt), C.byref(ns), _p(sc))
    e.refused(NRANKS, "kmi_extract_route_records_dev", ctx, cfg, dev, 12, 0, 257, dev, 0, C.byref(nt), C.byref(ns), _p(sc))
    e.refused("records are the tuples of the position indexes (index_kind POSITION / POSQUAL)", "kmi_extract_route_records_dev", ctx, cfg, dev, 12, 0,
              4, dev, 0, C.byref(nt), C.byref(ns), _p(sc))
    for name, args in calls(cfg, pcfg, 4, _p(sc), 12):
        assert getattr(e.lib, name)(None, *args[1:]) == L.ERR_INVALID
    # nothing to route: every destination's count is zero
    for name, args in calls(cfg, pcfg, 3, _p(sc), 0):
        sc[:] = 7
        nt.value = ns.value = 99
        e.ok(name, *args)
        assert (sc[:3] == 0).all() and (sc[3:] == 7).all(), name
        if "extract" in name:
            assert nt.value == 0 and ns.value == 0, name


def test_communicator_of_another_context(env):
    e, L = env, env.L
    count, pos, g, oc = e.count.h, e.pos.h, e.graph.h, e.other_comm
    km, va, pa, by = _p(e.kmers), _p(e.values), _p(e.pairs), _p(e.bytes)
    r, u64, need_more = _dirty_results(L), C.c_uint64(99), C.c_int(5)
    out32 = _p(np.zeros(12, np.uint32))
    size = e.count.local_size()
    for name, args in (("kmi_index_insert_dist_host", (count, oc, km, 12)),
                       ("kmi_index_insert_tuples_dist_host", (pos, oc, km, va, 12)),
                       ("kmi_index_insert_pairs_dist_host", (count, oc, pa, 12)),
                       ("kmi_index_update_pairs_dist_host", (count, oc, pa, 12, 0, C.byref(u64))),
                       ("kmi_index_route_pairs_dist_host", (count, oc, pa, 12, C.byref(r))),
                       ("kmi_index_build_dist_host", (count, oc, by, e.bytes.size, 0)),
                       ("kmi_index_build_range_dist_host", (count, oc, by, e.bytes.size, 0, e.bytes.size, 1, C.byref(need_more))),
                       ("kmi_index_find_dist_host", (count, oc, km, 12, C.byref(r))),
                       ("kmi_index_erase_dist_host", (count, oc, km, 12, C.byref(u64))),
                       ("kmi_index_lookup_dist_host", (count, oc, km, 12, out32)),
                       ("kmi_dbg_build_dist_host", (g, oc, by, e.bytes.size)),
                       ("kmi_dbg_build_range_dist_host", (g, oc, by, e.bytes.size, 0, e.bytes.size, 1, C.byref(need_more))),
                       ("kmi_dbg_find_dist_host", (g, oc, km, 12, C.byref(r))),
                       ("kmi_dbg_erase_dist_host", (g, oc, km, 12, C.byref(u64)))):
        e.refused(OTHER_CTX, name, *args)
    assert e.count.local_size() == size
    # a null communicator sets no text
    e.refused(None, "kmi_index_insert_dist_host", count, None, km, 12)
    e.refused(None, "kmi_dbg_find_dist_host", g, None, km, 12, C.byref(r))


def test_export_capacity_and_kind(env):
    e, L = env, env.L
    keys, c32, v64 = np.zeros((12, 1), np.uint64), np.zeros(12, np.uint32), np.zeros((12, 1), np.uint64)
    n_count, n_pos = e.count.local_size(), e.pos.local_size()
    assert 0 < n_count <= 12 and n_pos == 12
    n = C.c_uint64(99)
    e.refused(EXPORT_SMALL, "kmi_index_export_host", e.count.h, _p(keys), _p(c32), n_count - 1, C.byref(n), status=L.ERR_OVERFLOW)
    assert n.value == 0
    n.value = 99
    e.refused(EXPORT_SMALL, "kmi_index_export_tuples_host", e.pos.h, _p(keys), _p(v64), n_pos - 1, C.byref(n), status=L.ERR_OVERFLOW)
    assert n.value == 0
    n.value = 99
    e.refused("a position index exports tuples: kmi_index_export_tuples_host", "kmi_index_export_host", e.pos.h, _p(keys), _p(c32), 12, C.byref(n))
    assert n.value == 0
    n.value = 99
    e.refused("export_tuples needs a position index", "kmi_index_export_tuples_host", e.count.h, _p(keys), _p(v64), 12, C.byref(n))
    assert n.value == 0
    e.refused(None, "kmi_index_export_host", e.count.h, _p(keys), _p(c32), 12, None)
    e.refused(None, "kmi_index_export_tuples_host", e.pos.h, _p(keys), _p(v64), 12, None)


def test_out_parameters_are_zero_after_a_refusal(env):
    e, L = env, env.L
    km, dev = _p(e.kmers), C.c_void_p(256)
    # n_erased
    for name, args in (("kmi_index_erase_host", (e.count.h, None, 3)), ("kmi_index_erase_dist_host", (e.count.h, e.comm, None, 3)),
                       ("kmi_dbg_erase_host", (e.graph.h, None, 3)), ("kmi_dbg_erase_dist_host", (e.graph.h, e.comm, None, 3))):
        n = C.c_uint64(99)
        e.refused(NULL_BUFFER, name, *args, C.byref(n))
        assert n.value == 0, name
    # n_updated
    for name, args in (("kmi_index_update_pairs_host", (e.count.h, None, 3, 0)), ("kmi_index_update_pairs_dist_host", (e.count.h, e.comm, None, 3, 0))):
        n = C.c_uint64(99)
        e.refused(NULL_BUFFER, name, *args, C.byref(n))
        assert n.value == 0, name
    # n_hits
    n = C.c_uint64(99)
    e.refused("locate() is a member of the position indexes", "kmi_index_locate_dev", e.count.h, dev, 12, 4, dev, dev, None, 0, C.byref(n))
    assert n.value == 0
    # kmi_results
    for name, args in (("kmi_index_count_host", (e.count.h, None, 3)), ("kmi_index_find_host", (e.pos.h, None, 3)),
                       ("kmi_index_count_dist_host", (e.count.h, e.comm, None, 3)), ("kmi_index_find_dist_host", (e.pos.h, e.comm, None, 3)),
                       ("kmi_dbg_find_host", (e.graph.h, None, 3)), ("kmi_dbg_find_dist_host", (e.graph.h, e.comm, None, 3))):
        r = _dirty_results(L)
        e.refused(NULL_BUFFER, name, *args, C.byref(r))
        assert _zeroed(r), name
    # a queried key that is held still comes back afterwards: the refusals left the indexes alone
    r = L.Results()
    e.ok("kmi_index_count_host", e.count.h, km, 12, C.byref(r))
    assert r.n == e.count.local_size()
    e.lib.kmi_results_free(C.byref(r))
