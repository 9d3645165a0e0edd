"""A FASTQ file over ranks by BYTE RANGE: every rank holds bytes [lo, hi) of the file plus look-ahead, wherever that cuts, finds
on the device the first record start at or after its first byte and the first one at or after its nominal end (the four-line
rule of FASTQParser::find_first_record, fastq_loader.hpp:269-364, as partitioned_file applies it, file.hpp:1216-1430) and parses
what lies between; its neighbours apply the same rule at the same file positions, so the partitions tile the file. This is what
Index::build_posix / build_mmap(filename, comm) do with comm.size() > 1, through four entry points:

  1. kmi_fastq_find_records_dev              the rule at explicit positions, also of a buffer that starts inside the file
  2. kmi_extract_range_host                  read_file_* of one rank of several
  3. kmi_index_build_range_dist_host         count, position and position + quality indexes
     kmi_dbg_build_range_dist_host           de Bruijn nodes
  4. the collectives that had only ever run on one rank: kmi_index_update_pairs_dist_host, kmi_dbg_erase_dist_host,
     kmi_dbg_count_dist_host, kmi_index_build_fasta_file_dist_host

1 and 2 are checked against tests/fastq_range_model.py (pinned on the CPU by tests/test_fastq_range_model.py) and the oracle's
parse of the whole file; 3 and 4 against the oracle's single map of the whole file, the ranks being processes that share GPU 0
over a gloo group (kmerind_amd/transport.py), as in test_gpu_dist_clayer.py. Every comparison is exact."""
import ctypes as C
import os
import socket
import time

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import fastq_range_model as M
from tests import index_model as IM
from tests import oracle as orc

pytestmark = pytest.mark.gpu
ALPHA = {"DNA": orc.DNA, "DNA5": orc.DNA5}
STRAND = {"canonical": orc.CANONICAL, "single": orc.SINGLE}
SECTION2 = {"calls": 0, "seconds": 0.0}


GAVE_UP = []   # why the ranks of an earlier test were given up: nothing more is started on the GPU after that


@pytest.fixture(autouse=True)
def _nothing_after_ranks_were_given_up():
    assert not GAVE_UP, "not started: %s" % GAVE_UP[0]
    yield


@pytest.fixture(scope="module")
def ctx():
    import kmerind_amd as K
    c = K.Context(0)
    yield c
    c.close()


def _synth(n_reads, genome_len, seed):
    import kmerind_amd as K
    return bytes(K.synth_fastq(seed=seed, genome_len=genome_len, n_reads=n_reads))


# ---------------------------------------------------------------------------
# 1. kmi_fastq_find_records_dev against the model
# ---------------------------------------------------------------------------
def _find_records(ctx, dptr, n_bytes, starts_file, positions):
    from kmerind_amd import _lib as L
    pos = np.ascontiguousarray(positions, dtype=np.uint64)
    out = np.full(max(pos.size, 1), 0xDEADBEEF, dtype=np.uint64)
    ctx.check(L.lib.kmi_fastq_find_records_dev(ctx.h, C.c_void_p(dptr), n_bytes, starts_file, pos.ctypes.data_as(C.c_void_p) if pos.size else out.ctypes.data_as(C.c_void_p),
                                               pos.size, out.ctypes.data_as(C.c_void_p)))
    return out[:pos.size] if pos.size else out


def _model_table(buf, starts_file, positions):
    return np.array([M.first_record_from(buf, int(p), bool(starts_file)) for p in positions], dtype=np.uint64)


@pytest.mark.parametrize("name,data", M.small_inputs(), ids=[x[0] for x in M.small_inputs()])
def test_find_records_small_inputs_every_position_every_buffer_start(ctx, name, data):
    """every position 0..n (and some beyond) in one call, with buffer_starts_file 1 and 0; the same for the buffer data[c:] at
    every c, passed as d + c (an unaligned device pointer: the kernel reads bytewise); the same for buffers data[c:c + m] that
    end inside each of the four lines. The expectation for data[c:] is the whole file's table shifted by c (the rule only
    looks forward: test_fastq_range_model.py::test_the_rule_only_looks_forward), the one for a truncated buffer is the model on
    those very bytes."""
    n = len(data)
    d = ctx.alloc(n + 64)
    try:
        ctx.to_device(d, np.frombuffer(data, dtype=np.uint8))
        beyond = [n + 1, n + 1000, 1 << 40]
        allpos = list(range(n + 1)) + beyond
        inside = _model_table(data, False, range(n + 1))          # position q of the file, looked at without knowing what lies before
        for sf in (1, 0):
            got = _find_records(ctx, d, n, sf, allpos)
            exp = _model_table(data, sf, allpos)
            assert (got == exp).all(), (name, "whole buffer", sf, np.flatnonzero(got != exp)[:5])
        for c in range(1, n + 1):
            pos = list(range(n - c + 1)) + [n - c + 1, n - c + 77]
            exp0 = np.concatenate([inside[c:] - np.uint64(c), np.full(2, n - c, np.uint64)])
            for sf in (0, 1):
                got = _find_records(ctx, d + c, n - c, sf, pos)
                exp = exp0.copy()
                if sf:
                    exp[0] = 0
                assert (got == exp).all(), (name, "data[%d:]" % c, sf, np.flatnonzero(got != exp)[:5])
        for m in (2, 7, 33, 48, 52, 91, 135):
            for c in range(0, n):
                buf = data[c:c + m]
                pos = list(range(len(buf) + 2))
                exp0 = _model_table(buf, 0, pos)
                for sf in (0, 1):
                    got = _find_records(ctx, d + c, len(buf), sf, pos)
                    exp = exp0.copy()
                    exp[0] = M.first_record_from(buf, 0, bool(sf))    # (the only position starts_file bears on)
                    assert (got == exp).all(), (name, "data[%d:%d]" % (c, c + m), sf, np.flatnonzero(got != exp)[:5])
    finally:
        ctx.free(d)


def _large_inputs():
    return [("natural.withN.fastq", M.golden("natural.withN.fastq")), ("test.medium.fastq", M.golden("test.medium.fastq")),
            ("test.unitiqs.fastq", M.golden("test.unitiqs.fastq")), ("synth", None)]


@pytest.mark.parametrize("name,data", _large_inputs(), ids=[x[0] for x in _large_inputs()])
def test_find_records_large_inputs(ctx, name, data):
    """about 1500 positions per call; n_pos = 0, a position at n and positions beyond n; whole buffers and buffers that start
    at an odd byte inside the file"""
    if data is None:
        data = _synth(3000, 30_000, 23)
    n = len(data)
    d = ctx.alloc(n + 64)
    try:
        ctx.to_device(d, np.frombuffer(data, dtype=np.uint8))
        untouched = _find_records(ctx, d, n, 0, [])
        assert untouched[0] == 0xDEADBEEF                                             # n_pos = 0: nothing is written
        stride = max(1, n // 1500)
        for c in (0, 1, 61, n // 3 + 1, n // 2, n - 700, n - 1):
            pos = sorted(set(list(range(0, n - c, stride)) + list(range(min(300, n - c))) + [n - c - 1, n - c, n - c + 1, n - c + 4096, 1 << 50]))
            for sf in (0, 1):
                got = _find_records(ctx, d + c, n - c, sf, pos)
                exp = _model_table(data[c:], sf, pos)
                assert (got == exp).all(), (name, c, sf, np.flatnonzero(got != exp)[:5])
    finally:
        ctx.free(d)


# ---------------------------------------------------------------------------
# 2. kmi_extract_range_host: every two-way cut, then p-way splits
# ---------------------------------------------------------------------------
def _range_call(ctx, cfg, nw, buf, offset, nominal, eof):
    """-> (need_more, kmers, ids, quality bits, n_seqs)"""
    from kmerind_amd import _lib as L
    a = np.frombuffer(buf, dtype=np.uint8)
    need, t = C.c_int(0), L.Tuples()
    t0 = time.perf_counter()
    ctx.check(L.lib.kmi_extract_range_host(ctx.h, C.byref(cfg), a.ctypes.data_as(C.c_void_p) if a.size else None, a.size, offset, nominal, eof,
                                           C.byref(need), C.byref(t)))
    SECTION2["seconds"] += time.perf_counter() - t0
    SECTION2["calls"] += 1
    nt = t.n_tuples
    km = np.ctypeslib.as_array(t.kmers, shape=(nt * nw,)).copy().reshape(nt, nw) if nt else np.zeros((0, nw), np.uint64)
    ids = np.ctypeslib.as_array(t.ids, shape=(nt,)).copy() if nt and t.ids else np.zeros(0, np.uint64)
    qb = np.ctypeslib.as_array(t.quals, shape=(nt,)).copy().view(np.uint32) if nt and t.quals else np.zeros(0, np.uint32)
    ns = t.n_seqs
    L.lib.kmi_tuples_free(C.byref(t))
    return need.value, km, ids, qb, ns


class _Whole:
    """the oracle's parse of the whole file, and of its prefixes that end at a record start (for the boundary a rank's tuple
    count implies)"""

    def __init__(self, data, k, kind):
        self.data, self.kind = data, kind
        self.s = orc.kspec(k)
        self.ex = orc.extract(self.s, data, orc.FASTQ, want_ids=kind != "count", want_quals=kind == "posqual")
        self.prefix = {}

    def upto(self, f):
        """(tuples, sequences) of the records that start before file position f (a record start, or the file's length)"""
        if f not in self.prefix:
            e = orc.extract(self.s, self.data[:f], orc.FASTQ)
            self.prefix[f] = (e["kmers"].shape[0], e["n_seqs"])
        return self.prefix[f]

    def same(self, parts, label):
        km = np.concatenate([p[1] for p in parts])
        assert km.shape == self.ex["kmers"].shape and (km == self.ex["kmers"]).all(), label
        if self.kind != "count":
            assert (np.concatenate([p[2] for p in parts]) == self.ex["ids"]).all(), label
        if self.kind == "posqual":
            assert (np.concatenate([p[3] for p in parts]) == self.ex["quals"].view(np.uint32)).all(), label
        assert sum(p[4] for p in parts) == self.ex["n_seqs"], label


def _rank_reads(ctx, cfg, whole, lo, hi, look, label):
    """one rank of several reads file bytes [lo, hi) plus look-ahead, four times more while asked to; checked against the model's
    partition of the same range: not more rounds, nothing returned with need_more, and the boundaries the tuple counts imply"""
    data, n = whole.data, len(whole.data)
    begin, end, model_rounds = M.partition_of(data, lo, hi, look)
    rounds = 0
    while True:
        stop = min(n, hi + look)
        need, km, ids, qb, ns = _range_call(ctx, cfg, whole.s.n_words, data[lo:stop], lo, hi - lo, 1 if stop == n else 0)
        rounds += 1
        assert rounds <= model_rounds, (label, rounds, model_rounds)
        if not need:
            break
        assert km.shape[0] == 0 and ids.size == 0 and qb.size == 0 and ns == 0, label      # need_more: nothing parsed
        look *= 4
    (t0, s0), (t1, s1) = whole.upto(begin), whole.upto(end)
    assert (km.shape[0], ns) == (t1 - t0, s1 - s0), (label, (begin, end), km.shape[0], ns)
    if whole.kind != "count" and km.shape[0]:
        assert (ids == whole.ex["ids"][t0:t1]).all(), (label, "ids of the records in [%d, %d)" % (begin, end))
    return need, km, ids, qb, ns


TWO_WAY = [("tricky", 21, "position", 16), ("tricky", 31, "posqual", 16), ("tricky", 15, "count", 16), ("tricky-crlf", 21, "position", 16),
           ("tricky-no-final-eol", 21, "position", 16), ("test.small.fastq", 21, "position", 16), ("tricky", 21, "position", 1)]


@pytest.mark.parametrize("name,k,kind,look", TWO_WAY, ids=["%s-k%d-%s-look%d" % c for c in TWO_WAY])
def test_extract_range_every_two_way_cut(ctx, name, k, kind, look):
    """for every c in 0..n: rank 0 reads data[0 : c + look] with nominal c (buffer_offset 0), rank 1 reads data[c:] (buffer_offset
    c, to the file's end). The two ranks' tuples, one after the other, are the oracle's tuples of the whole file in file order:
    k-mers, ids (so buffer_offset + cut is the file position) and quality bits."""
    import kmerind_amd as K
    data = dict(M.small_inputs(12))[name]
    whole = _Whole(data, k, kind)
    assert whole.ex["kmers"].shape[0] > 0
    cfg = K.make_config(k, "DNA", index_kind=kind)
    n = len(data)
    before = dict(SECTION2)
    for c in range(n + 1):
        label = "%s k=%d %s cut %d" % (name, k, kind, c)
        r0 = _rank_reads(ctx, cfg, whole, 0, c, look, label + " rank 0")
        r1 = _rank_reads(ctx, cfg, whole, c, n, look, label + " rank 1")
        whole.same([r0, r1], label)
    print("\nsection 2 %s k=%d %s look=%d: %d calls, %.2f s in the library" % (name, k, kind, look, SECTION2["calls"] - before["calls"],
                                                                             SECTION2["seconds"] - before["seconds"]))


@pytest.mark.parametrize("p", [3, 5, 8, 30])
@pytest.mark.parametrize("name", ["tricky", "test.small.fastq"])
def test_extract_range_p_way_split(ctx, name, p):
    """p ranks, the equal split; with 30 there are more ranks than records: ranges that hold no record start give nothing, and
    interior ranks' buffers reach the file's end"""
    import kmerind_amd as K
    data = dict(M.small_inputs(24))[name]
    n = len(data)
    before = dict(SECTION2)
    for k, kind in ((21, "position"), (31, "posqual")):
        whole = _Whole(data, k, kind)
        cfg = K.make_config(k, "DNA", index_kind=kind)
        parts = [_rank_reads(ctx, cfg, whole, n * r // p, n * (r + 1) // p, 16, "%s p=%d rank %d" % (name, p, r)) for r in range(p)]
        whole.same(parts, "%s p=%d k=%d" % (name, p, k))
        if p == 30:
            assert any(x[4] == 0 for x in parts)
    print("\nsection 2 %s p=%d: %d calls, %.2f s in the library" % (name, p, SECTION2["calls"] - before["calls"], SECTION2["seconds"] - before["seconds"]))


# ---------------------------------------------------------------------------
# 3 and 4. the collectives over 2, 3 and 4 ranks
# ---------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _case(kind, name, data, k, alpha="DNA", strand="canonical", exists=False, second=None, extra=None, look=16):
    return dict(kind=kind, name=name, data=data, k=k, alpha=alpha, strand=strand, exists=exists, second=second, extra=extra, look=look)


def _label(c):
    return "%s %s k=%d %s %s%s%s" % (c["kind"], c["name"], c["k"], c["alpha"], c["strand"], " then a second file" if c["second"] else "",
                                    " + " + c["extra"] if c["extra"] else "")


def _build_range(fn, ctx, h, comm_h, data, world, rank, look, say):
    """what the facade's build_posix does: block `rank` of the equal split plus look-ahead, 16 times more while the library asks"""
    n = len(data)
    lo, hi = n * rank // world, n * (rank + 1) // world
    rounds = 0
    while True:
        end = min(n, hi + look)
        buf = np.frombuffer(data[lo:end], dtype=np.uint8).copy()
        need = C.c_int(0)
        say("build [%d, %d) + %d, round %d" % (lo, hi, look, rounds + 1))
        ctx.check(fn(h, comm_h, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, lo, hi - lo, 1 if end == n else 0, C.byref(need)))
        rounds += 1
        if not need.value:
            return rounds
        look *= 16


def _take(L, r, nw, vw, dbg=False):
    n = r.n
    keys = np.ctypeslib.as_array(r.keys, shape=(n * nw,)).copy().reshape(n, nw) if n else np.zeros((0, nw), np.uint64)
    if dbg:
        vals = np.ctypeslib.as_array(r.values, shape=(n * 5,)).copy().view(np.uint32).reshape(n, 10)[:, :9].astype(np.uint64) if n else np.zeros((0, 9), np.uint64)
    else:
        vals = np.ctypeslib.as_array(r.values, shape=(n * vw,)).copy().reshape(n, vw) if n else np.zeros((0, vw), np.uint64)
    L.lib.kmi_results_free(C.byref(r))
    return keys, vals


def _query(L, ctx, fn, h, comm_h, q, nw, vw, dbg=False):
    r = L.Results()
    ctx.check(fn(h, comm_h, q.ctypes.data_as(C.c_void_p), q.shape[0], C.byref(r)))
    return _take(L, r, nw, vw, dbg)


def _strangers(s, n, seed):
    """k-mers of a random text over the alphabet's letters (a random bit pattern need not be a k-mer of DNA5)"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTN" if s.alphabet == orc.DNA5 else b"ACGT", dtype=np.uint8)
    return orc.kmers_from_string(s, letters[rng.integers(0, letters.size, s.k + n - 1)].tobytes())


def _queries(s, kmers, rank, n_present=300, n_other=60):
    """a rank's own queries: k-mers of the file on either strand, with repeats, and k-mers that are (almost surely) not in it"""
    rng = np.random.default_rng(100 + rank)
    parts = [_strangers(s, n_other, 1000 + rank)]
    if kmers.shape[0]:
        pick = kmers[rng.integers(0, kmers.shape[0], n_present)]
        parts += [pick, orc.revcomp(s, pick[::4])]
    return np.ascontiguousarray(np.concatenate(parts))


UPDATE_OPS = ("add", "max", "min", "assign")


def _stored(s, strand, kmers):
    return np.unique(orc.canonical(s, kmers) if strand == "canonical" else kmers, axis=0)


def _update_pairs(s, strand, stored, rank, world, op):
    """a rank's (key, value) pairs for update(): stored keys on either strand, repeats, keys the index does not hold; for assign
    every stored key appears in one pair on one rank only (the order of pairs of one key across ranks is not defined)"""
    rng = np.random.default_rng(7 * rank + UPDATE_OPS.index(op))
    if op == "assign":
        keys = stored[rank::world][:150]
    else:
        keys = stored[rng.integers(0, stored.shape[0], 200)]
    if strand == "canonical":
        keys = np.concatenate([keys[::2], orc.revcomp(s, keys[1::2])])
    keys = np.concatenate([keys, _strangers(s, 30, 50 + rank)])
    vals = {"add": rng.integers(0, 1 << 32, keys.shape[0]), "max": rng.integers(0, 12, keys.shape[0]), "min": rng.integers(1, 6, keys.shape[0]),
            "assign": rng.integers(0, 1 << 32, keys.shape[0])}[op].astype(np.uint64)
    return np.ascontiguousarray(np.concatenate([keys, vals.reshape(-1, 1)], axis=1))


def _erase_queries(s, kmers, rank):
    rng = np.random.default_rng(300 + rank)
    own = kmers[rank::5][:200]
    return np.ascontiguousarray(np.concatenate([own, orc.revcomp(s, kmers[rank::11][:50]), own[:40], kmers[rng.integers(0, kmers.shape[0], 30)],
                                                _strangers(s, 25, 70 + rank)]))


def _worker(rank, world, port, cases, ret, state):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), KMI_DIST_CHUNKS="3")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        out = []
        for ci, c in enumerate(cases):
            def say(what, ci=ci, c=c):
                state[rank] = "case %d (%s): %s" % (ci, _label(c), what)
            s = orc.kspec(c["k"], ALPHA[c["alpha"]])
            nw = s.n_words
            data, kind = c["data"], c["kind"]
            res = dict(rounds=[])
            size = C.c_uint64()
            if kind in ("count", "position", "posqual", "fasta-count", "fasta-position"):
                fasta = kind.startswith("fasta")
                ik = kind.split("-")[-1]
                cfg = K.make_config(c["k"], c["alpha"], strand=c["strand"], index_kind=ik, seq_format="fasta" if fasta else "fastq")
                idx = K.CountIndex(ctx, cfg) if ik == "count" else K.PositionIndex(ctx, cfg)
                vw = {"count": 1, "position": 1, "posqual": 2}[ik]
                if fasta:
                    say("build from the whole FASTA file")
                    buf = np.frombuffer(data, dtype=np.uint8).copy()
                    ctx.check(L.lib.kmi_index_build_fasta_file_dist_host(idx.h, comm.h, buf.ctypes.data_as(C.c_void_p), buf.size))
                else:
                    for d in (data, c["second"]):
                        if d is not None:
                            res["rounds"].append(_build_range(L.lib.kmi_index_build_range_dist_host, ctx, idx.h, comm.h, d, world, rank, c["look"], say))
                res["owner_ranks"] = idx.owner_ranks()
                say("size")
                ctx.check(L.lib.kmi_index_size_dist(idx.h, comm.h, C.byref(size)))
                res["size"] = size.value
                k0, v0 = idx.to_vector()
                res["keys"], res["vals"] = np.asarray(k0).reshape(-1, nw).copy(), np.asarray(v0).astype(np.uint64).reshape(-1, vw)
                kmers = orc.extract(s, data, orc.FASTA if fasta else orc.FASTQ)["kmers"]
                q = _queries(s, kmers, rank)
                res["q"] = q
                say("count")
                ck, cv = _query(L, ctx, L.lib.kmi_index_count_dist_host, idx.h, comm.h, q, nw, vw)   # (answers are as wide as the index's values)
                res["count"] = (ck, cv[:, :1].copy())
                say("find")
                res["find"] = _query(L, ctx, L.lib.kmi_index_find_dist_host, idx.h, comm.h, q, nw, vw)
                if c["extra"] == "update":
                    res["updates"] = []
                    stored = _stored(s, c["strand"], kmers)
                    for op in UPDATE_OPS:
                        say("update " + op)
                        pairs = _update_pairs(s, c["strand"], stored, rank, world, op)
                        nu = C.c_uint64()
                        ctx.check(L.lib.kmi_index_update_pairs_dist_host(idx.h, comm.h, pairs.ctypes.data_as(C.c_void_p), pairs.shape[0], UPDATE_OPS.index(op), C.byref(nu)))
                        k1, v1 = idx.to_vector()
                        res["updates"].append((nu.value, k1.copy(), np.asarray(v1).astype(np.uint64)))
                idx.close()
            else:
                g = K.DeBruijnNodes(ctx, K.make_config(c["k"], c["alpha"]), exists_only=c["exists"])
                res["rounds"].append(_build_range(L.lib.kmi_dbg_build_range_dist_host, ctx, g.h, comm.h, data, world, rank, c["look"], say))
                say("size")
                ctx.check(L.lib.kmi_dbg_size_dist(g.h, comm.h, C.byref(size)))
                res["size"] = size.value
                k0, v0 = g.to_vector()
                res["keys"], res["vals"] = np.asarray(k0).reshape(-1, nw).copy(), np.asarray(v0).astype(np.uint64).reshape(-1, 9)
                kmers = orc.dbg_parse(s, data)[0]
                q = _queries(s, kmers, rank, 200, 30)
                res["q"] = q
                say("find")
                res["find"] = _query(L, ctx, L.lib.kmi_dbg_find_dist_host, g.h, comm.h, q, nw, 5, dbg=True)
                if c["extra"] == "erase":
                    eq = _erase_queries(s, kmers, rank)
                    say("count")
                    res["count"] = _query(L, ctx, L.lib.kmi_dbg_count_dist_host, g.h, comm.h, eq, nw, 1)
                    say("erase")
                    ne = C.c_uint64()
                    ctx.check(L.lib.kmi_dbg_erase_dist_host(g.h, comm.h, eq.ctypes.data_as(C.c_void_p), eq.shape[0], C.byref(ne)))
                    ctx.check(L.lib.kmi_dbg_size_dist(g.h, comm.h, C.byref(size)))
                    k1, v1 = g.to_vector()
                    res["erase"] = (ne.value, size.value, np.asarray(k1).reshape(-1, nw).copy(), np.asarray(v1).astype(np.uint64).reshape(-1, 9))
                g.close()
            say("done")
            out.append(res)
        ret[rank] = out
        comm.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


def _run(world, cases, timeout=420):
    """one process group for the whole list of cases. The ranks get `timeout` seconds; when they have not come back by then they are
    ended and the test fails with what each rank was doing last -- nothing is tried again, here or in the tests that follow"""
    mgr = mp.Manager()
    ret, state = mgr.dict(), mgr.dict()
    pc = mp.spawn(_worker, args=(world, _free_port(), cases, ret, state), nprocs=world, join=False)
    deadline = time.monotonic() + timeout
    try:
        while not pc.join(timeout=2):
            if time.monotonic() > deadline:
                last = dict(state)
                GAVE_UP.append("the ranks did not come back within %d s; each rank's last state: %s" % (timeout, last))
                for p in pc.processes:
                    p.kill()
                pytest.fail(GAVE_UP[0])
    except mp.ProcessExitedException as e:   # a rank died of a signal
        GAVE_UP.append("%s; each rank's last state: %s" % (e, dict(state)))
        raise
    return [[ret[r][i] for r in range(world)] for i in range(len(cases))]


def _srows(keys, vals, nw, vw):
    """(key, value) rows in lexicographic order, for multiset comparison"""
    m = np.concatenate([np.asarray(keys, np.uint64).reshape(-1, nw), np.asarray(vals).astype(np.uint64).reshape(-1, vw)], axis=1)
    return m[np.lexsort([m[:, i] for i in range(m.shape[1] - 1, -1, -1)])] if m.shape[0] else m


def _eq(a, b, label):
    assert a.shape == b.shape, (label, a.shape, b.shape)
    assert (a == b).all(), (label, "first differing rows", a[(a != b).any(axis=1)][:3], b[(a != b).any(axis=1)][:3])


def _check_index(c, per_rank):
    """count / position / position + quality index: union, ownership, size, count and find against the oracle's single map"""
    label = _label(c)
    world = len(per_rank)
    s = orc.kspec(c["k"], ALPHA[c["alpha"]])
    nw = s.n_words
    ik = c["kind"].split("-")[-1]
    fmt = orc.FASTA if c["kind"].startswith("fasta") else orc.FASTQ
    vw = {"count": 1, "position": 1, "posqual": 2}[ik]
    if ik == "count":
        om = orc.CountMap(s, STRAND[c["strand"]])
    else:
        om = orc.MultiMap(s, STRAND[c["strand"]], vw)
    kmers = None
    for d in (c["data"], c["second"]):
        if d is None:
            continue
        ex = orc.extract(s, d, fmt, want_ids=ik != "count", want_quals=ik == "posqual")
        kmers = ex["kmers"] if kmers is None else kmers
        if ik == "count":
            om.insert(ex["kmers"])
        elif ik == "position":
            om.insert(ex["kmers"], ex["ids"].reshape(-1, 1))
        else:
            om.insert(ex["kmers"], np.concatenate([ex["ids"].reshape(-1, 1), ex["quals"].view(np.uint32).astype(np.uint64).reshape(-1, 1)], axis=1))
    keys = np.concatenate([p["keys"] for p in per_rank])
    _eq(_srows(keys, np.concatenate([p["vals"] for p in per_rank]), nw, vw), _srows(*om.export(), nw, vw), label + ": the union of the ranks' entries")
    owners = {}
    for r, p in enumerate(per_rank):
        for key in set(map(tuple, p["keys"].tolist())):
            assert owners.setdefault(key, r) == r, (label, "a key on two ranks", key)
        assert p["size"] == om.size(), (label, "size()", r)
        ck, cv = om.count(p["q"])
        _eq(_srows(*p["count"], nw, 1), _srows(ck, cv, nw, 1), label + ": count() of rank %d" % r)
        fk, fv = om.find(p["q"])
        _eq(_srows(*p["find"], nw, vw), _srows(fk, fv, nw, vw), label + ": find() of rank %d" % r)
    if c["extra"] == "owners":
        assert all(p["owner_ranks"] == world for p in per_rank), (label, [p["owner_ranks"] for p in per_rank])
    if c["extra"] == "update":
        model = IM.CountModel(c["k"], ALPHA[c["alpha"]], STRAND[c["strand"]])
        model.insert(kmers)
        stored = _stored(s, c["strand"], kmers)
        for i, op in enumerate(UPDATE_OPS):
            pairs = np.concatenate([_update_pairs(s, c["strand"], stored, r, world, op) for r in range(world)])
            hits = model.update_pairs(pairs[:, :nw], pairs[:, nw], op)
            assert hits > 0 and sum(p["updates"][i][0] for p in per_rank) == hits, (label, op, "n_updated over ranks")
            _eq(_srows(np.concatenate([p["updates"][i][1] for p in per_rank]), np.concatenate([p["updates"][i][2] for p in per_rank]), nw, 1),
                _srows(*model.export(), nw, 1), label + ": entries after update " + op)
    return [r for p in per_rank for r in p["rounds"]]


def _check_dbg(c, per_rank):
    """de Bruijn nodes with all nine counters against the oracle's map of the whole file: an edge between one rank's last read and
    the next rank's first, a read parsed twice or not at all, each shows in the counters"""
    label = _label(c)
    s = orc.kspec(c["k"], ALPHA[c["alpha"]])
    nw = s.n_words
    kmers, edges = orc.dbg_parse(s, c["data"])
    om = orc.DbgMap(s, exists_only=c["exists"])
    om.insert(kmers, edges)
    keys = np.concatenate([p["keys"] for p in per_rank])
    _eq(_srows(keys, np.concatenate([p["vals"] for p in per_rank]), nw, 9), _srows(*om.export(canonical=True), nw, 9), label + ": the union of the ranks' nodes")
    assert np.unique(keys, axis=0).shape[0] == keys.shape[0], (label, "a node on two ranks")
    for r, p in enumerate(per_rank):
        assert p["size"] == om.size(), (label, "size()", r)
        _eq(_srows(*p["find"], nw, 9), _srows(*om.find(p["q"], canonical=True), nw, 9), label + ": find() of rank %d" % r)
    if c["extra"] == "erase":
        model = IM.NodeModel(c["k"], ALPHA[c["alpha"]])
        model.insert(kmers, edges)
        for r, p in enumerate(per_rank):
            _eq(_srows(*p["count"], nw, 1), _srows(*model.count(_erase_queries(s, kmers, r)), nw, 1), label + ": count() of rank %d" % r)
        gone = model.erase(np.concatenate([_erase_queries(s, kmers, r) for r in range(len(per_rank))]))
        assert gone > 0 and sum(p["erase"][0] for p in per_rank) == gone, (label, "n_erased_local over ranks")
        assert all(p["erase"][1] == model.size() for p in per_rank), (label, "size() after erase")
        _eq(_srows(np.concatenate([p["erase"][2] for p in per_rank]), np.concatenate([p["erase"][3] for p in per_rank]), nw, 9),
            _srows(*model.export(), nw, 9), label + ": the nodes left after erase")
    return [r for p in per_rank for r in p["rounds"]]


def _check(c, per_rank):
    return _check_dbg(c, per_rank) if c["kind"] == "dbg" else _check_index(c, per_rank)


def _files():
    return [("tricky", M.tricky(24)), ("test.small.fastq", M.golden("test.small.fastq")), ("natural.withN.fastq", M.golden("natural.withN.fastq")),
            ("synth", _synth(3000, 30_000, 29))]


def _cases(world):
    files = _files()
    small_synth = ("synth-1200", _synth(1200, 10_000, 31))
    values = files[:3] + [small_synth]           # the position indexes and the graphs keep every tuple: a smaller synthetic file
    out = []
    # ---- count index through exchanged super-k-mers (2 and 4 ranks; a rank count that is no power of two takes the k-mer route)
    for name, d in files:
        out.append(_case("count", name, d, 31, extra="owners" if name == "synth" and world != 3 else None))
        out.append(_case("count", name, d, 21, strand="single", extra="owners" if name == "synth" and world != 3 else None))
    # ---- count index, k-mer route
    for name, d in files:
        if world == 2:
            out += [_case("count", name, d, 15), _case("count", name, d, 21, alpha="DNA5")]
        if world == 3:
            out += [_case("count", name, d, 63)]
        if world == 4:
            out += [_case("count", name, d, 15, strand="single"), _case("count", name, d, 63, strand="single"), _case("count", name, d, 21, alpha="DNA5")]
    # a second file into the filled index: counts add up
    out.append(_case("count", "synth", files[3][1], 31, second=files[2][1]))
    out.append(_case("count", "natural.withN.fastq", files[2][1], 15 if world != 3 else 31, second=files[0][1]))
    # ---- update() over ranks, on an index of either route
    out.append(_case("count", "synth", files[3][1], 31, extra="update"))
    out.append(_case("count", "natural.withN.fastq", files[2][1], 15, strand="single", extra="update"))
    # ---- position and position + quality index
    for name, d in values:
        out += [_case("position", name, d, 31), _case("posqual", name, d, 21)]
    # ---- de Bruijn nodes
    for name, d in values:
        out += [_case("dbg", name, d, 21), _case("dbg", name, d, 31), _case("dbg", name, d, 40, alpha="DNA5")]
    out.append(_case("dbg", "natural.withN.fastq", files[2][1], 31, exists=True))
    if world == 3:
        out.append(_case("dbg", "synth-1200", small_synth[1], 31, extra="erase"))
        out.append(_case("dbg", "tricky", files[0][1], 21, extra="erase"))
    # ---- a FASTA file every rank holds whole
    if world in (2, 3):
        fa = M.golden("test.fasta")
        out += [_case("fasta-count", "test.fasta", fa, 15), _case("fasta-position", "test.fasta", fa, 15)]
    return out


@pytest.mark.parametrize("world", [2, 3, 4])
def test_collective_builds_by_byte_range(world):
    """block r of the equal split per rank, 16 bytes of look-ahead to begin with. Against the oracle's single map of the whole
    file: the union of the ranks' exports is that map, no key sits on two ranks, size() is the oracle's on every rank, every
    rank's own count / find queries get the oracle's answers, and some rank had to read further. With it the collectives that
    had only run on one rank: update() with every updater, erase / count of the node map, the build from a whole FASTA file."""
    cases = _cases(world)
    res = _run(world, cases)
    rounds = []
    for c, per_rank in zip(cases, res):
        rounds += _check(c, per_rank)
    assert any(r > 1 for r in rounds)


def test_one_record_over_four_ranks():
    """test.debruijn.tiny.fastq holds one record: three of four ranks hold nothing and still enter every collective"""
    d = M.golden("test.debruijn.tiny.fastq")
    name = "test.debruijn.tiny.fastq"
    cases = [_case("count", name, d, 31), _case("count", name, d, 21, strand="single"), _case("count", name, d, 15), _case("count", name, d, 21, alpha="DNA5"),
             _case("count", name, d, 31, second=M.tricky(24)), _case("count", name, d, 63), _case("position", name, d, 31), _case("posqual", name, d, 21),
             _case("dbg", name, d, 21), _case("dbg", name, d, 31), _case("dbg", name, d, 40, alpha="DNA5"), _case("dbg", name, d, 21, exists=True)]
    res = _run(4, cases, timeout=240)
    for c, per_rank in zip(cases, res):
        _check(c, per_rank)


def _record(rng, tag, n=50, eol=b"\n", qual=None):
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    return b"@" + tag + eol + seq + eol + b"+" + eol + (qual if qual is not None else b"I" * n) + eol


def _pinned(before, after, seed, eol=b"\n", blank_tail=False):
    """pad so that the two-way split n // 2 falls exactly between `before` and `after`: a record in front and one behind
    (blank_tail: only blank lines behind, for a cut inside the file's last record)"""
    rng = np.random.default_rng(seed)
    rec_len = lambda n: 3 + 2 * n + 4 * len(eol)
    for a in range(30, 600):
        for b in range(30, 600):
            left, right = rec_len(a) + len(before), len(after) + (b * len(eol) if blank_tail else rec_len(b))
            if (left + right) // 2 == left:
                data = _record(rng, b"p", a, eol) + before + after + (eol * b if blank_tail else _record(rng, b"q", b, eol))
                assert len(data) // 2 == rec_len(a) + len(before)
                return data
    raise AssertionError("no padding found")


def _pinned_cuts():
    rng = np.random.default_rng(9)
    r = [_record(rng, b"r%d" % i, 50) for i in range(4)]
    rc = [_record(rng, b"c%d" % i, 50, b"\r\n") for i in range(3)]
    at_qual = _record(rng, b"a", 50, qual=(b"@" * 50))
    h, s, p, q = at_qual.split(b"\n")[:4]
    # place: (bytes before the cut, bytes from the cut on, the byte the cut falls on, how to pad)
    out = {
        "on the '@' that opens a record": (r[0], r[1] + r[2], b"@", {}),
        "on the '\\n' before a record": (r[0][:-1], b"\n" + r[1] + r[2], b"\n", {}),
        "between '\\r' and '\\n'": (rc[0][:-1], b"\n" + rc[1] + rc[2], b"\n", dict(eol=b"\r\n")),
        "on the first byte of a quality line that begins with '@'": (r[0] + h + b"\n" + s + b"\n" + p + b"\n", q + b"\n" + r[1], b"@", {}),
        "on the '+'": (r[0] + h + b"\n" + s + b"\n", p + b"\n" + q + b"\n" + r[1], b"+", {}),
        "on the last byte of the file's last record": (r[0] + r[1][:-1], b"\n", b"\n", dict(blank_tail=True)),
        "on the last quality character of the file's last record": (r[0] + r[1][:-2], r[1][-2:], b"I", dict(blank_tail=True)),
    }
    return {name: (_pinned(b, a, 100 + i, **kw), at) for i, (name, (b, a, at, kw)) in enumerate(out.items())}


def test_pinned_cuts():
    """two ranks, the cut n // 2 placed on purpose; each place is its own assertion against the oracle, for a position index
    (whose ids are file positions) and a node map, with 16 bytes and with 64 KB of look-ahead"""
    pinned = _pinned_cuts()
    cases = []
    for name, (data, at) in pinned.items():
        c = len(data) // 2
        assert data[c:c + 1] == at, name                                        # the places are where they are meant to be
        for look in (16, 1 << 16):
            cases += [_case("position", name, data, 21, look=look), _case("dbg", name, data, 21, look=look), _case("count", name, data, 15, look=look)]
    d = pinned["between '\\r' and '\\n'"][0]
    assert d[len(d) // 2 - 1:len(d) // 2 + 1] == b"\r\n"
    d = pinned["on the '@' that opens a record"][0]
    assert len(d) // 2 in M.true_record_starts(d) and M.partition_of(d, 0, len(d) // 2, 16, 16)[1] > len(d) // 2      # that record belongs to rank 0
    d = pinned["on the first byte of a quality line that begins with '@'"][0]
    assert len(d) // 2 not in M.true_record_starts(d)
    res = _run(2, cases, timeout=240)
    for c, per_rank in zip(cases, res):
        _check(c, per_rank)
