"""A FASTA file over ranks by BYTE RANGE, at every cut and at the seams of the scan. A rank holds file bytes [lo, hi) plus
look-ahead, wherever that cuts; what it cannot know from its own bytes comes from the other ranks' block summaries
(kmi_fasta_block_summary_dev: the line-kind machine over a block as a transfer function), composed left to right, and a de Bruijn
block's in-edge from their left carries, composed right to left. Checked here:

  a, b  kmi_fasta_block_summary_dev against tests/fasta_block_model.py (pinned on the CPU by tests/test_fasta_block_model.py):
        every prefix and suffix of small inputs, and the seams of the scan's units -- the 16-byte chunk, the 1024-byte wavefront,
        the 8192-byte tile and the group of 1024 tiles
  c, d  kmi_extract_fasta_range_dist_host at every two-way and three-way cut, against the oracle's parse of the whole file
  e     kmi_index_build_fasta_range_dist_host at every two-way cut, against the oracle's MultiMap
  f, g  kmi_dbg_build_fasta_range_dist_host at every two- and three-way cut and with the carry crossing tiles and groups, against
        the oracle's node map of the whole file
  h     kmi_fasta_partition_dev against the model's partition of the equal split

The range functions take any tiling of the file in rank order, so a sweep over every cut drives them. Ranks are processes that
share GPU 0 over a gloo group (kmerind_amd/transport.py), as in test_gpu_fastq_ranges.py. Every comparison is exact."""
import ctypes as C
import os
import socket
import time

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import fasta_block_model as M
from tests import oracle as orc

pytestmark = pytest.mark.gpu
ALPHA = {"DNA": orc.DNA, "DNA5": orc.DNA5}
POS = np.uint64((1 << 40) - 1)
TILE, GROUP = 8192, 8192 * 1024

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


class _OnDevice:
    """a buffer in HBM for the length of a `with`"""

    def __init__(self, ctx, data):
        self.ctx, self.data = ctx, data

    def __enter__(self):
        self.d = self.ctx.alloc(len(self.data) + 64)
        self.ctx.to_device(self.d, np.frombuffer(self.data, dtype=np.uint8))
        return self.d

    def __exit__(self, *exc):
        self.ctx.free(self.d)


def _summary(ctx, dptr, n_bytes, first_ls):
    from kmerind_amd import _lib as L
    out = np.full(6, 0xDEADBEEF, dtype=np.uint64)
    ctx.check(L.lib.kmi_fasta_block_summary_dev(ctx.h, C.c_void_p(dptr), n_bytes, first_ls, out.ctypes.data_as(C.c_void_p)))
    return [int(x) for x in out]


# ---------------------------------------------------------------------------
# a. the summary of every prefix and every suffix
# ---------------------------------------------------------------------------
def _summary_inputs():
    return M.small_inputs() + [("wave", M.wave_input())]


@pytest.mark.parametrize("name,data", _summary_inputs(), ids=[x[0] for x in _summary_inputs()])
def test_summary_of_every_prefix_and_suffix(ctx, name, data):
    """all six words -- the state behind the bytes and the records started, for each of the three incoming states -- of data[:m]
    for every m and of data[c:] for every c (passed as d + c, an unaligned device pointer), each with first_is_line_start 1 and
    0: with 0 a buffer whose first byte is '>' or ';' opens no header line. n_bytes = 0 is the identity."""
    n = len(data)
    if name == "wave":
        assert 2 * 1024 + 200 < n < 3 * 1024
    compared = 0
    with _OnDevice(ctx, data) as d:
        for fl in (1, 0):
            assert _summary(ctx, d, 0, fl) == [0, 0, 1, 0, 2, 0]
            for m in range(1, n + 1):
                assert _summary(ctx, d, m, fl) == M.summary(data[:m], bool(fl)), (name, "data[:%d]" % m, fl)
            for c in range(1, n):
                assert _summary(ctx, d + c, n - c, fl) == M.summary(data[c:], bool(fl)), (name, "data[%d:]" % c, fl)
            compared += 2 * n
    firsts = [c for c in range(n) if data[c:c + 1] in (b">", b";")]
    assert firsts and any(M.summary(data[c:], True) != M.summary(data[c:], False) for c in firsts)
    print("\n(a) %s: %d summaries compared" % (name, compared))


# ---------------------------------------------------------------------------
# b. the summary at the seams of the scan's units
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", [16, 1024, TILE, GROUP])
def test_summary_at_a_seam(ctx, B):
    """B = a chunk, a wavefront, a tile, a group of tiles. Across byte B: '\\n' | '>', '\\n' | the first sequence byte behind a
    header (a record starts exactly at B), '\\r' | '\\n', a header line, a sequence line; buffers of B - 1, B, B + 1 and
    B + 8193 bytes (the seam is the buffer's last byte, lies just behind it, is followed by one byte, by a tile and a byte)"""
    compared = 0
    for name, data in M.seam_inputs(B, line=60 if B < GROUP else 65521):
        with _OnDevice(ctx, data) as d:
            for m in (B - 1, B, B + 1, B + 8193):
                for fl in (1, 0):
                    assert _summary(ctx, d, m, fl) == M.summary(data[:m], bool(fl)), (B, name, m, fl)
                    compared += 1
    print("\n(b) seam %d: %d summaries compared" % (B, compared))


def _three_groups():
    """just over two groups of tiles (16.8 MB): a record start in each of the three groups, lines of 65521 characters"""
    g = np.random.default_rng(17)
    line = M._seq(g, 65521) + b"\n"
    out, size = [], 0
    for i, at in enumerate((3 * TILE + 5, GROUP + 1023 * TILE + 77, 2 * GROUP + 11)):
        while size + len(line) <= at - 8:
            out.append(line)
            size += len(line)
        pad = at - 7 - size                      # a last line that ends where the header has to begin
        out += [M._seq(g, pad - 1) + b"\n", b">rec %d\n" % i]
        size += pad + 7
        assert size == at
    out += [M._seq(g, 3000) + b"\n", M._seq(g, 1000)]
    data = b"".join(out)
    starts = [p[0] for p in M.walk(data, True, M.OUTSIDE) if p[3]]
    assert [s // GROUP for s in starts] == [0, 1, 2] and 2 * GROUP < len(data) < 2 * GROUP + TILE
    return data, starts


def test_summary_over_three_groups(ctx):
    """the host loop over the groups' summaries: a record start in each of three groups, the buffer cut short behind each of them
    and at the groups' seams"""
    data, starts = _three_groups()
    n = len(data)
    with _OnDevice(ctx, data) as d:
        lengths = [n, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP, 2 * GROUP + 1] + [s + x for s in starts for x in (0, 1)]
        for m in lengths:
            for fl in (1, 0):
                got = _summary(ctx, d, m, fl)
                assert got == M.summary(data[:m], bool(fl)), (m, fl)
        assert _summary(ctx, d, n, 1)[1::2] == [3, 4, 3]     # (entered in HEADER, the lines in front of the first header are a record)
        c = GROUP - 3                                      # a suffix that begins inside a line, at an odd address
        assert _summary(ctx, d + c, n - c, 0) == M.summary(data[c:], False)
    print("\n(b) three groups: %d summaries compared" % (2 * len(lengths) + 2))


# ---------------------------------------------------------------------------
# h. kmi_fasta_partition_dev against the model
# ---------------------------------------------------------------------------
FIELDS = ("begin", "end", "valid_bytes", "start_state", "at_line_start", "records_before", "index_shift")


def _partition_dev(ctx, dptr, n, p, k):
    from kmerind_amd import _lib as L
    be = np.zeros(2 * p, dtype=np.uint64)
    parts = (L.FastaPartition * p)()
    ctx.check(L.lib.kmi_fasta_partition_dev(ctx.h, C.c_void_p(dptr), n, p, k, be.ctypes.data_as(C.c_void_p), parts))
    return [dict(begin=int(be[2 * r]), end=int(be[2 * r + 1]), valid_bytes=int(parts[r].valid_bytes), start_state=int(parts[r].start_state),
                 at_line_start=int(parts[r].at_line_start), records_before=int(parts[r].records_before), index_shift=int(parts[r].index_shift))
            for r in range(p)]


def _compare_partitions(ctx, d, data, p, k, mask, label):
    got = _partition_dev(ctx, d, len(data), p, k)
    cuts = M.equal_cuts(len(data), p)
    for r in range(p):
        exp = M.partition(data, cuts, r, k, mask)
        assert got[r] == exp, (label, "p=%d k=%d block %d" % (p, k, r), got[r], exp)
    return p


@pytest.mark.parametrize("name", ["main", "opens-with-semicolon"])
def test_partition_dev_every_part_count(ctx, name):
    """p = 1 .. n + 3 blocks of the equal split: begin, end and the five fields of every block. Beyond p = n blocks are empty."""
    data = dict(M.small_inputs())[name]
    n = len(data)
    mask = M.seq_mask(data)
    blocks = 0
    with _OnDevice(ctx, data) as d:
        for k in (5, 1):
            for p in range(1, n + 4):
                blocks += _compare_partitions(ctx, d, data, p, k, mask, name)
    print("\n(h) %s: %d blocks compared" % (name, blocks))


def test_partition_dev_at_tile_seams(ctx):
    """n = 3 x 8192 with p = 3 and 6 (cuts at 8192, 16384 and 4096, ...) and n = 3 x 8192 + 3 with p = 3 (cuts one byte behind a
    tile's first byte), with the seam placements of test_summary_at_a_seam at the first and at the second cut"""
    blocks = 0
    for n, ps in ((3 * TILE, (3, 6)), (3 * TILE + 3, (3,))):
        for B in (n // 3, 2 * n // 3):
            for name, data in M.seam_inputs(B, tail=n - B):
                assert len(data) == n
                mask = M.seq_mask(data)
                with _OnDevice(ctx, data) as d:
                    for p in ps:
                        assert B in M.equal_cuts(n, p)
                        for k in (21, 2):
                            blocks += _compare_partitions(ctx, d, data, p, k, mask, (n, B, name))
    print("\n(h) tile seams: %d blocks compared" % blocks)


# ---------------------------------------------------------------------------
# c - g. the collectives over 2, 3 and 4 ranks
# ---------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _job(kind, name, data, k, alpha, tilings, look=16):
    """kind: extract | index | dbg. tilings: [cuts], cuts = the file positions 0 = c0 <= c1 <= ... <= c_world = n; rank r holds
    [c_r, c_r+1) and `look` bytes of look-ahead to begin with, 16 times more each time the library asks"""
    return dict(kind=kind, name=name, data=data, k=k, alpha=alpha, tilings=tilings, look=look)


def _two_way(n):
    return [[0, c, n] for c in range(n + 1)]


def _three_way(n):
    return [[0, c1, c2, n] for c1 in range(n + 1) for c2 in range(c1, n + 1)]


def _rank_rounds(call, data, lo, hi, look):
    """the rank's calls on [lo, hi) + look-ahead until the library has enough: [(look, reaches_eof, need_more, what call returned)]"""
    n = len(data)
    rounds = []
    while True:
        end = min(n, hi + look)
        buf = np.frombuffer(data[lo:end], dtype=np.uint8).copy()
        need = C.c_int(0)
        got = call(buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, lo, hi - lo, 1 if end == n else 0,
                   data[lo - 1] if lo > 0 else -1, need)
        rounds.append((look, end == n, need.value, got))
        if not need.value:
            return rounds
        assert end < n, "need_more on a buffer that reaches the file's end"     # (asking again would change nothing)
        look *= 16


def _worker(rank, world, port, jobs, ret, state):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        out = []
        for ji, job in enumerate(jobs):
            data, k, kind = job["data"], job["k"], job["kind"]
            nw = orc.kspec(k, ALPHA[job["alpha"]]).n_words
            cfg = K.make_config(k, job["alpha"], seq_format="fasta", index_kind="count" if kind == "dbg" else "position")
            res = []
            t0 = time.perf_counter()
            for ti, cuts in enumerate(job["tilings"]):
                state[rank] = "job %d (%s %s k=%d), tiling %d %s" % (ji, kind, job["name"], k, ti, cuts)
                lo, hi = cuts[rank], cuts[rank + 1]
                if kind == "extract":
                    def call(ptr, nb, off, nominal, eof, prev, need):
                        t = L.Tuples()
                        ctx.check(L.lib.kmi_extract_fasta_range_dist_host(ctx.h, C.byref(cfg), comm.h, ptr, nb, off, nominal, eof, prev, C.byref(need), C.byref(t)))
                        nt = t.n_tuples
                        km = np.ctypeslib.as_array(t.kmers, shape=(nt * nw,)).copy().reshape(nt, nw) if nt else np.zeros((0, nw), np.uint64)
                        ids = np.ctypeslib.as_array(t.ids, shape=(nt,)).copy() if nt and t.ids else np.zeros(0, np.uint64)
                        L.lib.kmi_tuples_free(C.byref(t))
                        return km, ids
                    res.append(_rank_rounds(call, data, lo, hi, job["look"]))
                else:
                    obj = K.PositionIndex(ctx, cfg) if kind == "index" else K.DeBruijnNodes(ctx, cfg)
                    fn = L.lib.kmi_index_build_fasta_range_dist_host if kind == "index" else L.lib.kmi_dbg_build_fasta_range_dist_host

                    def call(ptr, nb, off, nominal, eof, prev, need):
                        ctx.check(fn(obj.h, comm.h, ptr, nb, off, nominal, eof, prev, C.byref(need)))
                        return None
                    rounds = _rank_rounds(call, data, lo, hi, job["look"])
                    keys, vals = obj.to_vector()
                    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, nw).copy()
                    vals = np.asarray(vals).astype(np.uint64).reshape(keys.shape[0], 1 if kind == "index" else 9)
                    obj.close()
                    res.append((rounds, keys, vals))
            out.append((res, time.perf_counter() - t0))
        state[rank] = "done"
        ret[rank] = out
        comm.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


def _run(world, jobs, timeout=240):
    """one process group for the whole list of jobs. The ranks get `timeout` seconds; when they have not come back by then they
    are ended and the test fails with what each rank was doing last -- nothing is tried again, here or in the tests that follow.
    -> per job: ([per tiling: [per rank: result]], seconds the slowest rank spent in it)"""
    for job in jobs:
        for cuts in job["tilings"]:
            assert len(cuts) == world + 1 and cuts[0] == 0 and cuts[-1] == len(job["data"]) and all(a <= b for a, b in zip(cuts, cuts[1:]))
    mgr = mp.Manager()
    ret, state = mgr.dict(), mgr.dict()
    pc = mp.spawn(_worker, args=(world, _free_port(), jobs, ret, state), nprocs=world, join=False)
    deadline = time.monotonic() + timeout
    try:
        while not pc.join(timeout=2):
            if time.monotonic() > deadline:
                GAVE_UP.append("the ranks did not come back within %d s; each rank's last state: %s" % (timeout, dict(state)))
                for p in pc.processes:
                    p.kill()
                pytest.fail(GAVE_UP[0])
    except mp.ProcessExitedException as e:   # a rank died of a signal
        GAVE_UP.append("%s; each rank's last state: %s" % (e, dict(state)))
        raise
    except Exception as e:                   # a rank raised: the others wait in a collective for it
        GAVE_UP.append("%s; each rank's last state: %s" % (str(e).strip().splitlines()[-1], dict(state)))
        raise
    outs = [ret[r] for r in range(world)]    # (one transfer per rank: every look into the manager's dict copies the whole value)
    return [([[outs[r][j][0][t] for r in range(world)] for t in range(len(job["tilings"]))], max(outs[r][j][1] for r in range(world)))
            for j, job in enumerate(jobs)]


def _check_rounds(job, cuts, r, rounds, behind):
    """need_more comes with nothing parsed, never on a buffer that reaches the file's end, and only where the model says the
    look-ahead does not hold `behind` sequence characters for every state the block may end in (an upper bound on the rounds:
    a library that asks less often still passes)"""
    label = (job["kind"], job["name"], job["k"], cuts, "rank %d" % r)
    for look, eof, need, got in rounds:
        if need:
            assert not eof, label
            assert not M.lookahead_suffices(job["data"], cuts[r], cuts[r + 1], look, behind), (label, "need_more with %d bytes of look-ahead" % look)
            if got is not None:
                assert got[0].shape[0] == 0 and got[1].size == 0, (label, "tuples returned with need_more")
    assert not rounds[-1][2], label
    return sum(1 for x in rounds if x[2])


def _check_extract(job, per_tiling):
    """per rank, from the oracle alone: the whole file's tuples whose position lies in [lo, hi), k-mers and ids in file order"""
    s = orc.kspec(job["k"], ALPHA[job["alpha"]])
    ex = orc.extract(s, job["data"], orc.FASTA, want_ids=True)
    assert ex["kmers"].shape[0] > 0, job["name"]
    pos = ex["ids"] & POS
    asked = 0
    for cuts, per_rank in zip(job["tilings"], per_tiling):
        for r, rounds in enumerate(per_rank):
            asked += _check_rounds(job, cuts, r, rounds, job["k"] - 1)
            km, ids = rounds[-1][3]
            sel = (pos >= np.uint64(cuts[r])) & (pos < np.uint64(cuts[r + 1]))
            label = (job["name"], job["k"], job["alpha"], cuts, "rank %d" % r)
            assert km.shape[0] == int(sel.sum()), (label, km.shape[0], int(sel.sum()))
            assert (ids == ex["ids"][sel]).all(), (label, "ids")
            assert (km == ex["kmers"][sel]).all(), (label, "k-mers")
    return asked


def _rows(keys, vals):
    if keys.shape[0] == 0:
        return np.zeros((0, 0), np.uint64)
    return orc.sorted_rows(keys, vals)


def _check_maps(job, per_tiling):
    """the union of the ranks' entries is the oracle's single map of the whole file: (key, id) rows of a position index, nodes
    with all nine counters of a de Bruijn graph; no need_more without cause"""
    s = orc.kspec(job["k"], ALPHA[job["alpha"]])
    if job["kind"] == "index":
        ex = orc.extract(s, job["data"], orc.FASTA, want_ids=True)
        om = orc.MultiMap(s, orc.CANONICAL, 1)
        om.insert(ex["kmers"], ex["ids"].reshape(-1, 1))
        exp = _rows(*om.export())
    else:
        om = orc.DbgMap(s)
        om.insert(*orc.dbg_parse(s, job["data"], orc.FASTA))
        exp = _rows(*om.export(canonical=True))
    assert exp.shape[0] > 0, job["name"]
    asked = 0
    for cuts, per_rank in zip(job["tilings"], per_tiling):
        for r, (rounds, _, _) in enumerate(per_rank):
            asked += _check_rounds(job, cuts, r, rounds, job["k"] - 1 if job["kind"] == "index" else job["k"])
        got = _rows(np.concatenate([p[1] for p in per_rank]), np.concatenate([p[2].reshape(p[1].shape[0], exp.shape[1] - s.n_words) for p in per_rank]))
        label = (job["kind"], job["name"], job["k"], job["alpha"], cuts)
        assert got.shape == exp.shape, (label, got.shape, exp.shape)
        assert (got == exp).all(), (label, "first differing rows", got[(got != exp).any(axis=1)][:3], exp[(got != exp).any(axis=1)][:3])
    return asked


def _report(section, jobs, results, asked):
    for job, (_, seconds) in zip(jobs, results):
        print("\n(%s) %s %s k=%d %s look=%d: %d tilings, %.2f s in the ranks" % (section, job["kind"], job["name"], job["k"], job["alpha"], job["look"],
                                                                            len(job["tilings"]), seconds))
    print("(%s) need_more answered %d times" % (section, asked))


@pytest.mark.parametrize("look", [16, 1])
def test_extract_at_every_two_way_cut(look):
    """(c) rank 0 holds [0, c), rank 1 [c, n), for every c = 0 .. n: empty first and last blocks, cuts between '\\r' and '\\n',
    inside headers and blank lines; ids are file positions, so buffer_offset is the file offset of the buffer"""
    inputs = dict(M.small_inputs())
    m = inputs["main"]
    jobs = [_job("extract", "main", m, 15, "DNA", _two_way(len(m)), look), _job("extract", "main", m, 21, "DNA5", _two_way(len(m)), look)]
    jobs += [_job("extract", name, inputs[name], 5, "DNA", _two_way(len(inputs[name])), look) for name in ("main-crlf", "opens-with-header", "opens-with-semicolon")]
    results = _run(2, jobs)
    asked = sum(_check_extract(job, res) for job, (res, _) in zip(jobs, results))
    assert asked > 0            # some rank had to read further
    _report("c", jobs, results, asked)


def test_extract_at_every_three_way_cut():
    """(d) every c1 <= c2 of the 48-byte input over three ranks: empty first, middle and last blocks, and blocks with no line
    start and no sequence character, which the incoming state passes straight through"""
    data = M.three_way_input()
    jobs = [_job("extract", "three-way", data, 4, "DNA", _three_way(len(data)), 16), _job("extract", "three-way", data, 4, "DNA", _three_way(len(data)), 1)]
    results = _run(3, jobs)
    asked = sum(_check_extract(job, res) for job, (res, _) in zip(jobs, results))
    assert asked > 0
    _report("d", jobs, results, asked)


def test_position_index_at_every_two_way_cut():
    """(e) the union of the two ranks' (key, id) rows is the oracle's multimap of the whole file, at every cut. The ids hold the
    sequence index: with rank 0 holding nothing the index shift still comes from the file's first byte, for a file with orphan
    lines in front of the first header and for one that opens with a header"""
    inputs = dict(M.small_inputs())
    jobs = [_job("index", name, inputs[name], 15, "DNA", _two_way(len(inputs[name]))) for name in ("main", "opens-with-header")]
    results = _run(2, jobs)
    asked = sum(_check_maps(job, res) for job, (res, _) in zip(jobs, results))
    _report("e", jobs, results, asked)


def test_debruijn_nodes_at_every_two_way_cut():
    """(f) the union of the node maps, with all nine counters: an in-edge lost or invented at the cut shows in them"""
    inputs = dict(M.small_inputs())
    jobs = [_job("dbg", "main", inputs["main"], 5, "DNA", _two_way(len(inputs["main"]))),
            _job("dbg", "main-crlf", inputs["main-crlf"], 15, "DNA5", _two_way(len(inputs["main-crlf"])))]
    results = _run(2, jobs)
    asked = sum(_check_maps(job, res) for job, (res, _) in zip(jobs, results))
    assert asked > 0
    _report("f", jobs, results, asked)


def test_debruijn_nodes_at_every_three_way_cut():
    """(f) three ranks, every c1 <= c2 of the 48-byte input: the middle block may hold no sequence character and no record start,
    then the third block's in-edge comes from the first"""
    data = M.three_way_input()
    jobs = [_job("dbg", "three-way", data, 4, "DNA", _three_way(len(data)))]
    results = _run(3, jobs)
    asked = sum(_check_maps(job, res) for job, (res, _) in zip(jobs, results))
    _report("f", jobs, results, asked)


# ---- g. the carry across tiles and groups
def _carry_cases():
    """name -> (data, cuts): two ranks, the cut placed on purpose. Rank 1 always continues with sequence characters; whether they
    continue rank 0's record, and behind which base, is decided many tiles earlier"""
    g = np.random.default_rng(23)
    seq = lambda n: M._seq(g, n)
    tail = seq(50) + b"\n>z\n" + seq(30) + b"\n"
    out = {}
    for G in (TILE + 10, 2 * TILE + 10, GROUP + 10):
        for eol, ename in ((b"\n", "LF"), (b"\r\n", "CR-LF")):
            blank = eol * (G // len(eol))
            left = b">r\n" + seq(59) + b"C" + eol + blank
            out["%d bytes of %s blank lines behind the last character" % (G, ename)] = (left + tail, [0, len(left), len(left) + len(tail)])
            left = b">r\n" + seq(60) + eol + b">h2" + eol + eol + blank
            out["a header, a blank line and %d bytes of %s blank lines" % (G, ename)] = (left + tail, [0, len(left), len(left) + len(tail)])
    # group 0 has its last event in its last tile, group 1 one in its first tile, behind another base: the LAST group decides
    a = b">r\n" + seq(60) + b"\n"
    a += b"\n" * (1023 * TILE + 100 - len(a)) + seq(30) + b"T\n"
    a += b"\n" * (GROUP + 50 - len(a)) + seq(30) + b"A\n" + b"\n" * 40
    assert a[1023 * TILE + 130:1023 * TILE + 131] == b"T" and a[GROUP + 80:GROUP + 81] == b"A" and len(a) < GROUP + TILE
    out["groups: T in tile 1023 of group 0, A in tile 0 of group 1"] = (a + tail, [0, len(a), len(a) + len(tail)])
    # inside one tile an earlier T and a later A, in different wavefronts: the later one decides, not the larger byte
    b = b">r\n" + seq(60) + b"\n" + b"\n" * 9000
    b += seq(40) + b"T\n" + b"\n" * 2000 + seq(10) + b"A\n" + b"\n" * 100
    first, last = b.rindex(b"T\n"), b.rindex(b"A\n")
    assert first // TILE == last // TILE == 1 and last - first > 1024
    out["tile: an earlier T, a later A"] = (b + tail, [0, len(b), len(b) + len(tail)])
    return out


def test_carry_across_tiles_and_groups():
    """(g) k = 21, two ranks. The in-edge of rank 1's first window is rank 0's last sequence character -- or none, when a record
    starts behind it -- found in the first of many tiles or groups of rank 0's block. Each case is its own assertion against
    the oracle's map of the whole file."""
    cases = _carry_cases()
    jobs = [_job("dbg", name, data, 21, "DNA", [cuts]) for name, (data, cuts) in cases.items()]
    results = _run(2, jobs)
    for job, (res, _) in zip(jobs, results):
        _check_maps(job, res)
    _report("g", jobs, results, 0)


def test_carry_through_two_ranks_of_blank_lines():
    """(g) four ranks; ranks 1 and 2 hold 20 KB of blank lines each (LF, CR-LF): two and a half tiles that pass rank 0's carry on"""
    g = np.random.default_rng(29)
    head = b">r\n" + M._seq(g, 70) + b"\n"
    tail = M._seq(g, 60) + b"\n>q\n" + M._seq(g, 40) + b"\n"
    data = head + b"\n" * 20480 + b"\r\n" * 10240 + tail
    cuts = [0, len(head), len(head) + 20480, len(head) + 40960, len(data)]
    head2 = head + b";h\n\n"                   # the same behind a header and a blank line: no in-edge
    data2 = head2 + b"\n" * 20480 + b"\r\n" * 10240 + tail
    cuts2 = [0, len(head2), len(head2) + 20480, len(head2) + 40960, len(data2)]
    jobs = [_job("dbg", "20 KB of blank lines on ranks 1 and 2", data, 21, "DNA", [cuts]),
            _job("dbg", "a header, then 20 KB of blank lines on ranks 1 and 2", data2, 21, "DNA", [cuts2])]
    results = _run(4, jobs)
    for job, (res, _) in zip(jobs, results):
        _check_maps(job, res)
    _report("g", jobs, results, 0)
