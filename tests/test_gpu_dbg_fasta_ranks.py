"""The de Bruijn node map from a FASTA file over ranks by BYTE RANGE (kmi_dbg_build_fasta_range_dist_host; the engine's
build_posix<FASTAParser> with comm.size() > 1). Every rank holds 1/p of the file's bytes plus look-ahead, wherever that cuts; the
edges at a block boundary are what a graph adds to the index's bookkeeping: the in-edge of the block's first window comes from the
blocks before it (their left carries, composed over blocks that hold no sequence character), and the block's last window needs k
sequence characters behind the block, not k - 1. Checked against the oracle's single map of the whole file: the union of the
ranks' nodes, with all nine counters, must be that map whatever the rank count and wherever the cuts fall. Ranks share one GPU
over a gloo group (kmerind_amd/transport.py), as in test_gpu_dist_clayer.py."""
import ctypes as C
import os
import re
import socket
import subprocess
import tempfile

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import oracle as orc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "data")
ALPHA = {"DNA": orc.DNA, "DNA5": orc.DNA5}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _n_words(k, alpha):
    return (k * (3 if alpha == "DNA5" else 2) + 63) // 64


def _block(n, world, rank):
    lo = n // world * rank + (n % world) * rank // world
    hi = n if rank + 1 == world else n // world * (rank + 1) + (n % world) * (rank + 1) // world
    return lo, hi


def _build_range(L, ctx, g, comm_h, data, world, rank, look):
    """what the facade's build_posix does: the block plus look-ahead, more when the library asks; returns the rounds taken"""
    n = len(data)
    lo, hi = _block(n, world, rank)
    rounds = 0
    while True:
        end = min(n, hi + look)
        buf = np.frombuffer(data[lo:end], dtype=np.uint8).copy()
        need = C.c_int(0)
        ptr = buf.ctypes.data_as(C.c_void_p) if buf.size else None
        ctx.check(L.lib.kmi_dbg_build_fasta_range_dist_host(g.h, comm_h, ptr, buf.size, lo, hi - lo, 1 if end == n else 0,
                                                            data[lo - 1] if lo > 0 else -1, C.byref(need)))
        rounds += 1
        if not need.value:
            return rounds
        look *= 16


def _worker(rank, world, port, cases, ret):
    """cases: (data, k, alpha, exists_only, look). Per case: (keys, counts9, size_dist, find keys, find values, rounds)"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        out = []
        for data, k, alpha, exists, look in cases:
            nw = _n_words(k, alpha)
            g = K.DeBruijnNodes(ctx, K.make_config(k, alpha, seq_format="fasta"), exists_only=exists)
            rounds = _build_range(L, ctx, g, comm.h, data, world, rank, look)
            n = C.c_uint64()
            ctx.check(L.lib.kmi_dbg_size_dist(g.h, comm.h, C.byref(n)))
            keys, cnt = g.to_vector()
            # find() over the communicator: this rank's queries (k-mers of its own block, both strands, and some that are no node)
            kmers = orc.dbg_parse(orc.kspec(k, ALPHA[alpha]), data, orc.FASTA)[0]
            q = np.ascontiguousarray(np.concatenate([kmers[rank::5][:200], orc.revcomp(orc.kspec(k, ALPHA[alpha]), kmers[rank::11][:50]),
                                                     np.random.default_rng(rank).integers(0, 1 << 40, (20, nw), dtype=np.uint64)]))
            r = L.Results()
            ctx.check(L.lib.kmi_dbg_find_dist_host(g.h, comm.h, q.ctypes.data_as(C.c_void_p), q.shape[0], C.byref(r)))
            fk = np.ctypeslib.as_array(r.keys, shape=(r.n * nw,)).copy().reshape(-1, nw) if r.n else np.zeros((0, nw), np.uint64)
            fv = np.ctypeslib.as_array(r.values, shape=(r.n * 5,)).copy().view(np.uint32).reshape(r.n, 10)[:, :9].copy() if r.n else np.zeros((0, 9), np.uint32)
            L.lib.kmi_results_free(C.byref(r))
            out.append((np.asarray(keys).reshape(-1, nw).copy(), np.asarray(cnt).copy(), n.value, q, fk, fv, rounds))
            g.close()
        ret[rank] = out
        comm.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


def _rows(keys, counts):
    keys, counts = np.asarray(keys, np.uint64), np.asarray(counts).astype(np.uint64)
    if keys.size == 0 and counts.size == 0:   # (no node at all: a file without a k-mer of this length)
        return np.zeros((0, 0), np.uint64)
    return orc.sorted_rows(keys, counts)


def _run(world, cases):
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), cases, ret), nprocs=world, join=True)
    return [[ret[r][i] for r in range(world)] for i in range(len(cases))]


def _check(case, per_rank, label):
    data, k, alpha, exists, _ = case
    s = orc.kspec(k, ALPHA[alpha])
    om = orc.DbgMap(s, exists_only=exists)
    om.insert(*orc.dbg_parse(s, data, orc.FASTA))
    got = _rows(np.concatenate([p[0] for p in per_rank]), np.concatenate([p[1] for p in per_rank]))
    exp = _rows(*om.export(canonical=True))
    assert got.shape == exp.shape, (label, got.shape, exp.shape)
    assert (got == exp).all(), label
    for r, p in enumerate(per_rank):
        assert p[2] == om.size(), (label, r)
        fk, fc = om.find(p[3], canonical=True)
        assert (_rows(p[4], p[5]) == _rows(fk, fc)).all(), (label, r)
    return [p[6] for p in per_rank]


def _pass_through():
    """a record whose middle is a long run of blank lines (CRLF and LF), a header that fills a whole block: with four ranks
    some blocks hold no sequence character and no record start, so a block's in-edge comes from two blocks back"""
    rng = np.random.default_rng(3)
    seq = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).tolist())
    return (b">r1\n" + seq(70) + b"\n" + b"\n" * 150 + b"\r\n" * 60 + seq(50) + b"\n>r2 " + b"h" * 260 + b"\n" + seq(45) + b"\n" + seq(45) + b"\n")


def _inputs():
    from tests.test_gpu_fasta import _synthetic_fasta
    out = [(name, open(os.path.join(GOLD, name), "rb").read()) for name in ("test.fasta", "test2.fasta", "natural.withN.fasta", "test.unitiqs.fasta")]
    out.append(("synthetic-lf-orphan", _synthetic_fasta(np.random.default_rng(11), 12, line=60, eol=b"\n", orphan=True, max_len=600)))
    out.append(("synthetic-crlf", _synthetic_fasta(np.random.default_rng(12), 12, line=60, eol=b"\r\n", orphan=False, max_len=600)))
    out.append(("pass-through", _pass_through()))
    return out


KA = {2: [(15, "DNA"), (31, "DNA5")], 3: [(21, "DNA"), (63, "DNA5")], 4: [(31, "DNA"), (21, "DNA5"), (63, "DNA")]}


@pytest.mark.parametrize("world", [2, 3, 4])
def test_union_over_ranks_is_the_whole_file(world):
    """the union of the ranks' node maps is the oracle's map of the whole file (k-mers with their eight edge counters and their
    occurrences), size() is the oracle's on every rank, find() over the communicator answers each rank's own queries; the
    look-ahead starts at 16 bytes, so ranks have to ask for more"""
    inputs = _inputs()
    cases = [(data, k, alpha, False, 16) for _, data in inputs for k, alpha in KA[world]]
    labels = ["%s k=%d %s" % (name, k, alpha) for name, _ in inputs for k, alpha in KA[world]]
    if world == 3:   # the edge-presence kind once over ranks
        cases.append((inputs[3][1], 31, "DNA", True, 16))
        labels.append("test.unitiqs.fasta exists")
    res = _run(world, cases)
    more = False
    for case, per_rank, label in zip(cases, res, labels):
        rounds = _check(case, per_rank, label)
        more = more or any(r > 1 for r in rounds)
    assert more   # some rank had to read further


def _pinned(before, after, seed):
    """pad both sides with a record each so that the two-way split falls exactly between `before` and `after`"""
    rng = np.random.default_rng(seed)
    seq = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).tolist())
    a = max(40, len(after) - len(before) + 40)
    b = a + len(before) - len(after)
    left = b">p\n" + seq(a) + b"\n" + before
    right = after + b">q\n" + seq(b) + b"\n"
    data = left + right
    assert len(data) // 2 == len(left)
    return data


def test_pinned_block_boundaries():
    """two ranks, the cut placed on purpose: between a record's first and second sequence character, between '\\r' and '\\n',
    inside a header, inside a blank line and at its start, and exactly k - 1, k and k + 1 sequence characters before a record ends.
    Each is its own assertion against the oracle: these fail when the left carry, its use in the extract pass, or the k-character
    look-ahead is wrong."""
    k = 21
    rng = np.random.default_rng(9)
    seq = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).tolist())
    s1, s2 = seq(60), seq(60)
    specs = {
        "first|second character": (b">r1\n" + s1[:1], s1[1:] + b"\n" + s2 + b"\n"),
        "\\r|\\n": (b">r1\r\n" + s1[:30] + b"\r", b"\n" + s1[30:] + b"\r\n" + s2 + b"\r\n"),
        "inside a header": (b">r1 some", b" description\n" + s1 + b"\n" + s2 + b"\n"),
        "inside a blank line": (b">r1\n" + s1 + b"\r\n\r", b"\n" + s2 + b"\n"),
        "start of a blank line": (b">r1\n" + s1 + b"\n", b"\n" + s2 + b"\n"),
        "k - 1 before the end": (b">r1\n" + s1 + b"\n" + s2[:20], s2[20:20 + k - 1] + b"\n>r2\n" + seq(40) + b"\n"),
        "k before the end": (b">r1\n" + s1 + b"\n" + s2[:20], s2[20:20 + k] + b"\n>r2\n" + seq(40) + b"\n"),
        "k + 1 before the end": (b">r1\n" + s1 + b"\n" + s2[:20], s2[20:20 + k + 1] + b"\n>r2\n" + seq(40) + b"\n"),
        "k before the end, across a line": (b">r1\n" + s1 + b"\n" + s2[:20], s2[20:30] + b"\n" + s2[30:30 + k - 10] + b"\n>r2\n" + seq(40) + b"\n"),
    }
    names = list(specs)
    cases = []
    for i, name in enumerate(names):
        data = _pinned(*specs[name], seed=100 + i)
        cases += [(data, k, "DNA", False, 16), (data, k, "DNA", False, 1 << 16)]
    res = _run(2, cases)
    for i, name in enumerate(names):
        for j in range(2):
            _check(cases[2 * i + j], res[2 * i + j], name + (" (16 B look-ahead)" if j == 0 else " (64 KB look-ahead)"))


def test_one_rank_communicator_matches_the_whole_file_build():
    """the new entry over a one-rank RCCL communicator (with and without KMI_FORCE_DIST) gives the nodes kmi_dbg_build_host
    gives on the same FASTA bytes; both are the oracle's"""
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    from tests.test_gpu_fasta import _synthetic_fasta
    for force in ("0", "1"):
        os.environ["KMI_FORCE_DIST"] = force
        try:
            ctx = K.Context(0, rank=0, nranks=1)
            comm = C.c_void_p()
            ctx.check(L.lib.kmi_comm_create(ctx.h, None, C.byref(comm)))
            try:
                for name, data, k, alpha in [("natural.withN.fasta", open(os.path.join(GOLD, "natural.withN.fasta"), "rb").read(), 31, "DNA"),
                                             ("synthetic", _synthetic_fasta(np.random.default_rng(4), 30, line=60, eol=b"\r\n", orphan=True, max_len=900), 21, "DNA5")]:
                    cfg = K.make_config(k, alpha, seq_format="fasta")
                    g1 = K.DeBruijnNodes(ctx, cfg)
                    g1.build(data)
                    g2 = K.DeBruijnNodes(ctx, cfg)
                    rounds = _build_range(L, ctx, g2, comm, data, 1, 0, 16)
                    assert rounds == 1
                    a, b = _rows(*g1.to_vector()), _rows(*g2.to_vector())
                    assert a.shape == b.shape and (a == b).all(), (name, force)
                    s = orc.kspec(k, ALPHA[alpha])
                    om = orc.DbgMap(s)
                    om.insert(*orc.dbg_parse(s, data, orc.FASTA))
                    assert (a == _rows(*om.export(canonical=True))).all(), (name, force)
                    g1.close()
                    g2.close()
                # a FASTQ graph is refused
                g3 = K.DeBruijnNodes(ctx, K.make_config(21))
                need = C.c_int(0)
                buf = np.frombuffer(b">r\nACGT\n", dtype=np.uint8).copy()
                st = L.lib.kmi_dbg_build_fasta_range_dist_host(g3.h, comm, buf.ctypes.data_as(C.c_void_p), buf.size, 0, buf.size, 1, -1, C.byref(need))
                assert st != 0
                g3.close()
            finally:
                L.lib.kmi_comm_destroy(comm)
                ctx.close()
        finally:
            os.environ.pop("KMI_FORCE_DIST", None)


def _example():
    exe = os.path.join(ROOT, "examples", "de_bruijn_graph_construction")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "de_bruijn_graph_construction"])
    return exe


@pytest.mark.parametrize("force_dist", [False, True])
def test_example_on_fasta(force_dist):
    """examples/de_bruijn_graph_construction.cpp on a FASTA file (FASTAParser by the extension): node counts and checksums of
    find(), the neighbours, the whole map and erase against the oracle; with KMI_FORCE_DIST=1 the build takes the byte-range
    entry over a one-rank communicator"""
    path = os.path.join(GOLD, "natural.withN.fasta")
    env = dict(os.environ, KMI_FORCE_DIST="1" if force_dist else "0")
    out = subprocess.run([_example(), path], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    k = 21
    s = orc.kspec(k)
    data = open(path, "rb").read()
    kmers, edges = orc.dbg_parse(s, data, orc.FASTA)
    qk = orc.extract(s, data, orc.FASTA)["kmers"]
    q = qk[: qk.shape[0] // 2] if qk.shape[0] > 50 else qk
    mask = np.uint64((1 << (2 * k)) - 1)
    for tag, exists in (("count", False), ("exist", True)):
        m = re.search(tag + r" nodes (\d+) size (\d+) found (\d+) keysum (\d+) edgesum (\d+) nbrsum (\d+) a_out_t_in (\d+)", out.stdout)
        assert m, out.stdout
        got = tuple(int(x) for x in m.groups())
        om = orc.DbgMap(s, exists_only=exists)
        om.insert(kmers, edges)
        fk, fc = om.find(q, canonical=True)
        w = np.arange(1, 9, dtype=np.uint64)
        nbr = 0
        for key, c in zip(fk[:, 0].tolist(), fc.tolist()):
            for i in range(4):
                if c[i]:
                    nbr += (((key << 2) | i) & int(mask)) % 1000003
                if c[4 + i]:
                    nbr += ((key >> 2) | (i << (2 * (k - 1)))) % 1000003
        ak, ac = om.export(canonical=True)
        assert got == (om.size(), om.size(), fk.shape[0], int(fk[:, 0].sum()), int((fc[:, :8].astype(np.uint64) * w).sum()), nbr,
                       int(ac[:, 0].astype(np.uint64).sum() + ac[:, 7].astype(np.uint64).sum())), tag
        m = re.search(tag + r" erased (\d+) left (\d+) keysum (\d+)", out.stdout)
        assert m, out.stdout
        gone = {tuple(r) for r in orc.canonical(s, q[::3]).tolist()} & {tuple(r) for r in ak.tolist()}
        stay = [r for r in ak.tolist() if tuple(r) not in gone]
        assert tuple(int(x) for x in m.groups()) == (len(gone), len(stay), sum(int(r[0]) % 1000003 for r in stay))


@pytest.mark.parametrize("name,fmt", [("natural.withN.fasta", orc.FASTA), ("test.debruijn.small.fastq", orc.FASTQ)])
def test_example_over_two_ranks_on_the_socket_transport(name, fmt):
    """two processes of the example, one graph over both: kmerind::comm.transport is the example's AF_UNIX messenger, so the engine
    runs the library's multi-rank code without RCCL. The ranks' local sizes add up to the oracle's size, both ranks report that
    size, and the ranks' checksums add up to the whole map's"""
    exe = _example()
    path = os.path.join(GOLD, name)
    env = dict(os.environ)
    env.pop("KMI_FORCE_DIST", None)
    with tempfile.TemporaryDirectory() as d:
        procs = [subprocess.Popen([exe, path, str(r), "2", d], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for r in range(2)]
        outs = []
        for p in procs:
            try:
                o, e = p.communicate(timeout=300)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
            outs.append((p.returncode, o, e))
    for rc, o, e in outs:
        assert rc == 0, e
    k = 21
    s = orc.kspec(k)
    data = open(path, "rb").read()
    kmers, edges = orc.dbg_parse(s, data, fmt)
    w = np.arange(1, 9, dtype=np.uint64)
    for tag, exists in (("count", False), ("exist", True)):
        om = orc.DbgMap(s, exists_only=exists)
        om.insert(kmers, edges)
        ak, ac = om.export(canonical=True)
        local, keysum, edgesum = 0, 0, 0
        for r, (_, o, _) in enumerate(outs):
            m = re.search(tag + r" rank (\d+) local_size (\d+) size (\d+) keysum (\d+) edgesum (\d+)", o)
            assert m, o
            rr, ls, sz, ks, es = (int(x) for x in m.groups())
            assert rr == r and sz == om.size(), (tag, r)
            local += ls; keysum += ks; edgesum += es
        assert local == om.size(), tag
        assert keysum == sum(int(x) % 1000003 for x in ak[:, 0].tolist()), tag
        assert edgesum == int((ac[:, :8].astype(np.uint64) * w).sum()), tag
