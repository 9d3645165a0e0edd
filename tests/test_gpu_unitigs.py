"""Unitigs of a de Bruijn node map on the GPU (kmi_dbg_compact / DeBruijnNodes.unitigs) against the plain-Python model
(tests/unitig_model.py), whose input is always the oracle's node map, never the GPU's. Also: exact answers where the unitigs are
known without the model (a random genome, a circle), the refusals, and the C++ example."""
import ctypes as C
import os
import re
import socket
import subprocess
import tempfile

import numpy as np
import pytest

from tests import oracle as orc
from tests import unitig_model as M

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "data")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import kmerind_amd as K
    c = K.Context(0)
    yield c
    c.close()


def _gpu(g, t=1):
    from kmerind_amd.core import split_unitigs
    off, bases, occ, circ = g.unitigs(t)
    assert off.shape[0] == occ.shape[0] + 1 and int(off[-1]) == bases.shape[0]
    return sorted((s.decode(), int(o), bool(c)) for s, o, c in zip(split_unitigs(off, bases), occ, circ))


def _oracle_map(data, k, fmt=orc.FASTQ, exists=False):
    s = orc.kspec(k)
    om = orc.DbgMap(s, exists_only=exists)
    om.insert(*orc.dbg_parse(s, data, fmt))
    return om.export(canonical=True)


def _model(data, k, t=1, fmt=orc.FASTQ, exists=False):
    return M.unitigs(*_oracle_map(data, k, fmt, exists), k, t)


def _fastq(reads):
    return "".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads)).encode()


def _fasta(records, width=80):
    out = []
    for i, r in enumerate(records):
        out.append(">s%d\n" % i)
        out += [r[j:j + width] + "\n" for j in range(0, len(r), width)]
    return "".join(out).encode()


def _genome(rng, n):
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, n)])


def _synthetic_reads(seed, k, n_reads=1500):
    """reads of a genome with repeats (copies longer than k), SNP variants, poly-A stretches, both strands"""
    rng = np.random.default_rng(seed)
    g = _genome(rng, 6000)
    rep = g[1000:1000 + 3 * k]
    g = g[:2500] + rep + g[2500:4000] + rep + g[4000:] + "A" * (2 * k) + _genome(rng, 400)
    snp = list(g)
    for p in rng.integers(0, len(g), 12):
        snp[p] = "ACGT"[(("ACGT".index(snp[p])) + 1) % 4]
    snp = "".join(snp)
    reads = []
    for i in range(n_reads):
        src = snp if i % 5 == 0 else g
        p = int(rng.integers(0, len(src) - 100))
        r = src[p:p + int(rng.integers(max(k, 60), 150))]
        reads.append(M.revcomp(r) if rng.random() < 0.5 else r)
    return _fastq(reads)


@pytest.mark.parametrize("name,k", [("test.debruijn.tiny.fastq", 21), ("test.debruijn.tiny.fastq", 31), ("test.debruijn.small.fastq", 21),
                                    ("test.debruijn.small.fastq", 31), ("natural.withN.fastq", 21)])
def test_golden_fastq_against_the_model(ctx, name, k):
    import kmerind_amd as K
    data = open(os.path.join(GOLD, name), "rb").read()
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    g.build(data)
    for t in (1, 2):
        assert _gpu(g, t) == _model(data, k, t), t
    g.close()


@pytest.mark.parametrize("k", [15, 21, 31, 32, 33, 63, 96])
def test_synthetic_reads_against_the_model(ctx, k):
    import kmerind_amd as K
    data = _synthetic_reads(k, k)
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    g.build(data)
    exp = _model(data, k)
    got = _gpu(g)
    assert len(got) == len(exp) and got == exp
    assert len(exp) > 10 and any(len(s) > 200 for s, _, _ in exp)   # (branches and long unitigs both)
    g.close()


def test_fasta_graph_against_the_model(ctx):
    import kmerind_amd as K
    data = open(os.path.join(GOLD, "natural.fasta"), "rb").read()
    g = K.DeBruijnNodes(ctx, K.make_config(21, seq_format="fasta"))
    g.build(data)
    assert _gpu(g) == _model(data, 21, fmt=orc.FASTA)
    g.close()


def test_edge_exists_map(ctx):
    import kmerind_amd as K
    data = open(os.path.join(GOLD, "test.debruijn.small.fastq"), "rb").read()
    g = K.DeBruijnNodes(ctx, K.make_config(31), exists_only=True)
    g.build(data)
    got = _gpu(g)
    assert got == _model(data, 31, exists=True)
    assert all(o == 0 for _, o, _ in got)
    # t = 2 on 0 / 1 counters: no edge counts, every node is a unitig of its own
    assert len(_gpu(g, 2)) == g.local_size()
    g.close()


def test_after_erase(ctx):
    import kmerind_amd as K
    k = 31
    data = _synthetic_reads(5, k, 600)
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    g.build(data)
    keys, cnt = _oracle_map(data, k)
    victims = keys[::7]
    assert g.erase(victims) == victims.shape[0]
    keep = np.ones(keys.shape[0], bool)
    keep[::7] = False
    assert _gpu(g) == M.unitigs(keys[keep], cnt[keep], k)
    g.close()


def test_empty_and_one_node_maps(ctx):
    import kmerind_amd as K
    g = K.DeBruijnNodes(ctx, K.make_config(21))
    off, bases, occ, circ = g.unitigs()
    assert off.tolist() == [0] and bases.size == 0 and occ.size == 0 and circ.size == 0
    read = "ACCGATTGCAGGTTACGGATC"
    g.build(_fastq([read]))
    assert _gpu(g) == [(min(read, M.revcomp(read)), 1, False)]
    g.close()


def test_compact_twice_and_after_insert(ctx):
    import kmerind_amd as K
    k = 21
    a = _synthetic_reads(7, k, 400)
    b = _synthetic_reads(8, k, 400)
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    g.build(a)
    first = _gpu(g)
    assert first == _model(a, k)
    assert _gpu(g) == first
    g.insert(*orc.dbg_parse(orc.kspec(k), b))
    exp = _model(a + b, k)
    assert exp != first and _gpu(g) == exp
    g.close()


def test_random_genome_is_one_unitig(ctx):
    """2 Mbp random single-record FASTA, k = 31: one path of 2e6 - 30 nodes, about 21 rounds of pointer jumping"""
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    genome = _genome(np.random.default_rng(2024), 2_000_000)
    g = K.DeBruijnNodes(ctx, K.make_config(31, seq_format="fasta"))
    g.build(_fasta([genome]))
    assert g.local_size() == len(genome) - 30
    L.lib.kmi_profile_enable(ctx.h, 1)
    L.lib.kmi_profile_reset(ctx.h)
    got = _gpu(g)
    recs = (L.KernelTime * 64)()
    n = C.c_size_t()
    ctx.check(L.lib.kmi_profile_get(ctx.h, recs, 64, C.byref(n)))
    L.lib.kmi_profile_enable(ctx.h, 0)
    rounds = sum(r.launches for r in recs[:n.value] if r.name == b"unitig_jump")
    assert got == [(min(genome, M.revcomp(genome)), len(genome) - 30, False)]
    assert 20 <= rounds <= 23, rounds
    g.close()


def test_circle_is_one_circular_unitig(ctx):
    import kmerind_amd as K
    k = 31
    rng = np.random.default_rng(9)
    circle = _genome(rng, 50_000)
    ring = circle + circle[:200]
    reads = []
    for p in range(0, len(circle), 50):
        r = ring[p:p + 150]
        reads.append(M.revcomp(r) if (p // 50) % 2 else r)
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    g.build(_fastq(reads))
    ext = circle + circle[:k - 1]
    m = min(M.canonical(ext[i:i + k]) for i in range(len(circle)))
    start = circle if m in ext else M.revcomp(circle)   # spelled from m in its stored orientation
    i = (start + start[:k - 1]).find(m)
    seq = (start + start)[i:i + len(circle) + k - 1]
    got = _gpu(g)
    assert len(got) == 1 and got[0][0] == seq and got[0][2] is True
    assert got == _model(_fastq(reads), k)
    g.close()


def test_a_million_nodes_against_the_model(ctx):
    import kmerind_amd as K
    data = K.synth_fastq(seed=5, genome_len=1_000_000, n_reads=60_000)
    k = 31
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    g.build(data)
    assert g.local_size() > 900_000
    assert _gpu(g) == _model(data.tobytes(), k)
    g.close()


def test_refusals(ctx):
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    nu, nb = C.c_uint64(), C.c_uint64()
    data = open(os.path.join(GOLD, "test.debruijn.tiny.fastq"), "rb").read()
    # DNA5: not a 2-bit alphabet
    g5 = K.DeBruijnNodes(ctx, K.make_config(21, "DNA5"))
    g5.build(data)
    assert L.lib.kmi_dbg_compact(g5.h, 1, C.byref(nu), C.byref(nb)) == L.ERR_INVALID
    g5.close()
    g = K.DeBruijnNodes(ctx, K.make_config(21))
    g.build(data)
    # export before any compaction; t = 0
    assert L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0) == L.ERR_INVALID
    assert L.lib.kmi_dbg_compact(g.h, 0, C.byref(nu), C.byref(nb)) == L.ERR_INVALID
    assert L.lib.kmi_dbg_compact(g.h, 1, C.byref(nu), C.byref(nb)) == L.OK and nu.value > 0
    assert L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0) == L.OK
    off = np.zeros(nu.value + 1, np.uint64)
    assert L.lib.kmi_dbg_unitigs_export_host(g.h, off.ctypes.data_as(C.c_void_p), None, None, None, nu.value - 1, 0) == L.ERR_OVERFLOW
    # a change drops the result
    g.erase(orc.dbg_parse(orc.kspec(21), data)[0][:3])
    assert L.lib.kmi_dbg_unitigs_export_host(g.h, None, None, None, None, 0, 0) == L.ERR_INVALID
    g.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_rank_worker(rank, world, port, data, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        g = K.DeBruijnNodes(ctx, K.make_config(21))
        half = data[rank]
        buf = np.frombuffer(half, dtype=np.uint8).copy()
        ctx.check(L.lib.kmi_dbg_build_dist_host(g.h, comm.h, buf.ctypes.data_as(C.c_void_p), buf.size))
        nu, nb = C.c_uint64(), C.c_uint64()
        st = L.lib.kmi_dbg_compact(g.h, 1, C.byref(nu), C.byref(nb))
        g.clear()   # a cleared map is whole again (empty)
        st2 = L.lib.kmi_dbg_compact(g.h, 1, C.byref(nu), C.byref(nb))
        ret[rank] = (st, st2, nu.value)
        g.close()
        comm.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


def test_share_of_a_build_over_two_ranks_is_refused():
    import torch.multiprocessing as mp
    from kmerind_amd import _lib as L
    lines = _synthetic_reads(3, 21, 200).rstrip(b"\n").split(b"\n")
    cut = len(lines) // 8 * 4   # (four-line records)
    parts = [b"\n".join(lines[:cut]) + b"\n", b"\n".join(lines[cut:]) + b"\n"]
    ret = mp.Manager().dict()
    mp.spawn(_two_rank_worker, args=(2, _free_port(), parts, ret), nprocs=2, join=True)
    for r in range(2):
        assert ret[r] == (L.ERR_INVALID, L.OK, 0), (r, ret[r])


def _example():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "de_bruijn_unitigs"], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "examples", "de_bruijn_unitigs")


def _read_fasta(path):
    recs = []
    for block in open(path).read().split(">")[1:]:
        head, seq = block.split("\n", 1)
        m = re.fullmatch(r"u(\d+) len=(\d+) occ=(\d+) circular=([01])", head)
        assert m, head
        seq = seq.replace("\n", "")
        assert int(m.group(1)) == len(recs) and int(m.group(2)) == len(seq)
        recs.append((seq, int(m.group(3)), m.group(4) == "1"))
    return recs


@pytest.mark.parametrize("name,fmt,t", [("test.debruijn.small.fastq", orc.FASTQ, 1), ("test.debruijn.small.fastq", orc.FASTQ, 2),
                                        ("natural.fasta", orc.FASTA, 1)])
def test_example_writes_the_unitigs(name, fmt, t):
    exe = _example()
    path = os.path.join(GOLD, name)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "u.fasta")
        p = subprocess.run([exe, path, out] + ([str(t)] if t != 1 else []), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        got = _read_fasta(out)
    exp = _model(open(path, "rb").read(), 31, t, fmt=fmt)
    assert sorted(got) == exp
    n_nodes = sum(len(s) - 30 for s, _, _ in exp)
    assert p.stdout.strip() == "unitigs %d bases %d nodes %d" % (len(exp), sum(len(s) for s, _, _ in exp), n_nodes)
