"""Which way a build from FASTQ takes through the super-k-mer driver (kmi_sk_build.h), pinned from outside: for every arm of the
fall-back chain -- the one-pass front end, the general front end asked for (KMI_FRONT=general), the general front end behind a
one-pass front end that declined a well-formed input, and the k-mer pipeline (KMI_FUSED_PATH=kmer) -- the index must be the
oracle's CountMap, key for key and count for count, and the context's profile must show the kernels of that arm and none of another.
The same for the de Bruijn node build (edge records from the one-pass front end; the tuple path when a read holds an N, which
the edge records cannot carry, and the general front end must NOT be tried in between; the tuple path asked for), and for a
build over two ranks through the transport back end in which one chunk of one rank's share is an input the one-pass front end declines.

Inputs: about 200 reads of 100 .. 150 bases drawn from a 3000-base genome (so counts above one), among them one read of k - 1
bases and one of exactly k; the same file without its final newline; a file of under 64 bytes (the one-pass front end does not
look at it; for k >= 29 it holds no k-mer at all). The declining input is that file followed by 300 records of two bases: more
than eight line starts in 64 bytes is "crowded lines" to the one-pass front end (kmi_front.h, reason 4), and well-formed FASTQ.

k = 17, 21, 23, 31, 32: the four window widths, and sk_reduce's instantiation for 32-mers (a key can equal the empty marker).

Not reached here: the general front end exceeding its item capacity on a real input (sk_minimizer_kernel raising FLAG_SK_DECLINED),
behind which the k-mer pipeline runs. Under KMI_FRONT=general, k = 17 and 31, 300 reads of 150 bases that are one base, AC, ACGT,
TGCA, TTGGCCAA repeated or descending runs (TTTGA TTGCA TGCCA ...), and 40 reads of 5000 bases of A and of AC, all stayed within
the capacities; tests/test_gpu_dist_clayer.py reaches the hand-over behind that arm through KMI_SK_DBG=7.
The low-complexity inputs of the node build's edge records (one base, tandem repeats, the last reads of the buffer) are in
tests/test_gpu_debruijn_records.py."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import oracle as orc

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


KS = [17, 21, 23, 31, 32]
ARMS = {"one-pass": {}, "general": {"KMI_FRONT": "general"}, "declined": {}, "kmer": {"KMI_FUSED_PATH": "kmer"}}


def _ctx_with(env):
    """a context made under these environment settings (they are read when the context is made)"""
    import kmerind_amd as K
    old = {n: os.environ.get(n) for n in env}
    os.environ.update(env)
    try:
        return K.Context(0)
    finally:
        for n, v in old.items():
            if v is None:
                del os.environ[n]
            else:
                os.environ[n] = v


@pytest.fixture(scope="module")
def contexts():
    made = {}
    def get(name, env):
        if name not in made:
            made[name] = _ctx_with(env)
        return made[name]
    yield get
    for c in made.values():
        c.close()


def _fastq(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(reads))


def _reads(k, seed, n=200):
    rng = np.random.default_rng(seed)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=3000)].tobytes()
    reads = []
    for i in range(n):
        ln = int(rng.integers(100, 151))
        at = int(rng.integers(0, len(genome) - ln))
        reads.append(genome[at:at + ln])
    reads[n // 3] = genome[5:5 + k - 1]          # one read shorter than k
    reads[2 * n // 3] = genome[40:40 + k]        # one of exactly k
    return reads


CROWDED = b"@a\nAC\n+\nII\n" * 300                # lines of a few bytes: well-formed, and not the one-pass front end's input


@pytest.fixture(scope="module")
def inputs():
    """per k: the inputs and the oracle's k-mers of each, made once"""
    out = {}
    for k in KS:
        main = _fastq(_reads(k, 9000 + k))
        tiny = b"@r\n" + main.split(b"\n")[1][:25] + b"\n+\n" + b"I" * 25 + b"\n"
        assert len(tiny) < 64
        d = {"main": main, "no-final-newline": main[:-1], "tiny": tiny, "declining": main + CROWDED}
        s = orc.kspec(k, orc.DNA)
        out[k] = {name: (data, orc.extract(s, data, orc.FASTQ)["kmers"]) for name, data in d.items()}
    return out


def _profiled(ctx, fn):
    """the names of the kernels fn() launched, in the order of their first launch"""
    ctx.profile(True)
    ctx.profile_reset()
    fn()
    names = [p["name"] for p in ctx.profile_get() if p["launches"]]
    ctx.profile(False)
    return names


def _assert_is_oracle_map(idx, k, kmers, what):
    s = orc.kspec(k, orc.DNA)
    om = orc.CountMap(s, orc.CANONICAL)
    om.insert(kmers)
    a, b = orc.sorted_pairs(*idx.to_vector()), orc.sorted_pairs(*om.export())
    assert a[0].shape == b[0].shape, what
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), what


def _assert_arm(arm, names, what):
    if arm == "one-pass":
        assert "sk_front" in names and "sk_reduce" in names, (what, names)
        assert not {"fastq_list", "sk_minimizer", "fastq_scan_tiles"} & set(names), (what, names)
    elif arm == "general":
        assert "sk_front" not in names, (what, names)
        assert {"fastq_list", "sk_minimizer", "sk_reduce"} <= set(names), (what, names)
    elif arm == "declined":
        assert {"sk_front", "fastq_list", "sk_minimizer", "sk_reduce"} <= set(names), (what, names)
        assert names.index("sk_front") < names.index("fastq_list") < names.index("sk_minimizer"), (what, names)
    else:
        assert not {"sk_front", "sk_reduce", "sk_minimizer"} & set(names), (what, names)
        assert "fastq_list" in names, (what, names)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("arm", list(ARMS))
def test_count_index_arm(contexts, inputs, arm, k):
    import kmerind_amd as K
    ctx = contexts("kmer" if arm == "kmer" else ("general" if arm == "general" else "default"), ARMS[arm])
    for name in (["declining"] if arm == "declined" else ["main", "no-final-newline", "tiny"]):
        data, kmers = inputs[k][name]
        idx = K.CountIndex(ctx, K.make_config(k, "DNA", strand="canonical"))
        names = _profiled(ctx, lambda: idx.build(data))
        what = "%s k=%d %s" % (arm, k, name)
        print(what, names)
        _assert_is_oracle_map(idx, k, kmers, what)
        idx.close()
        if name in ("main", "declining"):
            _assert_arm(arm, names, what)
        elif name == "tiny" and arm != "kmer":
            assert "sk_front" not in names, (what, names)      # under 64 bytes: not looked at by the one-pass front end


# ------------------------------------------------------------------------------------------------------ the de Bruijn node build
def _with_one_n(data):
    lines = data.split(b"\n")
    b = bytearray(lines[1 + 4 * 7])
    b[len(b) // 2] = ord("N")
    lines[1 + 4 * 7] = bytes(b)
    return b"\n".join(lines)


@pytest.mark.parametrize("k", [21, 31])
@pytest.mark.parametrize("arm", ["edges", "declined-by-N", "tuples"])
def test_de_bruijn_node_build_arm(contexts, inputs, arm, k):
    import kmerind_amd as K
    ctx = contexts("dbg-tuples", {"KMI_DBG_SUPERKMER": "0"}) if arm == "tuples" else contexts("default", {})
    data = inputs[k]["main"][0]
    if arm == "declined-by-N":
        data = _with_one_n(data)
    s = orc.kspec(k)
    om = orc.DbgMap(s)
    om.insert(*orc.dbg_parse(s, data))
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    names = _profiled(ctx, lambda: g.build(data))
    what = "dbg %s k=%d" % (arm, k)
    print(what, names)
    assert g.local_size() == om.size(), what
    nodes = lambda keys, counts: orc.sorted_rows(keys, counts.astype(np.uint64))
    assert (nodes(*g.to_vector()) == nodes(*om.export(canonical=True))).all(), what
    g.close()
    if arm == "edges":
        assert {"sk_front", "sk_reduce", "sk_edges_accumulate"} <= set(names) and "dbg_accumulate" not in names, (what, names)
    elif arm == "declined-by-N":
        assert "sk_front" in names and "dbg_accumulate" in names, (what, names)
        assert not {"sk_minimizer", "sk_reduce", "sk_edges_accumulate"} & set(names), (what, names)   # no general front end in between
    else:
        assert "dbg_accumulate" in names and not {"sk_front", "sk_reduce", "sk_edges_accumulate"} & set(names), (what, names)


# ------------------------------------------------------------------------------------------- two ranks over the transport back end
def _rank_worker(rank, world, port, shares, k, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), KMI_DIST_CHUNKS="2")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        idx = K.CountIndex(ctx, K.make_config(k, "DNA", strand="canonical"))
        buf = np.frombuffer(shares[rank], dtype=np.uint8).copy()
        d = ctx.alloc(buf.size + 64)
        ctx.to_device(d, buf)
        ctx.profile(True)
        ctx.profile_reset()
        ctx.check(L.lib.kmi_index_build_dist_dev(idx.h, comm.h, C.c_void_p(d), buf.size, sum(len(s) for s in shares[:rank])))
        launches = {p["name"]: p["launches"] for p in ctx.profile_get() if p["launches"]}
        keys, cnts = idx.to_vector()
        ret[rank] = dict(keys=keys.copy(), cnts=cnts.copy(), launches=launches)
        idx.close()
        comm.close()
        ctx.free(d)
        ctx.close()
    finally:
        dist.destroy_process_group()


def test_two_ranks_one_chunk_declined(inputs):
    """rank 0: two chunks the one-pass front end takes. Rank 1: its second chunk holds the records of two bases, so the one-pass
    front end declines that chunk and the general front end makes its records; both chunks still travel as records."""
    k = 31
    main = inputs[k]["main"][0]
    shares = [main, main + CROWDED]
    ret = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(2, _free_port(), shares, k, ret), nprocs=2, join=True)
    s = orc.kspec(k)
    om = orc.CountMap(s, orc.CANONICAL)
    om.insert(orc.extract(s, shares[0] + shares[1], orc.FASTQ)["kmers"])
    keys = np.concatenate([ret[r]["keys"] for r in range(2)])
    a, b = orc.sorted_pairs(keys, np.concatenate([ret[r]["cnts"] for r in range(2)])), orc.sorted_pairs(*om.export())
    assert a[0].shape == b[0].shape and (a[0] == b[0]).all() and (a[1] == b[1]).all()
    assert np.unique(keys, axis=0).shape[0] == keys.shape[0]
    l0, l1 = ret[0]["launches"], ret[1]["launches"]
    print(l0, l1)
    assert l0.get("sk_front") == 2 and "sk_minimizer" not in l0 and "sk_reduce" in l0, l0
    assert l1.get("sk_front") == 2 and l1.get("fastq_list") == 1 and l1.get("sk_minimizer") == 1 and "sk_reduce" in l1, l1
