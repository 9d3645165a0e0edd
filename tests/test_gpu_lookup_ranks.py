"""kmi_index_lookup_dist_*: counts in the caller's order from a count index held over ranks. Two to four processes share the GPU
over kmerind_amd.transport.GroupComm (as in test_gpu_setops_ranks.py); every rank asks its own mix of present keys, absent keys,
reverse complements of present keys and one key 300 times, one rank asks nothing in one case, and every rank's counts must be
those of tests/index_model.py's CountModel built over the WHOLE input. The bytes a rank puts on the wire are bounded by its key
words and four bytes per key it answered: where a query sits in the caller's array stays at home."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import index_model as M
from tests import oracle as orc
from tests import read_profile_model as RP

pytestmark = pytest.mark.gpu

STRAND = {"single": orc.SINGLE, "canonical": orc.CANONICAL}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, k, strand, fill, data, queries, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        from kmerind_amd import fileio
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        idx = K.CountIndex(ctx, K.make_config(k, "DNA", strand=strand))
        b, e = fileio.partition_fastq(data, world)[rank]
        buf = np.frombuffer(data[b:e], dtype=np.uint8).copy()
        if fill == "build":      # kmi_index_build_dist_dev: the minimizer-owner rule where a build through super-k-mers applies
            d = ctx.alloc(max(buf.size, 16) + 64)
            if buf.size:
                ctx.to_device(d, buf)
            ctx.check(L.lib.kmi_index_build_dist_dev(idx.h, comm.h, C.c_void_p(d), buf.size, b))
            ctx.free(d)
        else:                    # kmi_index_insert_dist_host: KeyToRank
            km = np.ascontiguousarray(orc.extract(orc.kspec(k), bytes(buf), orc.FASTQ)["kmers"])
            ctx.check(L.lib.kmi_index_insert_dist_host(idx.h, comm.h, km.ctypes.data_as(C.c_void_p), km.shape[0]))
        q = np.ascontiguousarray(queries[rank])
        nq = q.shape[0]
        before = comm.calls["bytes"]
        counts = idx.lookup(q, comm=comm)
        sent = comm.calls["bytes"] - before
        answered = ctx.debug_counter(12)
        # the device form into a buffer of exactly nq words with a guard behind it
        guard = np.full(nq + 64, 0xDEADBEEF, dtype=np.uint32)
        dq, dc = ctx.alloc(max(q.nbytes, 8)), ctx.alloc(guard.nbytes)
        if nq:
            ctx.to_device(dq, q)
        ctx.to_device(dc, guard)
        idx.lookup_device(dq, nq, dc, comm=comm)
        ctx.to_host(guard, dc)
        ctx.free(dq)
        ctx.free(dc)
        ret[rank] = dict(owner=idx.owner_ranks(), local=idx.local_size(), counts=counts, dev=guard[:nq].copy(),
                         intact=bool((guard[nq:] == 0xDEADBEEF).all()), sent=sent, answered=answered)
        idx.close()
        comm.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


def _queries(rng, model, s, rank, empty):
    """rank r's mix, different for every rank: present keys, absent keys, reverse complements of present keys, one key 300 times"""
    if empty:
        return np.zeros((0, s.n_words), dtype=np.uint64)
    stored = model.export()[0]
    present = stored[rng.integers(0, stored.shape[0], 700 + 150 * rank)]
    absent = orc.kmers_from_string(s, M.random_seq(rng, 200 + 50 * rank + s.k - 1))
    rc = orc.revcomp(s, stored[rng.integers(0, stored.shape[0], 150)])
    block = np.repeat(stored[rng.integers(0, stored.shape[0], 1)], 300, axis=0)
    q = np.concatenate([present, absent, rc])
    q = q[rng.permutation(q.shape[0])]
    at = int(rng.integers(0, q.shape[0]))
    return np.ascontiguousarray(np.concatenate([q[:at], block, q[at:]]))


# (k, strand, how the index is filled, ranks, the rank that asks nothing or None, owner ranks expected)
# The minimizer-owner rule takes a power of two of ranks (kmi_index_build_dist_dev falls back to KeyToRank otherwise), so it is
# asserted for worlds 2 and 4; world 3 runs the same build under KeyToRank.
CASES = [
    pytest.param(31, "canonical", "build", 2, None, 2, id="a-k31-owner-2"),
    pytest.param(31, "canonical", "build", 3, 1, 1, id="a-k31-build-3"),
    pytest.param(31, "canonical", "build", 4, None, 4, id="a-k31-owner-4"),
    pytest.param(21, "single", "insert", 2, None, 1, id="b-k21-single-keytorank-2"),
    pytest.param(40, "canonical", "build", 3, None, 1, id="c-k40-two-words-3"),
]


@pytest.mark.parametrize("k,strand,fill,world,empty_rank,owners", CASES)
def test_lookup_over_ranks_matches_the_model(k, strand, fill, world, empty_rank, owners):
    rng = np.random.default_rng(1000 + k + world)
    genome = M.random_seq(rng, 20_000)
    data = M.fastq(M.background(rng, 400, read_len=100, genome=genome))
    s = orc.kspec(k)
    model = M.CountModel(k, orc.DNA, STRAND[strand])
    model.insert(orc.extract(s, data, orc.FASTQ)["kmers"])
    queries = [_queries(rng, model, s, r, r == empty_rank) for r in range(world)]
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), k, strand, fill, data, queries, ret), nprocs=world, join=True)
    R = [ret[r] for r in range(world)]
    assert sum(x["local"] for x in R) == model.size()
    kb = 8 * s.n_words
    for r, x in enumerate(R):
        assert x["owner"] == owners
        want = RP.lookup(model, queries[r])
        if queries[r].shape[0]:
            assert 0 < np.count_nonzero(want) < want.shape[0]
        assert x["counts"].shape == want.shape and (x["counts"] == want).all(), "rank %d, host form" % r
        assert x["intact"] and (x["dev"] == want).all(), "rank %d, device form" % r
        # the key words out, four bytes per answered key back, and the count words of the exchanges: no index word travels
        assert x["sent"] <= queries[r].shape[0] * kb + x["answered"] * 4 + 64 * world, (r, x["sent"], x["answered"])
    assert sum(x["answered"] for x in R) == sum(q.shape[0] for q in queries)
