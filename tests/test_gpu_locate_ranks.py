"""kmi_index_locate_dist_*: occ, offsets and values in the caller's order from a position / position + quality index held over
ranks, against tests/locate_model.py's LocateModel built over the WHOLE input. Two or three processes share the GPU over
kmerind_amd.transport.GroupComm. The input carries 30 reads of one base -- one key with a few thousand occurrences, more than a
tile of the copy that brings the returned values into query order, so its segment crosses tile boundaries -- and a 12-base repeat;
one rank asks the heavy key 50 times. max_occ is 1, 4 and KMI_LOCATE_ALL; a sizing call precedes every filling call; rank 1's
capacity is one hit short once (its peers must not notice); one case shrinks the owners' tables so that they take several passes."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import index_model as M
from tests import locate_model as LM
from tests import multimap_cases as MC
from tests import oracle as orc

pytestmark = pytest.mark.gpu

STRAND = {"single": orc.SINGLE, "canonical": orc.CANONICAL}
CAPS = (1, 4, LM.LOCATE_ALL)
GUARD = 64
PATTERN = 0xA5A5A5A5DEADBEEF
PATTERN32 = 0xDEADBEEF


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, k, strand, kind, env, data, hot, queries, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.update(env)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        from kmerind_amd import fileio
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        idx = K.PositionIndex(ctx, K.make_config(k, "DNA", strand=strand, index_kind=kind))
        vw = idx.value_words
        b, e = fileio.partition_fastq(data, world)[rank]
        buf = np.frombuffer(data[b:e], dtype=np.uint8).copy()
        ctx.check(L.lib.kmi_index_build_dist_host(idx.h, comm.h, buf.ctypes.data_as(C.c_void_p), buf.size, b))
        if hot is not None:   # rank 0 brings every hot tuple, the others none: KeyToRank spreads them
            hk, hv = hot if rank == 0 else (hot[0][:0], hot[1][:0])
            hk, hv = np.ascontiguousarray(hk), np.ascontiguousarray(hv)
            ctx.check(L.lib.kmi_index_insert_tuples_dist_host(idx.h, comm.h, hk.ctypes.data_as(C.c_void_p), hv.ctypes.data_as(C.c_void_p),
                                                              hk.shape[0]))
        q = np.ascontiguousarray(queries[rank])
        nq = q.shape[0]
        out = dict(local=idx.local_size(), tile=ctx.debug_counter(11), host={}, npass=0)
        for cap in CAPS:
            out["host"][cap] = idx.locate(q, cap, comm=comm)   # the sizing call, then the filling call
            out["npass"] = max(out["npass"], ctx.debug_counter(8))
        # the device form with KMI_LOCATE_ALL: sizing, then a value buffer of exactly n_hits rows -- one row short on rank 1
        h_occ = np.full(nq + GUARD, PATTERN32, dtype=np.uint32)
        h_off = np.full(nq + 1 + GUARD, PATTERN, dtype=np.uint64)
        dq, d_occ, d_off = ctx.alloc(max(q.nbytes, 8)), ctx.alloc(h_occ.nbytes), ctx.alloc(h_off.nbytes)
        if nq:
            ctx.to_device(dq, q)
        ctx.to_device(d_occ, h_occ)
        ctx.to_device(d_off, h_off)
        n = idx.locate_device(dq, nq, d_occ, d_off, comm=comm)
        capacity = n - 1 if rank == 1 else n
        h_val = np.full(capacity * vw + GUARD, PATTERN, dtype=np.uint64)
        d_val = ctx.alloc(h_val.nbytes)
        ctx.to_device(d_val, h_val)
        hits = C.c_uint64(12345)
        st = L.lib.kmi_index_locate_dist_dev(idx.h, comm.h, C.c_void_p(dq), nq, L.LOCATE_ALL, C.c_void_p(d_occ), C.c_void_p(d_off),
                                             C.c_void_p(d_val), capacity, C.byref(hits))
        ctx.to_host(h_occ, d_occ)
        ctx.to_host(h_off, d_off)
        ctx.to_host(h_val, d_val)
        for p in (dq, d_occ, d_off, d_val):
            ctx.free(p)
        out["dev"] = dict(st=st, sized=n, hits=hits.value, occ=h_occ[:nq].copy(), off=h_off[:nq + 1].copy(),
                          val=h_val[:capacity * vw].reshape(capacity, vw).copy(),
                          intact=bool((h_occ[nq:] == PATTERN32).all() and (h_off[nq + 1:] == np.uint64(PATTERN)).all() and
                                      (h_val[capacity * vw:] == np.uint64(PATTERN)).all()))
        ret[rank] = out
        idx.close()
        comm.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


def _input(rng, k):
    unit = M.random_seq(rng, 12)
    seqs = M.background(rng, 400, read_len=100, genome=M.random_seq(rng, 20_000)) + M.poly_reads(b"A", 30) + [(unit * 13)[:150]] * 3
    order = rng.permutation(len(seqs))
    return MC.fastq(rng, [seqs[i] for i in order]), unit


def _queries(rng, model, s, rank, heavy, unit, hot):
    """a different mix on every rank: stored keys (light and repeated ones), absent keys, reverse complements, the 12-base repeat's
    keys; rank 0 asks the heavy key 50 times, every other rank once"""
    stored = np.array(sorted(model.d), dtype=np.uint64).reshape(-1, s.n_words)
    parts = [stored[rng.integers(0, stored.shape[0], 500 + 100 * rank)],
             MC.random_kmers(s, rng, 150 + 30 * rank),
             orc.revcomp(s, stored[rng.integers(0, stored.shape[0], 100)]),
             orc.kmers_from_string(s, (unit * 13)[:s.k + 11]),
             np.repeat(heavy, 50 if rank == 0 else 1, axis=0)]
    if hot is not None:
        parts.append(hot[rng.integers(0, hot.shape[0], 300)])
    q = np.concatenate(parts)
    return np.ascontiguousarray(q[rng.permutation(q.shape[0])])


# (k, strand, index kind, ranks, environment, hot keys in one bucket)
CASES = [
    pytest.param(21, "canonical", "position", 2, {}, False, id="k21-position-2"),
    pytest.param(31, "canonical", "posqual", 2, {}, False, id="k31-posqual-2"),
    pytest.param(40, "canonical", "position", 3, {}, False, id="k40-position-3"),
    pytest.param(31, "single", "position", 2, {"KMI_LOOKUP_CAP": "64"}, True, id="k31-single-small-tables-2"),
]


@pytest.mark.parametrize("k,strand,kind,world,env,with_hot", CASES)
def test_locate_over_ranks_matches_the_model(k, strand, kind, world, env, with_hot):
    from kmerind_amd import _lib as L
    rng = np.random.default_rng(2000 + k + world)
    s = orc.kspec(k)
    vw = MC.VW[kind]
    data, unit = _input(rng, k)
    model = LM.LocateModel(s, STRAND[strand], vw)
    model.build(data)
    hot = hot_keys = None
    if with_hot:   # 400 distinct keys of one placement bucket, one to three entries each: more than a 64-slot table takes in a pass
        hot_keys = MC.hot_keys(k, "DNA", 400)
        hot = MC.hot_tuples(rng, hot_keys, vw, s, n_filler=0)
        model.insert(*hot)
    heavy = model.transform(orc.kmers_from_string(s, b"A" * k))
    queries = [_queries(rng, model, s, r, heavy, unit, hot_keys) for r in range(world)]
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), k, strand, kind, env, data, hot, queries, ret), nprocs=world, join=True)
    R = [ret[r] for r in range(world)]
    assert sum(x["local"] for x in R) == model.size()
    n_heavy = len(model.d[tuple(heavy[0].tolist())])
    for r, x in enumerate(R):
        assert n_heavy > x["tile"] > 0          # the heavy key's segment crosses tile boundaries of the copy
        for cap in CAPS:
            want = model.locate(queries[r], cap)
            assert LM.difference(x["host"][cap], want) is None, "rank %d, max_occ %d: %s" % (r, cap, LM.difference(x["host"][cap], want))
        if with_hot:
            assert x["npass"] > 1               # the owner's tables took several passes
        want = model.locate(queries[r], LM.LOCATE_ALL)
        d = x["dev"]
        assert d["intact"] and d["sized"] == int(want[1][-1]) and d["hits"] == d["sized"]
        assert (d["occ"] == want[0]).all() and (d["off"] == want[1]).all()
        if r == 1:   # one hit short: exact totals, occ and offsets in full, nothing written into values; the peers do not notice
            assert d["st"] == L.ERR_OVERFLOW and (d["val"] == np.uint64(PATTERN)).all()
        else:
            assert d["st"] == L.OK
            assert LM.values_difference(d["val"], want[1], want[2]) is None, "rank %d, device form" % r
