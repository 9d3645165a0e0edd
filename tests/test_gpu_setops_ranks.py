"""kmi_index_compare_dist_host and kmi_index_combine over two ranks: two processes share the GPU over
kmerind_amd.transport.GroupComm (as in test_gpu_spectrum_ranks.py). Both indexes are built over the same communicator, so a key of
either lives on the same rank: the all-reduced overlap on every rank is the overlap of the two whole maps, and combine runs locally
on each rank with the union of the shares being the combined map."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import index_model as M
from tests import oracle as orc
from tests import setops_model as SM

pytestmark = pytest.mark.gpu
K_ = 31


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, datas, shares, queries, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        cfg = K.make_config(K_, "DNA", strand="canonical")

        def built(which):
            idx = K.CountIndex(ctx, cfg)
            b, e = shares[which][rank]
            buf = np.frombuffer(datas[which][b:e], dtype=np.uint8).copy()
            d = ctx.alloc(max(buf.size, 16) + 64)
            if buf.size:
                ctx.to_device(d, buf)
            ctx.check(L.lib.kmi_index_build_dist_dev(idx.h, comm.h, C.c_void_p(d), buf.size, b))
            ctx.free(d)
            return idx

        def find_all(idx):
            r = L.Results()
            ctx.check(L.lib.kmi_index_find_dist_host(idx.h, comm.h, queries.ctypes.data_as(C.c_void_p), queries.shape[0], C.byref(r)))
            n = r.n
            fk = np.ctypeslib.as_array(r.keys, shape=(n,)).copy().reshape(-1, 1) if n else np.zeros((0, 1), dtype=np.uint64)
            fv = np.ctypeslib.as_array(r.values, shape=(n,)).copy() if n else np.zeros(0, dtype=np.uint64)
            L.lib.kmi_results_free(C.byref(r))
            return fk, fv

        a, a2, b = built("a"), built("a"), built("b")
        out = dict(owner=(a.owner_ranks(), b.owner_ranks()), local=(a.local_size(), b.local_size()))
        before = comm.calls["allreduce"]
        out["overlap"] = a.compare(b, comm=comm)
        out["reduces"] = comm.calls["allreduce"] - before
        # an index built on this rank alone does not share the owner rule
        alone = K.CountIndex(ctx, cfg)
        alone.insert(queries[:100])
        o = L.IndexOverlap()
        before = comm.calls["allreduce"]
        out["alone"] = (alone.owner_ranks(), L.lib.kmi_index_compare_dist_host(alone.h, a.h, comm.h, C.byref(o)),
                        L.lib.kmi_index_compare_dist_host(a.h, alone.h, comm.h, C.byref(o)), comm.calls["allreduce"] - before)
        out["n_min"] = a.combine(b, "intersect_min")
        out["f_min"] = find_all(a)
        out["n_add"] = a2.combine(b, "union_add")
        out["f_add"] = find_all(a2)
        out["local_b_after"] = b.local_size()
        ret[rank] = out
        for i in (a, a2, b, alone):
            i.close()
        comm.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", ["plain", "empty-rank0"])
def test_compare_and_combine_over_two_ranks(case):
    from kmerind_amd import _lib as L
    from kmerind_amd import fileio
    rng = np.random.default_rng(77)
    genome = M.random_seq(rng, 20_000)
    datas = {"a": M.fastq(M.background(rng, 400, genome=genome)),
             "b": M.fastq(M.background(rng, 400, genome=genome[:10_000] + M.random_seq(rng, 10_000)), tag=b"s")}
    shares = {w: ([(0, 0), (0, len(d))] if case == "empty-rank0" else list(fileio.partition_fastq(d, 2))) for w, d in datas.items()}
    s = orc.kspec(K_)
    models = {}
    for w, d in datas.items():
        models[w] = M.CountModel(K_, orc.DNA, orc.CANONICAL)
        models[w].insert(orc.extract(s, d, orc.FASTQ)["kmers"])
    ma, mb = models["a"], models["b"]
    queries = np.ascontiguousarray(np.concatenate([ma.export()[0], mb.export()[0]]))
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), datas, shares, queries, ret), nprocs=2, join=True)
    R = [ret[r] for r in range(2)]
    want = SM.overlap(ma, mb)
    assert 0 < want["n_shared"] < min(want["n_a"], want["n_b"])
    w_min, w_add = SM.combined(ma, mb, "intersect_min"), SM.combined(ma, mb, "union_add")
    for x in R:
        assert x["owner"] == R[0]["owner"] and x["owner"][0] == x["owner"][1]
        if case == "plain":
            assert x["owner"] == (2, 2)   # the record exchange built both
        assert {w: x["overlap"][w] for w in SM.WORDS} == {w: want[w] for w in SM.WORDS}
        assert x["overlap"]["jaccard"] == want["jaccard"] and x["overlap"]["weighted_jaccard"] == want["weighted_jaccard"]
        assert x["reduces"] <= 2   # the verdict and the sums
        if x["owner"][0] != 1:   # refused on this rank, before anything collective
            assert x["alone"] == (1, L.ERR_INVALID, L.ERR_INVALID, 0)
        assert M.first_difference(x["f_min"][0], x["f_min"][1], *w_min.find(queries)) is None
        assert M.first_difference(x["f_add"][0], x["f_add"][1], *w_add.find(queries)) is None
    assert sum(x["local"][0] for x in R) == ma.size() and sum(x["local"][1] for x in R) == mb.size()
    assert sum(x["n_min"] for x in R) == w_min.size() and sum(x["n_add"] for x in R) == w_add.size()
    assert sum(x["local_b_after"] for x in R) == mb.size()
