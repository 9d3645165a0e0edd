"""kmi_index_spectrum_dist_host and kmi_index_retain_counts over two ranks: two processes share the GPU over
kmerind_amd.transport.GroupComm (as in test_gpu_dist_clayer.py). The all-reduced spectrum on every rank is the spectrum of the
oracle's single map; the filter runs locally on each rank and the union of the shares is the filtered map."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import index_model as M
from tests import oracle as orc
from tests import spectrum_cases as S

pytestmark = pytest.mark.gpu
K_ = 31
N_BINS = 300


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, data, shares, queries, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        idx = K.CountIndex(ctx, K.make_config(K_, "DNA", strand="canonical"))
        b, e = shares[rank]
        buf = np.frombuffer(data[b:e], dtype=np.uint8).copy()
        d = ctx.alloc(max(buf.size, 16) + 64)
        if buf.size:
            ctx.to_device(d, buf)
        ctx.check(L.lib.kmi_index_build_dist_dev(idx.h, comm.h, C.c_void_p(d), buf.size, b))
        local_before = idx.local_size()
        hist = np.ones(N_BINS, dtype=np.uint64)
        t = L.SpectrumTotals()
        before = comm.calls["allreduce"]
        ctx.check(L.lib.kmi_index_spectrum_dist_host(idx.h, comm.h, N_BINS, hist.ctypes.data_as(C.c_void_p), C.byref(t)))
        reduces = comm.calls["allreduce"] - before
        erased = idx.retain_counts(2)
        r = L.Results()
        ctx.check(L.lib.kmi_index_count_dist_host(idx.h, comm.h, queries.ctypes.data_as(C.c_void_p), queries.shape[0], C.byref(r)))
        n = r.n
        ck = np.ctypeslib.as_array(r.keys, shape=(n,)).copy().reshape(-1, 1)
        cv = np.ctypeslib.as_array(r.values, shape=(n,)).copy()
        L.lib.kmi_results_free(C.byref(r))
        hist2 = np.ones(N_BINS, dtype=np.uint64)
        ctx.check(L.lib.kmi_index_spectrum_dist_host(idx.h, comm.h, N_BINS, hist2.ctypes.data_as(C.c_void_p), None))
        ret[rank] = dict(hist=hist, totals=K.CountIndex._totals(t), reduces=reduces, local_before=local_before, erased=erased,
                         local_after=idx.local_size(), ck=ck, cv=cv, hist2=hist2)
        idx.close()
        comm.close()
        ctx.free(d)
        ctx.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", ["plain", "empty-rank0"])
def test_spectrum_and_filter_over_two_ranks(case):
    from kmerind_amd import fileio
    rng = np.random.default_rng(31)
    data = M.fastq(M.background(rng, 400))
    shares = [(0, 0), (0, len(data))] if case == "empty-rank0" else list(fileio.partition_fastq(data, 2))
    s = orc.kspec(K_)
    allk = orc.extract(s, data, orc.FASTQ)["kmers"]
    model = M.CountModel(K_, orc.DNA, orc.CANONICAL)
    model.insert(allk)
    queries = np.ascontiguousarray(allk)
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), data, shares, queries, ret), nprocs=2, join=True)
    R = [ret[r] for r in range(2)]
    om = orc.CountMap(s, orc.CANONICAL)
    om.insert(allk)
    want = S.spectrum_of_counts(om.export()[1], N_BINS)
    assert want[1] == S.model_spectrum(model, N_BINS)[1]
    assert (model.export()[1] == 1).any() and (model.export()[1] >= 2).any()
    for x in R:
        S.assert_spectrum((x["hist"], x["totals"]), want, case)
        assert x["reduces"] == 3   # the verdict, the sums, the extremes
    assert R[0]["totals"] == R[1]["totals"]
    assert sum(x["local_before"] for x in R) == model.size()
    counts = model.export()[1]
    assert sum(x["erased"] for x in R) == int((counts < 2).sum())
    assert sum(x["local_after"] for x in R) == int((counts >= 2).sum())
    filtered = model.copy()
    filtered.d = {key: c for key, c in model.d.items() if c >= 2}
    ek, ec = filtered.count(queries)
    for x in R:
        assert M.first_difference(x["ck"], x["cv"], ek, ec) is None
        S.assert_spectrum((x["hist2"], None), (S.model_spectrum(filtered, N_BINS)[0], None), case + " after the filter")
