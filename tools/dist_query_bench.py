"""seed_reads and lookup against an index held over ranks, against the route they replace (not the headline metric). 2 and then 4
ranks share GPU 0 over kmerind_amd.transport.GroupComm (gloo), so what is timed is the protocol's device work and its staging
through the host, not an interconnect.
  python tools/dist_query_bench.py [genome_Mbp [reads]]
Per world size: a position index (k = 21, canonical) of a synthetic FASTA genome built over the ranks
(kmi_index_build_fasta_file_dist_host) and a count index of the reads built over the ranks (kmi_index_build_dist_host); every rank
takes its record-aligned share of the 150-base reads. Timed (every route warmed once; a barrier before, the slowest rank counts):
  (a) seed_reads over ranks, device form: the sizing call and the call into buffers of exactly that size
  (b) the route it replaces on the same index and reads: kmi_extract_dev of the share, kmi_index_find_dist_host, the strand
      transform, and the numpy join back to read order; must reach the same occ, offsets and per-window sorted values
  (c) lookup over ranks of the share's k-mers (device form) against kmi_index_find_dist_host on the count index + the numpy join
  (d) the segmented copy (qd_segcopy) of the filling call against a device-to-device copy of the value bytes it moves
Default: 20 Mbp, 40 000 reads."""
import ctypes as C
import os
import socket
import sys
import time

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
K_ = 21


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _join(q, fk, fv, max_occ):
    """(occ, offsets, values) in query order from the (key, value) pairs a find() returned: sort the pairs by key, search every
    query's key, gather"""
    order = np.argsort(fk, kind="stable")
    fk, fv = fk[order], fv[order]
    uk, first, cnt = np.unique(fk, return_index=True, return_counts=True)
    at = np.minimum(np.searchsorted(uk, q), max(uk.size - 1, 0))
    hit = uk[at] == q if uk.size else np.zeros(q.size, dtype=bool)
    occ = np.where(hit, cnt[at] if uk.size else 0, 0).astype(np.uint32)
    listed = np.where(occ <= max_occ, occ, 0).astype(np.uint64)
    off = np.zeros(q.size + 1, dtype=np.uint64)
    np.cumsum(listed, out=off[1:])
    src = np.repeat(first[at].astype(np.int64) - off[:-1].astype(np.int64), listed.astype(np.int64)) + np.arange(int(off[-1]), dtype=np.int64)
    return occ, off, fv[src], (first, at, hit)


def _worker(rank, world, port, fasta, fastq, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import torch
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        from kmerind_amd import fileio
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)

        def slowest(ms):
            t = torch.tensor([ms], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t[0])

        def timed(fn):
            fn()
            dist.barrier()
            t0 = time.perf_counter()
            r = fn()
            return r, slowest((time.perf_counter() - t0) * 1e3)

        pidx = K.PositionIndex(ctx, K.make_config(K_, "DNA", strand="canonical", index_kind="position", seq_format="fasta"))
        ctx.check(L.lib.kmi_index_build_fasta_file_dist_host(pidx.h, comm.h, fasta.ctypes.data_as(C.c_void_p), fasta.size))
        b, e = fileio.partition_fastq(fastq, world)[rank]
        share = np.ascontiguousarray(fastq[b:e])
        cidx = K.CountIndex(ctx, K.make_config(K_, "DNA", strand="canonical"))
        ctx.check(L.lib.kmi_index_build_dist_host(cidx.h, comm.h, share.ctypes.data_as(C.c_void_p), share.size, b))
        d_in = ctx.alloc(share.size + 64)
        ctx.to_device(d_in, share)

        # ---- (a) seed_reads over ranks
        def seed():
            nr, nk, nh = pidx.seed_reads_device(d_in, share.size, comm=comm)
            occ, off, val = np.zeros(nk, dtype=np.uint32), np.zeros(nk + 1, dtype=np.uint64), np.zeros(max(nh, 1), dtype=np.uint64)
            d = [ctx.alloc(max(n, 8)) for n in (nr * 32, occ.nbytes, off.nbytes, val.nbytes)]
            pidx.seed_reads_device(d_in, share.size, d[0], nr, d[1], d[2], nk, d[3], nh, comm=comm)
            ctx.synchronize()
            return d, (occ, off, val[:nh])

        def seed_and_free():
            d, arrays = seed()
            for p in d:
                ctx.free(p)
            return arrays

        seed_and_free()
        ctx.profile(True)
        ctx.profile_reset()
        dist.barrier()
        t0 = time.perf_counter()
        d, (occ, off, val) = seed()
        seed_ms = slowest((time.perf_counter() - t0) * 1e3)
        kern = {p["name"]: p["total_ms"] for p in ctx.profile_get() if p["launches"]}
        ctx.profile(False)
        for a, p in zip((occ, off, val), d[1:]):
            if a.nbytes:
                ctx.to_host(a, p)
        for p in d:
            ctx.free(p)
        nq, n_hits = occ.size, val.size

        # ---- (b) the route it replaces
        qcfg = K.make_config(K_, "DNA", strand="canonical")

        def windows():
            dq = ctx.alloc(max(nq, 1) * 8)
            nt, ns = C.c_uint64(), C.c_uint64()
            ctx.check(L.lib.kmi_extract_dev(ctx.h, C.byref(qcfg), C.c_void_p(d_in), share.size, 0, C.c_void_p(dq), None, nq, C.byref(nt), C.byref(ns)))
            q = np.zeros(nq, dtype=np.uint64)
            if nq:
                ctx.to_host(q, dq)
            ctx.free(dq)
            return q

        def find(idx, q):
            r = L.Results()
            ctx.check(L.lib.kmi_index_find_dist_host(idx.h, comm.h, q.ctypes.data_as(C.c_void_p), q.shape[0], C.byref(r)))
            fk = np.ctypeslib.as_array(r.keys, shape=(r.n,)).copy() if r.n else np.zeros(0, dtype=np.uint64)
            fv = np.ctypeslib.as_array(r.values, shape=(r.n,)).copy() if r.n else np.zeros(0, dtype=np.uint64)
            L.lib.kmi_results_free(C.byref(r))
            return fk, fv

        def old_seed():
            q = windows()
            fk, fv = find(pidx, q)
            return _join(ctx.canonical(qcfg, q)[:, 0] if nq else q, fk, fv, L.LOCATE_ALL)[:3]

        (h_occ, h_off, h_val), old_seed_ms = timed(old_seed)
        assert (occ == h_occ).all() and (off == h_off).all(), "rank %d: the two routes disagree on occ / offsets" % rank
        win = np.repeat(np.arange(nq, dtype=np.int64), (h_off[1:] - h_off[:-1]).astype(np.int64))
        assert (val[np.lexsort((val, win))] == h_val[np.lexsort((h_val, win))]).all(), "rank %d: the two routes disagree on the values" % rank

        # ---- (c) lookup over ranks
        q = windows()
        dq, dc = ctx.alloc(max(q.nbytes, 8)), ctx.alloc(max(nq * 4, 8))
        if nq:
            ctx.to_device(dq, q)

        def new_lookup():
            cidx.lookup_device(dq, nq, dc, comm=comm)
            counts = np.zeros(nq, dtype=np.uint32)
            if nq:
                ctx.to_host(counts, dc)
            return counts

        def old_lookup():
            fk, fv = find(cidx, q)
            qc = ctx.canonical(qcfg, q)[:, 0] if nq else q
            order = np.argsort(fk)
            fk, fv = fk[order], fv[order]
            at = np.minimum(np.searchsorted(fk, qc), max(fk.size - 1, 0))
            return np.where(fk[at] == qc, fv[at], 0).astype(np.uint32) if fk.size else np.zeros(nq, dtype=np.uint32)

        counts, lookup_ms = timed(new_lookup)
        h_counts, old_lookup_ms = timed(old_lookup)
        assert (counts == h_counts).all(), "rank %d: the two lookup routes disagree" % rank
        ctx.free(dq)
        ctx.free(dc)

        # ---- (d) the segmented copy against a plain copy of the value bytes it reads and writes
        # (one rank after the other: the ranks share the GPU. The kernel's own time above was taken while the peers worked too.)
        src, dst = ctx.alloc(max(n_hits, 1) * 8), ctx.alloc(max(n_hits, 1) * 8)
        copy_ms = 0.0
        for turn in range(world):
            dist.barrier()
            if turn != rank:
                continue
            ctx.check(L.lib.kmi_copy_on_device(ctx.h, C.c_void_p(dst), C.c_void_p(src), max(n_hits, 1) * 8))
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                ctx.check(L.lib.kmi_copy_on_device(ctx.h, C.c_void_p(dst), C.c_void_p(src), max(n_hits, 1) * 8))
            ctx.synchronize()
            copy_ms = (time.perf_counter() - t0) * 1e3 / 10
        dist.barrier()
        ctx.free(src)
        ctx.free(dst)
        out[rank] = dict(nq=nq, n_hits=n_hits, reads=int(np.count_nonzero(share == 10)) // 4, seed_ms=seed_ms, old_seed_ms=old_seed_ms,
                         lookup_ms=lookup_ms, old_lookup_ms=old_lookup_ms, segcopy_ms=kern.get("qd_segcopy", float("nan")), copy_ms=copy_ms,
                         entries=(pidx.local_size(), cidx.local_size()),
                         kern={n: round(v, 3) for n, v in kern.items() if v >= 0.01})
        ctx.free(d_in)
        pidx.close()
        cidx.close()
        comm.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


def main():
    from locate_bench import synth
    g = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 40_000
    fasta, fastq = synth(g, n_reads, np.random.default_rng(4))
    print("position index (k=%d canonical) of a FASTA genome of %d Mbp and count index of %d reads of 150 bases (%d bytes of FASTQ), both held "
          "over ranks that share one GPU over gloo" % (K_, g, n_reads, fastq.size))
    for world in (2, 4):
        out = mp.Manager().dict()
        mp.spawn(_worker, args=(world, _free_port(), fasta, fastq, out), nprocs=world, join=True)
        R = [out[r] for r in range(world)]
        x = R[0]
        print("%d ranks: entries per rank %s / %s; windows per rank %s; hits per rank %s"
              % (world, [r["entries"][0] for r in R], [r["entries"][1] for r in R], [r["nq"] for r in R], [r["n_hits"] for r in R]))
        print("  (a) seed_reads over ranks, sizing call + filling call: %.1f ms wall (slowest rank)" % x["seed_ms"])
        print("      kernels of both calls on rank 0 (ms): %s" % x["kern"])
        print("  (b) extract_dev + find_dist_host + strand transform + numpy join: %.1f ms wall (slowest rank); the routes agree; new route %.1f x faster"
              % (x["old_seed_ms"], x["old_seed_ms"] / x["seed_ms"]))
        print("  (c) lookup over ranks, device form + counts to the host: %.1f ms; find_dist_host + numpy join: %.1f ms; the routes agree; new route %.1f x faster"
              % (x["lookup_ms"], x["old_lookup_ms"], x["old_lookup_ms"] / x["lookup_ms"]))
        for r, y in enumerate(R):
            print("  (d) rank %d: qd_segcopy %.3f ms for %d hits; device-to-device copy of their %d value bytes: %.3f ms (mean of 10); kernel / copy = %.2f"
                  % (r, y["segcopy_ms"], y["n_hits"], y["n_hits"] * 8, y["copy_ms"], y["segcopy_ms"] / y["copy_ms"]))


if __name__ == "__main__":
    main()
