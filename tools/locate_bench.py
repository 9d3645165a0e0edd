"""Seeding reads against a position index on the device against the host route it replaces (not the headline metric): a position
index (k = 21, canonical) of a synthetic FASTA genome, as tools/fasta_bench.py synthesises it, and 150-base reads cut from both
strands of that genome.
  python tools/locate_bench.py [genome_Mbp [reads [max_occ]]]
Timed (every route warmed once, the device synchronised before the host clock is read):
  (a) seed_reads_device: the sizing call and the call into buffers of exactly that size; wall time and the per-kernel times
  (b) today's route to the same arrays: kmi_extract_dev, kmi_index_find_hits_dev + kmi_index_find_dev, the results to the host,
      the strand transform of the reads' k-mers, and the join back to read order with numpy (sort the found pairs by key, search
      every window's key, gather); must reach the same occ, offsets and per-window sorted values
  (c) a device-to-device copy of the bytes the two per-bucket kernels must read: the bandwidth yardstick
Default: 100 Mbp, 200 000 reads, no cap."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kmerind_amd as K
from kmerind_amd import _lib as L
from kmerind_amd.core import READ_SEEDS_DTYPE

READ_LEN = 150
COMP = np.zeros(256, dtype=np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


def synth(g_mbp, n_reads, rng):
    """(FASTA bytes, FASTQ bytes): G random bases, 80 per line, one header per 50 Mbp; reads of READ_LEN bases from random places
    of the records, every second one reverse-complemented"""
    parts, seqs = [], []
    for r in range(max(1, g_mbp // 50)):
        n = min(50, g_mbp) * 1_000_000 // 80 * 80
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n, dtype=np.uint8)]
        lines = np.empty((n // 80, 81), dtype=np.uint8)
        lines[:, :80] = seq.reshape(-1, 80)
        lines[:, 80] = 10
        parts += [np.frombuffer(b">chr%d\n" % r, dtype=np.uint8), lines.reshape(-1)]
        seqs.append(seq)
    genome = np.concatenate(seqs)
    per = seqs[0].size
    rec = rng.integers(0, len(seqs), size=n_reads)
    start = rec * per + rng.integers(0, per - READ_LEN + 1, size=n_reads)
    bases = genome[start[:, None] + np.arange(READ_LEN)[None, :]]
    flip = np.arange(n_reads) % 2 == 1
    bases[flip] = COMP[bases[flip][:, ::-1]]
    out = np.empty((n_reads, 3 + READ_LEN + 1 + 2 + READ_LEN + 1), dtype=np.uint8)
    out[:, 0:3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    out[:, 3:3 + READ_LEN] = bases
    out[:, 3 + READ_LEN:6 + READ_LEN] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    out[:, 6 + READ_LEN:6 + 2 * READ_LEN] = ord("I")
    out[:, -1] = 10
    return np.concatenate(parts), out.reshape(-1)


def to_dev(host, dev):
    return torch.from_numpy(np.concatenate([host, np.zeros((-host.size) % 16 + 16, np.uint8)])).to(dev)


def main():
    g = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 200_000
    max_occ = int(sys.argv[3]) if len(sys.argv) > 3 else L.LOCATE_ALL
    k = 21
    dev = torch.device("cuda", 0)
    fasta, fastq = synth(g, n_reads, np.random.default_rng(4))
    d_fa, d_fq = to_dev(fasta, dev), to_dev(fastq, dev)
    ctx = K.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    cfg = K.make_config(k, "DNA", strand="canonical", index_kind="position", seq_format="fasta")
    idx = K.PositionIndex(ctx, cfg)
    idx.build_device(d_fa.data_ptr(), fasta.size)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx.clear(); idx.build_device(d_fa.data_ptr(), fasta.size)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    n_entries = idx.local_size()
    print("position index, k=%d canonical, FASTA genome of %d Mbp: %d entries, built in %.1f ms; %d reads of %d bases (%d bytes of FASTQ), max_occ %s"
          % (k, g, n_entries, build_ms, n_reads, READ_LEN, fastq.size, "none" if max_occ == L.LOCATE_ALL else max_occ))

    # ---- (a) the device route
    def seed():
        nr, nk, nh = idx.seed_reads_device(d_fq.data_ptr(), fastq.size, max_occ=max_occ)
        rows = torch.empty(nr * 32, dtype=torch.uint8, device=dev)
        occ = torch.empty(nk, dtype=torch.int32, device=dev)
        off = torch.empty(nk + 1, dtype=torch.int64, device=dev)
        val = torch.empty(max(nh, 1), dtype=torch.int64, device=dev)
        idx.seed_reads_device(d_fq.data_ptr(), fastq.size, rows.data_ptr(), nr, occ.data_ptr(), off.data_ptr(), nk, val.data_ptr(), nh, max_occ=max_occ)
        torch.cuda.synchronize()
        return rows, occ, off, val[:nh]

    seed()
    ctx.profile(True); ctx.profile_reset()
    t0 = time.perf_counter()
    rows, occ, off, val = seed()
    seed_ms = (time.perf_counter() - t0) * 1e3
    kern = {p["name"]: round(p["total_ms"], 3) for p in ctx.profile_get() if p["launches"] and p["total_ms"] >= 0.01}
    ctx.profile(False)
    nq, n_hits = occ.numel(), val.numel()
    rows_h = rows.cpu().numpy().view(READ_SEEDS_DTYPE)
    print("(a) seed_reads_device, sizing call + filling call: %.2f ms wall; %d reads, %d windows, %d hits, %d windows listed, passes %d"
          % (seed_ms, rows_h.shape[0], nq, n_hits, int(rows_h["n_listed"].sum()), ctx.debug_counter(8)))
    print("    kernels of both calls (ms): %s" % kern)

    # ---- (b) today's route
    def host_route():
        t = [time.perf_counter()]
        qk = torch.empty(nq, dtype=torch.int64, device=dev)
        nt, ns, nf = C.c_uint64(), C.c_uint64(), C.c_uint64()
        qcfg = K.make_config(k, "DNA", strand="canonical")
        ctx.check(L.lib.kmi_extract_dev(ctx.h, C.byref(qcfg), C.c_void_p(d_fq.data_ptr()), fastq.size, 0, C.c_void_p(qk.data_ptr()), None, nq,
                                        C.byref(nt), C.byref(ns)))
        ctx.check(L.lib.kmi_index_find_hits_dev(idx.h, C.c_void_p(qk.data_ptr()), nq, C.byref(nf)))
        fk = torch.empty(max(nf.value, 1), dtype=torch.int64, device=dev)
        fv = torch.empty(max(nf.value, 1), dtype=torch.int64, device=dev)
        ctx.check(L.lib.kmi_index_find_dev(idx.h, C.c_void_p(qk.data_ptr()), nq, C.c_void_p(fk.data_ptr()), C.c_void_p(fv.data_ptr()), C.byref(nf)))
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        q = qk.cpu().numpy().view(np.uint64)
        fkh, fvh = fk[:nf.value].cpu().numpy().view(np.uint64), fv[:nf.value].cpu().numpy().view(np.uint64)
        t.append(time.perf_counter())
        q = ctx.canonical(qcfg, q)[:, 0]
        t.append(time.perf_counter())
        order = np.argsort(fkh, kind="stable")
        fkh, fvh = fkh[order], fvh[order]
        uk, first, cnt = np.unique(fkh, return_index=True, return_counts=True)
        at = np.minimum(np.searchsorted(uk, q), max(uk.size - 1, 0))
        hit = uk[at] == q if uk.size else np.zeros(q.size, dtype=bool)
        h_occ = np.where(hit, cnt[at] if uk.size else 0, 0).astype(np.uint32)
        listed = np.where(h_occ <= max_occ, h_occ, 0).astype(np.uint64)
        h_off = np.zeros(q.size + 1, dtype=np.uint64)
        np.cumsum(listed, out=h_off[1:])
        src = np.repeat(first[at].astype(np.int64) - h_off[:-1].astype(np.int64), listed.astype(np.int64)) + np.arange(int(h_off[-1]), dtype=np.int64)
        h_val = fvh[src]
        t.append(time.perf_counter())
        return h_occ, h_off, h_val, [(b - a) * 1e3 for a, b in zip(t, t[1:])]

    host_route()
    h_occ, h_off, h_val, parts = host_route()
    print("(b) extract_dev + find_hits_dev + find_dev, results to the host, strand transform, numpy join: %.1f + %.1f + %.1f + %.1f = %.1f ms wall"
          % (*parts, sum(parts)))
    g_occ, g_off, g_val = occ.cpu().numpy().view(np.uint32), off.cpu().numpy().view(np.uint64), val.cpu().numpy().view(np.uint64)
    assert (g_occ == h_occ).all() and (g_off == h_off).all(), "the two routes disagree on occ / offsets"
    # per window sorted values: sort by (window, value) on both sides
    win = np.repeat(np.arange(nq, dtype=np.int64), (h_off[1:] - h_off[:-1]).astype(np.int64))
    assert (g_val[np.lexsort((g_val, win))] == h_val[np.lexsort((h_val, win))]).all(), "the two routes disagree on the values"
    print("    the two routes agree on occ, offsets and every window's sorted values; device route %.1f x faster" % (sum(parts) / seed_ms))

    # ---- (c) the yardstick: the bytes the two per-bucket kernels must read at least, device to device
    count_bytes = n_entries * 8 + nq * 16                           # the index keys once, the query records
    fill_bytes = 2 * n_entries * 8 + nq * 16 + n_hits * (4 + 8)     # the keys twice (count, group), the records, a position and a value per hit
    for name, nbytes, times in (("bucket_locate_count", count_bytes, 2), ("bucket_locate_fill", fill_bytes, 1)):
        src = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
        dst = torch.empty_like(src)
        dst.copy_(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        copy_ms = e0.elapsed_time(e1) / 5
        kms = kern.get(name, float("nan")) / times
        print("(c) %s: %.3f ms per launch; device-to-device copy of its %d bytes: %.3f ms (mean of 5); kernel / copy = %.2f"
              % (name, kms, nbytes, copy_ms, kms / copy_ms))
        del src, dst
    idx.close()
    ctx.close()


if __name__ == "__main__":
    main()
