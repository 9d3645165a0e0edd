"""De Bruijn node build rate (not the headline metric): kmi_dbg_build_dev over a resident FASTQ buffer, per-kernel times,
and the checker's CPU restatement on a bounded sample for scale.
  python tools/dbg_bench.py [reads] [genome] [k]
FASTA: a synthetic genome of 60-character lines (8 records), built from host bytes on one rank -- kmi_dbg_build_host over the whole
file, and kmi_dbg_build_fasta_range_dist_host over a one-rank communicator on the same bytes -- with per-kernel times.
  python tools/dbg_bench.py --fasta [genome] [k]
Unitigs: the node map of the FASTQ input above (default: config 2's, 10 M reads of a 100 Mbp genome, k = 31), then kmi_dbg_compact
timed warm, with its pointer-jumping rounds, per-kernel times and unitig statistics.
  python tools/dbg_bench.py --unitigs [reads] [genome] [k]"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kmerind_amd as K


def synth_fasta(genome, n_rec=8, line=60, seed=7):
    rng = np.random.default_rng(seed)
    parts = []
    per = genome // n_rec
    for r in range(n_rec):
        bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, per, dtype=np.uint8)]
        n_lines = (per + line - 1) // line
        body = np.full(n_lines * (line + 1), ord("\n"), dtype=np.uint8)
        pad = np.zeros(n_lines * line, dtype=bool)
        pad[:per] = True
        grid = body.reshape(n_lines, line + 1)
        full = np.full(n_lines * line, ord("\n"), dtype=np.uint8)
        full[:per] = bases
        grid[:, :line] = full.reshape(n_lines, line)
        flat = grid.reshape(-1)
        flat = flat[np.concatenate([pad.reshape(n_lines, line), np.ones((n_lines, 1), dtype=bool)], axis=1).reshape(-1)]
        parts.append(np.frombuffer(b">chr%d synthetic\n" % r, dtype=np.uint8))
        parts.append(flat)
    return np.ascontiguousarray(np.concatenate(parts))


def timed(ctx, steps, fn):
    fn()   # warm-up: workspace and node arrays reach their size
    torch.cuda.synchronize()
    ctx.profile(True); ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    prof = sorted(ctx.profile_get(), key=lambda p: -p["total_ms"])
    ctx.profile(False)
    return dt, {p["name"]: round(p["total_ms"] / steps, 3) for p in prof if p["launches"]}


def main_fasta(argv):
    from kmerind_amd import _lib as L
    genome = int(argv[0]) if len(argv) > 0 else 200_000_000
    k = int(argv[1]) if len(argv) > 1 else 31
    host = synth_fasta(genome)
    ctx = K.Context(0)
    g = K.DeBruijnNodes(ctx, K.make_config(k, seq_format="fasta"))
    steps = 3

    def whole():
        g.clear(); g.build(host)
    dt, prof = timed(ctx, steps, whole)
    print("FASTA de Bruijn nodes, k=%d, %d bytes (%d bp, 60-character lines): kmi_dbg_build_host %.2f ms per build, %d nodes"
          % (k, host.size, genome, dt * 1e3, g.local_size()))
    print(prof)
    if not hasattr(L.lib, "kmi_dbg_build_fasta_range_dist_host"):
        return
    comm = C.c_void_p()
    ctx.check(L.lib.kmi_comm_create(ctx.h, None, C.byref(comm)))
    need = C.c_int(0)

    def ranged():
        g.clear()
        ctx.check(L.lib.kmi_dbg_build_fasta_range_dist_host(g.h, comm, host.ctypes.data_as(C.c_void_p), host.size, 0, host.size, 1, -1, C.byref(need)))
    dt, prof = timed(ctx, steps, ranged)
    print("kmi_dbg_build_fasta_range_dist_host, one-rank communicator, same bytes: %.2f ms per build, %d nodes" % (dt * 1e3, g.local_size()))
    print(prof)
    L.lib.kmi_comm_destroy(comm)


def main_unitigs(argv):
    from kmerind_amd import _lib as L
    n_reads = int(argv[0]) if len(argv) > 0 else 10_000_000
    genome = int(argv[1]) if len(argv) > 1 else 100_000_000
    k = int(argv[2]) if len(argv) > 2 else 31
    host = np.asarray(K.synth_fastq(seed=2, genome_len=genome, n_reads=n_reads))   # (config 2's seed)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(host).to(dev)
    ctx = K.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    g.build_device(d.data_ptr(), host.size)
    del d
    torch.cuda.synchronize()
    nu, nb = C.c_uint64(), C.c_uint64()

    def compact():
        ctx.check(L.lib.kmi_dbg_compact(g.h, 1, C.byref(nu), C.byref(nb)))
    steps = 5
    dt, prof = timed(ctx, steps, compact)
    ctx.profile(True); ctx.profile_reset()
    compact()
    rounds = sum(p["launches"] for p in ctx.profile_get() if p["name"] == "unitig_jump")
    ctx.profile(False)
    off, bases, occ, circ = g.unitigs(1)
    lens = np.sort(np.diff(off.astype(np.int64)))[::-1]
    n50 = int(lens[np.searchsorted(np.cumsum(lens), lens.sum() / 2)]) if lens.size else 0
    print("unitigs of the de Bruijn graph, k=%d, %d reads over %d bp, %d nodes: kmi_dbg_compact %.2f ms (warm, mean of %d), %d jumping rounds"
          % (k, n_reads, genome, g.local_size(), dt * 1e3, steps, rounds))
    print(prof)
    print("%d unitigs, %d bases, %d circular; length max %d, mean %.1f, N50 %d; occurrences %d"
          % (nu.value, nb.value, int(circ.sum()), int(lens[0]) if lens.size else 0, float(lens.mean()) if lens.size else 0.0, n50, int(occ.sum())))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--fasta":
        return main_fasta(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--unitigs":
        return main_unitigs(sys.argv[2:])
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    genome = int(sys.argv[2]) if len(sys.argv) > 2 else 20_000_000
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 31
    host = np.asarray(K.synth_fastq(seed=5, genome_len=genome, n_reads=n_reads))
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(host).to(dev)
    ctx = K.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    for _ in range(2):
        g.clear(); g.build_device(d.data_ptr(), host.size)
    torch.cuda.synchronize()
    ctx.profile(True); ctx.profile_reset()
    steps = 3
    t0 = time.perf_counter()
    for _ in range(steps):
        g.clear(); g.build_device(d.data_ptr(), host.size)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    nk = n_reads * (150 - k + 1)
    prof = sorted(ctx.profile_get(), key=lambda p: -p["total_ms"])
    print("de Bruijn nodes, k=%d, %d reads over %d bp: %.2f ms per build, %.2f G k-mers/s, %d nodes" % (k, n_reads, genome, dt * 1e3, nk / dt / 1e9, g.local_size()))
    print({p["name"]: round(p["total_ms"] / steps, 3) for p in prof if p["launches"]})
    # the checker's restatement on the first 20 000 reads (one core)
    from tests import oracle as orc
    s = orc.kspec(k)
    head = bytes(host[: 315 * 20_000])
    t0 = time.perf_counter()
    kk, ee = orc.dbg_parse(s, head)
    m = orc.DbgMap(s)
    m.insert(kk, ee)
    dt_cpu = time.perf_counter() - t0
    print("CPU restatement (1 core, 20 000 reads): %.2f M k-mers/s" % (kk.shape[0] / dt_cpu / 1e6))


if __name__ == "__main__":
    main()
