"""De Bruijn node build rate (not the headline metric): kmi_dbg_build_dev over a resident FASTQ buffer, per-kernel times,
and the checker's CPU restatement on a bounded sample for scale.
  python tools/dbg_bench.py [reads] [genome] [k]
FASTA: a synthetic genome of 60-character lines (8 records), built from host bytes on one rank -- kmi_dbg_build_host over the whole
file, and kmi_dbg_build_fasta_range_dist_host over a one-rank communicator on the same bytes -- with per-kernel times.
  python tools/dbg_bench.py --fasta [genome] [k]
Unitigs: the node map of the FASTQ input above (default: config 2's, 10 M reads of a 100 Mbp genome, k = 31), then kmi_dbg_compact
timed warm, with its pointer-jumping rounds, per-kernel times and unitig statistics.
  python tools/dbg_bench.py --unitigs [reads] [genome] [k]
Unitigs over ranks: N processes share the GPU over a gloo group (kmerind_amd/transport.py, as tests/test_gpu_dist_clayer.py starts
them); every rank builds its share of the reads collectively, then kmi_dbg_compact_dist_host is timed warm, with its jumping rounds,
exchanges, bytes exchanged per node and per-kernel times of rank 0. The transport stages every message through pinned host memory
and gloo, so these are not RCCL numbers. Default input: 1 M reads of a 10 Mbp genome (1e7 nodes), k = 31. --out FILE: the figures as JSON.
  python tools/dbg_bench.py --unitigs --ranks N [--out FILE] [reads] [genome] [k]
Cleaning: the same FASTQ input with substitutions put into the sequence lines on the host (numpy, seeded, default 0.5 % per base), so
that singleton nodes exist; then spectrum, retain_counts(2), prune_edges(1), each timed warm on a second build with per-kernel times,
and the unitig count and N50 as built, after the filter and after pruning. Yardsticks in the same run: unitig_table + unitig_links of
kmi_dbg_compact on the map prune_edges runs on, and device-to-device copies of the bytes the row compaction needs (lower bound) and
of every old entry read whole (upper bound of what it fetches).
  python tools/dbg_bench.py --clean [--rate R] [reads] [genome] [k]
Cleaning over ranks: N processes share the GPU over a gloo group as for --unitigs --ranks (staging through pinned host memory: not an
interconnect); retain on every rank's share, kmi_dbg_prune_edges_dist_host timed warm, bytes exchanged per node, the slowest rank's
wall time. Default input: 1 M reads of a 10 Mbp genome, k = 31.
  python tools/dbg_bench.py --clean --ranks N [--rate R] [--out FILE] [reads] [genome] [k]
Tip clipping: the --clean input after retain_counts(2) and prune_edges(1); then rounds of clip_tips(1, 2 k) + prune_edges(1) until a
round clips nothing (at most --rounds), each clip_tips timed once with its per-kernel times on a map whose workspace a first pass
over the whole pipeline has warmed, with the stats, the unitig count and the N50 behind every round. The yardstick in the same run:
kmi_dbg_compact on the map the first round runs on, whose table, links and jumping stages the call shares.
  python tools/dbg_bench.py --tips [--rate R] [--rounds N] [reads] [genome] [k]
Tip clipping over ranks: N processes share the GPU over a gloo group as for --clean --ranks (staging through pinned host memory: the
figures are device work plus host staging, not an interconnect), on its input after retain_counts(2) and prune_edges(1) over the
ranks; then rounds of kmi_dbg_clip_tips_dist_host + prune_edges until a round clips nothing anywhere (at most --rounds), each timed
once on a warmed workspace: wall on the slowest rank, the summed tips_dist_* kernel times of rank 0, exchanges, bytes exchanged per
node, the stats. Beside them, in the same run, the one-rank kmi_dbg_clip_tips on the same graph (the ranks' reads in one buffer), round
by round; the totals over the ranks must equal its stats in every round, or the run fails. Default input: 1 M reads of a 10 Mbp
genome, k = 31.
  python tools/dbg_bench.py --tips --ranks N [--rate R] [--rounds N] [--out FILE] [reads] [genome] [k]
Bubble popping: the map that --tips ends with; then rounds of pop_bubbles(1, 2 k) + prune_edges(1) until a round pops nothing (at
most --rounds), each pop_bubbles timed once with its per-kernel times, with the stats, the unitig count and the N50 behind every
round, and one tip round behind the last. The yardsticks in the same run: kmi_dbg_compact on the map the first round runs on, and a
device-to-device copy of the bytes bubbles_classify and bubbles_judge touch.
  python tools/dbg_bench.py --bubbles [--rate R] [--rounds N] [reads] [genome] [k]
Bubble popping over ranks: N processes share the GPU over a gloo group as for --tips --ranks (device work plus host staging, not an
interconnect), on the graph that --tips --ranks ends with; then rounds of kmi_dbg_pop_bubbles_dist_host + prune_edges until a round
pops nothing anywhere (at most --rounds), each timed once on a warmed workspace: wall on the slowest rank, the bubbles_dist_* kernel
times and all kernel times of rank 0, exchanges and bytes exchanged per node, split into the unitig stages' share and the call's own,
the stats. Beside them, in the same run, the one-rank kmi_dbg_pop_bubbles on the same graph, round by round; every field of the
totals over the ranks must equal its stats in every round, or the run fails. Default input: 1 M reads of a 10 Mbp genome, k = 31.
  python tools/dbg_bench.py --bubbles --ranks N [--rate R] [--rounds N] [--out FILE] [reads] [genome] [k]"""
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


def _ranks_worker(rank, world, port, n_reads, genome, k, steps, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kmerind_amd import _lib as L
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        lo, hi = n_reads * rank // world, n_reads * (rank + 1) // world
        host = np.asarray(K.synth_fastq(seed=2, genome_len=genome, n_reads=hi - lo, first_read=lo))
        g = K.DeBruijnNodes(ctx, K.make_config(k))
        t0 = time.perf_counter()
        g.build_dist(host, comm)
        build_s = time.perf_counter() - t0
        del host
        if rank == 0:
            print("built over %d ranks in %.1f s; rank 0 holds %d nodes" % (world, build_s, g.local_size()), flush=True)
        out = [C.c_uint64() for _ in range(4)]

        def compact():
            ctx.check(L.lib.kmi_dbg_compact_dist_host(g.h, comm.h, 1, *[C.byref(v) for v in out]))
        dist.barrier()
        t0 = time.perf_counter()
        compact()
        cold = time.perf_counter() - t0
        if rank == 0:
            print("first compaction %.2f s" % cold, flush=True)
        ctx.profile(True); ctx.profile_reset()
        dist.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            compact()
        warm = (time.perf_counter() - t0) / steps
        prof = {p["name"]: round(p["total_ms"] / steps, 3) for p in sorted(ctx.profile_get(), key=lambda p: -p["total_ms"]) if p["launches"]}
        ctx.profile(False)
        cnt = []
        v = C.c_uint64()
        for which in (5, 6, 7):
            ctx.check(L.lib.kmi_ctx_debug_counter(ctx.h, which, C.byref(v)))
            cnt.append(v.value)
        ret[rank] = dict(nodes=g.local_size(), cold_s=cold, warm_s=warm, rounds=cnt[0], exchanges=cnt[1], bytes_sent=cnt[2], unitigs_local=out[0].value,
                         unitigs_total=out[2].value, bases_total=out[3].value, kernels_ms=prof, build_s=build_s)
        g.close()
        comm.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


def main_unitigs_ranks(argv):
    import json
    import socket
    import torch.multiprocessing as mp
    world = int(argv[0])
    argv = argv[1:]
    out_path = None
    if argv and argv[0] == "--out":
        out_path, argv = argv[1], argv[2:]
    n_reads = int(argv[0]) if len(argv) > 0 else 1_000_000
    genome = int(argv[1]) if len(argv) > 1 else 10_000_000
    k = int(argv[2]) if len(argv) > 2 else 31
    steps = 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ret = mp.Manager().dict()
    mp.spawn(_ranks_worker, args=(world, port, n_reads, genome, k, steps, ret), nprocs=world, join=True)
    res = [ret[r] for r in range(world)]
    nodes = sum(r["nodes"] for r in res)
    sent = sum(r["bytes_sent"] for r in res)
    summary = dict(ranks=world, k=k, reads=n_reads, genome=genome, nodes=nodes, nodes_per_rank=[r["nodes"] for r in res],
                   warm_ms_per_rank=[round(r["warm_s"] * 1e3, 1) for r in res], cold_ms_rank0=round(res[0]["cold_s"] * 1e3, 1), steps=steps,
                   rounds=res[0]["rounds"], exchanges=res[0]["exchanges"], bytes_exchanged=sent, bytes_per_node=round(sent / max(nodes, 1), 1),
                   unitigs_total=res[0]["unitigs_total"], bases_total=res[0]["bases_total"], unitigs_per_rank=[r["unitigs_local"] for r in res],
                   kernels_ms_rank0=res[0]["kernels_ms"], transport="gloo over pinned host staging (not RCCL)")
    print("unitigs over %d ranks (gloo transport, pinned host staging: not RCCL), k=%d, %d reads over %d bp, %d nodes: kmi_dbg_compact_dist_host "
          "%.1f ms warm on the slowest rank (mean of %d), %d jumping rounds, %d exchanges, %.1f bytes exchanged per node"
          % (world, k, n_reads, genome, nodes, max(summary["warm_ms_per_rank"]), steps, summary["rounds"], summary["exchanges"], summary["bytes_per_node"]))
    print(json.dumps(summary))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


def with_substitutions(host, n_reads, rate, seed=11, read_len=150):
    """the FASTQ buffer of K.synth_fastq with substitutions in the sequence lines: every base changes to the next letter with
    probability `rate` (the number of changes is drawn once, their places uniformly)"""
    rec = host.size // n_reads
    off = int(np.flatnonzero(host[:rec] == ord("\n"))[0]) + 1   # the sequence line follows the header
    assert host.size == rec * n_reads and host[off + read_len] == ord("\n")
    rng = np.random.default_rng(seed)
    n_err = int(rng.binomial(n_reads * read_len, rate))
    at = rng.integers(0, n_reads * read_len, n_err, dtype=np.int64)
    pos = (at // read_len) * rec + off + at % read_len
    nxt = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"CGTA"):
        nxt[a] = b
    host = host.copy()
    host[pos] = nxt[host[pos]]
    return host, n_err


def _n50(off):
    lens = np.sort(np.diff(off.astype(np.int64)))[::-1]
    return int(lens[np.searchsorted(np.cumsum(lens), lens.sum() / 2)]) if lens.size else 0


def _flag(argv, name, default, conv):
    if name in argv:
        i = argv.index(name)
        v = conv(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def main_clean(argv):
    argv = list(argv)
    rate = _flag(argv, "--rate", 0.005, float)
    n_reads = int(argv[0]) if len(argv) > 0 else 10_000_000
    genome = int(argv[1]) if len(argv) > 1 else 100_000_000
    k = int(argv[2]) if len(argv) > 2 else 31
    host, n_err = with_substitutions(np.asarray(K.synth_fastq(seed=2, genome_len=genome, n_reads=n_reads)), n_reads, rate)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(host).to(dev)
    ctx = K.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    print("cleaning a de Bruijn node map, k=%d, %d reads over %d bp, %d substitutions (%.3g per base, seeded); one run on one GPU"
          % (k, n_reads, genome, n_err, rate))

    def kernels():
        prof = {p["name"]: round(p["total_ms"], 3) for p in sorted(ctx.profile_get(), key=lambda p: -p["total_ms"]) if p["launches"]}
        ctx.profile_reset()
        return prof

    def step(name, fn):
        torch.cuda.synchronize()
        ctx.profile_reset()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        prof = kernels()
        print("%-28s %9.2f ms  %s" % (name, ms, prof), flush=True)
        return r, prof

    for run in ("warm-up", "timed"):
        g.clear(); g.build_device(d.data_ptr(), host.size)
        torch.cuda.synchronize()
        ctx.profile(run == "timed"); ctx.profile_reset()
        if run == "timed":
            print("-- second build, every step timed once (wall time with the host's part, then the kernels' own times)")
        quiet = (lambda name, fn: (fn(), {})) if run == "warm-up" else step
        n0 = g.local_size()
        (hist, totals), _ = quiet("spectrum(256)", lambda: g.spectrum(256))
        (off0, _, _, _), _ = quiet("unitigs, as built", lambda: g.unitigs(1))
        erased, p_ret = quiet("retain_counts(2)", lambda: g.retain_counts(2))
        n1 = g.local_size()
        (off1, _, _, _), p_cmp = quiet("unitigs, after the filter", lambda: g.unitigs(1))
        stats, p_pr = quiet("prune_edges(1)", lambda: g.prune_edges(1))
        again, p_pr2 = quiet("prune_edges(1), second call", lambda: g.prune_edges(1))
        (off2, _, _, _), _ = quiet("unitigs, after pruning", lambda: g.unitigs(1))
    ctx.profile(False)
    print("spectrum: bins 1..5 %s, totals %s" % (hist[1:6].tolist(), totals))
    print("nodes %d -> %d (%d erased)" % (n0, n1, erased))
    print("prune stats %s" % stats)
    print("second call %s" % again)
    for name, off in (("as built", off0), ("after retain_counts(2)", off1), ("after prune_edges(1)", off2)):
        print("unitigs %-24s %10d, N50 %d" % (name, off.shape[0] - 1, _n50(off)))
    # yardstick of the prune kernel: table + links of the compaction on the same map in the same run
    links, table = p_cmp.get("unitig_links", float("nan")), p_cmp.get("unitig_table", float("nan"))
    print("dbg_prune %.3f ms (second call %.3f ms) + unitig_table %.3f ms; kmi_dbg_compact on the same %d nodes: unitig_links %.3f ms + unitig_table %.3f ms;"
          " dbg_prune / unitig_links = %.2f" % (p_pr.get("dbg_prune", float("nan")), p_pr2.get("dbg_prune", float("nan")), p_pr.get("unitig_table", float("nan")),
                                                n1, links, table, p_pr.get("dbg_prune", float("nan")) / links))
    # yardstick of the row compaction: a device-to-device copy of the bytes it reads and writes. The kernel reads the count of EVERY old
    # entry (4 bytes) but the key and the row of the SURVIVORS alone, and writes key, count and row of the survivors: those are the
    # bytes it needs. The survivors' keys and rows lie scattered among the others', so the memory system fetches more than that (whole
    # sectors around an 8-byte key); how much has not been counted. Every old entry read whole is the upper bound of what it can fetch.
    nw = g.n_words
    needed = n0 * 4 + n1 * (8 * nw + 32) + n1 * (8 * nw + 4 + 32)
    upper = n0 * (8 * nw + 4 + 32) + n1 * (8 * nw + 4 + 32)
    g.close()
    compact_ms = p_ret.get("bucket_retain_compact", float("nan"))
    for name, moved in (("the bytes it needs (every old count; key and row of the survivors; the survivors written)", needed),
                        ("the upper bound (every old entry read whole; the survivors written)", upper)):
        a = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        b.copy_(a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        copy_ms = e0.elapsed_time(e1) / 5
        del a, b
        print("bucket_retain_compact %.3f ms; %s: %d bytes read + written, device-to-device copy of as many %.3f ms (mean of 5), ratio %.2f"
              % (compact_ms, name, moved, copy_ms, compact_ms / copy_ms))


def main_tips(argv):
    argv = list(argv)
    rate = _flag(argv, "--rate", 0.005, float)
    max_rounds = _flag(argv, "--rounds", 8, int)
    n_reads = int(argv[0]) if len(argv) > 0 else 10_000_000
    genome = int(argv[1]) if len(argv) > 1 else 100_000_000
    k = int(argv[2]) if len(argv) > 2 else 31
    host, n_err = with_substitutions(np.asarray(K.synth_fastq(seed=2, genome_len=genome, n_reads=n_reads)), n_reads, rate)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(host).to(dev)
    ctx = K.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    print("clipping the tips of a de Bruijn node map, k=%d, %d reads over %d bp, %d substitutions (%.3g per base, seeded), after retain_counts(2) and "
          "prune_edges(1); clip_tips(1, %d); one run on one GPU" % (k, n_reads, genome, n_err, rate, 2 * k))

    def step(name, fn):
        torch.cuda.synchronize()
        ctx.profile_reset()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        prof = {p["name"]: round(p["total_ms"], 3) for p in sorted(ctx.profile_get(), key=lambda p: -p["total_ms"]) if p["launches"]}
        ctx.profile_reset()
        print("%-28s %9.2f ms  %s" % (name, ms, prof), flush=True)
        return r, ms, prof

    for run in ("warm-up", "timed"):
        g.clear(); g.build_device(d.data_ptr(), host.size)
        g.retain_counts(2)
        g.prune_edges(1)
        torch.cuda.synchronize()
        if run == "warm-up":   # the workspace and the pool reach their sizes
            g.unitigs(1); g.clip_tips(1); g.prune_edges(1); g.unitigs(1)
            continue
        ctx.profile(True); ctx.profile_reset()
        print("-- second build, every step timed once (wall time with the host's part, then the kernels' own times)")
        n1 = g.local_size()
        (off, _, _, _), cmp_ms, p_cmp = step("unitigs, before clipping", lambda: g.unitigs(1))
        print("unitigs %-24s %10d, N50 %d, %d nodes" % ("before clipping", off.shape[0] - 1, _n50(off), n1))
        first = None
        for r in range(1, max_rounds + 1):
            stats, ms, prof = step("clip_tips(1, %d), round %d" % (2 * k, r), lambda: g.clip_tips(1))
            first = first or (ms, prof, stats)
            pst, _, _ = step("prune_edges(1), round %d" % r, lambda: g.prune_edges(1))
            (off, _, _, _), _, _ = step("unitigs, round %d" % r, lambda: g.unitigs(1))
            print("round %d: %s; pruning cleared %d; unitigs %d, N50 %d, %d nodes"
                  % (r, stats, pst["n_set_before"] - pst["n_set_after"], off.shape[0] - 1, _n50(off), g.local_size()), flush=True)
            if stats["n_tips_clipped"] == 0:
                break
    ctx.profile(False)
    ms, prof, stats = first
    own = prof.get("tips_classify", float("nan")) + prof.get("tips_judge", float("nan"))
    shared = sum(v for n, v in prof.items() if n.startswith("unitig_"))
    shared_cmp = sum(v for n, v in p_cmp.items() if n in prof and n.startswith("unitig_"))
    print("round 1 on %d nodes: clip_tips %.2f ms wall against kmi_dbg_compact %.2f ms wall; tips_classify %.3f + tips_judge %.3f = %.3f ms against "
          "unitig_links %.3f ms (%.2f); the stages both run: %.3f ms in clip_tips, %.3f ms in kmi_dbg_compact; removal: tips_retain_count %.3f + "
          "bucket_offsets %.3f + tips_retain_compact %.3f ms"
          % (n1, ms, cmp_ms, prof.get("tips_classify", float("nan")), prof.get("tips_judge", float("nan")), own, p_cmp.get("unitig_links", float("nan")),
             own / p_cmp.get("unitig_links", float("nan")), shared, shared_cmp, prof.get("tips_retain_count", float("nan")),
             prof.get("bucket_offsets", float("nan")), prof.get("tips_retain_compact", float("nan"))))
    # bytes the two kernels of the call's own touch, against a device-to-device copy of as many: classify reads per node the scan
    # record (16) and writes the class (1); per head also the direction and circular flags (2), a ranking record (16) and two rows (64);
    # judge reads every class (1). Candidates add a key, a lookup, a row and a junction word each: few, not counted.
    nu = stats["n_unitigs"]
    moved = n1 * (16 + 1 + 1) + nu * (2 + 16 + 64)
    a = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    copy_ms = e0.elapsed_time(e1) / 5
    print("tips_classify + tips_judge %.3f ms; the bytes they touch (18 per node, 82 more per unitig): %d, device-to-device copy of as many %.3f ms "
          "(mean of 5), ratio %.2f" % (own, moved, copy_ms, own / copy_ms))
    g.close()


def main_bubbles(argv):
    argv = list(argv)
    rate = _flag(argv, "--rate", 0.005, float)
    max_rounds = _flag(argv, "--rounds", 8, int)
    n_reads = int(argv[0]) if len(argv) > 0 else 10_000_000
    genome = int(argv[1]) if len(argv) > 1 else 100_000_000
    k = int(argv[2]) if len(argv) > 2 else 31
    host, n_err = with_substitutions(np.asarray(K.synth_fastq(seed=2, genome_len=genome, n_reads=n_reads)), n_reads, rate)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(host).to(dev)
    ctx = K.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    print("popping the bubbles of a de Bruijn node map, k=%d, %d reads over %d bp, %d substitutions (%.3g per base, seeded), after retain_counts(2), "
          "prune_edges(1) and the rounds of clip_tips(1, %d) + prune_edges(1) of --tips; pop_bubbles(1, %d); one run on one GPU"
          % (k, n_reads, genome, n_err, rate, 2 * k, 2 * k))

    def step(name, fn):
        torch.cuda.synchronize()
        ctx.profile_reset()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        prof = {p["name"]: round(p["total_ms"], 3) for p in sorted(ctx.profile_get(), key=lambda p: -p["total_ms"]) if p["launches"]}
        ctx.profile_reset()
        print("%-28s %9.2f ms  %s" % (name, ms, prof), flush=True)
        return r, ms, prof

    for run in ("warm-up", "timed"):
        g.clear(); g.build_device(d.data_ptr(), host.size)
        g.retain_counts(2)
        g.prune_edges(1)
        for _ in range(max_rounds):   # the end state of --tips
            clipped = g.clip_tips(1)["n_tips_clipped"]
            g.prune_edges(1)
            if clipped == 0:
                break
        torch.cuda.synchronize()
        if run == "warm-up":   # the workspace and the pool reach their sizes
            g.unitigs(1); g.pop_bubbles(1); g.prune_edges(1); g.unitigs(1)
            continue
        ctx.profile(True); ctx.profile_reset()
        print("-- second build, every step timed once (wall time with the host's part, then the kernels' own times)")
        n1 = g.local_size()
        (off, _, _, _), cmp_ms, p_cmp = step("unitigs, before popping", lambda: g.unitigs(1))
        print("unitigs %-24s %10d, N50 %d, %d nodes" % ("before popping", off.shape[0] - 1, _n50(off), n1))
        first = None
        for r in range(1, max_rounds + 1):
            stats, ms, prof = step("pop_bubbles(1, %d), round %d" % (2 * k, r), lambda: g.pop_bubbles(1))
            first = first or (ms, prof, stats)
            pst, _, _ = step("prune_edges(1), round %d" % r, lambda: g.prune_edges(1))
            (off, _, _, _), _, _ = step("unitigs, round %d" % r, lambda: g.unitigs(1))
            print("round %d: %s; pruning cleared %d; unitigs %d, N50 %d, %d nodes"
                  % (r, stats, pst["n_set_before"] - pst["n_set_after"], off.shape[0] - 1, _n50(off), g.local_size()), flush=True)
            if stats["n_popped"] == 0:
                break
        tip, _, _ = step("clip_tips(1, %d), behind the popping" % (2 * k), lambda: g.clip_tips(1))
        print("a tip round behind the popping: %s" % tip)
    ctx.profile(False)
    ms, prof, stats = first
    nan = float("nan")
    own = prof.get("bubbles_classify", nan) + prof.get("bubbles_judge", nan)
    shared = sum(v for n, v in prof.items() if n.startswith("unitig_"))
    shared_cmp = sum(v for n, v in p_cmp.items() if n in prof and n.startswith("unitig_"))
    print("round 1 on %d nodes: pop_bubbles %.2f ms wall against kmi_dbg_compact %.2f ms wall; bubbles_classify %.3f + bubbles_judge %.3f = %.3f ms "
          "against unitig_links %.3f ms (%.2f); the stages both run: %.3f ms in pop_bubbles, %.3f ms in kmi_dbg_compact; removal: tips_retain_count %.3f + "
          "bucket_offsets %.3f + tips_retain_compact %.3f ms"
          % (n1, ms, cmp_ms, prof.get("bubbles_classify", nan), prof.get("bubbles_judge", nan), own, p_cmp.get("unitig_links", nan),
             own / p_cmp.get("unitig_links", nan), shared, shared_cmp, prof.get("tips_retain_count", nan), prof.get("bucket_offsets", nan),
             prof.get("tips_retain_compact", nan)))
    # bytes the two kernels of the call's own touch, against a device-to-device copy of as many. Per node: classify reads the scan record
    # (16) and writes the class (1), judge reads the class (1) and writes the verdict (1). Per head: the direction and circular flags (2), a
    # ranking record (16) and two rows (64). Per branch, classify: two end keys, two table probes (a slot and the key it names), the
    # neighbours' ranking record and direction (17), their rows (32), two junctions written (16), two mask words (8); judge: the junctions
    # (16), two rows (64), a mask word (4), the junction node's key, its own ranking record and direction (17), and for one sibling a
    # probe, a ranking record and direction (17), a class (1) and two junctions (16)
    nw, nu, nb = g.n_words, stats["n_unitigs"], stats["n_branches"]
    per_branch = 2 * (8 * nw + 4 + 8 * nw + 17 + 32) + 16 + 8 + 16 + 64 + 4 + 8 * nw + 17 + (4 + 8 * nw + 17 + 1 + 16)
    moved = n1 * (16 + 1 + 1 + 1) + nu * (2 + 16 + 64) + nb * per_branch
    a = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    copy_ms = e0.elapsed_time(e1) / 5
    print("bubbles_classify + bubbles_judge %.3f ms; the bytes they touch (19 per node, 82 more per unitig, %d more per branch): %d, device-to-device "
          "copy of as many %.3f ms (mean of 5), ratio %.2f" % (own, per_branch, moved, copy_ms, own / copy_ms))
    g.close()


def _clean_ranks_worker(rank, world, port, n_reads, genome, k, rate, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        lo, hi = n_reads * rank // world, n_reads * (rank + 1) // world
        host, _ = with_substitutions(np.asarray(K.synth_fastq(seed=2, genome_len=genome, n_reads=hi - lo, first_read=lo)), hi - lo, rate, seed=11 + rank)
        g = K.DeBruijnNodes(ctx, K.make_config(k))
        out = {}
        for run in ("warm-up", "timed"):
            g.clear(); g.build_dist(host, comm)
            n0 = g.local_size()
            hist, _ = g.spectrum(16, comm=comm)
            erased = g.retain_counts(2)
            ctx.profile(run == "timed"); ctx.profile_reset()
            dist.barrier()
            t0 = time.perf_counter()
            stats = g.prune_edges(1, comm=comm)
            wall = time.perf_counter() - t0
            prof = {p["name"]: round(p["total_ms"], 3) for p in sorted(ctx.profile_get(), key=lambda p: -p["total_ms"]) if p["launches"]}
            ctx.profile(False)
            out = dict(nodes_built=n0, nodes=g.local_size(), erased=erased, prune_ms=wall * 1e3, stats=stats, total=dict(g.prune_totals), kernels_ms=prof,
                       bytes_sent=ctx.debug_counter(13), hist=hist[:6].tolist())
        g.unitigs(1, comm=comm)
        out["unitigs_total"] = g.unitig_totals[0]
        ret[rank] = out
        g.close()
        comm.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


def main_clean_ranks(argv):
    import json
    import socket
    import torch.multiprocessing as mp
    argv = list(argv)
    world = int(argv.pop(0))
    rate = _flag(argv, "--rate", 0.005, float)
    out_path = _flag(argv, "--out", None, str)
    n_reads = int(argv[0]) if len(argv) > 0 else 1_000_000
    genome = int(argv[1]) if len(argv) > 1 else 10_000_000
    k = int(argv[2]) if len(argv) > 2 else 31
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ret = mp.Manager().dict()
    mp.spawn(_clean_ranks_worker, args=(world, port, n_reads, genome, k, rate, ret), nprocs=world, join=True)
    res = [ret[r] for r in range(world)]
    nodes = sum(r["nodes"] for r in res)
    sent = sum(r["bytes_sent"] for r in res)
    summary = dict(ranks=world, k=k, reads=n_reads, genome=genome, rate=rate, nodes_built=sum(r["nodes_built"] for r in res), nodes=nodes,
                   nodes_per_rank=[r["nodes"] for r in res], prune_ms_per_rank=[round(r["prune_ms"], 1) for r in res], bytes_exchanged=sent,
                   bytes_per_node=round(sent / max(nodes, 1), 1), stats_total=res[0]["total"], unitigs_total_after=res[0]["unitigs_total"],
                   kernels_ms_rank0=res[0]["kernels_ms"], transport="gloo over pinned host staging (not an interconnect)")
    print("cleaning over %d ranks (gloo transport, staging through pinned host memory: not an interconnect), k=%d, %d reads over %d bp, %d nodes after "
          "retain_counts(2): kmi_dbg_prune_edges_dist_host %.1f ms warm on the slowest rank (one call), %.1f bytes exchanged per node"
          % (world, k, n_reads, genome, nodes, max(summary["prune_ms_per_rank"]), summary["bytes_per_node"]))
    print(json.dumps(summary))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


def _share_reads(rank, world, n_reads, genome, rate):
    """the reads of one rank of the --clean / --tips inputs over ranks"""
    lo, hi = n_reads * rank // world, n_reads * (rank + 1) // world
    return with_substitutions(np.asarray(K.synth_fastq(seed=2, genome_len=genome, n_reads=hi - lo, first_read=lo)), hi - lo, rate, seed=11 + rank)[0]


def _tips_ranks_worker(rank, world, port, n_reads, genome, k, rate, max_rounds, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        host = _share_reads(rank, world, n_reads, genome, rate)
        g = K.DeBruijnNodes(ctx, K.make_config(k))
        rounds = []
        for run in ("warm-up", "timed"):
            g.clear(); g.build_dist(host, comm)
            g.retain_counts(2)
            g.prune_edges(1, comm=comm)
            for r in range(1, (1 if run == "warm-up" else max_rounds) + 1):   # (the warm-up: the workspace and the pool reach their sizes)
                n_before = g.local_size()
                ctx.profile(run == "timed"); ctx.profile_reset()
                dist.barrier()
                t0 = time.perf_counter()
                stats = g.clip_tips(1, comm=comm)
                wall = time.perf_counter() - t0
                prof = {p["name"]: round(p["total_ms"], 3) for p in sorted(ctx.profile_get(), key=lambda p: -p["total_ms"]) if p["launches"]}
                ctx.profile(False)
                total = dict(g.clip_totals)
                pst = g.prune_edges(1, comm=comm)
                if run == "timed":
                    rounds.append(dict(nodes=n_before, clip_ms=wall * 1e3, stats=stats, total=total, kernels_ms=prof, exchanges=ctx.debug_counter(14),
                                       bytes_sent=ctx.debug_counter(15), pruned_behind=g.prune_totals["n_set_before"] - g.prune_totals["n_set_after"]))
                if total["n_tips_clipped"] == 0:
                    break
        g.unitigs(1, comm=comm)
        ret[rank] = dict(rounds=rounds, unitigs_total=g.unitig_totals[0], nodes_final=g.local_size())
        g.close()
        comm.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


def main_tips_ranks(argv):
    import json
    import socket
    import torch.multiprocessing as mp
    argv = list(argv)
    world = int(argv.pop(0))
    rate = _flag(argv, "--rate", 0.005, float)
    max_rounds = _flag(argv, "--rounds", 8, int)
    out_path = _flag(argv, "--out", None, str)
    n_reads = int(argv[0]) if len(argv) > 0 else 1_000_000
    genome = int(argv[1]) if len(argv) > 1 else 10_000_000
    k = int(argv[2]) if len(argv) > 2 else 31
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ret = mp.Manager().dict()
    mp.spawn(_tips_ranks_worker, args=(world, port, n_reads, genome, k, rate, max_rounds, ret), nprocs=world, join=True)
    res = [ret[r] for r in range(world)]
    # the one-rank call on the same graph: the ranks' reads in one buffer, after the ranks' processes have left the GPU
    host = np.concatenate([_share_reads(r, world, n_reads, genome, rate) for r in range(world)])
    ctx = K.Context(0)
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    one = []
    for run in ("warm-up", "timed"):
        g.clear(); g.build(host)
        g.retain_counts(2)
        g.prune_edges(1)
        for r in range(1, (1 if run == "warm-up" else max_rounds) + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats = g.clip_tips(1)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            g.prune_edges(1)
            if run == "timed":
                one.append(dict(clip_ms=ms, stats=stats))
            if stats["n_tips_clipped"] == 0:
                break
    one_unitigs = g.unitigs(1)[0].shape[0] - 1
    g.close()
    ctx.close()
    n_rounds = len(res[0]["rounds"])
    assert n_rounds == len(one), "the ranks ran %d rounds, the one rank %d" % (n_rounds, len(one))
    print("clipping tips over %d ranks (gloo transport, staging through pinned host memory: device work plus host staging, not an interconnect), k=%d, "
          "%d reads over %d bp (%.3g substitutions per base), after retain_counts(2) and prune_edges(1); clip_tips(1, %d); every call timed once, warm"
          % (world, k, n_reads, genome, rate, 2 * k))
    rows = []
    for i in range(n_rounds):
        per = [r["rounds"][i] for r in res]
        total = per[0]["total"]
        for x in per:
            assert x["total"] == total, "the totals differ between ranks in round %d" % (i + 1)
        assert total == one[i]["stats"], "round %d: over ranks %s, one rank %s" % (i + 1, total, one[i]["stats"])
        for f in total:
            assert sum(x["stats"][f] for x in per) == total[f], (i + 1, f)
        nodes = sum(x["nodes"] for x in per)
        sent = sum(x["bytes_sent"] for x in per)
        own = round(sum(v for n, v in per[0]["kernels_ms"].items() if n.startswith("tips_dist_")), 3)
        rows.append(dict(round=i + 1, nodes=nodes, clip_ms_per_rank=[round(x["clip_ms"], 1) for x in per], clip_ms_slowest=round(max(x["clip_ms"] for x in per), 1),
                         tips_dist_kernels_ms_rank0=own, kernels_ms_rank0=per[0]["kernels_ms"], exchanges=per[0]["exchanges"], bytes_exchanged=sent,
                         bytes_per_node=round(sent / max(nodes, 1), 1), stats_total=total, stats_per_rank=[x["stats"] for x in per],
                         pruned_behind=per[0]["pruned_behind"], one_rank_clip_ms=round(one[i]["clip_ms"], 2)))
        print("round %d on %d nodes: kmi_dbg_clip_tips_dist_host %.1f ms on the slowest rank (%s), tips_dist_* kernels of rank 0 %.3f ms, %d exchanges, "
              "%.1f bytes exchanged per node; one-rank kmi_dbg_clip_tips on the same graph %.2f ms; totals = one-rank stats: %s"
              % (i + 1, nodes, rows[-1]["clip_ms_slowest"], rows[-1]["clip_ms_per_rank"], own, rows[-1]["exchanges"], rows[-1]["bytes_per_node"],
                 one[i]["clip_ms"], total), flush=True)
    assert res[0]["unitigs_total"] == one_unitigs, (res[0]["unitigs_total"], one_unitigs)
    summary = dict(ranks=world, k=k, reads=n_reads, genome=genome, rate=rate, rounds=rows, unitigs_total_after=res[0]["unitigs_total"],
                   nodes_after=sum(r["nodes_final"] for r in res), transport="gloo over pinned host staging (not an interconnect)")
    print("unitigs afterwards: %d over the ranks, %d on one rank" % (res[0]["unitigs_total"], one_unitigs))
    print(json.dumps(summary))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


def _bubbles_ranks_worker(rank, world, port, n_reads, genome, k, rate, max_rounds, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        host = _share_reads(rank, world, n_reads, genome, rate)
        g = K.DeBruijnNodes(ctx, K.make_config(k))
        rounds = []
        for run in ("warm-up", "timed"):
            g.clear(); g.build_dist(host, comm)
            g.retain_counts(2)
            g.prune_edges(1, comm=comm)
            for _ in range(max_rounds):   # the end state of --tips --ranks
                g.clip_tips(1, comm=comm)
                g.prune_edges(1, comm=comm)
                if g.clip_totals["n_tips_clipped"] == 0:
                    break
            for r in range(1, (1 if run == "warm-up" else max_rounds) + 1):   # (the warm-up: the workspace and the pool reach their sizes)
                n_before = g.local_size()
                ctx.profile(run == "timed"); ctx.profile_reset()
                dist.barrier()
                t0 = time.perf_counter()
                stats = g.pop_bubbles(1, comm=comm)
                wall = time.perf_counter() - t0
                prof = {p["name"]: round(p["total_ms"], 3) for p in sorted(ctx.profile_get(), key=lambda p: -p["total_ms"]) if p["launches"]}
                ctx.profile(False)
                total = dict(g.pop_totals)
                sent = [ctx.debug_counter(i) for i in (16, 17, 18, 19)]
                g.prune_edges(1, comm=comm)
                if run == "timed":
                    rounds.append(dict(nodes=n_before, pop_ms=wall * 1e3, stats=stats, total=total, kernels_ms=prof, exchanges=sent[0], bytes_sent=sent[1],
                                       stage_exchanges=sent[2], stage_bytes_sent=sent[3],
                                       pruned_behind=g.prune_totals["n_set_before"] - g.prune_totals["n_set_after"]))
                if total["n_popped"] == 0:
                    break
        g.unitigs(1, comm=comm)
        ret[rank] = dict(rounds=rounds, unitigs_total=g.unitig_totals[0], nodes_final=g.local_size())
        g.close()
        comm.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


def main_bubbles_ranks(argv):
    import json
    import socket
    import torch.multiprocessing as mp
    argv = list(argv)
    world = int(argv.pop(0))
    rate = _flag(argv, "--rate", 0.005, float)
    max_rounds = _flag(argv, "--rounds", 8, int)
    out_path = _flag(argv, "--out", None, str)
    n_reads = int(argv[0]) if len(argv) > 0 else 1_000_000
    genome = int(argv[1]) if len(argv) > 1 else 10_000_000
    k = int(argv[2]) if len(argv) > 2 else 31
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ret = mp.Manager().dict()
    mp.spawn(_bubbles_ranks_worker, args=(world, port, n_reads, genome, k, rate, max_rounds, ret), nprocs=world, join=True)
    res = [ret[r] for r in range(world)]
    # the one-rank call on the same graph: the ranks' reads in one buffer, after the ranks' processes have left the GPU
    host = np.concatenate([_share_reads(r, world, n_reads, genome, rate) for r in range(world)])
    ctx = K.Context(0)
    g = K.DeBruijnNodes(ctx, K.make_config(k))
    one = []
    for run in ("warm-up", "timed"):
        g.clear(); g.build(host)
        g.retain_counts(2)
        g.prune_edges(1)
        for _ in range(max_rounds):
            clipped = g.clip_tips(1)["n_tips_clipped"]
            g.prune_edges(1)
            if clipped == 0:
                break
        for r in range(1, (1 if run == "warm-up" else max_rounds) + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats = g.pop_bubbles(1)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            g.prune_edges(1)
            if run == "timed":
                one.append(dict(pop_ms=ms, stats=stats))
            if stats["n_popped"] == 0:
                break
    one_unitigs = g.unitigs(1)[0].shape[0] - 1
    g.close()
    ctx.close()
    n_rounds = len(res[0]["rounds"])
    assert n_rounds == len(one), "the ranks ran %d rounds, the one rank %d" % (n_rounds, len(one))
    print("popping bubbles over %d ranks (gloo transport, staging through pinned host memory: device work plus host staging, not an interconnect), k=%d, "
          "%d reads over %d bp (%.3g substitutions per base), after retain_counts(2), prune_edges(1) and the rounds of clip_tips(1, %d) + prune_edges(1); "
          "pop_bubbles(1, %d); every call timed once, warm" % (world, k, n_reads, genome, rate, 2 * k, 2 * k))
    rows = []
    for i in range(n_rounds):
        per = [r["rounds"][i] for r in res]
        total = per[0]["total"]
        for x in per:
            assert x["total"] == total, "the totals differ between ranks in round %d" % (i + 1)
        assert total == one[i]["stats"], "round %d: over ranks %s, one rank %s" % (i + 1, total, one[i]["stats"])   # every field, every round
        for f in total:
            assert sum(x["stats"][f] for x in per) == total[f], (i + 1, f)
        nodes = sum(x["nodes"] for x in per)
        sent, staged = sum(x["bytes_sent"] for x in per), sum(x["stage_bytes_sent"] for x in per)
        own = round(sum(v for n, v in per[0]["kernels_ms"].items() if n.startswith("bubbles_dist_")), 3)
        every = round(sum(per[0]["kernels_ms"].values()), 3)
        rows.append(dict(round=i + 1, nodes=nodes, pop_ms_per_rank=[round(x["pop_ms"], 1) for x in per], pop_ms_slowest=round(max(x["pop_ms"] for x in per), 1),
                         bubbles_dist_kernels_ms_rank0=own, all_kernels_ms_rank0=every, kernels_ms_rank0=per[0]["kernels_ms"], exchanges=per[0]["exchanges"],
                         stage_exchanges=per[0]["stage_exchanges"], bytes_exchanged=sent, stage_bytes_exchanged=staged,
                         bytes_per_node=round(sent / max(nodes, 1), 1), stage_bytes_per_node=round(staged / max(nodes, 1), 1), stats_total=total,
                         stats_per_rank=[x["stats"] for x in per], pruned_behind=per[0]["pruned_behind"], one_rank_pop_ms=round(one[i]["pop_ms"], 2)))
        x = rows[-1]
        print("round %d on %d nodes: kmi_dbg_pop_bubbles_dist_host %.1f ms on the slowest rank (%s); rank 0: bubbles_dist_* kernels %.3f ms, all kernels %.3f "
              "ms; %d exchanges (%d the stages', %d the call's own), %.1f bytes exchanged per node (%.1f the stages', %.1f the call's own); one-rank "
              "kmi_dbg_pop_bubbles on the same graph %.2f ms; totals = one-rank stats: %s"
              % (i + 1, nodes, x["pop_ms_slowest"], x["pop_ms_per_rank"], own, every, x["exchanges"], x["stage_exchanges"], x["exchanges"] - x["stage_exchanges"],
                 x["bytes_per_node"], x["stage_bytes_per_node"], x["bytes_per_node"] - x["stage_bytes_per_node"], one[i]["pop_ms"], total), flush=True)
    assert res[0]["unitigs_total"] == one_unitigs, (res[0]["unitigs_total"], one_unitigs)
    summary = dict(ranks=world, k=k, reads=n_reads, genome=genome, rate=rate, rounds=rows, unitigs_total_after=res[0]["unitigs_total"],
                   nodes_after=sum(r["nodes_final"] for r in res), transport="gloo over pinned host staging (not an interconnect)")
    print("unitigs afterwards: %d over the ranks, %d on one rank" % (res[0]["unitigs_total"], one_unitigs))
    print(json.dumps(summary))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--clean" and sys.argv[2] == "--ranks":
        return main_clean_ranks(sys.argv[3:])
    if len(sys.argv) > 3 and sys.argv[1] == "--tips" and sys.argv[2] == "--ranks":
        return main_tips_ranks(sys.argv[3:])
    if len(sys.argv) > 3 and sys.argv[1] == "--bubbles" and sys.argv[2] == "--ranks":
        return main_bubbles_ranks(sys.argv[3:])
    if len(sys.argv) > 1 and sys.argv[1] == "--clean":
        return main_clean(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--tips":
        return main_tips(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--bubbles":
        return main_bubbles(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--fasta":
        return main_fasta(sys.argv[2:])
    if len(sys.argv) > 3 and sys.argv[1] == "--unitigs" and sys.argv[2] == "--ranks":
        return main_unitigs_ranks(sys.argv[3:])
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
