"""Queries in read order on config 2's input (10 M synthetic 150-base reads of a 100 Mbp genome, k = 31, canonical): one JSON line each for

  profile_reads   CountIndex.profile_reads_device of the reads the index was built from (every k-mer of 10 M reads)
  lookup          CountIndex.lookup_device of the first 1e8 extracted k-mers
  composed        the only route to the same per-k-mer counts without these calls: kmi_extract_dev + kmi_index_find_dev (one
                  row per distinct key, unordered) + a join back to the occurrences in torch on the device (canonical form of
                  every k-mer, sort of the find result, torch.searchsorted); its answer is compared with lookup's

Times are host clocks around calls that end in a stream synchronise, after one warm-up call, the median of --reps; the per-kernel
times come from a further call under kmi_profile_get. Writes the lines to --out (profiles/) and prints them.

  python tools/profile_bench.py [--reads 10000000] [--genome 100000000] [--queries 100000000] [--reps 3] [--out profiles/NAME.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def _lsr(x, n):
    return (x >> n) & ((1 << (64 - n)) - 1)


def canonical31(x, k):
    """min(k-mer, reverse complement) of one-word 2-bit k-mers held in int64 (first base in the highest bits, k < 32)"""
    import torch
    y = ~x
    for sh, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        y = (_lsr(y, sh) & m) | ((y & m) << sh)
    y = _lsr(y, 32) | (y << 32)
    y = _lsr(y, 64 - 2 * k)
    return torch.minimum(x, y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--queries", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("profile_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    k, read_len = 31, 150
    per_read = read_len - k + 1
    stream = torch.cuda.current_stream(dev)
    ctx = K.Context(device=0, stream=stream.cuda_stream)
    cfg = K.make_config(k, "DNA", strand="canonical")
    host = K.synth_fastq(2, args.genome, args.reads, read_len)
    nbytes = int(host.nbytes)
    d_bytes = torch.from_numpy(host).to(dev)
    idx = K.CountIndex(ctx, cfg)
    idx.build_device(d_bytes.data_ptr(), nbytes)
    torch.cuda.synchronize(dev)
    n_kmers = args.reads * per_read
    workload = "k=%d canonical, %d synthetic %d-base reads of a %d bp genome (seed 2), %d distinct k-mers in the index" % (
        k, args.reads, read_len, args.genome, idx.local_size())

    def timed(fn):
        fn()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) * 1e3)
        ctx.profile(True)
        ctx.profile_reset()
        fn()
        torch.cuda.synchronize(dev)
        kern = {p["name"]: round(p["total_ms"], 3) for p in ctx.profile_get() if p["launches"]}
        ctx.profile(False)
        return float(np.median(ts)), [round(t, 3) for t in ts], kern

    lines = []

    # 1. the profile of every read
    rows = torch.empty((args.reads + 1, 5), dtype=torch.int64, device=dev)   # 40 bytes per row
    n_rows = [0]

    def profile():
        n_rows[0] = idx.profile_reads_device(d_bytes.data_ptr(), nbytes, rows.data_ptr(), args.reads + 1, 2)
    ms, all_ms, kern = timed(profile)
    assert n_rows[0] == args.reads
    r = rows[:args.reads]
    n_k, n_present = (r[:, 2] & 0xFFFFFFFF), (r[:, 2] >> 32) & 0xFFFFFFFF
    assert int(n_k.sum()) == n_kmers and bool((n_k == n_present).all()), "reads profiled against their own index hold all their k-mers"
    lines.append({"what": "profile_reads_device", "workload": workload, "reads": args.reads, "kmers": n_kmers, "input_bytes": nbytes,
                  "ms": round(ms, 3), "runs_ms": all_ms, "G_kmers_per_s": round(n_kmers / ms / 1e6, 2), "GB_per_s": round(nbytes / ms / 1e6, 2),
                  "passes_of_fullest_bucket": ctx.debug_counter(8), "kernels_ms": kern})
    del rows, r

    # the queries: the k-mers of the first reads, as parsed
    n_sub_reads = min(args.reads, (args.queries + per_read - 1) // per_read)
    nq = n_sub_reads * per_read
    sub_bytes = n_sub_reads * (nbytes // args.reads)
    d_q = torch.empty((nq + 64, 1), dtype=torch.int64, device=dev)
    nt, ns = C.c_uint64(), C.c_uint64()

    def extract():
        ctx.check(L.lib.kmi_extract_dev(ctx.h, C.byref(cfg), C.c_void_p(d_bytes.data_ptr()), sub_bytes, 0, C.c_void_p(d_q.data_ptr()), None, nq,
                                        C.byref(nt), C.byref(ns)))
    extract()
    assert nt.value == nq

    # 2. the lookup
    d_counts = torch.empty(nq, dtype=torch.int32, device=dev)

    def lookup():
        idx.lookup_device(d_q.data_ptr(), nq, d_counts.data_ptr())
    ms, all_ms, kern = timed(lookup)
    lines.append({"what": "lookup_device", "workload": workload, "queries": nq, "ms": round(ms, 3), "runs_ms": all_ms,
                  "G_queries_per_s": round(nq / ms / 1e6, 2), "passes_of_fullest_bucket": ctx.debug_counter(8), "kernels_ms": kern})

    # 3. the composed route: extract + find + join
    ok = torch.empty((nq, 1), dtype=torch.int64, device=dev)
    ov = torch.empty(nq, dtype=torch.int64, device=dev)
    n_out = C.c_uint64()
    joined = [None]

    def composed():
        extract()
        ctx.check(L.lib.kmi_index_find_dev(idx.h, C.c_void_p(d_q.data_ptr()), nq, C.c_void_p(ok.data_ptr()), C.c_void_p(ov.data_ptr()), C.byref(n_out)))
        keys, order = torch.sort(ok[:n_out.value, 0])
        vals = ov[:n_out.value][order]
        want = canonical31(d_q[:nq, 0], k)
        pos = torch.searchsorted(keys, want).clamp_(max=keys.numel() - 1)
        joined[0] = torch.where(keys[pos] == want, vals[pos], torch.zeros_like(want))
    ms_c, all_c, kern_c = timed(composed)
    ms_e, all_e, _ = timed(extract)
    same = bool((joined[0] == d_counts.to(torch.int64)).all())
    lines.append({"what": "kmi_extract_dev + kmi_index_find_dev + torch.sort / torch.searchsorted join", "workload": workload, "queries": nq,
                  "ms": round(ms_c, 3), "runs_ms": all_c, "of_which_extract_ms": round(ms_e, 3), "G_queries_per_s": round(nq / ms_c / 1e6, 2),
                  "distinct_keys_found": n_out.value, "equals_lookup_device": same, "kernels_ms": kern_c,
                  "lookup_device_plus_extract_ms": round(lines[1]["ms"] + ms_e, 3)})
    assert same, "the composed route and lookup_device disagree"

    text = "\n".join(json.dumps(ln) for ln in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    idx.close()
    ctx.close()


if __name__ == "__main__":
    main()
