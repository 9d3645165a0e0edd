"""Two count indexes compared and combined on the device against the host route they replace (not the headline metric): two
samples of config 2's shape (k = 31, canonical, coverage 15, `reads` reads each) from two genomes that share half their bases --
half of every sample's reads come from one common genome, half from a genome of the sample's own -- built on the device and left
as the build leaves them (large ones are sparse).
  python tools/setops_bench.py [reads]
Timed (every call warmed once, the device synchronised before the host clock is read):
  (a) kmi_index_compare                      wall time and the bucket_join kernel (mean of 5)
  (b) kmi_index_combine(INTERSECT_MIN / UNION_ADD), each on fresh builds: wall time and kernels
  (c) today's route on the same indexes: to_vector() of a + b.lookup() + the numpy predicate + erase() / update_pairs(assign);
      must reach the same sizes
  (d) a device-to-device copy of the bytes the join must read, 12 per entry of a and of b: the bandwidth yardstick
Default: config 2's size, 10 M reads per sample."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kmerind_amd as K

NAMES = ("bucket_join", "bucket_join_compact", "bucket_offsets", "bucket_merge", "bucket_compact")


def kernels(ctx, per=1):
    return {p["name"]: round(p["total_ms"] / per, 3) for p in ctx.profile_get() if p["name"] in NAMES and p["launches"]}


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    half = n_reads // 2
    glen = half * 10   # coverage 15 on each half genome
    k = 31
    dev = torch.device("cuda", 0)
    common = (K.synth_fastq(seed=20, genome_len=glen, n_reads=half), K.synth_fastq(seed=20, genome_len=glen, n_reads=half, first_read=half))
    samples = []
    for i, own_seed in enumerate((21, 22)):
        host = np.concatenate([np.asarray(common[i]), np.asarray(K.synth_fastq(seed=own_seed, genome_len=glen, n_reads=half))])
        samples.append((torch.from_numpy(host).to(dev), host.size))
    del common
    ctx = K.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    cfg = K.make_config(k, "DNA", strand="canonical")
    a, b = K.CountIndex(ctx, cfg), K.CountIndex(ctx, cfg)

    def build(idx, which):
        idx.clear()
        idx.build_device(samples[which][0].data_ptr(), samples[which][1])
        torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        ctx.profile(True); ctx.profile_reset()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        kk = kernels(ctx)
        ctx.profile(False)
        return r, ms, kk

    build(a, 0); build(b, 1)
    n_a, n_b = a.local_size(), b.local_size()
    print("two count indexes, k=%d canonical, %d reads each over 2 x %d bp (one half common): %d and %d entries" % (k, n_reads, glen, n_a, n_b))

    # ---- (a) compare
    o = a.compare(b)
    steps = 5
    torch.cuda.synchronize()
    ctx.profile(True); ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(steps):
        o = a.compare(b)
    torch.cuda.synchronize()
    cmp_ms = (time.perf_counter() - t0) * 1e3 / steps
    cmp_k = kernels(ctx, steps)
    ctx.profile(False)
    print("(a) kmi_index_compare: %.3f ms wall per call (mean of %d), kernels %s, passes %d" % (cmp_ms, steps, cmp_k, ctx.debug_counter(10)))
    print("    %s" % {w: o[w] for w in ("n_a", "n_b", "n_shared", "sum_a", "sum_b", "sum_min_shared")})
    print("    jaccard %.6f, weighted jaccard %.6f" % (o["jaccard"], o["weighted_jaccard"]))

    # ---- (d) the yardstick: 12 bytes per entry of a and of b, device to device
    src = torch.zeros(3 * (n_a + n_b), dtype=torch.int32, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    copy_ms = e0.elapsed_time(e1) / steps
    del src, dst
    print("(d) device-to-device copy of (%d + %d) x 12 bytes: %.3f ms (mean of %d); bucket_join kernel / copy = %.2f"
          % (n_a, n_b, copy_ms, steps, cmp_k.get("bucket_join", float("nan")) / copy_ms))

    # ---- (b) combine on fresh builds: a warming call, fresh builds again, the timed call
    sizes = {}
    for op in ("intersect_min", "union_add"):
        a.combine(b, op)
        build(a, 0); build(b, 1)
        n, ms, kk = timed(lambda: a.combine(b, op))
        sizes[op] = n
        print("(b) kmi_index_combine(%s): %.3f ms wall, %d entries, kernels %s" % (op, ms, n, kk))
        build(a, 0); build(b, 1)

    # ---- (c) today's route to intersect_min
    t0 = time.perf_counter()
    keys, counts = a.to_vector()
    export_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    cb = b.lookup(keys)
    lookup_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    # (lookup answers 0 for absent keys and for stored zeros alike; a build stores no zero)
    losers = np.ascontiguousarray(keys[cb == 0])
    lower = (cb != 0) & (cb < counts)
    lk, lv = np.ascontiguousarray(keys[lower]), cb[lower]
    pred_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    a.erase(losers)
    a.update_pairs(lk, lv, op="assign")
    apply_ms = (time.perf_counter() - t0) * 1e3
    assert a.local_size() == sizes["intersect_min"], "the two routes disagree on the intersection"
    host_ms = export_ms + lookup_ms + pred_ms + apply_ms
    print("(c) to_vector + lookup + numpy predicate + erase / update_pairs: %.1f + %.1f + %.1f + %.1f = %.1f ms wall"
          % (export_ms, lookup_ms, pred_ms, apply_ms, host_ms))


if __name__ == "__main__":
    main()
