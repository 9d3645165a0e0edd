"""Count spectrum and count filter of a count index on the device against the host routes they replace (not the headline metric):
synth_fastq input of config 2's shape (k = 31, canonical, coverage 15: genome = 10 bases per read), built on the device.
  python tools/spectrum_bench.py [reads] [n_bins]
Timed, on indexes as the build leaves them (a large one is sparse):
  kmi_index_spectrum_dev          wall time per call and the count_spectrum kernel (warm, mean of 5)
  kmi_index_retain_counts(2)      wall time of the call and its two kernels, on a fresh build each time (first call, and a second one
                                  that finds the blocks of the first in the context's pool)
  (a) export_host + np.bincount   today's route to the spectrum
  (b) export_host + host predicate + erase_host of the losers: today's erase_if route
  a device-to-device copy of an array of the size of `vals` (4 bytes per entry): the bandwidth yardstick of the spectrum kernel
Default: config 2 itself, 10 M reads."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kmerind_amd as K


def kernels(ctx, names, per=1):
    return {p["name"]: round(p["total_ms"] / per, 3) for p in ctx.profile_get() if p["name"] in names and p["launches"]}


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    n_bins = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    genome = n_reads * 10
    k = 31
    host = np.asarray(K.synth_fastq(seed=2, genome_len=genome, n_reads=n_reads))   # (config 2's seed)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(host).to(dev)
    ctx = K.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    idx = K.CountIndex(ctx, K.make_config(k, "DNA", strand="canonical"))

    def build():
        idx.clear()
        t0 = time.perf_counter()
        idx.build_device(d.data_ptr(), host.size)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    build()
    build_ms = build()
    n = idx.local_size()
    print("count index, k=%d canonical, %d reads over %d bp: %d entries, build %.2f ms (warm)" % (k, n_reads, genome, n, build_ms))

    # ---- spectrum on the device
    hist_d = torch.ones(n_bins, dtype=torch.int64, device=dev)
    idx.spectrum_device(hist_d.data_ptr(), n_bins)
    steps = 5
    ctx.profile(True); ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(steps):
        totals = idx.spectrum_device(hist_d.data_ptr(), n_bins)
    spec_ms = (time.perf_counter() - t0) * 1e3 / steps
    spec_k = kernels(ctx, ("count_spectrum",), steps)
    ctx.profile(False)
    hist_dev = hist_d.cpu().numpy().astype(np.uint64)
    print("kmi_index_spectrum_dev, n_bins=%d: %.3f ms wall per call (mean of %d), kernels %s" % (n_bins, spec_ms, steps, spec_k))
    print("  bins 0..7 %s, totals %s" % (hist_dev[:8].tolist(), totals))

    # ---- the yardstick: 4 bytes per entry, device to device
    a = torch.zeros(n, dtype=torch.int32, device=dev)
    b = torch.empty_like(a)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    copy_ms = e0.elapsed_time(e1) / steps
    del a, b
    ratio = spec_k.get("count_spectrum", float("nan")) / copy_ms
    print("device-to-device copy of %d x 4 bytes: %.3f ms (mean of %d); count_spectrum kernel / copy = %.2f" % (n, copy_ms, steps, ratio))

    # ---- the filter on the device: fresh builds, first and second call
    names = ("bucket_retain_count", "bucket_retain_compact", "bucket_offsets")
    for which in ("first call", "second call"):
        if which == "second call":
            build()
        ctx.profile(True); ctx.profile_reset()
        t0 = time.perf_counter()
        erased = idx.retain_counts(2)
        retain_ms = (time.perf_counter() - t0) * 1e3
        rk = kernels(ctx, names)
        ctx.profile(False)
        print("kmi_index_retain_counts(2), %s: %.3f ms wall, %d of %d entries erased, %d left, fullest bucket %d, kernels %s (sum %.3f ms)"
              % (which, retain_ms, erased, n, idx.local_size(), ctx.debug_counter(9), rk,
                 sum(v for key, v in rk.items() if key != "bucket_offsets")))
    kept_dev = idx.local_size()

    # ---- today's routes, on a fresh build
    build()
    t0 = time.perf_counter()
    keys, counts = idx.to_vector()
    export_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    hist_host = np.bincount(np.minimum(counts, n_bins - 1), minlength=n_bins).astype(np.uint64)
    binc_ms = (time.perf_counter() - t0) * 1e3
    assert (hist_host == hist_dev).all(), "the two routes disagree on the spectrum"
    print("(a) export_host + np.bincount: %.1f + %.1f = %.1f ms wall" % (export_ms, binc_ms, export_ms + binc_ms))
    t0 = time.perf_counter()
    losers = np.ascontiguousarray(keys[counts < 2])
    pred_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    gone = idx.erase(losers)
    erase_ms = (time.perf_counter() - t0) * 1e3
    assert gone == erased and idx.local_size() == kept_dev, "the two routes disagree on the filter"
    print("(b) export_host + host predicate + erase_host: %.1f + %.1f + %.1f = %.1f ms wall" % (export_ms, pred_ms, erase_ms, export_ms + pred_ms + erase_ms))
    print("spectrum: device %.3f ms against %.1f ms; filter: device %.3f ms against %.1f ms" % (spec_ms, export_ms + binc_ms, retain_ms, export_ms + pred_ms + erase_ms))


if __name__ == "__main__":
    main()
