"""What test_gpu_spectrum.py and test_gpu_retain_counts.py share: the two contexts, the built indexes (adversarial, background and
crowded reads, built on the device) with their tests/index_model.CountModel -- computed once per (k, alphabet, strand) and never
changed: the tests work on copies -- and the numpy model of the spectrum. Test-side only."""
import numpy as np

from tests import index_model as M
from tests import oracle as orc

STRAND = {"single": orc.SINGLE, "canonical": orc.CANONICAL}
ALPHA = {"DNA": orc.DNA, "DNA5": orc.DNA5, "DNA16": orc.DNA16}
_CASES = {}


def make_contexts():
    """dense: the default; sparse: KMI_SPARSE_MIN=1 leaves every super-k-mer build sparse"""
    import pytest
    import kmerind_amd as K
    out = {}
    for name, env in (("dense", {}), ("sparse", {"KMI_SPARSE_MIN": "1"})):
        with pytest.MonkeyPatch.context() as mp:
            for key, v in env.items():
                mp.setenv(key, v)
            out[name] = K.Context(0)
    return out


def reads_case(k, alphabet, strand):
    """(FASTQ bytes, k-mer spec, base model, probes) -- shared, read-only"""
    key = (k, alphabet, strand)
    if key not in _CASES:
        rng = np.random.default_rng(7000 + 10 * k + len(alphabet) + len(strand))
        s = orc.kspec(k, ALPHA[alphabet])
        data = M.fastq(M.adversarial_reads(rng, k) + M.background(rng, 300) + M.crowded_reads(rng, copies=3000))
        model = M.CountModel(k, ALPHA[alphabet], STRAND[strand])
        model.insert(orc.extract(s, data, orc.FASTQ)["kmers"])
        stored = model.export()[0]
        if alphabet == "DNA":
            q = M.probes(s, stored, rng)
        else:   # (M.probes' one-base variants flip 2-bit codes)
            pick = stored[rng.integers(0, stored.shape[0], min(1500, stored.shape[0]))]
            q = np.concatenate([pick, orc.revcomp(s, pick[: pick.shape[0] // 2]), orc.kmers_from_string(s, M.random_seq(rng, 300 + s.k - 1)),
                                orc.kmers_from_string(s, b"A" * s.k), orc.kmers_from_string(s, b"T" * s.k)])
        _CASES[key] = (data, s, model, q)
    return _CASES[key]


def build_device(ctx, idx, data):
    buf = np.frombuffer(data, dtype=np.uint8)
    d = ctx.alloc(buf.size + 64)
    try:
        ctx.to_device(d, buf)
        idx.build_device(d, buf.size)
    finally:
        ctx.free(d)


def built_index(ctx, k, alphabet, strand):
    """(index built on the device from the case's reads, a private copy of its model, probes)"""
    import kmerind_amd as K
    data, _s, model, q = reads_case(k, alphabet, strand)
    idx = K.CountIndex(ctx, K.make_config(k, alphabet, strand=strand))
    build_device(ctx, idx, data)
    return idx, model.copy(), q


def spectrum_of_counts(counts, n_bins):
    """(hist, totals) of an array of stored counts: the model of kmi_index_spectrum_*"""
    c = np.asarray(counts, dtype=np.int64)
    hist = np.bincount(np.minimum(c, n_bins - 1), minlength=n_bins).astype(np.uint64)
    totals = {"n_entries": int(c.size), "sum_counts": int(c.sum(dtype=np.uint64)) if c.size else 0,
              "min_count": int(c.min()) if c.size else 0, "max_count": int(c.max()) if c.size else 0}
    return hist, totals


def model_spectrum(model, n_bins):
    return spectrum_of_counts(model.export()[1], n_bins)


def spectrum_device(ctx, idx, n_bins):
    """kmi_index_spectrum_dev into a buffer pre-filled with ones"""
    d = ctx.alloc(8 * n_bins)
    try:
        ctx.to_device(d, np.ones(n_bins, dtype=np.uint64))
        totals = idx.spectrum_device(d, n_bins)
        hist = np.zeros(n_bins, dtype=np.uint64)
        ctx.to_host(hist, d)
        return hist, totals
    finally:
        ctx.free(d)


def assert_spectrum(got, want, where):
    (gh, gt), (wh, wt) = got, want
    assert gh.dtype == np.uint64 and gh.shape == wh.shape, where
    bad = np.nonzero(gh != wh)[0]
    assert bad.size == 0, "%s: %d bins differ; first bin %d: got %d, expected %d" % (where, bad.size, bad[0], gh[bad[0]], wh[bad[0]])
    assert gt == wt, "%s: totals %r, expected %r" % (where, gt, wt)
