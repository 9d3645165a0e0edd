"""Queries after a super-k-mer build: the build files every k-mer in the bucket of the minimizer its rolling walk finds (the one-pass
front end kmi_front.h, the general one sk_minimizer, the FASTA runs), and count / find / erase send a key to the bucket
sk_key_bucket18 (kmi_minimizer.h) computes for it -- a separate restatement of the same walk. to_vector() reads every bucket and
cannot see a key filed in the wrong one; these tests ask for keys one by one, for every k of the super-k-mer build (every W, the
even minimizer lengths with their palindromes, the m >= 16 mask at k = 28, the k = 32 key that equals the empty marker), in the
dense and in the sparse form, against tests/index_model.py."""
import numpy as np
import pytest

from tests import index_model as M
from tests import oracle as orc

pytestmark = pytest.mark.gpu

STRAND = {"single": orc.SINGLE, "canonical": orc.CANONICAL}
KMER_PIPELINE = {"fastq_scatter", "fasta_extract"}   # (the k-mer pipeline's own passes; the general front end scans too)


@pytest.fixture(scope="module")
def ctxs():
    """contexts by (front end, form): KMI_FRONT=general takes the general front end, KMI_SPARSE_MIN=1 leaves every build sparse"""
    import kmerind_amd as K
    out = {}
    for front in ("default", "general"):
        for form in ("dense", "sparse"):
            with pytest.MonkeyPatch.context() as mp:
                if front == "general":
                    mp.setenv("KMI_FRONT", "general")
                if form == "sparse":
                    mp.setenv("KMI_SPARSE_MIN", "1")
                out[front, form] = K.Context(0)
    yield out
    for c in out.values():
        c.close()


def _build_device(ctx, idx, data):
    buf = np.frombuffer(data, dtype=np.uint8)
    d = ctx.alloc(buf.size + 64)
    try:
        ctx.to_device(d, buf)
        idx.build_device(d, buf.size)
    finally:
        ctx.free(d)


def _paths(k):
    paths = [("front", "fastq", "all"), ("general", "fastq", "all"), ("fasta", "fasta", "all")]
    if k in (17, 24, 32):
        paths.append(("n_split", "fastq", "n_split"))
    return paths


@pytest.mark.parametrize("strand", ["single", "canonical"])
@pytest.mark.parametrize("k", list(range(17, 33)))
def test_query_bucket_agrees_with_every_build_path(ctxs, k, strand):
    import kmerind_amd as K
    rng = np.random.default_rng(100 + k)
    s = orc.kspec(k)
    reads = M.adversarial_reads(rng, k) + M.background(rng, 300, genome_len=25_000)
    inputs = {"fastq": M.fastq(reads), "fasta": M.fasta(reads), "n_split": M.fastq(M.with_n_runs(rng, reads, k))}
    models = {}
    for path, fmt, flt in _paths(k):
        data = inputs["n_split" if flt == "n_split" else fmt]
        m = M.CountModel(k, strand=STRAND[strand])
        m.insert(orc.extract(s, data, orc.FASTA if fmt == "fasta" else orc.FASTQ,
                             seq_filter=orc.SEQ_N_SPLIT if flt == "n_split" else orc.SEQ_ALL)["kmers"])
        models[path] = (data, m, M.probes(s, m.export()[0], rng))
    for form in ("dense", "sparse"):
        for path, fmt, flt in _paths(k):
            data, model, q = models[path]
            ctx = ctxs["general" if path == "general" else "default", form]
            idx = K.CountIndex(ctx, K.make_config(k, "DNA", strand=strand, seq_format=fmt, seq_filter=flt))
            ctx.profile(True)
            ctx.profile_reset()
            if fmt == "fasta":
                idx.build(data)
            else:
                _build_device(ctx, idx, data)
            names = {p["name"] for p in ctx.profile_get() if p["launches"]}
            ctx.profile(False)
            want = {"sk_reduce", {"front": "sk_front", "general": "sk_minimizer", "fasta": "fasta_runs", "n_split": "sk_minimizer"}[path]}
            assert want <= names and not (names & KMER_PIPELINE), (path, form, sorted(names))
            if path == "front":
                assert "fastq_scan_tiles" not in names, sorted(names)   # one pass: the front end did not hand the input over
            if path == "general":
                assert "sk_front" not in names, sorted(names)
            where = "k=%d %s %s %s" % (k, strand, path, form)
            if form == "sparse":   # queries on the sparse form first (to_vector makes the index dense)
                d = M.state_difference(idx, model, q, full=False)
                assert d is None, "%s: %s" % (where, d)
            d = M.state_difference(idx, model, q)
            assert d is None, "%s: %s" % (where, d)
            victims = q[rng.permutation(q.shape[0])[: q.shape[0] // 3]]
            after = model.copy()
            assert idx.erase(victims) == after.erase(victims), where
            d = M.state_difference(idx, after, q)
            assert d is None, "%s, after erase: %s" % (where, d)
            idx.close()
