"""A count index is a state machine -- layout (placement hash or minimizer bucket), form (dense or sparse), merge (adopt the build's
output or add a scratch index's pairs) and the context's shared workspace slots -- and most of its logic lives in the transitions.
These tests run operation sequences and check the whole state after every step against tests/index_model.py: local_size,
to_vector, and count / find / exists on a probe set (to_vector alone cannot see a key filed in the wrong bucket).
(a) a table of scripted sequences, each naming one transition and asserting through the profile that it happened;
(b) seeded random sequences over two count indexes and a de Bruijn node map on one context, with inputs that grow."""
import numpy as np
import pytest

from tests import index_model as M
from tests import oracle as orc

pytestmark = pytest.mark.gpu

STRAND = {"single": orc.SINGLE, "canonical": orc.CANONICAL}


@pytest.fixture(scope="module")
def ctxs():
    """a context per form: KMI_SPARSE_MIN=1 leaves every super-k-mer build sparse"""
    import kmerind_amd as K
    out = {}
    for form in ("dense", "sparse"):
        with pytest.MonkeyPatch.context() as mp:
            if form == "sparse":
                mp.setenv("KMI_SPARSE_MIN", "1")
            out[form] = K.Context(0)
    yield out
    for c in out.values():
        c.close()


class Log:
    """the operations so far, for failure messages"""

    def __init__(self, seed):
        self.seed, self.ops = seed, []

    def __str__(self):
        return "seed %s, operations: %s" % (self.seed, " -> ".join(self.ops))


class CountSeq:
    """a CountIndex and its model, driven step by step"""

    def __init__(self, ctx, k, strand, log, name="A", saturating=False):
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        self.K, self.L, self.ctx, self.k, self.log, self.name = K, L, ctx, k, log, name
        self.s = orc.kspec(k)
        self.idx = K.CountIndex(ctx, K.make_config(k, "DNA", strand=strand))
        if saturating:
            ctx.check(L.lib.kmi_index_set_saturating(self.idx.h, 1))
        self.model = M.CountModel(k, strand=STRAND[strand], saturating=saturating)
        self.rng = np.random.default_rng(k)

    def close(self):
        self.idx.close()

    def step(self, op, *args, full=True):
        """run one operation on both sides -> {kernel name: launches} of the library's side; then compare the whole state (full =
        False: the queries only, which leave a sparse index sparse)"""
        self.ctx.profile(True)
        self.ctx.profile_reset()
        ret = getattr(self, "_" + op)(*args)
        prof = {p["name"]: p["launches"] for p in self.ctx.profile_get() if p["launches"]}
        self.ctx.profile(False)
        self.log.ops.append("%s.%s" % (self.name, op))
        if ret is not None:
            assert ret[0] == ret[1], "%s returned %s, expected %s (%s)" % (op, ret[0], ret[1], self.log)
        self.check(full)
        return prof

    def check(self, full=True):
        q = M.probes(self.s, self.model.export()[0], self.rng, n_stored=800, n_absent=100)
        d = M.state_difference(self.idx, self.model, q, full)
        assert d is None, "index %s (k=%d): %s (%s)" % (self.name, self.k, d, self.log)

    def _kmers(self, data, fmt=orc.FASTQ):
        return orc.extract(self.s, data, fmt)["kmers"]

    def _build(self, data):
        self.idx.build(data)
        self.model.insert(self._kmers(data))

    def _build_device(self, data):
        buf = np.frombuffer(data, dtype=np.uint8)
        d = self.ctx.alloc(buf.size + 64)
        try:
            self.ctx.to_device(d, buf)
            self.idx.build_device(d, buf.size)
        finally:
            self.ctx.free(d)
        self.model.insert(self._kmers(data))

    def _build_fasta(self, data):
        L = self.L
        self.ctx.check(L.lib.kmi_index_set_seq_format(self.idx.h, L.FMT_FASTA))
        try:
            self.idx.build(data)
        finally:
            self.ctx.check(L.lib.kmi_index_set_seq_format(self.idx.h, L.FMT_FASTQ))
        self.model.insert(self._kmers(data, orc.FASTA))

    def _insert(self, kmers):
        self.idx.insert(kmers)
        self.model.insert(kmers)

    def _insert_pairs(self, kmers, counts):
        self.idx.insert_pairs(kmers, counts)
        self.model.insert_pairs(kmers, counts)

    def _update(self, kmers, values, op):
        return self.idx.update_pairs(kmers, values, op), self.model.update_pairs(kmers, values, op)

    def _erase(self, q):
        return self.idx.erase(q), self.model.erase(q)

    def _clear(self):
        self.idx.clear()
        self.model.clear()

    def _query(self):
        pass

    # inputs drawn for this index
    def stored_sample(self, n):
        keys = self.model.export()[0]
        return keys[self.rng.integers(0, keys.shape[0], n)] if keys.shape[0] else keys

    def query_keys(self, n):
        """stored keys (either strand) and keys that are not stored"""
        st = self.stored_sample(n)
        return np.concatenate([st, orc.revcomp(self.s, st[: n // 3]), orc.kmers_from_string(self.s, M.random_seq(self.rng, n // 4 + self.k))])


class NodeSeq:
    """a DeBruijnNodes map and its model"""

    def __init__(self, ctx, k, log, name="G"):
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        self.K, self.L, self.ctx, self.k, self.log, self.name = K, L, ctx, k, log, name
        self.s = orc.kspec(k)
        self.g = K.DeBruijnNodes(ctx, K.make_config(k, "DNA"))
        self.model = M.NodeModel(k)
        self.rng = np.random.default_rng(k + 1)

    def close(self):
        self.g.close()

    def step(self, op, *args):
        self.ctx.profile(True)
        self.ctx.profile_reset()
        ret = getattr(self, "_" + op)(*args)
        prof = {p["name"]: p["launches"] for p in self.ctx.profile_get() if p["launches"]}
        self.ctx.profile(False)
        self.log.ops.append("%s.%s" % (self.name, op))
        if ret is not None:
            assert ret[0] == ret[1], "%s returned %s, expected %s (%s)" % (op, ret[0], ret[1], self.log)
        keys = self.model.export()[0]
        q = M.probes(self.s, keys, self.rng, n_stored=600, n_absent=100)
        d = M.node_state_difference(self.g, self.model, q)
        assert d is None, "node map %s (k=%d): %s (%s)" % (self.name, self.k, d, self.log)
        return prof

    def _build(self, data):
        self.g.build(data)
        self.model.build(data)

    def _build_fasta(self, data):
        L = self.L
        self.ctx.check(L.lib.kmi_dbg_set_seq_format(self.g.h, L.FMT_FASTA))
        try:
            self.g.build(data)
        finally:
            self.ctx.check(L.lib.kmi_dbg_set_seq_format(self.g.h, L.FMT_FASTQ))
        self.model.build(data, orc.FASTA)

    def _insert(self, data):
        kmers, edges = orc.dbg_parse(self.s, data)
        self.g.insert(kmers, edges)
        self.model.insert(kmers, edges)

    def _erase(self, q):
        return self.g.erase(q), self.model.erase(q)

    def _query(self):
        pass


GENOME = M.random_seq(np.random.default_rng(12345), 30_000)


def _reads(rng, n, genome_len=None):
    """reads of one shared genome (later batches meet the keys of earlier ones), or of a fresh one of genome_len bases"""
    return M.background(rng, n, genome=None if genome_len else GENOME, genome_len=genome_len or 0)


# ---- (a) scripted transitions
def row_insert_then_build(c, rng, ctx):
    """k-mers first (placement layout), then a build merges into them through a scratch index"""
    c.step("insert", c._kmers(M.fastq(_reads(rng, 80))))
    assert "sk_reduce" in c.step("build", M.fastq(_reads(rng, 200) + M.adversarial_reads(rng, c.k)))


def row_build_insert_build_update_erase(c, rng, ctx):
    """build -> insert (relayout to the placement hash) -> build -> update -> erase -> query"""
    assert "sk_reduce" in c.step("build", M.fastq(_reads(rng, 200) + M.adversarial_reads(rng, c.k)))
    p = c.step("insert", c._kmers(M.fastq(_reads(rng, 60))))
    assert {"zip_pairs", "unzip_pairs"} <= set(p), p
    assert "sk_reduce" in c.step("build", M.fastq(_reads(rng, 300)))
    q = c.query_keys(2000)
    c.step("update", q, rng.integers(0, 1000, q.shape[0]), "max")
    c.step("erase", c.query_keys(1500))
    c.step("query")


def row_erase_all_then_build(c, rng, ctx):
    """an index that has_data with 0 entries takes the adopt branch of the build"""
    c.step("build", M.fastq(_reads(rng, 200)))
    c.step("erase", c.model.export()[0])
    assert c.model.size() == 0
    assert "sk_reduce" in c.step("build", M.fastq(_reads(rng, 300) + M.adversarial_reads(rng, c.k)))
    c.step("insert", c._kmers(M.fastq(_reads(rng, 50))))


def row_erase_all_then_insert(c, rng, ctx):
    """erased to empty after a super-k-mer build, then k-mers: they are filed by the placement hash and must be asked for by it"""
    c.step("build", M.fastq(_reads(rng, 200)))
    c.step("erase", c.model.export()[0])
    c.step("insert", c._kmers(M.fastq(_reads(rng, 100))))
    c.step("query")


def row_room_on_the_adopt_path(c, rng, ctx):
    """erased to empty, then builds of >= 4096 records: fine buckets with room (no sk_fine_count, one sk_scatter_fine), and
    one read copied 3000 times, which outgrows its room and repeats the back end counted (sk_fine_count, a second scatter)"""
    c.step("build", M.fastq(_reads(rng, 100)))
    c.step("erase", c.model.export()[0])
    p = c.step("build", M.fastq(_reads(rng, 3000, genome_len=200_000)))
    assert "sk_fine_count" not in p and p.get("sk_scatter_fine") == 1, p
    c.step("erase", c.model.export()[0])
    p = c.step("build", M.fastq(_reads(rng, 1000, genome_len=200_000) + M.crowded_reads(rng, 3000)))
    assert "sk_fine_count" in p and p.get("sk_scatter_fine") == 2, p


def row_sparse_update(c, rng, ctx):
    """update, count and erase on a sparse minimizer-layout index"""
    p = c.step("build", M.fastq(_reads(rng, 300) + M.adversarial_reads(rng, c.k)), full=False)
    assert "sk_reduce" in p and "bucket_compact" not in p, p
    q = c.query_keys(2000)
    c.step("update", q, rng.integers(0, 1000, q.shape[0]), "add", full=False)
    c.step("query")
    c.step("build", M.fastq(_reads(rng, 100)), full=False)
    c.step("erase", c.query_keys(500))


def row_clear_then_build(c, rng, ctx):
    c.step("build", M.fastq(_reads(rng, 200)))
    c.step("insert", c._kmers(M.fastq(_reads(rng, 30))))
    c.step("clear")
    c.step("build", M.fastq(_reads(rng, 250) + M.adversarial_reads(rng, c.k)))


def row_saturating_merge(c, rng, ctx):
    """a saturating index: pairs at the ceiling, then builds whose counts go through a scratch merge onto them"""
    data = M.fastq(_reads(rng, 200, genome_len=5_000))
    top = c._kmers(data)[::7]
    c.step("insert_pairs", top, np.full(top.shape[0], M.MASK32 - 40, dtype=np.uint64))
    c.step("build", data)
    c.step("build", data)
    assert max(c.model.d.values()) == M.MASK32


def row_fastq_then_fasta(c, rng, ctx):
    reads = _reads(rng, 200) + M.adversarial_reads(rng, c.k)
    c.step("build", M.fastq(reads))
    assert "fasta_runs" in c.step("build_fasta", M.fasta(_reads(rng, 150) + reads[:20]))
    c.step("build", M.fastq(_reads(rng, 100)))


def row_host_and_device_builds(c, rng, ctx):
    c.step("build", M.fastq(_reads(rng, 150)))
    c.step("build_device", M.fastq(_reads(rng, 300) + M.adversarial_reads(rng, c.k)))
    c.step("build", M.fastq(_reads(rng, 600)))


def row_two_indexes(c, rng, ctx):
    """two indexes (other k, other strand) interleaved on one context: one's conversions must not touch the other's state"""
    k2 = 22 if c.k != 22 else 31
    other = CountSeq(ctx, k2, "single" if c.model.strand == orc.CANONICAL else "canonical", c.log, "B")
    try:
        c.step("build", M.fastq(_reads(rng, 100)))
        other.step("build", M.fastq(_reads(rng, 150)))
        c.step("insert", c._kmers(M.fastq(_reads(rng, 200))))
        other.step("erase", other.query_keys(600))
        c.step("build", M.fastq(_reads(rng, 500)))
        other.step("insert", other._kmers(M.fastq(_reads(rng, 400))))
        c.check()
        other.check()
    finally:
        other.close()


ROWS = [row_insert_then_build, row_build_insert_build_update_erase, row_erase_all_then_build, row_erase_all_then_insert,
        row_room_on_the_adopt_path, row_sparse_update, row_clear_then_build, row_saturating_merge, row_fastq_then_fasta,
        row_host_and_device_builds, row_two_indexes]


@pytest.mark.parametrize("k,strand", [(31, "canonical"), (28, "single")])
@pytest.mark.parametrize("row", ROWS, ids=[r.__name__[4:] for r in ROWS])
def test_transition(ctxs, row, k, strand):
    ctx = ctxs["sparse" if row is row_sparse_update else "dense"]
    rng = np.random.default_rng(k)
    c = CountSeq(ctx, k, strand, Log("%s k=%d" % (row.__name__, k)), saturating=row is row_saturating_merge)
    try:
        row(c, rng, ctx)
    finally:
        c.close()


def test_node_map_relayout_carries_edge_counts(ctxs):
    """a graph built through super-k-mers, then tuples: the nodes change to the placement layout and their counts and edge
    counters -- past 16 bits on the poly-A node -- must follow them; then erase and another build"""
    ctx = ctxs["dense"]
    rng = np.random.default_rng(3)
    g = NodeSeq(ctx, 31, Log("node map"))
    try:
        assert "sk_edges_accumulate" in g.step("build", M.fastq(_reads(rng, 300) + M.poly_reads(b"A", 620)))
        assert "dbg_follow" in g.step("insert", M.fastq(_reads(rng, 200)))
        assert int(g.model.export()[1].max()) > 0xFFFF
        g.step("erase", np.concatenate([g.model.export()[0][::5], orc.kmers_from_string(g.s, b"A" * 31)]))
        g.step("build_fasta", M.fasta(_reads(rng, 100)))
    finally:
        g.close()


# ---- (b) seeded random sequences
K2 = {17: 31, 20: 28, 22: 32, 28: 20, 31: 17, 32: 22, 40: 31}
COUNT_OPS = ["build", "build_device", "build_fasta", "insert", "insert_pairs", "update", "erase", "erase_all", "clear", "query"]
NODE_OPS = ["build", "build_fasta", "insert", "erase", "query"]


def _count_op(c, rng, op, n_reads):
    reads = _reads(rng, n_reads) + (M.adversarial_reads(rng, c.k) if rng.integers(0, 2) else [])
    if op == "build":
        c.step("build", M.fastq(reads))
    elif op == "build_device":
        c.step("build_device", M.fastq(reads) + (bytes(c.K.synth_fastq(seed=int(rng.integers(1 << 30)), genome_len=20_000, n_reads=n_reads))))
    elif op == "build_fasta":
        c.step("build_fasta", M.fasta(reads))
    elif op == "insert":
        c.step("insert", np.concatenate([c._kmers(M.fastq(reads[: max(1, n_reads // 2)])), c.stored_sample(n_reads)]))
    elif op == "insert_pairs":
        q = np.concatenate([c._kmers(M.fastq(reads[: max(1, n_reads // 4)])), c.stored_sample(n_reads)])
        cnt = rng.integers(1, 6, q.shape[0]).astype(np.uint64)
        cnt[rng.random(q.shape[0]) < 0.02] = M.MASK32 - 2    # counts that wrap
        c.step("insert_pairs", q, cnt)
    elif op == "update":
        q = c.query_keys(20 * n_reads)
        c.step("update", q, rng.integers(0, 1 << 20, q.shape[0]), ["add", "max", "min", "assign"][int(rng.integers(0, 4))])
    elif op == "erase":
        c.step("erase", c.query_keys(10 * n_reads))
    elif op == "erase_all":
        c.step("erase", c.model.export()[0])
    else:
        c.step(op)


def _node_op(g, rng, op, n_reads):
    reads = _reads(rng, n_reads)
    if op == "build":
        g.step("build", M.fastq(reads))
    elif op == "build_fasta":
        g.step("build_fasta", M.fasta(reads))
    elif op == "insert":
        g.step("insert", M.fastq(reads))
    elif op == "erase":
        keys = g.model.export()[0]
        g.step("erase", np.concatenate([keys[rng.integers(0, keys.shape[0], max(1, keys.shape[0] // 3))] if keys.shape[0] else keys,
                                        orc.kmers_from_string(g.s, M.random_seq(rng, 50 + g.k))]))
    else:
        g.step(op)


SEQUENCES = [(k, strand, form, seed) for k in (17, 20, 22, 28, 31, 32) for strand in ("single", "canonical")
             for form in ("dense", "sparse") for seed in (0, 1)] + [(40, strand, "dense", 0) for strand in ("single", "canonical")]


@pytest.mark.parametrize("k,strand,form,seed", SEQUENCES)
def test_random_sequence(ctxs, k, strand, form, seed):
    """about a dozen operations over two count indexes and a node map on one context; inputs grow 8 x along the sequence, so
    workspace slots are reallocated in the middle of it. k = 40 (two words, never sparse) is the k-mer pipeline's control."""
    ctx = ctxs[form]
    rng = np.random.default_rng(1000 * k + 10 * seed + (strand == "single") + 2 * (form == "sparse"))
    log = Log("%d (k=%d %s %s)" % (seed, k, strand, form))
    a = CountSeq(ctx, k, strand, log, "A")
    b = CountSeq(ctx, K2[k], "single" if strand == "canonical" else "canonical", log, "B")
    g = NodeSeq(ctx, k, log, "G")
    try:
        order = ["A"] * 6 + ["B"] * 3 + ["G"] * 4
        rng.shuffle(order)
        done = {"A": 0, "B": 0, "G": 0}
        for i, who in enumerate(order):
            n_reads = 40 << (4 * i // len(order))                       # 40, 80, 160, 320 reads along the sequence
            if who == "G":
                op = "build" if done["G"] == 0 else ("insert" if done["G"] == 1 else NODE_OPS[int(rng.integers(0, len(NODE_OPS)))])
                if done["G"] == 0:   # poly-A: the edge counters of one node pass 16 bits before the relayout that follows
                    g.step("build", M.fastq(_reads(rng, n_reads) + M.poly_reads(b"A", 620)))
                else:
                    _node_op(g, rng, op, n_reads)
            else:
                c = a if who == "A" else b
                op = ["build", "build_device", "build_fasta"][int(rng.integers(0, 3))] if done[who] == 0 else \
                    COUNT_OPS[int(rng.integers(0, len(COUNT_OPS)))]
                _count_op(c, rng, op, n_reads)
            done[who] += 1
        a.check()
        b.check()
    finally:
        a.close(); b.close(); g.close()
