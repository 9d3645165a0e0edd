"""kmi_index_locate_*: the occurrences of every query of a position / position + quality index, in query order, against
tests/locate_model.py -- one to three key words, one and two value words, FASTQ and FASTA builds on the device, duplicates, both
strands, absent keys, a cap that some keys exceed and others meet, buckets that need several passes, a key with 150 000 values
(at k = 32 the table's empty marker), and the edges of the interface. occ and offsets are compared exactly, values per query as
sorted rows."""
import ctypes as C

import numpy as np
import pytest

from tests import index_model as M
from tests import locate_model as LM
from tests import multimap_cases as MC
from tests import oracle as orc

pytestmark = pytest.mark.gpu

STRAND = {"single": orc.SINGLE, "canonical": orc.CANONICAL}
GUARD = 64                              # words behind a device buffer that a call must leave alone
PATTERN = 0xA5A5A5A5DEADBEEF
PATTERN32 = 0xDEADBEEF


@pytest.fixture(scope="module")
def ctxs():
    """default: the tables' own sizes; small: tables of 64 home slots (KMI_LOOKUP_CAP), so that ordinary buckets need passes"""
    import kmerind_amd as K
    out = {}
    for name, env in (("default", {}), ("small", {"KMI_LOOKUP_CAP": "64"})):
        with pytest.MonkeyPatch.context() as mp:
            for key, v in env.items():
                mp.setenv(key, v)
            out[name] = K.Context(0)
    yield out
    for c in out.values():
        c.close()


def make_index(ctx, k, alpha, strand, kind, fmt="fastq"):
    import kmerind_amd as K
    s = orc.kspec(k, MC.ALPHA[alpha])
    vw = MC.VW[kind]
    idx = K.PositionIndex(ctx, K.make_config(k, alpha, strand=strand, index_kind=kind, seq_format=fmt))
    return s, vw, idx, LM.LocateModel(s, STRAND[strand], vw)


def build_device(ctx, idx, data):
    buf = np.frombuffer(data, dtype=np.uint8)
    d = ctx.alloc(buf.size + 64)
    try:
        ctx.to_device(d, buf)
        idx.build_device(d, buf.size)
    finally:
        ctx.free(d)


def locate_raw(ctx, idx, q, max_occ, capacity, with_values=True):
    """kmi_index_locate_dev into device buffers of exactly nq / nq + 1 / capacity * vw words, each followed by GUARD words of a
    pattern (the value buffer is the pattern throughout) -> (status, n_hits, occ, offsets, values, guards intact)"""
    from kmerind_amd import _lib as L
    q = np.ascontiguousarray(q, dtype=np.uint64).reshape(-1, idx.n_words)
    nq, vw = q.shape[0], idx.value_words
    h_occ = np.full(nq + GUARD, PATTERN32, dtype=np.uint32)
    h_off = np.full(nq + 1 + GUARD, PATTERN, dtype=np.uint64)
    h_val = np.full(capacity * vw + GUARD, PATTERN, dtype=np.uint64)
    dq, d_occ, d_off, d_val = ctx.alloc(max(q.nbytes, 8)), ctx.alloc(h_occ.nbytes), ctx.alloc(h_off.nbytes), ctx.alloc(h_val.nbytes)
    try:
        if nq:
            ctx.to_device(dq, q)
        ctx.to_device(d_occ, h_occ)
        ctx.to_device(d_off, h_off)
        ctx.to_device(d_val, h_val)
        n = C.c_uint64(12345)
        st = L.lib.kmi_index_locate_dev(idx.h, C.c_void_p(dq), nq, max_occ, C.c_void_p(d_occ), C.c_void_p(d_off),
                                        C.c_void_p(d_val) if with_values else None, capacity if with_values else 0, C.byref(n))
        ctx.to_host(h_occ, d_occ)
        ctx.to_host(h_off, d_off)
        ctx.to_host(h_val, d_val)
    finally:
        for p in (dq, d_occ, d_off, d_val):
            ctx.free(p)
    intact = bool((h_occ[nq:] == PATTERN32).all() and (h_off[nq + 1:] == np.uint64(PATTERN)).all() and
                  (h_val[capacity * vw:] == np.uint64(PATTERN)).all())
    return st, n.value, h_occ[:nq], h_off[:nq + 1], h_val[:capacity * vw].reshape(capacity, vw), intact


def locate_device(ctx, idx, q, max_occ):
    """the sizing call, then the call into a value buffer of exactly n_hits rows"""
    from kmerind_amd import _lib as L
    st, n, occ0, off0, _, intact = locate_raw(ctx, idx, q, max_occ, 0, with_values=False)
    assert st == L.OK and intact
    st, n2, occ, off, values, intact = locate_raw(ctx, idx, q, max_occ, n)
    assert st == L.OK and intact and n2 == n
    assert (occ == occ0).all() and (off == off0).all()          # the sizing call leaves occ and offsets complete
    return occ, off, values


def stored_keys(model):
    return np.array(sorted(model.d), dtype=np.uint64).reshape(-1, model.s.n_words)


def cap_from(model):
    """a max_occ that some stored keys exceed and others meet exactly, and three keys of each kind"""
    mult = {key: len(v) for key, v in model.d.items()}
    levels = sorted(set(mult.values()))
    assert len(levels) >= 3
    cap = levels[len(levels) // 2]
    at = [key for key, m in sorted(mult.items()) if m == cap][:3]
    above = [key for key, m in sorted(mult.items()) if m > cap][:3]
    assert at and above
    return cap, np.array(at + above, dtype=np.uint64).reshape(-1, model.s.n_words)


# ---- model parity
# (a position + quality index reads FASTQ only)
BUILDS = [(k, alpha, kind, fmt) for k, alpha, kind in MC.PASS_SHAPES for fmt in ("fastq", "fasta") if not (kind == "posqual" and fmt == "fasta")]


@pytest.mark.parametrize("k,alpha,kind,fmt", BUILDS)
def test_locate_matches_the_model(ctxs, k, alpha, kind, fmt):
    """indexes built on the device from reads of both strands of a 3000-base genome, so that keys repeat; queries: stored keys,
    their reverse complements, absent k-mers, the all-A and all-T k-mers, every probe twice, shuffled; device and host forms; no
    cap, and a cap that some keys exceed and others meet"""
    ctx = ctxs["default"]
    s, vw, idx, model = make_index(ctx, k, alpha, "canonical", kind, fmt)
    rng = np.random.default_rng(1000 * k + 10 * vw + (fmt == "fasta"))
    seqs = MC.reads(rng, 150, k)
    data = MC.fastq(rng, seqs) if fmt == "fastq" else MC.fasta(seqs)
    build_device(ctx, idx, data)
    model.build(data, orc.FASTQ if fmt == "fastq" else orc.FASTA)
    assert idx.local_size() == model.size() > len(model.d)            # keys repeat
    cap, extra = cap_from(model)
    probes = np.concatenate([M.probes(s, stored_keys(model), rng, n_stored=600, n_absent=200), extra])
    q = np.concatenate([probes, probes])
    q = np.ascontiguousarray(q[rng.permutation(q.shape[0])])
    before = idx.to_vector()
    for max_occ in (LM.LOCATE_ALL, cap):
        want = model.locate(q, max_occ)
        assert int((want[0] == 0).sum()) > 0 and int((want[0] == cap).sum()) > 0 and int((want[0] > cap).sum()) > 0
        if max_occ == cap:
            assert int(want[1][-1]) < int(model.locate(q)[1][-1])    # the cap removes hits
        d = LM.difference(locate_device(ctx, idx, q, max_occ), want)
        assert d is None, "device form, max_occ %d: %s" % (max_occ, d)
        d = LM.difference(idx.locate(q, None if max_occ == LM.LOCATE_ALL else max_occ), want)
        assert d is None, "host form, max_occ %d: %s" % (max_occ, d)
    after = idx.to_vector()
    assert (before[0] == after[0]).all() and (before[1] == after[1]).all()   # the index is not changed
    idx.close()


# ---- several passes
@pytest.mark.parametrize("k,alpha,kind", MC.PASS_SHAPES)
def test_locate_in_several_passes(ctxs, k, alpha, kind):
    """N_HOT = 16 000 distinct keys of ONE placement bucket, each one to three times, among 20 000 random k-mers: more distinct keys
    than any table takes in one pass, so both kernels split the bucket's entries and queries into passes, under the tables' own
    sizes and under 64 home slots. The two answers are equal to each other and to the model."""
    got = {}
    s = orc.kspec(k, MC.ALPHA[alpha])
    rng = np.random.default_rng(100 * k + MC.VW[kind])
    hot = MC.hot_keys(k, alpha, MC.N_HOT)
    kmers, vals = MC.hot_tuples(rng, hot, MC.VW[kind], s)
    q = MC.pass_queries(rng, hot, s)
    model = LM.LocateModel(s, orc.SINGLE, MC.VW[kind])
    model.insert(kmers, vals)
    for name in ("default", "small"):
        ctx = ctxs[name]
        _, vw, idx, _ = make_index(ctx, k, alpha, "single", kind)
        idx.insert(kmers, vals)
        for max_occ in (LM.LOCATE_ALL, 2):
            want = model.locate(q, max_occ)
            got[name, max_occ] = locate_device(ctx, idx, q, max_occ)
            assert ctx.debug_counter(8) >= 2, "%s table: %d passes" % (name, ctx.debug_counter(8))
            d = LM.difference(got[name, max_occ], want)
            assert d is None, "%s table, max_occ %d: %s" % (name, max_occ, d)
        idx.close()
    for max_occ in (LM.LOCATE_ALL, 2):
        a, b = got["default", max_occ], got["small", max_occ]
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2].shape == b[2].shape


# ---- a heavy key
@pytest.mark.parametrize("k,alpha,kind", MC.HEAVY_SHAPES)
def test_locate_a_heavy_key(ctxs, k, alpha, kind):
    """one key with N_HEAVY = 150 000 values among 5000 random tuples, asked twice among stored and absent keys: all 300 000 values
    are listed without a cap (a group far longer than a workgroup has lanes: copied by whole wavefronts), none of them with
    max_occ = 1000, where occ still says 150 000. At k = 32 the key is the table's empty marker."""
    ctx = ctxs["default"]
    s, vw, idx, model = make_index(ctx, k, alpha, "single", kind)
    rng = np.random.default_rng(100 * k + vw + 1)
    heavy = MC.hot_keys(k, alpha, 1) if k != 32 else np.array([[MC.EMPTY_MARKER]], dtype=np.uint64)
    filler = MC.random_kmers(s, rng, 5000)
    for a, b in ((filler, MC.distinct_values(rng, filler.shape[0], vw)), MC.heavy_tuples(heavy, vw=vw)):
        idx.insert(a, b)
        model.insert(a, b)
    assert idx.local_size() == model.size() == 5000 + MC.N_HEAVY
    q = np.concatenate([filler[:300], heavy, MC.random_kmers(s, rng, 200), heavy, filler[100:200]])
    at = [300, 501]
    occ, off, values = locate_device(ctx, idx, q, LM.LOCATE_ALL)
    assert occ[at].tolist() == [MC.N_HEAVY] * 2 and [int(off[i + 1] - off[i]) for i in at] == [MC.N_HEAVY] * 2
    assert values.shape[0] == int(off[-1]) >= 2 * MC.N_HEAVY
    assert LM.difference((occ, off, values), model.locate(q)) is None
    for i in at:
        assert np.unique(values[int(off[i]):int(off[i + 1]), 0]).size == MC.N_HEAVY
    occ, off, values = locate_device(ctx, idx, q, 1000)
    assert occ[at].tolist() == [MC.N_HEAVY] * 2 and [int(off[i + 1] - off[i]) for i in at] == [0, 0]
    assert LM.difference((occ, off, values), model.locate(q, 1000)) is None
    assert values.shape[0] == int(off[-1]) == int(model.locate(q)[1][-1]) - 2 * MC.N_HEAVY
    idx.close()


# ---- edges
def test_locate_edges(ctxs):
    import kmerind_amd as K
    from kmerind_amd import _lib as L
    ctx = ctxs["default"]
    s, vw, idx, model = make_index(ctx, 31, "DNA", "canonical", "position")
    rng = np.random.default_rng(5)
    data = MC.fastq(rng, MC.reads(rng, 60, 31))
    q = MC.tuples_of(s, data, 1)[0][:500]
    # an empty index: occ = 0 everywhere, offsets all 0
    st, n, occ, off, _, intact = locate_raw(ctx, idx, q, LM.LOCATE_ALL, 0)
    assert st == L.OK and n == 0 and intact and not occ.any() and not off.any()
    occ, off, values = idx.locate(q)
    assert not occ.any() and not off.any() and values.shape == (0, 1)
    build_device(ctx, idx, data)
    model.build(data)
    before = idx.to_vector()
    want = model.locate(q)
    n_hits = int(want[1][-1])
    assert n_hits > q.shape[0]
    # nq = 0: offsets[0] = 0, nothing else is touched
    st, n, occ, off, values, intact = locate_raw(ctx, idx, q[:0], LM.LOCATE_ALL, 4)
    assert st == L.OK and n == 0 and intact and off.tolist() == [0] and (values == np.uint64(PATTERN)).all()
    occ, off, values = idx.locate(q[:0])
    assert occ.shape == (0,) and off.tolist() == [0] and values.shape == (0, 1)
    # max_occ = 0
    st, n, *_ = locate_raw(ctx, idx, q, 0, n_hits)
    assert st == L.ERR_INVALID
    with pytest.raises(L.KmiError) as e:
        idx.locate(q, max_occ=0)
    assert e.value.status == L.ERR_INVALID
    # the sizing call: occ, offsets and n_hits, no values
    st, n, occ, off, _, intact = locate_raw(ctx, idx, q, LM.LOCATE_ALL, 0, with_values=False)
    assert st == L.OK and n == n_hits and intact and (occ == want[0]).all() and (off == want[1]).all()
    # capacity one short: occ and offsets complete, nothing written into values
    st, n, occ, off, values, intact = locate_raw(ctx, idx, q, LM.LOCATE_ALL, n_hits - 1)
    assert st == L.ERR_OVERFLOW and n == n_hits and intact
    assert (occ == want[0]).all() and (off == want[1]).all() and (values == np.uint64(PATTERN)).all()
    # exactly enough
    st, n, occ, off, values, intact = locate_raw(ctx, idx, q, LM.LOCATE_ALL, n_hits)
    assert st == L.OK and intact and LM.difference((occ, off, values), want) is None
    after = idx.to_vector()
    assert (before[0] == after[0]).all() and (before[1] == after[1]).all()
    idx.close()
    # a count index
    cidx = K.CountIndex(ctx, K.make_config(31, "DNA", strand="canonical"))
    cidx.build(data)
    cidx.value_words = 1
    st, *_ = locate_raw(ctx, cidx, q, LM.LOCATE_ALL, 16)
    assert st == L.ERR_INVALID
    cidx.close()
