"""The comm= argument of CountIndex.lookup / profile_reads and PositionIndex.locate / seed_reads (and their _device forms) reaches
the collective entry of the C ABI: with a communicator every call goes to the kmi_index_*_dist_* symbol, with arguments that fit
the signature kmerind_amd._lib declares for it; without one, to the one-rank symbol as before. No GPU: the library handle of
kmerind_amd.core is replaced by a recorder."""
import ctypes as C

import numpy as np
import pytest


class _Recorder:
    """stands in for the CDLL: every function records (name, args), checks them against SIGNATURES and returns KMI_OK"""

    def __init__(self, L):
        self.L, self.calls = L, []

    def __getattr__(self, name):
        restype, argtypes = self.L.SIGNATURES[name]   # KeyError: the wrapper asked for a symbol the header does not declare

        def fn(*args):
            assert len(args) == len(argtypes), "%s takes %d arguments, got %d" % (name, len(argtypes), len(args))
            for i, (a, t) in enumerate(zip(args, argtypes)):
                try:
                    t.from_param(a)
                except (TypeError, C.ArgumentError) as e:
                    raise AssertionError("%s, argument %d: %r does not fit %s (%s)" % (name, i, a, t, e))
            self.calls.append((name, args))
            return 0
        return fn


class _Ctx:
    h = C.c_void_p(1)

    @staticmethod
    def check(st):
        assert st == 0


class _Comm:
    h = C.c_void_p(2)


@pytest.fixture()
def rec(monkeypatch):
    from kmerind_amd import _lib as L
    from kmerind_amd import core
    r = _Recorder(L)
    monkeypatch.setattr(core, "lib", r)
    return r


def _index(cls, value_words):
    idx = cls.__new__(cls)
    idx.ctx, idx.h, idx.n_words, idx.value_words = _Ctx(), C.c_void_p(3), 1, value_words
    return idx


FASTQ = b"@r\nACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIII\n"
Q = np.arange(5, dtype=np.uint64)


def _calls(kind):
    import kmerind_amd as K
    if kind == "count":
        idx = _index(K.CountIndex, 0)
        return [("lookup", lambda c: idx.lookup(Q, comm=c)),
                ("lookup", lambda c: idx.lookup_device(4096, 5, 8192, comm=c), "_dev"),
                ("profile_reads", lambda c: idx.profile_reads(FASTQ, 2, comm=c)),
                ("profile_reads", lambda c: idx.profile_reads_device(4096, len(FASTQ), 8192, 1, comm=c), "_dev")]
    idx = _index(K.PositionIndex, 1)
    return [("locate", lambda c: idx.locate(Q, 4, comm=c)),
            ("locate", lambda c: idx.locate_device(4096, 5, 8192, 12288, comm=c), "_dev"),
            ("seed_reads", lambda c: idx.seed_reads(FASTQ, comm=c)),
            ("seed_reads", lambda c: idx.seed_reads_device(4096, len(FASTQ), comm=c), "_dev")]


@pytest.mark.parametrize("kind", ["count", "position"])
def test_comm_argument_reaches_the_dist_symbol(rec, kind):
    for name, call, *form in _calls(kind):
        form = form[0] if form else "_host"
        del rec.calls[:]
        call(None)
        assert rec.calls and {n for n, _ in rec.calls} == {"kmi_index_%s%s" % (name, form)}
        del rec.calls[:]
        call(_Comm())
        want = "kmi_index_%s_dist%s" % (name, form)
        assert rec.calls and {n for n, _ in rec.calls} == {want}
        for _, args in rec.calls:
            assert args[1] is _Comm.h          # the communicator's handle, right behind the index's
        if form == "_host" and name != "lookup":
            assert len(rec.calls) == 2         # the sizing call and the filling call, on every rank


def test_dist_signatures_are_the_one_rank_ones_plus_the_communicator():
    from kmerind_amd import _lib as L
    for name in ("lookup", "profile_reads", "locate", "seed_reads"):
        for form in ("_dev", "_host"):
            res, args = L.SIGNATURES["kmi_index_%s%s" % (name, form)]
            dres, dargs = L.SIGNATURES["kmi_index_%s_dist%s" % (name, form)]
            assert dres is res and dargs == [args[0], C.c_void_p] + args[1:]
