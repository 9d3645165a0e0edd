"""kmi_index_seed_reads_dist_* and kmi_index_profile_reads_dist_*: every rank brings its own record-aligned FASTQ share and gets
the rows, occ, offsets and values of ITS reads -- relative to its own buffer -- from a position index (built from a FASTA file
over the ranks) and a count index (built from the reads over the ranks) whose entries are spread over all ranks. Expected values
are tests/locate_model.py's and tests/read_profile_model.py's over the whole reference / the whole read set. The shares are
uneven (three quarters of the records on rank 0), empty on one rank, or four; with KMI_PROFILE_BATCH=4096 the ranks run different
numbers of rounds, and the result must be that of the default batch. A damaged record on one rank ends the call on every rank."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import index_model as M
from tests import locate_model as LM
from tests import oracle as orc
from tests import read_profile_model as RP

pytestmark = pytest.mark.gpu
K_ = 21
SOLID = 2
CAP = 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, env, fasta, reads, shares, damaged, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.update(env)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmerind_amd as K
        from kmerind_amd import _lib as L
        from kmerind_amd.transport import GroupComm
        ctx = K.Context(0, rank=rank, nranks=world)
        comm = GroupComm(ctx)
        pidx = K.PositionIndex(ctx, K.make_config(K_, "DNA", strand="canonical", index_kind="position", seq_format="fasta"))
        fa = np.frombuffer(fasta, dtype=np.uint8).copy()
        ctx.check(L.lib.kmi_index_build_fasta_file_dist_host(pidx.h, comm.h, fa.ctypes.data_as(C.c_void_p), fa.size))
        cidx = K.CountIndex(ctx, K.make_config(K_, "DNA", strand="canonical"))
        b, e = shares[rank]
        share = reads[b:e]
        buf = np.frombuffer(share, dtype=np.uint8).copy()
        ctx.check(L.lib.kmi_index_build_dist_host(cidx.h, comm.h, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, b))
        out = dict(local=(pidx.local_size(), cidx.local_size()))
        if damaged is not None:
            mine = np.frombuffer(damaged[rank], dtype=np.uint8).copy()
            nr, nk, nh = C.c_uint64(), C.c_uint64(), C.c_uint64()
            st = L.lib.kmi_index_seed_reads_dist_host(pidx.h, comm.h, mine.ctypes.data_as(C.c_void_p), mine.size, L.LOCATE_ALL, None, 0, None, None,
                                                      0, None, 0, C.byref(nr), C.byref(nk), C.byref(nh))
            out["seed_err"] = (st, (L.lib.kmi_last_error(ctx.h) or b"").decode())
            st = L.lib.kmi_index_profile_reads_dist_host(cidx.h, comm.h, mine.ctypes.data_as(C.c_void_p), mine.size, SOLID, None, 0, C.byref(nr))
            out["profile_err"] = (st, (L.lib.kmi_last_error(ctx.h) or b"").decode())
            # the communicator and both indexes are as good as before
            out["seeds"] = pidx.seed_reads(share, comm=comm)
        else:
            out["seeds"] = pidx.seed_reads(share, comm=comm)
            out["seeds_cap"] = pidx.seed_reads(share, CAP, comm=comm)
            out["profile"] = cidx.profile_reads(share, SOLID, comm=comm)
            out["answered"] = ctx.debug_counter(12)
            # the device forms: the sizing call, then buffers of exactly the sizes it gave
            d_in = ctx.alloc(buf.size + 64)
            if buf.size:
                ctx.to_device(d_in, buf)
            nr, nk, nh = pidx.seed_reads_device(d_in, buf.size, comm=comm)
            rows, occ = np.zeros(nr, dtype=LM.ROW), np.zeros(nk, dtype=np.uint32)
            offs, vals = np.zeros(nk + 1, dtype=np.uint64), np.zeros((nh, 1), dtype=np.uint64)
            d = [ctx.alloc(max(a.nbytes, 8)) for a in (rows, occ, offs, vals)]
            got = pidx.seed_reads_device(d_in, buf.size, d[0], nr, d[1], d[2], nk, d[3], nh, comm=comm)
            for a, p in zip((rows, occ, offs, vals), d):
                if a.nbytes:
                    ctx.to_host(a, p)
                ctx.free(p)
            out["seeds_dev"] = (got == (nr, nk, nh), rows, occ, offs, vals)
            prof = np.zeros(nr, dtype=RP.ROW)
            dp = ctx.alloc(max(prof.nbytes, 8))
            n = cidx.profile_reads_device(d_in, buf.size, dp, nr, SOLID, comm=comm)
            if prof.nbytes:
                ctx.to_host(prof, dp)
            ctx.free(dp)
            ctx.free(d_in)
            out["profile_dev"] = (n, prof)
        ret[rank] = out
        pidx.close()
        cidx.close()
        comm.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def inputs():
    """the reference (20 000 bases in three FASTA records), the reads (FASTQ: 400 of 100 bases from both strands of it, three
    shorter than k, five the reference does not hold) and the models over the whole of each"""
    rng = np.random.default_rng(4242)
    genome = M.random_seq(rng, 20_000)
    fasta = M.fasta([genome[:7_000], genome[7_000:15_000], genome[15_000:]])
    seqs = M.background(rng, 400, read_len=100, genome=genome) + [M.random_seq(rng, n) for n in (5, 12, 20)] + \
        [M.random_seq(rng, 100) for _ in range(5)]
    reads = M.fastq([seqs[i] for i in rng.permutation(len(seqs))])
    s = orc.kspec(K_)
    lm = LM.LocateModel(s, orc.CANONICAL, 1)
    lm.build(fasta, orc.FASTA)
    cm = M.CountModel(K_, orc.DNA, orc.CANONICAL)
    cm.insert(orc.extract(s, reads, orc.FASTQ)["kmers"])
    starts = [int(r.record_offset) for r in orc.records(reads, orc.FASTQ)]
    return dict(fasta=fasta, reads=reads, s=s, lm=lm, cm=cm, starts=starts)


def _shares(inp, which):
    from kmerind_amd import fileio
    n = len(inp["reads"])
    if which == "three-quarters":
        cut = inp["starts"][3 * len(inp["starts"]) // 4]
        return [(0, cut), (cut, n)]
    if which == "empty-rank0":
        return [(0, 0), (0, n)]
    return list(fileio.partition_fastq(inp["reads"], 4))


def _run(inp, shares, env, damaged=None):
    world = len(shares)
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), env, inp["fasta"], inp["reads"], shares, damaged, ret), nprocs=world, join=True)
    return [ret[r] for r in range(world)]


def _seeds_difference(got, want):
    return LM.first_row_difference(got[0], want[0]) or LM.difference(got[1:], want[1:])


def _check(inp, shares, R):
    assert sum(x["local"][0] for x in R) == inp["lm"].size() and sum(x["local"][1] for x in R) == inp["cm"].size()
    assert sum(x["answered"] for x in R) == sum(int(x["seeds"][1].shape[0]) for x in R)   # (of the last call: the profile's windows)
    for r, x in enumerate(R):
        share = inp["reads"][shares[r][0]:shares[r][1]]
        want = inp["lm"].seed_reads(share)
        for name, w in (("seeds", want), ("seeds_cap", inp["lm"].seed_reads(share, CAP))):
            d = _seeds_difference(x[name], w)
            assert d is None, "rank %d, %s: %s" % (r, name, d)
        ok, *dev = x["seeds_dev"]
        d = _seeds_difference(dev, want)
        assert ok and d is None, "rank %d, device form: %s" % (r, d)
        wp = RP.profile(share, inp["s"], inp["cm"], SOLID)
        for name, got in (("host", x["profile"]), ("device", x["profile_dev"][1])):
            d = RP.first_row_difference(got, wp)
            assert d is None, "rank %d, profile, %s form: %s" % (r, name, d)
        assert x["profile_dev"][0] == wp.shape[0]


BATCHES = {"batch-4096": {"KMI_PROFILE_BATCH": "4096"}, "batch-default": {}}


@pytest.fixture(scope="module")
def uneven(inputs):
    """the runs with three quarters of the records on rank 0, by batch size: made once, shared by the tests below"""
    done = {}

    def get(name):
        if name not in done:
            done[name] = _run(inputs, _shares(inputs, "three-quarters"), BATCHES[name])
        return done[name]
    return get


@pytest.mark.parametrize("batch", list(BATCHES))
def test_uneven_shares(inputs, uneven, batch):
    """three quarters of the records on rank 0: with batches of 4096 bytes some twenty rounds on rank 0 and a third of that on
    rank 1, with the default batch one round"""
    shares = _shares(inputs, "three-quarters")
    want = inputs["lm"].seed_reads(inputs["reads"][shares[0][0]:shares[0][1]])
    assert int(want[2][-1]) > 0 and int((want[0]["n_kmers"] == 0).sum()) > 0 and int((want[1] == 0).sum()) > 0
    _check(inputs, shares, uneven(batch))


def test_results_do_not_depend_on_the_batch_size(uneven):
    for a, b in zip(uneven("batch-4096"), uneven("batch-default")):
        for got, other in zip(a["seeds"][:3], b["seeds"][:3]):
            assert (got == other).all()
        assert sorted(a["seeds"][3][:, 0].tolist()) == sorted(b["seeds"][3][:, 0].tolist())
        assert (a["profile"] == b["profile"]).all()


@pytest.mark.parametrize("which,env", [("empty-rank0", {"KMI_PROFILE_BATCH": "4096"}), ("four-ranks", {})])
def test_an_empty_share_and_four_ranks(inputs, which, env):
    shares = _shares(inputs, which)
    _check(inputs, shares, _run(inputs, shares, env))


def test_a_damaged_record_ends_the_call_on_every_rank(inputs):
    """rank 1's last record has its '+' line damaged (behind several good batches): rank 1 returns the parse error, rank 0
    KMI_ERR_PEER with the collectives' wording, both processes join, and the next collective call works"""
    from kmerind_amd import _lib as L
    shares = _shares(inputs, "three-quarters")
    mine = [inputs["reads"][b:e] for b, e in shares]
    at = mine[1].rindex(b"\n+\n")
    damaged = [mine[0], mine[1][:at] + b"\n-\n" + mine[1][at + 3:]]
    R = _run(inputs, shares, {"KMI_PROFILE_BATCH": "4096"}, damaged)
    for name in ("seed_err", "profile_err"):
        assert R[1][name][0] == L.ERR_PARSE, R[1][name]
        assert R[0][name][0] == L.ERR_PEER and "another rank" in R[0][name][1], R[0][name]
    for r, x in enumerate(R):
        d = _seeds_difference(x["seeds"], inputs["lm"].seed_reads(mine[r]))
        assert d is None, "rank %d after the error: %s" % (r, d)
