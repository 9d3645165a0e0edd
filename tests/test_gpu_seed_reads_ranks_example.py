"""examples/seed_reads_ranks.cpp through the facade: with KMI_FORCE_DIST=1 the one rank builds its index through the collective
build and asks it through kmi_index_seed_reads_dist_host (an RCCL communicator of one rank, the rank being its own peer). Its
table for the golden files must be the table examples/seed_reads prints for them on one rank, and both the rows of
tests/locate_model.py."""
import os
import subprocess

import pytest

from tests import locate_model as LM
from tests import oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
HEADER = "#seq_offset\tn_kmers\tn_listed\tn_hits"


def _table(exe, args, env=None):
    out = subprocess.run([os.path.join(ROOT, "examples", exe)] + args, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, **(env or {})))
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert HEADER in lines, out.stdout
    return lines[lines.index(HEADER):]   # (RCCL greets on stdout when a communicator is made)


@pytest.mark.parametrize("max_occ", [None, 3])
def test_seed_reads_ranks_example(max_occ):
    for exe in ("seed_reads", "seed_reads_ranks"):
        if not os.path.exists(os.path.join(ROOT, "examples", exe)):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    ref, reads = os.path.join(DATA, "natural.fasta"), os.path.join(DATA, "natural.fastq")
    args = [ref, reads] + ([] if max_occ is None else [str(max_occ)])
    got = _table("seed_reads_ranks", args, {"KMI_FORCE_DIST": "1"})
    assert got == _table("seed_reads", args)
    model = LM.LocateModel(orc.kspec(21, orc.DNA), orc.CANONICAL, 1)
    model.build(open(ref, "rb").read(), orc.FASTA)
    rows, occ, offsets, _ = model.seed_reads(open(reads, "rb").read(), LM.LOCATE_ALL if max_occ is None else max_occ)
    assert got[0] == HEADER
    assert got[1:-1] == ["%d\t%d\t%d\t%d" % (r["seq_offset"], r["n_kmers"], r["n_listed"], r["n_hits"]) for r in rows]
    assert got[-1] == "#total\t%d\t%d\t%d" % (rows.shape[0], occ.shape[0], int(offsets[-1]))
    assert int(offsets[-1]) > 0
