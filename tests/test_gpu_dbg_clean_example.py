"""examples/de_bruijn_clean.cpp through the facade (NodeIndex::spectrum, retain_counts, prune_edges, unitigs) on the cleaning
pipeline's input: every printed count against tests/dbg_clean_model.py and tests/unitig_model.py on the oracle's node map."""
import os
import subprocess
import tempfile

import pytest

from tests import dbg_clean_model as D
from tests import oracle as orc
from tests import unitig_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _valley(hist):
    """the example's rule: the first count whose bin is lower than the one before and not higher than the one behind; else 1"""
    for c in range(1, len(hist) - 2):
        if hist[c] < hist[c - 1] and hist[c] <= hist[c + 1]:
            return c
    return 1


@pytest.mark.parametrize("n_bins", [256, 8])
def test_de_bruijn_clean_example(n_bins):
    k = 31
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "de_bruijn_clean"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "examples", "de_bruijn_clean")
    genome, reads = D.pipeline_reads(k)
    data = D.fastq(reads)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.fastq")
        with open(path, "wb") as f:
            f.write(data)
        out = subprocess.run([exe, path, str(n_bins)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = [line.split("\t") for line in out.stdout.splitlines() if "\t" in line]
    assert [g[0] for g in got] == ["nodes_before", "unitigs_before", "n50_before", "threshold", "erased", "nodes_after", "set_before", "weak",
                                   "absent", "unreciprocated", "set_after", "isolated", "unitigs_after", "n50_after"]
    vals = dict((g[0], int(g[1])) for g in got)
    s = orc.kspec(k)
    om = orc.DbgMap(s)
    om.insert(*orc.dbg_parse(s, data))
    nodes = D.nodes_of(*om.export(canonical=True), k)
    before = M.unitigs_from_strings(nodes)
    thr = _valley(D.spectrum(nodes, n_bins)[0])
    kept = D.retain(nodes, thr, 2**32 - 1)
    pruned, stats = D.prune(kept, 1)
    after = M.unitigs_from_strings(pruned)
    assert thr > 1 and len(kept) < len(nodes) and len(after) < len(before)
    assert vals == dict(nodes_before=len(nodes), unitigs_before=len(before), n50_before=D.n50([len(x) for x, _, _ in before]), threshold=thr,
                        erased=len(nodes) - len(kept), nodes_after=len(kept), set_before=stats["n_set_before"], weak=stats["n_weak"],
                        absent=stats["n_absent"], unreciprocated=stats["n_unreciprocated"], set_after=stats["n_set_after"],
                        isolated=stats["n_isolated"], unitigs_after=len(after), n50_after=D.n50([len(x) for x, _, _ in after]))
