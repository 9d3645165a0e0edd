"""examples/de_bruijn_bubbles.cpp through the facade (NodeIndex::spectrum, retain_counts, prune_edges, clip_tips, pop_bubbles,
unitigs) on the cleaning pipeline's input: every printed count against tests/dbg_clean_model.py, tests/tips_model.py,
tests/bubbles_model.py and tests/unitig_model.py on the oracle's node map. With min_count = 1 no node is filtered: the tip rounds
leave 19 unitigs, and one round of popping leaves the genome. With a limit of 3 nodes nothing is short enough to leave; with the
spectrum's valley as the threshold the filter has removed the errors already."""
import os
import subprocess
import tempfile

import pytest

from tests import bubbles_model as B
from tests import dbg_clean_model as D
from tests import oracle as orc
from tests import tips_model as T
from tests import unitig_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _valley(hist):
    for c in range(1, len(hist) - 2):
        if hist[c] < hist[c - 1] and hist[c] <= hist[c + 1]:
            return c
    return 1


def _shape(nodes):
    u = M.unitigs_from_strings(nodes)
    return len(u), D.n50([len(x) for x, _, _ in u])


def _expected(nodes, min_count, max_nodes):
    """the example's lines as (name, value) pairs, from the models"""
    out = [("nodes_built", len(nodes))] + list(zip(("unitigs_built", "n50_built"), _shape(nodes)))
    thr = min_count if min_count else _valley(D.spectrum(nodes, 256)[0])
    kept = D.retain(nodes, thr, 2**32 - 1)
    out += [("threshold", thr), ("erased", len(nodes) - len(kept))] + list(zip(("unitigs_filtered", "n50_filtered"), _shape(kept)))
    cur, ps = D.prune(kept, 1)
    out += [("cleared_pruned", ps["n_set_before"] - ps["n_set_after"])] + list(zip(("unitigs_pruned", "n50_pruned"), _shape(cur)))
    p = 0
    while True:
        p += 1
        r = 0
        while True:
            r += 1
            cur, s = T.clip(cur, 1, max_nodes)
            cur, ps = D.prune(cur, 1)
            pre = "p%d_t%d_" % (p, r)
            out += [(pre + "candidates", s["n_candidates"]), (pre + "clipped", s["n_tips_clipped"]), (pre + "nodes_removed", s["n_nodes_removed"]),
                    (pre + "cleared", ps["n_set_before"] - ps["n_set_after"])] + list(zip((pre + "unitigs", pre + "n50"), _shape(cur)))
            if s["n_tips_clipped"] == 0:
                break
        popped, r = 0, 0
        while True:
            r += 1
            cur, s = B.pop(cur, 1, max_nodes)
            cur, ps = D.prune(cur, 1)
            pre = "p%d_b%d_" % (p, r)
            out += [(pre + "branches", s["n_branches"]), (pre + "bubbles", s["n_bubbles"]), (pre + "popped", s["n_popped"]),
                    (pre + "nodes_removed", s["n_nodes_removed"]), (pre + "cleared", ps["n_set_before"] - ps["n_set_after"])]
            out += list(zip((pre + "unitigs", pre + "n50"), _shape(cur)))
            popped += s["n_popped"]
            if s["n_popped"] == 0:
                break
        if popped == 0:
            break
    return out + [("passes", p), ("nodes_final", len(cur))] + list(zip(("unitigs_final", "n50_final"), _shape(cur)))


@pytest.mark.parametrize("args,passes,final", [(["1"], 2, (1, 1500)), (["1", "3"], 1, (29, 115)), ([], 1, (1, 1480))])
def test_de_bruijn_bubbles_example(args, passes, final):
    k = 31
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "de_bruijn_bubbles"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "examples", "de_bruijn_bubbles")
    genome, reads = D.pipeline_reads(k)
    data = D.fastq(reads)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.fastq")
        with open(path, "wb") as f:
            f.write(data)
        out = subprocess.run([exe, path] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = [(line.split("\t")[0], int(line.split("\t")[1])) for line in out.stdout.splitlines() if "\t" in line]
    s = orc.kspec(k)
    om = orc.DbgMap(s)
    om.insert(*orc.dbg_parse(s, data))
    nodes = D.nodes_of(*om.export(canonical=True), k)
    want = _expected(nodes, int(args[0]) if args else 0, int(args[1]) if len(args) > 1 else 2 * k)
    assert got == want
    vals = dict(got)
    assert (vals["passes"], (vals["unitigs_final"], vals["n50_final"])) == (passes, final)
    if args == ["1"]:   # the README's figures for this input
        assert (vals["unitigs_pruned"], vals["p1_t2_unitigs"], vals["p1_t2_n50"]) == (29, 19, 259)
        assert (vals["p1_b1_branches"], vals["p1_b1_bubbles"], vals["p1_b1_popped"], vals["p1_b1_nodes_removed"], vals["p1_b1_cleared"]) == (12, 6, 6, 186, 0)
        assert (vals["p1_b1_unitigs"], vals["p1_b1_n50"], vals["p1_b2_popped"], vals["p2_b1_popped"]) == (1, 1500, 0, 0)
