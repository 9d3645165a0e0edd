"""examples/compare_samples.cpp through the facade (Index::compare, Index::combine on two indexes of one context) on two small
FASTQ files written with the model's generators: every printed line against tests/setops_model.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import index_model as M
from tests import oracle as orc
from tests import setops_model as SM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k", [21, 31])
def test_compare_samples_example(tmp_path, k):
    exe = os.path.join(ROOT, "examples", "compare_samples")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    rng = np.random.default_rng(600 + k)
    genome = M.random_seq(rng, 20_000)
    datas = [M.fastq(M.background(rng, 300, genome=genome)),
             M.fastq(M.background(rng, 300, genome=genome[:10_000] + M.random_seq(rng, 10_000)), tag=b"s")]
    paths = []
    for i, d in enumerate(datas):
        paths.append(str(tmp_path / ("sample%d.fastq" % i)))
        with open(paths[-1], "wb") as f:
            f.write(d)
    out = subprocess.run([exe] + paths + ([] if k == 21 else [str(k)]), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = [line.split("\t") for line in out.stdout.splitlines()]
    assert [g[0] for g in got] == list(SM.WORDS) + ["jaccard", "weighted_jaccard", "a_only", "shared", "merged", "merged_sum_counts"]
    vals = dict(got)
    s = orc.kspec(k, orc.DNA)
    ma, mb = M.CountModel(k, orc.DNA, orc.CANONICAL), M.CountModel(k, orc.DNA, orc.CANONICAL)
    ma.insert(orc.extract(s, datas[0], orc.FASTQ)["kmers"])
    mb.insert(orc.extract(s, datas[1], orc.FASTQ)["kmers"])
    want = SM.overlap(ma, mb)
    assert 0 < want["n_shared"] < min(want["n_a"], want["n_b"])
    assert {w: int(vals[w]) for w in SM.WORDS} == {w: want[w] for w in SM.WORDS}
    assert vals["jaccard"] == "%.6f" % want["jaccard"] and vals["weighted_jaccard"] == "%.6f" % want["weighted_jaccard"]
    assert int(vals["a_only"]) == SM.combined(ma, mb, "subtract_keys").size() == want["n_a"] - want["n_shared"]
    assert int(vals["shared"]) == SM.combined(ma, mb, "intersect_min").size() == want["n_shared"]
    merged = SM.combined(ma, mb, "union_add")
    assert int(vals["merged"]) == merged.size()
    assert int(vals["merged_sum_counts"]) == sum(merged.d.values()) == want["sum_a"] + want["sum_b"]
