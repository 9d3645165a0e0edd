"""examples/count_spectrum.cpp through the facade (Index::count_spectrum, Index::retain_counts) on a golden FASTQ file: the printed
bins, totals, threshold and sizes against tests/index_model.CountModel."""
import os
import subprocess

import numpy as np
import pytest

from tests import index_model as M
from tests import oracle as orc
from tests import spectrum_cases as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _valley(hist):
    """the example's rule: the first count whose bin is lower than the one before and not higher than the one behind; else 1"""
    for c in range(1, len(hist) - 2):
        if hist[c] < hist[c - 1] and hist[c] <= hist[c + 1]:
            return c
    return 1


@pytest.mark.parametrize("n_bins", [256, 8])
def test_count_spectrum_example(n_bins):
    exe = os.path.join(ROOT, "examples", "count_spectrum")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    path = os.path.join(ROOT, "tests", "golden", "data", "test.medium.fastq")
    out = subprocess.run([exe, path, str(n_bins)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = [line.split("\t") for line in out.stdout.splitlines()]
    names = [g[0] for g in got]
    vals = dict((g[0], int(g[1])) for g in got)
    shown = min(16, n_bins)
    assert names == ["bin%d" % c for c in range(shown)] + ["entries", "sum_counts", "min_count", "max_count", "threshold", "size_before",
                                                          "erased", "size_after"]
    s = orc.kspec(21, orc.DNA)
    model = M.CountModel(21, orc.DNA, orc.CANONICAL)
    model.insert(orc.extract(s, open(path, "rb").read(), orc.FASTQ)["kmers"])
    hist, totals = S.model_spectrum(model, n_bins)
    assert [vals["bin%d" % c] for c in range(shown)] == hist[:shown].tolist()
    assert {"n_entries": vals["entries"], "sum_counts": vals["sum_counts"], "min_count": vals["min_count"], "max_count": vals["max_count"]} == totals
    thr = _valley(hist.tolist())
    counts = model.export()[1]
    assert vals["threshold"] == thr
    assert vals["size_before"] == model.size() and vals["erased"] == int((counts < thr).sum())
    assert vals["size_after"] == int((counts >= thr).sum()) == vals["size_before"] - vals["erased"]
