"""The read-profile model (tests/read_profile_model.py) on the stored FASTQ files, each profiled against its own counts, where
the expected rows have closed forms that do not depend on how the model groups k-mers by read; and the boundary: the header
declares the four entry points and the shared library exports them. CPU only."""
import os
import re

import numpy as np
import pytest

from tests import index_model as M
from tests import oracle as orc
from tests import read_profile_model as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")


@pytest.mark.parametrize("k", [21, 31])
@pytest.mark.parametrize("fname", ["test.small.fastq", "natural.withN.fastq"])
def test_a_file_profiled_against_its_own_counts(fname, k):
    data = open(os.path.join(DATA, fname), "rb").read()
    s = orc.kspec(k)
    ex = orc.extract(s, data, orc.FASTQ)
    model = M.CountModel(k)
    model.insert(ex["kmers"])
    rows = RP.profile(data, s, model, solid=2)
    assert rows.shape[0] == len(orc.records(data, orc.FASTQ)) == ex["n_seqs"]
    assert (rows["n_present"] == rows["n_kmers"]).all()
    has = rows["n_kmers"] > 0
    assert has.any() and (rows["lowest"][has] >= 1).all() and (rows["highest"] >= rows["lowest"]).all()
    assert (rows["n_solid"] <= rows["n_present"]).all() and (rows["reserved"] == 0).all()
    assert int(rows["n_kmers"].sum()) == ex["kmers"].shape[0]
    # every occurrence of a key of count c contributes c: sum over reads = sum over keys of c^2
    counts = model.export()[1].astype(np.uint64)
    assert int(rows["sum_counts"].sum()) == int((counts * counts).sum())
    # solid: the occurrences of keys seen at least twice
    assert int(rows["n_solid"].sum()) == int(counts[counts >= 2].sum())
    for i, r in enumerate(orc.records(data, orc.FASTQ)):   # the sequence line starts right behind the header line's end
        assert data[int(rows["seq_offset"][i]) - 1:int(rows["seq_offset"][i])] in (b"\n", b"\r") and r.seq_begin == rows["seq_offset"][i]


def test_lookup_model_answers_in_query_order():
    k = 21
    s = orc.kspec(k)
    model = M.CountModel(k)
    a, b = orc.kmers_from_string(s, b"ACGTTGCATGCATGGGATTACA" * 2), orc.kmers_from_string(s, b"T" * 30)
    model.insert(np.concatenate([a, a[:5]]))
    q = np.concatenate([b[:2], a[:6], orc.revcomp(s, a[:3]), a[:1]])
    want = [0, 0] + [int(model.find(a[i:i + 1])[1][0]) for i in range(6)] + [int(model.find(a[i:i + 1])[1][0]) for i in range(3)]
    want.append(want[2])
    assert RP.lookup(model, q).tolist() == want


def test_header_declares_and_library_exports_the_entry_points():
    from kmerind_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "kmerind_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("kmi_index_lookup_dev", "kmi_index_lookup_host", "kmi_index_profile_reads_dev", "kmi_index_profile_reads_host"):
        assert re.search(r"\bkmi_status\s+%s\s*\(" % name, text), name
        assert hasattr(L.lib, name) and name in L.SIGNATURES, name
    assert re.search(r"\}\s*kmi_read_profile\s*;", text)
    from kmerind_amd import core
    assert core.READ_PROFILE_DTYPE == RP.ROW and RP.ROW.itemsize == 40
