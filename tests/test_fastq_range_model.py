"""The model of tests/fastq_range_model.py, pinned on the CPU: its four-line rule is the oracle's restatement of
FASTQParser::find_first_record (orc_fastq_align, fastq_loader.hpp:269-364) at every position of every input, and two ranks that
apply its range decision to [0, c) and [c, n) tile the file at a true record start whatever c and whatever the look-ahead. With
this the reference rule alone satisfies what tests/test_gpu_fastq_ranges.py asserts of the library."""
import glob
import os

import pytest

from tests import fastq_range_model as M
from tests import oracle as orc


def _inputs():
    out = [("tricky-40", M.tricky(24)), ("tricky-40-crlf", M.tricky(24, eol=b"\r\n")), ("tricky-40-no-final-eol", M.tricky(24, final_eol=False)),
           ("tricky-10", M.tricky(24, read_len=10)), ("tricky-10-crlf", M.tricky(24, read_len=10, eol=b"\r\n")),
           ("tricky-10-no-final-eol", M.tricky(24, read_len=10, final_eol=False))]
    out += [(os.path.basename(p), M.golden(os.path.basename(p))) for p in sorted(glob.glob(os.path.join(M.GOLD, "*.fastq")))]
    return out


INPUTS = _inputs()
IDS = [name for name, _ in INPUTS]


def test_the_inputs_are_what_the_range_tests_expect():
    assert len(INPUTS) == 6 + 11
    assert all(len(d) < 3072 for _, d in M.small_inputs())
    assert len(M.tricky(12)) < 1100 and orc.extract(orc.kspec(31), M.tricky(12), orc.FASTQ)["n_seqs"] == 12
    assert orc.extract(orc.kspec(21), M.golden("test.small.fastq"), orc.FASTQ)["n_seqs"] == 7
    assert orc.extract(orc.kspec(21), M.golden("test.debruijn.tiny.fastq"), orc.FASTQ)["n_seqs"] == 1
    assert orc.extract(orc.kspec(21), M.golden("test.unitiqs.fastq"), orc.FASTQ)["n_seqs"] == 2
    q = [M.tricky(4).split(b"\n")[4 * i + 3][:2] for i in range(4)]
    assert q == [b"@@", b"+I", b"@+", b"II"]


@pytest.mark.parametrize("name,data", INPUTS, ids=IDS)
def test_the_rule_is_the_oracles_at_every_position(name, data):
    n = len(data)
    for pos in range(1, n):
        assert M.first_record_from(data, pos) == orc.fastq_align(data, pos), (name, pos)
    # what the oracle's function cannot be asked: the ends, and position 0 of a buffer that starts inside the file
    assert M.first_record_from(data, 0) == 0 and M.first_record_from(data, n) == n and M.first_record_from(data, n + 5) == n
    assert M.first_record_from(data, 0, starts_file=False) == M.first_record_from(data, 1)   # (byte 0 is no EOL: the same line)


@pytest.mark.parametrize("name,data", INPUTS, ids=IDS)
def test_the_rule_on_a_buffer_that_starts_inside_the_file(name, data):
    """the first record start of data[c:], found without knowing what lies before c, is the file's first record start at or
    after c: a neighbour that looks from position c of the whole file finds the same place"""
    n = len(data)
    for c in range(n + 1):
        tail = data[c:]
        got = c + M.first_record_from(tail, 0, starts_file=(c == 0))
        assert got == (M.first_record_from(data, c) if c else 0), (name, c)


def test_the_rule_only_looks_forward():
    """position p of the buffer data[c:] is position c + p of the file, whatever c and p: the table of a buffer that starts inside
    the file is the file's table shifted (what test_gpu_fastq_ranges.py expects of kmi_fastq_find_records_dev on d + c)"""
    for name, data in M.small_inputs(12):
        n = len(data)
        table = [M.first_record_from(data, q, starts_file=False) for q in range(n + 1)]
        for c in range(n + 1):
            tail = data[c:]
            assert [M.first_record_from(tail, p, starts_file=False) for p in range(n - c + 1)] == [t - c for t in table[c:]], (name, c)


@pytest.mark.parametrize("name,data", INPUTS, ids=IDS)
def test_two_ranks_tile_the_file_at_a_true_record_start(name, data):
    n = len(data)
    starts = set(M.true_record_starts(data)) | {n}
    worst = 0
    for c in range(n + 1):
        for look in (1, 16, 1 << 20):
            b0, e0, r0 = M.partition_of(data, 0, c, look)
            b1, e1, r1 = M.partition_of(data, c, n, look)
            assert (b0, e1) == (0, n) and e0 == b1, (name, c, look, (b0, e0), (b1, e1))
            assert e0 in starts, (name, c, look, e0)
            assert r1 == 1 and (look < (1 << 20) or r0 == 1)
            worst = max(worst, r0)
    assert worst <= 9   # (a 31 KB record from one byte of look-ahead: 4^8 bytes cover it)


@pytest.mark.parametrize("p", [3, 5, 8, 30])
def test_p_ranks_tile_the_file(p):
    for name, data in INPUTS[:6] + [("test.small.fastq", M.golden("test.small.fastq"))]:
        n = len(data)
        starts = set(M.true_record_starts(data)) | {n}
        parts = [M.partition_of(data, n * r // p, n * (r + 1) // p, 16) for r in range(p)]
        assert parts[0][0] == 0 and parts[-1][1] == n, name
        for a, b in zip(parts, parts[1:]):
            assert a[1] == b[0] and a[1] in starts, (name, p, parts)
        if p == 30:
            assert any(a[0] == a[1] for a in parts), name   # more ranks than records: some range holds no record start
