"""tests/fasta_block_model.py pinned on the oracle's parse of whole files and on brute-force byte scans, on the CPU: the GPU
tests (test_gpu_fasta_ranges.py) compare the library with this model, so the model itself must not be the product's rules
written twice. Everything is exact."""
import numpy as np
import pytest

from tests import fasta_block_model as M
from tests import oracle as orc

SMALL = M.small_inputs()
IDS = [x[0] for x in SMALL]
POS = (1 << 40) - 1


def _ls(data, lo):
    return lo == 0 or data[lo - 1:lo] == b"\n"


def _tuples(data, k=4):
    ex = orc.extract(orc.kspec(k), data, orc.FASTA, want_ids=True)
    return ex, (ex["ids"] & np.uint64(POS)).astype(np.int64), (ex["ids"] >> np.uint64(40)).astype(np.int64)


def test_the_inputs_hold_what_they_are_meant_to():
    m = M.main_input()
    assert len(m) <= 200 and len(M.three_way_input()) == 48
    assert m.startswith(b"AC\nGT\n>") and not m.endswith(b"\n")                         # orphan lines, no final EOL
    assert b">r1 a>b\n;note\n" in m and b"\n;mid\n" in m                                # ';' in a header group and between sequence lines
    assert b"\n\n" in m and b"\r\n\r\n" in m and b">r2\n>r3" in m and b">s\nACG\n>" in m  # blank lines, header | header, a short record
    lone = [i for i in range(len(m)) if m[i:i + 1] == b"\r" and m[i + 1:i + 2] != b"\n"]
    assert lone and M.seq_mask(m)[lone[0] - 1] and M.seq_mask(m)[lone[0] + 1]            # a lone '\r' inside a sequence line
    gt = [i for i in range(len(m)) if m[i:i + 1] == b">" and M.seq_mask(m)[i]]
    assert gt                                                                            # '>' as a sequence character
    assert b"\n" not in M.crlf(m).replace(b"\r\n", b"")
    d = dict(SMALL)
    assert d["opens-with-header"][:1] == b">" and d["opens-with-semicolon"][:1] == b";"
    for name, data in SMALL:
        assert len(data) <= 210, name
        assert orc.extract(orc.kspec(5 if name != "three-way" else 4), data, orc.FASTA)["kmers"].shape[0] > 0, name
    for k, alpha in ((15, orc.DNA), (21, orc.DNA5)):
        assert orc.extract(orc.kspec(k, alpha), m, orc.FASTA)["kmers"].shape[0] > 0


@pytest.mark.parametrize("name,data", SMALL + [(n, M.golden(n)) for n in M.GOLDEN_FASTA], ids=IDS + list(M.GOLDEN_FASTA))
def test_records_of_a_whole_file_are_the_oracles(name, data):
    ex, pos, _ = _tuples(data)
    s = M.summary(data, True)
    assert s[1] == ex["n_seqs"], (name, s, ex["n_seqs"])
    mask = M.seq_mask(data)
    assert mask[pos].all(), name                       # every k-mer of the oracle begins on a sequence character
    # and its window is the k sequence characters from there on: nothing but EOLs (and the characters) in between
    ends = [M.overlap_end(data, int(p) + 1, 3) for p in pos[:: max(1, pos.size // 200)]]
    a = np.frombuffer(data, dtype=np.uint8)
    for p, e in zip(pos[:: max(1, pos.size // 200)].tolist(), ends):
        w = a[p:e]
        assert int(mask[p:e].sum()) == 4 and ((w == 10) | (w == 13) | mask[p:e]).all(), (name, p, e)


@pytest.mark.parametrize("name,data", SMALL, ids=IDS)
def test_summaries_compose_over_every_two_and_three_way_cut(name, data):
    n = len(data)
    whole = M.summary(data, True)
    S = {(lo, hi): M.summary(data[lo:hi], _ls(data, lo)) for lo in range(n + 1) for hi in range(lo, n + 1)}
    assert S[(0, n)] == whole
    for c1 in range(n + 1):
        for c2 in range(c1, n + 1):      # (c2 = n: the two-way cuts, with an empty third block)
            blocks = [S[(0, c1)], S[(c1, c2)], S[(c2, n)]]
            for state_in in (M.OUTSIDE, M.HEADER, M.SEQUENCE):
                out, records, _ = M.compose(blocks, state_in)
                assert [out, records] == whole[2 * state_in:2 * state_in + 2], (name, c1, c2, state_in)
    # an empty block and a block without a line start pass the state through
    assert M.summary(b"", True) == [0, 0, 1, 0, 2, 0] and M.summary(b"CGT\r", False) == [0, 0, 1, 0, 2, 0]


def _sequence_index_of_first_tuple(data, part, hi, pos, seq):
    """-> (expected, got) for the first oracle tuple inside the block, None when the block holds none. The index of a tuple =
    index_shift + the records that start at or before it - 1; those before the block are the partition's records_before, those
    inside come from a walk of the block that starts in the partition's state"""
    lo = part["begin"]
    inside = np.flatnonzero((pos >= lo) & (pos < hi))
    if inside.size == 0:
        return None
    p = int(pos[inside[0]])
    started = sum(1 for piece in M.walk(data[lo:p + 1], bool(part["at_line_start"]), part["start_state"]) if piece[3])
    return int(seq[inside[0]]), part["records_before"] + part["index_shift"] + started - 1, started


@pytest.mark.parametrize("name,data", SMALL, ids=IDS)
def test_partition_fields_give_the_oracles_sequence_index(name, data):
    n = len(data)
    ex, pos, seq = _tuples(data)
    assert (np.diff(ex["ids"].astype(np.int64)) > 0).all()           # position | seq << 40, in file order
    tilings = [[0, c, n] for c in range(n + 1)]
    if name == "three-way":
        tilings += [[0, c1, c2, n] for c1 in range(n + 1) for c2 in range(c1, n + 1)]
    checked = plain = 0
    for cuts in tilings:
        for r in range(len(cuts) - 1):
            part = M.partition(data, cuts, r)
            assert part["valid_bytes"] == cuts[r + 1] - cuts[r] and part["index_shift"] == (0 if data[:1] in (b">", b";") else 1)
            res = _sequence_index_of_first_tuple(data, part, cuts[r + 1], pos, seq)
            if res is None:
                continue
            exp, got, started = res
            assert got == exp, (name, cuts, r, part)
            checked += 1
            if started == 1:     # the block's first tuple opens the first record that starts inside the block
                assert part["records_before"] + part["index_shift"] == exp
                plain += 1
    assert checked > n and plain > 0
    # ids shift with file_offset
    ex2 = orc.extract(orc.kspec(4), data, orc.FASTA, file_offset=1000, want_ids=True)
    assert (ex2["ids"] == ex["ids"] + np.uint64(1000)).all()


def _in_edge_by_bytes(data, lo):
    """brute force: the last sequence character before byte lo that no record start separates from it"""
    state, prev, at_ls = M.OUTSIDE, None, True
    for i in range(lo):
        c = data[i]
        if at_ls:
            if c in (62, 59):
                state = M.HEADER
            else:
                if state == M.HEADER:
                    prev = None
                state = M.OUTSIDE if state == M.OUTSIDE else M.SEQUENCE
        if state == M.SEQUENCE and c not in (10, 13):
            prev = c
        at_ls = c == 10
    return prev


@pytest.mark.parametrize("name,data", SMALL, ids=IDS)
def test_left_carries_compose_right_to_left(name, data):
    n = len(data)
    expect = [_in_edge_by_bytes(data, lo) for lo in range(n + 1)]
    assert any(e is None for e in expect[5:]) and any(e is not None for e in expect)
    pairs = [(c, c) for c in range(n + 1)] if name != "three-way" else [(c1, c2) for c1 in range(n + 1) for c2 in range(c1, n + 1)]
    passed = 0
    for c1, c2 in pairs:
        blocks = [(0, c1), (c1, c2)]
        sums = [M.summary(data[lo:hi], _ls(data, lo)) for lo, hi in blocks]
        entered = M.compose(sums)[2]
        carries = [M.left_carry(data[lo:hi], _ls(data, lo), st) for (lo, hi), st in zip(blocks, entered)]
        passed += carries[1] == M.PASS and c2 > c1
        assert M.compose_carry(carries) == expect[c2], (name, c1, c2, carries)
    if name == "three-way":
        assert passed > 0      # a non-empty middle block that hands the block before it through


def test_lookahead_and_overlap_end():
    d = b">h\nAC\r\nGT\n>x\nTTTT\n"
    assert M.overlap_end(d, 3, 0) == 3 and M.overlap_end(d, 3, 2) == 5 and M.overlap_end(d, 3, 3) == 8 and M.overlap_end(d, 4, 3) == 9
    assert M.overlap_end(d, 3, 9) == len(d) and M.overlap_end(d, 10, 1) == 14           # skips the header; too few: the file's end
    assert M.lookahead_suffices(d, 0, 3, 2, 2) is False     # 'AC' are sequence characters only when the block ends in HEADER or SEQUENCE
    assert M.lookahead_suffices(d, 0, 5, 100, 50) is True   # reaches the file's end
    assert M.lookahead_suffices(d, 0, 10, 3, 0) is True
    e = b">h\nACGT\nACGT\n"
    assert M.lookahead_suffices(e, 3, 8, 3, 3) is False and M.lookahead_suffices(e, 0, 5, 4, 2) is False   # (nothing counts from OUTSIDE)
    f = b"AC\n>h\nACGT\nA"
    assert M.lookahead_suffices(f, 0, 1, 9, 4) is True and M.lookahead_suffices(f, 0, 1, 9, 5) is False    # 'C' counts from SEQUENCE only
    assert M.equal_cuts(10, 3) == [0, 3, 6, 10] and M.equal_cuts(2, 4) == [0, 0, 1, 1, 2]


@pytest.mark.parametrize("B", [16, 1024, 8192])
def test_seam_inputs_put_the_places_on_the_seam(B):
    for name, d in M.seam_inputs(B):
        assert len(d) == B + 8193, name
        mask = M.seq_mask(d)
        if name == "nl|header":
            assert d[B - 1:B + 1] == b"\n>"
        if name == "nl|record start":
            assert d[B - 1:B] == b"\n" and any(p[0] == B and p[3] for p in M.walk(d, True, M.OUTSIDE))
        if name == "cr|lf":
            assert d[B - 1:B + 1] == b"\r\n"
        if name == "header across":
            assert any(p[0] < B - 1 and p[1] > B + 1 and p[2] == M.HEADER for p in M.walk(d, True, M.OUTSIDE))
        if name == "sequence across":
            assert b"\n" not in d[B - 2:B + 2] and (mask[B - 2:B + 2].all() or B == 16)
