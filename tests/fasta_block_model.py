"""Plain byte-wise model of the bookkeeping a rank of several needs for ITS block of a FASTA file: the line-kind machine over a
block as a transfer function (kmi_fasta_block_summary_dev), the left carry that gives a de Bruijn block its in-edge, the
partition record of a block of any tiling of the file (kmi_fasta_partition_dev, kmi_*_fasta_range_dist_host) and where the
look-ahead behind a block must reach. No GPU, no library, no kmerind_amd.fileio: numpy finds the line starts, the walk is per
line (so 8 MB inputs with long lines stay fast). Also the inputs the FASTA range tests share.

The rules:
  * a line starts at byte 0 of a file and after every '\\n'; a '\\r' does not end a line;
  * a line whose first byte is '>' or ';' is a header line;
  * the machine's state is the kind of the last line that started: OUTSIDE (before any header), HEADER, SEQUENCE;
  * a record starts at the start of a non-header line that follows a header line;
  * sequence characters are the bytes of SEQUENCE lines that are neither '\\r' nor '\\n'."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden", "data")
OUTSIDE, HEADER, SEQUENCE = 0, 1, 2
PASS, CUT = "pass", "cut"
_NL, _CR, _GT, _SEMI = 10, 13, 62, 59


def _arr(buf):
    return np.frombuffer(bytes(buf), dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else np.asarray(buf, dtype=np.uint8)


def line_starts(buf, first_ls):
    """the positions inside the buffer at which a line starts; byte 0 only when the caller says so"""
    a = _arr(buf)
    s = np.flatnonzero(a == _NL) + 1
    s = s[s < a.size]
    if first_ls and a.size:
        s = np.concatenate([np.zeros(1, dtype=s.dtype), s])
    return s.tolist()


def walk(buf, first_ls, state_in):
    """-> [(begin, end, state, record_starts_here)]: the pieces of the buffer between line starts, with the state the machine
    is in over each; the first piece (up to the first line start) is the rest of a line that began before the buffer"""
    a = _arr(buf)
    starts = line_starts(a, first_ls)
    out = []
    state = state_in
    if not starts or starts[0] > 0:
        if a.size:
            out.append((0, starts[0] if starts else a.size, state, False))
    for i, q in enumerate(starts):
        c = int(a[q])
        event = False
        if c == _GT or c == _SEMI:
            state = HEADER
        else:
            event = state == HEADER
            state = OUTSIDE if state == OUTSIDE else SEQUENCE
        out.append((q, starts[i + 1] if i + 1 < len(starts) else a.size, state, event))
    return out


def summary(buf, first_ls):
    """out6 of kmi_fasta_block_summary_dev: for the incoming states OUTSIDE, HEADER, SEQUENCE in turn, the state behind the
    bytes and the records that start inside"""
    out = []
    for state_in in (OUTSIDE, HEADER, SEQUENCE):
        pieces = walk(buf, first_ls, state_in)
        out += [pieces[-1][2] if pieces else state_in, sum(1 for p in pieces if p[3])]
    return out


def compose(summaries, state_in=OUTSIDE):
    """blocks' summaries left to right -> (state behind the last block, records started, [state each block is entered in])"""
    state, records, entered = state_in, 0, []
    for s in summaries:
        entered.append(state)
        records += s[2 * state + 1]
        state = s[2 * state]
    return state, records, entered


def _last_char(a, begin, end):
    """the last byte of a[begin:end] that is neither '\\r' nor '\\n' (None if there is none)"""
    j = end - 1
    while j >= begin and (a[j] == _NL or a[j] == _CR):
        j -= 1
    return int(a[j]) if j >= begin else None


def left_carry(buf, first_ls, state_in):
    """what the buffer says about the sequence character before the byte that follows it: PASS (no sequence character and no
    record start inside: ask the block before), CUT (a record starts behind the last sequence character, or there is a record
    start and no sequence character), or the raw byte of the last sequence character"""
    a = _arr(buf)
    last = PASS
    for begin, end, state, event in walk(a, first_ls, state_in):
        if event:
            last = CUT
        if state == SEQUENCE:
            c = _last_char(a, begin, end)
            if c is not None:
                last = c
    return last


def compose_carry(carries):
    """the blocks' left carries (each for the state its block is entered in), the nearest block last: the in-edge of the block
    behind them, a raw byte or None"""
    for c in reversed(carries):
        if c == PASS:
            continue
        return None if c == CUT else c
    return None


def seq_mask(data, first_ls=True, state_in=OUTSIDE):
    """per byte: is it a sequence character"""
    a = _arr(data)
    m = np.zeros(a.size, dtype=bool)
    for begin, end, state, _ in walk(a, first_ls, state_in):
        if state == SEQUENCE:
            m[begin:end] = True
    return m & (a != _NL) & (a != _CR)


def _after_nth(mask, begin, nth):
    """the position behind the nth True of mask[begin:], len(mask) when there are fewer"""
    if nth <= 0:
        return begin
    idx = np.flatnonzero(mask[begin:])
    return begin + int(idx[nth - 1]) + 1 if idx.size >= nth else mask.size


def overlap_end(data, hi, behind, mask=None):
    """where the look-ahead behind a block that ends at file position hi must reach: behind the behind-th sequence character
    at or after hi (the file's end when there are fewer). mask = seq_mask(data), for callers that ask often"""
    return max(hi, _after_nth(seq_mask(data) if mask is None else mask, hi, behind))


def partition(data, cuts, r, k=1, mask=None):
    """block r = [cuts[r], cuts[r + 1]) of a tiling of the file (cuts[0] = 0, cuts[-1] = len(data), non-decreasing): begin, end
    (with the k - 1 sequence characters of overlap) and the kmi_fasta_partition fields"""
    a = _arr(data)
    lo, hi = cuts[r], cuts[r + 1]
    pieces = walk(a[:lo], True, OUTSIDE)
    return dict(begin=lo, end=overlap_end(a, hi, k - 1, mask), valid_bytes=hi - lo,
                start_state=pieces[-1][2] if pieces else OUTSIDE,
                at_line_start=1 if lo == 0 or a[lo - 1] == _NL else 0,
                records_before=sum(1 for p in pieces if p[3]),
                index_shift=0 if a.size and a[0] in (_GT, _SEMI) else 1)


def lookahead_suffices(data, lo, hi, look, behind):
    """a rank holds file bytes [lo, hi) and `look` bytes behind them. True when the buffer reaches the file's end, or when for
    every state the machine may be in at hi the `behind` sequence characters at or after hi lie inside data[hi : hi + look]
    (the rank does not know the state yet when it has to decide)"""
    a = _arr(data)
    if hi + look >= a.size or behind == 0:
        return True
    ahead = a[hi:hi + look]
    first_ls = hi == 0 or a[hi - 1] == _NL
    return all(int(seq_mask(ahead, first_ls, s).sum()) >= behind for s in (OUTSIDE, HEADER, SEQUENCE))


def equal_cuts(n, p):
    """the equal split: block r = [n r / p, n (r + 1) / p)"""
    return [n * i // p for i in range(p + 1)]


# ---- the inputs of the range tests
def golden(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


GOLDEN_FASTA = ("test.fasta", "test2.fasta", "natural.fasta", "natural.withN.fasta", "test.unitiqs.fasta")


def _seq(rng, n, letters=b"ACGT"):
    return np.frombuffer(letters, dtype=np.uint8)[rng.integers(0, len(letters), n)].tobytes()


def main_input(seed=1):
    """about 200 bytes with everything a block boundary can fall on: orphan lines before the first header, a ';' line inside a
    header group and one between two sequence lines, '>' in the middle of a line, a blank line and a CR-LF blank line inside a
    sequence, a lone '\\r', a header directly followed by a header, a record shorter than any k in use, no final EOL"""
    g = np.random.default_rng(seed)
    return (b"AC\nGT\n"                                                   # orphan lines
            b">r1 a>b\n;note\n" + _seq(g, 24) + b"\n\n" + _seq(g, 9) + b"\r\n\r\n" + _seq(g, 12) + b"\n"
            b";mid\n" + _seq(g, 23) + b"\n"                               # a ';' line between two sequence lines: a new record
            b">r2\n>r3\r\n" + _seq(g, 11) + b"\r" + _seq(g, 14) + b"\r\n"   # header after header; a lone '\r' inside a line
            b">s\nACG\n"                                                  # shorter than k
            b">r4\n" + _seq(g, 13) + b">" + _seq(g, 12) + b"N" + _seq(g, 14))   # '>' in the middle of a line; no final EOL


def crlf(data):
    return data.replace(b"\r\n", b"\n").replace(b"\n", b"\r\n")


def three_way_input():
    """48 bytes for the sweep over every pair of cuts"""
    d = b"A\n>a\n;b\nACGTA\r\n\nCC>GT\n>c\n>d\r\nTTGCA\rG\n>e\nAC\n\nGGAT"
    assert len(d) == 48
    return d


def small_inputs():
    """(label, bytes), each about 200 bytes or less"""
    m = main_input()
    tail = m[m.index(b">r1"):]
    return [("main", m), ("main-crlf", crlf(m)), ("opens-with-header", tail), ("opens-with-semicolon", b";first\n" + tail),
            ("three-way", three_way_input())]


def wave_input(seed=2):
    """about 2.3 KB, 60-character lines, LF and CR-LF records and an orphan line: two 1024-byte seams are crossed"""
    g = np.random.default_rng(seed)
    out = [_seq(g, 37) + b"\n"]
    for i in range(9):
        eol = b"\r\n" if i % 2 else b"\n"
        out.append(b">w%d some text" % i + eol)
        if i == 3:
            out.append(b";another header line" + eol)
        for _ in range(int(g.integers(2, 7))):
            out.append(_seq(g, 60) + eol)
        if i == 4:
            out.append(eol)
    return b"".join(out)


SEAM_PLACES = ("nl|header", "nl|record start", "cr|lf", "header across", "sequence across")


def seam_inputs(B, tail=8193, line=60, seed=3):
    """[(label, bytes)]: for every place of SEAM_PLACES a buffer of B + tail bytes in which that place falls on byte B (the
    byte before the bar is B - 1, the byte behind it is B); the tests take the prefixes of B - 1, B, B + 1 and all bytes.
    `line` = characters per sequence line: long lines for the 8 MB seam, so that a walk per line stays short"""
    g = np.random.default_rng(seed + B % 1000)
    n = B + tail

    def fill(m, opened):
        """m bytes of records (header first unless one is open), ending with '\\n'"""
        out, left = [], m
        if not opened:
            h = b">fill\n"
            if left < len(h) + 2:
                return b"\n" * left
            out.append(h)
            left -= len(h)
        lines = 0
        while left > 0:
            lines += 1
            if lines % 5 == 0 and left > 8:   # a new record every few lines, so that record counts differ along the buffer
                out.append(b">f\n")
                left -= 3
                continue
            w = min(line, left - 1)
            if 0 < left - (w + 1) < 2:      # (never leave a single byte for a line of its own)
                w -= 1
            out.append(_seq(g, w) + b"\n")
            left -= w + 1
        return b"".join(out)

    def around(before, after):
        """... before | after ...: `before` ends at B - 1"""
        head = B - len(before)
        if head >= 8:
            left = fill(head, False) + before
        else:                                # the 16-byte seam: no room for records in front
            left = (b"\n" * head + before)[-B:] if head >= 0 else before[-B:]
        body = left + after
        return body + fill(n - len(body), True)

    s1, s2 = _seq(g, 11), _seq(g, 25)
    out = {
        "nl|header": around(s1 + b"\n", b">next record\n" + s2 + b"\n"),
        "nl|record start": around(b">h\n", s2 + b"\n"),
        "cr|lf": around(s1 + b"\r", b"\n" + s2 + b"\r\n"),
        "header across": around(b">a header th", b"at crosses\n" + s2 + b"\n"),
        "sequence across": around(s1, s2 + b"\n"),
    }
    for name, d in out.items():
        assert len(d) == n, (name, len(d), n)
    assert out["nl|header"][B - 1:B + 1] == b"\n>" and out["cr|lf"][B - 1:B + 1] == b"\r\n"
    assert out["nl|record start"][B - 3:B] == b">h\n" and out["nl|record start"][B:B + 1] in (b"A", b"C", b"G", b"T")
    return [(name, out[name]) for name in SEAM_PLACES]
