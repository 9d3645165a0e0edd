"""Plain-Python model of how a rank of several cuts its byte range of a FASTQ file at record starts (the four-line rule of
FASTQParser::find_first_record, fastq_loader.hpp:269-364, as partitioned_file applies it, file.hpp:1216-1430), and of the
decision kmi_extract_range_host / kmi_index_build_range_dist_host / kmi_dbg_build_range_dist_host take on a buffer that holds
the nominal range plus look-ahead. No GPU, no library: bytes and ints, written for reading rather than speed. Also the inputs
the range tests share."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden", "data")


def _is_eol(b):
    return b == 10 or b == 13


def _line_end(data, i):
    """the first EOL byte at or after i (len(data) if none): the loop `while i < n and not _is_eol(data[i]): i += 1`,
    as two searches so that a 31 KB line does not cost 31 K steps"""
    a, b = data.find(b"\n", i), data.find(b"\r", i)
    return min(x if x >= 0 else len(data) for x in (a, b))


def first_record_from(data, pos, starts_file=True):
    """first record start at or after byte `pos` of the buffer (len(data) if none is decidable inside the buffer).
    starts_file = False: byte 0 of the buffer lies somewhere inside the file, so position 0 is examined like any other"""
    n = len(data)
    if pos == 0 and starts_file:
        return 0
    if pos >= n:
        return n
    i = _line_end(data, pos)                # the rest of this (partial) line
    starts, firsts = [], []
    for _ in range(4):
        while i < n and _is_eol(data[i]):
            i += 1
        if i >= n:
            return n
        starts.append(i)
        firsts.append(data[i])
        i = _line_end(data, i)
    at, plus = ord("@"), ord("+")
    if firsts[0] == at and firsts[2] == plus:
        return starts[0]
    if firsts[1] == at and firsts[3] == plus:
        return starts[1]
    if firsts[0] == plus and firsts[2] == at:
        return starts[2]
    if firsts[1] == plus and firsts[3] == at:
        return starts[3]
    return n


def range_decision(buf, buffer_offset, nominal, reaches_eof):
    """the buffer holds file bytes [buffer_offset, buffer_offset + len(buf)); the rank's nominal range is its first `nominal`
    bytes. -> (need_more, cut0, cut1): the partition is buf[cut0:cut1], or need_more = 1 when its end is not decidable
    inside the buffer (then the cuts are None)"""
    n = len(buf)
    if n == 0:
        return 0, 0, 0
    nominal = min(nominal, n)
    starts_file = buffer_offset == 0
    cut0 = first_record_from(buf, 0, starts_file)
    cut1 = first_record_from(buf, nominal, starts_file)
    if nominal >= n:
        cut1 = n
    if not reaches_eof and (cut1 >= n or (cut0 >= n and buffer_offset != 0)):
        return 1, None, None
    if cut1 < cut0:
        cut1 = cut0
    return 0, cut0, cut1


def partition_of(data, lo, hi, look, grow=4):
    """what a rank that owns file bytes [lo, hi) ends up with when it reads `look` bytes of look-ahead and `grow` times more
    each time it is asked to: (begin, end, rounds), file positions"""
    n = len(data)
    rounds = 0
    while True:
        end = min(n, hi + look)
        need, c0, c1 = range_decision(data[lo:end], lo, hi - lo, end == n)
        rounds += 1
        if not need:
            return lo + c0, lo + c1, rounds
        look *= grow


def true_record_starts(data):
    """the byte offsets of lines 0, 4, 8, ... (a line ends with '\\n'; a '\\r' before it belongs to the line)"""
    out, pos = [], 0
    for i, line in enumerate(bytes(data).split(b"\n")):
        if i % 4 == 0 and pos < len(data):
            out.append(pos)
        pos += len(line) + 1
    return out


# ---- the inputs of the range tests
_QUALS = (b"@", b"+I", b"@+", b"I")   # quality lines that begin with '@', '+', '@+' (test_gpu_kmer_ops.py's `tricky` file)


def tricky(n_records=24, read_len=40, eol=b"\n", final_eol=True, seed=5):
    """records whose quality lines look like header and separator lines; random bases, so that every k-mer has its own place"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    recs = []
    for i in range(n_records):
        seq = letters[rng.integers(0, 4, read_len)].tobytes()
        q = _QUALS[i % 4]
        qual = (q * read_len)[:read_len]
        recs.append(b"@r%d" % i + eol + seq + eol + b"+" + eol + qual + eol)
    data = b"".join(recs)
    return data if final_eol else data[:len(data) - len(eol)]


def golden(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def small_inputs(n_records=24):
    """(label, bytes), each below 3 KB"""
    return [("tricky", tricky(n_records)), ("tricky-crlf", tricky(n_records, eol=b"\r\n")),
            ("tricky-no-final-eol", tricky(n_records, final_eol=False)), ("test.small.fastq", golden("test.small.fastq")),
            ("test.debruijn.tiny.fastq", golden("test.debruijn.tiny.fastq"))]
