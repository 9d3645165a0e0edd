"""Plain-Python model of de Bruijn node map compaction (kmi_dbg_compact; the definition is in include/kmerind_hip.h).

Input: canonical node keys and their counts[9] (out A C G T, in A C G T, occurrences), such as the oracle's
DbgMap.export(canonical=True), plus the threshold t = min_edge_count. Output: the sorted list of
(sequence, occurrences, circular). No GPU, no library: strings and dicts, written for reading rather than speed."""
import numpy as np

_COMP = str.maketrans("ACGT", "TGCA")
BASES = "ACGT"


def revcomp(s):
    return s.translate(_COMP)[::-1]


def canonical(s):
    r = revcomp(s)
    return s if s <= r else r


def decode_keys(keys, k):
    """(n, n_words) uint64 keys -> k-mer strings (base 0 in the most significant two bits)"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    keys = keys.reshape(keys.shape[0], -1)
    codes = np.empty((keys.shape[0], k), dtype=np.uint8)
    for i in range(k):
        b = 2 * (k - 1 - i)
        codes[:, i] = (keys[:, b // 64] >> np.uint64(b % 64)) & np.uint64(3)
    letters = np.frombuffer(BASES.encode(), dtype=np.uint8)[codes]
    return [x.decode() for x in np.ascontiguousarray(letters).view("S%d" % k).ravel()] if k else []


def encode_kmer(s, n_words):
    """k-mer string -> n_words uint64 words (the inverse of decode_keys)"""
    v = 0
    for c in s:
        v = (v << 2) | BASES.index(c)
    return np.array([(v >> (64 * w)) & ((1 << 64) - 1) for w in range(n_words)], dtype=np.uint64)


class Graph:
    """nodes: canonical k-mer -> counts[9]; the links of the definition"""

    def __init__(self, nodes, t=1):
        assert t >= 1
        self.nodes, self.t = nodes, t
        self.k = len(next(iter(nodes))) if nodes else 0

    def degree(self, v, end):
        c = self.nodes[v]
        lo = 0 if end == "out" else 4
        return sum(1 for b in range(4) if c[lo + b] >= self.t)

    def link(self, v, end):
        """the (node, entered end) the end of v links to, or None"""
        t, c = self.t, self.nodes[v]
        if v == revcomp(v):
            return None   # a palindrome links to nothing
        lo = 0 if end == "out" else 4
        bs = [b for b in range(4) if c[lo + b] >= t]
        if len(bs) != 1:
            return None
        x = v[1:] + BASES[bs[0]] if end == "out" else BASES[bs[0]] + v[:-1]
        w = canonical(x)
        if w not in self.nodes or w == v or w == revcomp(w):
            return None
        # the end of w that is entered, and the reciprocal base there
        if end == "out":
            e, base = ("in", v[0]) if w == x else ("out", BASES[3 - BASES.index(v[0])])
        else:
            e, base = ("out", v[-1]) if w == x else ("in", BASES[3 - BASES.index(v[-1])])
        cw = self.nodes[w]
        if self.degree(w, e) != 1 or cw[(0 if e == "out" else 4) + BASES.index(base)] < t:
            return None
        return (w, e)

    # oriented walking: state (v, fwd). Forward leaves by the out end, reverse by the in end.
    def step(self, v, fwd):
        r = self.link(v, "out" if fwd else "in")
        if r is None:
            return None
        w, e = r
        return (w, e == "in")

    def unitigs(self):
        k, seen, out = self.k, set(), []
        for v0 in self.nodes:
            if v0 in seen:
                continue
            # walk backwards (the reverse state) to the far end, or around a cycle
            s, cyc = (v0, False), False
            while True:
                nx = self.step(*s)
                if nx is None:
                    break
                if nx == (v0, False):
                    cyc = True
                    break
                s = nx
            if cyc:
                ring, s = [], (v0, True)
                while True:
                    ring.append(s)
                    s = self.step(*s)
                    if s == (v0, True):
                        break
                m = min(v for v, _ in ring)
                i = ring.index((m, True)) if (m, True) in ring else None
                if i is None:   # the ring as walked passes m reversed: walk it the other way from (m, forward)
                    ring, s = [], (m, True)
                    while True:
                        ring.append(s)
                        s = self.step(*s)
                        if s == (m, True):
                            break
                    i = 0
                states = ring[i:] + ring[:i]
            else:
                states, s = [], (s[0], not s[1])   # the far end, turned round
                while s is not None:
                    states.append(s)
                    s = self.step(*s)
            kms = [v if f else revcomp(v) for v, f in states]
            seq = kms[0] + "".join(x[-1] for x in kms[1:])
            assert len(seq) == len(states) + k - 1
            if not cyc:
                seq = min(seq, revcomp(seq))
            occ = 0
            for v, _ in states:
                assert v not in seen, "a node in two unitigs"
                seen.add(v)
                occ += int(self.nodes[v][8])
            out.append((seq, occ, cyc))
        assert len(seen) == len(self.nodes)
        return sorted(out)


def unitigs_from_strings(nodes, t=1):
    """nodes: dict canonical k-mer string -> counts[9]"""
    return Graph(nodes, t).unitigs() if nodes else []


def unitigs(keys, counts9, k, t=1):
    """the model on an exported node map: sorted [(sequence, occurrences, circular)]"""
    strs = decode_keys(keys, k)
    counts9 = np.asarray(counts9)
    nodes = {s: [int(x) for x in counts9[i]] for i, s in enumerate(strs)}
    for s in nodes:
        assert s == canonical(s), "the model takes canonical keys"
    return unitigs_from_strings(nodes, t)


def graph_of_reads(reads, k, exists=False):
    """a node map from reads (strings over ACGTN) as the library builds it from DNA: an N inside a window reads as A, an N
    neighbour counts for all four bases (DNA16 presence bits); nodes under their canonical strand with their edges turned"""
    nodes = {}
    for r in reads:
        for i in range(len(r) - k + 1):
            x = r[i:i + k].replace("N", "A")
            left = r[i - 1] if i > 0 else None
            right = r[i + k] if i + k < len(r) else None
            outs = [] if right is None else (list(range(4)) if right == "N" else [BASES.index(right)])
            ins = [] if left is None else (list(range(4)) if left == "N" else [BASES.index(left)])
            w = canonical(x)
            if w != x:   # the reverse strand: edges change sides, complemented
                outs, ins = [3 - b for b in ins], [3 - b for b in outs]
            c = nodes.setdefault(w, [0] * 9)
            for b in outs:
                c[b] += 1
            for b in ins:
                c[4 + b] += 1
            c[8] += 1
    if exists:
        for c in nodes.values():
            for j in range(8):
                c[j] = 1 if c[j] else 0
            c[8] = 0
    return nodes
