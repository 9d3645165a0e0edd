"""Plain-Python model of cleaning a de Bruijn node map (kmi_dbg_spectrum_* / kmi_dbg_retain_counts / kmi_dbg_prune_edges; the
definitions are in include/kmerind_hip.h).

Nodes are a dict canonical k-mer string -> counts[9] (out A C G T, in A C G T, occurrences), as unitig_model.py takes them, such as
the oracle's DbgMap.export(canonical=True) put through nodes_of(). No GPU, no library: strings and dicts, written for reading."""
import numpy as np

from tests.unitig_model import BASES, canonical, decode_keys, revcomp

STATS = ("n_nodes", "n_set_before", "n_weak", "n_absent", "n_unreciprocated", "n_set_after", "n_isolated", "n_requests")


def nodes_of(keys, counts9, k):
    """an exported node map -> dict canonical k-mer -> counts[9] (in export order)"""
    if np.asarray(keys).shape[0] == 0:
        return {}
    strs = decode_keys(keys, k)
    counts9 = np.asarray(counts9)
    nodes = {s: [int(x) for x in counts9[i]] for i, s in enumerate(strs)}
    for s in nodes:
        assert s == canonical(s), "the model takes canonical keys"
    return nodes


def spectrum(nodes, n_bins):
    """(hist[n_bins], totals) of counts[8]"""
    hist = [0] * n_bins
    occ = [c[8] for c in nodes.values()]
    for c in occ:
        hist[min(c, n_bins - 1)] += 1
    return hist, {"n_entries": len(occ), "sum_counts": sum(occ), "min_count": min(occ) if occ else 0, "max_count": max(occ) if occ else 0}


def retain(nodes, lo, hi):
    """the nodes with lo <= counts[8] <= hi, in their old order, with their counters as they are"""
    return {v: list(c) for v, c in nodes.items() if lo <= c[8] <= hi}


def _comp(b):
    return BASES[3 - BASES.index(b)]


def neighbour(v, j):
    """counter j of node v (0..3 out A C G T, 4..7 in A C G T) -> (w, index of the reciprocal counter in w's row, rule 3 exempt)"""
    b = BASES[j & 3]
    if j < 4:
        x, mine = v[1:] + b, v[0]
    else:
        x, mine = b + v[:-1], v[-1]
    w = canonical(x)
    if j < 4:   # (w, in, v[0]) or (w, out, comp(v[0]))
        recip = 4 + BASES.index(mine) if w == x else BASES.index(_comp(mine))
    else:       # (w, out, v[k-1]) or (w, in, comp(v[k-1]))
        recip = BASES.index(mine) if w == x else 4 + BASES.index(_comp(mine))
    return w, recip, v == revcomp(v) or x == revcomp(x)


def prune(nodes, t, exists=False):
    """(nodes, stats) after kmi_dbg_prune_edges with min_edge_count = t, judged against `nodes` as given. exists: the counters are
    read as 0 / 1 (an EDGE_EXISTS map's export already shows them that way)"""
    assert t >= 1

    def read(c):
        return (1 if c else 0) if exists else c
    out = {}
    s = dict.fromkeys(STATS, 0)
    s["n_nodes"] = len(nodes)
    for v, c in nodes.items():
        new = list(c)
        for j in range(8):
            e = read(c[j])
            if e == 0:
                continue
            s["n_set_before"] += 1
            if e < t:
                s["n_weak"] += 1
                new[j] = 0
                continue
            w, recip, exempt = neighbour(v, j)
            if w not in nodes:
                s["n_absent"] += 1
                new[j] = 0
            elif not exempt and read(nodes[w][recip]) < t:
                s["n_unreciprocated"] += 1
                new[j] = 0
        if not any(new[:8]):
            s["n_isolated"] += 1
        out[v] = new
    s["n_set_after"] = s["n_set_before"] - s["n_weak"] - s["n_absent"] - s["n_unreciprocated"]
    return out, s


def pipeline_reads(k):
    """(genome, reads) of the cleaning pipeline's test input: a 1500-base random genome tiled by error-free 100-base reads on both
    strands, plus 11 reads with one substitution each (base 50 or base 5 of the read changed to the next letter)"""
    rng = np.random.default_rng(k)
    genome = "".join(np.array(list(BASES))[rng.integers(0, 4, 1500)])
    reads = []
    for p in range(0, 1401, 10):
        r = genome[p:p + 100]
        reads += [r, revcomp(r)]
    for i, p in enumerate(range(40, 1400, 130)):
        r = list(genome[p:p + 100])
        at = 50 if i % 2 == 0 else 5
        r[at] = BASES[(BASES.index(r[at]) + 1) % 4]
        reads.append("".join(r))
    return genome, reads


def fastq(reads):
    return "".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads)).encode()


def n50(lengths):
    lengths = sorted(lengths, reverse=True)
    half, run = sum(lengths) / 2.0, 0
    for x in lengths:
        run += x
        if run >= half:
            return x
    return 0
