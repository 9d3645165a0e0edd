"""Plain-Python model of clipping the tips of a de Bruijn node map (kmi_dbg_clip_tips; the definition is in include/kmerind_hip.h).

Nodes are a dict canonical k-mer string -> counts[9] (out A C G T, in A C G T, occurrences), as unitig_model.py and
dbg_clean_model.py take them. No GPU, no library: strings and dicts, written for reading."""
import numpy as np

from tests.dbg_clean_model import neighbour
from tests.unitig_model import BASES, Graph

STATS = ("n_nodes", "n_unitigs", "n_candidates", "n_tips_clipped", "n_islands", "n_islands_removed", "n_nodes_removed",
         "n_counters_cleared")
CLIP_ISLANDS = 1


def components(g):
    """the unitigs of Graph g as [(states, circular)]: states are (node, forward) in walking order; a path starts at one of its ends"""
    seen, out = set(), []
    for v0 in g.nodes:
        if v0 in seen:
            continue
        s, cyc = (v0, False), False   # backwards to the far end, or around a cycle
        while True:
            nx = g.step(*s)
            if nx is None:
                break
            if nx == (v0, False):
                cyc = True
                break
            s = nx
        states, s = [], ((v0, True) if cyc else (s[0], not s[1]))
        while s is not None and not (cyc and states and s == (v0, True)):
            states.append(s)
            s = g.step(*s)
        for v, _ in states:
            assert v not in seen, "a node in two unitigs"
            seen.add(v)
        out.append((states, cyc))
    assert len(seen) == len(g.nodes)
    return out


def _ends(states):
    """the two ends of a path unitig that its links do not use: (node, "out" / "in")"""
    (v0, f0), (v1, f1) = states[0], states[-1]
    return (v0, "in" if f0 else "out"), (v1, "out" if f1 else "in")


def clip(nodes, t, max_tip_nodes, flags=0, exists=False, trace=None):
    """(nodes, stats) after kmi_dbg_clip_tips(t, max_tip_nodes, flags), judged against `nodes` as given. exists: the counters are
    read as 0 / 1 (an EDGE_EXISTS map's export already shows them that way). trace: a list that receives, per candidate,
    (attached node, its counter, junction node, junction counter, number of nodes, clipped)"""
    assert t >= 1 and max_tip_nodes >= 1

    def read(c):
        return (1 if c else 0) if exists else c
    view = {v: [read(x) for x in c[:8]] + [c[8]] for v, c in nodes.items()}
    g = Graph(view, t)
    s = dict.fromkeys(STATS, 0)
    s["n_nodes"] = len(nodes)
    comps = components(g) if nodes else []
    s["n_unitigs"] = len(comps)
    gone, cands = set(), []   # cands: (states, junction node, junction counter)
    for states, cyc in comps:
        if cyc or len(states) > max_tip_nodes:
            continue
        ends = _ends(states)
        deg = [g.degree(*e) for e in ends]
        if deg == [0, 0]:
            s["n_islands"] += 1
            if flags & CLIP_ISLANDS:
                s["n_islands_removed"] += 1
                gone.update(v for v, _ in states)
            continue
        if sorted(deg) != [0, 1]:
            continue
        v, e = ends[deg.index(1)]
        lo = 0 if e == "out" else 4
        j = next(lo + b for b in range(4) if view[v][lo + b] >= t)
        w, recip, _ = neighbour(v, j)
        if w not in view or any(w == x for x, _ in states) or view[w][recip] < t:
            continue
        cands.append((states, w, recip, v, j))
    s["n_candidates"] = len(cands)
    named = {(w, j) for _, w, j, _, _ in cands}
    assert len(named) == len(cands), "a counter named by two candidates"

    def key(w, j):
        return (view[w][j], 0 if (w, j) in named else 1, -(j & 3))
    clear = []
    for states, w, j, v0, j0 in cands:
        lo = j & 4
        clipped = any(jj != j and view[w][jj] >= t and key(w, jj) > key(w, j) for jj in range(lo, lo + 4))
        if clipped:
            s["n_tips_clipped"] += 1
            gone.update(v for v, _ in states)
            clear.append((w, j))
        if trace is not None:
            trace.append((v0, j0, w, j, len(states), clipped))
    out = {v: list(c) for v, c in nodes.items() if v not in gone}
    for w, j in clear:
        if w in out:
            out[w][j] = 0
            s["n_counters_cleared"] += 1
    s["n_nodes_removed"] = len(nodes) - len(out)
    return out, s


# ---- test inputs
def rand_seq(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, n))


def other_base(b, step=1):
    return BASES[(BASES.index(b) + step) % 4]


def tip_reads(k, seed, tip_nodes, main=2, tip=1):
    """a random genome of 4 k bases read `main` times, and `tip` reads that follow it up to a substituted base and `tip_nodes` - 1
    bases further: a dead-end chain of tip_nodes nodes (tip_nodes <= k) hanging off the node in front of the substitution"""
    assert 1 <= tip_nodes <= k
    g = rand_seq(np.random.default_rng(seed), 4 * k)
    p = 2 * k + 3   # the substituted base
    r = g[p - k - 4:p] + other_base(g[p]) + g[p + 1:p + tip_nodes]
    return [g] * main + [r] * tip


def junction_reads(k, seed, branches, trunk=None):
    """a trunk of 3 k random bases whose last k-mer is followed by one branch per entry of `branches`: (base step 0..3 from a random
    base, nodes, weight). A branch of n nodes is a dead-end chain of n nodes read `weight` times; branches differ in their first
    base, so the trunk's last node is a junction of len(branches) counters"""
    rng = np.random.default_rng(seed)
    t = rand_seq(rng, 3 * k) if trunk is None else trunk
    b0 = BASES[int(rng.integers(0, 4))]
    reads = [t]
    for step, n, weight in branches:
        ext = rand_seq(rng, n - 1)
        reads += [t[-(k + 2):] + other_base(b0, step) + ext] * weight
    return reads

