"""Plain-Python model of popping the bubbles of a de Bruijn node map (kmi_dbg_pop_bubbles; the definition is in
include/kmerind_hip.h).

Nodes are a dict canonical k-mer string -> counts[9] (out A C G T, in A C G T, occurrences), as unitig_model.py, dbg_clean_model.py
and tips_model.py take them. No GPU, no library: strings and dicts, written for reading."""
import numpy as np

from tests.dbg_clean_model import neighbour, prune
from tests.tips_model import _ends, clip, components, other_base, rand_seq
from tests.unitig_model import Graph, revcomp

STATS = ("n_nodes", "n_unitigs", "n_branches", "n_bubbles", "n_popped", "n_nodes_removed", "n_counters_cleared", "reserved")


def pop(nodes, t, max_bubble_nodes, exists=False, trace=None):
    """(nodes, stats) after kmi_dbg_pop_bubbles(t, max_bubble_nodes, 0), judged against `nodes` as given. exists: the counters are
    read as 0 / 1 (an EDGE_EXISTS map's export already shows them that way). trace: a list that receives, per branch that has a
    sibling, (junctions, key, number of nodes, popped); junctions are the branch's two (attached node, its counter, junction node,
    junction counter), the one at the smaller junction node first"""
    assert t >= 1 and max_bubble_nodes >= 1

    def read(c):
        return (1 if c else 0) if exists else c
    view = {v: [read(x) for x in c[:8]] + [c[8]] for v, c in nodes.items()}
    g = Graph(view, t)
    s = dict.fromkeys(STATS, 0)
    s["n_nodes"] = len(nodes)
    comps = components(g) if nodes else []
    s["n_unitigs"] = len(comps)
    branches = []   # (states, the two junctions)
    for states, cyc in comps:
        if cyc:
            continue
        ends = _ends(states)
        if [g.degree(*e) for e in ends] != [1, 1]:
            continue
        junctions = []
        for v, e in ends:
            lo = 0 if e == "out" else 4
            j = next(lo + b for b in range(4) if view[v][lo + b] >= t)
            w, recip, _ = neighbour(v, j)
            if w in view and not any(w == x for x, _ in states) and view[w][recip] >= t:
                junctions.append((v, j, w, recip))
        if len(junctions) == 2 and junctions[0][2] != junctions[1][2]:
            branches.append((states, sorted(junctions, key=lambda x: x[2])))
    s["n_branches"] = len(branches)
    named = [(w, j) for _, js in branches for _, _, w, j in js]
    assert len(set(named)) == len(named), "a counter named by two branches"
    families = {}   # the unordered pair of junction ends -> its branches
    for i, (states, js) in enumerate(branches):
        families.setdefault(frozenset((w, j >> 2) for _, _, w, j in js), []).append(i)

    def key(js):
        c = [view[w][j] for _, _, w, j in js]
        return (min(c), max(c), -(js[0][3] & 3))
    gone, clear = set(), []
    for family in families.values():
        if len(family) < 2:
            continue
        keys = [key(branches[i][1]) for i in family]
        assert len(set(keys)) == len(keys), "the key is not a total order within a bubble"
        s["n_bubbles"] += 1
        for i, ky in zip(family, keys):
            states, js = branches[i]
            popped = len(states) <= max_bubble_nodes and ky < max(keys)
            if popped:
                s["n_popped"] += 1
                gone.update(v for v, _ in states)
                clear += [(w, j) for _, _, w, j in js]
            if trace is not None:
                trace.append((js, ky, len(states), popped))
    out = {v: list(c) for v, c in nodes.items() if v not in gone}
    for w, j in clear:
        if w in out:
            out[w][j] = 0
            s["n_counters_cleared"] += 1
    s["n_nodes_removed"] = len(nodes) - len(out)
    return out, s


def clean_tips(nodes, t=1, max_tip_nodes=None, exists=False):
    """clip + prune rounds until a round clips nothing -> nodes"""
    k = len(next(iter(nodes)))
    while True:
        nodes, s = clip(nodes, t, 2 * k if max_tip_nodes is None else max_tip_nodes, 0, exists)
        nodes, _ = prune(nodes, t, exists)
        if s["n_tips_clipped"] == 0:
            return nodes


# ---- test inputs
def substitution_reads(k, seed, main=2, variant=1, step=1):
    """a random genome of 4 k bases read `main` times, and the same read `variant` times with base 2 k substituted: a bubble whose two
    branches have k nodes each"""
    g = rand_seq(np.random.default_rng(seed), 4 * k)
    return [g] * main + [g[:2 * k] + other_base(g[2 * k], step) + g[2 * k + 1:]] * variant


def deletion_reads(k, seed, main=2, variant=1):
    """... with base 2 k deleted (and its neighbours different, so that the deletion is not a shorter run of one letter): the
    variant's branch has k - 1 nodes, the genome's k"""
    rng = np.random.default_rng(seed)
    while True:
        g = rand_seq(rng, 4 * k)
        if g[2 * k - 1] != g[2 * k] != g[2 * k + 1]:
            return [g] * main + [g[:2 * k] + g[2 * k + 1:]] * variant


def three_way_reads(k, seed, weights=(3, 2, 1)):
    """the genome and two substitutions of the same base, read weights[i] times each: three siblings"""
    g = rand_seq(np.random.default_rng(seed), 4 * k)
    return [g[:2 * k] + other_base(g[2 * k], i) + g[2 * k + 1:] for i, w in enumerate(weights) for _ in range(w)]


def fuzz_reads(rng, k):
    """a random genome of 3 k + 2 ... 3 k + 30 bases read whole 1-3 times, plus 1-4 variants read 1-3 times on either strand; a
    variant is a window of the genome with one substitution, one deleted base or 1-3 inserted bases at least k bases from both ends
    of the window"""
    g = rand_seq(rng, int(rng.integers(3 * k + 2, 3 * k + 31)))
    reads = [g] * int(rng.integers(1, 4))
    for _ in range(int(rng.integers(1, 5))):
        a = int(rng.integers(0, len(g) - (2 * k + 1) + 1))
        w = g[a:int(rng.integers(a + 2 * k + 1, len(g) + 1))]
        p = int(rng.integers(k, len(w) - k))   # k bases in front, at least k behind
        kind = int(rng.integers(0, 3))
        if kind == 0:
            v = w[:p] + other_base(w[p], int(rng.integers(1, 4))) + w[p + 1:]
        elif kind == 1:
            v = w[:p] + w[p + 1:]
        else:
            v = w[:p] + rand_seq(rng, int(rng.integers(1, 4))) + w[p:]
        if rng.random() < 0.5:
            v = revcomp(v)
        reads += [v] * int(rng.integers(1, 4))
    return reads
