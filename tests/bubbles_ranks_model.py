"""Plain-Python restatement of the PROTOCOL of kmi_dbg_pop_bubbles_dist_host (kmerind_amd/csrc/kmi_dbg_bubbles_dist.h): p simulated
ranks, an arbitrary owner(node) function, and no communication but lists of records between ranks, in the steps of the device code.
A rank reads its own rows and what arrived, nothing else. What the stages of kmi_dbg_compact_dist_host leave on every rank (per node
its unitig's two end states, its distances to them, circ) is given, computed from tips_model.components: that part has its own
model and tests.

Nodes are a dict canonical k-mer string -> counts[9], as bubbles_model.py takes them. States are global words rank << 32 | 2 *
(position on the rank) + (0 forward, 1 reverse), as on the device; records are tuples of such words, counter values and k-mer
strings."""
from tests.dbg_clean_model import neighbour
from tests.bubbles_model import STATS
from tests.tips_model import components
from tests.unitig_model import Graph


class _Rank:
    def __init__(self, me):
        self.me = me
        self.keys = []      # position -> k-mer
        self.pos = {}       # k-mer -> position (the rank's table)
        self.rows = {}      # k-mer -> the eight counters as the compaction reads them
        self.succ = {}      # local state -> (end state reached, distance): the stages' ranking records
        self.circ = {}      # position -> on a cycle
        self.own = {}       # end state -> (degree, counter): bubbles_dist_req
        self.jw = {}        # end state -> (junction node's global position, counter, value): bubbles_dist_junction_set
        self.jo = {}        # identity end -> the far junction: bubbles_dist_match_req
        self.verdict = set()
        self.clr = set()    # (position, counter)
        self.gone = set()   # positions
        self.stats = dict.fromkeys(STATS, 0)

    def gs(self, s):
        return (self.me << 32) | s


def _rank_of(gs):
    return gs >> 32


def _exchange(ranks, out):
    """out[r]: list of (destination rank, record) -> per rank the records that arrived, with their source, in source order"""
    got = [[] for _ in ranks]
    for src, recs in enumerate(out):
        for dst, rec in recs:
            got[dst].append((src, rec))
    return got


def _answers(ranks, got, answer):
    """the answers to what arrived go back to the sources in arrival order"""
    out = [[] for _ in ranks]
    for r, arrived in enumerate(got):
        for i, (src, rec) in enumerate(arrived):
            out[r].append((src, answer(ranks[r], i, rec)))
    return [[rec for _, rec in x] for x in _exchange(ranks, out)]


def stages(nodes, t, exists=False):
    """(the counters as the compaction reads them, the unitigs as tips_model.components gives them): the same for every placement"""
    def read(c):
        return (1 if c else 0) if exists else c
    view = {v: [read(x) for x in c[:8]] for v, c in nodes.items()}
    return view, (components(Graph(view, t)) if nodes else [])


def pop(nodes, t, max_bubble_nodes, p, owner, exists=False, staged=None):
    """(nodes after the call, total stats, local stats per rank, exchanges). staged: stages(nodes, t, exists), when the caller has it"""
    assert t >= 1 and max_bubble_nodes >= 1 and p >= 1
    view, comps = stages(nodes, t, exists) if staged is None else staged
    ranks = [_Rank(r) for r in range(p)]
    place = {}
    for v in nodes:
        rk = ranks[owner(v)]
        place[v] = (rk.me, len(rk.keys))
        rk.pos[v] = len(rk.keys)
        rk.keys.append(v)
        rk.rows[v] = view[v]

    # ---- what the stages leave: per state the end state it leads to and the distance; the unitig's owner counts it
    def state(v, fwd):
        r, i = place[v]
        return (r << 32) | (2 * i + (0 if fwd else 1))
    for states, cyc in comps:
        if cyc:
            for v, _ in states:
                ranks[place[v][0]].circ[place[v][1]] = True
            ranks[place[min(v for v, _ in states)][0]].stats["n_unitigs"] += 1
            continue
        first, last = state(states[0][0], not states[0][1]), state(*states[-1])
        ranks[_rank_of(min(first, last))].stats["n_unitigs"] += 1   # (the device counts a unitig where its head is: the sums agree)
        for i, (v, f) in enumerate(states):
            rk = ranks[place[v][0]]
            rk.succ[state(v, f) & 0xFFFFFFFF] = (last, len(states) - 1 - i)
            rk.succ[state(v, not f) & 0xFFFFFFFF] = (first, i)
    exchanges = 0
    for rk in ranks:
        rk.stats["n_nodes"] = len(rk.keys)

    # ---- junction: every end of degree 1 asks the owner of its neighbour
    out = [[] for _ in ranks]
    for rk in ranks:
        for s, (e, d) in sorted(rk.succ.items()):
            if d != 0:
                continue
            v, lo = rk.keys[s >> 1], 4 * (s & 1)
            live = [lo + b for b in range(4) if rk.rows[v][lo + b] >= t]
            rk.own[s] = (len(live), live[-1] if live else 0)
            if len(live) == 1:
                w, recip, _ = neighbour(v, live[0])
                far = rk.succ[s ^ 1][0]
                out[rk.me].append((owner(w), (w, rk.gs(s), recip, min(rk.gs(s), far))))

    def junction(rk, i, rec):
        w, frm, recip, ident = rec
        if w in rk.pos:
            q = rk.pos[w]   # (a node of a cycle is no node of the requester's unitig, which is a path)
            mine = None if rk.circ.get(q) else min(rk.succ[2 * q][0], rk.succ[2 * q + 1][0])
            if mine != ident and rk.rows[w][recip] >= t:
                return (frm & 0xFFFFFFFF, (rk.me << 32) | q, recip, rk.rows[w][recip])
        return (frm & 0xFFFFFFFF, None, 0, 0)
    got = _exchange(ranks, out)
    back = _answers(ranks, got, junction)
    exchanges += 2
    for rk in ranks:
        for s, node, ctr, val in back[rk.me]:
            if node is not None:
                rk.jw[s] = (node, ctr, val)

    # ---- pairing: the identity end asks the other end for its junction and that junction node's k-mer
    def nbr(rk, s):
        return neighbour(rk.keys[s >> 1], rk.own[s][1])[0]
    out = [[] for _ in ranks]
    for rk in ranks:
        for s in sorted(rk.jw):
            far = rk.succ[s ^ 1][0]
            if rk.own[s][0] == 1 and rk.gs(s) < far:
                out[rk.me].append((_rank_of(far), (far, rk.gs(s))))

    def pair_tell(rk, i, rec):
        e = rec[0] & 0xFFFFFFFF
        if rk.own.get(e, (0, 0))[0] == 1 and e in rk.jw:
            return (rec[1] & 0xFFFFFFFF, rk.jw[e], nbr(rk, e))
        return (rec[1] & 0xFFFFFFFF, None, None)
    back = _answers(ranks, _exchange(ranks, out), pair_tell)
    exchanges += 2

    # ---- matching: the branch goes to the owner of its junction node with the smaller k-mer
    out = [[] for _ in ranks]
    for rk in ranks:
        for s, far, far_kmer in back[rk.me]:
            if far is None or far[0] == rk.jw[s][0]:
                continue
            rk.stats["n_branches"] += 1
            rk.jo[s] = far
            near, near_kmer = rk.jw[s], nbr(rk, s)
            (site, site_kmer), other = ((far, far_kmer), near) if far_kmer < near_kmer else ((near, near_kmer), far)
            out[rk.me].append((owner(site_kmer), (site_kmer, rk.gs(s), site[1], other[0], other[1], other[2])))
    got = _exchange(ranks, out)
    slot = [dict() for _ in ranks]
    for rk in ranks:   # first launch: which record names which counter
        for i, (_, (kmer, _, ctr, _, _, _)) in enumerate(got[rk.me]):
            assert (rk.pos[kmer], ctr) not in slot[rk.me], "a counter named by two branches"
            slot[rk.me][(rk.pos[kmer], ctr)] = i

    def judge(rk, i, rec):   # second launch: reads the rank's rows and what the first wrote
        kmer, frm, j, o_node, o_ctr, o_val = rec
        w, row, lo = rk.pos[kmer], rk.rows[kmer], j & 4
        mine = (min(row[j], o_val), max(row[j], o_val), -(j & 3))
        sibling = greater = False
        for x in range(lo, lo + 4):
            r = slot[rk.me].get((w, x))
            if x == j or r is None:
                continue
            _, _, _, y_node, y_ctr, y_val = got[rk.me][r][1]
            if (y_node, y_ctr >> 2) != (o_node, o_ctr >> 2):
                continue
            sibling = True
            greater = greater or (min(row[x], y_val), max(row[x], y_val), -(x & 3)) > mine
        rk.stats["n_bubbles"] += 1 if sibling and not greater else 0
        return (frm & 0xFFFFFFFF, sibling, greater)
    back = _answers(ranks, got, judge)
    exchanges += 2

    # ---- verdicts and clears
    out = [[] for _ in ranks]
    for rk in ranks:
        for s, sibling, greater in back[rk.me]:
            if greater and rk.succ[s ^ 1][1] + 1 <= max_bubble_nodes:
                rk.stats["n_popped"] += 1
                rk.verdict.add(s)
                for node, ctr, _ in (rk.jw[s], rk.jo[s]):
                    out[rk.me].append((node >> 32, (node & 0xFFFFFFFF, ctr)))
    for rk, arrived in zip(ranks, _exchange(ranks, out)):
        rk.clr.update(rec for _, rec in arrived)
    exchanges += 1

    # ---- telling the nodes of short paths
    out = [[] for _ in ranks]
    for rk in ranks:
        for q in range(len(rk.keys)):
            if not rk.circ.get(q) and rk.succ[2 * q][1] + rk.succ[2 * q + 1][1] + 1 <= max_bubble_nodes:
                ident = min(rk.succ[2 * q][0], rk.succ[2 * q + 1][0])
                out[rk.me].append((_rank_of(ident), (ident, q)))
    back = _answers(ranks, _exchange(ranks, out), lambda rk, i, rec: (rec[1], (rec[0] & 0xFFFFFFFF) in rk.verdict))
    exchanges += 2
    for rk in ranks:
        rk.gone.update(q for q, leaves in back[rk.me] if leaves)

    # ---- removal
    after, total = {}, dict.fromkeys(STATS, 0)
    for rk in ranks:
        for q, v in enumerate(rk.keys):
            if q in rk.gone:
                continue
            row = list(nodes[v])
            for ctr in range(8):
                if (q, ctr) in rk.clr:
                    row[ctr] = 0
                    rk.stats["n_counters_cleared"] += 1
            after[v] = row
        rk.stats["n_nodes_removed"] = len(rk.gone)
        for f in STATS:
            total[f] += rk.stats[f]
    return after, total, [rk.stats for rk in ranks], exchanges
