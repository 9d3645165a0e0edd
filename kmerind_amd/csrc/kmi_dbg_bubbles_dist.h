// Popping the bubbles of a de Bruijn node map held over the ranks of a communicator (kmi_dbg_pop_bubbles_dist_host). The graph is
// the union of the ranks' node maps and the definition is the one of kmi_dbg_pop_bubbles (include/kmerind_hip.h), unchanged. What
// one lane of bubbles_classify and bubbles_judge reads from one memory lives on up to four ranks here -- a branch's two end nodes
// and its two junction nodes -- so every dependent load of the one-rank kernels becomes a record sent to the rank that holds the
// row, and a dense kernel over the records that arrived.
//
//   stages      ud_stages of kmi_unitig_dist.h: every node knows its unitig's two end states (global), its distances to them, and
//               circ. The unitig's identity is min(E0, E1); the end state with that value is the unitig's IDENTITY END, and its
//               owner is where the branch is assembled, counted and told its verdict.
//   junction    bubbles_dist_req: per END STATE e (a state without successor) of a path unitig of ANY length the owner reads the
//               degree of the end by which e leaves the unitig and, for degree 1, stages (canonical neighbour k-mer, own gs |
//               reciprocal counter << 48, unitig identity): (NW + 2) x 8 bytes, grouped by kmi_route_tuples_dev as the tips'
//               requests are, exchange. It does not wait to learn the far end's degree: that would cost an exchange of its own,
//               and the far end's degree comes with the pairing below. bubbles_dist_junction, at the owner of the neighbour w:
//               rule 2 for that end from its own rows (w is a node, w's identity is not the requester's, the reciprocal counter is
//               >= t) -> (requester's local state | counter value << 32, valid << 63 | (rank << 32 | w) << 3 | counter), 16 bytes,
//               back in arrival order. bubbles_dist_junction_set keeps the two words per end state.
//   pairing     bubbles_dist_pair_ask: the identity end, when its own junction is valid, asks the owner of the unitig's other end
//               state (other end's gs, own gs), 16 bytes, ud_group, exchange (a one-node unitig asks itself).
//               bubbles_dist_pair_tell answers (requester's local state, the other end's junction word, its counter value, the
//               canonical k-mer of that junction node): (NW + 3) x 8 bytes, back in arrival order; the junction word is 0 when
//               that end has another degree than 1 or no valid junction. The k-mer travels because rule 4's tie-break asks which
//               junction node has the smaller k-mer, and one of the two is remote.
//   matching    bubbles_dist_match_req, at the identity end: rule 2's last clause (the two junction nodes differ), the branch is
//               counted HERE. The junction node with the smaller k-mer is the branch's matching SITE; siblings share the pair of
//               junction ends, so they all arrive at one site. The request is (site's k-mer, v0, v1), (NW + 2) x 8 bytes, routed
//               by k-mer as the junction requests are:
//                 v0 = identity end's gs | site counter << 48 | far counter << 51 | far junction node's rank << 54 (8 bits: at
//                      most 256 ranks take part)
//                 v1 = far counter's value | far junction node << 32
//               At the site, TWO launches (workgroups of one launch do not see each other's writes). bubbles_dist_mark: lookup of
//               the site node w, slot[8 w + counter] = the arrived record's index -- a counter is named by at most one branch, so
//               a plain store of a word of its own; the word doubles as the candidate bit of the one-rank code. bubbles_dist_judge
//               reads only what the first launch wrote: per arrived branch the other marked counters of the same junction end of
//               w, the records that named them, whether their far junction end is this branch's, and the keys (min, max, -base):
//               the site's own counter values from its rows, the far ones from the records, and on a tie the base at the site,
//               which IS the junction node with the smaller k-mer, so no k-mer is loaded. The bubble is counted HERE, by the lane
//               of its greatest branch. Answer (identity end's local state, sibling | greater << 1), 16 bytes, arrival order.
//   verdict     bubbles_dist_verdict, at the identity end: M applies to the branch's own length only; a popped branch is counted
//               HERE, its identity end state gets the verdict "leaves", and two one-way records go to the owners of the two
//               junction nodes (junction node's forward gs | counter << 48), 16 bytes, ud_group, one exchange;
//               bubbles_dist_clear ORs the counter into the node's byte of `clr` (four nodes share a word: tips_set).
//   telling     bubbles_dist_ask: every node of a path unitig of at most M nodes asks the owner of its identity end ONCE (the
//               verdict lives at that end alone): 16 bytes out, 16 back, tips_dist_tell / tips_dist_gone as they are. Nodes of
//               longer unitigs and of cycles send nothing.
//   removal     tips_dist_retain_count / bucket_offsets / tips_dist_retain_compact / td_swap of kmi_dbg_tips_dist.h as they are.
//               A junction node usually lives on another rank than the branch, so a rank from which no node leaves can still have
//               counters to clear: it rewrites its rows. Only a rank with neither keeps its arrays.
// Nine exchanges after the stages': junction 2, pairing 2, matching 2, clears 1, telling 2. The verdict of each rank goes through
// dist_agree before every one of them (td_exchange) and once more when the fresh arrays are filled, before any map changes: all ranks
// swap, or none does. Stats reach the global words as one atomic per wavefront and word (prune_flush); request slots come from
// ud_wave_slot; 16-byte records are whole ulonglong2 loads and stores.
//
// Footprint per node beyond the stages: 32 bytes of slot words (one per counter), 32 of junction words (own and far, per state), 8 of
// junction counter values, 5 of per-state and per-node flags, 1 of clear mask; the request staging reuses the stages' end k-mers.
//
// Included by kmi_index.hip after kmi_dbg_tips_dist.h and kmi_dbg_bubbles.h.
#pragma once

namespace kmi {

// device words of a pop call over ranks (TD_CLEARED = 3 and TD_SURVIVORS = 4 are the removal's, kmi_dbg_tips_dist.h)
enum { BD_BRANCHES = 0, BD_BUBBLES = 1, BD_POPPED = 2, BD_REQ = 5, BD_MATCH = 6 };
constexpr uint64_t kBdValid = 1ull << 63;   // a junction word: valid << 63 | (rank << 32 | node) << 3 | counter
constexpr uint32_t kBdNoSlot = 0xFFFFFFFFu;

// the canonical k-mer behind counter jc of node q, and the reciprocal counter
template <int NW>
__device__ __forceinline__ uint32_t bd_neighbour(const uint64_t *__restrict__ keys, uint64_t q, uint32_t jc, const KShape &shape, uint64_t (&c)[NW]) {
  uint64_t key[NW], rc[NW];
  uni_load<NW>(keys, q, key);
  revcomp_words<NW, 2>(key, rc, shape);
  uint32_t recip;
  bool exempt;
  prune_neighbour<NW>(key, uni_eq<NW>(key, rc), jc, shape, c, &recip, &exempt);
  return recip;
}

// own[s] as in tips_dist_ends (degree, last counter >= t, kTdEnd) for the end states of path unitigs of any length; an end of
// degree 1 stages its junction request
template <int NW>
__global__ __launch_bounds__(256) void bubbles_dist_req_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ edges,
                                                              const UdRec *__restrict__ rec, const uint8_t *__restrict__ circ, uint64_t ns, KShape shape,
                                                              uint32_t me, uint32_t t, bool exists, uint8_t *__restrict__ own, uint64_t *__restrict__ req,
                                                              uint64_t cap, unsigned long long *__restrict__ stats) {
  for (uint64_t s0 = (uint64_t)blockIdx.x * blockDim.x; s0 < ns; s0 += (uint64_t)gridDim.x * blockDim.x) {   // (uniform per wavefront)
    const uint64_t s = s0 + threadIdx.x;
    bool send = false;
    uint32_t o = 0;
    uint64_t c[NW], val = 0, ident = 0;
    if (s < ns && rec[s].dist == 0ull && !circ[s >> 1]) {
      // state (q, o) leaves by q's out end (o = 0) or in end (o = 1), where base j of the strand read is in-counter comp(j)
      uint32_t e[8], deg = 0, jc = 0;
      uni_counters(edges, s >> 1, exists, e);
#pragma unroll
      for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t x = (s & 1u) ? 4u + 3u - j : j;
        if (e[x] >= t) { ++deg; jc = x; }
      }
      o = kTdEnd | deg | (jc << 3);
      if (deg == 1u) {
        const uint32_t recip = bd_neighbour<NW>(keys, s >> 1, jc, shape, c);
        const uint64_t mine = ud_gs(me, (uint32_t)s), far_gs = rec[s ^ 1ull].succ & kUdStateMask;
        ident = mine < far_gs ? mine : far_gs;
        val = mine | ((uint64_t)recip << 48);
        send = true;
      }
    }
    if (s < ns) own[s] = (uint8_t)o;
    const uint64_t slot = ud_wave_slot(stats + BD_REQ, send);
    if (send && slot < cap) {
#pragma unroll
      for (int w = 0; w < NW; ++w) req[slot * (NW + 2) + w] = c[w];
      req[slot * (NW + 2) + NW] = val;
      req[slot * (NW + 2) + NW + 1] = ident;
    }
  }
}

// rule 2 for one end, at the owner of the neighbour
template <int NW>
__global__ __launch_bounds__(256) void bubbles_dist_junction_kernel(const uint64_t *__restrict__ req, uint64_t n_req, const uint64_t *__restrict__ keys,
                                                                   const uint32_t *__restrict__ edges, uint64_t n, const uint32_t *__restrict__ tab,
                                                                   uint64_t mask, const UdRec *__restrict__ rec, uint32_t t, bool exists, uint32_t me,
                                                                   ulonglong2 *__restrict__ ans) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_req; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t key[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) key[w] = req[i * (NW + 2) + w];
    const uint64_t val = req[i * (NW + 2) + NW], ident = req[i * (NW + 2) + NW + 1];
    const uint32_t recip = (uint32_t)(val >> 48) & 7u;
    uint64_t x = (uint64_t)(uint32_t)val, y = 0;
    const uint32_t w = uni_lookup<NW>(keys, tab, mask, key);
    if (w != kNoNext && (uint64_t)w < n) {
      const uint64_t e0 = rec[2u * (uint64_t)w].succ & kUdStateMask, e1 = rec[2u * (uint64_t)w + 1u].succ & kUdStateMask;
      uint32_t f[8];
      uni_counters(edges, w, exists, f);
      if ((e0 < e1 ? e0 : e1) != ident && f[recip] >= t) {   // a node, not one of this unitig, reciprocated
        x |= (uint64_t)f[recip] << 32;
        y = kBdValid | (ud_gs(me, w) << 3) | recip;
      }
    }
    ans[i] = make_ulonglong2(x, y);
  }
}
__global__ __launch_bounds__(256) void bubbles_dist_junction_set_kernel(const ulonglong2 *__restrict__ ans, uint64_t n_ans, uint64_t *__restrict__ jw,
                                                                       uint32_t *__restrict__ jv, uint64_t ns) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ans; i += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 a = ans[i];
    const uint64_t s = (uint32_t)a.x;
    if (s < ns) { jw[s] = a.y; jv[s] = (uint32_t)(a.x >> 32); }
  }
}

// the identity end with a valid junction asks the other end for its junction
__global__ __launch_bounds__(256) void bubbles_dist_pair_ask_kernel(const UdRec *__restrict__ rec, const uint8_t *__restrict__ own,
                                                                   const uint64_t *__restrict__ jw, uint64_t ns, uint32_t me, ulonglong2 *__restrict__ stage) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * blockDim.x) {
    ulonglong2 out = make_ulonglong2(kUdNone, 0ull);
    if ((own[s] & kTdEnd) && (own[s] & 7u) == 1u && (jw[s] & kBdValid)) {
      const uint64_t mine = ud_gs(me, (uint32_t)s), far_gs = rec[s ^ 1ull].succ & kUdStateMask;
      if (mine < far_gs) out = make_ulonglong2(far_gs, mine);
    }
    stage[s] = out;
  }
}
// answer of NW + 3 words: requester's local state, junction word (0: none), counter value, the junction node's canonical k-mer
template <int NW>
__global__ __launch_bounds__(256) void bubbles_dist_pair_tell_kernel(const ulonglong2 *__restrict__ q, uint64_t n_q, const uint64_t *__restrict__ keys,
                                                                    const uint8_t *__restrict__ own, const uint64_t *__restrict__ jw,
                                                                    const uint32_t *__restrict__ jv, uint64_t ns, KShape shape, uint64_t *__restrict__ ans) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 r = q[i];
    const uint64_t e = (uint32_t)r.x;
    uint64_t *a = ans + i * (NW + 3);
    uint64_t c[NW] = {}, j = 0, v = 0;
    if (e < ns && (own[e] & kTdEnd) && (own[e] & 7u) == 1u && (jw[e] & kBdValid)) {
      (void)bd_neighbour<NW>(keys, e >> 1, ((uint32_t)own[e] >> 3) & 7u, shape, c);
      j = jw[e]; v = jv[e];
    }
    a[0] = (uint64_t)(uint32_t)r.y; a[1] = j; a[2] = v;
#pragma unroll
    for (int w = 0; w < NW; ++w) a[3 + w] = c[w];
  }
}

// at the identity end: the branch is assembled and counted, its far junction kept, and its matching request staged
template <int NW>
__global__ __launch_bounds__(256) void bubbles_dist_match_req_kernel(const uint64_t *__restrict__ ans, uint64_t n_ans, const uint64_t *__restrict__ keys,
                                                                    const uint8_t *__restrict__ own, const uint64_t *__restrict__ jw,
                                                                    const uint32_t *__restrict__ jv, uint64_t ns, KShape shape, uint32_t me,
                                                                    uint64_t *__restrict__ jo, uint64_t *__restrict__ req, uint64_t cap,
                                                                    unsigned long long *__restrict__ stats) {
  uint32_t n_br = 0;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n_ans; i0 += (uint64_t)gridDim.x * blockDim.x) {   // (uniform per wavefront)
    const uint64_t i = i0 + threadIdx.x;
    bool send = false;
    uint64_t c[NW], v0 = 0, v1 = 0;
    if (i < n_ans) {
      const uint64_t *a = ans + i * (NW + 3);
      const uint64_t s = a[0], far = a[1];
      if (s < ns && (far & kBdValid) && (jw[s] & kBdValid) && ((far ^ jw[s]) & ~kBdValid) >> 3 != 0ull) {   // two different junction nodes
        ++n_br;
        jo[s] = far;
        const uint64_t near = jw[s];
        uint64_t mine[NW], theirs[NW];
        (void)bd_neighbour<NW>(keys, s >> 1, ((uint32_t)own[s] >> 3) & 7u, shape, mine);
#pragma unroll
        for (int w = 0; w < NW; ++w) theirs[w] = a[3 + w];
        const bool far_site = less_words<NW>(theirs, mine);   // the junction node with the smaller k-mer hosts the matching
        const uint64_t site = far_site ? far : near, other = far_site ? near : far;
        const uint32_t other_val = far_site ? jv[s] : (uint32_t)a[2];
#pragma unroll
        for (int w = 0; w < NW; ++w) c[w] = far_site ? theirs[w] : mine[w];
        const uint64_t other_node = (other & ~kBdValid) >> 3;
        v0 = ud_gs(me, (uint32_t)s) | ((site & 7ull) << 48) | ((other & 7ull) << 51) | (((other_node >> 32) & 0xFFull) << 54);
        v1 = (uint64_t)other_val | ((other_node & 0xFFFFFFFFull) << 32);
        send = true;
      }
    }
    const uint64_t slot = ud_wave_slot(stats + BD_MATCH, send);
    if (send && slot < cap) {
#pragma unroll
      for (int w = 0; w < NW; ++w) req[slot * (NW + 2) + w] = c[w];
      req[slot * (NW + 2) + NW] = v0;
      req[slot * (NW + 2) + NW + 1] = v1;
    }
  }
  prune_flush(stats, BD_BRANCHES, n_br);
}

// at the site, first launch: which record names which counter. ans[i] = (identity end's local state, site node or kNoNext)
template <int NW>
__global__ __launch_bounds__(256) void bubbles_dist_mark_kernel(const uint64_t *__restrict__ req, uint64_t n_req, const uint64_t *__restrict__ keys, uint64_t n,
                                                               const uint32_t *__restrict__ tab, uint64_t mask, uint32_t *__restrict__ slot,
                                                               ulonglong2 *__restrict__ ans) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_req; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t key[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) key[w] = req[i * (NW + 2) + w];
    const uint64_t v0 = req[i * (NW + 2) + NW];
    uint32_t w = uni_lookup<NW>(keys, tab, mask, key);
    if (w != kNoNext && (uint64_t)w < n) slot[8u * (uint64_t)w + ((uint32_t)(v0 >> 48) & 7u)] = (uint32_t)i;
    else w = kNoNext;
    ans[i] = make_ulonglong2((uint64_t)(uint32_t)v0, (uint64_t)w);
  }
}
// second launch: rules 3-5 up to the length limit. out[i] = (identity end's local state, sibling | greater << 1)
template <int NW>
__global__ __launch_bounds__(256) void bubbles_dist_judge_kernel(const uint64_t *__restrict__ req, uint64_t n_req, const uint32_t *__restrict__ edges, uint64_t n,
                                                                bool exists, const uint32_t *__restrict__ slot, const ulonglong2 *__restrict__ marked,
                                                                ulonglong2 *__restrict__ out, unsigned long long *__restrict__ stats) {
  uint32_t n_bub = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_req; i += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 m = marked[i];
    const uint64_t w = m.y;
    bool sibling = false, greater = false;
    if (w < n) {
      const uint64_t v0 = req[i * (NW + 2) + NW], v1 = req[i * (NW + 2) + NW + 1];
      const uint32_t j = (uint32_t)(v0 >> 48) & 7u, lo = j & 4u;
      uint32_t f[8];
      uni_counters(edges, w, exists, f);
      const uint32_t c_far = (uint32_t)v1, mn = min(f[j], c_far), mx = max(f[j], c_far);
#pragma unroll
      for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t x = lo + b;
        if (x == j) continue;
        const uint32_t r = slot[8u * w + x];
        if (r == kBdNoSlot || (uint64_t)r >= n_req) continue;
        const uint64_t y0 = req[(uint64_t)r * (NW + 2) + NW], y1 = req[(uint64_t)r * (NW + 2) + NW + 1];
        if ((y0 >> 53) != (v0 >> 53) || (y1 >> 32) != (v1 >> 32)) continue;   // another far junction end: no sibling
        sibling = true;
        const uint32_t d_far = (uint32_t)y1, ymn = min(f[x], d_far), ymx = max(f[x], d_far);
        // on a tie the base at the junction node with the smaller k-mer decides: this node
        greater = greater || ymn > mn || (ymn == mn && (ymx > mx || (ymx == mx && (x & 3u) < (j & 3u))));
      }
    }
    n_bub += sibling && !greater ? 1u : 0u;
    out[i] = make_ulonglong2(m.x, (sibling ? 1ull : 0ull) | (greater ? 2ull : 0ull));
  }
  prune_flush(stats, BD_BUBBLES, n_bub);
}

// at the identity end: the length limit, the verdict of the end state, and the two clear records (stage[s] and stage[s ^ 1]: the
// other state of an identity end's node is never an identity end, and `stage` holds "none" everywhere else)
__global__ __launch_bounds__(256) void bubbles_dist_verdict_kernel(const ulonglong2 *__restrict__ ans, uint64_t n_ans, const UdRec *__restrict__ rec,
                                                                  const uint64_t *__restrict__ jw, const uint64_t *__restrict__ jo, uint64_t ns,
                                                                  uint32_t max_nodes, uint8_t *__restrict__ verdict, ulonglong2 *__restrict__ stage,
                                                                  unsigned long long *__restrict__ stats) {
  uint32_t n_pop = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ans; i += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 a = ans[i];
    const uint64_t s = a.x;
    if (s >= ns || !(a.y & 2ull) || rec[s ^ 1ull].dist + 1ull > (uint64_t)max_nodes) continue;
    ++n_pop;
    verdict[s] = 1u;
    const uint64_t j2[2] = {jw[s], jo[s]};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const uint64_t node = (j2[e] & ~kBdValid) >> 3;
      stage[s ^ (uint64_t)e] = make_ulonglong2((node & 0xFFFF00000000ull) | (uint64_t)(2u * (uint32_t)node) | ((j2[e] & 7ull) << 48), 0ull);
    }
  }
  prune_flush(stats, BD_POPPED, n_pop);
}
__global__ __launch_bounds__(256) void bubbles_dist_clear_kernel(const ulonglong2 *__restrict__ in, uint64_t n_in, uint32_t *__restrict__ clr, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t x = in[i].x, w = (uint64_t)((uint32_t)x >> 1);
    if (w < n) tips_set(clr, w, (uint32_t)(x >> 48) & 7u);
  }
}

// every node of a short path asks the owner of its unitig's identity end
__global__ __launch_bounds__(256) void bubbles_dist_ask_kernel(const UdRec *__restrict__ rec, const uint8_t *__restrict__ circ, uint64_t n, uint32_t me,
                                                              uint32_t max_nodes, ulonglong2 *__restrict__ stage) {
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t e0 = rec[2u * q].succ & kUdStateMask, e1 = rec[2u * q + 1u].succ & kUdStateMask;
    stage[q] = td_short_path(rec, circ, q, max_nodes) ? make_ulonglong2(e0 < e1 ? e0 : e1, ud_gs(me, 2u * (uint32_t)q)) : make_ulonglong2(kUdNone, 0ull);
  }
}

// ---- host side ----
// n_send staged requests of NW + 2 words go to the owners of their k-mers; `answer` launches the kernels that write one 16-byte
// answer per request that arrived (the buffer holds twice that many records: room for what a first launch leaves a second); the
// answers return in arrival order. pre: what this rank found wrong on its own since the last agreement
template <int NW, typename Answer>
static kmi_status bd_routed_trip(UdRun &u, kmi_status pre, const uint64_t *req_stage, uint64_t n_send, Answer answer, const ulonglong2 **got, uint64_t *n_got) {
  kmi_ctx *ctx = u.ctx;
  constexpr size_t rb = (NW + 2) * sizeof(uint64_t);
  void *d_send = nullptr, *d_req = nullptr, *d_ans = nullptr, *d_got = nullptr;
  std::vector<uint64_t> sc(u.p, 0), rc, rc2;
  uint64_t n_req = 0;
  kmi_status st = pre;
  if (st != KMI_OK) n_send = 0;
  if (st == KMI_OK) st = ws_get(ctx, WS_DIST_A, (size_t)(n_send + 64u) * rb, &d_send);
  if (st == KMI_OK && n_send) st = kmi_route_tuples_dev(ctx, &u.g->nodes->cfg, req_stage, (size_t)n_send, (uint32_t)u.p, 2, (uint64_t *)d_send, sc.data());
  if (st != KMI_OK) sc.assign(u.p, 0);
  KMI_TRY(td_exchange(u, st, d_send, sc, rb, WS_DIST_B, &d_req, rc, &n_req));
  st = ws_get(ctx, WS_DIST_C, (size_t)(2u * n_req + 8u) * sizeof(ulonglong2), &d_ans);
  if (st == KMI_OK && n_req) {
    answer((const uint64_t *)d_req, n_req, (ulonglong2 *)d_ans);
    if (hipGetLastError() != hipSuccess) st = set_err(ctx, KMI_ERR_DEVICE, "pop_bubbles: an answer kernel did not start");
  }
  KMI_TRY(td_exchange(u, st, d_ans, rc, sizeof(ulonglong2), WS_DIST_D, &d_got, rc2, n_got));
  *got = (const ulonglong2 *)d_got;
  if (*n_got != n_send) return set_err(ctx, KMI_ERR_DEVICE, "pop_bubbles: requests and answers do not add up");
  return KMI_OK;
}

// collective. pre: what this rank found wrong on its own so far; it still takes part until the verdicts are agreed on. stats: the
// eight words of kmi_dbg_pop_stats in its order, this rank's
template <int NW>
static kmi_status dbg_pop_dist_impl(kmi_dbg *g, kmi_comm *comm, uint32_t t, uint32_t max_nodes, kmi_status pre, uint64_t *stats) {
  kmi_ctx *ctx = g->ctx;
  kmi_index *idx = g->nodes;
  const bool exists = g->node_kind == KMI_DBG_EDGE_EXISTS;
  const uint64_t n = (idx->has_data && pre == KMI_OK) ? idx->n_entries : 0, ns = 2u * n, nw4 = (n + 3u) / 4u;
  const uint64_t *keys = (const uint64_t *)idx->keys;
  // the slot: device words; per state the own and the far junction word; survivors per fine bucket; the clear bytes (four nodes a
  // word); a record index per counter; per state the junction counter's value; then bytes: per state its own end and the verdict,
  // per node gone
  void *p_bub = nullptr;
  const size_t b_words = sizeof(unsigned long long) * TD_WORDS, b_junc = (size_t)ns * sizeof(uint64_t), b_cnt = sizeof(uint32_t) * kNumFine,
               b_mask = (size_t)nw4 * sizeof(uint32_t), b_slot = (size_t)n * 8u * sizeof(uint32_t), b_val = (size_t)ns * sizeof(uint32_t);
  const size_t b_all = b_words + 2u * b_junc + b_cnt + b_mask + b_slot + b_val + (size_t)2u * ns + (size_t)n + 16u;
  TdFresh fresh;
  kmi_status st = pre;
  if (st == KMI_OK) st = ws_get(ctx, WS_DBG_BUBBLES, b_all, &p_bub);
  if (st == KMI_OK && pool_alloc(ctx, (void **)&fresh.off, kOffBytes) != hipSuccess) st = set_err(ctx, KMI_ERR_NOMEM, "hipMalloc failed for the bucket offsets");
  unsigned long long *d_stats = (unsigned long long *)p_bub;
  uint64_t *jw = (uint64_t *)((char *)p_bub + b_words), *jo = jw + ns;
  uint32_t *out_cnt = (uint32_t *)(jo + ns);
  uint32_t *clr = out_cnt + kNumFine, *slot = clr + nw4, *jv = slot + 8u * n;
  uint8_t *own = (uint8_t *)(jv + ns), *verdict = own + ns, *gone = verdict + ns;
  if (st == KMI_OK && (hipMemsetAsync(p_bub, 0, b_all, ctx->stream) != hipSuccess ||
                       (n && hipMemsetAsync(slot, 0xFF, b_slot, ctx->stream) != hipSuccess)))
    st = set_err(ctx, KMI_ERR_DEVICE, "pop_bubbles: memset failed");
  UdStages s;
  st = ud_stages<NW>(g, comm, t, st, &s);   // (agrees on st before its first exchange)
  if (st != KMI_OK) { td_release(ctx, fresh); return st; }
  ctx->bubbles_dist_stage_exchanges = g->unitig_exchanges; ctx->bubbles_dist_stage_bytes = g->unitig_bytes_sent;   // (the stages' share)
  UdRun &u = s.u;
  const UdRec *rec = u.rec;
  const uint32_t *edges = (const uint32_t *)g->edges;
  const uint8_t *circ = (const uint8_t *)s.circ;
  auto fail = [&](kmi_status e) { td_release(ctx, fresh); return e; };
  auto launched = [&]() { return hipGetLastError() == hipSuccess ? KMI_OK : set_err(ctx, KMI_ERR_DEVICE, "pop_bubbles: a kernel did not start"); };
  // the number of requests a kernel staged through ud_wave_slot, at most `cap`
  auto staged = [&](kmi_status at, int word, uint64_t cap, uint64_t *out) {
    *out = 0;
    if (at != KMI_OK) return at;
    if (hipMemcpyAsync(out, d_stats + word, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
      *out = 0;
      return set_err(ctx, KMI_ERR_DEVICE, "pop_bubbles: the requests could not be counted");
    }
    if (*out > cap) { *out = 0; return set_err(ctx, KMI_ERR_DEVICE, "pop_bubbles: more requests than states"); }
    return KMI_OK;
  };
  const ulonglong2 *got = nullptr;
  uint64_t n_got = 0, n_send = 0;
  uint64_t *req_stage = s.endk;   // the stages' end k-mers: (ns + 8) x (NW + 2) words, no longer read

  // ---- junctions: two exchanges
  if (ns) {
    ProfScope ps(ctx, "bubbles_dist_req", ns);
    hipLaunchKernelGGL((bubbles_dist_req_kernel<NW>), dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, keys, edges, rec, circ, ns, g->shape, u.me, t, exists, own,
                       req_stage, ns, d_stats);
  }
  st = staged(launched(), BD_REQ, ns, &n_send);
  st = bd_routed_trip<NW>(u, st, req_stage, n_send, [&](const uint64_t *q, uint64_t n_q, ulonglong2 *a) {
    ProfScope ps(ctx, "bubbles_dist_junction", n_q);
    hipLaunchKernelGGL((bubbles_dist_junction_kernel<NW>), dim3(uni_grid(n_q)), dim3(256), 0, ctx->stream, q, n_q, keys, edges, n, (const uint32_t *)s.tab,
                       s.slots - 1u, rec, t, exists, u.me, a);
  }, &got, &n_got);
  if (st != KMI_OK) return fail(st);
  if (n_got) {
    ProfScope ps(ctx, "bubbles_dist_junction_set", n_got);
    hipLaunchKernelGGL(bubbles_dist_junction_set_kernel, dim3(uni_grid(n_got)), dim3(256), 0, ctx->stream, got, n_got, jw, jv, ns);
  }

  // ---- pairing: two exchanges, the answers (NW + 3) words wide
  if (ns) {
    ProfScope ps(ctx, "bubbles_dist_pair_ask", ns);
    hipLaunchKernelGGL(bubbles_dist_pair_ask_kernel, dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, rec, (const uint8_t *)own, (const uint64_t *)jw, ns, u.me, u.stage);
  }
  st = td_round_trip(u, "pop_bubbles", launched(), ns, (NW + 3) * sizeof(uint64_t), [&](const ulonglong2 *q, uint64_t n_q, void *a) {
    ProfScope ps(ctx, "bubbles_dist_pair_tell", n_q);
    hipLaunchKernelGGL((bubbles_dist_pair_tell_kernel<NW>), dim3(uni_grid(n_q)), dim3(256), 0, ctx->stream, q, n_q, keys, (const uint8_t *)own, (const uint64_t *)jw,
                       (const uint32_t *)jv, ns, g->shape, (uint64_t *)a);
  }, false, (const void **)&got, &n_got);
  if (st != KMI_OK) return fail(st);

  // ---- matching: two exchanges
  if (n_got) {
    ProfScope ps(ctx, "bubbles_dist_match_req", n_got);
    hipLaunchKernelGGL((bubbles_dist_match_req_kernel<NW>), dim3(uni_grid(n_got)), dim3(256), 0, ctx->stream, (const uint64_t *)got, n_got, keys, (const uint8_t *)own,
                       (const uint64_t *)jw, (const uint32_t *)jv, ns, g->shape, u.me, jo, req_stage, ns, d_stats);
  }
  st = staged(launched(), BD_MATCH, ns, &n_send);
  st = bd_routed_trip<NW>(u, st, req_stage, n_send, [&](const uint64_t *q, uint64_t n_q, ulonglong2 *a) {
    // the marks go beside the answers: the judge reads the one and writes the other
    ulonglong2 *marked = a + n_q;
    {
      ProfScope ps(ctx, "bubbles_dist_mark", n_q);
      hipLaunchKernelGGL((bubbles_dist_mark_kernel<NW>), dim3(uni_grid(n_q)), dim3(256), 0, ctx->stream, q, n_q, keys, n, (const uint32_t *)s.tab, s.slots - 1u, slot,
                         marked);
    }
    {
      ProfScope ps(ctx, "bubbles_dist_judge", n_q);
      hipLaunchKernelGGL((bubbles_dist_judge_kernel<NW>), dim3(uni_grid(n_q)), dim3(256), 0, ctx->stream, q, n_q, edges, n, exists, (const uint32_t *)slot,
                         (const ulonglong2 *)marked, a, d_stats);
    }
  }, &got, &n_got);
  if (st != KMI_OK) return fail(st);

  // ---- verdicts and clears: one exchange
  if (ns && hipMemsetAsync(u.stage, 0xFF, (size_t)ns * sizeof(ulonglong2), ctx->stream) != hipSuccess) st = set_err(ctx, KMI_ERR_DEVICE, "pop_bubbles: memset failed");
  if (st == KMI_OK && n_got) {
    ProfScope ps(ctx, "bubbles_dist_verdict", n_got);
    hipLaunchKernelGGL(bubbles_dist_verdict_kernel, dim3(uni_grid(n_got)), dim3(256), 0, ctx->stream, got, n_got, rec, (const uint64_t *)jw, (const uint64_t *)jo, ns,
                       max_nodes, verdict, u.stage, d_stats);
  }
  if (st == KMI_OK) st = launched();
  st = td_round_trip(u, "pop_bubbles", st, ns, sizeof(ulonglong2), [](const ulonglong2 *, uint64_t, void *) {}, true, (const void **)&got, &n_got);
  if (st != KMI_OK) return fail(st);
  if (n_got) {
    ProfScope ps(ctx, "bubbles_dist_clear", n_got);
    hipLaunchKernelGGL(bubbles_dist_clear_kernel, dim3(uni_grid(n_got)), dim3(256), 0, ctx->stream, got, n_got, clr, n);
  }

  // ---- the verdict to the nodes: two exchanges
  if (n) {
    ProfScope ps(ctx, "bubbles_dist_ask", n);
    hipLaunchKernelGGL(bubbles_dist_ask_kernel, dim3(uni_grid(n)), dim3(256), 0, ctx->stream, rec, circ, n, u.me, max_nodes, u.stage);
  }
  st = td_round_trip(u, "pop_bubbles", launched(), n, sizeof(ulonglong2), [&](const ulonglong2 *q, uint64_t n_q, void *a) {
    ProfScope ps(ctx, "tips_dist_tell", n_q);
    hipLaunchKernelGGL(tips_dist_tell_kernel, dim3(uni_grid(n_q)), dim3(256), 0, ctx->stream, q, n_q, (const uint8_t *)verdict, ns, (ulonglong2 *)a);
  }, false, (const void **)&got, &n_got);
  if (st != KMI_OK) return fail(st);
  if (n_got) {
    ProfScope ps(ctx, "tips_dist_gone", n_got);
    hipLaunchKernelGGL(tips_dist_gone_kernel, dim3(uni_grid(n_got)), dim3(256), 0, ctx->stream, got, n_got, gone, ns);
  }

  // ---- removal: the fresh arrays are filled before the last agreement, so all ranks swap or none does
  uint64_t h[8] = {0};
  st = launched();   // (what fails from here on is agreed on before the swap)
  if (st == KMI_OK && n) {
    {
      ProfScope ps(ctx, "tips_dist_retain_count", n);
      hipLaunchKernelGGL(tips_dist_retain_count_kernel, dim3(kNumFine / (kTipsCountThreads / kWave)), dim3(kTipsCountThreads), 0, ctx->stream,
                         (const uint8_t *)gone, (const uint32_t *)clr, (const uint64_t *)idx->bucket_off, out_cnt, d_stats);
    }
    {
      ProfScope ps(ctx, "tips_dist_offsets", kNumFine);
      hipLaunchKernelGGL(bucket_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t *)out_cnt, fresh.off, (uint64_t *)d_stats, (int)TD_SURVIVORS);
    }
    st = launched();
  }
  if (st == KMI_OK && (hipMemcpyAsync(h, d_stats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess))
    st = set_err(ctx, KMI_ERR_DEVICE, "pop_bubbles: the verdicts could not be read");
  const uint64_t total = n ? h[TD_SURVIVORS] : 0;
  if (st == KMI_OK && total > n) st = set_err(ctx, KMI_ERR_DEVICE, "pop_bubbles: more survivors than nodes");
  // a rank from which no node leaves can still have counters to clear (a junction node lives where its k-mer hashes to)
  const bool touched = st == KMI_OK && n && (total != n || h[TD_CLEARED] != 0);
  if (touched) {
    fresh.kb = (total ? total : 1) * NW * sizeof(uint64_t); fresh.vb = (total ? total : 1) * sizeof(uint32_t); fresh.rb = (total ? total : 1) * 8 * sizeof(uint32_t);
    const hipError_t e1 = pool_alloc(ctx, (void **)&fresh.keys, fresh.kb), e2 = pool_alloc(ctx, (void **)&fresh.vals, fresh.vb),
                     e3 = pool_alloc(ctx, (void **)&fresh.rows, fresh.rb);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) st = set_err(ctx, KMI_ERR_NOMEM, "hipMalloc failed for the node arrays");
    if (st == KMI_OK && total) {
      {
        ProfScope ps(ctx, "tips_dist_retain_compact", n);
        hipLaunchKernelGGL((tips_dist_retain_compact_kernel<NW>), dim3(kNumFine), dim3(kRetainTile), 0, ctx->stream, keys, (const uint32_t *)idx->vals,
                           (const uint64_t *)idx->bucket_off, (const uint8_t *)gone, (const uint32_t *)clr, (const uint64_t *)fresh.off, fresh.keys, fresh.vals,
                           (const uint4 *)g->edges, (uint4 *)fresh.rows);
      }
      st = launched();
      if (st == KMI_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = set_err(ctx, KMI_ERR_DEVICE, "pop_bubbles: the compaction failed");
    }
  }
  st = dist_agree(comm, st);   // before the swap: all ranks change their maps, or none does
  if (st != KMI_OK) return fail(st);
  if (touched) td_swap(g, fresh, total);
  else td_release(ctx, fresh);
  stats[0] = n; stats[1] = s.nu; stats[2] = h[BD_BRANCHES]; stats[3] = h[BD_BUBBLES]; stats[4] = h[BD_POPPED];
  stats[5] = n - total; stats[6] = h[TD_CLEARED]; stats[7] = 0;
  return KMI_OK;
}

// collective; stats_local / stats_total: eight words each
static kmi_status dbg_pop_bubbles_dist(kmi_dbg *g, kmi_comm *comm, uint32_t min_edge_count, uint32_t max_bubble_nodes, uint32_t flags, uint64_t *stats_local,
                                       uint64_t *stats_total) {
  kmi_ctx *ctx = g->ctx;
  memset(stats_local, 0, sizeof(uint64_t) * 8);
  memset(stats_total, 0, sizeof(uint64_t) * 8);
  // argument errors are every rank's alike: nothing collective has started
  if (g->shape.bits != 2) return set_err(ctx, KMI_ERR_INVALID, "pop_bubbles: only 2-bit alphabets");
  if (min_edge_count == 0) return set_err(ctx, KMI_ERR_INVALID, "pop_bubbles: min_edge_count must be at least 1");
  if (max_bubble_nodes == 0) return set_err(ctx, KMI_ERR_INVALID, "pop_bubbles: max_bubble_nodes must be at least 1");
  if (flags) return set_err(ctx, KMI_ERR_INVALID, "pop_bubbles: unknown flags");
  if ((uint32_t)comm_size(comm) > kUdMaxRanks) return set_err(ctx, KMI_ERR_INVALID, "pop_bubbles: more than 256 ranks");
  kmi_index *idx = g->nodes;
  kmi_status pre = KMI_OK;
  if (idx->has_data && idx->n_entries >= 0x7FFFFFFFull) pre = set_err(ctx, KMI_ERR_OVERFLOW, "pop_bubbles: more than 2^31 - 2 nodes on this rank");
  else if (idx->has_data && idx->n_entries) pre = ensure_dense(idx);
  // the stages count their exchanges in the graph, where the last compaction's are that call's to report
  const uint32_t rounds = g->unitig_rounds;
  const uint64_t exchanges = g->unitig_exchanges, bytes = g->unitig_bytes_sent;
  g->unitig_exchanges = 0; g->unitig_bytes_sent = 0;
  ctx->bubbles_dist_stage_exchanges = 0; ctx->bubbles_dist_stage_bytes = 0;
  kmi_status st = KMI_ERR_INVALID;
  switch (g->shape.n_words) {
    case 1: st = dbg_pop_dist_impl<1>(g, comm, min_edge_count, max_bubble_nodes, pre, stats_local); break;
    case 2: st = dbg_pop_dist_impl<2>(g, comm, min_edge_count, max_bubble_nodes, pre, stats_local); break;
    case 3: st = dbg_pop_dist_impl<3>(g, comm, min_edge_count, max_bubble_nodes, pre, stats_local); break;
    case 4: st = dbg_pop_dist_impl<4>(g, comm, min_edge_count, max_bubble_nodes, pre, stats_local); break;
  }
  ctx->bubbles_dist_exchanges = g->unitig_exchanges; ctx->bubbles_dist_bytes = g->unitig_bytes_sent;
  g->unitig_rounds = rounds; g->unitig_exchanges = exchanges; g->unitig_bytes_sent = bytes;
  if (st != KMI_OK) { memset(stats_local, 0, sizeof(uint64_t) * 8); return st; }
  dbg_unitigs_drop(g);   // (on every rank, whether it lost a node or not; a call that fails leaves the earlier compaction's result too)
  memcpy(stats_total, stats_local, sizeof(uint64_t) * 8);
  return comm_allreduce_sum(comm, stats_total, 8);
}

}  // namespace kmi
