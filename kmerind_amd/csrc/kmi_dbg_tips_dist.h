// Clipping the tips of a de Bruijn node map held over the ranks of a communicator (kmi_dbg_clip_tips_dist_host). The graph is the
// union of the ranks' node maps and the definition is the one of kmi_dbg_clip_tips (include/kmerind_hip.h), unchanged; what changes
// is who can see what. A tip's nodes, its two end nodes and its junction node live on up to as many ranks as it has nodes + 1, so
// every rule that one lane of tips_classify reads from one memory becomes a record sent to the rank that holds the row.
//
//   stages      ud_stages of kmi_unitig_dist.h (links, ranking, cycle pass, ends, heads): every node knows its unitig's two end
//               states E0 = rec[2p].succ, E1 = rec[2p + 1].succ (global), its distances to them, and circ. The unitig's identity
//               is min(E0, E1): every node of it, on any rank, computes the same word.
//   ends        tips_dist_ends: per END STATE e (a state without successor) of a path unitig of at most M nodes, the owner reads the
//               degree of the end by which e leaves the unitig and, for degree 1, that end's counter. It sends the degree to the
//               owner of the other end state: (other end's gs | degree << 48, own gs), 16 bytes, grouped with ud_group, ONE exchange
//               (a one-node unitig's two end states are its node's two states: it talks to itself). tips_dist_ends_set stores what
//               arrived per state. Both ends then know: island (0, 0), possible candidate ({0, 1}), or neither.
//   request     tips_dist_req: an island is counted by the owner of the smaller of its two end states, and with
//               KMI_DBG_CLIP_ISLANDS both end states get the verdict "leaves". The degree-1 end of a possible candidate stages
//               (canonical neighbour k-mer, own gs | reciprocal counter << 48, unitig identity): (NW + 2) x 8 bytes, grouped by
//               kmi_route_tuples_dev as the pruning's requests are, exchange.
//   junction    the owner of the neighbour w, in TWO launches (workgroups of one launch do not see each other's writes, and rule 4
//               reads the candidate bits of every tip of the junction end: kmi_dbg_tips.h). tips_dist_junction: lookup, rule 3 (w
//               is a node, its identity is not the requester's, the reciprocal counter is >= t), ORs the candidate bit into w's
//               byte of `cand` and keeps (w, counter, candidate) in the answer's second word. tips_dist_judge: rule 4 from w's row
//               and `cand`; a clipped tip ORs its junction counter into w's byte of `clr`; the answer becomes (requester's local
//               state, candidate | clipped << 1), 16 bytes, back in arrival order: the second exchange of the pair.
//               tips_dist_verdict writes the attached end state's verdict and counts candidates and clipped tips THERE: on the rank
//               that holds the tip's attached (degree 1) end.
//   verdict     every node of a path unitig of at most M nodes asks the owners of BOTH of its unitig's end states (tips_dist_ask:
//               (end state, own gs) per state, 16 bytes, ud_group, exchange; tips_dist_tell answers (requester's local state,
//               verdict byte), 16 bytes back; tips_dist_gone) and leaves when either says so: an island's ends both know, a tip's
//               attached end knows, its dead end does not. Asking both costs a second record per node of a short unitig and saves
//               the forwarding exchange that an agreed end would need. Nodes of longer unitigs and of cycles send nothing.
//   removal     tips_dist_retain_count / tips_dist_offsets / tips_dist_retain_compact: the count -> bucket_offsets -> compact scheme
//               of tips_retain_* with the per-node `gone` byte as the predicate; the copied row is ANDed with the complement of the
//               node's clear byte. A junction node usually lives on another rank than the tip, so a rank from which no node leaves
//               can still have counters to clear: it rewrites its rows. Only a rank with neither keeps its arrays.
// Five exchanges after the stages'. The verdict of each rank goes through dist_agree before every one of them that follows a step
// of its own (grouping, routing, the answer buffer) and once more when the fresh arrays are filled, before any map changes: all
// ranks swap, or none does. Stats reach the global words as one atomic per wavefront and word (prune_flush); request slots come from
// ud_wave_slot; the masks hold four nodes a word (tips_set / tips_byte).
//
// Footprint per node beyond the stages: 7 bytes of per-state and per-node flags, 2 of masks; the request staging reuses the stages'
// end k-mers. What bubble popping over ranks (kmi_dbg_bubbles_dist.h) takes from here: td_round_trip (staged 16-byte questions to the
// owners of global states, answers back), tips_dist_tell / tips_dist_gone, the per-node removal kernels and td_swap.
//
// Included by kmi_index.hip after kmi_unitig_dist.h and kmi_dbg_tips.h.
#pragma once

namespace kmi {

// device words of a clip call over ranks
enum { TD_CAND = 0, TD_CLIPPED = 1, TD_ISLANDS = 2, TD_CLEARED = 3, TD_SURVIVORS = 4, TD_REQ = 5, TD_WORDS = 16 };
// a state's byte of `own`: bits 0..2 the degree of its leaving end, 3..5 the last counter >= t of that end, bit 7: an end state of a
// path unitig of at most M nodes
constexpr uint32_t kTdEnd = 0x80u;

__device__ __forceinline__ bool td_short_path(const UdRec *__restrict__ rec, const uint8_t *__restrict__ circ, uint64_t q, uint32_t max_nodes) {
  return !circ[q] && rec[2u * q].dist + rec[2u * q + 1u].dist + 1u <= (uint64_t)max_nodes;
}

__global__ __launch_bounds__(256) void tips_dist_ends_kernel(const uint32_t *__restrict__ edges, const UdRec *__restrict__ rec,
                                                            const uint8_t *__restrict__ circ, uint64_t ns, uint32_t me, uint32_t t, bool exists,
                                                            uint32_t max_nodes, uint8_t *__restrict__ own, ulonglong2 *__restrict__ stage) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t q = s >> 1;
    uint32_t o = 0;
    ulonglong2 out = make_ulonglong2(kUdNone, 0ull);
    if (rec[s].dist == 0ull && td_short_path(rec, circ, q, max_nodes)) {
      // state (q, o) leaves by q's out end (o = 0) or in end (o = 1), where base j of the strand read is in-counter comp(j)
      uint32_t e[8], deg = 0, jc = 0;
      uni_counters(edges, q, exists, e);
#pragma unroll
      for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t x = (s & 1u) ? 4u + 3u - j : j;
        if (e[x] >= t) { ++deg; jc = x; }
      }
      o = kTdEnd | deg | (jc << 3);
      out = make_ulonglong2((rec[s ^ 1ull].succ & kUdStateMask) | ((uint64_t)deg << 48), ud_gs(me, (uint32_t)s));
    }
    own[s] = (uint8_t)o;
    stage[s] = out;
  }
}
// other[e] = the degree of the far end + 1 (0: nothing arrived)
__global__ __launch_bounds__(256) void tips_dist_ends_set_kernel(const ulonglong2 *__restrict__ in, uint64_t n_in, uint8_t *__restrict__ other, uint64_t ns) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t x = in[i].x, e = (uint32_t)x;
    if (e < ns) other[e] = (uint8_t)(1u + ((uint32_t)(x >> 48) & 7u));
  }
}

// islands are settled here; the degree-1 end of a possible candidate stages its request (NW + 2 words)
template <int NW>
__global__ __launch_bounds__(256) void tips_dist_req_kernel(const uint64_t *__restrict__ keys, const UdRec *__restrict__ rec, uint64_t ns, KShape shape,
                                                           uint32_t me, bool islands, const uint8_t *__restrict__ own, const uint8_t *__restrict__ other,
                                                           uint8_t *__restrict__ verdict, uint64_t *__restrict__ req, uint64_t cap,
                                                           unsigned long long *__restrict__ stats) {
  uint32_t n_isl = 0;
  for (uint64_t s0 = (uint64_t)blockIdx.x * blockDim.x; s0 < ns; s0 += (uint64_t)gridDim.x * blockDim.x) {   // (uniform per wavefront)
    const uint64_t s = s0 + threadIdx.x;
    bool send = false;
    uint64_t c[NW], val = 0, ident = 0;
    if (s < ns && (own[s] & kTdEnd) && other[s] != 0u) {
      const uint32_t deg = own[s] & 7u, jc = (own[s] >> 3) & 7u, far = (uint32_t)other[s] - 1u;
      const uint64_t mine = ud_gs(me, (uint32_t)s), far_gs = rec[s ^ 1ull].succ & kUdStateMask;
      ident = mine < far_gs ? mine : far_gs;
      if (deg == 0u && far == 0u) {
        if (ident == mine) ++n_isl;
        if (islands) verdict[s] = 1u;
      } else if (deg == 1u && far == 0u) {
        uint64_t key[NW], rc[NW];
        uni_load<NW>(keys, s >> 1, key);
        revcomp_words<NW, 2>(key, rc, shape);
        uint32_t recip;
        bool exempt;
        prune_neighbour<NW>(key, uni_eq<NW>(key, rc), jc, shape, c, &recip, &exempt);
        val = mine | ((uint64_t)recip << 48);
        send = true;
      }
    }
    const uint64_t slot = ud_wave_slot(stats + TD_REQ, send);
    if (send && slot < cap) {
#pragma unroll
      for (int w = 0; w < NW; ++w) req[slot * (NW + 2) + w] = c[w];
      req[slot * (NW + 2) + NW] = val;
      req[slot * (NW + 2) + NW + 1] = ident;
    }
  }
  prune_flush(stats, TD_ISLANDS, n_isl);
}

// rule 3 at the junction's owner; ans[i] = (requester's local state, w << 8 | counter << 1 | candidate) for the second launch
template <int NW>
__global__ __launch_bounds__(256) void tips_dist_junction_kernel(const uint64_t *__restrict__ req, uint64_t n_req, const uint64_t *__restrict__ keys,
                                                                const uint32_t *__restrict__ edges, uint64_t n, const uint32_t *__restrict__ tab,
                                                                uint64_t mask, const UdRec *__restrict__ rec, uint32_t t, bool exists,
                                                                uint32_t *__restrict__ cand, ulonglong2 *__restrict__ ans) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_req; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t key[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) key[w] = req[i * (NW + 2) + w];
    const uint64_t val = req[i * (NW + 2) + NW], ident = req[i * (NW + 2) + NW + 1];
    const uint32_t recip = (uint32_t)(val >> 48) & 7u;
    uint64_t y = 0;
    const uint32_t w = uni_lookup<NW>(keys, tab, mask, key);
    if (w != kNoNext && (uint64_t)w < n) {
      const uint64_t e0 = rec[2u * (uint64_t)w].succ & kUdStateMask, e1 = rec[2u * (uint64_t)w + 1u].succ & kUdStateMask;
      uint32_t f[8];
      uni_counters(edges, w, exists, f);
      const bool is_cand = (e0 < e1 ? e0 : e1) != ident && f[recip] >= t;   // a node, not one of this unitig, reciprocated
      if (is_cand) tips_set(cand, w, recip);
      y = ((uint64_t)w << 8) | ((uint64_t)recip << 1) | (is_cand ? 1ull : 0ull);
    }
    ans[i] = make_ulonglong2((uint64_t)(uint32_t)val, y);
  }
}
// rule 4, as tips_judge_kernel applies it; ans[i].y becomes candidate | clipped << 1
__global__ __launch_bounds__(256) void tips_dist_judge_kernel(const uint32_t *__restrict__ edges, uint64_t n, uint32_t t, bool exists,
                                                             const uint32_t *__restrict__ cand, uint32_t *__restrict__ clr, ulonglong2 *__restrict__ ans,
                                                             uint64_t n_req) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_req; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t y = ans[i].y, w = y >> 8;
    const uint32_t j = (uint32_t)(y >> 1) & 7u, lo = j & 4u;
    bool clip = false;
    if ((y & 1ull) && w < n) {
      uint32_t f[8];
      uni_counters(edges, w, exists, f);
      const uint32_t bits = tips_byte(cand, w);
#pragma unroll
      for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t x = lo + b;
        if (x == j || f[x] < t) continue;
        const bool real = !((bits >> x) & 1u);   // (the candidate's own counter is not)
        clip = clip || f[x] > f[j] || (f[x] == f[j] && (real || x < j));
      }
      if (clip) tips_set(clr, w, j);
    }
    ans[i].y = (y & 1ull) | (clip ? 2ull : 0ull);
  }
}
// at the attached end: the verdict of its state, and the counts of candidates and clipped tips
__global__ __launch_bounds__(256) void tips_dist_verdict_kernel(const ulonglong2 *__restrict__ ans, uint64_t n_ans, uint8_t *__restrict__ verdict, uint64_t ns,
                                                               unsigned long long *__restrict__ stats) {
  uint32_t n_cand = 0, n_clip = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ans; i += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 a = ans[i];
    if (a.x >= ns) continue;
    n_cand += (uint32_t)(a.y & 1ull);
    if (a.y & 2ull) { ++n_clip; verdict[a.x] = 1u; }
  }
  prune_flush(stats, TD_CAND, n_cand);
  prune_flush(stats, TD_CLIPPED, n_clip);
}

// every state of a node of a short path asks the owner of the end state it leads to
__global__ __launch_bounds__(256) void tips_dist_ask_kernel(const UdRec *__restrict__ rec, const uint8_t *__restrict__ circ, uint64_t ns, uint32_t me,
                                                           uint32_t max_nodes, ulonglong2 *__restrict__ stage) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * blockDim.x)
    stage[s] = td_short_path(rec, circ, s >> 1, max_nodes) ? make_ulonglong2(rec[s].succ & kUdStateMask, ud_gs(me, (uint32_t)s))
                                                           : make_ulonglong2(kUdNone, 0ull);
}
__global__ __launch_bounds__(256) void tips_dist_tell_kernel(const ulonglong2 *__restrict__ req, uint64_t n_req, const uint8_t *__restrict__ verdict,
                                                            uint64_t ns, ulonglong2 *__restrict__ ans) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_req; i += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 q = req[i];
    const uint64_t e = (uint32_t)q.x;
    ans[i] = make_ulonglong2((uint64_t)(uint32_t)q.y, e < ns ? (uint64_t)verdict[e] : 0ull);
  }
}
// (two answers can name one node: both write the same byte value)
__global__ __launch_bounds__(256) void tips_dist_gone_kernel(const ulonglong2 *__restrict__ ans, uint64_t n_ans, uint8_t *__restrict__ gone, uint64_t ns) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ans; i += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 a = ans[i];
    if (a.x < ns && a.y) gone[a.x >> 1] = 1u;
  }
}

// ---- removal by a per-node byte: tips_retain_count_kernel / tips_retain_compact_kernel with the predicate "gone[i] == 0"
__global__ __launch_bounds__(kTipsCountThreads) void tips_dist_retain_count_kernel(const uint8_t *__restrict__ gone, const uint32_t *__restrict__ clr,
                                                                                  const uint64_t *__restrict__ idx_off, uint32_t *__restrict__ out_cnt,
                                                                                  unsigned long long *__restrict__ stats) {
  const uint32_t b = blockIdx.x * (kTipsCountThreads / kWave) + wave_id();   // (the grid is kNumFine wavefronts exactly)
  const uint64_t ib = idx_off[b], ie = idx_off[b + 1];
  uint32_t keep = 0, cleared = 0;
  for (uint64_t i = ib + lane_id(); i < ie; i += kWave) {
    if (gone[i]) continue;
    ++keep;
    cleared += (uint32_t)__popc(tips_byte(clr, i));
  }
  keep = wave_reduce_sum(keep);
  if (lane_id() == 0) out_cnt[b] = keep;
  prune_flush(stats, TD_CLEARED, cleared);
}
template <int NW>
__global__ __launch_bounds__(kRetainTile) void tips_dist_retain_compact_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                                              const uint64_t *__restrict__ idx_off, const uint8_t *__restrict__ gone,
                                                                              const uint32_t *__restrict__ clr, const uint64_t *__restrict__ new_off,
                                                                              uint64_t *__restrict__ new_keys, uint32_t *__restrict__ new_vals,
                                                                              const uint4 *__restrict__ rows, uint4 *__restrict__ new_rows) {
  __shared__ uint32_t s_scan[kRetainTile / kWave + 2];
  const uint32_t b = blockIdx.x;
  uint64_t dst = new_off[b];
  const uint64_t dst_end = new_off[b + 1];
  if (dst == dst_end) return;   // nothing of this bucket survives
  const uint64_t ib = idx_off[b], ie = idx_off[b + 1];
  for (uint64_t t0 = ib; t0 < ie; t0 += kRetainTile) {
    const uint64_t i = t0 + threadIdx.x;
    const bool keep = i < ie && !gone[i];
    uint32_t total;
    const uint32_t pos = block_exclusive_scan<uint32_t>(keep ? 1u : 0u, s_scan, &total);
    if (keep && dst + pos < dst_end) {   // (the bound holds by construction: the count pass saw the same nodes)
      const uint64_t o = dst + pos;
#pragma unroll
      for (int w = 0; w < NW; ++w) new_keys[o * NW + w] = keys[i * NW + w];
      new_vals[o] = vals[i];
      const uint32_t m = tips_byte(clr, i);
      uint4 r0 = rows[i * 2u], r1 = rows[i * 2u + 1u];
      r0.x = (m & 1u) ? 0u : r0.x; r0.y = (m & 2u) ? 0u : r0.y; r0.z = (m & 4u) ? 0u : r0.z; r0.w = (m & 8u) ? 0u : r0.w;
      r1.x = (m & 16u) ? 0u : r1.x; r1.y = (m & 32u) ? 0u : r1.y; r1.z = (m & 64u) ? 0u : r1.z; r1.w = (m & 128u) ? 0u : r1.w;
      new_rows[o * 2u] = r0; new_rows[o * 2u + 1u] = r1;
    }
    dst += total;
  }
}

// ---- host side ----
// grouped records to their owners once every rank's own step before it (`mine`) is agreed on
static kmi_status td_exchange(UdRun &u, kmi_status mine, const void *send, const std::vector<uint64_t> &sc, size_t elem_bytes, WsSlot slot, void **recv,
                              std::vector<uint64_t> &rc, uint64_t *total) {
  KMI_TRY(dist_agree(u.comm, mine));
  return ud_exchange(u, send, sc, elem_bytes, slot, recv, rc, total);
}

// The 16-byte questions staged in u.stage[0, n_staged) (first word: the global state asked, kUdNone: none) go to the owners of
// those states; `answer` launches the kernel that writes one 16-byte answer per question that arrived (questions, their number,
// answers); the answers return in arrival order: *got, *n_got. one_way: the questions are all there is (*got = what arrived).
// pre: what this rank found wrong on its own since the last agreement
// who: the call's name in the error texts; ans_bytes: the size of an answer (16, or wider: then `answer` and the caller read *got as words)
template <typename Answer>
static kmi_status td_round_trip(UdRun &u, const char *who, kmi_status pre, uint64_t n_staged, size_t ans_bytes, Answer answer, bool one_way, const void **got,
                                uint64_t *n_got) {
  kmi_ctx *ctx = u.ctx;
  ulonglong2 *grouped = nullptr;
  std::vector<uint64_t> sc(u.p, 0), rc, rc2;
  void *p_req = nullptr, *p_ans = nullptr, *p_got = nullptr;
  uint64_t n_req = 0;
  kmi_status st = pre;
  if (st == KMI_OK) st = ud_group(u, n_staged, &grouped, sc);
  KMI_TRY(td_exchange(u, st, grouped, sc, sizeof(ulonglong2), WS_DIST_B, &p_req, rc, &n_req));
  if (one_way) { *got = p_req; *n_got = n_req; return KMI_OK; }
  st = ws_get(ctx, WS_DIST_C, (size_t)(n_req + 8u) * ans_bytes, &p_ans);
  if (st == KMI_OK && n_req) {
    answer((const ulonglong2 *)p_req, n_req, p_ans);
    if (hipGetLastError() != hipSuccess) st = set_err(ctx, KMI_ERR_DEVICE, "%s: an answer kernel did not start", who);
  }
  KMI_TRY(td_exchange(u, st, p_ans, rc, ans_bytes, WS_DIST_D, &p_got, rc2, n_got));
  *got = p_got;
  return KMI_OK;
}

// the fresh arrays of a rank's surviving nodes
struct TdFresh {
  uint64_t *keys = nullptr, *off = nullptr; uint32_t *vals = nullptr, *rows = nullptr;
  size_t kb = 0, vb = 0, rb = 0;
};
static void td_release(kmi_ctx *ctx, TdFresh &f) {
  if (f.keys) pool_free(ctx, f.keys, f.kb);
  if (f.vals) pool_free(ctx, f.vals, f.vb);
  if (f.rows) pool_free(ctx, f.rows, f.rb);
  if (f.off) pool_free(ctx, f.off, kOffBytes);
  f = TdFresh{};
}
// the old arrays go back to the pool as in dbg_clip_impl (the index is dense here: no bucket_cnt)
static void td_swap(kmi_dbg *g, TdFresh &f, uint64_t total) {
  kmi_ctx *ctx = g->ctx;
  kmi_index *idx = g->nodes;
  pool_free(ctx, idx->keys, idx->keys_bytes);
  pool_free(ctx, idx->vals, idx->vals_bytes);
  pool_free(ctx, idx->bucket_off, kOffBytes);
  if (idx->dense_off) pool_free(ctx, idx->dense_off, kOffBytes);
  pool_free(ctx, g->edges, g->edges_bytes);
  idx->keys = f.keys; idx->vals = f.vals; idx->bucket_off = f.off; idx->dense_off = nullptr;
  idx->keys_bytes = f.kb; idx->vals_bytes = f.vb;
  idx->n_entries = total;
  g->edges = f.rows; g->edges_bytes = f.rb;
  f = TdFresh{};
}

// collective. pre: what this rank found wrong on its own so far; it still takes part until the verdicts are agreed on. stats: the
// eight words of kmi_dbg_clip_stats in its order, this rank's
template <int NW>
static kmi_status dbg_clip_dist_impl(kmi_dbg *g, kmi_comm *comm, uint32_t t, uint32_t max_nodes, uint32_t flags, kmi_status pre, uint64_t *stats) {
  kmi_ctx *ctx = g->ctx;
  kmi_index *idx = g->nodes;
  const bool exists = g->node_kind == KMI_DBG_EDGE_EXISTS;
  const bool islands = (flags & KMI_DBG_CLIP_ISLANDS) != 0;
  const uint64_t n = (idx->has_data && pre == KMI_OK) ? idx->n_entries : 0, ns = 2u * n, nw4 = (n + 3u) / 4u;
  const uint64_t *keys = (const uint64_t *)idx->keys;
  // the slot: device words, survivors per fine bucket, candidate and clear bytes (four nodes a word), then bytes: per state its own
  // end, the far end's degree and the verdict; per node gone
  void *p_tips = nullptr;
  const size_t b_words = sizeof(unsigned long long) * TD_WORDS, b_cnt = sizeof(uint32_t) * kNumFine, b_mask = (size_t)nw4 * sizeof(uint32_t);
  const size_t b_all = b_words + b_cnt + 2u * b_mask + (size_t)3u * ns + (size_t)n + 16u;
  TdFresh fresh;
  kmi_status st = pre;
  if (st == KMI_OK) st = ws_get(ctx, WS_DBG_TIPS, b_all, &p_tips);
  if (st == KMI_OK && pool_alloc(ctx, (void **)&fresh.off, kOffBytes) != hipSuccess) st = set_err(ctx, KMI_ERR_NOMEM, "hipMalloc failed for the bucket offsets");
  if (st == KMI_OK && hipMemsetAsync(p_tips, 0, b_all, ctx->stream) != hipSuccess) st = set_err(ctx, KMI_ERR_DEVICE, "clip_tips: memset failed");
  UdStages s;
  st = ud_stages<NW>(g, comm, t, st, &s);   // (agrees on st before its first exchange)
  if (st != KMI_OK) { td_release(ctx, fresh); return st; }
  UdRun &u = s.u;
  unsigned long long *d_stats = (unsigned long long *)p_tips;
  uint32_t *out_cnt = (uint32_t *)((char *)p_tips + b_words);
  uint32_t *cand = (uint32_t *)((char *)out_cnt + b_cnt), *clr = cand + nw4;
  uint8_t *own = (uint8_t *)(clr + nw4), *other = own + ns, *verdict = other + ns, *gone = verdict + ns;
  const UdRec *rec = u.rec;
  const uint32_t *edges = (const uint32_t *)g->edges;
  auto fail = [&](kmi_status e) { td_release(ctx, fresh); return e; };
  auto launched = [&]() { return hipGetLastError() == hipSuccess ? KMI_OK : set_err(ctx, KMI_ERR_DEVICE, "clip_tips: a kernel did not start"); };
  const ulonglong2 *got = nullptr;
  uint64_t n_got = 0;

  // ---- end degrees: one exchange
  if (ns) {
    ProfScope ps(ctx, "tips_dist_ends", ns);
    hipLaunchKernelGGL(tips_dist_ends_kernel, dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, edges, rec, (const uint8_t *)s.circ, ns, u.me, t, exists, max_nodes,
                       own, u.stage);
  }
  st = td_round_trip(u, "clip_tips", launched(), ns, sizeof(ulonglong2), [](const ulonglong2 *, uint64_t, void *) {}, true, (const void **)&got, &n_got);
  if (st != KMI_OK) return fail(st);
  if (n_got) {
    ProfScope ps(ctx, "tips_dist_ends_set", n_got);
    hipLaunchKernelGGL(tips_dist_ends_set_kernel, dim3(uni_grid(n_got)), dim3(256), 0, ctx->stream, got, n_got, other, ns);
  }

  // ---- junction requests and answers: two exchanges. The staging is the stages' end k-mers: (ns + 8) x (NW + 2) words, no longer read
  uint64_t *req_stage = s.endk;
  uint64_t n_send = 0;
  st = launched();
  if (st == KMI_OK && ns) {
    {
      ProfScope ps(ctx, "tips_dist_req", ns);
      hipLaunchKernelGGL((tips_dist_req_kernel<NW>), dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, keys, rec, ns, g->shape, u.me, islands, (const uint8_t *)own,
                         (const uint8_t *)other, verdict, req_stage, ns, d_stats);
    }
    st = launched();
    if (st == KMI_OK && (hipMemcpyAsync(&n_send, d_stats + TD_REQ, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                         hipStreamSynchronize(ctx->stream) != hipSuccess))
      st = set_err(ctx, KMI_ERR_DEVICE, "clip_tips: the requests could not be counted");
    if (st == KMI_OK && n_send > ns) st = set_err(ctx, KMI_ERR_DEVICE, "clip_tips: more requests than states");
    if (st != KMI_OK) n_send = 0;
  }
  {
    constexpr size_t rb = (NW + 2) * sizeof(uint64_t);
    void *d_send = nullptr, *d_req = nullptr, *d_ans = nullptr, *d_got = nullptr;
    std::vector<uint64_t> sc(u.p, 0), rc, rc2;
    uint64_t n_req = 0;
    if (st == KMI_OK) st = ws_get(ctx, WS_DIST_A, (size_t)(n_send + 64u) * rb, &d_send);
    if (st == KMI_OK && n_send) st = kmi_route_tuples_dev(ctx, &idx->cfg, req_stage, (size_t)n_send, (uint32_t)u.p, 2, (uint64_t *)d_send, sc.data());
    st = td_exchange(u, st, d_send, sc, rb, WS_DIST_B, &d_req, rc, &n_req);
    if (st != KMI_OK) return fail(st);
    st = ws_get(ctx, WS_DIST_C, (size_t)(n_req + 8u) * sizeof(ulonglong2), &d_ans);
    if (st == KMI_OK && n_req) {
      {
        ProfScope ps(ctx, "tips_dist_junction", n_req);
        hipLaunchKernelGGL((tips_dist_junction_kernel<NW>), dim3(uni_grid(n_req)), dim3(256), 0, ctx->stream, (const uint64_t *)d_req, n_req, keys, edges, n,
                           (const uint32_t *)s.tab, s.slots - 1u, rec, t, exists, cand, (ulonglong2 *)d_ans);
      }
      {
        ProfScope ps(ctx, "tips_dist_judge", n_req);
        hipLaunchKernelGGL(tips_dist_judge_kernel, dim3(uni_grid(n_req)), dim3(256), 0, ctx->stream, edges, n, t, exists, (const uint32_t *)cand, clr,
                           (ulonglong2 *)d_ans, n_req);
      }
      st = launched();
    }
    st = td_exchange(u, st, d_ans, rc, sizeof(ulonglong2), WS_DIST_D, &d_got, rc2, &n_got);
    if (st != KMI_OK) return fail(st);
    if (n_got != n_send) st = set_err(ctx, KMI_ERR_DEVICE, "clip_tips: requests and answers do not add up");
    if (st == KMI_OK && n_got) {
      ProfScope ps(ctx, "tips_dist_verdict", n_got);
      hipLaunchKernelGGL(tips_dist_verdict_kernel, dim3(uni_grid(n_got)), dim3(256), 0, ctx->stream, (const ulonglong2 *)d_got, n_got, verdict, ns, d_stats);
    }
  }

  // ---- the verdict to the nodes: two exchanges
  if (ns) {
    ProfScope ps(ctx, "tips_dist_ask", ns);
    hipLaunchKernelGGL(tips_dist_ask_kernel, dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, rec, (const uint8_t *)s.circ, ns, u.me, max_nodes, u.stage);
  }
  if (st == KMI_OK) st = launched();
  st = td_round_trip(u, "clip_tips", st, ns, sizeof(ulonglong2), [&](const ulonglong2 *q, uint64_t n_q, void *a) {
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
    st = set_err(ctx, KMI_ERR_DEVICE, "clip_tips: the verdicts could not be read");
  const uint64_t total = n ? h[TD_SURVIVORS] : 0;
  if (st == KMI_OK && total > n) st = set_err(ctx, KMI_ERR_DEVICE, "clip_tips: more survivors than nodes");
  // a rank from which no node leaves can still have counters to clear (a tip's junction node lives where its k-mer hashes to)
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
      if (st == KMI_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = set_err(ctx, KMI_ERR_DEVICE, "clip_tips: the compaction failed");
    }
  }
  st = dist_agree(comm, st);   // before the swap: all ranks change their maps, or none does
  if (st != KMI_OK) return fail(st);
  if (touched) td_swap(g, fresh, total);
  else td_release(ctx, fresh);
  stats[0] = n; stats[1] = s.nu; stats[2] = h[TD_CAND]; stats[3] = h[TD_CLIPPED]; stats[4] = h[TD_ISLANDS];
  stats[5] = islands ? h[TD_ISLANDS] : 0; stats[6] = n - total; stats[7] = h[TD_CLEARED];
  return KMI_OK;
}

// collective; stats_local / stats_total: eight words each
static kmi_status dbg_clip_tips_dist(kmi_dbg *g, kmi_comm *comm, uint32_t min_edge_count, uint32_t max_tip_nodes, uint32_t flags, uint64_t *stats_local,
                                     uint64_t *stats_total) {
  kmi_ctx *ctx = g->ctx;
  memset(stats_local, 0, sizeof(uint64_t) * 8);
  memset(stats_total, 0, sizeof(uint64_t) * 8);
  // argument errors are every rank's alike: nothing collective has started
  if (g->shape.bits != 2) return set_err(ctx, KMI_ERR_INVALID, "clip_tips: only 2-bit alphabets");
  if (min_edge_count == 0) return set_err(ctx, KMI_ERR_INVALID, "clip_tips: min_edge_count must be at least 1");
  if (max_tip_nodes == 0) return set_err(ctx, KMI_ERR_INVALID, "clip_tips: max_tip_nodes must be at least 1");
  if (flags & ~(uint32_t)KMI_DBG_CLIP_ISLANDS) return set_err(ctx, KMI_ERR_INVALID, "clip_tips: unknown flags");
  if ((uint32_t)comm_size(comm) > kUdMaxRanks) return set_err(ctx, KMI_ERR_INVALID, "clip_tips: more than 256 ranks");
  kmi_index *idx = g->nodes;
  kmi_status pre = KMI_OK;
  if (idx->has_data && idx->n_entries >= 0x7FFFFFFFull) pre = set_err(ctx, KMI_ERR_OVERFLOW, "clip_tips: more than 2^31 - 2 nodes on this rank");
  else if (idx->has_data && idx->n_entries) pre = ensure_dense(idx);
  // the stages count their exchanges in the graph, where the last compaction's are that call's to report
  const uint32_t rounds = g->unitig_rounds;
  const uint64_t exchanges = g->unitig_exchanges, bytes = g->unitig_bytes_sent;
  g->unitig_exchanges = 0; g->unitig_bytes_sent = 0;
  kmi_status st = KMI_ERR_INVALID;
  switch (g->shape.n_words) {
    case 1: st = dbg_clip_dist_impl<1>(g, comm, min_edge_count, max_tip_nodes, flags, pre, stats_local); break;
    case 2: st = dbg_clip_dist_impl<2>(g, comm, min_edge_count, max_tip_nodes, flags, pre, stats_local); break;
    case 3: st = dbg_clip_dist_impl<3>(g, comm, min_edge_count, max_tip_nodes, flags, pre, stats_local); break;
    case 4: st = dbg_clip_dist_impl<4>(g, comm, min_edge_count, max_tip_nodes, flags, pre, stats_local); break;
  }
  ctx->tips_dist_exchanges = g->unitig_exchanges; ctx->tips_dist_bytes = g->unitig_bytes_sent;
  g->unitig_rounds = rounds; g->unitig_exchanges = exchanges; g->unitig_bytes_sent = bytes;
  if (st != KMI_OK) { memset(stats_local, 0, sizeof(uint64_t) * 8); return st; }
  dbg_unitigs_drop(g);   // (on every rank, whether it lost a node or not; a call that fails leaves the earlier compaction's result too)
  memcpy(stats_total, stats_local, sizeof(uint64_t) * 8);
  return comm_allreduce_sum(comm, stats_total, 8);
}

}  // namespace kmi
