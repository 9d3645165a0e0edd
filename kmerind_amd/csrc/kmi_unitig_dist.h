// Unitigs of a de Bruijn node map held over the ranks of a communicator (kmi_dbg_compact_dist_host). The graph is the union of the
// ranks' node maps; the definition is the one of kmi_dbg_compact (include/kmerind_hip.h) plus the ownership rule written there. The
// helpers (table, k-mer arithmetic, counters, scan) are those of kmi_unitig.h; what changes is that a node's neighbour lives on
// another rank almost always (nodes are placed by KeyToRank of the canonical k-mer), so every step that follows a link is an
// exchange with kernels on both sides.
//
// STATES are global: gs = rank << 32 | local state (2p: node p forward, 2p + 1: reverse complement), 48 bits; kUdNone: none.
// Limits: at most 2^31 - 2 nodes per rank and 2^16 ranks in the encoding (KMI_ERR_OVERFLOW beyond); distances and occurrence sums are
// 64-bit words of their own, so they cannot wrap for a graph that fits. The grouping kernels keep one counter per rank in LDS and the
// link requests go through kmi_route_tuples_dev: 256 ranks at most (KMI_ERR_INVALID beyond), as for every other collective here.
//
//   links      unitig_dist_link_req: per node end of degree 1 the entered oriented k-mer v as unitig_links_kernel builds it ->
//              (canonical(v), requester gs | fwd << 48 | reciprocal base << 49), grouped by kmi_route_tuples_dev, exchange;
//              unitig_dist_link_ans: the owner looks v up in its unitig_table and applies rule 2 with its own counters -> (requester's
//              local state, entered gs or none); the answers leave in the order the requests arrived (grouped by source already),
//              exchange; unitig_dist_link_set writes next[]. Two exchanges of (NW + 1) x 8 and 16 bytes per node end of degree 1.
//   ranking    pointer jumping over global states in request / reply form, one launch per round per side: unitig_dist_jump_req stages
//              (successor gs, requester gs) for every state that is not done, unitig_dist_group_* groups the staged 16-byte records by
//              their explicit destination rank (count, offsets, scatter), exchange; unitig_dist_jump_ans reads the successor's record
//              -> (successor's successor | done << 63, distance, occurrence sum, requester's local state), exchange in arrival
//              order; unitig_dist_jump_set adds it up. A state is done once its successor is known to be terminal (the flag travels
//              with the reply) and sends nothing from then on. 48 bytes per state that still moves per round, two exchanges per
//              round. The number of rounds is global: ceil(log2(states of all ranks)) + 1 at most, an all-reduce of the "some
//              state is not done" flags every other round.
//   cycles     states not done at the bound lie on cycles; one all-reduce of their count, nothing else when it is 0. Else a second
//              jumping over those states only (unitig_dist_cycle_*) carries the candidate itself -- the smallest canonical k-mer seen
//              (NW words) and its forward global state -- because the key is remote; every cycle is cut in front of (m, forward) as
//              unitig_cut_kernel does, and the ranking resumes for the cut states.
//   ends       per state: the oriented k-mer its unitig ends with read the other way and the end node's occurrence count, from the
//              end state's owner (unitig_dist_end_*: one request per state, 16 bytes out, (NW + 2) x 8 back)
//   heads      unitig_dist_heads: direction, rank in the unitig, length; heads are counted and scanned locally (the scan kernels of
//              kmi_unitig.h): unitig ids and base offsets are rank-local, in the order of the heads' entries
//   emit       unitig_dist_emit: a head writes its k bases and the unitig's record; every other node stages (head's rank << 32 | head's
//              node, rank in unitig | letter << 62), grouped, one exchange; unitig_dist_emit_recv writes bases[offset(head) + k - 1 + r]
//
// Footprint per node of the rank: 8..16 bytes of table, 16 of next, 64 of ranking records, 16 of scan, 32..80 of staging (16 bytes
// per state; (NW + 1) x 8 per state for the link requests), (NW + 2) x 16 of end k-mers / cycle candidates, 2 of flags -- about 200
// bytes for one-word keys -- plus the exchange buffers (WS_DIST_A..D: what one exchange sends and receives, at most the staging size
// each way when the ranks are balanced) and the result owned by the graph.
#pragma once

namespace kmi {

constexpr uint64_t kUdNone = ~0ull;
constexpr uint64_t kUdStateMask = 0xFFFFFFFFFFFFull;   // rank << 32 | local state
constexpr uint32_t kUdMaxRanks = 256;                  // LDS counters of the grouping kernels

__device__ __forceinline__ uint64_t ud_gs(uint32_t rank, uint32_t s) { return ((uint64_t)rank << 32) | (uint64_t)s; }
__device__ __forceinline__ uint32_t ud_rank(uint64_t gs) { return (uint32_t)(gs >> 32) & 0xFFFFu; }

// a ranking record: the state reached so far (itself for a state without next), its distance, the occurrences of the nodes from the
// state up to there (exclusive), and whether that state is known to be the end of the chain
struct alignas(16) UdRec { uint64_t succ, dist, sum, done; };
__device__ __forceinline__ UdRec ud_rec(uint64_t self, uint64_t nx, uint64_t occ) {
  return nx == kUdNone ? UdRec{self, 0ull, 0ull, 1ull} : UdRec{nx, 1ull, occ, 0ull};
}

// position of this lane among the wavefront's lanes that add to the same counter; one atomic per distinct counter. Called by whole
// wavefronts (lanes with nothing to add pass valid = false).
__device__ __forceinline__ uint32_t ud_wave_add(uint32_t *ctr, uint32_t d, bool valid) {
  uint32_t slot = 0;
  unsigned long long todo = __ballot(valid);
  while (todo) {   // (uniform)
    const int lead = __ffsll((long long)todo) - 1;
    const uint32_t dl = (uint32_t)__shfl((int)d, lead);
    const bool mine = valid && d == dl;
    const unsigned long long m = __ballot(mine);
    uint32_t base = 0;
    if ((int)lane_id() == lead) base = atomicAdd(&ctr[dl], (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, lead);
    if (mine) slot = base + (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
    todo &= ~m;
  }
  return slot;
}
// ... to one 64-bit global counter
__device__ __forceinline__ uint64_t ud_wave_slot(unsigned long long *ctr, bool valid) {
  const unsigned long long m = __ballot(valid);
  unsigned long long base = 0;
  if (lane_id() == 0u && m) base = atomicAdd(ctr, (unsigned long long)__popcll(m));
  base = (unsigned long long)__shfl((long long)base, 0);
  return base + (uint64_t)__popcll(m & ((1ull << lane_id()) - 1ull));
}

// ---- grouping of staged 16-byte records by the destination rank in bits 32..47 of their first word (kUdNone: no record) ----
constexpr int kUdGroupNT = 256;
__host__ __device__ inline uint64_t ud_chunk(uint64_t n, uint32_t groups) { return ((n + groups - 1) / groups + kUdGroupNT - 1) / kUdGroupNT * kUdGroupNT; }

__global__ __launch_bounds__(kUdGroupNT) void unitig_dist_group_count_kernel(const ulonglong2 *__restrict__ in, uint64_t n, uint32_t p,
                                                                            unsigned long long *__restrict__ cnt) {
  __shared__ uint32_t s_hist[kUdMaxRanks];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t chunk = ud_chunk(n, gridDim.x), b0 = blockIdx.x * chunk, b1 = b0 + chunk < n ? b0 + chunk : n;
  for (uint64_t i0 = b0; i0 < b1; i0 += kUdGroupNT) {
    const uint64_t i = i0 + threadIdx.x;
    const uint64_t x = i < b1 ? in[i].x : kUdNone;
    const uint32_t d = ud_rank(x);
    (void)ud_wave_add(s_hist, d, x != kUdNone && d < p);
  }
  __syncthreads();
  if (threadIdx.x < p && s_hist[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
}
// one workgroup: cursor[r] = records for the ranks below r
__global__ __launch_bounds__(kUdGroupNT) void unitig_dist_group_offsets_kernel(const unsigned long long *__restrict__ cnt, uint32_t p,
                                                                              unsigned long long *__restrict__ cursor) {
  if (threadIdx.x == 0) {
    unsigned long long run = 0;
    for (uint32_t r = 0; r < p; ++r) { cursor[r] = run; run += cnt[r]; }
  }
}
__global__ __launch_bounds__(kUdGroupNT) void unitig_dist_group_scatter_kernel(const ulonglong2 *__restrict__ in, uint64_t n, uint32_t p,
                                                                              unsigned long long *__restrict__ cursor, ulonglong2 *__restrict__ out,
                                                                              uint64_t cap) {
  __shared__ uint32_t s_hist[kUdMaxRanks];
  __shared__ unsigned long long s_base[kUdMaxRanks];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t chunk = ud_chunk(n, gridDim.x), b0 = blockIdx.x * chunk, b1 = b0 + chunk < n ? b0 + chunk : n;
  for (uint64_t i0 = b0; i0 < b1; i0 += kUdGroupNT) {
    const uint64_t i = i0 + threadIdx.x;
    const uint64_t x = i < b1 ? in[i].x : kUdNone;
    const uint32_t d = ud_rank(x);
    (void)ud_wave_add(s_hist, d, x != kUdNone && d < p);
  }
  __syncthreads();
  if (threadIdx.x < p) {
    const uint32_t c = s_hist[threadIdx.x];
    s_base[threadIdx.x] = c ? atomicAdd(&cursor[threadIdx.x], (unsigned long long)c) : 0ull;
  }
  __syncthreads();
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t i0 = b0; i0 < b1; i0 += kUdGroupNT) {
    const uint64_t i = i0 + threadIdx.x;
    const ulonglong2 v = i < b1 ? in[i] : make_ulonglong2(kUdNone, 0ull);
    const uint32_t d = ud_rank(v.x);
    const bool valid = v.x != kUdNone && d < p;
    const uint32_t slot = ud_wave_add(s_hist, d, valid);
    if (valid) {
      const uint64_t pos = s_base[d] + slot;
      if (pos < cap) out[pos] = v;
    }
  }
}

// ---- links ----
// per node end of degree 1 whose entered k-mer v is no palindrome: (canonical(v), requester gs | fwd << 48 | reciprocal base << 49);
// next[] starts as "none" for every state
template <int NW>
__global__ __launch_bounds__(256) void unitig_dist_link_req_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ edges, uint64_t n,
                                                                  KShape shape, uint32_t t, bool exists, uint32_t me, uint64_t *__restrict__ req,
                                                                  uint64_t cap, unsigned long long *__restrict__ n_req, uint64_t *__restrict__ next) {
  const uint32_t k = shape.k;
  for (uint64_t p0 = (uint64_t)blockIdx.x * blockDim.x; p0 < n; p0 += (uint64_t)gridDim.x * blockDim.x) {   // (uniform per wavefront)
    const uint64_t p = p0 + threadIdx.x;
    const bool act = p < n;
    uint64_t key[NW], rc[NW];
    uint32_t e[8];
    bool pal = true;
    if (act) {
      uni_load<NW>(keys, p, key);
      revcomp_words<NW, 2>(key, rc, shape);
      pal = uni_eq<NW>(key, rc);
      uni_counters(edges, p, exists, e);
    }
#pragma unroll
    for (uint32_t o = 0; o < 2u; ++o) {
      bool send = false;
      uint64_t c[NW], val = 0;
      if (act) {
        uint32_t deg = 0, b = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
          const uint32_t cn = o ? e[4u + 3u - j] : e[j];
          if (cn >= t) { ++deg; b = j; }
        }
        if (!pal && deg == 1u) {
          const uint64_t(&u)[NW] = o ? rc : key;
          const uint32_t u0 = uni_base<NW>(u, 0u, k);
          uint64_t v[NW], vr[NW];
#pragma unroll
          for (int w = NW - 1; w >= 0; --w) v[w] = (u[w] << 2) | (w > 0 ? (u[w - 1] >> 62) : 0ull);
          v[0] |= b;
          mask_words<NW>(v, shape);
          revcomp_words<NW, 2>(v, vr, shape);
          const bool fwd = !less_words<NW>(vr, v);
          send = !uni_eq<NW>(v, vr);
#pragma unroll
          for (int w = 0; w < NW; ++w) c[w] = fwd ? v[w] : vr[w];
          val = ud_gs(me, 2u * (uint32_t)p + o) | ((uint64_t)(fwd ? 1u : 0u) << 48) | ((uint64_t)(fwd ? u0 : 3u - u0) << 49);
        }
        next[2u * p + o] = kUdNone;
      }
      const uint64_t slot = ud_wave_slot(n_req, send);
      if (send && slot < cap) {
#pragma unroll
        for (int w = 0; w < NW; ++w) req[slot * (NW + 1) + w] = c[w];
        req[slot * (NW + 1) + NW] = val;
      }
    }
  }
}
// the owner's side of rule 2: node present, not the requester's own node, entered end of degree 1, reciprocal counter >= t
template <int NW>
__global__ __launch_bounds__(256) void unitig_dist_link_ans_kernel(const uint64_t *__restrict__ req, uint64_t n_req, const uint64_t *__restrict__ keys,
                                                                  const uint32_t *__restrict__ edges, const uint32_t *__restrict__ tab, uint64_t mask,
                                                                  uint32_t t, bool exists, uint32_t me, ulonglong2 *__restrict__ ans) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_req; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t key[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) key[w] = req[i * (NW + 1) + w];
    const uint64_t val = req[i * (NW + 1) + NW], from = val & kUdStateMask;
    const bool fwd = (val >> 48) & 1ull;
    const uint32_t want = (uint32_t)(val >> 49) & 3u;
    uint64_t entered = kUdNone;
    const uint32_t w = uni_lookup<NW>(keys, tab, mask, key);
    if (w != kNoNext && !(ud_rank(from) == me && ((uint32_t)from >> 1) == w)) {
      uint32_t f[8];
      uni_counters(edges, w, exists, f);
      const uint32_t base = fwd ? 4u : 0u;
      uint32_t dw = 0;
#pragma unroll
      for (uint32_t j = 0; j < 4u; ++j) dw += f[base + j] >= t ? 1u : 0u;
      if (dw == 1u && f[base + want] >= t) entered = ud_gs(me, 2u * w + (fwd ? 0u : 1u));
    }
    ans[i] = make_ulonglong2((uint64_t)(uint32_t)from, entered);
  }
}
__global__ __launch_bounds__(256) void unitig_dist_link_set_kernel(const ulonglong2 *__restrict__ ans, uint64_t n_ans, uint64_t *__restrict__ next, uint64_t ns) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ans; i += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 a = ans[i];
    if (a.x < ns) next[a.x] = a.y;
  }
}

// ---- ranking ----
__global__ __launch_bounds__(256) void unitig_dist_rank_init_kernel(const uint64_t *__restrict__ next, const uint32_t *__restrict__ occ, uint64_t ns,
                                                                   uint32_t me, UdRec *__restrict__ rec) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * blockDim.x)
    rec[s] = ud_rec(ud_gs(me, (uint32_t)s), next[s], occ ? (uint64_t)occ[s >> 1] : 0ull);
}
// staged request of a state that is not done: (successor, requester)
__global__ __launch_bounds__(256) void unitig_dist_jump_req_kernel(const UdRec *__restrict__ rec, uint64_t ns, uint32_t me, ulonglong2 *__restrict__ stage) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * blockDim.x) {
    const UdRec a = rec[s];
    stage[s] = a.done ? make_ulonglong2(kUdNone, 0ull) : make_ulonglong2(a.succ, ud_gs(me, (uint32_t)s));
  }
}
struct alignas(16) UdReply { uint64_t succ_done, dist, sum, to; };
__global__ __launch_bounds__(256) void unitig_dist_jump_ans_kernel(const ulonglong2 *__restrict__ req, uint64_t n_req, const UdRec *__restrict__ rec,
                                                                  uint64_t ns, UdReply *__restrict__ ans) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_req; i += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 q = req[i];
    const uint64_t tgt = (uint32_t)q.x;
    UdRec b = UdRec{q.x & kUdStateMask, 0ull, 0ull, 1ull};   // (a target this rank does not have ends the chain: never the case)
    if (tgt < ns) b = rec[tgt];
    ans[i] = UdReply{b.succ | (b.done << 63), b.dist, b.sum, (uint64_t)(uint32_t)q.y};
  }
}
// *moved = 1 when some state is still not done
__global__ __launch_bounds__(256) void unitig_dist_jump_set_kernel(const UdReply *__restrict__ ans, uint64_t n_ans, UdRec *__restrict__ rec, uint64_t ns,
                                                                  uint32_t *__restrict__ moved) {
  bool mv = false;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ans; i += (uint64_t)gridDim.x * blockDim.x) {
    const UdReply b = ans[i];
    if (b.to >= ns) continue;
    const UdRec a = rec[b.to];
    const uint64_t done = b.succ_done >> 63;
    rec[b.to] = UdRec{b.succ_done & kUdStateMask, a.dist + b.dist, a.sum + b.sum, done};
    mv = mv || !done;
  }
  if (__any(mv) && lane_id() == 0u) *moved = 1u;
}

// ---- cycles: a record per state of NW + 2 words: pointer (kUdNone: not on a cycle), candidate's forward gs, candidate's key ----
template <int NW>
__global__ __launch_bounds__(256) void unitig_dist_cycle_init_kernel(const UdRec *__restrict__ rec, const uint64_t *__restrict__ next,
                                                                    const uint64_t *__restrict__ keys, uint64_t ns, uint32_t me, uint64_t *__restrict__ cyc) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t *c = cyc + s * (NW + 2);
    if (rec[s].done) { c[0] = kUdNone; continue; }
    c[0] = next[s];
    c[1] = ud_gs(me, 2u * (uint32_t)(s >> 1));
#pragma unroll
    for (int w = 0; w < NW; ++w) c[2 + w] = keys[(s >> 1) * NW + w];
  }
}
__global__ __launch_bounds__(256) void unitig_dist_count_moving_kernel(const UdRec *__restrict__ rec, uint64_t ns, unsigned long long *__restrict__ n_cyc) {
  for (uint64_t s0 = (uint64_t)blockIdx.x * blockDim.x; s0 < ns; s0 += (uint64_t)gridDim.x * blockDim.x) {   // (uniform per wavefront)
    const uint64_t s = s0 + threadIdx.x;
    const unsigned long long m = __ballot(s < ns && !rec[s < ns ? s : 0].done);
    if (m && lane_id() == 0u) atomicAdd(n_cyc, (unsigned long long)__popcll(m));
  }
}
template <int NW>
__global__ __launch_bounds__(256) void unitig_dist_cycle_req_kernel(const uint64_t *__restrict__ cyc, uint64_t ns, uint32_t me, ulonglong2 *__restrict__ stage) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t ptr = cyc[s * (NW + 2)];
    stage[s] = ptr == kUdNone ? make_ulonglong2(kUdNone, 0ull) : make_ulonglong2(ptr, ud_gs(me, (uint32_t)s));
  }
}
// reply of NW + 3 words: requester's local state, then the target's record
template <int NW>
__global__ __launch_bounds__(256) void unitig_dist_cycle_ans_kernel(const ulonglong2 *__restrict__ req, uint64_t n_req, const uint64_t *__restrict__ cyc,
                                                                   uint64_t ns, uint64_t *__restrict__ ans) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_req; i += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 q = req[i];
    const uint64_t tgt = (uint32_t)q.x;
    uint64_t *a = ans + i * (NW + 3);
    a[0] = (uint64_t)(uint32_t)q.y;
#pragma unroll
    for (int w = 0; w < NW + 2; ++w) a[1 + w] = tgt < ns ? cyc[tgt * (NW + 2) + w] : kUdNone;
  }
}
template <int NW>
__global__ __launch_bounds__(256) void unitig_dist_cycle_set_kernel(const uint64_t *__restrict__ ans, uint64_t n_ans, uint64_t *__restrict__ cyc, uint64_t ns) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ans; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t *a = ans + i * (NW + 3);
    const uint64_t s = a[0];
    if (s >= ns || a[1] == kUdNone) continue;
    uint64_t *c = cyc + s * (NW + 2);
    uint64_t ka[NW], kb[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) { ka[w] = c[2 + w]; kb[w] = a[3 + w]; }
    c[0] = a[1];
    if (less_words<NW>(kb, ka)) {
      c[1] = a[2];
#pragma unroll
      for (int w = 0; w < NW; ++w) c[2 + w] = kb[w];
    }
  }
}
// cut every cycle in front of (m, forward): (m, reverse) and the state that led into (m, forward) lose their next
template <int NW>
__global__ __launch_bounds__(256) void unitig_dist_cut_kernel(const uint64_t *__restrict__ cyc, uint64_t *__restrict__ next, UdRec *__restrict__ rec, uint64_t ns,
                                                             uint32_t me, const uint32_t *__restrict__ occ, uint8_t *__restrict__ circ) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t *c = cyc + s * (NW + 2);
    if (c[0] == kUdNone) continue;
    const uint64_t m = c[1], mine = ud_gs(me, 2u * (uint32_t)(s >> 1));
    uint64_t nx = next[s];
    if (mine == m ? (s & 1u) != 0u : nx == m) nx = kUdNone;
    next[s] = nx;
    rec[s] = ud_rec(ud_gs(me, (uint32_t)s), nx, occ ? (uint64_t)occ[s >> 1] : 0ull);
    if (!(s & 1u)) circ[s >> 1] = 1u;
  }
}

// ---- ends: per state, (occurrences of the end node, the k-mer of the end state read the other way): NW + 1 words ----
__global__ __launch_bounds__(256) void unitig_dist_end_req_kernel(const UdRec *__restrict__ rec, uint64_t ns, uint32_t me, ulonglong2 *__restrict__ stage) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * blockDim.x)
    stage[s] = make_ulonglong2(rec[s].succ & kUdStateMask, ud_gs(me, (uint32_t)s));
}
template <int NW>
__global__ __launch_bounds__(256) void unitig_dist_end_ans_kernel(const ulonglong2 *__restrict__ req, uint64_t n_req, const uint64_t *__restrict__ keys,
                                                                 const uint32_t *__restrict__ occ, uint64_t ns, KShape shape, uint64_t *__restrict__ ans) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_req; i += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 q = req[i];
    const uint32_t e = (uint32_t)q.x;
    uint64_t *a = ans + i * (NW + 2);
    uint64_t u[NW] = {};
    uint64_t oc = 0;
    if ((uint64_t)e < ns) {
      uni_state_kmer<NW>(keys, e ^ 1u, shape, u);
      oc = occ ? (uint64_t)occ[e >> 1] : 0ull;
    }
    a[0] = (uint64_t)(uint32_t)q.y;
    a[1] = oc;
#pragma unroll
    for (int w = 0; w < NW; ++w) a[2 + w] = u[w];
  }
}
template <int NW>
__global__ __launch_bounds__(256) void unitig_dist_end_set_kernel(const uint64_t *__restrict__ ans, uint64_t n_ans, uint64_t *__restrict__ endk, uint64_t ns) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ans; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t *a = ans + i * (NW + 2);
    if (a[0] >= ns) continue;
#pragma unroll
    for (int w = 0; w < NW + 1; ++w) endk[a[0] * (NW + 1) + w] = a[1 + w];
  }
}

// per node: the spelling direction (the one whose first k-mer is smaller), and (1, length in bases) for a head, (0, 0) for the others
template <int NW>
__global__ __launch_bounds__(256) void unitig_dist_heads_kernel(const UdRec *__restrict__ rec, const uint64_t *__restrict__ endk, uint64_t n, KShape shape,
                                                               ulonglong2 *__restrict__ scan, uint8_t *__restrict__ dir) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
    const UdRec a0 = rec[2u * p], a1 = rec[2u * p + 1u];
    uint64_t f0[NW], f1[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) { f0[w] = endk[(2u * p + 1u) * (NW + 1) + 1 + w]; f1[w] = endk[(2u * p) * (NW + 1) + 1 + w]; }
    const uint32_t d = less_words<NW>(f1, f0) ? 1u : 0u;
    const uint64_t r = d ? a0.dist : a1.dist;
    const uint64_t len = a0.dist + a1.dist + shape.k;
    scan[p] = r == 0u ? make_ulonglong2(1ull, len) : make_ulonglong2(0ull, 0ull);
    dir[p] = (uint8_t)d;
  }
}

// a head writes its k bases and its unitig's record; every other node stages (head's rank << 32 | head's node, r | letter << 62)
template <int NW>
__global__ __launch_bounds__(256) void unitig_dist_emit_kernel(const uint64_t *__restrict__ keys, const UdRec *__restrict__ rec, const uint64_t *__restrict__ endk,
                                                              uint64_t n, KShape shape, const ulonglong2 *__restrict__ scan, const uint8_t *__restrict__ dir,
                                                              const uint8_t *__restrict__ circ, uint32_t letters, char *__restrict__ bases, uint64_t nb,
                                                              uint64_t *__restrict__ u_off, uint64_t *__restrict__ u_occ, uint8_t *__restrict__ u_circ, uint64_t nu,
                                                              ulonglong2 *__restrict__ stage) {
  const uint32_t k = shape.k;
  auto letter = [&](uint32_t c) { return (char)(letters >> (8u * c)); };
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t d = dir[p];
    const UdRec ad = rec[2u * p + d], ao = rec[2u * p + 1u - d];
    uint64_t u[NW];
    uni_state_kmer<NW>(keys, 2u * (uint32_t)p + d, shape, u);
    if (ao.dist == 0u) {
      stage[p] = make_ulonglong2(kUdNone, 0ull);
      const ulonglong2 sc = scan[p];   // (unitig id, base offset)
      if (sc.x >= nu || sc.y + k > nb) continue;
      for (uint32_t i = 0; i < k; ++i) bases[sc.y + i] = letter(uni_base<NW>(u, i, k));
      u_off[sc.x] = sc.y;
      u_occ[sc.x] = ad.sum + endk[(2u * p + d) * (NW + 1)];
      u_circ[sc.x] = circ[p];
    } else {
      const uint64_t h = (ao.succ & kUdStateMask) ^ 1ull;   // the head's state in the spelling direction
      stage[p] = make_ulonglong2((h & 0xFFFF00000000ull) | (uint64_t)((uint32_t)h >> 1), ao.dist | ((uint64_t)((uint32_t)u[0] & 3u) << 62));
    }
  }
}
__global__ __launch_bounds__(256) void unitig_dist_emit_recv_kernel(const ulonglong2 *__restrict__ in, uint64_t n_in, const ulonglong2 *__restrict__ scan, uint64_t n,
                                                                   uint32_t k, uint32_t letters, char *__restrict__ bases, uint64_t nb, uint64_t nu) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 v = in[i];
    const uint64_t head = (uint32_t)v.x, r = v.y & ~(3ull << 62);
    if (head >= n) continue;
    const ulonglong2 sc = scan[head];
    const uint64_t pos = sc.y + k - 1u + r;
    if (sc.x < nu && pos >= sc.y && pos < nb) bases[pos] = (char)(letters >> (8u * (uint32_t)(v.y >> 62)));
  }
}

}  // namespace kmi

struct kmi_comm;
static kmi_status dist_agree(kmi_comm *comm, kmi_status mine);
static kmi_status dist_exchange(kmi_comm *comm, const void *send_dev, const uint64_t *send_counts, size_t elem_bytes, kmi::WsSlot slot, void **recv_dev,
                                std::vector<uint64_t> &recv_counts, uint64_t *total);

namespace kmi {

struct UdRun {   // what the phases of one compaction share
  kmi_dbg *g; kmi_comm *comm; kmi_ctx *ctx;
  int p; uint32_t me;
  uint64_t n, ns;
  ulonglong2 *stage;            // [ns] staged 16-byte records
  unsigned long long *d_cnt;    // [p] counts, [p] cursors, then scalars: [2p] link requests / cycle states, [2p + 1] moved (u32)
  UdRec *rec;
};

// an exchange of the compaction: dist_exchange, counted
static kmi_status ud_exchange(UdRun &u, const void *send, const std::vector<uint64_t> &sc, size_t elem_bytes, WsSlot slot, void **recv, std::vector<uint64_t> &rc,
                              uint64_t *total) {
  uint64_t sent = 0;
  for (int r = 0; r < u.p; ++r) sent += sc[r];
  ++u.g->unitig_exchanges;
  u.g->unitig_bytes_sent += sent * elem_bytes;
  return dist_exchange(u.comm, send, sc.data(), elem_bytes, slot, recv, rc, total);
}

// the staged records grouped by destination rank into WS_DIST_A; sc = records per rank
static kmi_status ud_group(UdRun &u, uint64_t n_staged, ulonglong2 **out, std::vector<uint64_t> &sc) {
  kmi_ctx *ctx = u.ctx;
  sc.assign(u.p, 0);
  void *pv;
  KMI_TRY(ws_get(ctx, WS_DIST_A, (size_t)(n_staged + 8u) * sizeof(ulonglong2), &pv));
  *out = (ulonglong2 *)pv;
  if (n_staged == 0) return KMI_OK;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n_staged + 4095u) / 4096u, 2048u);
  KMI_HIP(ctx, hipMemsetAsync(u.d_cnt, 0, sizeof(unsigned long long) * (size_t)u.p, ctx->stream));
  {
    ProfScope ps(ctx, "unitig_dist_group_count", n_staged);
    hipLaunchKernelGGL(unitig_dist_group_count_kernel, dim3(grid), dim3(kUdGroupNT), 0, ctx->stream, (const ulonglong2 *)u.stage, n_staged, (uint32_t)u.p, u.d_cnt);
  }
  {
    ProfScope ps(ctx, "unitig_dist_group_offsets", (uint64_t)u.p);
    hipLaunchKernelGGL(unitig_dist_group_offsets_kernel, dim3(1), dim3(kUdGroupNT), 0, ctx->stream, (const unsigned long long *)u.d_cnt, (uint32_t)u.p, u.d_cnt + u.p);
  }
  {
    ProfScope ps(ctx, "unitig_dist_group_scatter", n_staged);
    hipLaunchKernelGGL(unitig_dist_group_scatter_kernel, dim3(grid), dim3(kUdGroupNT), 0, ctx->stream, (const ulonglong2 *)u.stage, n_staged, (uint32_t)u.p,
                       u.d_cnt + u.p, *out, n_staged);
  }
  KMI_HIP(ctx, hipGetLastError());
  KMI_HIP(ctx, hipMemcpyAsync(sc.data(), u.d_cnt, sizeof(uint64_t) * (size_t)u.p, hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KMI_OK;
}

// staged requests -> grouped -> the owners (WS_DIST_B); *n_req of them arrived, from rc[r] each
static kmi_status ud_send_requests(UdRun &u, uint64_t n_staged, const ulonglong2 **req, uint64_t *n_req, std::vector<uint64_t> &rc) {
  ulonglong2 *grouped;
  std::vector<uint64_t> sc;
  KMI_TRY(ud_group(u, n_staged, &grouped, sc));
  void *pv;
  KMI_TRY(ud_exchange(u, grouped, sc, sizeof(ulonglong2), WS_DIST_B, &pv, rc, n_req));
  *req = (const ulonglong2 *)pv;
  return KMI_OK;
}

// pointer jumping until no state moves anywhere or the bound is reached
static kmi_status ud_rank_rounds(UdRun &u, uint32_t bound) {
  kmi_ctx *ctx = u.ctx;
  uint32_t *d_moved = (uint32_t *)(u.d_cnt + 2 * u.p + 1);
  for (uint32_t r = 0; r < bound; ++r) {
    const bool check = (r & 1u) || r + 1u == bound;
    if (check) KMI_HIP(ctx, hipMemsetAsync(d_moved, 0, sizeof(uint32_t), ctx->stream));
    if (u.ns) {
      ProfScope ps(ctx, "unitig_dist_jump_req", u.ns);
      hipLaunchKernelGGL(unitig_dist_jump_req_kernel, dim3(uni_grid(u.ns)), dim3(256), 0, ctx->stream, (const UdRec *)u.rec, u.ns, u.me, u.stage);
    }
    const ulonglong2 *req; uint64_t n_req = 0, n_ans = 0;
    std::vector<uint64_t> rc, rc2;
    KMI_TRY(ud_send_requests(u, u.ns, &req, &n_req, rc));
    void *p_ans, *p_got;
    KMI_TRY(ws_get(ctx, WS_DIST_C, (size_t)(n_req + 8u) * sizeof(UdReply), &p_ans));
    if (n_req) {
      ProfScope ps(ctx, "unitig_dist_jump_ans", n_req);
      hipLaunchKernelGGL(unitig_dist_jump_ans_kernel, dim3(uni_grid(n_req)), dim3(256), 0, ctx->stream, req, n_req, (const UdRec *)u.rec, u.ns, (UdReply *)p_ans);
    }
    KMI_HIP(ctx, hipGetLastError());
    KMI_TRY(ud_exchange(u, p_ans, rc, sizeof(UdReply), WS_DIST_D, &p_got, rc2, &n_ans));
    if (n_ans) {
      ProfScope ps(ctx, "unitig_dist_jump_set", n_ans);
      hipLaunchKernelGGL(unitig_dist_jump_set_kernel, dim3(uni_grid(n_ans)), dim3(256), 0, ctx->stream, (const UdReply *)p_got, n_ans, u.rec, u.ns, d_moved);
    }
    KMI_HIP(ctx, hipGetLastError());
    ++u.g->unitig_rounds;
    if (check) {
      uint32_t moved = 0;
      KMI_HIP(ctx, hipMemcpyAsync(&moved, d_moved, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
      KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
      uint64_t any = moved ? 1u : 0u;
      KMI_TRY(comm_allreduce_sum(u.comm, &any));
      if (!any) break;
    }
  }
  return KMI_OK;
}

// what the stages up to the heads and their scan leave in the workspace, for kmi_dbg_compact_dist_host and for
// kmi_dbg_clip_tips_dist_host (kmi_dbg_tips_dist.h), as UniStages of kmi_unitig.h does on one rank. Afterwards every node p knows
// its unitig's two end states (rec[2p].succ and rec[2p + 1].succ, global), its distances to them (rec[..].dist, so the unitig has
// rec[2p].dist + rec[2p + 1].dist + 1 nodes) and circ[p]; a head is the node with rec[2p + 1 - dir[p]].dist == 0.
struct UdStages {
  UdRun u;
  uint32_t *tab; uint64_t slots;   // unitig_table of this rank's nodes
  uint64_t *next, *endk;
  uint8_t *dir, *circ;
  ulonglong2 *scan;                // per node (unitig id, base offset), rank-local
  uint64_t nu, nb;                 // this rank's unitigs and their bases
};

// links, ranking, cycle pass, ends, heads and scan. pre: what this rank found wrong on its own so far; it is agreed on, with the
// workspace, before the first exchange
template <int NW>
static kmi_status ud_stages(kmi_dbg *g, kmi_comm *comm, uint32_t t, kmi_status pre, UdStages *out) {
  kmi_ctx *ctx = g->ctx;
  kmi_index *idx = g->nodes;
  const KShape shape = g->shape;
  const bool exists = g->node_kind == KMI_DBG_EDGE_EXISTS;
  UdRun &u = out->u;
  u = UdRun{};
  u.g = g; u.comm = comm; u.ctx = ctx;
  u.p = comm_size(comm); u.me = (uint32_t)comm_rank(comm);
  u.n = (idx->has_data && pre == KMI_OK) ? idx->n_entries : 0; u.ns = 2u * u.n;
  const uint64_t n = u.n, ns = u.ns;
  const uint32_t *occ = exists ? nullptr : (const uint32_t *)idx->vals;
  const uint64_t *keys = (const uint64_t *)idx->keys;
  uint64_t slots = 1024;
  while (slots < 2u * n) slots <<= 1;
  const uint64_t n_tiles = (n + kUniScanTile - 1) / kUniScanTile;
  void *p_tab = nullptr, *p_next = nullptr, *p_rank = nullptr, *p_node = nullptr, *p_scan = nullptr, *p_stage = nullptr, *p_end = nullptr, *p_cnt = nullptr;
  // every rank-local failure up to here and the workspace are agreed on before the first exchange
  kmi_status st = pre;
  auto get = [&](WsSlot slot, size_t bytes, void **out) { if (st == KMI_OK) st = ws_get(ctx, slot, bytes, out); };
  get(WS_UNI_TAB, (size_t)slots * sizeof(uint32_t), &p_tab);
  get(WS_UNI_NEXT, (size_t)(ns + 8u) * sizeof(uint64_t), &p_next);
  get(WS_UNI_RANK, (size_t)(ns + 8u) * sizeof(UdRec), &p_rank);
  get(WS_UNI_NODE, 64u + (size_t)2u * n + 64u, &p_node);
  get(WS_UNI_SCAN, (size_t)(n + n_tiles + 64u) * sizeof(ulonglong2), &p_scan);
  get(WS_UNI_STAGE, (size_t)(ns + 8u) * (NW + 1 > 2 ? NW + 1 : 2) * sizeof(uint64_t), &p_stage);
  get(WS_UNI_END, (size_t)(ns + 8u) * (NW + 2) * sizeof(uint64_t), &p_end);
  get(WS_UNI_CNT, sizeof(unsigned long long) * (2u * (size_t)u.p + 8u), &p_cnt);
  KMI_TRY(dist_agree(comm, st));
  uint32_t *tab = (uint32_t *)p_tab;
  uint64_t *next = (uint64_t *)p_next, *endk = (uint64_t *)p_end;
  u.rec = (UdRec *)p_rank; u.stage = (ulonglong2 *)p_stage; u.d_cnt = (unsigned long long *)p_cnt;
  uint8_t *dir = (uint8_t *)p_node + 64, *circ = dir + n;
  ulonglong2 *scan = (ulonglong2 *)p_scan, *sums = scan + n;
  unsigned long long *d_scalar = u.d_cnt + 2 * u.p;
  uint64_t total_states = ns;
  KMI_TRY(comm_allreduce_sum(comm, &total_states));
  uint32_t bound = 1;
  while (((uint64_t)1 << (bound - 1u)) < total_states) ++bound;   // ceil(log2 of the states of all ranks) + 1

  // ---- links
  KMI_HIP(ctx, hipMemsetAsync(tab, 0xFF, (size_t)slots * sizeof(uint32_t), ctx->stream));
  KMI_HIP(ctx, hipMemsetAsync(p_node, 0, 64u + (size_t)2u * n, ctx->stream));
  KMI_HIP(ctx, hipMemsetAsync(d_scalar, 0, 2 * sizeof(unsigned long long), ctx->stream));
  uint64_t n_link = 0;
  if (n) {
    {
      ProfScope ps(ctx, "unitig_dist_table", n);
      hipLaunchKernelGGL((unitig_table_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, n, tab, slots - 1u);
    }
    {
      ProfScope ps(ctx, "unitig_dist_link_req", n);
      hipLaunchKernelGGL((unitig_dist_link_req_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, (const uint32_t *)g->edges, n, shape, t, exists,
                         u.me, (uint64_t *)p_stage, ns, d_scalar, next);
    }
    KMI_HIP(ctx, hipGetLastError());
    KMI_HIP(ctx, hipMemcpyAsync(&n_link, d_scalar, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  {
    constexpr size_t rb = (NW + 1) * sizeof(uint64_t);
    void *d_send, *d_req, *d_ans, *d_got;
    std::vector<uint64_t> sc(u.p, 0), rc, rc2;
    uint64_t n_req = 0, n_ans = 0;
    KMI_TRY(ws_get(ctx, WS_DIST_A, (size_t)(n_link + 64u) * rb, &d_send));
    if (n_link) KMI_TRY(kmi_route_tuples_dev(ctx, &idx->cfg, (const uint64_t *)p_stage, (size_t)n_link, (uint32_t)u.p, 1, (uint64_t *)d_send, sc.data()));
    KMI_TRY(ud_exchange(u, d_send, sc, rb, WS_DIST_B, &d_req, rc, &n_req));
    KMI_TRY(ws_get(ctx, WS_DIST_C, (size_t)(n_req + 8u) * sizeof(ulonglong2), &d_ans));
    if (n_req) {
      ProfScope ps(ctx, "unitig_dist_link_ans", n_req);
      hipLaunchKernelGGL((unitig_dist_link_ans_kernel<NW>), dim3(uni_grid(n_req)), dim3(256), 0, ctx->stream, (const uint64_t *)d_req, n_req, keys,
                         (const uint32_t *)g->edges, (const uint32_t *)tab, slots - 1u, t, exists, u.me, (ulonglong2 *)d_ans);
    }
    KMI_HIP(ctx, hipGetLastError());
    KMI_TRY(ud_exchange(u, d_ans, rc, sizeof(ulonglong2), WS_DIST_D, &d_got, rc2, &n_ans));
    if (n_ans) {
      ProfScope ps(ctx, "unitig_dist_link_set", n_ans);
      hipLaunchKernelGGL(unitig_dist_link_set_kernel, dim3(uni_grid(n_ans)), dim3(256), 0, ctx->stream, (const ulonglong2 *)d_got, n_ans, next, ns);
    }
    if (ns) {
      ProfScope ps(ctx, "unitig_dist_rank_init", ns);
      hipLaunchKernelGGL(unitig_dist_rank_init_kernel, dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, (const uint64_t *)next, occ, ns, u.me, u.rec);
    }
    KMI_HIP(ctx, hipGetLastError());
  }

  // ---- ranking, cycles
  KMI_TRY(ud_rank_rounds(u, bound));
  uint64_t n_cyc = 0;
  if (ns) {
    KMI_HIP(ctx, hipMemsetAsync(d_scalar, 0, sizeof(unsigned long long), ctx->stream));
    {
      ProfScope ps(ctx, "unitig_dist_count_moving", ns);
      hipLaunchKernelGGL(unitig_dist_count_moving_kernel, dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, (const UdRec *)u.rec, ns, d_scalar);
    }
    KMI_HIP(ctx, hipGetLastError());
    KMI_HIP(ctx, hipMemcpyAsync(&n_cyc, d_scalar, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  KMI_TRY(comm_allreduce_sum(comm, &n_cyc));
  if (n_cyc) {
    uint64_t *cyc = endk;   // (the end k-mers come later)
    if (ns) {
      ProfScope ps(ctx, "unitig_dist_cycle_init", ns);
      hipLaunchKernelGGL((unitig_dist_cycle_init_kernel<NW>), dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, (const UdRec *)u.rec, (const uint64_t *)next, keys, ns,
                         u.me, cyc);
    }
    uint32_t rounds = 1;
    while (((uint64_t)1 << (rounds - 1u)) < n_cyc) ++rounds;   // a cycle has at most n_cyc / 2 nodes
    for (uint32_t r = 0; r < rounds; ++r) {
      if (ns) {
        ProfScope ps(ctx, "unitig_dist_cycle_req", ns);
        hipLaunchKernelGGL((unitig_dist_cycle_req_kernel<NW>), dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, (const uint64_t *)cyc, ns, u.me, u.stage);
      }
      const ulonglong2 *req; uint64_t n_req = 0, n_ans = 0;
      std::vector<uint64_t> rc, rc2;
      KMI_TRY(ud_send_requests(u, ns, &req, &n_req, rc));
      constexpr size_t ab = (NW + 3) * sizeof(uint64_t);
      void *p_ans, *p_got;
      KMI_TRY(ws_get(ctx, WS_DIST_C, (size_t)(n_req + 8u) * ab, &p_ans));
      if (n_req) {
        ProfScope ps(ctx, "unitig_dist_cycle_ans", n_req);
        hipLaunchKernelGGL((unitig_dist_cycle_ans_kernel<NW>), dim3(uni_grid(n_req)), dim3(256), 0, ctx->stream, req, n_req, (const uint64_t *)cyc, ns, (uint64_t *)p_ans);
      }
      KMI_HIP(ctx, hipGetLastError());
      KMI_TRY(ud_exchange(u, p_ans, rc, ab, WS_DIST_D, &p_got, rc2, &n_ans));
      if (n_ans) {
        ProfScope ps(ctx, "unitig_dist_cycle_set", n_ans);
        hipLaunchKernelGGL((unitig_dist_cycle_set_kernel<NW>), dim3(uni_grid(n_ans)), dim3(256), 0, ctx->stream, (const uint64_t *)p_got, n_ans, cyc, ns);
      }
      KMI_HIP(ctx, hipGetLastError());
    }
    if (ns) {
      ProfScope ps(ctx, "unitig_dist_cut", ns);
      hipLaunchKernelGGL((unitig_dist_cut_kernel<NW>), dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, (const uint64_t *)cyc, next, u.rec, ns, u.me, occ, circ);
    }
    KMI_HIP(ctx, hipGetLastError());
    KMI_TRY(ud_rank_rounds(u, bound));
  }

  // ---- ends, heads, scan
  {
    if (ns) {
      ProfScope ps(ctx, "unitig_dist_end_req", ns);
      hipLaunchKernelGGL(unitig_dist_end_req_kernel, dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, (const UdRec *)u.rec, ns, u.me, u.stage);
    }
    const ulonglong2 *req; uint64_t n_req = 0, n_ans = 0;
    std::vector<uint64_t> rc, rc2;
    KMI_TRY(ud_send_requests(u, ns, &req, &n_req, rc));
    constexpr size_t ab = (NW + 2) * sizeof(uint64_t);
    void *p_ans, *p_got;
    KMI_TRY(ws_get(ctx, WS_DIST_C, (size_t)(n_req + 8u) * ab, &p_ans));
    if (n_req) {
      ProfScope ps(ctx, "unitig_dist_end_ans", n_req);
      hipLaunchKernelGGL((unitig_dist_end_ans_kernel<NW>), dim3(uni_grid(n_req)), dim3(256), 0, ctx->stream, req, n_req, keys, occ, ns, shape, (uint64_t *)p_ans);
    }
    KMI_HIP(ctx, hipGetLastError());
    KMI_TRY(ud_exchange(u, p_ans, rc, ab, WS_DIST_D, &p_got, rc2, &n_ans));
    if (n_ans) {
      ProfScope ps(ctx, "unitig_dist_end_set", n_ans);
      hipLaunchKernelGGL((unitig_dist_end_set_kernel<NW>), dim3(uni_grid(n_ans)), dim3(256), 0, ctx->stream, (const uint64_t *)p_got, n_ans, endk, ns);
    }
    KMI_HIP(ctx, hipGetLastError());
  }
  ulonglong2 tot = make_ulonglong2(0ull, 0ull);
  if (n) {
    {
      ProfScope ps(ctx, "unitig_dist_heads", n);
      hipLaunchKernelGGL((unitig_dist_heads_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, (const UdRec *)u.rec, (const uint64_t *)endk, n, shape, scan, dir);
    }
    {
      ProfScope ps(ctx, "unitig_dist_scan", n);
      hipLaunchKernelGGL(unitig_scan_tiles_kernel, dim3((uint32_t)n_tiles), dim3(kUniScanNT), 0, ctx->stream, (const ulonglong2 *)scan, n, sums);
      hipLaunchKernelGGL(unitig_scan_sums_kernel, dim3(1), dim3(kUniScanNT), 0, ctx->stream, sums, n_tiles);
      hipLaunchKernelGGL(unitig_scan_apply_kernel, dim3((uint32_t)n_tiles), dim3(kUniScanNT), 0, ctx->stream, scan, n, (const ulonglong2 *)sums);
    }
    KMI_HIP(ctx, hipGetLastError());
    KMI_HIP(ctx, hipMemcpyAsync(&tot, sums + n_tiles, sizeof(tot), hipMemcpyDeviceToHost, ctx->stream));
    KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  out->tab = tab; out->slots = slots; out->next = next; out->endk = endk; out->dir = dir; out->circ = circ; out->scan = scan;
  out->nu = tot.x; out->nb = tot.y;
  return KMI_OK;
}

template <int NW>
static kmi_status dbg_compact_dist_impl(kmi_dbg *g, kmi_comm *comm, uint32_t t, kmi_status pre) {
  kmi_ctx *ctx = g->ctx;
  const KShape shape = g->shape;
  UdStages s;
  KMI_TRY(ud_stages<NW>(g, comm, t, pre, &s));
  UdRun &u = s.u;
  const uint64_t n = u.n, nu = s.nu, nb = s.nb;
  const uint64_t *keys = (const uint64_t *)g->nodes->keys, *endk = s.endk;
  const uint8_t *dir = s.dir, *circ = s.circ;
  const ulonglong2 *scan = s.scan;
  const ulonglong2 tot = make_ulonglong2(nu, nb);

  // ---- the result block (offsets[nu + 1], occurrences[nu], circular[nu], bases[nb]): agreed on before the last exchange
  const size_t off_b = (size_t)(nu + 1u) * 8u, occ_b = (size_t)nu * 8u, circ_b = ((size_t)nu + 15u) & ~(size_t)15u;
  const size_t bytes = off_b + occ_b + circ_b + (size_t)nb + 16u;
  void *buf = nullptr;
  kmi_status st = KMI_OK;
  if (nu && pool_alloc(ctx, &buf, bytes) != hipSuccess) st = set_err(ctx, KMI_ERR_NOMEM, "hipMalloc failed for the unitigs");
  if (buf) { g->uni_buf = buf; g->uni_bytes = bytes; }
  KMI_TRY(dist_agree(comm, st));
  uint64_t *u_off = (uint64_t *)buf, *u_occ = u_off + nu + 1u;
  uint8_t *u_circ = (uint8_t *)(u_occ + nu);
  char *u_bases = (char *)(u_circ + circ_b);
  const uint32_t letters = g->cfg.alphabet == KMI_ALPHA_RNA ? 0x55474341u /* "ACGU" */ : 0x54474341u /* "ACGT" */;
  if (n) {
    ProfScope ps(ctx, "unitig_dist_emit", n);
    hipLaunchKernelGGL((unitig_dist_emit_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, (const UdRec *)u.rec, (const uint64_t *)endk, n, shape,
                       (const ulonglong2 *)scan, (const uint8_t *)dir, (const uint8_t *)circ, letters, u_bases, nb, u_off, u_occ, u_circ, nu, u.stage);
  }
  KMI_HIP(ctx, hipGetLastError());
  {
    const ulonglong2 *in; uint64_t n_in = 0;
    std::vector<uint64_t> rc;
    KMI_TRY(ud_send_requests(u, n, &in, &n_in, rc));
    if (n_in && nu) {
      ProfScope ps(ctx, "unitig_dist_emit_recv", n_in);
      hipLaunchKernelGGL(unitig_dist_emit_recv_kernel, dim3(uni_grid(n_in)), dim3(256), 0, ctx->stream, in, n_in, (const ulonglong2 *)scan, n, shape.k, letters,
                         u_bases, nb, nu);
    }
    KMI_HIP(ctx, hipGetLastError());
  }
  if (nu) KMI_HIP(ctx, hipMemcpyAsync(u_off + nu, &tot.y, sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  g->n_unitigs = nu; g->n_unitig_bases = nb;
  return KMI_OK;
}

// collective; totals[0..1] = unitigs and bases over all ranks
static kmi_status dbg_compact_dist(kmi_dbg *g, kmi_comm *comm, uint32_t min_edge_count, uint64_t *totals) {
  kmi_ctx *ctx = g->ctx;
  dbg_unitigs_drop(g);
  g->unitig_rounds = 0; g->unitig_exchanges = 0; g->unitig_bytes_sent = 0;
  const int p = comm_size(comm);
  kmi_index *idx = g->nodes;
  kmi_status pre = KMI_OK;
  if (g->shape.bits != 2) pre = set_err(ctx, KMI_ERR_INVALID, "compact: only 2-bit alphabets");
  else if (min_edge_count == 0) pre = set_err(ctx, KMI_ERR_INVALID, "compact: min_edge_count must be at least 1");
  else if ((uint32_t)p > kUdMaxRanks) pre = set_err(ctx, (uint32_t)p > 65536u ? KMI_ERR_OVERFLOW : KMI_ERR_INVALID, "compact: more than 256 ranks");
  else if (idx->has_data && idx->n_entries >= 0x7FFFFFFFull) pre = set_err(ctx, KMI_ERR_OVERFLOW, "compact: more than 2^31 - 2 nodes on this rank");
  else if (idx->has_data && idx->n_entries) pre = ensure_dense(idx);
  kmi_status st = KMI_ERR_INVALID;
  switch (g->shape.n_words) {
    case 1: st = dbg_compact_dist_impl<1>(g, comm, min_edge_count, pre); break;
    case 2: st = dbg_compact_dist_impl<2>(g, comm, min_edge_count, pre); break;
    case 3: st = dbg_compact_dist_impl<3>(g, comm, min_edge_count, pre); break;
    case 4: st = dbg_compact_dist_impl<4>(g, comm, min_edge_count, pre); break;
  }
  ctx->unitig_dist_rounds = g->unitig_rounds; ctx->unitig_dist_exchanges = g->unitig_exchanges; ctx->unitig_dist_bytes = g->unitig_bytes_sent;
  if (st != KMI_OK) { dbg_unitigs_drop(g); return st; }
  g->uni_valid = true;
  totals[0] = g->n_unitigs; totals[1] = g->n_unitig_bases;
  KMI_TRY(comm_allreduce_sum(comm, &totals[0]));
  KMI_TRY(comm_allreduce_sum(comm, &totals[1]));
  return KMI_OK;
}

}  // namespace kmi
