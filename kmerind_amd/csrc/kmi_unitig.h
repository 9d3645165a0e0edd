// Unitigs of a de Bruijn node map held whole by one rank (kmi_dbg_compact). No counterpart in the reference: its
// test/test/debruijn/ ends at the node map. The graph being compacted is defined in include/kmerind_hip.h; here is how it is
// computed.
//
// STATES. Node p (its entry position in the dense node index) is read forward, as its stored k-mer (state 2p), or as the
// reverse complement (state 2p + 1). Leaving state (p, o) goes out of p's out end (o = 0) or in end (o = 1); next[s] is the state
// the unitig continues with (kNoNext: none). A link is symmetric, so prev(s) = next(s ^ 1) ^ 1 and a head of a chain is a state
// whose partner s ^ 1 has no next.
//
//   unitig_table    entry position -> open-addressing table of 2..4 x n u32 slots (key compared through the index's key array):
//                   the neighbours' lookups below, in input order, without touching the index's own query path
//   unitig_links    per node: both end degrees from g->edges, the neighbour behind a degree-1 end, its entered end's degree and
//                   reciprocal counter -> next[2p], next[2p + 1]; the list-ranking records of both states
//   unitig_jump     one launch per round (no grid-wide barrier: the L2s of the XCDs are not coherent across workgroups within a
//                   launch), double-buffered: (succ, dist, occurrence sum) of a state <- those of its successor. At most
//                   ceil(log2 2n) + 1 rounds; a device flag that a round still moved something is read every other round.
//   cycles          states whose final successor still has a next lie on cycles (rare). A second, smaller jumping over those
//                   states only finds each cycle's smallest canonical k-mer m (unitig_cycle_jump), the cycle is cut in front of
//                   (m, forward) (unitig_cut), and the ranking resumes for the cut states.
//   unitig_heads    per node: of its unitig's two spelling directions the one whose first k-mer is smaller (the ends are the final
//                   successors of its two states), its rank in that direction, the unitig's length; heads (rank 0) are counted
//   unitig_scan     exclusive scan of (heads, bases) in node order: unitig ids and base offsets, in the order of the heads' entries
//   unitig_emit     a head writes its k bases and its unitig's record; every other node its last base at offset + k - 1 + rank
//
// Footprint per node: 8..16 bytes of table, 8 of next, 64 of ranking records (two 16-byte records per state, ping-pong; the idle
// buffer holds the cycle pass and the scan), 2 of direction / cycle flags -- about 90 bytes -- plus the result (1 byte per base
// and 17 per unitig) owned by the graph.
#pragma once

namespace kmi {

constexpr uint32_t kNoNext = 0xFFFFFFFFu;   // (also the empty slot of the table: 2n states fit below it)

__device__ __forceinline__ uint64_t uni_mix64(uint64_t x) {   // the MurmurHash3 finaliser
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
template <int NW> __device__ __forceinline__ uint64_t uni_hash(const uint64_t (&k)[NW]) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
#pragma unroll
  for (int w = 0; w < NW; ++w) h = uni_mix64(h ^ k[w]);
  return h;
}
template <int NW> __device__ __forceinline__ void uni_load(const uint64_t *__restrict__ keys, uint64_t p, uint64_t (&k)[NW]) {
#pragma unroll
  for (int w = 0; w < NW; ++w) k[w] = keys[p * NW + w];
}
template <int NW> __device__ __forceinline__ bool uni_eq(const uint64_t (&a)[NW], const uint64_t (&b)[NW]) {
  bool e = true;
#pragma unroll
  for (int w = 0; w < NW; ++w) e = e && a[w] == b[w];
  return e;
}
// the k-mer of state (p, o): the stored key, or its reverse complement
template <int NW> __device__ __forceinline__ void uni_state_kmer(const uint64_t *__restrict__ keys, uint32_t s, const KShape &shape, uint64_t (&u)[NW]) {
  uint64_t k[NW];
  uni_load<NW>(keys, s >> 1, k);
  if (s & 1u) revcomp_words<NW, 2>(k, u, shape);
  else {
#pragma unroll
    for (int w = 0; w < NW; ++w) u[w] = k[w];
  }
}
// base i of a k-mer, i = 0 the first (the most significant two bits)
template <int NW> __device__ __forceinline__ uint32_t uni_base(const uint64_t (&u)[NW], uint32_t i, uint32_t k) {
  const uint32_t b = 2u * (k - 1u - i);
  return (uint32_t)(u[b >> 6] >> (b & 63u)) & 3u;
}

template <int NW>
__global__ __launch_bounds__(256) void unitig_table_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint32_t *__restrict__ tab, uint64_t mask) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t k[NW];
    uni_load<NW>(keys, i, k);
    uint64_t slot = uni_hash<NW>(k) & mask;
    while (atomicCAS(&tab[slot], kNoNext, (uint32_t)i) != kNoNext) slot = (slot + 1u) & mask;   // (distinct keys; load <= 1/2)
  }
}
template <int NW>
__device__ __forceinline__ uint32_t uni_lookup(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ tab, uint64_t mask, const uint64_t (&k)[NW]) {
  uint64_t slot = uni_hash<NW>(k) & mask;
  while (true) {
    const uint32_t p = tab[slot];
    if (p == kNoNext) return kNoNext;
    uint64_t e[NW];
    uni_load<NW>(keys, p, e);
    if (uni_eq<NW>(e, k)) return p;
    slot = (slot + 1u) & mask;
  }
}

// a ranking record: x = successor | distance << 32, y = occurrences of the nodes from the state up to its successor (exclusive).
// A state without next points at itself with distance 0 and sum 0.
__device__ __forceinline__ ulonglong2 uni_rec(uint32_t s, uint32_t nx, uint64_t occ) {
  return nx == kNoNext ? make_ulonglong2((uint64_t)s, 0ull) : make_ulonglong2((uint64_t)nx | (1ull << 32), occ);
}

// counters of node p as the definition reads them: EDGE_EXISTS maps show 0 / 1
__device__ __forceinline__ void uni_counters(const uint32_t *__restrict__ edges, uint64_t p, bool exists, uint32_t (&e)[8]) {
  const uint4 a = reinterpret_cast<const uint4 *>(edges)[p * 2u], b = reinterpret_cast<const uint4 *>(edges)[p * 2u + 1u];
  e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w; e[4] = b.x; e[5] = b.y; e[6] = b.z; e[7] = b.w;
  if (exists) {
#pragma unroll
    for (int t = 0; t < 8; ++t) e[t] = e[t] ? 1u : 0u;
  }
}

template <int NW>
__global__ __launch_bounds__(256) void unitig_links_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ edges,
                                                          const uint32_t *__restrict__ occ /* null: EDGE_EXISTS */, uint64_t n,
                                                          const uint32_t *__restrict__ tab, uint64_t mask, KShape shape, uint32_t t, bool exists,
                                                          uint32_t *__restrict__ next, ulonglong2 *__restrict__ rank) {
  const uint32_t k = shape.k;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t key[NW], rc[NW];
    uni_load<NW>(keys, p, key);
    revcomp_words<NW, 2>(key, rc, shape);
    const bool pal = uni_eq<NW>(key, rc);   // a palindrome links to nothing
    uint32_t e[8];
    uni_counters(edges, p, exists, e);
    const uint64_t my_occ = occ ? (uint64_t)occ[p] : 0ull;
#pragma unroll
    for (uint32_t o = 0; o < 2u; ++o) {
      uint32_t nx = kNoNext;
      // the end state (p, o) leaves by: o = 0 the out end, base b = counter b; o = 1 the in end, read on the other strand: base b
      // of the reverse complement is in-counter comp(b)
      uint32_t deg = 0, b = 0;
#pragma unroll
      for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t c = o ? e[4u + 3u - j] : e[j];
        if (c >= t) { ++deg; b = j; }
      }
      if (!pal && deg == 1u) {
        const uint64_t(&u)[NW] = o ? rc : key;
        const uint32_t u0 = uni_base<NW>(u, 0u, k);
        uint64_t v[NW], vr[NW];   // v = u[1 .. k-1] + b, the oriented k-mer entered
#pragma unroll
        for (int w = NW - 1; w >= 0; --w) v[w] = (u[w] << 2) | (w > 0 ? (u[w - 1] >> 62) : 0ull);
        v[0] |= b;
        mask_words<NW>(v, shape);
        revcomp_words<NW, 2>(v, vr, shape);
        const bool fwd = !less_words<NW>(vr, v);   // the neighbour is stored as v (entered by its in end) or as vr (by its out end)
        if (!uni_eq<NW>(v, vr)) {
          const uint32_t w = uni_lookup<NW>(keys, tab, mask, fwd ? v : vr);
          if (w != kNoNext && (uint64_t)w != p) {
            uint32_t f[8];
            uni_counters(edges, w, exists, f);
            const uint32_t base = fwd ? 4u : 0u, want = fwd ? u0 : 3u - u0;   // the entered end and the reciprocal base
            uint32_t dw = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) dw += f[base + j] >= t ? 1u : 0u;
            if (dw == 1u && f[base + want] >= t) nx = 2u * w + (fwd ? 0u : 1u);
          }
        }
      }
      const uint32_t s = 2u * (uint32_t)p + o;
      next[s] = nx;
      rank[s] = uni_rec(s, nx, my_occ);
    }
  }
}

// one round of pointer jumping; *moved = 1 when some state's successor changed
__global__ __launch_bounds__(256) void unitig_jump_kernel(const ulonglong2 *__restrict__ src, ulonglong2 *__restrict__ dst, uint64_t ns,
                                                         uint32_t *__restrict__ moved) {
  bool mv = false;
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 a = src[s];
    const uint32_t nx = (uint32_t)a.x;
    if (nx == (uint32_t)s) { dst[s] = a; continue; }
    const ulonglong2 b = src[nx];
    const uint32_t nn = (uint32_t)b.x;
    mv = mv || nn != nx;
    dst[s] = make_ulonglong2((uint64_t)nn | (((a.x >> 32) + (b.x >> 32)) << 32), a.y + b.y);
  }
  if (__any(mv) && lane_id() == 0u) *moved = 1u;
}

// states on cycles (their final successor still has a next): x = next | node << 32 for the jumping below, ~0 for the others
__global__ __launch_bounds__(256) void unitig_cycle_init_kernel(const uint32_t *__restrict__ next, const ulonglong2 *__restrict__ rank, uint64_t ns,
                                                               uint64_t *__restrict__ cyc, uint32_t *__restrict__ n_cyc) {
  for (uint64_t s0 = (uint64_t)blockIdx.x * blockDim.x; s0 < ns; s0 += (uint64_t)gridDim.x * blockDim.x) {   // (uniform per wavefront)
    const uint64_t s = s0 + threadIdx.x;
    bool c = false;
    if (s < ns) {
      c = next[(uint32_t)rank[s].x] != kNoNext;
      cyc[s] = c ? ((uint64_t)next[s] | ((s >> 1) << 32)) : ~0ull;
    }
    const unsigned long long m = __ballot(c);
    if (m && lane_id() == 0u) atomicAdd(n_cyc, (uint32_t)__popcll(m));
  }
}
// one round over the cycle states: the node with the smaller key of the two stretches
template <int NW>
__global__ __launch_bounds__(256) void unitig_cycle_jump_kernel(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, uint64_t ns,
                                                               const uint64_t *__restrict__ keys) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t a = src[s];
    if (a == ~0ull) { dst[s] = a; continue; }
    const uint64_t b = src[(uint32_t)a];
    const uint32_t ma = (uint32_t)(a >> 32), mb = (uint32_t)(b >> 32);
    uint32_t m = ma;
    if (mb != ma) {
      uint64_t ka[NW], kb[NW];
      uni_load<NW>(keys, ma, ka);
      uni_load<NW>(keys, mb, kb);
      if (less_words<NW>(kb, ka)) m = mb;
    }
    dst[s] = (b & 0xFFFFFFFFull) | ((uint64_t)m << 32);
  }
}
// cut every cycle in front of (m, forward), m its node with the smallest key: (m, reverse) and the state that led into (m, forward)
// lose their next; the cycle's states get fresh ranking records, and its nodes the circular flag
__global__ __launch_bounds__(256) void unitig_cut_kernel(const uint64_t *__restrict__ cyc, uint32_t *__restrict__ next, ulonglong2 *__restrict__ rank,
                                                        uint64_t ns, const uint32_t *__restrict__ occ, uint8_t *__restrict__ circ) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t c = cyc[s];
    if (c == ~0ull) continue;
    const uint32_t m = (uint32_t)(c >> 32);
    uint32_t nx = next[s];
    if ((s >> 1) == m ? (s & 1u) != 0u : nx == 2u * m) nx = kNoNext;
    next[s] = nx;
    rank[s] = uni_rec((uint32_t)s, nx, occ ? (uint64_t)occ[s >> 1] : 0ull);
    if (!(s & 1u)) circ[s >> 1] = 1u;
  }
}

// per node: the spelling direction (the one whose first k-mer is smaller; the first k-mer of direction o is that of the state
// reached by leaving in direction 1 - o, read the other way), and (1, length in bases) for a head, (0, 0) for the others
template <int NW>
__global__ __launch_bounds__(256) void unitig_heads_kernel(const uint64_t *__restrict__ keys, const ulonglong2 *__restrict__ rank, uint64_t n,
                                                          KShape shape, ulonglong2 *__restrict__ scan, uint8_t *__restrict__ dir) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
    const ulonglong2 a0 = rank[2u * p], a1 = rank[2u * p + 1u];
    uint64_t f0[NW], f1[NW];
    uni_state_kmer<NW>(keys, (uint32_t)a1.x ^ 1u, shape, f0);
    uni_state_kmer<NW>(keys, (uint32_t)a0.x ^ 1u, shape, f1);
    const uint32_t d = less_words<NW>(f1, f0) ? 1u : 0u;
    const uint64_t r = d ? (a0.x >> 32) : (a1.x >> 32);   // rank in direction d = distance to the far end going the other way
    const uint64_t len = (a0.x >> 32) + (a1.x >> 32) + 1u + shape.k - 1u;
    scan[p] = r == 0u ? make_ulonglong2(1ull, len) : make_ulonglong2(0ull, 0ull);
    dir[p] = (uint8_t)d;
  }
}

// exclusive scan of ulonglong2 pairs: tiles of kUniScanTile, their sums, then the tiles again
constexpr int kUniScanNT = 256, kUniScanIPT = 8, kUniScanTile = kUniScanNT * kUniScanIPT;
__device__ __forceinline__ ulonglong2 uni_add(ulonglong2 a, ulonglong2 b) { return make_ulonglong2(a.x + b.x, a.y + b.y); }
// exclusive scan over the workgroup (kUniScanNT threads); *total = the sum
__device__ __forceinline__ ulonglong2 uni_block_exclusive(ulonglong2 v, ulonglong2 *s_buf, ulonglong2 *total) {
  const uint32_t i = threadIdx.x;
  s_buf[i] = v;
  __syncthreads();
  for (uint32_t d = 1; d < (uint32_t)kUniScanNT; d <<= 1) {
    const ulonglong2 o = i >= d ? s_buf[i - d] : make_ulonglong2(0ull, 0ull);
    __syncthreads();
    s_buf[i] = uni_add(s_buf[i], o);
    __syncthreads();
  }
  const ulonglong2 inc = s_buf[i];
  *total = s_buf[kUniScanNT - 1];
  __syncthreads();
  return make_ulonglong2(inc.x - v.x, inc.y - v.y);
}
__global__ __launch_bounds__(kUniScanNT) void unitig_scan_tiles_kernel(const ulonglong2 *__restrict__ in, uint64_t n, ulonglong2 *__restrict__ sums) {
  __shared__ ulonglong2 s_buf[kUniScanNT];
  const uint64_t b0 = (uint64_t)blockIdx.x * kUniScanTile + (uint64_t)threadIdx.x * kUniScanIPT;
  ulonglong2 v = make_ulonglong2(0ull, 0ull);
  for (int j = 0; j < kUniScanIPT; ++j) if (b0 + j < n) v = uni_add(v, in[b0 + j]);
  ulonglong2 tot;
  (void)uni_block_exclusive(v, s_buf, &tot);
  if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}
// one workgroup: the tile sums in place (exclusive), the grand total behind them
__global__ __launch_bounds__(kUniScanNT) void unitig_scan_sums_kernel(ulonglong2 *__restrict__ sums, uint64_t n_tiles) {
  __shared__ ulonglong2 s_buf[kUniScanNT];
  ulonglong2 carry = make_ulonglong2(0ull, 0ull);
  for (uint64_t c0 = 0; c0 < n_tiles; c0 += kUniScanNT) {
    const uint64_t i = c0 + threadIdx.x;
    const ulonglong2 v = i < n_tiles ? sums[i] : make_ulonglong2(0ull, 0ull);
    ulonglong2 tot;
    const ulonglong2 ex = uni_block_exclusive(v, s_buf, &tot);
    if (i < n_tiles) sums[i] = uni_add(carry, ex);
    carry = uni_add(carry, tot);
  }
  if (threadIdx.x == 0) sums[n_tiles] = carry;
}
__global__ __launch_bounds__(kUniScanNT) void unitig_scan_apply_kernel(ulonglong2 *__restrict__ data, uint64_t n, const ulonglong2 *__restrict__ sums) {
  __shared__ ulonglong2 s_buf[kUniScanNT];
  const uint64_t b0 = (uint64_t)blockIdx.x * kUniScanTile + (uint64_t)threadIdx.x * kUniScanIPT;
  ulonglong2 v[kUniScanIPT], t = make_ulonglong2(0ull, 0ull);
  for (int j = 0; j < kUniScanIPT; ++j) { v[j] = b0 + j < n ? data[b0 + j] : make_ulonglong2(0ull, 0ull); t = uni_add(t, v[j]); }
  ulonglong2 tot;
  ulonglong2 run = uni_add(sums[blockIdx.x], uni_block_exclusive(t, s_buf, &tot));
  for (int j = 0; j < kUniScanIPT; ++j) {
    if (b0 + j < n) data[b0 + j] = run;
    run = uni_add(run, v[j]);
  }
}

// the result: bases of every node; a head also writes its unitig's offset, occurrence sum and circular flag
template <int NW>
__global__ __launch_bounds__(256) void unitig_emit_kernel(const uint64_t *__restrict__ keys, const ulonglong2 *__restrict__ rank, uint64_t n,
                                                         KShape shape, const ulonglong2 *__restrict__ scan, const uint8_t *__restrict__ dir,
                                                         const uint8_t *__restrict__ circ, const uint32_t *__restrict__ occ, uint32_t letters /* four chars */,
                                                         char *__restrict__ bases, uint64_t nb, uint64_t *__restrict__ u_off, uint64_t *__restrict__ u_occ,
                                                         uint8_t *__restrict__ u_circ, uint64_t nu) {
  // (the writes are checked against the totals of the scan: ranks and lengths come from the same records, so they always fit)
  const uint32_t k = shape.k;
  auto letter = [&](uint32_t c) { return (char)(letters >> (8u * c)); };
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t d = dir[p];
    const ulonglong2 ad = rank[2u * p + d], ao = rank[2u * p + 1u - d];
    const uint64_t r = ao.x >> 32;
    const uint32_t head = ((uint32_t)ao.x ^ 1u) >> 1;
    const ulonglong2 sc = scan[head];   // (unitig id, base offset)
    uint64_t u[NW];
    uni_state_kmer<NW>(keys, 2u * (uint32_t)p + d, shape, u);
    if (sc.x >= nu) continue;
    if (r == 0u) {
      if (sc.y + k > nb) continue;
      for (uint32_t i = 0; i < k; ++i) bases[sc.y + i] = letter(uni_base<NW>(u, i, k));
      const uint32_t tail = (uint32_t)ad.x >> 1;
      u_off[sc.x] = sc.y;
      u_occ[sc.x] = ad.y + (occ ? (uint64_t)occ[tail] : 0ull);
      u_circ[sc.x] = circ[p];
    } else if (sc.y + k - 1u + r < nb) {
      bases[sc.y + k - 1u + r] = letter((uint32_t)u[0] & 3u);
    }
  }
}

}  // namespace kmi

namespace kmi {

static void dbg_unitigs_drop(kmi_dbg *g) {
  if (g->uni_buf) pool_free(g->ctx, g->uni_buf, g->uni_bytes);
  g->uni_buf = nullptr; g->uni_bytes = 0;
  g->uni_valid = false; g->n_unitigs = 0; g->n_unitig_bases = 0;
}

static inline uint32_t uni_grid(uint64_t n) { const uint64_t b = (n + 255u) / 256u; return (uint32_t)(b < 1u ? 1u : (b > 16384u ? 16384u : b)); }

// pointer jumping from `*cur` (0 / 1: which half of the ranking buffer holds the records) until nothing moves or the bound is reached
static kmi_status uni_rank_rounds(kmi_dbg *g, ulonglong2 *rank2, uint64_t half, uint64_t ns, uint32_t *d_moved, uint32_t *cur) {
  kmi_ctx *ctx = g->ctx;
  uint32_t bound = 1;
  while (((uint64_t)1 << (bound - 1u)) < ns) ++bound;   // ceil(log2 ns) + 1
  for (uint32_t r = 0; r < bound; ++r) {
    const bool check = (r & 1u) || r + 1u == bound;
    if (check) KMI_HIP(ctx, hipMemsetAsync(d_moved, 0, sizeof(uint32_t), ctx->stream));
    {
      ProfScope ps(ctx, "unitig_jump", ns);
      hipLaunchKernelGGL(unitig_jump_kernel, dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, (const ulonglong2 *)(rank2 + *cur * half),
                         rank2 + (1u - *cur) * half, ns, d_moved);
    }
    KMI_HIP(ctx, hipGetLastError());
    *cur = 1u - *cur;
    ++g->unitig_rounds;
    if (check) {
      uint32_t moved = 1;
      KMI_HIP(ctx, hipMemcpyAsync(&moved, d_moved, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
      KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
      if (!moved) break;
    }
  }
  return KMI_OK;
}

// what the stages up to unitig_heads leave in the workspace, for kmi_dbg_compact and for kmi_dbg_clip_tips (kmi_dbg_tips.h)
struct UniStages {
  uint32_t *tab; uint64_t mask;   // the neighbour table
  ulonglong2 *rk;                 // final ranking records: rk[s] = (end state | distance << 32, occurrence sum)
  ulonglong2 *scan;               // per node (1, bases) for a head, (0, 0) for the others; the scan's tile sums fit behind n
  uint8_t *dir, *circ;            // per node: spelling direction, circular flag
};

// table, links, jumping, cycle pass, heads
template <int NW>
static kmi_status uni_stages(kmi_dbg *g, uint32_t t, UniStages *out) {
  kmi_ctx *ctx = g->ctx;
  kmi_index *idx = g->nodes;
  const KShape shape = g->shape;
  const uint64_t n = idx->n_entries, ns = 2u * n;
  const bool exists = g->node_kind == KMI_DBG_EDGE_EXISTS;
  const uint32_t *occ = exists ? nullptr : (const uint32_t *)idx->vals;
  const uint64_t *keys = (const uint64_t *)idx->keys;
  uint64_t slots = 1024;
  while (slots < 2u * n) slots <<= 1;
  void *p_tab, *p_next, *p_rank, *p_node;
  const uint64_t half = ns + n / kUniScanTile + 64u;   // records per half of the ranking buffer (the scan's tile sums fit behind n)
  KMI_TRY(ws_get(ctx, WS_UNI_TAB, (size_t)slots * sizeof(uint32_t), &p_tab));
  KMI_TRY(ws_get(ctx, WS_UNI_NEXT, (size_t)ns * sizeof(uint32_t), &p_next));
  KMI_TRY(ws_get(ctx, WS_UNI_RANK, (size_t)(2u * half) * sizeof(ulonglong2), &p_rank));
  KMI_TRY(ws_get(ctx, WS_UNI_NODE, 64u + (size_t)2u * n + 64u, &p_node));
  uint32_t *tab = (uint32_t *)p_tab, *next = (uint32_t *)p_next;
  ulonglong2 *rank2 = (ulonglong2 *)p_rank;   // two halves, at 0 and at `half` records
  uint32_t *d_scalars = (uint32_t *)p_node;   // [0] moved, [1] cycle states
  uint8_t *dir = (uint8_t *)p_node + 64, *circ = dir + n;
  KMI_HIP(ctx, hipMemsetAsync(tab, 0xFF, (size_t)slots * sizeof(uint32_t), ctx->stream));
  KMI_HIP(ctx, hipMemsetAsync(p_node, 0, 64u + (size_t)2u * n, ctx->stream));
  {
    ProfScope ps(ctx, "unitig_table", n);
    hipLaunchKernelGGL((unitig_table_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, n, tab, slots - 1u);
  }
  {
    ProfScope ps(ctx, "unitig_links", n);
    hipLaunchKernelGGL((unitig_links_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, (const uint32_t *)g->edges, occ, n,
                       (const uint32_t *)tab, slots - 1u, shape, t, exists, next, rank2);
  }
  KMI_HIP(ctx, hipGetLastError());
  uint32_t cur = 0;
  g->unitig_rounds = 0;
  KMI_TRY(uni_rank_rounds(g, rank2, half, ns, &d_scalars[0], &cur));
  // cycles: their states in the idle half (two u64 arrays of ns)
  ulonglong2 *rk = rank2 + cur * half;
  uint64_t *cyc = (uint64_t *)(rank2 + (1u - cur) * half);
  {
    ProfScope ps(ctx, "unitig_cycles", ns);
    hipLaunchKernelGGL(unitig_cycle_init_kernel, dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, (const uint32_t *)next, (const ulonglong2 *)rk, ns,
                       cyc, &d_scalars[1]);
  }
  KMI_HIP(ctx, hipGetLastError());
  uint32_t n_cyc = 0;
  KMI_HIP(ctx, hipMemcpyAsync(&n_cyc, &d_scalars[1], sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n_cyc) {
    uint32_t c = 0, rounds = 1;
    while (((uint64_t)1 << (rounds - 1u)) < n_cyc) ++rounds;   // a cycle has at most n_cyc / 2 nodes
    for (uint32_t r = 0; r < rounds; ++r) {
      ProfScope ps(ctx, "unitig_cycle_jump", ns);
      hipLaunchKernelGGL((unitig_cycle_jump_kernel<NW>), dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, (const uint64_t *)(cyc + c * ns),
                         cyc + (1u - c) * ns, ns, keys);
      c = 1u - c;
    }
    {
      ProfScope ps(ctx, "unitig_cut", ns);
      hipLaunchKernelGGL(unitig_cut_kernel, dim3(uni_grid(ns)), dim3(256), 0, ctx->stream, (const uint64_t *)(cyc + c * ns), next, rk, ns, occ, circ);
    }
    KMI_HIP(ctx, hipGetLastError());
    KMI_TRY(uni_rank_rounds(g, rank2, half, ns, &d_scalars[0], &cur));
    rk = rank2 + cur * half;
  }
  ulonglong2 *scan = rank2 + (1u - cur) * half;
  {
    ProfScope ps(ctx, "unitig_heads", n);
    hipLaunchKernelGGL((unitig_heads_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, (const ulonglong2 *)rk, n, shape, scan, dir);
  }
  KMI_HIP(ctx, hipGetLastError());
  out->tab = tab; out->mask = slots - 1u;
  out->rk = rk; out->scan = scan; out->dir = dir; out->circ = circ;
  return KMI_OK;
}

template <int NW>
static kmi_status dbg_compact_impl(kmi_dbg *g, uint32_t t) {
  kmi_ctx *ctx = g->ctx;
  kmi_index *idx = g->nodes;
  const KShape shape = g->shape;
  const uint64_t n = idx->n_entries;
  const uint32_t *occ = g->node_kind == KMI_DBG_EDGE_EXISTS ? nullptr : (const uint32_t *)idx->vals;
  const uint64_t *keys = (const uint64_t *)idx->keys;
  UniStages u;
  KMI_TRY(uni_stages<NW>(g, t, &u));
  ulonglong2 *rk = u.rk, *scan = u.scan, *sums = scan + n;
  const uint8_t *dir = u.dir, *circ = u.circ;
  const uint64_t n_tiles = (n + kUniScanTile - 1) / kUniScanTile;
  {
    ProfScope ps(ctx, "unitig_scan", n);
    hipLaunchKernelGGL(unitig_scan_tiles_kernel, dim3((uint32_t)n_tiles), dim3(kUniScanNT), 0, ctx->stream, (const ulonglong2 *)scan, n, sums);
    hipLaunchKernelGGL(unitig_scan_sums_kernel, dim3(1), dim3(kUniScanNT), 0, ctx->stream, sums, n_tiles);
    hipLaunchKernelGGL(unitig_scan_apply_kernel, dim3((uint32_t)n_tiles), dim3(kUniScanNT), 0, ctx->stream, scan, n, (const ulonglong2 *)sums);
  }
  KMI_HIP(ctx, hipGetLastError());
  ulonglong2 tot = make_ulonglong2(0ull, 0ull);
  KMI_HIP(ctx, hipMemcpyAsync(&tot, sums + n_tiles, sizeof(tot), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const uint64_t nu = tot.x, nb = tot.y;
  // the result block: offsets[nu + 1], occurrences[nu], circular[nu], bases[nb]
  const size_t off_b = (size_t)(nu + 1u) * 8u, occ_b = (size_t)nu * 8u, circ_b = ((size_t)nu + 15u) & ~(size_t)15u;
  const size_t bytes = off_b + occ_b + circ_b + (size_t)nb + 16u;
  void *buf = nullptr;
  if (pool_alloc(ctx, &buf, bytes) != hipSuccess) return set_err(ctx, KMI_ERR_NOMEM, "hipMalloc failed for the unitigs");
  g->uni_buf = buf; g->uni_bytes = bytes;
  uint64_t *u_off = (uint64_t *)buf, *u_occ = u_off + nu + 1u;
  uint8_t *u_circ = (uint8_t *)(u_occ + nu);
  char *u_bases = (char *)(u_circ + circ_b);
  const uint32_t letters = g->cfg.alphabet == KMI_ALPHA_RNA ? 0x55474341u /* "ACGU" */ : 0x54474341u /* "ACGT" */;
  {
    ProfScope ps(ctx, "unitig_emit", n);
    hipLaunchKernelGGL((unitig_emit_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, (const ulonglong2 *)rk, n, shape,
                       (const ulonglong2 *)scan, (const uint8_t *)dir, (const uint8_t *)circ, occ, letters, u_bases, nb, u_off, u_occ, u_circ, nu);
  }
  KMI_HIP(ctx, hipGetLastError());
  KMI_HIP(ctx, hipMemcpyAsync(u_off + nu, &tot.y, sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  g->n_unitigs = nu; g->n_unitig_bases = nb;
  return KMI_OK;
}

static kmi_status dbg_compact(kmi_dbg *g, uint32_t min_edge_count) {
  kmi_ctx *ctx = g->ctx;
  dbg_unitigs_drop(g);
  if (g->shape.bits != 2) return set_err(ctx, KMI_ERR_INVALID, "compact: only 2-bit alphabets");
  if (g->dist_share) return set_err(ctx, KMI_ERR_INVALID, "compact: the map holds one rank's share of a build over ranks");
  if (min_edge_count == 0) return set_err(ctx, KMI_ERR_INVALID, "compact: min_edge_count must be at least 1");
  kmi_index *idx = g->nodes;
  g->unitig_rounds = 0;
  if (idx->has_data && idx->n_entries) {
    KMI_TRY(ensure_dense(idx));
    if (idx->n_entries >= 0x7FFFFFFFull) return set_err(ctx, KMI_ERR_OVERFLOW, "compact: more than 2^31 - 2 nodes");
    kmi_status st = KMI_ERR_INVALID;
    switch (g->shape.n_words) {
      case 1: st = dbg_compact_impl<1>(g, min_edge_count); break;
      case 2: st = dbg_compact_impl<2>(g, min_edge_count); break;
      case 3: st = dbg_compact_impl<3>(g, min_edge_count); break;
      case 4: st = dbg_compact_impl<4>(g, min_edge_count); break;
    }
    if (st != KMI_OK) { dbg_unitigs_drop(g); return st; }
  }
  g->uni_valid = true;
  return KMI_OK;
}

}  // namespace kmi
