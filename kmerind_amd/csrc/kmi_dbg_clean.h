// Cleaning a de Bruijn node map on the device (no counterpart in the reference: its test/test/debruijn/ ends at the node map):
//   kmi_dbg_spectrum_*       the count spectrum of counts[8]: kmi_index_spectrum_* on g->nodes, whose values are the occurrences
//   kmi_dbg_retain_counts    keeps the nodes with lo <= counts[8] <= hi: index_retain_counts with the 32-byte edge rows as the payload
//                            of bucket_retain_compact_kernel (same new_off, same predicate, old order)
//   kmi_dbg_prune_edges      judges every counter that is not 0 against the map as it was (weak / absent / unreciprocated / kept; the
//                            definition is in include/kmerind_hip.h) and clears the ones that fail
//
// PRUNING ON ONE RANK. unitig_table_kernel / uni_lookup of kmi_unitig.h find the neighbours. dbg_prune_kernel gives a node to a
// lane, which walks the node's eight counters: a counter >= t costs the neighbour k-mer, its reverse complement, one lookup and the
// neighbour's row (two uint4). The judged row goes to a FRESH edge array: workgroups of one launch do not see each other's writes
// (the L2s of the XCDs are not coherent within a launch), and a row judged against rows already judged would make the result depend
// on the schedule. The arrays are swapped once the kernel has succeeded. The class counts are summed per lane over its nodes, per
// wavefront by a reduction, and reach the global words as one atomic per wavefront and word.
//
// OVER RANKS. The shape of the link resolution of kmi_unitig_dist.h, two exchanges:
//   dbg_prune_count     per node: counters != 0, counters < t; counters >= t are the requests to come (the staging is sized by them)
//   dbg_prune_req       the fresh row with the weak counters cleared, and per counter >= t the request (canonical neighbour, node
//                       position << 3 | counter, reciprocal counter << 40, rule 3 exempt << 43); kmi_route_tuples_dev groups them by
//                       KeyToRank of the neighbour; exchange ((NW + 1) x 8 bytes each)
//   dbg_prune_ans       the owner: lookup in its own table, the reciprocal counter of its own row -> the request's value word with the
//                       class in bits 44..45; back in arrival order (8 bytes each)
//   dbg_prune_set       clears the counters judged absent or unreciprocated in the fresh rows (one word per answer: no two answers
//                       name the same counter) and counts them
//   dbg_prune_isolated  per node: all eight counters of the fresh row 0
// The verdict of each rank goes through dist_agree before the first exchange, before the second, and before the swap.
//
// Included by kmi_index.hip after kmi_unitig.h, kmi_unitig_dist.h and kmi_spectrum.h.
#pragma once

namespace kmi {

// device words of a prune call: the first eight are kmi_dbg_prune_stats in its order, PR_REQ counts the staged requests
enum { PR_NODES = 0, PR_SET = 1, PR_WEAK = 2, PR_ABSENT = 3, PR_UNREC = 4, PR_AFTER = 5, PR_ISOLATED = 6, PR_REQUESTS = 7, PR_REQ = 8, PR_WORDS = 16 };
enum : uint32_t { PRUNE_KEPT = 0, PRUNE_ABSENT = 1, PRUNE_UNREC = 2 };

// Counter j (0..3 out A C G T, 4..7 in A C G T) of the node `key`: c = the canonical neighbour k-mer, *recip = the index of the
// reciprocal counter in the neighbour's row, *exempt = rule 3 does not apply (the node or the neighbour is its own reverse complement)
template <int NW>
__device__ __forceinline__ void prune_neighbour(const uint64_t (&key)[NW], bool pal, uint32_t j, const KShape &shape, uint64_t (&c)[NW], uint32_t *recip,
                                                bool *exempt) {
  const uint32_t k = shape.k, b = j & 3u;
  uint64_t x[NW], xr[NW];
  uint32_t mine;   // the base of the node that the neighbour sees: v[0] behind an out counter, v[k-1] behind an in counter
  if (j < 4u) {    // x = v[1..k-1] + b
#pragma unroll
    for (int w = NW - 1; w >= 0; --w) x[w] = (key[w] << 2) | (w > 0 ? (key[w - 1] >> 62) : 0ull);
    x[0] |= b;
    mask_words<NW>(x, shape);
    mine = uni_base<NW>(key, 0u, k);
  } else {         // x = b + v[0..k-2]
#pragma unroll
    for (int w = 0; w < NW; ++w) x[w] = (key[w] >> 2) | (w + 1 < NW ? (key[w + 1] << 62) : 0ull);
    const uint32_t top = 2u * (k - 1u);
    x[top >> 6] |= (uint64_t)b << (top & 63u);
    mine = (uint32_t)key[0] & 3u;
  }
  revcomp_words<NW, 2>(x, xr, shape);
  const bool fwd = !less_words<NW>(xr, x);   // the neighbour is stored as x, or as its reverse complement
#pragma unroll
  for (int w = 0; w < NW; ++w) c[w] = fwd ? x[w] : xr[w];
  // out: (w, in, v[0]) or (w, out, comp(v[0])); in: (w, out, v[k-1]) or (w, in, comp(v[k-1]))
  if (j < 4u) *recip = fwd ? 4u + mine : 3u - mine;
  else *recip = fwd ? mine : 4u + 3u - mine;
  *exempt = pal || uni_eq<NW>(x, xr);
}

// the raw row of node p, and its counters as the definition reads them
__device__ __forceinline__ void prune_row(const uint32_t *__restrict__ edges, uint64_t p, bool exists, uint32_t (&raw)[8], uint32_t (&e)[8]) {
  uni_counters(edges, p, false, raw);
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = exists ? (raw[j] ? 1u : 0u) : raw[j];
}
__device__ __forceinline__ void prune_store(uint32_t *__restrict__ out, uint64_t p, const uint32_t (&r)[8]) {
  reinterpret_cast<uint4 *>(out)[p * 2u] = make_uint4(r[0], r[1], r[2], r[3]);
  reinterpret_cast<uint4 *>(out)[p * 2u + 1u] = make_uint4(r[4], r[5], r[6], r[7]);
}
// a lane's sums -> one atomic per wavefront and word (called by whole wavefronts)
__device__ __forceinline__ void prune_flush(unsigned long long *__restrict__ stats, int word, uint32_t v) {
  const uint64_t s = wave_reduce_sum((uint64_t)v);
  if (lane_id() == 0u && s) atomicAdd(&stats[word], (unsigned long long)s);
}

template <int NW>
__global__ __launch_bounds__(256) void dbg_prune_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ edges, uint64_t n,
                                                       const uint32_t *__restrict__ tab, uint64_t mask, KShape shape, uint32_t t, bool exists,
                                                       uint32_t *__restrict__ out, unsigned long long *__restrict__ stats) {
  uint32_t n_set = 0, n_weak = 0, n_absent = 0, n_unrec = 0, n_iso = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t key[NW], rc[NW];
    uni_load<NW>(keys, p, key);
    revcomp_words<NW, 2>(key, rc, shape);
    const bool pal = uni_eq<NW>(key, rc);
    uint32_t raw[8], e[8];
    prune_row(edges, p, exists, raw, e);
    uint32_t left = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
      if (e[j] == 0u) { raw[j] = 0u; continue; }
      ++n_set;
      bool keep = false;
      if (e[j] < t) ++n_weak;
      else {
        uint64_t c[NW];
        uint32_t recip;
        bool exempt;
        prune_neighbour<NW>(key, pal, j, shape, c, &recip, &exempt);
        const uint32_t w = uni_lookup<NW>(keys, tab, mask, c);
        if (w == kNoNext) ++n_absent;
        else if (exempt) keep = true;
        else {
          uint32_t f[8];
          uni_counters(edges, w, exists, f);
          if (f[recip] < t) ++n_unrec;
          else keep = true;
        }
      }
      if (keep) ++left;
      else raw[j] = 0u;
    }
    n_iso += left == 0u ? 1u : 0u;
    prune_store(out, p, raw);
  }
  prune_flush(stats, PR_SET, n_set);
  prune_flush(stats, PR_WEAK, n_weak);
  prune_flush(stats, PR_ABSENT, n_absent);
  prune_flush(stats, PR_UNREC, n_unrec);
  prune_flush(stats, PR_ISOLATED, n_iso);
}

// ---- over ranks ----
constexpr uint64_t kPruneSlotMask = (1ull << 40) - 1ull;   // node position << 3 | counter

__global__ __launch_bounds__(256) void dbg_prune_count_kernel(const uint32_t *__restrict__ edges, uint64_t n, uint32_t t, bool exists,
                                                             unsigned long long *__restrict__ stats) {
  uint32_t n_set = 0, n_weak = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t raw[8], e[8];
    prune_row(edges, p, exists, raw, e);
#pragma unroll
    for (int j = 0; j < 8; ++j) { n_set += e[j] ? 1u : 0u; n_weak += (e[j] && e[j] < t) ? 1u : 0u; }
  }
  prune_flush(stats, PR_SET, n_set);
  prune_flush(stats, PR_WEAK, n_weak);
}

template <int NW>
__global__ __launch_bounds__(256) void dbg_prune_req_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ edges, uint64_t n, KShape shape,
                                                           uint32_t t, bool exists, uint32_t *__restrict__ out, uint64_t *__restrict__ req, uint64_t cap,
                                                           unsigned long long *__restrict__ n_req) {
  for (uint64_t p0 = (uint64_t)blockIdx.x * blockDim.x; p0 < n; p0 += (uint64_t)gridDim.x * blockDim.x) {   // (uniform per wavefront)
    const uint64_t p = p0 + threadIdx.x;
    const bool act = p < n;
    uint64_t key[NW], rc[NW];
    uint32_t raw[8], e[8];
    bool pal = false;
    if (act) {
      uni_load<NW>(keys, p, key);
      revcomp_words<NW, 2>(key, rc, shape);
      pal = uni_eq<NW>(key, rc);
      prune_row(edges, p, exists, raw, e);
    }
    // one atomic per wavefront and 64 nodes: the wavefront's requests lie together, counter 0 of its lanes first
    unsigned long long m[8];
    uint32_t total = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
      const bool send = act && e[j] >= t;   // (t >= 1: a counter that is 0 sends nothing)
      if (act && !send) raw[j] = 0u;
      m[j] = __ballot(send);
      total += (uint32_t)__popcll(m[j]);
    }
    unsigned long long run = 0;
    if (lane_id() == 0u && total) run = atomicAdd(n_req, (unsigned long long)total);
    run = (unsigned long long)__shfl((long long)run, 0);
    const unsigned long long below = (1ull << lane_id()) - 1ull;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
      const uint64_t slot = run + (uint64_t)__popcll(m[j] & below);
      run += (uint64_t)__popcll(m[j]);
      if (((m[j] >> lane_id()) & 1ull) && slot < cap) {
        uint64_t c[NW];
        uint32_t recip;
        bool exempt;
        prune_neighbour<NW>(key, pal, j, shape, c, &recip, &exempt);
#pragma unroll
        for (int w = 0; w < NW; ++w) req[slot * (NW + 1) + w] = c[w];
        req[slot * (NW + 1) + NW] = (p << 3) | j | ((uint64_t)recip << 40) | ((uint64_t)(exempt ? 1u : 0u) << 43);
      }
    }
    if (act) prune_store(out, p, raw);
  }
}

template <int NW>
__global__ __launch_bounds__(256) void dbg_prune_ans_kernel(const uint64_t *__restrict__ req, uint64_t n_req, const uint64_t *__restrict__ keys,
                                                           const uint32_t *__restrict__ edges, const uint32_t *__restrict__ tab, uint64_t mask, uint32_t t,
                                                           bool exists, uint64_t *__restrict__ ans) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_req; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t key[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) key[w] = req[i * (NW + 1) + w];
    const uint64_t val = req[i * (NW + 1) + NW];
    const uint32_t recip = (uint32_t)(val >> 40) & 7u;
    const bool exempt = (val >> 43) & 1ull;
    uint32_t cls = PRUNE_KEPT;
    const uint32_t w = uni_lookup<NW>(keys, tab, mask, key);
    if (w == kNoNext) cls = PRUNE_ABSENT;
    else if (!exempt) {
      uint32_t f[8];
      uni_counters(edges, w, exists, f);
      if (f[recip] < t) cls = PRUNE_UNREC;
    }
    ans[i] = (val & kPruneSlotMask) | ((uint64_t)cls << 44);
  }
}

__global__ __launch_bounds__(256) void dbg_prune_set_kernel(const uint64_t *__restrict__ ans, uint64_t n_ans, uint32_t *__restrict__ out, uint64_t n,
                                                           unsigned long long *__restrict__ stats) {
  uint32_t n_absent = 0, n_unrec = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ans; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t a = ans[i], slot = a & kPruneSlotMask;
    const uint32_t cls = (uint32_t)(a >> 44) & 3u;
    if (cls == PRUNE_KEPT || slot >= n * 8u) continue;
    out[slot] = 0u;
    n_absent += cls == PRUNE_ABSENT ? 1u : 0u;
    n_unrec += cls == PRUNE_UNREC ? 1u : 0u;
  }
  prune_flush(stats, PR_ABSENT, n_absent);
  prune_flush(stats, PR_UNREC, n_unrec);
}

__global__ __launch_bounds__(256) void dbg_prune_isolated_kernel(const uint32_t *__restrict__ out, uint64_t n, unsigned long long *__restrict__ stats) {
  uint32_t n_iso = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t r[8];
    uni_counters(out, p, false, r);
    n_iso += (r[0] | r[1] | r[2] | r[3] | r[4] | r[5] | r[6] | r[7]) == 0u ? 1u : 0u;
  }
  prune_flush(stats, PR_ISOLATED, n_iso);
}

// ---- host side ----
static kmi_status dbg_retain_counts(kmi_dbg *g, uint32_t lo, uint32_t hi, uint64_t *n_erased) {
  kmi_ctx *ctx = g->ctx;
  kmi_index *idx = g->nodes;
  if (n_erased) *n_erased = 0;
  if (g->node_kind == KMI_DBG_EDGE_EXISTS) return set_err(ctx, KMI_ERR_INVALID, "retain_counts: an EDGE_EXISTS map keeps no occurrence count");
  if (lo > hi) return set_err(ctx, KMI_ERR_INVALID, "retain_counts: lo > hi");
  ctx->retain_fullest = 0;
  if (!idx->has_data || idx->n_entries == 0) { dbg_unitigs_drop(g); return KMI_OK; }
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  KMI_TRY(ensure_dense(idx));
  uint32_t *rows = nullptr;
  size_t rows_bytes = 0;
  KMI_TRY(index_retain_counts(idx, lo, hi, n_erased, (const uint32_t *)g->edges, &rows, &rows_bytes));
  if (rows) {   // (null: nothing left the map)
    pool_free(ctx, g->edges, g->edges_bytes);
    g->edges = rows; g->edges_bytes = rows_bytes;
  }
  dbg_unitigs_drop(g);   // (behind everything that can fail: a call that fails leaves the earlier compaction's result too)
  return KMI_OK;
}

static inline uint64_t prune_slots(uint64_t n) {
  uint64_t slots = 1024;
  while (slots < 2u * n) slots <<= 1;
  return slots;
}
static void prune_finish(uint64_t *s, uint64_t n) {
  s[PR_NODES] = n;
  s[PR_AFTER] = s[PR_SET] - s[PR_WEAK] - s[PR_ABSENT] - s[PR_UNREC];
}

template <int NW>
static kmi_status dbg_prune_impl(kmi_dbg *g, uint32_t t, uint64_t *stats) {
  kmi_ctx *ctx = g->ctx;
  kmi_index *idx = g->nodes;
  const uint64_t n = idx->n_entries, slots = prune_slots(n);
  const bool exists = g->node_kind == KMI_DBG_EDGE_EXISTS;
  const uint64_t *keys = (const uint64_t *)idx->keys;
  void *p_tab, *p_cnt;
  KMI_TRY(ws_get(ctx, WS_UNI_TAB, (size_t)slots * sizeof(uint32_t), &p_tab));
  KMI_TRY(ws_get(ctx, WS_UNI_CNT, sizeof(unsigned long long) * PR_WORDS, &p_cnt));
  uint32_t *tab = (uint32_t *)p_tab;
  unsigned long long *d_stats = (unsigned long long *)p_cnt;
  uint32_t *ne = nullptr;
  const size_t eb = (size_t)n * 8 * sizeof(uint32_t);
  if (pool_alloc(ctx, (void **)&ne, eb) != hipSuccess) return set_err(ctx, KMI_ERR_NOMEM, "hipMalloc failed for the edge counts");
  hipError_t e = hipMemsetAsync(tab, 0xFF, (size_t)slots * sizeof(uint32_t), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_stats, 0, sizeof(unsigned long long) * PR_WORDS, ctx->stream);
  if (e == hipSuccess) {
    {
      ProfScope ps(ctx, "unitig_table", n);
      hipLaunchKernelGGL((unitig_table_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, n, tab, slots - 1u);
    }
    {
      ProfScope ps(ctx, "dbg_prune", n);
      hipLaunchKernelGGL((dbg_prune_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, (const uint32_t *)g->edges, n, (const uint32_t *)tab,
                         slots - 1u, g->shape, t, exists, ne, d_stats);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(stats, d_stats, sizeof(uint64_t) * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {   // the map stays as it was
    pool_free(ctx, ne, eb);
    return set_err(ctx, KMI_ERR_DEVICE, "prune_edges: %s", hipGetErrorString(e));
  }
  pool_free(ctx, g->edges, g->edges_bytes);
  g->edges = ne; g->edges_bytes = eb;
  prune_finish(stats, n);
  return KMI_OK;
}

// what every form refuses alike, before anything else happens
static kmi_status dbg_prune_check(kmi_dbg *g, uint32_t min_edge_count) {
  kmi_ctx *ctx = g->ctx;
  if (g->shape.bits != 2) return set_err(ctx, KMI_ERR_INVALID, "prune_edges: only 2-bit alphabets");
  if (min_edge_count == 0) return set_err(ctx, KMI_ERR_INVALID, "prune_edges: min_edge_count must be at least 1");
  return KMI_OK;
}

static kmi_status dbg_prune(kmi_dbg *g, uint32_t min_edge_count, uint64_t *stats) {
  kmi_ctx *ctx = g->ctx;
  memset(stats, 0, sizeof(uint64_t) * 8);
  KMI_TRY(dbg_prune_check(g, min_edge_count));
  if (g->dist_share) return set_err(ctx, KMI_ERR_INVALID, "prune_edges: the map holds one rank's share of a build over ranks");
  kmi_index *idx = g->nodes;
  if (!idx->has_data || idx->n_entries == 0) { dbg_unitigs_drop(g); return KMI_OK; }
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  KMI_TRY(ensure_dense(idx));
  if (idx->n_entries >= 0x7FFFFFFFull) return set_err(ctx, KMI_ERR_OVERFLOW, "prune_edges: more than 2^31 - 2 nodes");
  kmi_status st = KMI_ERR_INVALID;
  switch (g->shape.n_words) {
    case 1: st = dbg_prune_impl<1>(g, min_edge_count, stats); break;
    case 2: st = dbg_prune_impl<2>(g, min_edge_count, stats); break;
    case 3: st = dbg_prune_impl<3>(g, min_edge_count, stats); break;
    case 4: st = dbg_prune_impl<4>(g, min_edge_count, stats); break;
  }
  if (st == KMI_OK) dbg_unitigs_drop(g);   // (a call that fails leaves the earlier compaction's result too)
  return st;
}

// collective. pre: what this rank found wrong on its own so far; it still takes part until the verdicts are agreed on
template <int NW>
static kmi_status dbg_prune_dist_impl(kmi_dbg *g, kmi_comm *comm, uint32_t t, kmi_status pre, uint64_t *stats) {
  kmi_ctx *ctx = g->ctx;
  kmi_index *idx = g->nodes;
  const int p = comm_size(comm);
  const bool exists = g->node_kind == KMI_DBG_EDGE_EXISTS;
  const uint64_t n = (idx->has_data && pre == KMI_OK) ? idx->n_entries : 0, slots = prune_slots(n);
  const uint64_t *keys = (const uint64_t *)idx->keys;
  constexpr size_t rb = (NW + 1) * sizeof(uint64_t);
  void *p_tab = nullptr, *p_cnt = nullptr, *p_stage = nullptr;
  uint32_t *ne = nullptr;
  const size_t eb = (size_t)(n ? n : 1) * 8 * sizeof(uint32_t);
  uint64_t h[PR_WORDS] = {0};
  // every rank-local failure up to the staged requests is agreed on before the first exchange
  kmi_status st = pre;
  auto get = [&](WsSlot slot, size_t bytes, void **out) { if (st == KMI_OK) st = ws_get(ctx, slot, bytes, out); };
  auto hip = [&](hipError_t e) { if (st == KMI_OK && e != hipSuccess) st = set_err(ctx, KMI_ERR_DEVICE, "prune_edges: %s", hipGetErrorString(e)); };
  get(WS_UNI_TAB, (size_t)slots * sizeof(uint32_t), &p_tab);
  get(WS_UNI_CNT, sizeof(unsigned long long) * PR_WORDS, &p_cnt);
  if (st == KMI_OK && pool_alloc(ctx, (void **)&ne, eb) != hipSuccess) st = set_err(ctx, KMI_ERR_NOMEM, "hipMalloc failed for the edge counts");
  uint32_t *tab = (uint32_t *)p_tab;
  unsigned long long *d_stats = (unsigned long long *)p_cnt;
  uint64_t n_send = 0;
  if (st == KMI_OK) {
    hip(hipMemsetAsync(tab, 0xFF, (size_t)slots * sizeof(uint32_t), ctx->stream));
    hip(hipMemsetAsync(d_stats, 0, sizeof(unsigned long long) * PR_WORDS, ctx->stream));
  }
  if (st == KMI_OK && n) {
    {
      ProfScope ps(ctx, "unitig_table", n);
      hipLaunchKernelGGL((unitig_table_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, n, tab, slots - 1u);
    }
    {
      ProfScope ps(ctx, "dbg_prune_count", n);
      hipLaunchKernelGGL(dbg_prune_count_kernel, dim3(uni_grid(n)), dim3(256), 0, ctx->stream, (const uint32_t *)g->edges, n, t, exists, d_stats);
    }
    hip(hipGetLastError());
    hip(hipMemcpyAsync(h, d_stats, sizeof(uint64_t) * 8, hipMemcpyDeviceToHost, ctx->stream));
    hip(hipStreamSynchronize(ctx->stream));
    n_send = h[PR_SET] - h[PR_WEAK];
  }
  get(WS_UNI_STAGE, (size_t)(n_send + 8u) * rb, &p_stage);
  if (st == KMI_OK && n) {
    ProfScope ps(ctx, "dbg_prune_req", n);
    hipLaunchKernelGGL((dbg_prune_req_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, (const uint32_t *)g->edges, n, g->shape, t, exists, ne,
                       (uint64_t *)p_stage, n_send, d_stats + PR_REQ);
    hip(hipGetLastError());
  }
  void *d_send = nullptr;
  get(WS_DIST_A, (size_t)(n_send + 64u) * rb, &d_send);
  std::vector<uint64_t> sc(p, 0), rc, rc2;
  if (st == KMI_OK && n_send) st = kmi_route_tuples_dev(ctx, &idx->cfg, (const uint64_t *)p_stage, (size_t)n_send, (uint32_t)p, 1, (uint64_t *)d_send, sc.data());
  st = dist_agree(comm, st);
  if (st != KMI_OK) { if (ne) pool_free(ctx, ne, eb); return st; }
  // the two exchanges (receive buffers, whose size depends on what the peers send, grow inside an exchange as in the library's other
  // collectives); the fresh rows are this call's until the swap
  void *d_req = nullptr, *d_ans = nullptr, *d_got = nullptr;
  uint64_t n_req = 0, n_ans = 0;
  ctx->prune_dist_bytes = n_send * rb;
  st = dist_exchange(comm, d_send, sc.data(), rb, WS_DIST_B, &d_req, rc, &n_req);
  get(WS_DIST_C, (size_t)(n_req + 8u) * sizeof(uint64_t), &d_ans);
  if (st == KMI_OK && n_req) {
    ProfScope ps(ctx, "dbg_prune_ans", n_req);
    hipLaunchKernelGGL((dbg_prune_ans_kernel<NW>), dim3(uni_grid(n_req)), dim3(256), 0, ctx->stream, (const uint64_t *)d_req, n_req, keys,
                       (const uint32_t *)g->edges, (const uint32_t *)tab, slots - 1u, t, exists, (uint64_t *)d_ans);
    hip(hipGetLastError());
  }
  // the answer stage is this rank's own too (its buffer, its launch): agreed on, so that no rank waits in the second exchange for one
  // that has given up. What the transport itself reports inside an exchange is every rank's alike.
  st = dist_agree(comm, st);
  if (st != KMI_OK) { pool_free(ctx, ne, eb); return st; }
  ctx->prune_dist_bytes += n_req * sizeof(uint64_t);
  st = dist_exchange(comm, d_ans, rc.data(), sizeof(uint64_t), WS_DIST_D, &d_got, rc2, &n_ans);
  if (st != KMI_OK) { pool_free(ctx, ne, eb); return st; }
  if (n_ans) {
    ProfScope ps(ctx, "dbg_prune_set", n_ans);
    hipLaunchKernelGGL(dbg_prune_set_kernel, dim3(uni_grid(n_ans)), dim3(256), 0, ctx->stream, (const uint64_t *)d_got, n_ans, ne, n, d_stats);
  }
  if (n) {
    ProfScope ps(ctx, "dbg_prune_isolated", n);
    hipLaunchKernelGGL(dbg_prune_isolated_kernel, dim3(uni_grid(n)), dim3(256), 0, ctx->stream, (const uint32_t *)ne, n, d_stats);
  }
  hip(hipGetLastError());
  hip(hipMemcpyAsync(h, d_stats, sizeof(uint64_t) * PR_WORDS, hipMemcpyDeviceToHost, ctx->stream));
  hip(hipStreamSynchronize(ctx->stream));
  if (st == KMI_OK && (h[PR_REQ] != n_send || n_ans != n_send)) st = set_err(ctx, KMI_ERR_DEVICE, "prune_edges: requests and answers do not add up");
  st = dist_agree(comm, st);   // before the swap: all ranks change their maps, or none does
  if (st != KMI_OK) { pool_free(ctx, ne, eb); return st; }
  if (n) {
    pool_free(ctx, g->edges, g->edges_bytes);
    g->edges = ne; g->edges_bytes = eb;
  } else pool_free(ctx, ne, eb);
  memcpy(stats, h, sizeof(uint64_t) * 8);
  stats[PR_REQUESTS] = n_send;
  prune_finish(stats, n);
  return KMI_OK;
}

// collective; stats_local / stats_total: eight words each
static kmi_status dbg_prune_dist(kmi_dbg *g, kmi_comm *comm, uint32_t min_edge_count, uint64_t *stats_local, uint64_t *stats_total) {
  kmi_ctx *ctx = g->ctx;
  memset(stats_local, 0, sizeof(uint64_t) * 8);
  memset(stats_total, 0, sizeof(uint64_t) * 8);
  // argument errors are every rank's alike: nothing collective has started
  KMI_TRY(dbg_prune_check(g, min_edge_count));
  if ((uint32_t)comm_size(comm) > kUdMaxRanks) return set_err(ctx, KMI_ERR_INVALID, "prune_edges: more than 256 ranks");
  ctx->prune_dist_bytes = 0;
  kmi_index *idx = g->nodes;
  kmi_status pre = KMI_OK;
  if (idx->has_data && idx->n_entries >= 0x7FFFFFFFull) pre = set_err(ctx, KMI_ERR_OVERFLOW, "prune_edges: more than 2^31 - 2 nodes on this rank");
  else if (idx->has_data && idx->n_entries) pre = ensure_dense(idx);
  kmi_status st = KMI_ERR_INVALID;
  switch (g->shape.n_words) {
    case 1: st = dbg_prune_dist_impl<1>(g, comm, min_edge_count, pre, stats_local); break;
    case 2: st = dbg_prune_dist_impl<2>(g, comm, min_edge_count, pre, stats_local); break;
    case 3: st = dbg_prune_dist_impl<3>(g, comm, min_edge_count, pre, stats_local); break;
    case 4: st = dbg_prune_dist_impl<4>(g, comm, min_edge_count, pre, stats_local); break;
  }
  if (st != KMI_OK) { memset(stats_local, 0, sizeof(uint64_t) * 8); return st; }
  dbg_unitigs_drop(g);   // (the maps have changed on every rank; a call that fails leaves the earlier compaction's result too)
  memcpy(stats_total, stats_local, sizeof(uint64_t) * 8);
  return comm_allreduce_sum(comm, stats_total, 8);
}

}  // namespace kmi
