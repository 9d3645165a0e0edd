// Popping the bubbles of a de Bruijn node map held whole by one rank (kmi_dbg_pop_bubbles; no counterpart in the reference: its
// test/test/debruijn/ ends at the node map). The definition is in include/kmerind_hip.h; here is how it is computed.
//
//   uni_stages          table, links, jumping, cycle pass, heads of kmi_unitig.h, as the tip clipping takes them
//   bubbles_classify    one lane per head node: the degrees of the unitig's two ends; 1 and 1 -> behind either counter the neighbour
//                       (prune_neighbour / uni_lookup), its row and the reciprocal counter. Writes the unitig's class and its two
//                       junctions (node position << 3 | counter) at the head's position, and ORs both junction counters' bits into
//                       the junction nodes' bytes of `cand` (a counter is named by at most one branch, but four nodes share a
//                       word: an atomic).
//   bubbles_judge       a SEPARATE launch: workgroups of one launch do not see each other's writes (the L2s of the XCDs are not
//                       coherent within a launch), and rule 5 reads the classes, junctions and candidate bits of the siblings. Per
//                       branch: the other counters >= t of its first junction end whose candidate bit is set; the neighbour behind
//                       such a counter is a sibling's end node, tips_head gives that branch's head, its two junctions say whether it
//                       is a sibling, and the two junction nodes' rows give its key. The keys of the two junction nodes are loaded
//                       only when the counter values tie. The verdict goes to `gone`, which no lane of this launch reads: the
//                       judge reads only what bubbles_classify wrote. A popped branch ORs both junction counters into `clr`.
//   tips_retain_count,  (kmi_dbg_tips.h) the removal of the tip clipping with `gone` as the class array: a node leaves when its
//   bucket_offsets,     unitig's head is TIP_GONE, and the copied row is ANDed with the complement of the node's clear byte
//   tips_retain_compact
// The class counts reach the global words as one atomic per wavefront and word (prune_flush). When nothing leaves, nothing is
// cleared either (a cleared counter belongs to a popped branch), and the arrays stay.
//
// Footprint per node beyond the compaction's stages: 16 bytes of junctions, 4 of masks, class and verdict.
//
// Included by kmi_index.hip after kmi_dbg_tips.h.
#pragma once

namespace kmi {

// device words of a pop call (TP_CLEARED and TP_SURVIVORS are the removal's, kmi_dbg_tips.h)
enum { BB_UNITIGS = 0, BB_BRANCHES = 1, BB_BUBBLES = 2, BB_POPPED = 3 };
enum : uint8_t { BUB_NONE = 0, BUB_BRANCH = 1 };

template <int NW>
__global__ __launch_bounds__(256) void bubbles_classify_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ edges, uint64_t n,
                                                              const uint32_t *__restrict__ tab, uint64_t mask, KShape shape, uint32_t t, bool exists,
                                                              const ulonglong2 *__restrict__ rk, const ulonglong2 *__restrict__ scan,
                                                              const uint8_t *__restrict__ dir, const uint8_t *__restrict__ circ, uint8_t *__restrict__ cls,
                                                              uint64_t *__restrict__ junc, uint32_t *__restrict__ cand,
                                                              unsigned long long *__restrict__ stats) {
  uint32_t n_uni = 0, n_br = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
    uint8_t c = BUB_NONE;
    if (scan[p].x != 0ull) {   // a head
      ++n_uni;
      const uint32_t d = dir[p];
      const ulonglong2 ad = rk[2u * p + d];
      if (!circ[p] && (uint64_t)((uint32_t)ad.x >> 1) < n) {
        // the states that leave the unitig, as tips_classify reads them
        const uint32_t es[2] = {2u * (uint32_t)p + 1u - d, (uint32_t)ad.x};
        uint32_t deg[2] = {0u, 0u}, jc[2] = {0u, 0u};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          uint32_t e[8];
          uni_counters(edges, es[i] >> 1, exists, e);
#pragma unroll
          for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t x = (es[i] & 1u) ? 4u + 3u - j : j;
            if (e[x] >= t) { ++deg[i]; jc[i] = x; }
          }
        }
        if (deg[0] == 1u && deg[1] == 1u) {
          uint64_t jn[2] = {0ull, 0ull};
          bool ok = true;
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            if (!ok) continue;
            const uint64_t v = es[i] >> 1;
            uint64_t key[NW], rc[NW], nb[NW];
            uni_load<NW>(keys, v, key);
            revcomp_words<NW, 2>(key, rc, shape);
            uint32_t recip;
            bool exempt;
            prune_neighbour<NW>(key, uni_eq<NW>(key, rc), jc[i], shape, nb, &recip, &exempt);
            const uint32_t w = uni_lookup<NW>(keys, tab, mask, nb);
            ok = w != kNoNext && (uint64_t)w < n && (uint64_t)tips_head(rk, dir, w) != p;   // a node, and not one of this unitig
            if (ok) {
              uint32_t f[8];
              uni_counters(edges, w, exists, f);
              ok = f[recip] >= t;
              jn[i] = ((uint64_t)w << 3) | recip;
            }
          }
          if (ok && (jn[0] >> 3) != (jn[1] >> 3)) {   // (a loop that leaves and re-enters one node is no branch)
            ++n_br;
            c = BUB_BRANCH;
            junc[2u * p] = jn[0]; junc[2u * p + 1u] = jn[1];
            tips_set(cand, jn[0] >> 3, (uint32_t)jn[0] & 7u);
            tips_set(cand, jn[1] >> 3, (uint32_t)jn[1] & 7u);
          }
        }
      }
    }
    cls[p] = c;
  }
  prune_flush(stats, BB_UNITIGS, n_uni);
  prune_flush(stats, BB_BRANCHES, n_br);
}

// rules 3-5: the siblings of a branch are found from its first junction end; key = (min, max of the junction counters, -base of
// the junction counter at the junction node with the smaller k-mer)
template <int NW>
__global__ __launch_bounds__(256) void bubbles_judge_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ edges, uint64_t n,
                                                           const uint32_t *__restrict__ tab, uint64_t mask, KShape shape, uint32_t t, bool exists,
                                                           uint32_t max_nodes, const ulonglong2 *__restrict__ rk, const uint8_t *__restrict__ dir,
                                                           const uint8_t *__restrict__ cls, const uint64_t *__restrict__ junc,
                                                           const uint32_t *__restrict__ cand, uint8_t *__restrict__ gone, uint32_t *__restrict__ clr,
                                                           unsigned long long *__restrict__ stats) {
  uint32_t n_bub = 0, n_pop = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
    uint8_t verdict = TIP_NONE;
    if (cls[p] == BUB_BRANCH) {
      const uint64_t j0 = junc[2u * p], j1 = junc[2u * p + 1u], w0 = j0 >> 3, w1 = j1 >> 3;
      const uint32_t r0 = (uint32_t)j0 & 7u, r1 = (uint32_t)j1 & 7u, lo = r0 & 4u;
      if (w0 < n && w1 < n) {
        uint32_t f0[8], f1[8];
        uni_counters(edges, w0, exists, f0);
        uni_counters(edges, w1, exists, f1);
        const uint32_t mn = min(f0[r0], f1[r1]), mx = max(f0[r0], f1[r1]);
        const uint32_t bits = tips_byte(cand, w0);
        uint64_t k0[NW], rc0[NW];
        uni_load<NW>(keys, w0, k0);
        revcomp_words<NW, 2>(k0, rc0, shape);
        const bool pal0 = uni_eq<NW>(k0, rc0);
        bool sibling = false, greater = false;
        int first = -1;   // 0: w0 has the smaller k-mer, 1: w1; found when a tie asks for it
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
          const uint32_t x = lo + b;
          if (x == r0 || f0[x] < t || !((bits >> x) & 1u)) continue;
          uint64_t nb[NW];
          uint32_t recip;
          bool exempt;
          prune_neighbour<NW>(k0, pal0, x, shape, nb, &recip, &exempt);
          const uint32_t v = uni_lookup<NW>(keys, tab, mask, nb);   // the end node of the branch that named (w0, x)
          if (v == kNoNext || (uint64_t)v >= n) continue;
          const uint64_t h = tips_head(rk, dir, v);
          if (h >= n || cls[h] != BUB_BRANCH) continue;
          const uint64_t y0 = junc[2u * h], y1 = junc[2u * h + 1u], here = (w0 << 3) | x;
          if (y0 != here && y1 != here) continue;
          const uint64_t yb = y0 == here ? y1 : y0;
          if ((yb >> 2) != (j1 >> 2)) continue;   // another junction end: no sibling
          sibling = true;
          const uint32_t c0 = f0[x], c1 = f1[(uint32_t)yb & 7u], ymn = min(c0, c1), ymx = max(c0, c1);
          if (ymn != mn || ymx != mx) {
            greater = greater || ymn > mn || (ymn == mn && ymx > mx);
            continue;
          }
          if (first < 0) {
            uint64_t k1[NW];
            uni_load<NW>(keys, w1, k1);
            first = less_words<NW>(k1, k0) ? 1 : 0;
          }
          const uint32_t mine = (first ? r1 : r0) & 3u, theirs = (first ? (uint32_t)yb : x) & 3u;
          greater = greater || theirs < mine;
        }
        n_bub += sibling && !greater ? 1u : 0u;
        if (greater && (rk[2u * p + dir[p]].x >> 32) + 1u <= (uint64_t)max_nodes) {
          ++n_pop;
          verdict = TIP_GONE;
          tips_set(clr, w0, r0);
          tips_set(clr, w1, r1);
        }
      }
    }
    gone[p] = verdict;
  }
  prune_flush(stats, BB_BUBBLES, n_bub);
  prune_flush(stats, BB_POPPED, n_pop);
}

// ---- host side ----
// stats: the eight words of kmi_dbg_pop_stats in its order
template <int NW>
static kmi_status dbg_pop_impl(kmi_dbg *g, uint32_t t, uint32_t max_nodes, uint64_t *stats) {
  kmi_ctx *ctx = g->ctx;
  kmi_index *idx = g->nodes;
  const uint64_t n = idx->n_entries, nw4 = (n + 3u) / 4u;
  const bool exists = g->node_kind == KMI_DBG_EDGE_EXISTS;
  const uint64_t *keys = (const uint64_t *)idx->keys;
  // the slot: device words, survivors per fine bucket, two junctions per node, candidate and clear bytes (four nodes a word), classes, verdicts
  void *p_bub;
  const size_t b_words = sizeof(unsigned long long) * TP_WORDS, b_cnt = sizeof(uint32_t) * kNumFine, b_junc = (size_t)n * 2u * sizeof(uint64_t),
               b_mask = (size_t)nw4 * sizeof(uint32_t);
  KMI_TRY(ws_get(ctx, WS_DBG_BUBBLES, b_words + b_cnt + b_junc + 2u * b_mask + 2u * (size_t)n + 16u, &p_bub));
  unsigned long long *d_stats = (unsigned long long *)p_bub;
  uint32_t *out_cnt = (uint32_t *)((char *)p_bub + b_words);
  uint64_t *junc = (uint64_t *)((char *)out_cnt + b_cnt);
  uint32_t *cand = (uint32_t *)((char *)junc + b_junc), *clr = cand + nw4;
  uint8_t *cls = (uint8_t *)(clr + nw4), *gone = cls + n;
  const uint32_t rounds = g->unitig_rounds;   // (the rounds of the last compaction are that call's to report)
  UniStages u;
  const kmi_status st = uni_stages<NW>(g, t, &u);
  g->unitig_rounds = rounds;
  KMI_TRY(st);
  uint64_t *new_off = nullptr;
  KMI_HIP(ctx, pool_alloc(ctx, (void **)&new_off, kOffBytes));
  hipError_t e = hipMemsetAsync(d_stats, 0, b_words, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(cand, 0, 2u * b_mask, ctx->stream);
  if (e == hipSuccess) {
    {
      ProfScope ps(ctx, "bubbles_classify", n);
      hipLaunchKernelGGL((bubbles_classify_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, (const uint32_t *)g->edges, n,
                         (const uint32_t *)u.tab, u.mask, g->shape, t, exists, (const ulonglong2 *)u.rk, (const ulonglong2 *)u.scan,
                         (const uint8_t *)u.dir, (const uint8_t *)u.circ, cls, junc, cand, d_stats);
    }
    {
      ProfScope ps(ctx, "bubbles_judge", n);
      hipLaunchKernelGGL((bubbles_judge_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, (const uint32_t *)g->edges, n,
                         (const uint32_t *)u.tab, u.mask, g->shape, t, exists, max_nodes, (const ulonglong2 *)u.rk, (const uint8_t *)u.dir,
                         (const uint8_t *)cls, (const uint64_t *)junc, (const uint32_t *)cand, gone, clr, d_stats);
    }
    {
      ProfScope ps(ctx, "tips_retain_count", n);
      hipLaunchKernelGGL(tips_retain_count_kernel, dim3(kNumFine / (kTipsCountThreads / kWave)), dim3(kTipsCountThreads), 0, ctx->stream,
                         (const ulonglong2 *)u.rk, (const uint8_t *)u.dir, (const uint8_t *)gone, (const uint32_t *)clr, (const uint64_t *)idx->bucket_off,
                         out_cnt, d_stats);
    }
    {
      ProfScope ps(ctx, "bucket_offsets", kNumFine);
      hipLaunchKernelGGL(bucket_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t *)out_cnt, new_off, (uint64_t *)d_stats,
                         (int)TP_SURVIVORS);
    }
    e = hipGetLastError();
  }
  uint64_t h[8] = {0};
  if (e == hipSuccess) e = hipMemcpyAsync(h, d_stats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { pool_free(ctx, new_off, kOffBytes); return set_err(ctx, KMI_ERR_DEVICE, "pop_bubbles: %s", hipGetErrorString(e)); }
  const uint64_t total = h[TP_SURVIVORS];
  if (total > n) { pool_free(ctx, new_off, kOffBytes); return set_err(ctx, KMI_ERR_DEVICE, "pop_bubbles: more survivors than nodes"); }
  stats[0] = n; stats[1] = h[BB_UNITIGS]; stats[2] = h[BB_BRANCHES]; stats[3] = h[BB_BUBBLES]; stats[4] = h[BB_POPPED];
  stats[5] = n - total; stats[6] = h[TP_CLEARED]; stats[7] = 0;
  if (total == n) {   // nothing leaves, so nothing was cleared: the map stays exactly as it is
    pool_free(ctx, new_off, kOffBytes);
    return KMI_OK;
  }
  uint64_t *nk = nullptr; uint32_t *nv = nullptr, *nr = nullptr;
  const size_t kb = (total ? total : 1) * NW * sizeof(uint64_t), vb = (total ? total : 1) * sizeof(uint32_t), rb = (total ? total : 1) * 8 * sizeof(uint32_t);
  const hipError_t e1 = pool_alloc(ctx, (void **)&nk, kb), e2 = pool_alloc(ctx, (void **)&nv, vb), e3 = pool_alloc(ctx, (void **)&nr, rb);
  auto release = [&]() {
    if (nk) pool_free(ctx, nk, kb);
    if (nv) pool_free(ctx, nv, vb);
    if (nr) pool_free(ctx, nr, rb);
    pool_free(ctx, new_off, kOffBytes);
  };
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
    release();
    return set_err(ctx, KMI_ERR_NOMEM, "hipMalloc failed for the node arrays");
  }
  if (total) {
    ProfScope ps(ctx, "tips_retain_compact", n);
    hipLaunchKernelGGL((tips_retain_compact_kernel<NW>), dim3(kNumFine), dim3(kRetainTile), 0, ctx->stream, keys, (const uint32_t *)idx->vals,
                       (const uint64_t *)idx->bucket_off, (const ulonglong2 *)u.rk, (const uint8_t *)u.dir, (const uint8_t *)gone, (const uint32_t *)clr,
                       (const uint64_t *)new_off, nk, nv, (const uint4 *)g->edges, (uint4 *)nr);
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {   // the map stays as it was
    release();
    return set_err(ctx, KMI_ERR_DEVICE, "pop_bubbles: %s", hipGetErrorString(e));
  }
  // the old arrays go back to the pool as in dbg_clip_impl
  pool_free(ctx, idx->keys, idx->keys_bytes);
  pool_free(ctx, idx->vals, idx->vals_bytes);
  pool_free(ctx, idx->bucket_off, kOffBytes);
  if (idx->dense_off) pool_free(ctx, idx->dense_off, kOffBytes);
  pool_free(ctx, g->edges, g->edges_bytes);
  idx->keys = nk; idx->vals = nv; idx->bucket_off = new_off; idx->dense_off = nullptr;
  idx->keys_bytes = kb; idx->vals_bytes = vb;
  idx->n_entries = total;
  g->edges = nr; g->edges_bytes = rb;
  return KMI_OK;
}

static kmi_status dbg_pop_bubbles(kmi_dbg *g, uint32_t min_edge_count, uint32_t max_bubble_nodes, uint32_t flags, uint64_t *stats) {
  kmi_ctx *ctx = g->ctx;
  memset(stats, 0, sizeof(uint64_t) * 8);
  if (g->shape.bits != 2) return set_err(ctx, KMI_ERR_INVALID, "pop_bubbles: only 2-bit alphabets");
  if (min_edge_count == 0) return set_err(ctx, KMI_ERR_INVALID, "pop_bubbles: min_edge_count must be at least 1");
  if (max_bubble_nodes == 0) return set_err(ctx, KMI_ERR_INVALID, "pop_bubbles: max_bubble_nodes must be at least 1");
  if (flags) return set_err(ctx, KMI_ERR_INVALID, "pop_bubbles: unknown flags");
  if (g->dist_share) return set_err(ctx, KMI_ERR_INVALID, "pop_bubbles: the map holds one rank's share of a build over ranks");
  kmi_index *idx = g->nodes;
  if (!idx->has_data || idx->n_entries == 0) { dbg_unitigs_drop(g); return KMI_OK; }
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  KMI_TRY(ensure_dense(idx));
  if (idx->n_entries >= 0x7FFFFFFFull) return set_err(ctx, KMI_ERR_OVERFLOW, "pop_bubbles: more than 2^31 - 2 nodes");
  kmi_status st = KMI_ERR_INVALID;
  switch (g->shape.n_words) {
    case 1: st = dbg_pop_impl<1>(g, min_edge_count, max_bubble_nodes, stats); break;
    case 2: st = dbg_pop_impl<2>(g, min_edge_count, max_bubble_nodes, stats); break;
    case 3: st = dbg_pop_impl<3>(g, min_edge_count, max_bubble_nodes, stats); break;
    case 4: st = dbg_pop_impl<4>(g, min_edge_count, max_bubble_nodes, stats); break;
  }
  if (st != KMI_OK) { memset(stats, 0, sizeof(uint64_t) * 8); return st; }
  dbg_unitigs_drop(g);   // (behind everything that can fail: a call that fails leaves the earlier compaction's result too)
  return KMI_OK;
}

}  // namespace kmi
