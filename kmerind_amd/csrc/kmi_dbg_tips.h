// Clipping the tips of a de Bruijn node map held whole by one rank (kmi_dbg_clip_tips; no counterpart in the reference: its
// test/test/debruijn/ ends at the node map). The definition is in include/kmerind_hip.h; here is how it is computed.
//
//   uni_stages          table, links, jumping, cycle pass, heads of kmi_unitig.h: afterwards every node knows its unitig's two end
//                       states (the final successors of its two states), its distance to both, and whether the unitig is a cycle
//   tips_classify       one lane per head node: the degrees of the unitig's two ends; dead + degree 1 -> the neighbour behind the
//                       single counter (prune_neighbour / uni_lookup), its row and the reciprocal counter. Writes the unitig's
//                       class and junction (node position << 3 | counter) at the head's position, and ORs the junction counter's
//                       bit into the junction node's byte of `cand` (a counter is named by at most one candidate, but four nodes
//                       share a word: an atomic). Islands are settled here.
//   tips_judge          a SEPARATE launch: workgroups of one launch do not see each other's writes (the L2s of the XCDs are not
//                       coherent within a launch), and rule 4 reads the candidate bits of every tip of the junction end. Per
//                       candidate: the junction node's row and candidate bits -> the verdict; a clipped tip turns its class into
//                       TIP_GONE and ORs its junction counter into the junction node's byte of `clr`.
//   tips_retain_count   fine bucket b, one wavefront each: the nodes whose unitig's head is not TIP_GONE; the counters cleared in them
//   bucket_offsets      (kmi_index.hip) the new bucket offsets and the number of survivors
//   tips_retain_compact the compaction of retain_counts (bucket_retain_compact_kernel) with that predicate; the copied row is ANDed
//                       with the complement of the node's clear byte
// The class counts reach the global words as one atomic per wavefront and word (prune_flush). When nothing leaves, nothing is
// cleared either (a cleared counter belongs to a clipped tip), and the arrays stay.
//
// Footprint per node beyond the compaction's stages: 8 bytes of junction, 3 of masks and class.
//
// Included by kmi_index.hip after kmi_dbg_clean.h.
#pragma once

namespace kmi {

// device words of a clip call
enum { TP_UNITIGS = 0, TP_CAND = 1, TP_CLIPPED = 2, TP_ISLANDS = 3, TP_CLEARED = 4, TP_SURVIVORS = 5, TP_WORDS = 16 };
enum : uint8_t { TIP_NONE = 0, TIP_GONE = 1, TIP_CAND = 2 };

// the head of node p's unitig: the final successor of its state against the spelling direction, turned round
__device__ __forceinline__ uint32_t tips_head(const ulonglong2 *__restrict__ rk, const uint8_t *__restrict__ dir, uint64_t p) {
  return ((uint32_t)rk[2u * p + 1u - dir[p]].x ^ 1u) >> 1;
}
// node w's byte of a mask array: bit j = counter j
__device__ __forceinline__ uint32_t tips_byte(const uint32_t *__restrict__ m, uint64_t w) { return (m[w >> 2] >> (8u * (uint32_t)(w & 3u))) & 0xFFu; }
__device__ __forceinline__ void tips_set(uint32_t *__restrict__ m, uint64_t w, uint32_t j) { atomicOr(&m[w >> 2], 1u << (8u * (uint32_t)(w & 3u) + j)); }

template <int NW>
__global__ __launch_bounds__(256) void tips_classify_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ edges, uint64_t n,
                                                           const uint32_t *__restrict__ tab, uint64_t mask, KShape shape, uint32_t t, bool exists,
                                                           uint32_t max_nodes, bool islands, const ulonglong2 *__restrict__ rk,
                                                           const ulonglong2 *__restrict__ scan, const uint8_t *__restrict__ dir,
                                                           const uint8_t *__restrict__ circ, uint8_t *__restrict__ cls, uint64_t *__restrict__ junc,
                                                           uint32_t *__restrict__ cand, unsigned long long *__restrict__ stats) {
  uint32_t n_uni = 0, n_cand = 0, n_isl = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
    uint8_t c = TIP_NONE;
    if (scan[p].x != 0ull) {   // a head
      ++n_uni;
      const uint32_t d = dir[p];
      const ulonglong2 ad = rk[2u * p + d];
      if (!circ[p] && (ad.x >> 32) + 1u <= (uint64_t)max_nodes && (uint64_t)((uint32_t)ad.x >> 1) < n) {
        // the states that leave the unitig: the head against the spelling direction, the tail along it; state (q, o) leaves by q's out
        // end (o = 0) or in end (o = 1), where base j of the strand read is in-counter comp(j)
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
        if (deg[0] + deg[1] == 0u) {
          ++n_isl;
          c = islands ? TIP_GONE : TIP_NONE;
        } else if (deg[0] + deg[1] == 1u) {   // one end dead, the other with a single counter
          const int i = (int)deg[1];
          const uint64_t v = es[i] >> 1;
          uint64_t key[NW], rc[NW], nb[NW];
          uni_load<NW>(keys, v, key);
          revcomp_words<NW, 2>(key, rc, shape);
          uint32_t recip;
          bool exempt;
          prune_neighbour<NW>(key, uni_eq<NW>(key, rc), jc[i], shape, nb, &recip, &exempt);
          const uint32_t w = uni_lookup<NW>(keys, tab, mask, nb);
          if (w != kNoNext && (uint64_t)w < n && (uint64_t)tips_head(rk, dir, w) != p) {   // a node, and not one of this unitig
            uint32_t f[8];
            uni_counters(edges, w, exists, f);
            if (f[recip] >= t) {
              ++n_cand;
              c = TIP_CAND;
              junc[p] = ((uint64_t)w << 3) | recip;
              tips_set(cand, w, recip);
            }
          }
        }
      }
    }
    cls[p] = c;
  }
  prune_flush(stats, TP_UNITIGS, n_uni);
  prune_flush(stats, TP_CAND, n_cand);
  prune_flush(stats, TP_ISLANDS, n_isl);
}

// rule 4: counters >= t of the junction end ordered by (value, not a candidate's junction counter, -base); a candidate that is not
// the greatest is clipped
__global__ __launch_bounds__(256) void tips_judge_kernel(const uint32_t *__restrict__ edges, uint64_t n, uint32_t t, bool exists,
                                                        uint8_t *__restrict__ cls, const uint64_t *__restrict__ junc, const uint32_t *__restrict__ cand,
                                                        uint32_t *__restrict__ clr, unsigned long long *__restrict__ stats) {
  uint32_t n_clip = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
    if (cls[p] != TIP_CAND) continue;
    const uint64_t w = junc[p] >> 3;
    const uint32_t j = (uint32_t)junc[p] & 7u, lo = j & 4u;
    bool clip = false;
    if (w < n) {
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
    }
    cls[p] = clip ? TIP_GONE : TIP_NONE;
    if (clip) { ++n_clip; tips_set(clr, w, j); }
  }
  prune_flush(stats, TP_CLIPPED, n_clip);
}

// Fine bucket b, one wavefront each: how many of its nodes stay, and the counters cleared in those
constexpr int kTipsCountThreads = 256;
__global__ __launch_bounds__(kTipsCountThreads) void tips_retain_count_kernel(const ulonglong2 *__restrict__ rk, const uint8_t *__restrict__ dir,
                                                                             const uint8_t *__restrict__ cls, const uint32_t *__restrict__ clr,
                                                                             const uint64_t *__restrict__ idx_off, uint32_t *__restrict__ out_cnt,
                                                                             unsigned long long *__restrict__ stats) {
  const uint32_t b = blockIdx.x * (kTipsCountThreads / kWave) + wave_id();   // (the grid is kNumFine wavefronts exactly)
  const uint64_t ib = idx_off[b], ie = idx_off[b + 1];
  uint32_t keep = 0, cleared = 0;
  for (uint64_t i = ib + lane_id(); i < ie; i += kWave) {
    if (cls[tips_head(rk, dir, i)] == TIP_GONE) continue;
    ++keep;
    cleared += (uint32_t)__popc(tips_byte(clr, i));
  }
  keep = wave_reduce_sum(keep);
  if (lane_id() == 0) out_cnt[b] = keep;
  prune_flush(stats, TP_CLEARED, cleared);
}

// bucket_retain_compact_kernel with the predicate "the unitig's head is not TIP_GONE"; the rows lose the counters of the clear byte
template <int NW>
__global__ __launch_bounds__(kRetainTile) void tips_retain_compact_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                                         const uint64_t *__restrict__ idx_off, const ulonglong2 *__restrict__ rk,
                                                                         const uint8_t *__restrict__ dir, const uint8_t *__restrict__ cls,
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
    const bool keep = i < ie && cls[tips_head(rk, dir, i)] != TIP_GONE;
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
// stats: the eight words of kmi_dbg_clip_stats in its order
template <int NW>
static kmi_status dbg_clip_impl(kmi_dbg *g, uint32_t t, uint32_t max_nodes, uint32_t flags, uint64_t *stats) {
  kmi_ctx *ctx = g->ctx;
  kmi_index *idx = g->nodes;
  const uint64_t n = idx->n_entries, nw4 = (n + 3u) / 4u;
  const bool exists = g->node_kind == KMI_DBG_EDGE_EXISTS;
  const bool islands = (flags & KMI_DBG_CLIP_ISLANDS) != 0;
  const uint64_t *keys = (const uint64_t *)idx->keys;
  // the slot: device words, survivors per fine bucket, junction per node, candidate and clear bytes (four nodes a word), classes
  void *p_tips;
  const size_t b_words = sizeof(unsigned long long) * TP_WORDS, b_cnt = sizeof(uint32_t) * kNumFine, b_junc = (size_t)n * sizeof(uint64_t),
               b_mask = (size_t)nw4 * sizeof(uint32_t);
  KMI_TRY(ws_get(ctx, WS_DBG_TIPS, b_words + b_cnt + b_junc + 2u * b_mask + (size_t)n + 16u, &p_tips));
  unsigned long long *d_stats = (unsigned long long *)p_tips;
  uint32_t *out_cnt = (uint32_t *)((char *)p_tips + b_words);
  uint64_t *junc = (uint64_t *)((char *)out_cnt + b_cnt);
  uint32_t *cand = (uint32_t *)((char *)junc + b_junc), *clr = cand + nw4;
  uint8_t *cls = (uint8_t *)(clr + nw4);
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
      ProfScope ps(ctx, "tips_classify", n);
      hipLaunchKernelGGL((tips_classify_kernel<NW>), dim3(uni_grid(n)), dim3(256), 0, ctx->stream, keys, (const uint32_t *)g->edges, n,
                         (const uint32_t *)u.tab, u.mask, g->shape, t, exists, max_nodes, islands, (const ulonglong2 *)u.rk, (const ulonglong2 *)u.scan,
                         (const uint8_t *)u.dir, (const uint8_t *)u.circ, cls, junc, cand, d_stats);
    }
    {
      ProfScope ps(ctx, "tips_judge", n);
      hipLaunchKernelGGL(tips_judge_kernel, dim3(uni_grid(n)), dim3(256), 0, ctx->stream, (const uint32_t *)g->edges, n, t, exists, cls,
                         (const uint64_t *)junc, (const uint32_t *)cand, clr, d_stats);
    }
    {
      ProfScope ps(ctx, "tips_retain_count", n);
      hipLaunchKernelGGL(tips_retain_count_kernel, dim3(kNumFine / (kTipsCountThreads / kWave)), dim3(kTipsCountThreads), 0, ctx->stream,
                         (const ulonglong2 *)u.rk, (const uint8_t *)u.dir, (const uint8_t *)cls, (const uint32_t *)clr, (const uint64_t *)idx->bucket_off,
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
  if (e != hipSuccess) { pool_free(ctx, new_off, kOffBytes); return set_err(ctx, KMI_ERR_DEVICE, "clip_tips: %s", hipGetErrorString(e)); }
  const uint64_t total = h[TP_SURVIVORS];
  if (total > n) { pool_free(ctx, new_off, kOffBytes); return set_err(ctx, KMI_ERR_DEVICE, "clip_tips: more survivors than nodes"); }
  stats[0] = n; stats[1] = h[TP_UNITIGS]; stats[2] = h[TP_CAND]; stats[3] = h[TP_CLIPPED]; stats[4] = h[TP_ISLANDS];
  stats[5] = islands ? h[TP_ISLANDS] : 0; stats[6] = n - total; stats[7] = h[TP_CLEARED];
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
                       (const uint64_t *)idx->bucket_off, (const ulonglong2 *)u.rk, (const uint8_t *)u.dir, (const uint8_t *)cls, (const uint32_t *)clr,
                       (const uint64_t *)new_off, nk, nv, (const uint4 *)g->edges, (uint4 *)nr);
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {   // the map stays as it was
    release();
    return set_err(ctx, KMI_ERR_DEVICE, "clip_tips: %s", hipGetErrorString(e));
  }
  // the old arrays go back to the pool as in retain_counts_impl (the index is dense here: no bucket_cnt)
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

static kmi_status dbg_clip_tips(kmi_dbg *g, uint32_t min_edge_count, uint32_t max_tip_nodes, uint32_t flags, uint64_t *stats) {
  kmi_ctx *ctx = g->ctx;
  memset(stats, 0, sizeof(uint64_t) * 8);
  if (g->shape.bits != 2) return set_err(ctx, KMI_ERR_INVALID, "clip_tips: only 2-bit alphabets");
  if (min_edge_count == 0) return set_err(ctx, KMI_ERR_INVALID, "clip_tips: min_edge_count must be at least 1");
  if (max_tip_nodes == 0) return set_err(ctx, KMI_ERR_INVALID, "clip_tips: max_tip_nodes must be at least 1");
  if (flags & ~(uint32_t)KMI_DBG_CLIP_ISLANDS) return set_err(ctx, KMI_ERR_INVALID, "clip_tips: unknown flags");
  if (g->dist_share) return set_err(ctx, KMI_ERR_INVALID, "clip_tips: the map holds one rank's share of a build over ranks");
  kmi_index *idx = g->nodes;
  if (!idx->has_data || idx->n_entries == 0) { dbg_unitigs_drop(g); return KMI_OK; }
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  KMI_TRY(ensure_dense(idx));
  if (idx->n_entries >= 0x7FFFFFFFull) return set_err(ctx, KMI_ERR_OVERFLOW, "clip_tips: more than 2^31 - 2 nodes");
  kmi_status st = KMI_ERR_INVALID;
  switch (g->shape.n_words) {
    case 1: st = dbg_clip_impl<1>(g, min_edge_count, max_tip_nodes, flags, stats); break;
    case 2: st = dbg_clip_impl<2>(g, min_edge_count, max_tip_nodes, flags, stats); break;
    case 3: st = dbg_clip_impl<3>(g, min_edge_count, max_tip_nodes, flags, stats); break;
    case 4: st = dbg_clip_impl<4>(g, min_edge_count, max_tip_nodes, flags, stats); break;
  }
  if (st != KMI_OK) { memset(stats, 0, sizeof(uint64_t) * 8); return st; }
  dbg_unitigs_drop(g);   // (behind everything that can fail: a call that fails leaves the earlier compaction's result too)
  return KMI_OK;
}

}  // namespace kmi
