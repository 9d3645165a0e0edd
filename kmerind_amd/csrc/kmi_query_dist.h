// The queries in the caller's order over ranks: kmi_index_lookup_dist_*, kmi_index_profile_reads_dist_*, kmi_index_locate_dist_*,
// kmi_index_seed_reads_dist_* (collective; no counterpart in the reference, see kmi_lookup.h and kmi_locate.h). A key lives wholly
// on the rank that owns it, so a rank's queries travel to the owners, are answered there by the one-rank code ONCE over everything
// that arrived (all sources concatenated: the answers come in the order of the received keys, so source s's share is a contiguous
// slice), and the answers travel back. One round:
//   a. tag and route   the queries are (key words, position in the caller's array) records; route_pairs groups them by owner --
//                      the minimizer-bucket owner when idx->owner_lp says so, KeyToRank else -- in an order it does not specify;
//                      qd_split_kernel writes the key column into the send buffer and keeps the position column as perm[]
//                      (perm[j] = the query at routed place j). The position word is not sent.
//   (verdict)          one all-reduce: this rank's status so far (a parse error, the record limit), "I still have input", "I want
//                      values". Any error ends the call on every rank: the failing rank with its own, the others KMI_ERR_PEER.
//   b. exchange        the keys (dist_exchange), the owner's lookup_impl / locate_count_impl + locate_fill over all of them; a
//                      second all-reduce carries the owner's verdict (a bucket past the pass limit)
//   c. return          count / occ, 4 bytes per key, with the forward counts reversed (no count exchange); for locate the listed
//                      value words as one message per source, whose sizes both sides know already: the owner from its offsets at
//                      the source boundaries, the source from the offsets it rebuilds from the returned occ and max_occ
//   d. query order     counts[perm[j]] = ans[j], slot[perm[j]] = j; offsets = the scan of listed(i) in query order; the values by
//                      qd_segcopy_kernel, a segmented copy from the routed-order CSR to the query-order CSR driven by the OUTPUT
// The reads forms run one round per record-aligned batch of KMI_PROFILE_BATCH bytes; a rank that has run out of input takes part
// with zero queries until the "I still have input" sum is zero. A short capacity changes nothing that is sent or received.
//
// Included by kmi_index.hip behind the collectives' helpers (dist_check, dist_exchange, dist_agree).
#pragma once

namespace kmi {

// routed records (key words, position) -> the key column (what is sent) and the position column (what stays)
template <int NW>
__global__ __launch_bounds__(256) void qd_split_kernel(const uint64_t *__restrict__ recs, uint64_t n, uint64_t *__restrict__ keys,
                                                      uint64_t *__restrict__ perm) {
  constexpr int RW = NW + 1;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int w = 0; w < NW; ++w) keys[j * NW + w] = recs[j * RW + w];
    perm[j] = recs[j * RW + NW];
  }
}

// out[perm[j]] = ans[j]; slot (when asked for) becomes the inverse of perm
__global__ __launch_bounds__(256) void qd_scatter_kernel(const uint32_t *__restrict__ ans, const uint64_t *__restrict__ perm, uint64_t n,
                                                        uint32_t *__restrict__ out, uint64_t *__restrict__ slot) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = perm[j];
    if (i >= n) continue;   // (never: the positions are a permutation of 0 .. n - 1)
    out[i] = ans[j];
    if (slot) slot[i] = j;
  }
}

// The segmented copy, driven by the output. Workgroup t owns the hits [base + t * kSegCopyTile, ...) of the query-order CSR; lane
// l writes hit h0 + u * kSegCopyThreads + l in step u, so a wavefront's stores are whole lines whatever the segments look like.
// The tile's first query is one binary search of offsets[]; from there the queries' offsets -- and where each one's hits start in
// the routed-order CSR, routed_off[slot[i]] -- pass through LDS in chunks of kSegCopyChunk, and every hit finds its query by a
// binary search of the chunk in LDS: hit h of query i is read from routed place routed_off[slot[i]] + (h - offsets[i]). No lane
// walks a query's hits, so a key with 10^5 hits costs what 10^5 keys with one hit cost; queries without listed hits only pass
// through LDS. offsets[0] = base, offsets[n] = end.
constexpr int kSegCopyChunk = 1024;
template <int VW>
__global__ __launch_bounds__(kSegCopyThreads) void qd_segcopy_kernel(const uint64_t *__restrict__ offsets, const uint64_t *__restrict__ slot,
                                                                    const uint64_t *__restrict__ routed_off, const uint64_t *__restrict__ routed_vals,
                                                                    uint64_t n_routed_hits, uint64_t n, uint64_t base, uint64_t end,
                                                                    uint64_t *__restrict__ values) {
  __shared__ uint64_t s_off[kSegCopyChunk + 1];
  __shared__ uint64_t s_src[kSegCopyChunk];
  __shared__ uint64_t s_first;
  const uint64_t h0 = base + (uint64_t)blockIdx.x * kSegCopyTile;
  if (h0 >= end || n == 0) return;   // (uniform)
  const uint64_t h1 = h0 + kSegCopyTile < end ? h0 + kSegCopyTile : end;
  if (threadIdx.x == 0) {
    // the last i with offsets[i] <= h0: offsets[0] = base <= h0 < end = offsets[n], so it lies below n and holds hit h0
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (offsets[mid] <= h0) lo = mid; else hi = mid;
    }
    s_first = lo;
  }
  __syncthreads();
  uint64_t c0 = s_first;
  while (true) {
    const uint32_t cn = (uint32_t)(n - c0 < (uint64_t)kSegCopyChunk ? n - c0 : (uint64_t)kSegCopyChunk);   // (at least 1: c0 < n)
    for (uint32_t c = threadIdx.x; c <= cn; c += kSegCopyThreads) s_off[c] = offsets[c0 + c];
    for (uint32_t c = threadIdx.x; c < cn; c += kSegCopyThreads) {
      const uint64_t s = slot[c0 + c];
      s_src[c] = s < n ? routed_off[s] : n_routed_hits;
    }
    __syncthreads();
    const uint64_t lo_h = s_off[0], hi_h = s_off[cn];
#pragma unroll
    for (int u = 0; u < kSegCopyPerThread; ++u) {
      const uint64_t h = h0 + (uint64_t)u * kSegCopyThreads + threadIdx.x;
      if (h < h1 && h >= lo_h && h < hi_h) {
        uint32_t lo = 0, hi = cn;   // s_off[lo] <= h < s_off[hi]
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) / 2;
          if (s_off[mid] <= h) lo = mid; else hi = mid;
        }
        const uint64_t src = s_src[lo] + (h - s_off[lo]);
        if (src < n_routed_hits) {   // (always: both CSRs list the same hits per query)
#pragma unroll
          for (int w = 0; w < VW; ++w) values[h * VW + w] = routed_vals[src * VW + w];
        }
      }
    }
    if (hi_h >= h1 || c0 + cn >= n) break;   // (uniform: both from LDS words every lane read)
    c0 += cn;
    __syncthreads();   // (the next chunk overwrites the LDS arrays)
  }
}

// ---- host side
// what the tagging and routing of a round leaves: the send buffer grouped by owner, perm[], and after the exchange the keys received
struct QdState {
  size_t n = 0;
  std::vector<uint64_t> sc, rc;   // keys this rank sends to / has received from every rank
  uint64_t *send = nullptr, *perm = nullptr;
  void *d_q = nullptr;
  uint64_t total = 0;
};

// step a, local: recs_dev = n records (key words, position), consumed here
template <int NW, int BITS>
static kmi_status qd_prep(kmi_index *idx, kmi_comm *comm, const uint64_t *recs_dev, size_t n, QdState *qs) {
  kmi_ctx *ctx = idx->ctx;
  constexpr int RW = NW + 1;
  const int p = comm_size(comm);
  qs->n = n;
  qs->sc.assign(p, 0);
  void *routed, *w;
  KMI_TRY(ws_get(ctx, WS_DIST_D, (n + 8) * RW * sizeof(uint64_t), &routed));
  KMI_TRY(ws_get(ctx, WS_DIST_A, (n + 8) * NW * sizeof(uint64_t), &w)); qs->send = (uint64_t *)w;
  KMI_TRY(ws_get(ctx, WS_QD_PERM, (n + 8) * sizeof(uint64_t), &w)); qs->perm = (uint64_t *)w;
  KMI_TRY(route_pairs(ctx, &idx->cfg, idx->shape, recs_dev, n, (uint32_t)p, idx->owner_lp != 0, (uint64_t *)routed, qs->sc.data()));
  if (n) {
    ProfScope ps(ctx, "qd_split", n);
    hipLaunchKernelGGL((qd_split_kernel<NW>), dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 8192)), dim3(256), 0, ctx->stream,
                       (const uint64_t *)routed, (uint64_t)n, qs->send, qs->perm);
    KMI_HIP(ctx, hipGetLastError());
  }
  return KMI_OK;
}

// the verdict before a round's first exchange, with two riders summed over the ranks
static kmi_status qd_agree(kmi_comm *comm, kmi_status mine, uint64_t *more, uint64_t *want) {
  uint64_t w[3] = {mine != KMI_OK ? 1ull : 0ull, *more, *want};
  const kmi_status st = comm_allreduce_sum(comm, w, 3);
  if (mine != KMI_OK) return mine;
  if (st != KMI_OK) return st;
  if (w[0]) return set_err(comm_ctx(comm), KMI_ERR_PEER, "the collective was given up: another rank reported an error");
  *more = w[1]; *want = w[2];
  return KMI_OK;
}

// offs_dev at the boundaries of consecutive groups of cnt[s] elements: out[s] = the group's sum (synchronises)
static kmi_status qd_boundaries(kmi_ctx *ctx, const uint64_t *offs_dev, const std::vector<uint64_t> &cnt, std::vector<uint64_t> *out) {
  const size_t p = cnt.size();
  std::vector<uint64_t> b(p + 1, 0);
  uint64_t at = 0;
  for (size_t s = 0; s <= p; ++s) {
    KMI_HIP(ctx, hipMemcpyAsync(&b[s], offs_dev + at, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (s < p) at += cnt[s];
  }
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  out->assign(p, 0);
  for (size_t s = 0; s < p; ++s) (*out)[s] = b[s + 1] - b[s];
  return KMI_OK;
}

static unsigned qd_grid(uint64_t n) { return (unsigned)std::min<uint64_t>(n ? (n + 255) / 256 : 1, 8192); }

// steps b to d of a lookup round: counts_out[i] (device, qs->n words) for the records qd_prep took
template <int NW, int BITS>
static kmi_status qd_lookup_finish(kmi_index *idx, kmi_comm *comm, QdState *qs, uint32_t *counts_out, uint64_t *npass) {
  kmi_ctx *ctx = idx->ctx;
  KMI_TRY(dist_exchange(comm, qs->send, qs->sc.data(), NW * sizeof(uint64_t), WS_DIST_B, &qs->d_q, qs->rc, &qs->total));
  ctx->qd_answered += qs->total;
  uint32_t *rans = nullptr, *ans = nullptr;
  const kmi_status mine = [&]() -> kmi_status {
    void *w;
    KMI_TRY(ws_get(ctx, WS_QD_RANS, (qs->total + 8) * sizeof(uint32_t), &w)); rans = (uint32_t *)w;
    KMI_TRY(ws_get(ctx, WS_QD_ANS, (qs->n + 8) * sizeof(uint32_t), &w)); ans = (uint32_t *)w;
    const kmi_status st = lookup_impl<NW, BITS>(idx, (const uint64_t *)qs->d_q, (size_t)qs->total, rans);
    *npass = std::max<uint64_t>(*npass, ctx->lookup_npass);
    return st;
  }();
  KMI_TRY(dist_agree(comm, mine));   // (a bucket past the pass limit on one owner: nobody waits for its answers)
  KMI_TRY(comm_all_to_all_v(comm, rans, qs->rc.data(), ans, qs->sc.data(), sizeof(uint32_t)));
  if (qs->n) {
    ProfScope ps(ctx, "qd_scatter", qs->n);
    hipLaunchKernelGGL(qd_scatter_kernel, dim3(qd_grid(qs->n)), dim3(256), 0, ctx->stream, (const uint32_t *)ans, (const uint64_t *)qs->perm,
                       (uint64_t)qs->n, counts_out, (uint64_t *)nullptr);
    KMI_HIP(ctx, hipGetLastError());
  }
  return KMI_OK;
}

template <int VW>
static kmi_status qd_segcopy(kmi_ctx *ctx, const uint64_t *offsets, const uint64_t *slot, const uint64_t *routed_off, const uint64_t *routed_vals,
                             uint64_t n_routed_hits, uint64_t n, uint64_t base, uint64_t end, uint64_t *values) {
  const uint64_t tiles = (end - base + kSegCopyTile - 1) / kSegCopyTile;
  ProfScope ps(ctx, "qd_segcopy", end - base);
  hipLaunchKernelGGL((qd_segcopy_kernel<VW>), dim3((unsigned)tiles), dim3(kSegCopyThreads), 0, ctx->stream, offsets, slot, routed_off, routed_vals,
                     n_routed_hits, n, base, end, values);
  KMI_HIP(ctx, hipGetLastError());
  return KMI_OK;
}

// steps b to d of a locate round. occ_out (qs->n words) and offs_out (qs->n + 1 words, from `base`) are always written and
// *hits_end = base + this rank's listed hits. any_vals: some rank wants values, so they travel; this rank's land in values_out
// (hit h at word h * val_words) when it gave a buffer and they fit below cap_hits. Synchronises.
template <int NW, int BITS>
static kmi_status qd_locate_finish(kmi_index *idx, kmi_comm *comm, QdState *qs, uint32_t max_occ, bool any_vals, uint32_t *occ_out,
                                   uint64_t *offs_out, uint64_t base, uint64_t *values_out, size_t cap_hits, uint64_t *hits_end, uint64_t *npass) {
  kmi_ctx *ctx = idx->ctx;
  const size_t vb = idx->val_words * sizeof(uint64_t);
  KMI_TRY(dist_exchange(comm, qs->send, qs->sc.data(), NW * sizeof(uint64_t), WS_DIST_B, &qs->d_q, qs->rc, &qs->total));
  ctx->qd_answered += qs->total;
  uint32_t *rans = nullptr, *ans = nullptr;
  uint64_t *roffs = nullptr, *rvals = nullptr, *slot = nullptr, *offs = nullptr;
  std::vector<uint64_t> back, got;
  const size_t total = (size_t)qs->total, n = qs->n;
  // the owner's half: occ and offsets over everything that arrived, the listed values behind them, the hits of every source
  const kmi_status mine = [&]() -> kmi_status {
    void *w;
    KMI_TRY(ws_get(ctx, WS_QD_RANS, (total + 8) * sizeof(uint32_t), &w)); rans = (uint32_t *)w;
    KMI_TRY(ws_get(ctx, WS_QD_ROFFS, (total + 8) * sizeof(uint64_t), &w)); roffs = (uint64_t *)w;
    KMI_TRY(ws_get(ctx, WS_QD_ANS, (n + 8) * sizeof(uint32_t), &w)); ans = (uint32_t *)w;
    KMI_TRY(ws_get(ctx, WS_QD_SLOT, (n + 8) * sizeof(uint64_t), &w)); slot = (uint64_t *)w;
    KMI_TRY(ws_get(ctx, WS_QD_OFFS, (n + 8) * sizeof(uint64_t), &w)); offs = (uint64_t *)w;
    KMI_TRY(ws_get(ctx, WS_LOOKUP_RECS, (total + 8) * (NW + 1) * sizeof(uint64_t), &w));
    uint64_t *recs = (uint64_t *)w;
    KMI_TRY(lookup_begin(ctx));
    hipLaunchKernelGGL((lookup_zip_kernel<NW>), dim3(2048), dim3(256), 0, ctx->stream, (const uint64_t *)qs->d_q, (uint64_t)total, recs);
    Partitioned part;
    bool partitioned = false;
    uint64_t rend = 0;
    KMI_TRY((locate_count_impl<NW, BITS>(idx, recs, total, max_occ, rans, roffs, 0, &rend, &part, &partitioned)));
    KMI_TRY(ws_get(ctx, WS_QD_RVALS, (rend + 8) * vb, &w)); rvals = (uint64_t *)w;
    if (any_vals && rend && partitioned) KMI_TRY((locate_fill<NW>(idx, part, total, max_occ, roffs, rvals)));
    KMI_TRY(lookup_end(ctx));
    *npass = std::max<uint64_t>(*npass, ctx->lookup_npass);
    return qd_boundaries(ctx, roffs, qs->rc, &back);
  }();
  KMI_TRY(dist_agree(comm, mine));
  KMI_TRY(comm_all_to_all_v(comm, rans, qs->rc.data(), ans, qs->sc.data(), sizeof(uint32_t)));
  // the routed-order CSR: its offsets from the occ that came back; their values at the source boundaries are the messages' sizes
  KMI_TRY(device_exclusive_scan(ctx, ListedIn{ans, max_occ}, OffsetsOut{offs}, (uint64_t)n, 0, ctx->d_totals + TOT_LOCATE_HITS, true));
  KMI_TRY(qd_boundaries(ctx, offs, qs->sc, &got));
  uint64_t n_routed = 0;
  for (uint64_t g : got) n_routed += g;
  uint64_t *vals = nullptr;
  if (any_vals) {
    void *w;
    KMI_TRY(ws_get(ctx, WS_QD_VALS, (n_routed + 8) * vb, &w)); vals = (uint64_t *)w;
    KMI_TRY(comm_all_to_all_v(comm, rvals, back.data(), vals, got.data(), vb));
  }
  if (n) {
    ProfScope ps(ctx, "qd_scatter", n);
    hipLaunchKernelGGL(qd_scatter_kernel, dim3(qd_grid(n)), dim3(256), 0, ctx->stream, (const uint32_t *)ans, (const uint64_t *)qs->perm, (uint64_t)n,
                       occ_out, slot);
    KMI_HIP(ctx, hipGetLastError());
  }
  KMI_TRY(device_exclusive_scan(ctx, ListedIn{occ_out, max_occ}, OffsetsOut{offs_out}, (uint64_t)n, base, ctx->d_totals + TOT_LOCATE_HITS, true));
  KMI_TRY(locate_read_total(ctx, TOT_LOCATE_HITS, hits_end));
  if (vals && values_out && n && *hits_end > base && *hits_end <= cap_hits) {
    if (idx->val_words == 1) KMI_TRY((qd_segcopy<1>(ctx, offs_out, slot, offs, vals, n_routed, n, base, *hits_end, values_out)));
    else KMI_TRY((qd_segcopy<2>(ctx, offs_out, slot, offs, vals, n_routed, n, base, *hits_end, values_out)));
  }
  return KMI_OK;
}

// ---- lookup
template <int NW, int BITS>
static kmi_status lookup_dist_impl(kmi_index *idx, kmi_comm *comm, const uint64_t *q_dev, size_t nq, uint32_t *counts_dev) {
  kmi_ctx *ctx = idx->ctx;
  ctx->qd_answered = 0;
  QdState qs;
  const kmi_status mine = [&]() -> kmi_status {
    void *w;
    KMI_TRY(ws_get(ctx, WS_DIST_C, (nq + 8) * (NW + 1) * sizeof(uint64_t), &w));
    if (nq) hipLaunchKernelGGL((lookup_zip_kernel<NW>), dim3(2048), dim3(256), 0, ctx->stream, q_dev, (uint64_t)nq, (uint64_t *)w);
    return qd_prep<NW, BITS>(idx, comm, (const uint64_t *)w, nq, &qs);
  }();
  uint64_t more = 0, want = 0, npass = 0;
  KMI_TRY(qd_agree(comm, mine, &more, &want));
  KMI_TRY((qd_lookup_finish<NW, BITS>(idx, comm, &qs, counts_dev, &npass)));
  ctx->lookup_npass = npass;
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KMI_OK;
}
static kmi_status index_lookup_dist(kmi_index *idx, kmi_comm *comm, const uint64_t *q_dev, size_t nq, uint32_t *counts_dev) {
  KMI_DISPATCH(idx->shape, lookup_dist_impl, idx, comm, q_dev, nq, counts_dev);
}

// ---- locate
template <int NW, int BITS>
static kmi_status locate_dist_impl(kmi_index *idx, kmi_comm *comm, const uint64_t *q_dev, size_t nq, uint32_t max_occ, uint32_t *occ_dev,
                                   uint64_t *offs_dev, uint64_t *values_dev, size_t capacity, uint64_t *n_hits) {
  kmi_ctx *ctx = idx->ctx;
  ctx->qd_answered = 0;
  QdState qs;
  const kmi_status mine = [&]() -> kmi_status {
    void *w;
    KMI_TRY(ws_get(ctx, WS_DIST_C, (nq + 8) * (NW + 1) * sizeof(uint64_t), &w));
    if (nq) hipLaunchKernelGGL((lookup_zip_kernel<NW>), dim3(2048), dim3(256), 0, ctx->stream, q_dev, (uint64_t)nq, (uint64_t *)w);
    return qd_prep<NW, BITS>(idx, comm, (const uint64_t *)w, nq, &qs);
  }();
  const bool sizing = !values_dev && capacity == 0;
  uint64_t more = 0, want = sizing ? 0 : 1, npass = 0;
  KMI_TRY(qd_agree(comm, mine, &more, &want));
  uint32_t *occ = occ_dev;
  if (nq == 0) {   // (no other buffer than offsets is touched then; the round still wants a place for its zero answers)
    void *w;
    KMI_TRY(ws_get(ctx, WS_LOOKUP_CNT, 64, &w));
    occ = (uint32_t *)w;
  }
  KMI_TRY((qd_locate_finish<NW, BITS>(idx, comm, &qs, max_occ, want != 0, occ, offs_dev, 0, values_dev, capacity, n_hits, &npass)));
  ctx->lookup_npass = npass;
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (sizing) return KMI_OK;
  if (*n_hits > capacity) return set_err(ctx, KMI_ERR_OVERFLOW, "locate: capacity too small");
  return KMI_OK;
}
static kmi_status index_locate_dist(kmi_index *idx, kmi_comm *comm, const uint64_t *q_dev, size_t nq, uint32_t max_occ, uint32_t *occ_dev,
                                    uint64_t *offs_dev, uint64_t *values_dev, size_t capacity, uint64_t *n_hits) {
  KMI_DISPATCH(idx->shape, locate_dist_impl, idx, comm, q_dev, nq, max_occ, occ_dev, offs_dev, values_dev, capacity, n_hits);
}

// ---- the reads forms
// the next record-aligned batch of a rank's share, staged on the device and 16-byte aligned (as index_profile_reads cuts and stages it)
static kmi_status qd_stage_batch(kmi_ctx *ctx, const uint8_t *bytes, size_t n_bytes, bool on_device, uint64_t start, uint64_t *end_out,
                                 const uint8_t **b_out, size_t *len_out) {
  uint64_t end = n_bytes;
  if (on_device) KMI_TRY(fastq_batch_end(ctx, bytes, n_bytes, start, ctx->profile_batch, &end));
  else end = fastq_batch_end_host(bytes, n_bytes, start, ctx->profile_batch);
  if (end <= start || end > n_bytes) end = n_bytes;
  const size_t len = (size_t)(end - start);
  const uint8_t *b = bytes + start;
  if (on_device) KMI_TRY(align_input(ctx, &b, len));
  else {
    void *din;
    KMI_TRY(ws_get(ctx, WS_INPUT, len + 64, &din));
    KMI_HIP(ctx, hipMemcpyAsync(din, b, len, hipMemcpyHostToDevice, ctx->stream));
    b = (const uint8_t *)din;
  }
  *end_out = end; *b_out = b; *len_out = len;
  return KMI_OK;
}

// the windows of a batch as (key words, window number) records in WS_LOOKUP_RECS, and the read descriptors of the scan
template <int NW>
static kmi_status qd_batch_records(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *b, size_t len, uint64_t **recs, uint64_t *nt, ReadScan *rs,
                                   uint64_t *n_rec) {
  constexpr int RW = NW + 1;
  uint64_t ns = 0;
  KMI_TRY(extract_count(ctx, cfg, b, len, nt, &ns));   // (malformed input is reported here, in the builds' words)
  void *p;
  KMI_TRY(ws_get(ctx, WS_LOOKUP_RECS, (*nt ? *nt : 1) * RW * sizeof(uint64_t) + 64, &p));
  *recs = (uint64_t *)p;
  KMI_TRY(extract_run(ctx, cfg, b, len, 0, *recs, nullptr, (size_t)*nt, false, true, nt, &ns, nullptr, (uint32_t)RW, EDGES_NONE, rs));
  *n_rec = (rs->n_lines + 3) / 4;   // every header line opens a record
  if (*nt) hipLaunchKernelGGL((lookup_tag_kernel<NW>), dim3(2048), dim3(256), 0, ctx->stream, *recs, *nt);
  KMI_HIP(ctx, hipGetLastError());
  return KMI_OK;
}

template <int NW, int BITS>
static kmi_status profile_dist_impl(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, bool on_device, uint32_t solid,
                                    kmi_read_profile *out, size_t capacity, uint64_t *n_reads) {
  kmi_ctx *ctx = idx->ctx;
  kmi_config cfg = idx->cfg;
  cfg.seq_filter = KMI_SEQ_ALL;   // (as profile_batch_impl)
  uint64_t start = 0, done = 0, npass = 0;
  ctx->qd_answered = 0;
  kmi_status carry = KMI_OK;   // what went wrong on this rank behind a round's last exchange: the next verdict tells the peers
  while (true) {
    uint64_t end = start, nt = 0, n_rec = 0, *recs = nullptr;
    const uint8_t *b = nullptr;
    size_t len = 0;
    ReadScan rs{};
    uint32_t *counts = nullptr;
    kmi_read_profile *rows = nullptr;
    QdState qs;
    const kmi_status mine = carry != KMI_OK ? carry : [&]() -> kmi_status {
      void *p;
      if (start < n_bytes) {
        KMI_TRY(qd_stage_batch(ctx, bytes, n_bytes, on_device, start, &end, &b, &len));
        KMI_TRY((qd_batch_records<NW>(ctx, &cfg, b, len, &recs, &nt, &rs, &n_rec)));
      }
      KMI_TRY(ws_get(ctx, WS_LOOKUP_CNT, (nt ? nt : 1) * sizeof(uint32_t), &p)); counts = (uint32_t *)p;
      KMI_TRY(ws_get(ctx, WS_OUTPUT, (n_rec ? n_rec : 1) * sizeof(kmi_read_profile), &p)); rows = (kmi_read_profile *)p;
      return qd_prep<NW, BITS>(idx, comm, recs, (size_t)nt, &qs);
    }();
    uint64_t more = start < n_bytes ? 1 : 0, want = 0;
    KMI_TRY(qd_agree(comm, mine, &more, &want));
    if (!more) break;   // every rank has run out
    KMI_TRY((qd_lookup_finish<NW, BITS>(idx, comm, &qs, counts, &npass)));
    carry = [&]() -> kmi_status {
      if (n_rec) {
        ProfScope ps(ctx, "read_profile_reduce", nt);
        constexpr uint64_t per_block = kProfThreads / kProfLanes;
        const uint64_t blocks = std::min<uint64_t>((n_rec + per_block - 1) / per_block, 8192);
        hipLaunchKernelGGL(read_profile_reduce_kernel, dim3((unsigned)blocks), dim3(kProfThreads), 0, ctx->stream, rs.reads, n_rec, rs.eolw,
                           rs.n_eol_words, (uint64_t)len, idx->shape.k, (const uint32_t *)counts, nt, solid, start, rows);
        KMI_HIP(ctx, hipGetLastError());
      }
      const uint64_t room = done < capacity ? capacity - done : 0, take = n_rec < room ? n_rec : room;   // nothing is written past capacity
      if (take) KMI_HIP(ctx, hipMemcpyAsync(out + done, rows, take * sizeof(kmi_read_profile), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
      KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the staging buffers are the next round's)
      return KMI_OK;
    }();
    done += n_rec;
    start = end;
  }
  ctx->lookup_npass = npass;
  *n_reads = done;
  if (done > capacity) return set_err(ctx, KMI_ERR_OVERFLOW, "profile_reads: capacity too small");
  return KMI_OK;
}
static kmi_status index_profile_reads_dist(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, bool on_device, uint32_t solid,
                                           kmi_read_profile *out, size_t capacity, uint64_t *n_reads) {
  KMI_DISPATCH(idx->shape, profile_dist_impl, idx, comm, bytes, n_bytes, on_device, solid, out, capacity, n_reads);
}

template <int NW, int BITS>
static kmi_status seed_dist_impl(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, bool on_device, uint32_t max_occ,
                                 kmi_read_seeds *rows, size_t cap_reads, uint32_t *occ, uint64_t *offsets, size_t cap_kmers, uint64_t *values,
                                 size_t cap_hits, uint64_t *n_reads, uint64_t *n_kmers, uint64_t *n_hits) {
  kmi_ctx *ctx = idx->ctx;
  const hipMemcpyKind back = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t vw = idx->val_words;
  kmi_config cfg = idx->cfg;
  cfg.seq_format = KMI_FMT_FASTQ; cfg.seq_filter = KMI_SEQ_ALL; cfg.index_kind = KMI_INDEX_COUNT;   // (as seed_batch_impl)
  uint64_t *values_dev = values;
  kmi_status carry = KMI_OK;
  if (values && !on_device && cap_hits) {   // the hits of all batches are gathered on the device and copied once
    void *p;
    carry = ws_get(ctx, WS_OUTPUT2, cap_hits * vw * sizeof(uint64_t), &p);
    values_dev = (uint64_t *)p;
  }
  uint64_t start = 0, reads_done = 0, kmers_done = 0, hits_done = 0, npass = 0;
  ctx->qd_answered = 0;
  while (true) {
    uint64_t end = start, nt = 0, n_rec = 0, *recs = nullptr;
    const uint8_t *b = nullptr;
    size_t len = 0;
    ReadScan rs{};
    SeedBatch sb{};
    QdState qs;
    const kmi_status mine = carry != KMI_OK ? carry : [&]() -> kmi_status {
      void *p;
      if (start < n_bytes) {
        KMI_TRY(qd_stage_batch(ctx, bytes, n_bytes, on_device, start, &end, &b, &len));
        KMI_TRY((qd_batch_records<NW>(ctx, &cfg, b, len, &recs, &nt, &rs, &n_rec)));
      }
      KMI_TRY(ws_get(ctx, WS_LOOKUP_CNT, (nt ? nt : 1) * sizeof(uint32_t), &p)); sb.occ = (uint32_t *)p;
      KMI_TRY(ws_get(ctx, WS_LOCATE_OFF, (nt + 1) * sizeof(uint64_t), &p)); sb.offs = (uint64_t *)p;
      KMI_TRY(ws_get(ctx, WS_OUTPUT, (n_rec ? n_rec : 1) * sizeof(kmi_read_seeds), &p)); sb.rows = (kmi_read_seeds *)p;
      sb.n_rec = n_rec; sb.n_kmers = nt;
      if (n_rec) {
        ProfScope ps(ctx, "read_seeds_len", n_rec);
        hipLaunchKernelGGL(read_seeds_len_kernel, dim3((unsigned)std::min<uint64_t>((n_rec + 255) / 256, 8192)), dim3(256), 0, ctx->stream, rs.reads,
                           n_rec, rs.eolw, rs.n_eol_words, (uint64_t)len, idx->shape.k, start, sb.rows);
        KMI_TRY(device_exclusive_scan(ctx, RowKmersIn{sb.rows}, RowFirstOut{sb.rows}, n_rec, kmers_done, (uint64_t *)nullptr, false));
      }
      return qd_prep<NW, BITS>(idx, comm, recs, (size_t)nt, &qs);
    }();
    uint64_t more = start < n_bytes ? 1 : 0, want = cap_hits ? 1 : 0;
    KMI_TRY(qd_agree(comm, mine, &more, &want));
    if (!more) break;   // every rank has run out
    KMI_TRY((qd_locate_finish<NW, BITS>(idx, comm, &qs, max_occ, want != 0, sb.occ, sb.offs, hits_done, cap_hits ? values_dev : nullptr, cap_hits,
                                        &sb.hits_end, &npass)));
    carry = [&]() -> kmi_status {
      if (n_rec) {
        ProfScope ps(ctx, "read_seeds_rows", nt);
        constexpr uint64_t per_block = kProfThreads / kProfLanes;
        const uint64_t blocks = std::min<uint64_t>((n_rec + per_block - 1) / per_block, 8192);
        hipLaunchKernelGGL(read_seeds_rows_kernel, dim3((unsigned)blocks), dim3(kProfThreads), 0, ctx->stream, sb.rows, n_rec, kmers_done,
                           (const uint32_t *)sb.occ, (const uint64_t *)sb.offs, nt, max_occ);
        KMI_HIP(ctx, hipGetLastError());
      }
      // nothing is written past a capacity
      const uint64_t room_r = reads_done < cap_reads ? cap_reads - reads_done : 0, take_r = n_rec < room_r ? n_rec : room_r;
      if (take_r) KMI_HIP(ctx, hipMemcpyAsync(rows + reads_done, sb.rows, take_r * sizeof(kmi_read_seeds), back, ctx->stream));
      const uint64_t room_k = kmers_done < cap_kmers ? cap_kmers - kmers_done : 0, take_k = nt < room_k ? nt : room_k;
      if (take_k) KMI_HIP(ctx, hipMemcpyAsync(occ + kmers_done, sb.occ, take_k * sizeof(uint32_t), back, ctx->stream));
      if (offsets && kmers_done <= cap_kmers)   // (the batch's last word is the next batch's first)
        KMI_HIP(ctx, hipMemcpyAsync(offsets + kmers_done, sb.offs, (take_k + (take_k == nt ? 1 : 0)) * sizeof(uint64_t), back, ctx->stream));
      KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the staging buffers are the next round's)
      return KMI_OK;
    }();
    reads_done += n_rec;
    kmers_done += nt;
    hits_done = sb.hits_end;
    start = end;
  }
  ctx->lookup_npass = npass;
  *n_reads = reads_done; *n_kmers = kmers_done; *n_hits = hits_done;
  if (n_bytes == 0 && offsets) {
    if (on_device) KMI_HIP(ctx, hipMemsetAsync(offsets, 0, sizeof(uint64_t), ctx->stream)); else offsets[0] = 0;
  }
  if (!rows && !occ && !offsets && !values && !cap_reads && !cap_kmers && !cap_hits) return KMI_OK;   // the sizing call
  if (reads_done > cap_reads || kmers_done > cap_kmers || hits_done > cap_hits)
    return set_err(ctx, KMI_ERR_OVERFLOW, "seed_reads: capacity too small");
  if (values && values_dev != values && hits_done)
    KMI_HIP(ctx, hipMemcpyAsync(values, values_dev, hits_done * vw * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KMI_OK;
}
static kmi_status index_seed_reads_dist(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, bool on_device, uint32_t max_occ,
                                        kmi_read_seeds *rows, size_t cap_reads, uint32_t *occ, uint64_t *offsets, size_t cap_kmers, uint64_t *values,
                                        size_t cap_hits, uint64_t *n_reads, uint64_t *n_kmers, uint64_t *n_hits) {
  KMI_DISPATCH(idx->shape, seed_dist_impl, idx, comm, bytes, n_bytes, on_device, max_occ, rows, cap_reads, occ, offsets, cap_kmers, values, cap_hits,
               n_reads, n_kmers, n_hits);
}

}  // namespace kmi
