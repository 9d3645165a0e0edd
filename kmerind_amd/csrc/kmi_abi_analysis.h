// kmi_abi_analysis.h -- spectrum and retain, the de Bruijn node map's cleaning, compare / combine of two count indexes.
//
// Included by kmi_index.hip last (kmi_spectrum.h, kmi_dbg_clean.h, kmi_dbg_tips.h, kmi_dbg_tips_dist.h, kmi_dbg_bubbles.h, kmi_dbg_bubbles_dist.h and kmi_setops.h hold what it
// calls; alone, dist_check and dist_agree are kmi_index.hip's own).
#pragma once

extern "C" {

// ---- count spectrum and count filter (kmi_spectrum.h)
static kmi_status spectrum_entry(kmi_index *idx, uint32_t n_bins, uint64_t *hist, bool on_device, kmi_spectrum_totals *totals) {
  if (!idx) return KMI_ERR_INVALID;
  kmi_ctx *ctx = idx->ctx;
  if (idx->val_words) return set_err(ctx, KMI_ERR_INVALID, "spectrum() is a member of the count index");
  if (n_bins < 2 || n_bins > (uint32_t)KMI_SPECTRUM_MAX_BINS) return set_err(ctx, KMI_ERR_INVALID, "n_bins is 2 .. KMI_SPECTRUM_MAX_BINS");
  if (!hist) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  uint64_t *d_hist = hist;
  if (!on_device) {
    void *p;
    KMI_TRY(ws_get(ctx, WS_OUTPUT, n_bins * sizeof(uint64_t), &p));
    d_hist = (uint64_t *)p;
  }
  KMI_TRY(spectrum_run(idx, n_bins, d_hist));
  if (!on_device) KMI_HIP(ctx, hipMemcpyAsync(hist, d_hist, n_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (totals) KMI_TRY(spectrum_totals(idx, totals));
  else if (!on_device) KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KMI_OK;
}
kmi_status kmi_index_spectrum_dev(kmi_index *idx, uint32_t n_bins, uint64_t *hist_dev, kmi_spectrum_totals *totals) {
  return spectrum_entry(idx, n_bins, hist_dev, true, totals);
}
kmi_status kmi_index_spectrum_host(kmi_index *idx, uint32_t n_bins, uint64_t *hist, kmi_spectrum_totals *totals) {
  return spectrum_entry(idx, n_bins, hist, false, totals);
}

kmi_status kmi_index_spectrum_dist_host(kmi_index *idx, kmi_comm *comm, uint32_t n_bins, uint64_t *hist, kmi_spectrum_totals *totals) {
  KMI_TRY(dist_check(idx, comm));
  kmi_ctx *ctx = idx->ctx;
  // (argument errors are every rank's alike: nothing collective has started)
  if (idx->val_words) return set_err(ctx, KMI_ERR_INVALID, "spectrum() is a member of the count index");
  if (n_bins < 2 || n_bins > (uint32_t)KMI_SPECTRUM_MAX_BINS) return set_err(ctx, KMI_ERR_INVALID, "n_bins is 2 .. KMI_SPECTRUM_MAX_BINS");
  if (!hist) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  // the bins, then n_entries and sum_counts: one sum over the ranks; the largest count and ~(the smallest): one maximum
  std::vector<uint64_t> words((size_t)n_bins + 2, 0);
  kmi_spectrum_totals t{};
  const kmi_status mine = spectrum_entry(idx, n_bins, words.data(), false, &t);
  KMI_TRY(dist_agree(comm, mine));   // a rank whose pass failed does not leave the others in the all-reduce
  words[n_bins] = t.n_entries; words[(size_t)n_bins + 1] = t.sum_counts;
  uint64_t ext[2] = {t.max_count, t.n_entries ? (uint64_t)(uint32_t)~t.min_count : 0ull};   // (a rank without entries has no say in either)
  KMI_TRY(kmi::comm_allreduce_sum(comm, words.data(), words.size()));
  KMI_TRY(kmi::comm_allreduce(comm, ext, 2, 1));
  memcpy(hist, words.data(), sizeof(uint64_t) * n_bins);
  if (totals) {
    totals->n_entries = words[n_bins]; totals->sum_counts = words[(size_t)n_bins + 1];
    totals->max_count = (uint32_t)ext[0];
    totals->min_count = totals->n_entries ? ~(uint32_t)ext[1] : 0u;
  }
  return KMI_OK;
}

kmi_status kmi_index_retain_counts(kmi_index *idx, uint32_t lo, uint32_t hi, uint64_t *n_erased) {
  if (!idx) return KMI_ERR_INVALID;
  kmi_ctx *ctx = idx->ctx;
  if (n_erased) *n_erased = 0;
  if (idx->val_words) return set_err(ctx, KMI_ERR_INVALID, "retain_counts() is a member of the count index");
  if (lo > hi) return set_err(ctx, KMI_ERR_INVALID, "retain_counts: lo > hi");
  ctx->retain_fullest = 0;
  if (!idx->has_data || idx->n_entries == 0) return KMI_OK;
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  return index_retain_counts(idx, lo, hi, n_erased);
}

// ---- cleaning a de Bruijn node map (kmi_dbg_clean.h)
// the node index is a count index whose values are the occurrences: its own spectrum entry points do the work
static kmi_status dbg_has_occurrences(kmi_dbg *g) {
  if (g->node_kind == KMI_DBG_EDGE_EXISTS) return set_err(g->ctx, KMI_ERR_INVALID, "spectrum: an EDGE_EXISTS map keeps no occurrence count");
  return KMI_OK;
}
kmi_status kmi_dbg_spectrum_host(kmi_dbg *g, uint32_t n_bins, uint64_t *hist, kmi_spectrum_totals *totals) {
  if (!g) return KMI_ERR_INVALID;
  KMI_TRY(dbg_has_occurrences(g));
  return kmi_index_spectrum_host(g->nodes, n_bins, hist, totals);
}

kmi_status kmi_dbg_spectrum_dist_host(kmi_dbg *g, kmi_comm *comm, uint32_t n_bins, uint64_t *hist, kmi_spectrum_totals *totals) {
  if (!g) return KMI_ERR_INVALID;
  KMI_TRY(dist_check(g->nodes, comm));
  KMI_TRY(dbg_has_occurrences(g));   // (every rank's alike: nothing collective has started)
  return kmi_index_spectrum_dist_host(g->nodes, comm, n_bins, hist, totals);
}

kmi_status kmi_dbg_retain_counts(kmi_dbg *g, uint32_t lo, uint32_t hi, uint64_t *n_erased) {
  if (!g) return KMI_ERR_INVALID;
  return kmi::dbg_retain_counts(g, lo, hi, n_erased);
}

kmi_status kmi_dbg_prune_edges(kmi_dbg *g, uint32_t min_edge_count, kmi_dbg_prune_stats *stats) {
  if (!g) return KMI_ERR_INVALID;
  uint64_t s[8];
  const kmi_status st = kmi::dbg_prune(g, min_edge_count, s);
  if (stats) memcpy(stats, s, sizeof(s));
  return st;
}

kmi_status kmi_dbg_prune_edges_dist_host(kmi_dbg *g, kmi_comm *comm, uint32_t min_edge_count, kmi_dbg_prune_stats *stats_local,
                                         kmi_dbg_prune_stats *stats_total) {
  if (!g) return KMI_ERR_INVALID;
  if (stats_local) memset(stats_local, 0, sizeof(*stats_local));
  if (stats_total) memset(stats_total, 0, sizeof(*stats_total));
  KMI_TRY(dist_check(g->nodes, comm));
  uint64_t sl[8], stt[8];
  kmi_status st;
  if (alone(g->ctx, comm)) {
    st = kmi::dbg_prune(g, min_edge_count, sl);
    memcpy(stt, sl, sizeof(sl));
  } else st = kmi::dbg_prune_dist(g, comm, min_edge_count, sl, stt);
  if (stats_local) memcpy(stats_local, sl, sizeof(sl));
  if (stats_total) memcpy(stats_total, stt, sizeof(stt));
  return st;
}

kmi_status kmi_dbg_clip_tips(kmi_dbg *g, uint32_t min_edge_count, uint32_t max_tip_nodes, uint32_t flags, kmi_dbg_clip_stats *stats) {
  if (!g) return KMI_ERR_INVALID;
  static_assert(sizeof(kmi_dbg_clip_stats) == 8 * sizeof(uint64_t), "eight words");
  uint64_t s[8];
  const kmi_status st = kmi::dbg_clip_tips(g, min_edge_count, max_tip_nodes, flags, s);
  if (stats) memcpy(stats, s, sizeof(s));
  return st;
}

kmi_status kmi_dbg_clip_tips_dist_host(kmi_dbg *g, kmi_comm *comm, uint32_t min_edge_count, uint32_t max_tip_nodes, uint32_t flags,
                                       kmi_dbg_clip_stats *stats_local, kmi_dbg_clip_stats *stats_total) {
  if (!g) return KMI_ERR_INVALID;
  if (stats_local) memset(stats_local, 0, sizeof(*stats_local));
  if (stats_total) memset(stats_total, 0, sizeof(*stats_total));
  KMI_TRY(dist_check(g->nodes, comm));
  uint64_t sl[8], stt[8];
  kmi_status st;
  if (alone(g->ctx, comm)) {
    st = kmi::dbg_clip_tips(g, min_edge_count, max_tip_nodes, flags, sl);
    memcpy(stt, sl, sizeof(sl));
  } else st = kmi::dbg_clip_tips_dist(g, comm, min_edge_count, max_tip_nodes, flags, sl, stt);
  if (stats_local) memcpy(stats_local, sl, sizeof(sl));
  if (stats_total) memcpy(stats_total, stt, sizeof(stt));
  return st;
}

kmi_status kmi_dbg_pop_bubbles(kmi_dbg *g, uint32_t min_edge_count, uint32_t max_bubble_nodes, uint32_t flags, kmi_dbg_pop_stats *stats) {
  if (!g) return KMI_ERR_INVALID;
  static_assert(sizeof(kmi_dbg_pop_stats) == 8 * sizeof(uint64_t), "eight words");
  uint64_t s[8];
  const kmi_status st = kmi::dbg_pop_bubbles(g, min_edge_count, max_bubble_nodes, flags, s);
  if (stats) memcpy(stats, s, sizeof(s));
  return st;
}

kmi_status kmi_dbg_pop_bubbles_dist_host(kmi_dbg *g, kmi_comm *comm, uint32_t min_edge_count, uint32_t max_bubble_nodes, uint32_t flags,
                                         kmi_dbg_pop_stats *stats_local, kmi_dbg_pop_stats *stats_total) {
  if (!g) return KMI_ERR_INVALID;
  if (stats_local) memset(stats_local, 0, sizeof(*stats_local));
  if (stats_total) memset(stats_total, 0, sizeof(*stats_total));
  KMI_TRY(dist_check(g->nodes, comm));
  uint64_t sl[8], stt[8];
  kmi_status st;
  if (alone(g->ctx, comm)) {
    st = kmi::dbg_pop_bubbles(g, min_edge_count, max_bubble_nodes, flags, sl);
    memcpy(stt, sl, sizeof(sl));
  } else st = kmi::dbg_pop_bubbles_dist(g, comm, min_edge_count, max_bubble_nodes, flags, sl, stt);
  if (stats_local) memcpy(stats_local, sl, sizeof(sl));
  if (stats_total) memcpy(stats_total, stt, sizeof(stt));
  return st;
}

// ---- two count indexes compared and combined (kmi_setops.h)
kmi_status kmi_index_compare(kmi_index *a, kmi_index *b, kmi_index_overlap *out) {
  if (!a || !b || !out) return KMI_ERR_INVALID;
  kmi_ctx *ctx = a->ctx;
  memset(out, 0, sizeof(*out));
  KMI_TRY(setops_check(a, b, "compare"));
  ctx->setops_npass = 0;
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  const kmi_status st = index_compare(a, b, out);
  if (st != KMI_OK) memset(out, 0, sizeof(*out));
  return st;
}

kmi_status kmi_index_compare_dist_host(kmi_index *a, kmi_index *b, kmi_comm *comm, kmi_index_overlap *out) {
  KMI_TRY(dist_check(a, comm));
  // (argument errors are every rank's alike: nothing collective has started)
  if (!b || !out) return KMI_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  KMI_TRY(setops_check(a, b, "compare"));
  kmi_index_overlap mine_words{};
  const kmi_status mine = kmi_index_compare(a, b, &mine_words);
  KMI_TRY(dist_agree(comm, mine));   // a rank whose join failed does not leave the others in the all-reduce
  static_assert(sizeof(kmi_index_overlap) == 8 * sizeof(uint64_t), "eight words");
  uint64_t words[8];
  memcpy(words, &mine_words, sizeof(words));
  KMI_TRY(kmi::comm_allreduce_sum(comm, words, 8));
  memcpy(out, words, sizeof(words));
  return KMI_OK;
}

kmi_status kmi_index_combine(kmi_index *a, kmi_index *b, uint32_t op, uint64_t *n_entries) {
  if (!a || !b) return KMI_ERR_INVALID;
  kmi_ctx *ctx = a->ctx;
  if (n_entries) *n_entries = a->has_data ? a->n_entries : 0;
  KMI_TRY(setops_check(a, b, "combine"));
  if (op > (uint32_t)KMI_COMBINE_SUBTRACT_COUNTS) return set_err(ctx, KMI_ERR_INVALID, "combine: unknown op");
  if (a == b) return set_err(ctx, KMI_ERR_INVALID, "combine: a and b are the same index");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  const kmi_status st = index_combine(a, b, op);
  if (n_entries) *n_entries = a->has_data ? a->n_entries : 0;
  return st;
}

}  // extern "C"
