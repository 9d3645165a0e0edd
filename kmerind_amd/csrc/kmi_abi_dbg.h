// kmi_abi_dbg.h -- the kmi_dbg_* entry points: create, build and insert on one rank and over ranks, find, export, unitigs.
//
// Included by kmi_index.hip after kmi_abi_dist_build.h (kmi_debruijn.h, kmi_unitig.h and kmi_unitig_dist.h hold what it calls; the
// host glue and the collectives' helpers are kmi_index.hip's own, fasta_range_partition is kmi_abi_dist_build.h's).
#pragma once

extern "C" {

// ---- de Bruijn graph nodes (kmi_debruijn.h)
kmi_status kmi_dbg_create(kmi_ctx *ctx, const kmi_config *cfg, uint32_t node_kind, kmi_dbg **out) {
  if (!ctx || !out) return KMI_ERR_INVALID;
  KShape shape;
  if (!valid_config(cfg, &shape)) return set_err(ctx, KMI_ERR_INVALID, "bad kmi_config");
  if (node_kind > KMI_DBG_EDGE_EXISTS) return set_err(ctx, KMI_ERR_INVALID, "unknown node kind");
  if (cfg->seq_filter != KMI_SEQ_ALL)
    return set_err(ctx, KMI_ERR_INVALID, "de Bruijn nodes are built from every record of the input (no sequence filter), as the reference's engine is");
  kmi_dbg *g = new kmi_dbg();
  g->ctx = ctx; g->cfg = *cfg; g->shape = shape; g->node_kind = node_kind;
  kmi_config c = *cfg;   // the node map proper: both strands of a k-mer are one node, kept under the smaller one
  c.index_kind = KMI_INDEX_COUNT; c.strand = KMI_STRAND_CANONICAL; c.dist_trans = KMI_DIST_MODEL;
  const kmi_status st = kmi_index_create(ctx, &c, &g->nodes);
  if (st != KMI_OK) { delete g; return st; }
  *out = g;
  return KMI_OK;
}

// the SeqParser template argument of the engine's build_posix / build_mmap (FASTQParser or FASTAParser)
kmi_status kmi_dbg_set_seq_format(kmi_dbg *g, uint32_t seq_format) {
  if (!g) return KMI_ERR_INVALID;
  if (seq_format > KMI_FMT_FASTA) return set_err(g->ctx, KMI_ERR_INVALID, "unknown sequence format");
  g->cfg.seq_format = seq_format;
  return KMI_OK;
}

kmi_status kmi_dbg_destroy(kmi_dbg *g) {
  if (!g) return KMI_OK;
  (void)hipSetDevice(g->ctx->device);
  (void)hipStreamSynchronize(g->ctx->stream);
  dbg_unitigs_drop(g);
  if (g->edges) pool_free(g->ctx, g->edges, g->edges_bytes);
  (void)kmi_index_destroy(g->nodes);
  delete g;
  return KMI_OK;
}

kmi_status kmi_dbg_clear(kmi_dbg *g) {
  if (!g) return KMI_ERR_INVALID;
  KMI_TRY(kmi_index_clear(g->nodes));
  dbg_unitigs_drop(g);
  if (g->edges) pool_free(g->ctx, g->edges, g->edges_bytes);
  g->edges = nullptr; g->edges_bytes = 0;
  g->dist_share = false;
  return KMI_OK;
}

kmi_status kmi_dbg_local_size(kmi_dbg *g, uint64_t *n) {
  if (!g || !n) return KMI_ERR_INVALID;
  *n = g->nodes->n_entries;
  return KMI_OK;
}

kmi_status kmi_dbg_parse_dev(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes_dev, size_t n_bytes, uint64_t *out_records_dev,
                             size_t out_capacity, uint64_t *n_tuples) {
  if (!ctx || !n_tuples) return KMI_ERR_INVALID;
  KShape shape;
  if (!valid_config(cfg, &shape)) return set_err(ctx, KMI_ERR_INVALID, "bad kmi_config");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  uint64_t *recs = nullptr;
  KMI_TRY(dbg_parse(ctx, cfg, bytes_dev, n_bytes, false, &recs, n_tuples));
  if (!out_records_dev) return KMI_OK;   // count only
  if (*n_tuples > out_capacity) return set_err(ctx, KMI_ERR_OVERFLOW, "parse: output capacity too small");
  if (*n_tuples) KMI_HIP(ctx, hipMemcpyAsync(out_records_dev, recs, (size_t)*n_tuples * (shape.n_words + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KMI_OK;
}

kmi_status kmi_dbg_build_dev(kmi_dbg *g, const uint8_t *bytes_dev, size_t n_bytes) {
  if (!g) return KMI_ERR_INVALID;
  kmi_ctx *ctx = g->ctx;
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  if (n_bytes == 0) return KMI_OK;
  dbg_unitigs_drop(g);
  {   // an empty graph from clean FASTQ reads: through super-k-mer records (dbg_build_superkmer); else, and for what that declines, tuples
    bool done = false;
    KMI_TRY(dbg_build_superkmer(g, bytes_dev, n_bytes, &done));
    if (done) return KMI_OK;
  }
  uint64_t *recs = nullptr, nt = 0;
  KMI_TRY(dbg_parse(ctx, &g->cfg, bytes_dev, n_bytes, true, &recs, &nt));
  return dbg_insert(g, recs, (size_t)nt);
}

kmi_status kmi_dbg_build_host(kmi_dbg *g, const uint8_t *bytes, size_t n_bytes) {
  if (!g) return KMI_ERR_INVALID;
  kmi_ctx *ctx = g->ctx;
  if (n_bytes == 0) return KMI_OK;
  if (!bytes) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  void *din;
  KMI_TRY(stage_host(ctx, WS_INPUT, bytes, n_bytes, 64, &din));
  return kmi_dbg_build_dev(g, (const uint8_t *)din, n_bytes);
}

// tuples as the parser emits them (any strand; value word = edge byte); they are rewritten in place into node form
static kmi_status dbg_insert_tuples(kmi_dbg *g, uint64_t *recs_dev, size_t n) {
  dbg_unitigs_drop(g);
  KMI_TRY(dbg_edges(g->ctx, recs_dev, n, nullptr, 0, g->shape, false, true));
  return dbg_insert(g, recs_dev, n);
}

static kmi_status dbg_insert_entry(kmi_dbg *g, const uint64_t *records, size_t n, bool on_device) {
  if (!g) return KMI_ERR_INVALID;
  kmi_ctx *ctx = g->ctx;
  if (!on_device) {
    if (n == 0) return KMI_OK;
    if (!records) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  }
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return KMI_OK;
  void *dr;   // (the caller's buffer stays as it is)
  const size_t bytes = n * (g->shape.n_words + 1) * sizeof(uint64_t);
  KMI_TRY(ws_get(ctx, WS_DBG_RECS, bytes + 64, &dr));
  KMI_HIP(ctx, hipMemcpyAsync(dr, records, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  return dbg_insert_tuples(g, (uint64_t *)dr, n);
}
kmi_status kmi_dbg_insert_dev(kmi_dbg *g, const uint64_t *records_dev, size_t n) { return dbg_insert_entry(g, records_dev, n, true); }
kmi_status kmi_dbg_insert_host(kmi_dbg *g, const uint64_t *records, size_t n) { return dbg_insert_entry(g, records, n, false); }

kmi_status kmi_dbg_find_dev(kmi_dbg *g, const uint64_t *queries_dev, size_t nq, uint64_t *out_keys_dev, uint64_t *out_values_dev, uint64_t *n_out) {
  if (!g || !n_out) return KMI_ERR_INVALID;
  KMI_HIP(g->ctx, hipSetDevice(g->ctx->device));
  return dbg_find(g, queries_dev, nq, out_keys_dev, out_values_dev, n_out);
}

kmi_status kmi_dbg_find_host(kmi_dbg *g, const uint64_t *queries, size_t nq, kmi_results *out) {
  if (!g || !out) return KMI_ERR_INVALID;
  kmi_ctx *ctx = g->ctx;
  memset(out, 0, sizeof(*out));
  if (nq == 0) return KMI_OK;
  if (!queries) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t nw = g->shape.n_words;
  void *dq, *dk, *dv;
  KMI_TRY(ws_get(ctx, WS_INPUT, nq * nw * sizeof(uint64_t), &dq));
  KMI_TRY(ws_get(ctx, WS_OUTPUT, nq * nw * sizeof(uint64_t), &dk));
  KMI_TRY(ws_get(ctx, WS_OUTPUT2, nq * kDbgValueWords * sizeof(uint64_t), &dv));
  KMI_HIP(ctx, hipMemcpyAsync(dq, queries, nq * nw * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  uint64_t n = 0;
  KMI_TRY(dbg_find(g, (const uint64_t *)dq, nq, (uint64_t *)dk, (uint64_t *)dv, &n));
  return results_to_host(ctx, out, dk, dv, n, nw * sizeof(uint64_t), kDbgValueWords * sizeof(uint64_t));
}

kmi_status kmi_dbg_count_host(kmi_dbg *g, const uint64_t *queries, size_t nq, kmi_results *out) {
  if (!g) return KMI_ERR_INVALID;
  return kmi_index_count_host(g->nodes, queries, nq, out);
}

kmi_status kmi_dbg_export_host(kmi_dbg *g, uint64_t *keys, uint32_t *counts9, size_t capacity, uint64_t *n) {
  if (!g || !n) return KMI_ERR_INVALID;
  kmi_ctx *ctx = g->ctx;
  *n = 0;
  const uint64_t ne = g->nodes->n_entries;
  if (ne == 0) return KMI_OK;
  if (capacity < ne) return set_err(ctx, KMI_ERR_OVERFLOW, "export: capacity too small");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  if (keys) KMI_HIP(ctx, hipMemcpyAsync(keys, g->nodes->keys, ne * g->shape.n_words * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (counts9) {
    std::vector<uint32_t> e(ne * 8), s(ne);
    KMI_HIP(ctx, hipMemcpyAsync(e.data(), g->edges, ne * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    KMI_HIP(ctx, hipMemcpyAsync(s.data(), g->nodes->vals, ne * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const bool ex = g->node_kind == KMI_DBG_EDGE_EXISTS;
    for (uint64_t i = 0; i < ne; ++i) {
      for (int t = 0; t < 8; ++t) counts9[i * 9 + t] = ex ? (e[i * 8 + t] ? 1u : 0u) : e[i * 8 + t];
      counts9[i * 9 + 8] = ex ? 0u : s[i];
    }
  }
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *n = ne;
  return KMI_OK;
}

// the tail of the builds over ranks: nt node-form tuples grouped by KeyToRank of the canonical k-mer, one all-to-all, and what
// arrives inserted (a rank without tuples still enters the exchange)
static kmi_status dbg_route_exchange_insert(kmi_dbg *g, kmi_comm *comm, const uint64_t *recs, uint64_t nt) {
  kmi_ctx *ctx = g->ctx;
  const int p = kmi::comm_size(comm);
  const uint32_t rw = g->shape.n_words + 1u;
  void *d_send, *d_recv;
  uint64_t total = 0;
  KMI_TRY(ws_get(ctx, WS_DIST_A, ((size_t)nt + 64) * rw * sizeof(uint64_t), &d_send));
  std::vector<uint64_t> sc(p, 0), rc;
  if (nt) KMI_TRY(kmi_route_tuples_dev(ctx, &g->nodes->cfg, recs, (size_t)nt, (uint32_t)p, 1, (uint64_t *)d_send, sc.data()));
  KMI_TRY(dist_exchange(comm, d_send, sc.data(), rw * sizeof(uint64_t), WS_DIST_B, &d_recv, rc, &total));
  dbg_unitigs_drop(g);
  if (p > 1) g->dist_share = true;
  return dbg_insert(g, (const uint64_t *)d_recv, (size_t)total);
}

// build over ranks: parse the rank's share, group the node-form tuples by KeyToRank of the canonical k-mer, one all-to-all
// (imxx::distribute inside de_bruijn_nodes_distributed::insert, de_bruijn_nodes_distributed.hpp:243-250), insert what arrives
kmi_status kmi_dbg_build_dist_host(kmi_dbg *g, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes) {
  if (!g) return KMI_ERR_INVALID;
  KMI_TRY(dist_check(g->nodes, comm));
  kmi_ctx *ctx = g->ctx;
  if (alone(ctx, comm)) return kmi_dbg_build_host(g, bytes, n_bytes);
  if (n_bytes && !bytes) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  void *d_bytes;
  KMI_TRY(stage_host(ctx, WS_INPUT, bytes, n_bytes, 64, &d_bytes));
  uint64_t *recs = nullptr, nt = 0;
  KMI_TRY(dbg_parse(ctx, &g->cfg, (const uint8_t *)d_bytes, n_bytes, true, &recs, &nt));   // (an empty share still enters the collectives)
  return dbg_route_exchange_insert(g, comm, recs, nt);
}

// find() of the node map over ranks: query keys to the ranks that own their canonical k-mer (the node map's KeyToRank), every
// source's keys answered on their own, one return exchange of (k-mer, node) -- distributed_unordered_map.hpp:564-687 as the
// node map inherits it (de_bruijn_nodes_distributed.hpp:61)
kmi_status kmi_dbg_find_dist_host(kmi_dbg *g, kmi_comm *comm, const uint64_t *queries, size_t nq, kmi_results *out) {
  if (!g || !out) return KMI_ERR_INVALID;
  KMI_TRY(dist_check(g->nodes, comm));
  kmi_ctx *ctx = g->ctx;
  const int p = kmi::comm_size(comm);
  if (alone(ctx, comm)) return kmi_dbg_find_host(g, queries, nq, out);
  memset(out, 0, sizeof(*out));
  if (nq && !queries) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  const uint32_t nw = g->shape.n_words;
  const size_t kb = nw * sizeof(uint64_t), vb = kDbgValueWords * sizeof(uint64_t);
  void *d_q;
  std::vector<uint64_t> rc;
  uint64_t total = 0;
  KMI_TRY(keys_to_owners(g->nodes, comm, queries, nq, false, &d_q, rc, &total));
  void *d_rk, *d_rv;
  KMI_TRY(ws_get(ctx, WS_DIST_C, (total + 8) * kb, &d_rk));
  KMI_TRY(ws_get(ctx, WS_DIST_D, (total + 8) * vb, &d_rv));
  std::vector<uint64_t> back(p, 0);
  uint64_t off = 0, pos = 0;
  for (int s = 0; s < p; ++s) {
    uint64_t n = 0;
    if (rc[s]) KMI_TRY(dbg_find(g, (const uint64_t *)d_q + off * nw, (size_t)rc[s], (uint64_t *)d_rk + pos * nw, (uint64_t *)d_rv + pos * kDbgValueWords, &n));
    back[s] = n; off += rc[s]; pos += n;
  }
  return answers_to_askers(comm, d_rk, d_rv, back, kb, vb, out);
}

// build_posix / build_mmap(filename) of the engine with comm.size() > 1: the rank passes the bytes it read of the FASTQ file (its
// nominal range + look-ahead), the partition is cut at record starts on the device (kmi_index_build_range_dist_host's rule)
kmi_status kmi_dbg_build_range_dist_host(kmi_dbg *g, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint64_t buffer_offset,
                                         uint64_t nominal_bytes, int reaches_eof, int *need_more) {
  if (!g || !need_more) return KMI_ERR_INVALID;
  KMI_TRY(dist_check(g->nodes, comm));
  kmi_ctx *ctx = g->ctx;
  *need_more = 0;
  if (n_bytes && !bytes) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  void *d_bytes;   // (only the cut is made from this copy: the build stages the host bytes of the cut range itself)
  uint64_t cut[2] = {0, 0};
  if (n_bytes) KMI_TRY(fastq_range_cut(ctx, WS_INPUT2, bytes, n_bytes, buffer_offset, nominal_bytes, reaches_eof, &d_bytes, cut, need_more));
  if (*need_more) return KMI_OK;
  return kmi_dbg_build_dist_host(g, comm, bytes + cut[0], (size_t)(cut[1] - cut[0]));
}

// build over ranks from a FASTA file by BYTE RANGE (the engine's build_posix / build_mmap<FASTAParser> with comm.size() > 1): the
// bookkeeping of kmi_index_build_fasta_range_dist_host, where the block's windows need k sequence characters behind it (the last
// window's right neighbour) and its first window's left neighbour comes from the blocks before it (the left carries, in the same
// gather); then the node-form tuples of the block are routed, exchanged once and inserted as kmi_dbg_build_dist_host does
kmi_status kmi_dbg_build_fasta_range_dist_host(kmi_dbg *g, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint64_t buffer_offset,
                                               uint64_t nominal_bytes, int reaches_eof, int prev_byte, int *need_more) {
  if (!g || !need_more) return KMI_ERR_INVALID;
  KMI_TRY(dist_check(g->nodes, comm));
  kmi_ctx *ctx = g->ctx;
  *need_more = 0;
  if (g->cfg.seq_format != KMI_FMT_FASTA) return set_err(ctx, KMI_ERR_INVALID, "not a FASTA graph (kmi_dbg_set_seq_format)");
  if ((n_bytes && !bytes) || nominal_bytes > n_bytes) return set_err(ctx, KMI_ERR_INVALID, "bad buffer");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  void *d_bytes;
  KMI_TRY(stage_host(ctx, WS_INPUT, bytes, n_bytes, 64, &d_bytes));
  kmi_fasta_partition part; uint64_t end = 0; int carry = -1;
  KMI_TRY(fasta_range_partition(ctx, comm, g->shape.k, bytes, (const uint8_t *)d_bytes, n_bytes, buffer_offset, nominal_bytes, reaches_eof,
                                prev_byte, need_more, &part, &end, &carry));
  if (*need_more) return KMI_OK;
  uint64_t *recs = nullptr, nt = 0;
  KMI_TRY(kmi_ctx_set_fasta_partition(ctx, &part));
  ctx->fa_left_carry = carry;
  const kmi_status stp = dbg_parse(ctx, &g->cfg, (const uint8_t *)d_bytes, (size_t)end, true, &recs, &nt);
  ctx->fa_left_carry = -1;
  (void)kmi_ctx_set_fasta_partition(ctx, nullptr);
  KMI_TRY(stp);
  dbg_unitigs_drop(g);
  if (alone(ctx, comm)) return dbg_insert(g, recs, (size_t)nt);   // (one rank: every node is its own)
  return dbg_route_exchange_insert(g, comm, recs, nt);
}

// erase(): the nodes of the query keys (either strand) leave the map
kmi_status kmi_dbg_erase_host(kmi_dbg *g, const uint64_t *queries, size_t nq, uint64_t *n_erased) {
  if (!g) return KMI_ERR_INVALID;
  kmi_ctx *ctx = g->ctx;
  if (n_erased) *n_erased = 0;
  if (nq == 0) return KMI_OK;
  if (!queries) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  void *dq;
  const size_t kb = g->shape.n_words * sizeof(uint64_t);
  KMI_TRY(stage_host(ctx, WS_INPUT, queries, nq * kb, 8 * kb, &dq));
  dbg_unitigs_drop(g);
  return dbg_erase(g, (const uint64_t *)dq, nq, n_erased);
}

// ... over ranks: the keys travel to the ranks that own them (*n_erased_local = nodes that left THIS rank's part)
kmi_status kmi_dbg_erase_dist_host(kmi_dbg *g, kmi_comm *comm, const uint64_t *queries, size_t nq, uint64_t *n_erased_local) {
  if (!g) return KMI_ERR_INVALID;
  KMI_TRY(dist_check(g->nodes, comm));
  kmi_ctx *ctx = g->ctx;
  if (alone(ctx, comm)) return kmi_dbg_erase_host(g, queries, nq, n_erased_local);
  if (n_erased_local) *n_erased_local = 0;
  if (nq && !queries) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  void *d_q;
  std::vector<uint64_t> rc;
  uint64_t total = 0;
  KMI_TRY(keys_to_owners(g->nodes, comm, queries, nq, false, &d_q, rc, &total));
  dbg_unitigs_drop(g);
  return dbg_erase(g, (const uint64_t *)d_q, (size_t)total, n_erased_local);
}

// count() over ranks: the node map's keys live in a count index, whose collective answers 1 per node held
kmi_status kmi_dbg_count_dist_host(kmi_dbg *g, kmi_comm *comm, const uint64_t *queries, size_t nq, kmi_results *out) {
  if (!g) return KMI_ERR_INVALID;
  return kmi_index_count_dist_host(g->nodes, comm, queries, nq, out);
}

kmi_status kmi_dbg_size_dist(kmi_dbg *g, kmi_comm *comm, uint64_t *n) {
  if (!g) return KMI_ERR_INVALID;
  return kmi_index_size_dist(g->nodes, comm, n);
}

// unitigs (kmi_unitig.h): compaction on the device, the result kept in the graph until it changes
kmi_status kmi_dbg_compact(kmi_dbg *g, uint32_t min_edge_count, uint64_t *n_unitigs, uint64_t *n_bases) {
  if (!g) return KMI_ERR_INVALID;
  kmi_ctx *ctx = g->ctx;
  if (n_unitigs) *n_unitigs = 0;
  if (n_bases) *n_bases = 0;
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  KMI_TRY(dbg_compact(g, min_edge_count));
  if (n_unitigs) *n_unitigs = g->n_unitigs;
  if (n_bases) *n_bases = g->n_unitig_bases;
  return KMI_OK;
}

// ... of the union of the ranks' node maps (kmi_unitig_dist.h): collective
kmi_status kmi_dbg_compact_dist_host(kmi_dbg *g, kmi_comm *comm, uint32_t min_edge_count, uint64_t *n_unitigs_local, uint64_t *n_bases_local,
                                     uint64_t *n_unitigs_total, uint64_t *n_bases_total) {
  if (!g) return KMI_ERR_INVALID;
  if (n_unitigs_local) *n_unitigs_local = 0;
  if (n_bases_local) *n_bases_local = 0;
  if (n_unitigs_total) *n_unitigs_total = 0;
  if (n_bases_total) *n_bases_total = 0;
  KMI_TRY(dist_check(g->nodes, comm));
  kmi_ctx *ctx = g->ctx;
  uint64_t totals[2] = {0, 0};
  if (alone(ctx, comm)) {
    KMI_TRY(dbg_compact(g, min_edge_count));
    totals[0] = g->n_unitigs; totals[1] = g->n_unitig_bases;
  } else KMI_TRY(kmi::dbg_compact_dist(g, comm, min_edge_count, totals));
  if (n_unitigs_local) *n_unitigs_local = g->n_unitigs;
  if (n_bases_local) *n_bases_local = g->n_unitig_bases;
  if (n_unitigs_total) *n_unitigs_total = totals[0];
  if (n_bases_total) *n_bases_total = totals[1];
  return KMI_OK;
}

kmi_status kmi_dbg_unitigs_export_host(kmi_dbg *g, uint64_t *offsets, char *bases, uint64_t *occurrences, uint8_t *circular,
                                       size_t capacity_unitigs, size_t capacity_bases) {
  if (!g) return KMI_ERR_INVALID;
  kmi_ctx *ctx = g->ctx;
  if (!g->uni_valid) return set_err(ctx, KMI_ERR_INVALID, "no unitigs: kmi_dbg_compact has not run since the map last changed");
  const uint64_t nu = g->n_unitigs, nb = g->n_unitig_bases;
  if ((offsets || occurrences || circular) && capacity_unitigs < nu) return set_err(ctx, KMI_ERR_OVERFLOW, "unitigs export: capacity_unitigs too small");
  if (bases && capacity_bases < nb) return set_err(ctx, KMI_ERR_OVERFLOW, "unitigs export: capacity_bases too small");
  if (nu == 0) {
    if (offsets) offsets[0] = 0;
    return KMI_OK;
  }
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t *u_off = (const uint64_t *)g->uni_buf, *u_occ = u_off + nu + 1u;
  const uint8_t *u_circ = (const uint8_t *)(u_occ + nu);
  const char *u_bases = (const char *)(u_circ + (((size_t)nu + 15u) & ~(size_t)15u));
  if (offsets) KMI_HIP(ctx, hipMemcpyAsync(offsets, u_off, (size_t)(nu + 1u) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (occurrences) KMI_HIP(ctx, hipMemcpyAsync(occurrences, u_occ, (size_t)nu * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (circular) KMI_HIP(ctx, hipMemcpyAsync(circular, u_circ, (size_t)nu, hipMemcpyDeviceToHost, ctx->stream));
  if (bases && nb) KMI_HIP(ctx, hipMemcpyAsync(bases, u_bases, (size_t)nb, hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KMI_OK;
}

}  // extern "C"
