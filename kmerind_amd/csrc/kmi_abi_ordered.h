// kmi_abi_ordered.h -- super-k-mer produce / consume, owner ranks, update of pairs, and the queries in the caller's order:
// lookup, profile, locate and seed, on one rank and over ranks.
//
// Included by kmi_index.hip after kmi_abi_dbg.h (kmi_sk_build.h, kmi_update.h, kmi_lookup.h, kmi_locate.h and kmi_query_dist.h
// hold what it calls; alone and dist_check are kmi_index.hip's own).
#pragma once

extern "C" {

// ---- builds over ranks through exchanged super-k-mer records
kmi_status kmi_index_sk_produce_dev(kmi_index *idx, const uint8_t *bytes_dev, size_t n_bytes, uint32_t nranks, uint64_t *out_records_dev,
                                    size_t out_capacity, const uint64_t **records_dev, uint64_t *n_records, uint64_t *send_counts_host, int *produced) {
  if (!idx || !records_dev || !n_records || !send_counts_host || !produced) return KMI_ERR_INVALID;
  kmi_ctx *ctx = idx->ctx;
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  *produced = 0; *records_dev = nullptr; *n_records = 0;
  const uint32_t w = sk_width_of(idx);
  if (!w || !sk_rank_count(nranks)) return KMI_OK;   // not a case of this path: the caller routes k-mers
  if (ctx->sk_dbg == 7) return KMI_OK;   // (test knob: as if the input had exceeded a capacity of the front end)
  if (n_bytes) KMI_TRY(align_input(ctx, &bytes_dev, n_bytes));
  if (!out_records_dev) out_capacity = 0;
  return sk_produce(idx, w, bytes_dev, n_bytes, nranks, records_dev, n_records, send_counts_host, produced, out_records_dev, out_capacity);
}

kmi_status kmi_index_sk_consume_dev(kmi_index *idx, const uint64_t *records_dev, size_t n_records, uint32_t nranks) {
  if (!idx) return KMI_ERR_INVALID;
  kmi_ctx *ctx = idx->ctx;
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t w = sk_width_of(idx);
  if (!w || !sk_rank_count(nranks)) return set_err(ctx, KMI_ERR_INVALID, "no super-k-mer build for this index / rank count");
  if (n_records && !records_dev) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  return sk_consume(idx, w, records_dev, n_records, nranks);
}

kmi_status kmi_index_set_owner_ranks(kmi_index *idx, uint32_t nranks) {
  if (!idx) return KMI_ERR_INVALID;
  if (nranks == 0 || nranks > 8 || (nranks & (nranks - 1u))) return set_err(idx->ctx, KMI_ERR_INVALID, "owner ranks: 1, 2, 4 or 8");
  if (idx->has_data && idx->n_entries && (1u << idx->owner_lp) != nranks)
    return set_err(idx->ctx, KMI_ERR_INVALID, "the index holds entries distributed another way");
  idx->owner_lp = 31u - (uint32_t)__builtin_clz(nranks);
  return KMI_OK;
}

kmi_status kmi_index_set_saturating(kmi_index *idx, int on) {
  if (!idx) return KMI_ERR_INVALID;
  if (idx->val_words) return set_err(idx->ctx, KMI_ERR_INVALID, "saturating counts belong to the counting maps");
  idx->saturating = on != 0;
  return KMI_OK;
}

kmi_status kmi_index_sk_width(kmi_index *idx, uint32_t *w) {
  if (!idx || !w) return KMI_ERR_INVALID;
  *w = kmi::sk_width_of(idx);
  return KMI_OK;
}

kmi_status kmi_index_owner_ranks(kmi_index *idx, uint32_t *nranks) {
  if (!idx || !nranks) return KMI_ERR_INVALID;
  *nranks = 1u << idx->owner_lp;
  return KMI_OK;
}

kmi_status kmi_route_owner_dev(kmi_ctx *ctx, const kmi_config *cfg, const uint64_t *keys_dev, size_t n, uint32_t nranks, uint64_t *out_keys_dev,
                               uint64_t *send_counts_host) {
  if (!ctx) return KMI_ERR_INVALID;
  KShape shape;
  if (!valid_config(cfg, &shape)) return set_err(ctx, KMI_ERR_INVALID, "bad kmi_config");
  // (the shape alone, not KMI_FUSED_PATH: an index that is distributed by minimizer owner takes k-mers whatever path built it)
  if (sk_width_of_shape(shape) == 0 || nranks < 2 || nranks > 8 || (nranks & (nranks - 1u)) || !send_counts_host)
    return set_err(ctx, KMI_ERR_INVALID, "owner routing is for one-word DNA k-mers over 2, 4 or 8 ranks");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  for (uint32_t r = 0; r < nranks; ++r) send_counts_host[r] = 0;
  if (n == 0) return KMI_OK;
  return route_owner(ctx, cfg, shape, keys_dev, n, nranks, out_keys_dev, send_counts_host);
}

// ---- update() with a device-side updater (kmi_update.h)
static kmi_status update_pairs_entry(kmi_index *idx, const uint64_t *records, size_t n, bool on_device, uint32_t op, uint64_t *n_updated) {
  if (!idx || !n_updated) return KMI_ERR_INVALID;
  kmi_ctx *ctx = idx->ctx;
  *n_updated = 0;
  if (idx->val_words) return set_err(ctx, KMI_ERR_INVALID, "update() is a member of the counting maps");
  if (op > KMI_UPDATE_ASSIGN) return set_err(ctx, KMI_ERR_INVALID, "unknown updater");
  if (!on_device) {
    if (n == 0) return KMI_OK;
    if (!records) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  }
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return KMI_OK;
  void *dr;   // (the caller's buffer stays as it is)
  const size_t bytes = n * (idx->shape.n_words + 1) * sizeof(uint64_t);
  KMI_TRY(ws_get(ctx, WS_INPUT2, bytes + 64, &dr));
  KMI_HIP(ctx, hipMemcpyAsync(dr, records, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  return index_update_pairs(idx, (uint64_t *)dr, n, (int)op, n_updated);
}
kmi_status kmi_index_update_pairs_dev(kmi_index *idx, const uint64_t *records_dev, size_t n, uint32_t op, uint64_t *n_updated) {
  return update_pairs_entry(idx, records_dev, n, true, op, n_updated);
}
kmi_status kmi_index_update_pairs_host(kmi_index *idx, const uint64_t *records, size_t n, uint32_t op, uint64_t *n_updated) {
  return update_pairs_entry(idx, records, n, false, op, n_updated);
}

// ---- queries in the caller's order (kmi_lookup.h)
static kmi_status lookup_entry(kmi_index *idx, const uint64_t *queries, size_t nq, uint32_t *counts, bool on_device) {
  if (!idx) return KMI_ERR_INVALID;
  kmi_ctx *ctx = idx->ctx;
  if (idx->val_words) return set_err(ctx, KMI_ERR_INVALID, "lookup() is a member of the count index");
  if (nq == 0) return KMI_OK;
  if (!queries || !counts) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  if (on_device) return index_lookup(idx, queries, nq, counts);
  void *dq, *dc;
  KMI_TRY(ws_get(ctx, WS_INPUT, nq * idx->shape.n_words * sizeof(uint64_t), &dq));
  KMI_TRY(ws_get(ctx, WS_OUTPUT, nq * sizeof(uint32_t), &dc));
  KMI_HIP(ctx, hipMemcpyAsync(dq, queries, nq * idx->shape.n_words * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  KMI_TRY(index_lookup(idx, (const uint64_t *)dq, nq, (uint32_t *)dc));
  KMI_HIP(ctx, hipMemcpyAsync(counts, dc, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KMI_OK;
}
kmi_status kmi_index_lookup_dev(kmi_index *idx, const uint64_t *queries_dev, size_t nq, uint32_t *counts_dev) {
  return lookup_entry(idx, queries_dev, nq, counts_dev, true);
}
kmi_status kmi_index_lookup_host(kmi_index *idx, const uint64_t *queries, size_t nq, uint32_t *counts) {
  return lookup_entry(idx, queries, nq, counts, false);
}

static kmi_status profile_reads_entry(kmi_index *idx, const uint8_t *bytes, size_t n_bytes, bool on_device, uint32_t solid_threshold,
                                      kmi_read_profile *out, size_t capacity, uint64_t *n_reads) {
  if (!idx || !n_reads) return KMI_ERR_INVALID;
  kmi_ctx *ctx = idx->ctx;
  *n_reads = 0;
  if (idx->val_words) return set_err(ctx, KMI_ERR_INVALID, "profile_reads() is a member of the count index");
  if (idx->cfg.seq_format != KMI_FMT_FASTQ) return set_err(ctx, KMI_ERR_INVALID, "profile_reads() reads FASTQ");
  if (solid_threshold == 0) return set_err(ctx, KMI_ERR_INVALID, "solid_threshold is at least 1");
  if (n_bytes == 0) return KMI_OK;
  if (!bytes || (!out && capacity)) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  return index_profile_reads(idx, bytes, n_bytes, on_device, solid_threshold, out, capacity, n_reads);
}
kmi_status kmi_index_profile_reads_dev(kmi_index *idx, const uint8_t *bytes_dev, size_t n_bytes, uint32_t solid_threshold, kmi_read_profile *out_dev,
                                       size_t capacity, uint64_t *n_reads) {
  return profile_reads_entry(idx, bytes_dev, n_bytes, true, solid_threshold, out_dev, capacity, n_reads);
}
kmi_status kmi_index_profile_reads_host(kmi_index *idx, const uint8_t *bytes, size_t n_bytes, uint32_t solid_threshold, kmi_read_profile *out,
                                        size_t capacity, uint64_t *n_reads) {
  return profile_reads_entry(idx, bytes, n_bytes, false, solid_threshold, out, capacity, n_reads);
}

// ---- the position indexes in the caller's order (kmi_locate.h)
// what a locate over device buffers left, to the caller's host buffers; st = its status (occ and offsets are complete when only the
// capacity was short)
static kmi_status locate_download(kmi_index *idx, kmi_status st, size_t nq, uint32_t *occ, const void *dc, uint64_t *offsets, const void *dof,
                                  uint64_t *values, const void *dv, size_t capacity, const uint64_t *n_hits) {
  kmi_ctx *ctx = idx->ctx;
  if (st != KMI_OK && !(st == KMI_ERR_OVERFLOW && *n_hits > capacity)) return st;
  if (nq) KMI_HIP(ctx, hipMemcpyAsync(occ, dc, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipMemcpyAsync(offsets, dof, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (st == KMI_OK && values && *n_hits)
    KMI_HIP(ctx, hipMemcpyAsync(values, dv, *n_hits * idx->val_words * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return st;
}
static kmi_status locate_entry(kmi_index *idx, const uint64_t *queries, size_t nq, bool on_device, uint32_t max_occ, uint32_t *occ, uint64_t *offsets,
                               uint64_t *values, size_t capacity, uint64_t *n_hits) {
  if (!idx || !n_hits) return KMI_ERR_INVALID;
  kmi_ctx *ctx = idx->ctx;
  *n_hits = 0;
  if (!idx->val_words) return set_err(ctx, KMI_ERR_INVALID, "locate() is a member of the position indexes");
  if (max_occ == 0) return set_err(ctx, KMI_ERR_INVALID, "max_occ is at least 1");
  if (!offsets || (nq && (!queries || !occ)) || (!values && capacity)) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  if (on_device) return index_locate(idx, queries, nq, max_occ, occ, offsets, values, capacity, n_hits);
  void *dq, *dc, *dof, *dv = nullptr;
  const size_t q_bytes = nq * idx->shape.n_words * sizeof(uint64_t), v_bytes = capacity * idx->val_words * sizeof(uint64_t);
  KMI_TRY(ws_get(ctx, WS_INPUT, q_bytes, &dq));
  KMI_TRY(ws_get(ctx, WS_LOOKUP_CNT, nq * sizeof(uint32_t), &dc));
  KMI_TRY(ws_get(ctx, WS_LOCATE_OFF, (nq + 1) * sizeof(uint64_t), &dof));
  if (values) KMI_TRY(ws_get(ctx, WS_OUTPUT2, v_bytes, &dv));
  if (nq) KMI_HIP(ctx, hipMemcpyAsync(dq, queries, q_bytes, hipMemcpyHostToDevice, ctx->stream));
  const kmi_status st = index_locate(idx, (const uint64_t *)dq, nq, max_occ, (uint32_t *)dc, (uint64_t *)dof, (uint64_t *)dv, capacity, n_hits);
  return locate_download(idx, st, nq, occ, dc, offsets, dof, values, dv, capacity, n_hits);
}
kmi_status kmi_index_locate_dev(kmi_index *idx, const uint64_t *queries_dev, size_t nq, uint32_t max_occ, uint32_t *occ_dev, uint64_t *offsets_dev,
                                uint64_t *values_dev, size_t capacity, uint64_t *n_hits) {
  return locate_entry(idx, queries_dev, nq, true, max_occ, occ_dev, offsets_dev, values_dev, capacity, n_hits);
}
kmi_status kmi_index_locate_host(kmi_index *idx, const uint64_t *queries, size_t nq, uint32_t max_occ, uint32_t *occ, uint64_t *offsets,
                                 uint64_t *values, size_t capacity, uint64_t *n_hits) {
  return locate_entry(idx, queries, nq, false, max_occ, occ, offsets, values, capacity, n_hits);
}

static kmi_status seed_reads_entry(kmi_index *idx, const uint8_t *bytes, size_t n_bytes, bool on_device, uint32_t max_occ, kmi_read_seeds *rows,
                                   size_t cap_reads, uint32_t *occ, uint64_t *offsets, size_t cap_kmers, uint64_t *values, size_t cap_hits,
                                   uint64_t *n_reads, uint64_t *n_kmers, uint64_t *n_hits) {
  if (!idx || !n_reads || !n_kmers || !n_hits) return KMI_ERR_INVALID;
  kmi_ctx *ctx = idx->ctx;
  *n_reads = *n_kmers = *n_hits = 0;
  if (!idx->val_words) return set_err(ctx, KMI_ERR_INVALID, "seed_reads() is a member of the position indexes");
  if (max_occ == 0) return set_err(ctx, KMI_ERR_INVALID, "max_occ is at least 1");
  if ((n_bytes && !bytes) || (!rows && cap_reads) || ((!occ || !offsets) && cap_kmers) || (!values && cap_hits))
    return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  return index_seed_reads(idx, bytes, n_bytes, on_device, max_occ, rows, cap_reads, occ, offsets, cap_kmers, values, cap_hits, n_reads, n_kmers, n_hits);
}
kmi_status kmi_index_seed_reads_dev(kmi_index *idx, const uint8_t *bytes_dev, size_t n_bytes, uint32_t max_occ, kmi_read_seeds *rows_dev, size_t cap_reads,
                                    uint32_t *occ_dev, uint64_t *offsets_dev, size_t cap_kmers, uint64_t *values_dev, size_t cap_hits,
                                    uint64_t *n_reads, uint64_t *n_kmers, uint64_t *n_hits) {
  return seed_reads_entry(idx, bytes_dev, n_bytes, true, max_occ, rows_dev, cap_reads, occ_dev, offsets_dev, cap_kmers, values_dev, cap_hits, n_reads,
                          n_kmers, n_hits);
}
kmi_status kmi_index_seed_reads_host(kmi_index *idx, const uint8_t *bytes, size_t n_bytes, uint32_t max_occ, kmi_read_seeds *rows, size_t cap_reads,
                                     uint32_t *occ, uint64_t *offsets, size_t cap_kmers, uint64_t *values, size_t cap_hits, uint64_t *n_reads,
                                     uint64_t *n_kmers, uint64_t *n_hits) {
  return seed_reads_entry(idx, bytes, n_bytes, false, max_occ, rows, cap_reads, occ, offsets, cap_kmers, values, cap_hits, n_reads, n_kmers, n_hits);
}

// ---- the same four over ranks (kmi_query_dist.h). Everything checked here is refused on this rank before anything collective.
static kmi_status query_dist_check(kmi_index *idx, kmi_comm *comm, bool position, const char *what) {
  KMI_TRY(dist_check(idx, comm));
  kmi_ctx *ctx = idx->ctx;
  if (position != (idx->val_words != 0))
    return set_err(ctx, KMI_ERR_INVALID, position ? "%s() is a member of the position indexes" : "%s() is a member of the count index", what);
  if (idx->owner_lp && (1u << idx->owner_lp) != (uint32_t)kmi::comm_size(comm))
    return set_err(ctx, KMI_ERR_INVALID, "%s(): the index is distributed over another number of owner ranks than the communicator has", what);
  return KMI_OK;
}

static kmi_status lookup_dist_entry(kmi_index *idx, kmi_comm *comm, const uint64_t *queries, size_t nq, uint32_t *counts, bool on_device) {
  KMI_TRY(query_dist_check(idx, comm, false, "lookup"));
  kmi_ctx *ctx = idx->ctx;
  if (nq && (!queries || !counts)) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  if (alone(ctx, comm)) return lookup_entry(idx, queries, nq, counts, on_device);
  if (on_device) return index_lookup_dist(idx, comm, queries, nq, counts);
  void *dq = nullptr, *dc = nullptr;
  const size_t q_bytes = nq * idx->shape.n_words * sizeof(uint64_t);
  const kmi_status staged = [&]() -> kmi_status {
    KMI_TRY(ws_get(ctx, WS_INPUT, q_bytes + 64, &dq));
    KMI_TRY(ws_get(ctx, WS_OUTPUT, nq * sizeof(uint32_t) + 64, &dc));
    if (nq) KMI_HIP(ctx, hipMemcpyAsync(dq, queries, q_bytes, hipMemcpyHostToDevice, ctx->stream));
    return KMI_OK;
  }();
  if (staged != KMI_OK) { uint64_t more = 0, want = 0; return qd_agree(comm, staged, &more, &want); }   // (the peers are told in their first all-reduce)
  KMI_TRY(index_lookup_dist(idx, comm, (const uint64_t *)dq, nq, (uint32_t *)dc));
  if (nq) KMI_HIP(ctx, hipMemcpyAsync(counts, dc, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KMI_OK;
}
kmi_status kmi_index_lookup_dist_dev(kmi_index *idx, kmi_comm *comm, const uint64_t *queries_dev, size_t nq, uint32_t *counts_dev) {
  return lookup_dist_entry(idx, comm, queries_dev, nq, counts_dev, true);
}
kmi_status kmi_index_lookup_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *queries, size_t nq, uint32_t *counts) {
  return lookup_dist_entry(idx, comm, queries, nq, counts, false);
}

static kmi_status profile_reads_dist_entry(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, bool on_device, uint32_t solid_threshold,
                                           kmi_read_profile *out, size_t capacity, uint64_t *n_reads) {
  if (!n_reads) return KMI_ERR_INVALID;
  *n_reads = 0;
  KMI_TRY(query_dist_check(idx, comm, false, "profile_reads"));
  kmi_ctx *ctx = idx->ctx;
  if (idx->cfg.seq_format != KMI_FMT_FASTQ) return set_err(ctx, KMI_ERR_INVALID, "profile_reads() reads FASTQ");
  if (solid_threshold == 0) return set_err(ctx, KMI_ERR_INVALID, "solid_threshold is at least 1");
  if ((n_bytes && !bytes) || (!out && capacity)) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  if (alone(idx->ctx, comm))
    return on_device ? kmi_index_profile_reads_dev(idx, bytes, n_bytes, solid_threshold, out, capacity, n_reads)
                     : kmi_index_profile_reads_host(idx, bytes, n_bytes, solid_threshold, out, capacity, n_reads);
  return index_profile_reads_dist(idx, comm, bytes, n_bytes, on_device, solid_threshold, out, capacity, n_reads);
}
kmi_status kmi_index_profile_reads_dist_dev(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes_dev, size_t n_bytes, uint32_t solid_threshold,
                                            kmi_read_profile *out_dev, size_t capacity, uint64_t *n_reads) {
  return profile_reads_dist_entry(idx, comm, bytes_dev, n_bytes, true, solid_threshold, out_dev, capacity, n_reads);
}
kmi_status kmi_index_profile_reads_dist_host(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint32_t solid_threshold,
                                             kmi_read_profile *out, size_t capacity, uint64_t *n_reads) {
  return profile_reads_dist_entry(idx, comm, bytes, n_bytes, false, solid_threshold, out, capacity, n_reads);
}

static kmi_status locate_dist_entry(kmi_index *idx, kmi_comm *comm, const uint64_t *queries, size_t nq, bool on_device, uint32_t max_occ, uint32_t *occ,
                                    uint64_t *offsets, uint64_t *values, size_t capacity, uint64_t *n_hits) {
  if (!n_hits) return KMI_ERR_INVALID;
  *n_hits = 0;
  KMI_TRY(query_dist_check(idx, comm, true, "locate"));
  kmi_ctx *ctx = idx->ctx;
  if (max_occ == 0) return set_err(ctx, KMI_ERR_INVALID, "max_occ is at least 1");
  if (!offsets || (nq && (!queries || !occ)) || (!values && capacity)) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  if (alone(ctx, comm)) return locate_entry(idx, queries, nq, on_device, max_occ, occ, offsets, values, capacity, n_hits);
  if (on_device) return index_locate_dist(idx, comm, queries, nq, max_occ, occ, offsets, values, capacity, n_hits);
  void *dq = nullptr, *dc = nullptr, *dof = nullptr, *dv = nullptr;
  const size_t q_bytes = nq * idx->shape.n_words * sizeof(uint64_t), v_bytes = capacity * idx->val_words * sizeof(uint64_t);
  const kmi_status staged = [&]() -> kmi_status {
    KMI_TRY(ws_get(ctx, WS_INPUT, q_bytes + 64, &dq));
    KMI_TRY(ws_get(ctx, WS_OUTPUT, nq * sizeof(uint32_t) + 64, &dc));
    KMI_TRY(ws_get(ctx, WS_LOCATE_OFF, (nq + 1) * sizeof(uint64_t), &dof));
    if (values) KMI_TRY(ws_get(ctx, WS_OUTPUT2, v_bytes + 64, &dv));
    if (nq) KMI_HIP(ctx, hipMemcpyAsync(dq, queries, q_bytes, hipMemcpyHostToDevice, ctx->stream));
    return KMI_OK;
  }();
  if (staged != KMI_OK) { uint64_t more = 0, want = 0; return qd_agree(comm, staged, &more, &want); }   // (the peers are told in their first all-reduce)
  const kmi_status st = index_locate_dist(idx, comm, (const uint64_t *)dq, nq, max_occ, (uint32_t *)dc, (uint64_t *)dof, (uint64_t *)dv, capacity, n_hits);
  return locate_download(idx, st, nq, occ, dc, offsets, dof, values, dv, capacity, n_hits);
}
kmi_status kmi_index_locate_dist_dev(kmi_index *idx, kmi_comm *comm, const uint64_t *queries_dev, size_t nq, uint32_t max_occ, uint32_t *occ_dev,
                                     uint64_t *offsets_dev, uint64_t *values_dev, size_t capacity, uint64_t *n_hits) {
  return locate_dist_entry(idx, comm, queries_dev, nq, true, max_occ, occ_dev, offsets_dev, values_dev, capacity, n_hits);
}
kmi_status kmi_index_locate_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *queries, size_t nq, uint32_t max_occ, uint32_t *occ,
                                      uint64_t *offsets, uint64_t *values, size_t capacity, uint64_t *n_hits) {
  return locate_dist_entry(idx, comm, queries, nq, false, max_occ, occ, offsets, values, capacity, n_hits);
}

static kmi_status seed_reads_dist_entry(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, bool on_device, uint32_t max_occ,
                                        kmi_read_seeds *rows, size_t cap_reads, uint32_t *occ, uint64_t *offsets, size_t cap_kmers, uint64_t *values,
                                        size_t cap_hits, uint64_t *n_reads, uint64_t *n_kmers, uint64_t *n_hits) {
  if (!n_reads || !n_kmers || !n_hits) return KMI_ERR_INVALID;
  *n_reads = *n_kmers = *n_hits = 0;
  KMI_TRY(query_dist_check(idx, comm, true, "seed_reads"));
  kmi_ctx *ctx = idx->ctx;
  if (max_occ == 0) return set_err(ctx, KMI_ERR_INVALID, "max_occ is at least 1");
  if ((n_bytes && !bytes) || (!rows && cap_reads) || ((!occ || !offsets) && cap_kmers) || (!values && cap_hits))
    return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  if (alone(idx->ctx, comm))
    return seed_reads_entry(idx, bytes, n_bytes, on_device, max_occ, rows, cap_reads, occ, offsets, cap_kmers, values, cap_hits, n_reads, n_kmers, n_hits);
  return index_seed_reads_dist(idx, comm, bytes, n_bytes, on_device, max_occ, rows, cap_reads, occ, offsets, cap_kmers, values, cap_hits, n_reads,
                               n_kmers, n_hits);
}
kmi_status kmi_index_seed_reads_dist_dev(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes_dev, size_t n_bytes, uint32_t max_occ,
                                         kmi_read_seeds *rows_dev, size_t cap_reads, uint32_t *occ_dev, uint64_t *offsets_dev, size_t cap_kmers,
                                         uint64_t *values_dev, size_t cap_hits, uint64_t *n_reads, uint64_t *n_kmers, uint64_t *n_hits) {
  return seed_reads_dist_entry(idx, comm, bytes_dev, n_bytes, true, max_occ, rows_dev, cap_reads, occ_dev, offsets_dev, cap_kmers, values_dev, cap_hits,
                               n_reads, n_kmers, n_hits);
}
kmi_status kmi_index_seed_reads_dist_host(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint32_t max_occ, kmi_read_seeds *rows,
                                          size_t cap_reads, uint32_t *occ, uint64_t *offsets, size_t cap_kmers, uint64_t *values, size_t cap_hits,
                                          uint64_t *n_reads, uint64_t *n_kmers, uint64_t *n_hits) {
  return seed_reads_dist_entry(idx, comm, bytes, n_bytes, false, max_occ, rows, cap_reads, occ, offsets, cap_kmers, values, cap_hits, n_reads, n_kmers,
                               n_hits);
}

}  // extern "C"
