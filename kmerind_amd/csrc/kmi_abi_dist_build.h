// kmi_abi_dist_build.h -- builds and queries over ranks: build_dist_superkmer, the build entries, FASTQ / FASTA byte ranges,
// query_dist_host, count / find / erase / size over ranks.
//
// Included by kmi_index.hip after kmi_query_dist.h: behind its host glue and the collectives' helpers (dist_check, dist_exchange,
// keys_to_owners, answers_to_askers, dist_agree, dist_state).
#pragma once

// The count index over ranks through exchanged super-k-mer records, CHUNKED: the rank's share is cut into record-aligned chunks;
// the records of chunk c travel on the communicator's stream while the front end of chunk c + 1 runs on the context's; the
// counts of a chunk ride with the verdict ("this rank could not produce it": then every rank sends that chunk as k-mers to the
// same owners afterwards) and with the sender's largest message. What arrived is consumed in one go.
static kmi_status build_dist_superkmer(kmi_index *idx, uint32_t w, kmi_comm *comm, const uint8_t *d_bytes, size_t n_bytes, uint64_t file_offset) {
  kmi_ctx *ctx = idx->ctx;
  const int p = kmi::comm_size(comm);
  const uint32_t lp = 31u - (uint32_t)__builtin_clz((uint32_t)p);
  const uint32_t nch = (idx->cfg.seq_format == KMI_FMT_FASTQ) ? ctx->dist_chunks : 1u;
  std::vector<uint64_t> cuts(nch + 1, 0);
  if (n_bytes) {
    if (nch > 1) KMI_TRY(kmi_fastq_partition_dev(ctx, d_bytes, n_bytes, nch, cuts.data()));
    else cuts[1] = n_bytes;
  }
  // the receive pool: every rank's bytes are known after one all-reduce; a rank receives about a p-th of all records
  uint64_t all_bytes = n_bytes;
  KMI_TRY(kmi::comm_allreduce_sum(comm, &all_bytes));
  uint64_t pool_cap = (uint64_t)((double)all_bytes / p * 0.06 * 1.3 * ctx->dist_pool_pct / 100.0) + ctx->dist_pool_slack;
  void *pv;
  KMI_TRY(ws_get(ctx, WS_DIST_B, pool_cap * 16, &pv));
  uint64_t *pool = (uint64_t *)pv;
  uint64_t pool_pos = 0;
  bool pool_in_b = true;
  uint64_t *sendbuf[2] = {nullptr, nullptr};
  size_t send_cap[2] = {0, 0};
  std::vector<uint32_t> failed;
  std::vector<uint64_t> sc(p), rc(p);
  const uint32_t lp_before = idx->owner_lp;
  idx->owner_lp = lp;   // (every rank is here: the route was agreed on; an error below puts the old value back)
  // A rank that fails on its own -- a parse or length verdict of its front end, a workspace it cannot get -- still enters the
  // chunk's count exchange and says so there (count = kHardError), so that every rank leaves this function with an error instead
  // of waiting in a send / receive for a peer that has already returned.
  constexpr uint64_t kNotProduced = ~0ull, kHardError = ~0ull - 1ull;
  kmi_status st_local = KMI_OK;
  bool peer_error = false;
  for (uint32_t c = 0; c < nch && st_local == KMI_OK && !peer_error; ++c) {
    const size_t cb = (size_t)(cuts[c + 1] - cuts[c]);
    const int sb = (int)(c & 1u);
    int produced = 0;
    auto produce_chunk = [&]() -> kmi_status {
      const size_t want = (size_t)((double)cb * 0.06) + 8192;
      if (c >= 2) KMI_TRY(kmi::comm_exchange_wait(comm));   // the buffer's previous message has left (the transfer before the last is done)
      if (send_cap[sb] < want) { KMI_TRY(ws_get(ctx, sb ? WS_DIST_C : WS_DIST_A, want * 16, &pv)); sendbuf[sb] = (uint64_t *)pv; send_cap[sb] = want; }
      const uint64_t *recs = nullptr;
      uint64_t nrec = 0;
      const uint8_t *src = d_bytes + cuts[c];   // (any address: the one-pass front end loads unaligned; the general one aligns its input itself)
      if (ctx->sk_dbg == 9 && comm_rank_of(comm) == 1 && c == 1) return set_err(ctx, KMI_ERR_PARSE, "test knob KMI_SK_DBG=9: rank 1 fails on its second chunk");
      KMI_TRY(sk_produce(idx, w, src, cb, (uint32_t)p, &recs, &nrec, sc.data(), &produced, sendbuf[sb], send_cap[sb]));
      if (produced && nrec && recs != sendbuf[sb]) {   // more records than the buffer was sized for: a larger one, and a copy out of the workspace
        KMI_TRY(kmi::comm_exchange_wait(comm));
        KMI_TRY(ws_get(ctx, sb ? WS_DIST_C : WS_DIST_A, (nrec + 64) * 16, &pv)); sendbuf[sb] = (uint64_t *)pv; send_cap[sb] = nrec + 64;
        KMI_HIP(ctx, hipMemcpyAsync(sendbuf[sb], recs, nrec * 16, hipMemcpyDeviceToDevice, ctx->stream));
      }
      return KMI_OK;
    };
    st_local = produce_chunk();
    uint64_t mine = 0, largest = 0;
    for (int r = 0; r < p; ++r) mine = std::max(mine, sc[r] * 16);
    std::vector<uint64_t> tell(sc);
    if (st_local != KMI_OK) { for (int r = 0; r < p; ++r) tell[r] = kHardError; mine = 0; }
    else if (!produced) for (int r = 0; r < p; ++r) tell[r] = kNotProduced;
    {
      const kmi_status st_x = kmi::comm_all_to_all_counts2(comm, tell.data(), mine, rc.data(), &largest);
      if (st_x != KMI_OK) { idx->owner_lp = lp_before; return st_local != KMI_OK ? st_local : st_x; }   // (the exchange itself failed: nothing more to agree on)
    }
    for (int r = 0; r < p; ++r) peer_error = peer_error || rc[r] == kHardError;
    if (st_local != KMI_OK || peer_error) break;
    bool all_ok = produced != 0;
    for (int r = 0; r < p; ++r) all_ok = all_ok && rc[r] != kNotProduced;
    if (!all_ok) { failed.push_back(c); continue; }
    uint64_t n_in = 0;
    for (int r = 0; r < p; ++r) n_in += rc[r];
    // (from here to the payload exchange only allocation can fail: a rank that cannot hold what it is sent has no way left to say so)
    if (pool_pos + n_in > pool_cap) {   // the estimate was short (a very uneven input): a pool twice the need, what arrived so far moves over
      KMI_TRY(kmi::comm_exchange_wait(comm));
      const uint64_t ncap = 2 * (pool_pos + n_in) + ctx->dist_pool_slack;
      ++ctx->dist_pool_regrows;
      KMI_TRY(ws_get(ctx, pool_in_b ? WS_DIST_D : WS_DIST_B, ncap * 16, &pv));
      if (pool_pos) KMI_HIP(ctx, hipMemcpyAsync(pv, pool, pool_pos * 16, hipMemcpyDeviceToDevice, ctx->stream));
      pool = (uint64_t *)pv; pool_cap = ncap; pool_in_b = !pool_in_b;
    }
    KMI_TRY(kmi::comm_all_to_all_v_async(comm, sendbuf[sb], sc.data(), pool + 2 * pool_pos, rc.data(), 16, largest));
    pool_pos += n_in;
  }
  KMI_TRY(kmi::comm_exchange_join(comm));
  if (st_local != KMI_OK || peer_error) {
    // what arrived before the error is dropped: the index is as it was (the transfers queued so far have been joined)
    (void)hipStreamSynchronize(ctx->stream);
    idx->owner_lp = lp_before;
    if (st_local != KMI_OK) return st_local;
    return set_err(ctx, KMI_ERR_PEER, "the build over ranks was given up: another rank reported an error in its share of the input");
  }
  {
    kmi_status st_c = pool_pos ? sk_consume(idx, w, pool, pool_pos, (uint32_t)p) : KMI_OK;
    // chunks some rank could not produce as records follow as k-mers, collectively: first agree that every rank is still there
    if (!failed.empty()) st_c = dist_agree(comm, st_c);
    if (st_c != KMI_OK) { if (!pool_pos || !idx->n_entries) idx->owner_lp = lp_before; return st_c; }
  }
  idx->owner_lp = lp;
  // chunks some rank could not produce as records: their k-mers, routed to the same owners (collective: every rank has the same list)
  for (uint32_t c : failed) {
    const size_t cb = (size_t)(cuts[c + 1] - cuts[c]);
    const uint32_t nw = idx->shape.n_words;
    uint64_t nt = 0, ns = 0, total = 0;
    void *d_keys = nullptr, *d_send = nullptr, *d_recv = nullptr;
    auto route_chunk = [&]() -> kmi_status {
      const uint8_t *src = d_bytes + cuts[c];
      if (cb) { KMI_TRY(align_input(ctx, &src, cb)); KMI_TRY(extract_count(ctx, &idx->cfg, src, cb, &nt, &ns)); }
      KMI_TRY(ws_get(ctx, WS_OUTPUT, (nt + 64) * nw * sizeof(uint64_t), &d_keys));
      KMI_TRY(ws_get(ctx, WS_DIST_A, (nt + 64) * nw * sizeof(uint64_t), &d_send));
      send_cap[0] = 0;
      for (int r = 0; r < p; ++r) sc[r] = 0;
      if (nt) {
        KMI_TRY(extract_run(ctx, &idx->cfg, src, cb, file_offset + cuts[c], (uint64_t *)d_keys, nullptr, (size_t)nt, true, true, &nt, &ns));
        KMI_TRY(kmi_route_owner_dev(ctx, &idx->cfg, (const uint64_t *)d_keys, (size_t)nt, (uint32_t)p, (uint64_t *)d_send, sc.data()));
      }
      return KMI_OK;
    };
    KMI_TRY(dist_agree(comm, route_chunk()));
    std::vector<uint64_t> rcv;
    KMI_TRY(dist_exchange(comm, d_send, sc.data(), nw * sizeof(uint64_t), WS_DIST_D, &d_recv, rcv, &total));
    KMI_TRY(index_insert(idx, (const uint64_t *)d_recv, (size_t)total, false));
    idx->owner_lp = lp;
  }
  return KMI_OK;
}

extern "C" {

kmi_status kmi_index_build_dist_dev(kmi_index *idx, kmi_comm *comm, const uint8_t *d_bytes, size_t n_bytes, uint64_t file_offset) {
  KMI_TRY(dist_check(idx, comm));
  kmi_ctx *ctx = idx->ctx;
  const int p = kmi::comm_size(comm);
  if (alone(ctx, comm)) return kmi_index_build_dev(idx, d_bytes, n_bytes, file_offset);
  if (n_bytes && !d_bytes) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  const uint32_t nw = idx->shape.n_words, vw = idx->val_words, rw = nw + vw;
  void *d_send = nullptr, *d_recv;
  std::vector<uint64_t> sc(p, 0), rc;
  uint64_t nt = 0, ns = 0, total = 0;
  if (vw == 0) {
    // the route follows from state every rank has agreed on (never from one rank's own entry count: a rank with an empty share
    // would otherwise take another branch than its peers, and the branches issue different collectives)
    uint64_t holders = 0, owner_p = 0, owner_any = 0;
    KMI_TRY(dist_state(idx, comm, &holders, &owner_p, &owner_any));
    if (owner_any && owner_any != (uint64_t)p && holders)
      return set_err(ctx, KMI_ERR_INVALID, "the ranks disagree on how this index is distributed (some by minimizer owner, some not)");
    const uint32_t skw = sk_width_of(idx);
    const bool by_owner = owner_any != 0 && holders != 0;                 // the entries are already distributed by minimizer owner
    if (skw && sk_rank_count((uint32_t)p) && (holders == 0 || owner_p == (uint64_t)p)) {
      if (holders == 0) idx->owner_lp = 0;
      return build_dist_superkmer(idx, skw, comm, d_bytes, n_bytes, file_offset);
    }
    KMI_TRY(align_input(ctx, &d_bytes, n_bytes));   // (the scan's 16-byte loads: a range build hands in its buffer + the first record's offset)
    if (n_bytes) KMI_TRY(extract_count(ctx, &idx->cfg, d_bytes, n_bytes, &nt, &ns));   // (an empty share still enters the collectives)
    KMI_TRY(ws_get(ctx, WS_DIST_A, (nt + 64) * nw * sizeof(uint64_t), &d_send));
    if (by_owner) {
      // k-mers into an index that is distributed by minimizer owner go to those owners
      void *d_keys;
      KMI_TRY(ws_get(ctx, WS_OUTPUT, (nt + 64) * nw * sizeof(uint64_t), &d_keys));
      if (nt) {
        KMI_TRY(extract_run(ctx, &idx->cfg, d_bytes, n_bytes, file_offset, (uint64_t *)d_keys, nullptr, (size_t)nt, true, true, &nt, &ns));
        KMI_TRY(kmi_route_owner_dev(ctx, &idx->cfg, (const uint64_t *)d_keys, (size_t)nt, (uint32_t)p, (uint64_t *)d_send, sc.data()));
      }
    } else if (nt && idx->cfg.seq_format == KMI_FMT_FASTQ) {
      // read_file + the bucketing half of imxx::distribute, fused: the tuple array in file order never exists
      KMI_TRY(kmi_extract_route_dev(ctx, &idx->cfg, d_bytes, n_bytes, (uint32_t)p, (uint64_t *)d_send, (size_t)nt, &nt, &ns, sc.data()));
    } else if (nt) {
      void *d_keys;
      KMI_TRY(ws_get(ctx, WS_OUTPUT, (nt + 64) * nw * sizeof(uint64_t), &d_keys));
      KMI_TRY(extract_run(ctx, &idx->cfg, d_bytes, n_bytes, file_offset, (uint64_t *)d_keys, nullptr, (size_t)nt, true, true, &nt, &ns));
      KMI_TRY(kmi_route_dev(ctx, &idx->cfg, (const uint64_t *)d_keys, (size_t)nt, (uint32_t)p, (uint64_t *)d_send, sc.data()));
    }
    KMI_TRY(dist_exchange(comm, d_send, sc.data(), nw * sizeof(uint64_t), WS_DIST_B, &d_recv, rc, &total));
    return index_insert(idx, (const uint64_t *)d_recv, (size_t)total, false);
  }
  KMI_TRY(align_input(ctx, &d_bytes, n_bytes));
  if (n_bytes) KMI_TRY(extract_count(ctx, &idx->cfg, d_bytes, n_bytes, &nt, &ns));
  if (vw == 2 && idx->cfg.seq_format != KMI_FMT_FASTQ)
    return set_err(ctx, KMI_ERR_INVALID, "a position + quality index over ranks is built from FASTQ partitions");
  KMI_TRY(ws_get(ctx, WS_DIST_A, (nt + 64) * rw * sizeof(uint64_t), &d_send));
  if (nt)
    KMI_TRY(kmi_extract_route_records_dev(ctx, &idx->cfg, d_bytes, n_bytes, file_offset, (uint32_t)p, (uint64_t *)d_send, (size_t)nt + 64,
                                          &nt, &ns, sc.data()));
  KMI_TRY(dist_exchange(comm, d_send, sc.data(), rw * sizeof(uint64_t), WS_DIST_B, &d_recv, rc, &total));
  return index_insert_records(idx, (const uint64_t *)d_recv, (size_t)total, true);
}

kmi_status kmi_index_build_range_dist_host(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint64_t buffer_offset,
                                           uint64_t nominal_bytes, int reaches_eof, int *need_more) {
  KMI_TRY(dist_check(idx, comm));
  kmi_ctx *ctx = idx->ctx;
  if (!need_more) return KMI_ERR_INVALID;
  *need_more = 0;
  if (n_bytes && !bytes) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  if (idx->cfg.seq_format != KMI_FMT_FASTQ) return set_err(ctx, KMI_ERR_INVALID, "a byte range of a file is cut at FASTQ record starts here (a FASTA partition comes with kmi_ctx_set_fasta_partition)");
  void *d_bytes;
  uint64_t cut[2];
  KMI_TRY(fastq_range_cut(ctx, WS_INPUT, bytes, n_bytes, buffer_offset, nominal_bytes, reaches_eof, &d_bytes, cut, need_more));
  if (*need_more) return KMI_OK;
  return kmi_index_build_dist_dev(idx, comm, (const uint8_t *)d_bytes + cut[0], (size_t)(cut[1] - cut[0]), buffer_offset + cut[0]);
}

kmi_status kmi_index_build_fasta_file_dist_host(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes) {
  // every rank holds the WHOLE FASTA file; the block bookkeeping of an equal split over the ranks (where each block's valid range
  // begins, the machine state and the record count there: file.hpp:1436-1610 + fasta_loader.hpp:202-470) is computed on the device
  // from the whole buffer, every rank keeps its own block and enters the collective build with it
  KMI_TRY(dist_check(idx, comm));
  kmi_ctx *ctx = idx->ctx;
  if (idx->cfg.seq_format != KMI_FMT_FASTA) return set_err(ctx, KMI_ERR_INVALID, "not a FASTA index");
  if (n_bytes && !bytes) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  const uint32_t p = (uint32_t)kmi::comm_size(comm), r = (uint32_t)kmi::comm_rank(comm);
  void *d_bytes;
  KMI_TRY(stage_host(ctx, WS_INPUT, bytes, n_bytes, 64, &d_bytes));
  std::vector<uint64_t> be(2 * (size_t)p);
  std::vector<kmi_fasta_partition> parts(p);
  KMI_TRY(kmi_fasta_partition_dev(ctx, (const uint8_t *)d_bytes, n_bytes, p, idx->shape.k, be.data(), parts.data()));
  KMI_TRY(kmi_ctx_set_fasta_partition(ctx, &parts[r]));
  const kmi_status st = kmi_index_build_dist_dev(idx, comm, (const uint8_t *)d_bytes + be[2 * r], (size_t)(be[2 * r + 1] - be[2 * r]), be[2 * r]);
  (void)kmi_ctx_set_fasta_partition(ctx, nullptr);
  return st;
}

// FASTA over ranks by BYTE RANGE (file.hpp:1436-1610, fasta_loader.hpp:202-470): the rank brings only its block of an equal split of
// the file plus look-ahead, and what it cannot know from its own bytes -- the kind of line its first byte sits on, the records that
// start before it, whether the file opens with a header -- comes from the other ranks' block summaries (kmi_fasta_block_summary_dev:
// the line-kind machine over a block as a transfer function), gathered once and composed left to right. bytes = file bytes
// [buffer_offset, buffer_offset + n_bytes), the first nominal_bytes of them the rank's block; prev_byte = the file byte before the
// buffer (-1 at the file start); *need_more = 1: the `behind` sequence characters behind the block (the last windows' overlap: k - 1
// for k-mers, k for de Bruijn tuples, whose last window also needs its right neighbour) do not end inside the look-ahead -- nothing
// collective has happened, the caller reads further and calls again.
// the bookkeeping of a block: *need_more (nothing collective has happened then), or the partition record and where the block's
// windows end inside the buffer. d_bytes = the buffer on the device (already in flight on the context's stream). carry_out
// (optional): the raw byte of the last sequence character before the block in the same record, -1 when there is none (a record
// starts in between, or the block opens the file) -- the in-edge of the block's first window, from the blocks' left carries
// composed right to left.
static kmi_status fasta_range_partition(kmi_ctx *ctx, kmi_comm *comm, uint32_t behind, const uint8_t *bytes, const uint8_t *d_bytes, size_t n_bytes,
                                        uint64_t buffer_offset, uint64_t nominal_bytes, int reaches_eof, int prev_byte, int *need_more,
                                        kmi_fasta_partition *part_out, uint64_t *end_out, int *carry_out = nullptr) {
  const uint32_t p = (uint32_t)kmi::comm_size(comm), r = (uint32_t)kmi::comm_rank(comm);
  const bool first_ls = buffer_offset == 0 || prev_byte == (int)'\n';
  constexpr size_t NWD = 11;   // out6, the file's first byte, the block's length, the left carry per incoming state
  uint64_t mine[NWD] = {0, 0, 1, 0, 2, 0, 0, 0, 0, 0, 0};
  KMI_TRY(kmi::fasta_block_summary(ctx, d_bytes, (size_t)nominal_bytes, first_ls, mine, mine + 8));
  mine[6] = (buffer_offset == 0 && n_bytes) ? bytes[0] : 0;   // (rank 0: the file's first byte decides init_parser's index shift)
  mine[7] = nominal_bytes;
  // where the overlap ends: the behind-th sequence character at or behind the block's end, for every state the machine may be in there
  auto step = [](uint32_t &state, uint8_t c) {
    if (c == '>' || c == ';') state = KMI_FA_HEADER;
    else state = (state == KMI_FA_OUTSIDE) ? (uint32_t)KMI_FA_OUTSIDE : (uint32_t)KMI_FA_SEQUENCE;
  };
  uint64_t end_for[3] = {nominal_bytes, nominal_bytes, nominal_bytes};
  for (uint32_t st0 = 0; st0 < 3; ++st0) {
    if (behind == 0 || nominal_bytes >= n_bytes) { end_for[st0] = nominal_bytes < n_bytes ? nominal_bytes : n_bytes; continue; }
    uint32_t st = st0, need = behind;
    uint64_t i = nominal_bytes;
    for (; i < n_bytes && need; ++i) {
      const uint8_t c = bytes[i];
      const bool ls = i == 0 ? first_ls : bytes[i - 1] == '\n';
      if (ls) step(st, c);
      if (st == KMI_FA_SEQUENCE && c != '\n' && c != '\r') --need;
    }
    if (need && !reaches_eof) { *need_more = 1; return KMI_OK; }
    end_for[st0] = need ? n_bytes : i;
  }
  if (behind > 0 && nominal_bytes >= n_bytes && !reaches_eof && p > 1 && r + 1 < p) { *need_more = 1; return KMI_OK; }   // (no look-ahead at all behind a block that is not the file's last)
  // ---- collective from here on
  std::vector<uint64_t> all((size_t)p * NWD);
  KMI_TRY(kmi::comm_allgather_words(comm, mine, NWD, all.data()));
  uint32_t st = KMI_FA_OUTSIDE; uint64_t ev = 0;
  std::vector<uint32_t> st_in(r + 1);   // the state every block before this one is entered in
  for (uint32_t q = 0; q < r; ++q) { const uint64_t *t = &all[(size_t)q * NWD]; st_in[q] = st; ev += t[2 * st + 1]; st = (uint32_t)t[2 * st]; }
  if (carry_out) {
    *carry_out = -1;
    for (uint32_t q = r; q-- > 0;) {   // the nearest block to the left that holds a sequence character or a record start decides
      const uint64_t c = all[(size_t)q * NWD + 8 + st_in[q]];
      if (c == kmi::KMI_FA_CARRY_PASS) continue;
      if (c & kmi::KMI_FA_CARRY_BYTE) *carry_out = (int)(c & 0xFFu);
      break;
    }
  }
  uint64_t first = 0;
  for (uint32_t q = 0; q < p; ++q) if (all[(size_t)q * NWD + 7]) { first = all[(size_t)q * NWD + 6]; break; }   // the first non-empty block opens the file
  kmi_fasta_partition part; memset(&part, 0, sizeof(part));
  part.valid_bytes = nominal_bytes;
  part.start_state = buffer_offset == 0 ? (uint32_t)KMI_FA_OUTSIDE : st;
  part.at_line_start = first_ls ? 1u : 0u;
  part.records_before = ev;
  part.index_shift = (first == '>' || first == ';') ? 0u : 1u;
  const uint32_t st_end = (uint32_t)mine[2 * part.start_state];   // the machine's state behind the block
  const uint64_t end = end_for[st_end] < nominal_bytes ? nominal_bytes : end_for[st_end];
  *part_out = part;
  *end_out = end < n_bytes ? end : n_bytes;
  return KMI_OK;
}

kmi_status kmi_index_build_fasta_range_dist_host(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint64_t buffer_offset,
                                                 uint64_t nominal_bytes, int reaches_eof, int prev_byte, int *need_more) {
  KMI_TRY(dist_check(idx, comm));
  kmi_ctx *ctx = idx->ctx;
  if (!need_more) return KMI_ERR_INVALID;
  *need_more = 0;
  if (idx->cfg.seq_format != KMI_FMT_FASTA) return set_err(ctx, KMI_ERR_INVALID, "not a FASTA index");
  if ((n_bytes && !bytes) || nominal_bytes > n_bytes) return set_err(ctx, KMI_ERR_INVALID, "bad buffer");
  void *d_bytes;
  KMI_TRY(stage_host(ctx, WS_INPUT, bytes, n_bytes, 64, &d_bytes));
  kmi_fasta_partition part; uint64_t end = 0;
  KMI_TRY(fasta_range_partition(ctx, comm, idx->shape.k - 1u, bytes, (const uint8_t *)d_bytes, n_bytes, buffer_offset, nominal_bytes, reaches_eof,
                                prev_byte, need_more, &part, &end));
  if (*need_more) return KMI_OK;
  KMI_TRY(kmi_ctx_set_fasta_partition(ctx, &part));
  const kmi_status stb = kmi_index_build_dist_dev(idx, comm, (const uint8_t *)d_bytes, (size_t)end, buffer_offset);
  (void)kmi_ctx_set_fasta_partition(ctx, nullptr);
  return stb;
}

// read_file_* of a FASTA file on one rank of several, by byte range (kmer_file_helper.hpp:550-633 over FASTALoader's partitions,
// fasta_loader.hpp:202-470): the same bookkeeping, then the block's tuples to the host. Collective over comm (one small gather).
kmi_status kmi_extract_fasta_range_dist_host(kmi_ctx *ctx, const kmi_config *cfg, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes,
                                             uint64_t buffer_offset, uint64_t nominal_bytes, int reaches_eof, int prev_byte, int *need_more,
                                             kmi_tuples *out) {
  if (!ctx || !cfg || !comm || !out || !need_more) return KMI_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  *need_more = 0;
  if (cfg->seq_format != KMI_FMT_FASTA) return set_err(ctx, KMI_ERR_INVALID, "not FASTA");
  if ((n_bytes && !bytes) || nominal_bytes > n_bytes) return set_err(ctx, KMI_ERR_INVALID, "bad buffer");
  KMI_HIP(ctx, hipSetDevice(ctx->device));
  void *d_bytes;
  KMI_TRY(stage_host(ctx, WS_INPUT2, bytes, n_bytes, 64, &d_bytes));
  kmi_fasta_partition part; uint64_t end = 0;
  KMI_TRY(fasta_range_partition(ctx, comm, cfg->k - 1u, bytes, (const uint8_t *)d_bytes, n_bytes, buffer_offset, nominal_bytes, reaches_eof,
                                prev_byte, need_more, &part, &end));
  if (*need_more || end == 0) return KMI_OK;
  KMI_TRY(kmi_ctx_set_fasta_partition(ctx, &part));
  const kmi_status st = kmi_extract_host(ctx, cfg, bytes, (size_t)end, buffer_offset, out);
  (void)kmi_ctx_set_fasta_partition(ctx, nullptr);
  return st;
}

kmi_status kmi_index_build_dist_host(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint64_t file_offset) {
  KMI_TRY(dist_check(idx, comm));
  kmi_ctx *ctx = idx->ctx;
  if (alone(ctx, comm)) return kmi_index_build_host(idx, bytes, n_bytes, file_offset);
  if (n_bytes && !bytes) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  void *d_bytes;
  KMI_TRY(stage_host(ctx, WS_INPUT, bytes, n_bytes, 64, &d_bytes));
  return kmi_index_build_dist_dev(idx, comm, (const uint8_t *)d_bytes, n_bytes, file_offset);
}

static kmi_status query_dist_host(kmi_index *idx, kmi_comm *comm, int mode, const uint64_t *queries, size_t nq, kmi_results *out, uint64_t *n_erased) {
  KMI_TRY(dist_check(idx, comm));
  kmi_ctx *ctx = idx->ctx;
  const int p = kmi::comm_size(comm);
  if (alone(ctx, comm)) return query_host(idx, mode, queries, nq, out, n_erased);
  if (out) memset(out, 0, sizeof(*out));
  if (n_erased) *n_erased = 0;
  if (nq && !queries) return set_err(ctx, KMI_ERR_INVALID, "null buffer");
  const uint32_t nw = idx->shape.n_words, ow = idx->val_words ? idx->val_words : 1u;
  const size_t kb = nw * sizeof(uint64_t), vb = ow * sizeof(uint64_t);
  void *d_q;
  std::vector<uint64_t> rc;
  uint64_t total = 0;
  KMI_TRY(keys_to_owners(idx, comm, queries, nq, idx->owner_lp != 0, &d_q, rc, &total));
  if (mode == Q_ERASE) {
    uint64_t n = 0;
    if (total) KMI_TRY(index_query(idx, Q_ERASE, (const uint64_t *)d_q, (size_t)total, nullptr, nullptr, 0, &n));
    if (n_erased) *n_erased = n;
    return KMI_OK;
  }
  // every source rank's keys are answered on their own (a key two ranks ask about is answered to both). The answers of a multimap
  // find are sized by a count of the hits per source (a bound by the entries of the index, per source, is p times the index)
  const bool mm_find = idx->val_words > 0 && mode == Q_FIND;
  std::vector<uint64_t> back(p, 0);
  uint64_t bound = 0, off = 0;
  for (int s = 0; s < p; ++s) {
    if (mm_find) {
      if (rc[s]) KMI_TRY(index_query(idx, mode, (const uint64_t *)d_q + off * nw, (size_t)rc[s], nullptr, nullptr, 0, &back[s], nullptr, nullptr, true));
      bound += back[s];
    } else bound += query_result_bound(idx, mode, (size_t)rc[s]);
    off += rc[s];
  }
  void *d_rk, *d_rv;
  KMI_TRY(ws_get(ctx, WS_DIST_C, (bound + 8) * kb, &d_rk));
  KMI_TRY(ws_get(ctx, WS_DIST_D, (bound + 8) * vb, &d_rv));
  uint64_t pos = 0;
  off = 0;
  for (int s = 0; s < p; ++s) {
    uint64_t n = 0;
    if (rc[s] && (!mm_find || back[s]))
      KMI_TRY(index_query(idx, mode, (const uint64_t *)d_q + off * nw, (size_t)rc[s], (uint64_t *)d_rk + pos * nw, (uint64_t *)d_rv + pos * ow,
                          mm_find ? back[s] : query_result_bound(idx, mode, (size_t)rc[s]), &n));
    back[s] = n; off += rc[s]; pos += n;
  }
  return answers_to_askers(comm, d_rk, d_rv, back, kb, vb, out);
}

kmi_status kmi_index_count_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *queries, size_t nq, kmi_results *out) {
  if (!out) return KMI_ERR_INVALID;
  return query_dist_host(idx, comm, Q_COUNT, queries, nq, out, nullptr);
}
kmi_status kmi_index_find_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *queries, size_t nq, kmi_results *out) {
  if (!out) return KMI_ERR_INVALID;
  return query_dist_host(idx, comm, Q_FIND, queries, nq, out, nullptr);
}
kmi_status kmi_index_erase_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *queries, size_t nq, uint64_t *n_erased_local) {
  return query_dist_host(idx, comm, Q_ERASE, queries, nq, nullptr, n_erased_local);
}
kmi_status kmi_index_size_dist(kmi_index *idx, kmi_comm *comm, uint64_t *n) {
  if (!n) return KMI_ERR_INVALID;
  KMI_TRY(dist_check(idx, comm));
  *n = idx->n_entries;
  return kmi::comm_allreduce_sum(comm, n);
}

}  // extern "C"
