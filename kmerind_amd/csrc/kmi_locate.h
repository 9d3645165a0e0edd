// The position indexes in the caller's order (no counterpart in the reference, whose find() returns the (key, value) pairs of the
// distinct queried keys, unordered, and knows no cap on repeats):
//   kmi_index_locate_*      occ[i] = entries under InputTransform(queries[i]); a CSR (offsets, values) of the value words of every
//                           query with at most max_occ entries, one answer per query in query order
//   kmi_index_seed_reads_*  the same CSR over every window of every FASTQ record of a buffer, and one kmi_read_seeds row per record
// The queries travel as (key words, tag) records through the partition, as in kmi_lookup.h. A position index keeps a fine bucket's
// entries unsorted (bucket_concat_kernel), so both per-bucket kernels build an LDS table from the bucket's ENTRIES whose slot value is
// the key's multiplicity:
//   bucket_locate_count_kernel  streams the bucket's query records against it: occ[tag]
//   (device-wide exclusive scan of listed(i) into offsets)
//   bucket_locate_fill_kernel   turns the slot counts into group starts (workgroup scan over the slots), groups the bucket's entry
//                               positions by key in a scratch array (one u32 per index entry, claimed with an LDS cursor per slot)
//                               and copies every listed query's group to values[offsets[tag] ...]
// Entries are not distinct here, so entries / limit is no lower bound on the passes: both kernels start at one pass and double on
// table overflow, by pass_of(place_hash) for entries and queries alike.
//
// Included by kmi_index.hip after kmi_lookup.h.
#pragma once

namespace kmi {

// The fill kernel's table: a slot carries a cursor beside its count, a second u32, and with it QTabCfg's two- to four-word tables
// would need 165 to 172 KB. Fewer home slots instead: 28 / 36 / 44 B per slot give 140 / 135 / 132 KB, one workgroup of eight
// wavefronts per CU as in the lookup. One-word keys (16 B per slot) keep two workgroups per CU: 77 KB each.
template <int NW> struct LTabCfg {
  static constexpr int CAP = (NW == 1) ? 4864 : (NW == 2 ? 5120 : (NW == 3 ? 3840 : 3072));
  static constexpr int PAD = TabCfg<NW>::PAD;
  static constexpr int SLOTS = CAP + PAD;
  static constexpr int LIMIT = CAP * 3 / 4;
  static constexpr int NT = 512;
  // keys, count, tag (tagged tables), cursor; control words, the scan's scratch and the special key's cursor
  static constexpr int LDS_BYTES = SLOTS * (NW * 8 + 4 + (NW == 1 ? 0 : 4) + 4) + 256;
};
static_assert(LTabCfg<1>::LDS_BYTES <= 80 * 1024, "two workgroups of the one-word fill kernel share a CU's 160 KB of LDS");
static_assert(LTabCfg<2>::LDS_BYTES <= 160 * 1024 && LTabCfg<3>::LDS_BYTES <= 160 * 1024 && LTabCfg<4>::LDS_BYTES <= 160 * 1024,
              "the fill kernel's table, its cursors included, fits a CU's 160 KB of LDS");

// home slots of a bucket's table: twice the bucket's entries, at least 512, at most what the knob allows (as bucket_lookup_kernel)
template <int NW, typename CFG> __device__ __forceinline__ void locate_size_table(LdsTable<NW> &tab, uint64_t entries, uint32_t cap_limit) {
  uint32_t want = 2u * (uint32_t)(entries < (uint64_t)CFG::CAP ? entries : (uint64_t)CFG::CAP);
  want = (want + 255u) & ~255u;
  want = want < 512u ? 512u : want;
  want = want < cap_limit ? want : cap_limit;
  if (want < (uint32_t)CFG::CAP) { tab.cap = want; tab.slots = want + CFG::PAD; tab.limit = want * 3u / 4u; }
}

// Fine bucket b: table of the bucket's entries (key -> multiplicity), then occ[tag] for every query record of the bucket. A query is
// answered in the pass its hash belongs to, hit or miss, so every occ[] word is written exactly once per attempt.
template <int NW>
__global__ __launch_bounds__((QTabCfg<NW>::NT)) void bucket_locate_count_kernel(const uint64_t *__restrict__ recs, const uint64_t *__restrict__ rec_off,
                                                                              const uint64_t *__restrict__ idx_keys, const uint64_t *__restrict__ idx_off,
                                                                              uint32_t cap_limit, uint32_t *__restrict__ occ,
                                                                              uint32_t *__restrict__ over_limit, uint32_t *__restrict__ max_npass) {
  KMI_TABLE_LDS_CFG(NW, QTabCfg<NW>)
  constexpr int RW = NW + 1;
  const uint32_t b = blockIdx.x;
  const uint64_t rb = rec_off[b], re = rec_off[b + 1];
  if (rb == re) return;
  const uint64_t ib = idx_off[b], ie = idx_off[b + 1];
  if (ib == ie) {
    for (uint64_t i = rb + threadIdx.x; i < re; i += blockDim.x) occ[recs[i * RW + NW]] = 0u;
    return;
  }
  locate_size_table<NW, QTabCfg<NW>>(tab, ie - ib, cap_limit);
  uint32_t npass = 1;
  while (true) {
    bool failed = false;
    for (uint32_t pass = 0; pass < npass && !failed; ++pass) {
      table_clear<NW>(tab);
      lds_barrier();
      for_each_key<NW, BatchOf<NW>::U>(idx_keys, ib, ie, [&](const uint64_t (&k)[NW], uint64_t) {
        const uint32_t h = place_hash<NW>(k);
        if (pass_of(h, npass) != pass) return;
        const int s = table_upsert<NW>(tab, k, h);
        if (s >= 0) atomicAdd(&tab.vals[s], 1u); else if (s == -2) atomicAdd(tab.special, 1u);
      });
      lds_barrier();
      if (*tab.overflow) { failed = true; break; }
      for (uint64_t i = rb + threadIdx.x; i < re; i += blockDim.x) {
        uint64_t k[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) k[w] = recs[i * RW + w];
        const uint32_t h = place_hash<NW>(k);
        if (pass_of(h, npass) != pass) continue;
        const uint64_t tag = recs[i * RW + NW];
        const int s = table_find<NW>(tab, k, h);
        occ[tag] = s >= 0 ? tab.vals[s] : (s == -2 ? *tab.special : 0u);
      }
      lds_barrier();
    }
    if (!failed) break;
    npass *= 2;
    if (npass > kMaxPasses) { if (threadIdx.x == 0) atomicOr(over_limit, 1u); break; }
    lds_barrier();
  }
  if (threadIdx.x == 0) atomicMax(max_npass, npass > kMaxPasses ? kMaxPasses : npass);
}

// a group of at least this many entries is copied by its wavefront together, a shorter one by the query's own lane
constexpr uint32_t kLocateWaveMin = 32;

// Fine bucket b, after the scan: the same table and pass schedule. Per pass: count the entries per key, scan the slot counts into
// group starts (cur[slot]), claim cur[slot]++ for every entry of a listed key and write the entry's position (relative to the
// bucket) there -- pos[idx_off[b] ...], reused by every pass --, then copy the group of every listed query of the pass to
// values[offsets[tag] ...]. After the claims cur[slot] is the group's end, so a group is [cur - count, cur).
template <int NW, int VW>
__global__ __launch_bounds__((LTabCfg<NW>::NT)) void bucket_locate_fill_kernel(const uint64_t *__restrict__ recs, const uint64_t *__restrict__ rec_off,
                                                                             const uint64_t *__restrict__ idx_keys, const uint64_t *__restrict__ idx_mvals,
                                                                             const uint64_t *__restrict__ idx_off, uint32_t cap_limit, uint32_t max_occ,
                                                                             const uint64_t *__restrict__ offsets, uint32_t *pos,
                                                                             uint64_t *__restrict__ values, uint32_t *__restrict__ over_limit,
                                                                             uint32_t *__restrict__ max_npass) {
  using Cfg = LTabCfg<NW>;
  KMI_TABLE_LDS_CFG(NW, Cfg)
  __shared__ uint32_t s_cur[Cfg::SLOTS];
  __shared__ uint32_t s_scan[Cfg::NT / kWave + 1];
  __shared__ uint32_t s_sp;   // the cursor of the key that equals the empty marker
  constexpr int RW = NW + 1;
  const uint32_t b = blockIdx.x;
  const uint64_t rb = rec_off[b], re = rec_off[b + 1];
  if (rb == re) return;
  const uint64_t ib = idx_off[b], ie = idx_off[b + 1];
  if (ib == ie) return;
  if (ie - ib > 0xffffffffull) { if (threadIdx.x == 0) atomicOr(over_limit, 1u); return; }   // (the positions are 32-bit)
  {
    // a bucket none of whose queries lists anything has nothing to group
    int any = 0;
    for (uint64_t i = rb + threadIdx.x; i < re; i += blockDim.x) {
      const uint64_t tag = recs[i * RW + NW];
      any |= offsets[tag + 1] != offsets[tag];
    }
    if (!__syncthreads_or(any)) return;
  }
  locate_size_table<NW, Cfg>(tab, ie - ib, cap_limit);
  uint32_t npass = 1;
  while (true) {
    bool failed = false;
    for (uint32_t pass = 0; pass < npass && !failed; ++pass) {
      table_clear<NW>(tab);
      lds_barrier();
      for_each_key<NW, BatchOf<NW>::U>(idx_keys, ib, ie, [&](const uint64_t (&k)[NW], uint64_t) {
        const uint32_t h = place_hash<NW>(k);
        if (pass_of(h, npass) != pass) return;
        const int s = table_upsert<NW>(tab, k, h);
        if (s >= 0) atomicAdd(&tab.vals[s], 1u); else if (s == -2) atomicAdd(tab.special, 1u);
      });
      lds_barrier();
      if (*tab.overflow) { failed = true; break; }
      {
        // slot counts -> group starts: every thread takes a run of slots, the runs' sums go through the workgroup scan
        const uint32_t per = (tab.slots + (uint32_t)Cfg::NT - 1u) / (uint32_t)Cfg::NT;
        const uint32_t s0 = threadIdx.x * per < tab.slots ? threadIdx.x * per : tab.slots;
        const uint32_t s1 = s0 + per < tab.slots ? s0 + per : tab.slots;
        uint32_t sum = 0;
        for (uint32_t s = s0; s < s1; ++s) sum += tab.vals[s];
        uint32_t tot = 0;
        uint32_t base = block_exclusive_scan<uint32_t>(sum, s_scan, &tot);
        for (uint32_t s = s0; s < s1; ++s) { s_cur[s] = base; base += tab.vals[s]; }
        if (threadIdx.x == 0) s_sp = tot;   // the special key's group lies behind the slots'
      }
      lds_barrier();
      for_each_key<NW, BatchOf<NW>::U>(idx_keys, ib, ie, [&](const uint64_t (&k)[NW], uint64_t i) {
        const uint32_t h = place_hash<NW>(k);
        if (pass_of(h, npass) != pass) return;
        const int s = table_find<NW>(tab, k, h);
        // (the entries of a pass number at most ie - ib, so every claimed place lies inside the bucket's part of pos)
        if (s >= 0) { if (tab.vals[s] <= max_occ) pos[ib + atomicAdd(&s_cur[s], 1u)] = (uint32_t)(i - ib); }
        else if (s == -2) { if (*tab.special <= max_occ) pos[ib + atomicAdd(&s_sp, 1u)] = (uint32_t)(i - ib); }
      });
      __syncthreads();   // (drains the stores too: the positions are read back from memory by other lanes of the workgroup)
      for (uint64_t i0 = rb; i0 < re; i0 += blockDim.x) {   // (the same trips for every lane: the wavefront meets below)
        const uint64_t i = i0 + threadIdx.x;
        uint32_t cnt = 0, g = 0;
        uint64_t out = 0;
        if (i < re) {
          uint64_t k[NW];
#pragma unroll
          for (int w = 0; w < NW; ++w) k[w] = recs[i * RW + w];
          const uint32_t h = place_hash<NW>(k);
          if (pass_of(h, npass) == pass) {
            const int s = table_find<NW>(tab, k, h);
            uint32_t c = 0, end = 0;
            if (s >= 0) { c = tab.vals[s]; end = s_cur[s]; } else if (s == -2) { c = *tab.special; end = s_sp; }
            if (c != 0u && c <= max_occ) { cnt = c; g = end - c; out = offsets[recs[i * RW + NW]]; }
          }
        }
        const bool lng = cnt >= kLocateWaveMin;
        if (cnt != 0u && !lng) {
          for (uint32_t j = 0; j < cnt; ++j) {
            const uint64_t e = ib + pos[ib + g + j];
#pragma unroll
            for (int w = 0; w < VW; ++w) values[(out + j) * VW + w] = idx_mvals[e * VW + w];
          }
        }
        unsigned long long m = __ballot(lng);
        while (m) {
          const int src = __ffsll((long long)m) - 1;
          m &= m - 1ull;
          const uint32_t c2 = (uint32_t)__shfl((int)cnt, src, kWave), g2 = (uint32_t)__shfl((int)g, src, kWave);
          const uint64_t o2 = (uint64_t)__shfl((unsigned long long)out, src, kWave);
          for (uint32_t j = lane_id(); j < c2; j += kWave) {
            const uint64_t e = ib + pos[ib + g2 + j];
#pragma unroll
            for (int w = 0; w < VW; ++w) values[(o2 + j) * VW + w] = idx_mvals[e * VW + w];
          }
        }
      }
      __syncthreads();   // (the next pass writes pos again)
    }
    if (!failed) break;
    npass *= 2;
    if (npass > kMaxPasses) { if (threadIdx.x == 0) atomicOr(over_limit, 1u); break; }
    lds_barrier();
  }
  if (threadIdx.x == 0) atomicMax(max_npass, npass > kMaxPasses ? kMaxPasses : npass);
}

// ---- device-wide exclusive scan of in(i), i < n, from `base`: out(i, base + sum of in(j), j < i), and with write_end out(n, the end).
// Tiles of kScanTile values: their sums, one workgroup's running scan over the sums, then every tile again from its base.
constexpr int kScanThreads = 256, kScanItems = 8, kScanTile = kScanThreads * kScanItems;
struct ListedIn {   // listed(i): a key is listed whole or not at all
  const uint32_t *occ; uint32_t max_occ;
  __device__ __forceinline__ uint64_t operator()(uint64_t i) const { const uint32_t c = occ[i]; return c <= max_occ ? c : 0u; }
};
struct OffsetsOut {
  uint64_t *off;
  __device__ __forceinline__ void operator()(uint64_t i, uint64_t v) const { off[i] = v; }
};
struct RowKmersIn {
  const kmi_read_seeds *rows;
  __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return rows[i].n_kmers; }
};
struct RowFirstOut {
  kmi_read_seeds *rows;
  __device__ __forceinline__ void operator()(uint64_t i, uint64_t v) const { rows[i].first_kmer = v; }
};

template <typename In>
__global__ __launch_bounds__(kScanThreads) void scan_tile_sums_kernel(In in, uint64_t n, uint64_t n_tiles, uint64_t *__restrict__ tile_sums) {
  __shared__ uint64_t s_scan[kScanThreads / kWave + 1];
  for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint64_t i0 = t * kScanTile + (uint64_t)threadIdx.x * kScanItems;
    uint64_t sum = 0;
#pragma unroll
    for (int u = 0; u < kScanItems; ++u) if (i0 + u < n) sum += in(i0 + u);
    uint64_t tot = 0;
    (void)block_exclusive_scan<uint64_t>(sum, s_scan, &tot);
    if (threadIdx.x == 0) tile_sums[t] = tot;
  }
}
// tile_sums[t] := base + the sums before t; *end (when asked for) := base + all of them
__global__ __launch_bounds__(1024) void scan_tile_bases_kernel(uint64_t *__restrict__ tile_sums, uint64_t n_tiles, uint64_t base, uint64_t *__restrict__ end) {
  __shared__ uint64_t s_scan[1024 / kWave + 1];
  uint64_t carry = base;
  for (uint64_t t0 = 0; t0 < n_tiles; t0 += 1024) {
    const uint64_t t = t0 + threadIdx.x;
    const uint64_t v = t < n_tiles ? tile_sums[t] : 0ull;
    uint64_t tot = 0;
    const uint64_t ex = block_exclusive_scan<uint64_t>(v, s_scan, &tot);
    if (t < n_tiles) tile_sums[t] = carry + ex;
    carry += tot;
  }
  if (end && threadIdx.x == 0) *end = carry;
}
template <typename In, typename Out>
__global__ __launch_bounds__(kScanThreads) void scan_write_kernel(In in, Out out, uint64_t n, uint64_t n_tiles, const uint64_t *__restrict__ tile_sums,
                                                                 const uint64_t *__restrict__ end, bool write_end) {
  __shared__ uint64_t s_scan[kScanThreads / kWave + 1];
  if (write_end && blockIdx.x == 0 && threadIdx.x == 0) out(n, *end);
  for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint64_t i0 = t * kScanTile + (uint64_t)threadIdx.x * kScanItems;
    uint64_t v[kScanItems], sum = 0;
#pragma unroll
    for (int u = 0; u < kScanItems; ++u) { v[u] = i0 + u < n ? in(i0 + u) : 0ull; sum += v[u]; }
    uint64_t ex = tile_sums[t] + block_exclusive_scan<uint64_t>(sum, s_scan, (uint64_t *)nullptr);
#pragma unroll
    for (int u = 0; u < kScanItems; ++u) { if (i0 + u < n) out(i0 + u, ex); ex += v[u]; }
  }
}

// queued on the stream; *end_dev (a device word, or null) receives base + the sum, which write_end also hands to out(n, .)
template <typename In, typename Out>
static kmi_status device_exclusive_scan(kmi_ctx *ctx, In in, Out out, uint64_t n, uint64_t base, uint64_t *end_dev, bool write_end) {
  const uint64_t n_tiles = (n + kScanTile - 1) / kScanTile;
  void *p;
  KMI_TRY(ws_get(ctx, WS_LOCATE_SCAN, (n_tiles + 1) * sizeof(uint64_t), &p));
  uint64_t *tile_sums = (uint64_t *)p;
  const unsigned blocks = (unsigned)std::min<uint64_t>(n_tiles ? n_tiles : 1, 8192);
  ProfScope ps(ctx, "locate_scan", n);
  if (n_tiles) hipLaunchKernelGGL((scan_tile_sums_kernel<In>), dim3(blocks), dim3(kScanThreads), 0, ctx->stream, in, n, n_tiles, tile_sums);
  hipLaunchKernelGGL(scan_tile_bases_kernel, dim3(1), dim3(1024), 0, ctx->stream, tile_sums, n_tiles, base, end_dev);
  if (n_tiles || write_end)
    hipLaunchKernelGGL((scan_write_kernel<In, Out>), dim3(blocks), dim3(kScanThreads), 0, ctx->stream, in, out, n, n_tiles, (const uint64_t *)tile_sums,
                       (const uint64_t *)end_dev, write_end);
  KMI_HIP(ctx, hipGetLastError());
  return KMI_OK;
}

// the call's pass-limit flag and a device total, behind one synchronisation; the verdict in the words of the other queries
static kmi_status locate_read_total(kmi_ctx *ctx, TotalWord slot, uint64_t *v) {
  uint32_t over = 0;
  KMI_HIP(ctx, hipMemcpyAsync(v, ctx->d_totals + slot, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipMemcpyAsync(&over, ctx->d_flags + FLAG_LOOKUP_OVER, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return over ? lookup_end(ctx) : KMI_OK;   // (lookup_end reads the flag again and gives the verdict)
}

static uint32_t locate_cap(const kmi_ctx *ctx, uint32_t table_cap) {
  uint32_t cap = ctx->lookup_cap ? ctx->lookup_cap : table_cap;
  return cap < 64u ? 64u : (cap > table_cap ? table_cap : cap);
}

// The counting half on n records (key words, tag) with distinct tags below n: occ_dev[tag], offs_dev[0 .. n] from `base`, *end = base +
// the listed hits (synchronises). *part: where the partitioned records lie for the fill (untouched when *partitioned stays false).
template <int NW, int BITS>
static kmi_status locate_count_impl(kmi_index *idx, const uint64_t *recs_dev, size_t n, uint32_t max_occ, uint32_t *occ_dev, uint64_t *offs_dev,
                                    uint64_t base, uint64_t *end, Partitioned *part, bool *partitioned) {
  kmi_ctx *ctx = idx->ctx;
  *partitioned = false;
  if (n && (!idx->has_data || idx->n_entries == 0)) {   // an empty index answers 0 everywhere
    KMI_HIP(ctx, hipMemsetAsync(occ_dev, 0, n * sizeof(uint32_t), ctx->stream));
  } else if (n) {
    KMI_TRY(ensure_dense(idx));   // (a position index is never sparse)
    KMI_TRY((partition_impl<NW, BITS, 1>(ctx, &idx->cfg, idx->shape, recs_dev, n, true, WS_QUERY_A, WS_QUERY_B, part, idx->layout_w)));
    *partitioned = true;
    ProfScope ps(ctx, "bucket_locate_count", n);
    hipLaunchKernelGGL((bucket_locate_count_kernel<NW>), dim3(kNumFine), dim3(QTabCfg<NW>::NT), 0, ctx->stream, (const uint64_t *)part->keys,
                       (const uint64_t *)part->fine_off, (const uint64_t *)idx->keys, (const uint64_t *)idx->bucket_off,
                       locate_cap(ctx, (uint32_t)QTabCfg<NW>::CAP), occ_dev, ctx->d_flags + FLAG_LOOKUP_OVER, ctx->d_flags + FLAG_LOOKUP_NPASS);
    KMI_HIP(ctx, hipGetLastError());
  }
  KMI_TRY(device_exclusive_scan(ctx, ListedIn{occ_dev, max_occ}, OffsetsOut{offs_dev}, (uint64_t)n, base, ctx->d_totals + TOT_LOCATE_HITS, true));
  return locate_read_total(ctx, TOT_LOCATE_HITS, end);
}

// the filling half: values_dev[offs_dev[tag] ...] for the partitioned records of locate_count_impl; queued on the stream
template <int NW, int VW>
static kmi_status locate_fill_vw(kmi_index *idx, const Partitioned &part, size_t n, uint32_t max_occ, const uint64_t *offs_dev, uint64_t *values_dev) {
  kmi_ctx *ctx = idx->ctx;
  void *p;
  KMI_TRY(ws_get(ctx, WS_LOCATE_POS, idx->n_entries * sizeof(uint32_t) + 64, &p));
  ProfScope ps(ctx, "bucket_locate_fill", n);
  hipLaunchKernelGGL((bucket_locate_fill_kernel<NW, VW>), dim3(kNumFine), dim3(LTabCfg<NW>::NT), 0, ctx->stream, (const uint64_t *)part.keys,
                     (const uint64_t *)part.fine_off, (const uint64_t *)idx->keys, (const uint64_t *)idx->mvals, (const uint64_t *)idx->bucket_off,
                     locate_cap(ctx, (uint32_t)LTabCfg<NW>::CAP), max_occ, offs_dev, (uint32_t *)p, values_dev, ctx->d_flags + FLAG_LOOKUP_OVER,
                     ctx->d_flags + FLAG_LOOKUP_NPASS);
  KMI_HIP(ctx, hipGetLastError());
  return KMI_OK;
}
template <int NW>
static kmi_status locate_fill(kmi_index *idx, const Partitioned &part, size_t n, uint32_t max_occ, const uint64_t *offs_dev, uint64_t *values_dev) {
  if (idx->val_words == 1) return locate_fill_vw<NW, 1>(idx, part, n, max_occ, offs_dev, values_dev);
  return locate_fill_vw<NW, 2>(idx, part, n, max_occ, offs_dev, values_dev);
}

template <int NW, int BITS>
static kmi_status locate_impl(kmi_index *idx, const uint64_t *q_dev, size_t nq, uint32_t max_occ, uint32_t *occ_dev, uint64_t *offs_dev,
                              uint64_t *values_dev, size_t capacity, uint64_t *n_hits) {
  kmi_ctx *ctx = idx->ctx;
  KMI_TRY(lookup_begin(ctx));
  void *p;
  KMI_TRY(ws_get(ctx, WS_LOOKUP_RECS, nq * (NW + 1) * sizeof(uint64_t) + 64, &p));
  uint64_t *recs = (uint64_t *)p;
  hipLaunchKernelGGL((lookup_zip_kernel<NW>), dim3(2048), dim3(256), 0, ctx->stream, q_dev, (uint64_t)nq, recs);
  Partitioned part;
  bool partitioned = false;
  KMI_TRY((locate_count_impl<NW, BITS>(idx, recs, nq, max_occ, occ_dev, offs_dev, 0, n_hits, &part, &partitioned)));
  if (!values_dev && capacity == 0) return lookup_end(ctx);   // the sizing call
  if (*n_hits > capacity) { (void)lookup_end(ctx); return set_err(ctx, KMI_ERR_OVERFLOW, "locate: capacity too small"); }
  if (*n_hits && partitioned) KMI_TRY((locate_fill<NW>(idx, part, nq, max_occ, offs_dev, values_dev)));
  return lookup_end(ctx);
}
static kmi_status index_locate(kmi_index *idx, const uint64_t *q_dev, size_t nq, uint32_t max_occ, uint32_t *occ_dev, uint64_t *offs_dev,
                               uint64_t *values_dev, size_t capacity, uint64_t *n_hits) {
  KMI_DISPATCH(idx->shape, locate_impl, idx, q_dev, nq, max_occ, occ_dev, offs_dev, values_dev, capacity, n_hits);
}

// ---- seeds of reads
// one thread per record: where its sequence starts and how many windows it has (the sequence line's length from the scan's EOL
// bitmap, as read_profile_reduce_kernel finds it); first_kmer comes from the scan of n_kmers, the rest from read_seeds_rows_kernel
__global__ __launch_bounds__(256) void read_seeds_len_kernel(const ReadDesc *__restrict__ reads, uint64_t n_reads, const uint32_t *__restrict__ eolw,
                                                            uint64_t n_words, uint64_t n_bytes, uint32_t k, uint64_t byte_base,
                                                            kmi_read_seeds *__restrict__ rows) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * blockDim.x) {
    const ReadDesc rd = reads[r];
    uint64_t seq = n_bytes;
    uint32_t n_win = 0;
    if (rd.seq_pos != ~0ull) {
      seq = rd.seq_pos;
      uint64_t wi = seq >> 5, e1 = n_words * 32;
      if (wi < n_words) {
        uint32_t bits = eolw[wi] & (0xffffffffu << (seq & 31u));
        while (bits == 0u && ++wi < n_words) bits = eolw[wi];
        if (bits) e1 = wi * 32 + (uint32_t)__builtin_ctz(bits);
      }
      e1 = e1 < n_bytes ? e1 : n_bytes;
      const uint64_t len = e1 - seq;
      n_win = len >= k ? (uint32_t)(len - k + 1u) : 0u;
      if (rd.out_off == ~0ull) n_win = 0;   // (never otherwise: the extract pass numbers exactly these windows)
    }
    kmi_read_seeds row;
    row.seq_offset = byte_base + seq; row.first_kmer = 0; row.n_kmers = n_win; row.n_listed = 0u; row.n_hits = 0;
    rows[r] = row;
  }
}
// kProfLanes lanes per read over the batch's occ[] / offsets[] (both indexed from the batch's first window, kmer_base): the windows
// with a listed hit, and the read's hits as the difference of its two ends in offsets[]
__global__ __launch_bounds__(kProfThreads) void read_seeds_rows_kernel(kmi_read_seeds *__restrict__ rows, uint64_t n_reads, uint64_t kmer_base,
                                                                      const uint32_t *__restrict__ occ, const uint64_t *__restrict__ offsets,
                                                                      uint64_t n_kmers, uint32_t max_occ) {
  constexpr uint32_t GROUPS = kProfThreads / kProfLanes;
  const uint32_t grp = threadIdx.x / kProfLanes, gl = threadIdx.x % kProfLanes;
  for (uint64_t r0 = (uint64_t)blockIdx.x * GROUPS; r0 < n_reads; r0 += (uint64_t)gridDim.x * GROUPS) {   // (whole wavefronts reach the shuffles)
    const uint64_t r = r0 + grp;
    uint64_t o = 0;
    uint32_t n_win = 0;
    if (r < n_reads) {
      o = rows[r].first_kmer - kmer_base;
      n_win = rows[r].n_kmers;
      if (o + n_win > n_kmers) n_win = 0;   // (never: the rows' windows are the extract pass's)
    }
    uint32_t listed = 0;
    for (uint32_t w = gl; w < n_win; w += kProfLanes) {
      const uint32_t c = occ[o + w];
      listed += (c != 0u && c <= max_occ) ? 1u : 0u;
    }
#pragma unroll
    for (int d = kProfLanes / 2; d > 0; d >>= 1) listed += (uint32_t)__shfl_xor((int)listed, d, kProfLanes);
    if (gl == 0 && r < n_reads) {
      rows[r].n_listed = listed;
      rows[r].n_hits = n_win ? offsets[o + n_win] - offsets[o] : 0ull;
    }
  }
}

// what one batch leaves in the workspace, and what it adds to the call's totals
struct SeedBatch { kmi_read_seeds *rows; uint32_t *occ; uint64_t *offs; uint64_t n_rec, n_kmers, hits_end; };

// one record-aligned batch (bytes on the device, 16-byte aligned). kmer_base / hit_base: the windows and listed hits of the batches
// before. values_dev (null: counting only) takes the batch's hits when they fit below cap_hits. Synchronises.
template <int NW, int BITS>
static kmi_status seed_batch_impl(kmi_index *idx, const uint8_t *bytes_dev, size_t n_bytes, uint64_t byte_base, uint32_t max_occ, uint64_t kmer_base,
                                  uint64_t hit_base, uint64_t *values_dev, size_t cap_hits, SeedBatch *out) {
  kmi_ctx *ctx = idx->ctx;
  constexpr int RW = NW + 1;
  kmi_config cfg = idx->cfg;
  // the reads are FASTQ whatever the index was built from, every window counts, and the records are (key words, tag): no quality word
  cfg.seq_format = KMI_FMT_FASTQ; cfg.seq_filter = KMI_SEQ_ALL; cfg.index_kind = KMI_INDEX_COUNT;
  uint64_t nt = 0, ns = 0;
  KMI_TRY(extract_count(ctx, &cfg, bytes_dev, n_bytes, &nt, &ns));   // (malformed input is reported here, in the builds' words)
  void *p;
  KMI_TRY(ws_get(ctx, WS_LOOKUP_RECS, (nt ? nt : 1) * RW * sizeof(uint64_t) + 64, &p));
  uint64_t *recs = (uint64_t *)p;
  KMI_TRY(ws_get(ctx, WS_LOOKUP_CNT, (nt ? nt : 1) * sizeof(uint32_t), &p));
  out->occ = (uint32_t *)p;
  KMI_TRY(ws_get(ctx, WS_LOCATE_OFF, (nt + 1) * sizeof(uint64_t), &p));
  out->offs = (uint64_t *)p;
  ReadScan rs{};
  KMI_TRY(extract_run(ctx, &cfg, bytes_dev, n_bytes, 0, recs, nullptr, (size_t)nt, false, true, &nt, &ns, nullptr, (uint32_t)RW, EDGES_NONE, &rs));
  out->n_rec = (rs.n_lines + 3) / 4;   // every header line opens a record
  out->n_kmers = nt;
  KMI_TRY(ws_get(ctx, WS_OUTPUT, (out->n_rec ? out->n_rec : 1) * sizeof(kmi_read_seeds), &p));
  out->rows = (kmi_read_seeds *)p;
  if (nt) hipLaunchKernelGGL((lookup_tag_kernel<NW>), dim3(2048), dim3(256), 0, ctx->stream, recs, nt);
  if (out->n_rec) {
    ProfScope ps(ctx, "read_seeds_len", out->n_rec);
    hipLaunchKernelGGL(read_seeds_len_kernel, dim3((unsigned)std::min<uint64_t>((out->n_rec + 255) / 256, 8192)), dim3(256), 0, ctx->stream, rs.reads,
                       out->n_rec, rs.eolw, rs.n_eol_words, (uint64_t)n_bytes, idx->shape.k, byte_base, out->rows);
    KMI_TRY(device_exclusive_scan(ctx, RowKmersIn{out->rows}, RowFirstOut{out->rows}, out->n_rec, kmer_base, (uint64_t *)nullptr, false));
  }
  Partitioned part;
  bool partitioned = false;
  KMI_TRY((locate_count_impl<NW, BITS>(idx, recs, (size_t)nt, max_occ, out->occ, out->offs, hit_base, &out->hits_end, &part, &partitioned)));
  if (out->n_rec) {
    ProfScope ps(ctx, "read_seeds_rows", nt);
    constexpr uint64_t per_block = kProfThreads / kProfLanes;
    const uint64_t blocks = std::min<uint64_t>((out->n_rec + per_block - 1) / per_block, 8192);
    hipLaunchKernelGGL(read_seeds_rows_kernel, dim3((unsigned)blocks), dim3(kProfThreads), 0, ctx->stream, out->rows, out->n_rec, kmer_base,
                       (const uint32_t *)out->occ, (const uint64_t *)out->offs, nt, max_occ);
  }
  if (values_dev && partitioned && out->hits_end > hit_base && out->hits_end <= cap_hits)
    KMI_TRY((locate_fill<NW>(idx, part, (size_t)nt, max_occ, out->offs, values_dev)));
  KMI_HIP(ctx, hipGetLastError());
  return KMI_OK;
}
static kmi_status seed_batch(kmi_index *idx, const uint8_t *bytes_dev, size_t n_bytes, uint64_t byte_base, uint32_t max_occ, uint64_t kmer_base,
                             uint64_t hit_base, uint64_t *values_dev, size_t cap_hits, SeedBatch *out) {
  KMI_DISPATCH(idx->shape, seed_batch_impl, idx, bytes_dev, n_bytes, byte_base, max_occ, kmer_base, hit_base, values_dev, cap_hits, out);
}

// bytes: on the device (on_device) or on the host; the outputs likewise. Batches of at most ctx->profile_batch bytes; first_kmer and
// offsets of a batch start from what came before, so the arrays are those of one pass over the whole buffer.
static kmi_status index_seed_reads(kmi_index *idx, const uint8_t *bytes, size_t n_bytes, bool on_device, uint32_t max_occ, kmi_read_seeds *rows,
                                   size_t cap_reads, uint32_t *occ, uint64_t *offsets, size_t cap_kmers, uint64_t *values, size_t cap_hits,
                                   uint64_t *n_reads, uint64_t *n_kmers, uint64_t *n_hits) {
  kmi_ctx *ctx = idx->ctx;
  KMI_TRY(lookup_begin(ctx));
  const hipMemcpyKind back = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t vw = idx->val_words;
  uint64_t *values_dev = values;
  if (values && !on_device && cap_hits) {   // the hits of all batches are gathered on the device and copied once
    void *p;
    KMI_TRY(ws_get(ctx, WS_OUTPUT2, cap_hits * vw * sizeof(uint64_t), &p));
    values_dev = (uint64_t *)p;
  }
  uint64_t start = 0, reads_done = 0, kmers_done = 0, hits_done = 0;
  while (start < n_bytes) {
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
    SeedBatch sb{};
    KMI_TRY(seed_batch(idx, b, len, start, max_occ, kmers_done, hits_done, cap_hits ? values_dev : nullptr, cap_hits, &sb));
    // nothing is written past a capacity
    const uint64_t room_r = reads_done < cap_reads ? cap_reads - reads_done : 0, take_r = sb.n_rec < room_r ? sb.n_rec : room_r;
    if (take_r) KMI_HIP(ctx, hipMemcpyAsync(rows + reads_done, sb.rows, take_r * sizeof(kmi_read_seeds), back, ctx->stream));
    const uint64_t room_k = kmers_done < cap_kmers ? cap_kmers - kmers_done : 0, take_k = sb.n_kmers < room_k ? sb.n_kmers : room_k;
    if (take_k) KMI_HIP(ctx, hipMemcpyAsync(occ + kmers_done, sb.occ, take_k * sizeof(uint32_t), back, ctx->stream));
    if (offsets && kmers_done <= cap_kmers)   // (the batch's last word is the next batch's first)
      KMI_HIP(ctx, hipMemcpyAsync(offsets + kmers_done, sb.offs, (take_k + (take_k == sb.n_kmers ? 1 : 0)) * sizeof(uint64_t), back, ctx->stream));
    KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the staging buffers are the next batch's)
    reads_done += sb.n_rec;
    kmers_done += sb.n_kmers;
    hits_done = sb.hits_end;
    start = end;
  }
  *n_reads = reads_done; *n_kmers = kmers_done; *n_hits = hits_done;
  if (n_bytes == 0 && offsets) {
    if (on_device) KMI_HIP(ctx, hipMemsetAsync(offsets, 0, sizeof(uint64_t), ctx->stream)); else offsets[0] = 0;
  }
  KMI_TRY(lookup_end(ctx));
  if (!rows && !occ && !offsets && !values && !cap_reads && !cap_kmers && !cap_hits) return KMI_OK;   // the sizing call
  if (reads_done > cap_reads || kmers_done > cap_kmers || hits_done > cap_hits)
    return set_err(ctx, KMI_ERR_OVERFLOW, "seed_reads: capacity too small");
  if (values && values_dev != values && hits_done) {
    KMI_HIP(ctx, hipMemcpyAsync(values, values_dev, hits_done * vw * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return KMI_OK;
}

}  // namespace kmi
