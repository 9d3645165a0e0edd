// Queries in the caller's order (no counterpart in the reference, whose count() / find() answer once per distinct key, unordered):
//   kmi_index_lookup_*         counts[i] = the count stored for InputTransform(queries[i]), 0 when absent
//   kmi_index_profile_reads_*  one kmi_read_profile row per FASTQ record: how many of the read's k-mers the index holds and how
//                              abundant they are
// Both go through bucket_lookup_kernel: the queries travel as (key words, tag) records through the partition the other queries
// use, every fine bucket's workgroup builds an LDS table from the bucket's index ENTRIES -- distinct by construction, so the
// table's fill is known before it is built and nothing has to be deduplicated -- and streams the bucket's query records against
// it once per pass: counts[tag] = value. (The query kernel's table of distinct QUERY keys would have to read a bucket's queries
// twice, once to build and once more to answer each occurrence, and a profile asks about every k-mer of its reads: far more
// queries than entries.) The profile extracts a record-aligned batch in file order, tags k-mer t with t, looks the batch up and
// reduces counts[] per read (read_profile_reduce_kernel) from the read descriptors of the extract pass.
//
// Included by kmi_index.hip after kmi_update.h.
#pragma once

namespace kmi {

// records of the queries: (key words, position in the input)
template <int NW>
__global__ __launch_bounds__(256) void lookup_zip_kernel(const uint64_t *__restrict__ q, uint64_t n, uint64_t *__restrict__ recs) {
  constexpr int RW = NW + 1;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int w = 0; w < NW; ++w) recs[i * RW + w] = q[i * NW + w];
    recs[i * RW + NW] = i;
  }
}
// value word of the extract pass's records (the position id) := file-order index of the k-mer
template <int NW>
__global__ __launch_bounds__(256) void lookup_tag_kernel(uint64_t *__restrict__ recs, uint64_t n) {
  constexpr int RW = NW + 1;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) recs[i * RW + NW] = i;
}

// Fine bucket b: table of the bucket's entries (key -> count), then counts[tag] for every query record of the bucket. A bucket of
// more entries than the table takes runs in passes by pass_of(place_hash), entries and queries alike: a query is answered in the
// pass its hash belongs to, hit or miss, so every counts[] word is written exactly once per attempt and needs no clearing. The
// entries are distinct, so an attempt with fewer than entries / limit passes cannot fit and is not tried; from there npass doubles.
// cap_limit: home slots at most (KMI_LOOKUP_CAP); idx_cnt: sparse index (bucket b = idx_cnt[b] entries from idx_off[b]).
template <int NW>
__global__ __launch_bounds__((QTabCfg<NW>::NT)) void bucket_lookup_kernel(const uint64_t *__restrict__ recs, const uint64_t *__restrict__ rec_off,
                                                                        const uint64_t *__restrict__ idx_keys, const uint32_t *__restrict__ idx_vals,
                                                                        const uint64_t *__restrict__ idx_off, const uint32_t *__restrict__ idx_cnt,
                                                                        uint32_t cap_limit, uint32_t *__restrict__ counts, uint32_t *__restrict__ over_limit,
                                                                        uint32_t *__restrict__ max_npass) {
  KMI_TABLE_LDS_CFG(NW, QTabCfg<NW>)
  constexpr int RW = NW + 1;
  const uint32_t b = blockIdx.x;
  const uint64_t rb = rec_off[b], re = rec_off[b + 1];
  if (rb == re) return;
  const uint64_t ib = idx_off[b], ie = idx_cnt ? ib + idx_cnt[b] : idx_off[b + 1];
  if (ib == ie) {
    for (uint64_t i = rb + threadIdx.x; i < re; i += blockDim.x) counts[recs[i * RW + NW]] = 0u;
    return;
  }
  {
    // twice the bucket's entries of home slots, at least 512, at most what the knob allows
    uint32_t want = 2u * (uint32_t)((ie - ib) < (uint64_t)QTabCfg<NW>::CAP ? (ie - ib) : (uint64_t)QTabCfg<NW>::CAP);
    want = (want + 255u) & ~255u;
    want = want < 512u ? 512u : want;
    want = want < cap_limit ? want : cap_limit;
    if (want < (uint32_t)QTabCfg<NW>::CAP) { tab.cap = want; tab.slots = want + QTabCfg<NW>::PAD; tab.limit = want * 3u / 4u; }
  }
  uint32_t npass = 1;
  while ((uint64_t)npass * tab.limit < ie - ib && npass < kMaxPasses) npass *= 2;
  while (true) {
    bool failed = false;
    for (uint32_t pass = 0; pass < npass && !failed; ++pass) {
      table_clear<NW>(tab);
      lds_barrier();
      for_each_key<NW, BatchOf<NW>::U>(idx_keys, ib, ie, [&](const uint64_t (&k)[NW], uint64_t i) {
        const uint32_t h = place_hash<NW>(k);
        if (pass_of(h, npass) != pass) return;
        const int s = table_upsert<NW>(tab, k, h);
        if (s >= 0) tab.vals[s] = idx_vals[i]; else if (s == -2) *tab.special = idx_vals[i];
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
        counts[tag] = s >= 0 ? tab.vals[s] : (s == -2 ? *tab.special : 0u);
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

// Per read: the looked-up counts of its windows, counts[out_off, out_off + n_kmers), reduced to one row. kProfLanes lanes per read:
// a 150-base read has about 120 windows, which sixteen lanes cover in eight steps of one 64-byte line each with 94 % of the lanes
// at work (a whole wavefront would idle half its lanes in the second of two steps and spend the descriptor and bitmap reads of
// a read on all 64 of them), and the reduction is four shuffle steps inside the group. n_kmers is the sequence line's length from
// the scan's EOL bitmap (KMI_SEQ_ALL: every window of the line is a k-mer), so a read without a k-mer gets its row like any other.
constexpr int kProfLanes = 16;
constexpr int kProfThreads = 256;
__global__ __launch_bounds__(kProfThreads) void read_profile_reduce_kernel(const ReadDesc *__restrict__ reads, uint64_t n_reads,
                                                                          const uint32_t *__restrict__ eolw, uint64_t n_words, uint64_t n_bytes,
                                                                          uint32_t k, const uint32_t *__restrict__ counts, uint64_t n_counts,
                                                                          uint32_t solid, uint64_t byte_base, kmi_read_profile *__restrict__ out) {
  constexpr uint32_t GROUPS = kProfThreads / kProfLanes;
  const uint32_t grp = threadIdx.x / kProfLanes, gl = threadIdx.x % kProfLanes;
  // the loop bound is the same for every lane of a workgroup, so the shuffles below are reached by whole wavefronts
  for (uint64_t r0 = (uint64_t)blockIdx.x * GROUPS; r0 < n_reads; r0 += (uint64_t)gridDim.x * GROUPS) {
    const uint64_t r = r0 + grp;
    uint64_t seq = n_bytes, o = ~0ull;
    uint32_t n_win = 0;
    if (r < n_reads) {
      const ReadDesc rd = reads[r];
      o = rd.out_off;
      if (rd.seq_pos != ~0ull) {
        seq = rd.seq_pos;
        // end of the sequence line: the first EOL bit at or behind seq_pos (everything past the bitmap is EOL)
        uint64_t wi = seq >> 5, e1 = n_words * 32;
        if (wi < n_words) {
          uint32_t bits = eolw[wi] & (0xffffffffu << (seq & 31u));
          while (bits == 0u && ++wi < n_words) bits = eolw[wi];
          if (bits) e1 = wi * 32 + (uint32_t)__builtin_ctz(bits);
        }
        e1 = e1 < n_bytes ? e1 : n_bytes;
        const uint64_t len = e1 - seq;
        n_win = len >= k ? (uint32_t)(len - k + 1u) : 0u;
        if (o == ~0ull || o + n_win > n_counts) n_win = 0;   // (never: the extract pass numbers exactly these windows)
      }
    }
    uint64_t sum = 0;
    uint32_t present = 0, nsolid = 0, lo = 0xffffffffu, hi = 0;
    for (uint32_t w = gl; w < n_win; w += kProfLanes) {
      const uint32_t c = counts[o + w];
      sum += c; present += c ? 1u : 0u; nsolid += c >= solid ? 1u : 0u;
      lo = c < lo ? c : lo; hi = c > hi ? c : hi;
    }
#pragma unroll
    for (int d = kProfLanes / 2; d > 0; d >>= 1) {
      sum += (uint64_t)__shfl_xor((unsigned long long)sum, d, kProfLanes);
      present += (uint32_t)__shfl_xor((int)present, d, kProfLanes);
      nsolid += (uint32_t)__shfl_xor((int)nsolid, d, kProfLanes);
      const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, d, kProfLanes), h2 = (uint32_t)__shfl_xor((int)hi, d, kProfLanes);
      lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
    }
    if (gl == 0 && r < n_reads) {
      kmi_read_profile row;
      row.seq_offset = byte_base + seq; row.sum_counts = sum; row.n_kmers = n_win; row.n_present = present; row.n_solid = nsolid;
      row.lowest = n_win ? lo : 0u; row.highest = hi; row.reserved = 0u;
      out[r] = row;
    }
  }
}

static kmi_status lookup_begin(kmi_ctx *ctx) {
  ctx->lookup_npass = 0;
  // FLAG_LOOKUP_NPASS: the largest pass count of the call's buckets; FLAG_LOOKUP_OVER: a bucket went over the pass limit (words of their own: the scan of
  // every batch of a profile clears the low flag words)
  KMI_HIP(ctx, hipMemsetAsync(ctx->d_flags + FLAG_LOOKUP_NPASS, 0, 2 * sizeof(uint32_t), ctx->stream));
  return KMI_OK;
}
// waits for the call's work; the pass-limit verdict, reported as the other queries report it
static kmi_status lookup_end(kmi_ctx *ctx) {
  uint32_t f[2] = {0, 0};
  KMI_HIP(ctx, hipMemcpyAsync(f, ctx->d_flags + FLAG_LOOKUP_NPASS, sizeof(f), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->lookup_npass = f[0];
  if (f[1]) {
    return set_err(ctx, KMI_ERR_OVERFLOW, "a bucket could not be looked up within the pass limit");
  }
  return KMI_OK;
}

// counts_dev[tag] for n records (key words, tag) with distinct tags below the size of counts_dev; queued on the stream
template <int NW, int BITS>
static kmi_status lookup_records_impl(kmi_index *idx, const uint64_t *recs_dev, size_t n, uint32_t *counts_dev) {
  kmi_ctx *ctx = idx->ctx;
  if (n == 0) return KMI_OK;
  if (!idx->has_data || idx->n_entries == 0) {   // an empty index answers 0 everywhere
    KMI_HIP(ctx, hipMemsetAsync(counts_dev, 0, n * sizeof(uint32_t), ctx->stream));
    return KMI_OK;
  }
  Partitioned part;
  KMI_TRY((partition_impl<NW, BITS, 1>(ctx, &idx->cfg, idx->shape, recs_dev, n, true, WS_QUERY_A, WS_QUERY_B, &part, idx->layout_w)));
  uint32_t cap = ctx->lookup_cap ? ctx->lookup_cap : (uint32_t)QTabCfg<NW>::CAP;
  cap = cap < 64u ? 64u : (cap > (uint32_t)QTabCfg<NW>::CAP ? (uint32_t)QTabCfg<NW>::CAP : cap);
  {
    ProfScope ps(ctx, "bucket_lookup", n);
    hipLaunchKernelGGL((bucket_lookup_kernel<NW>), dim3(kNumFine), dim3(QTabCfg<NW>::NT), 0, ctx->stream, (const uint64_t *)part.keys,
                       (const uint64_t *)part.fine_off, (const uint64_t *)idx->keys, (const uint32_t *)idx->vals, (const uint64_t *)idx->bucket_off,
                       (const uint32_t *)idx->bucket_cnt, cap, counts_dev, ctx->d_flags + FLAG_LOOKUP_OVER, ctx->d_flags + FLAG_LOOKUP_NPASS);
  }
  KMI_HIP(ctx, hipGetLastError());
  return KMI_OK;
}

template <int NW, int BITS>
static kmi_status lookup_impl(kmi_index *idx, const uint64_t *q_dev, size_t nq, uint32_t *counts_dev) {
  kmi_ctx *ctx = idx->ctx;
  KMI_TRY(lookup_begin(ctx));
  void *p;
  KMI_TRY(ws_get(ctx, WS_LOOKUP_RECS, nq * (NW + 1) * sizeof(uint64_t) + 64, &p));
  uint64_t *recs = (uint64_t *)p;
  hipLaunchKernelGGL((lookup_zip_kernel<NW>), dim3(2048), dim3(256), 0, ctx->stream, q_dev, (uint64_t)nq, recs);
  KMI_TRY((lookup_records_impl<NW, BITS>(idx, recs, nq, counts_dev)));
  return lookup_end(ctx);
}
static kmi_status index_lookup(kmi_index *idx, const uint64_t *q_dev, size_t nq, uint32_t *counts_dev) {
  KMI_DISPATCH(idx->shape, lookup_impl, idx, q_dev, nq, counts_dev);
}

// one record-aligned batch (bytes on the device, 16-byte aligned): its rows into WS_OUTPUT, *n_rec of them; queued on the stream
template <int NW, int BITS>
static kmi_status profile_batch_impl(kmi_index *idx, const uint8_t *bytes_dev, size_t n_bytes, uint64_t byte_base, uint32_t solid,
                                     kmi_read_profile **rows, uint64_t *n_rec) {
  kmi_ctx *ctx = idx->ctx;
  constexpr int RW = NW + 1;
  kmi_config cfg = idx->cfg;
  cfg.seq_filter = KMI_SEQ_ALL;   // the windows are those of kmi_extract_dev with KMI_SEQ_ALL, whatever the index was built with
  uint64_t nt = 0, ns = 0;
  KMI_TRY(extract_count(ctx, &cfg, bytes_dev, n_bytes, &nt, &ns));   // (malformed input is reported here, in the builds' words)
  void *p;
  KMI_TRY(ws_get(ctx, WS_LOOKUP_RECS, (nt ? nt : 1) * RW * sizeof(uint64_t) + 64, &p));
  uint64_t *recs = (uint64_t *)p;
  KMI_TRY(ws_get(ctx, WS_LOOKUP_CNT, (nt ? nt : 1) * sizeof(uint32_t), &p));
  uint32_t *counts = (uint32_t *)p;
  ReadScan rs{};
  KMI_TRY(extract_run(ctx, &cfg, bytes_dev, n_bytes, 0, recs, nullptr, (size_t)nt, false, true, &nt, &ns, nullptr, (uint32_t)RW, EDGES_NONE, &rs));
  *n_rec = (rs.n_lines + 3) / 4;   // every header line opens a record
  KMI_TRY(ws_get(ctx, WS_OUTPUT, (*n_rec ? *n_rec : 1) * sizeof(kmi_read_profile), &p));
  *rows = (kmi_read_profile *)p;
  if (nt) {
    hipLaunchKernelGGL((lookup_tag_kernel<NW>), dim3(2048), dim3(256), 0, ctx->stream, recs, nt);
    KMI_TRY((lookup_records_impl<NW, BITS>(idx, recs, (size_t)nt, counts)));
  }
  if (*n_rec) {
    ProfScope ps(ctx, "read_profile_reduce", nt);
    constexpr uint64_t per_block = kProfThreads / kProfLanes;
    const uint64_t blocks = std::min<uint64_t>((*n_rec + per_block - 1) / per_block, 8192);
    hipLaunchKernelGGL(read_profile_reduce_kernel, dim3((unsigned)blocks), dim3(kProfThreads), 0, ctx->stream, rs.reads, *n_rec, rs.eolw,
                       rs.n_eol_words, (uint64_t)n_bytes, idx->shape.k, (const uint32_t *)counts, nt, solid, byte_base, *rows);
  }
  KMI_HIP(ctx, hipGetLastError());
  return KMI_OK;
}
static kmi_status profile_batch(kmi_index *idx, const uint8_t *bytes_dev, size_t n_bytes, uint64_t byte_base, uint32_t solid, kmi_read_profile **rows,
                                uint64_t *n_rec) {
  KMI_DISPATCH(idx->shape, profile_batch_impl, idx, bytes_dev, n_bytes, byte_base, solid, rows, n_rec);
}

// bytes: on the device (on_device) or on the host; out likewise. Batches of at most ctx->profile_batch bytes, so the workspace is
// that of one batch whatever the input's size.
static kmi_status index_profile_reads(kmi_index *idx, const uint8_t *bytes, size_t n_bytes, bool on_device, uint32_t solid, kmi_read_profile *out,
                                      size_t capacity, uint64_t *n_reads) {
  kmi_ctx *ctx = idx->ctx;
  KMI_TRY(lookup_begin(ctx));
  uint64_t start = 0, done = 0;
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
    kmi_read_profile *rows = nullptr;
    uint64_t n_rec = 0;
    KMI_TRY(profile_batch(idx, b, len, start, solid, &rows, &n_rec));
    const uint64_t room = done < capacity ? capacity - done : 0, take = n_rec < room ? n_rec : room;   // nothing is written past capacity
    if (take) KMI_HIP(ctx, hipMemcpyAsync(out + done, rows, take * sizeof(kmi_read_profile), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    if (!on_device) KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the staging buffers are the next batch's)
    done += n_rec;
    start = end;
  }
  *n_reads = done;
  KMI_TRY(lookup_end(ctx));
  if (done > capacity) return set_err(ctx, KMI_ERR_OVERFLOW, "profile_reads: capacity too small");
  return KMI_OK;
}

}  // namespace kmi
