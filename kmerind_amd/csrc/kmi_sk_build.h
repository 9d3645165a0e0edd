// kmi_sk_build.h -- the host driver of the super-k-mer build (included into kmi_index.hip behind the partition and reduce code):
// which indexes take the path and with which window, the two front ends and the door in front of them, the back end, the two
// halves of a build over ranks. The kernels are in kmi_superkmer.h and kmi_front.h.
#pragma once

namespace kmi {

// ---- which W: the one place where the window widths of sk_window_of are enumerated on the host
template <typename Fn>
static kmi_status sk_dispatch_w(uint32_t w, Fn &&fn) {   // sk_dispatch_w(w, [&](auto W) { return f<W>(...); })
  switch (w) {
    case 19: return fn(std::integral_constant<int, 19>{});
    case 13: return fn(std::integral_constant<int, 13>{});
    case 11: return fn(std::integral_constant<int, 11>{});
    default: return fn(std::integral_constant<int, 7>{});
  }
}

// ---- which indexes: the window width of the super-k-mer paths for this index, or 0 (they do not apply).
// SK_ANY_FORMAT: the shape and the context alone -- the layout of the entries (preferred_layout) and the FASTA build;
// SK_FASTQ: the builds from FASTQ bytes, on one rank and over ranks; SK_FASTQ_ONE_PASS: the one-pass front end must be allowed as
// well (the de Bruijn node build: only sk_front_kernel makes edge records)
enum SkInput { SK_ANY_FORMAT, SK_FASTQ, SK_FASTQ_ONE_PASS };
static uint32_t sk_width_of_shape(const KShape &s) { return (s.n_words == 1 && s.bits == 2) ? sk_window_of(s.k) : 0u; }
static uint32_t sk_width(const kmi_index *idx, SkInput in) {
  const kmi_ctx *ctx = idx->ctx;
  if (idx->val_words != 0 || !ctx->fused_superkmer) return 0u;
  if (in != SK_ANY_FORMAT && idx->cfg.seq_format != KMI_FMT_FASTQ) return 0u;
  if (in == SK_FASTQ_ONE_PASS && !ctx->front_fused) return 0u;
  return sk_width_of_shape(idx->shape);
}
static uint32_t sk_width_of(const kmi_index *idx) { return sk_width(idx, SK_FASTQ); }
// the layout a count index of this configuration is kept in when it has the choice (split / merge between ranks agree on it):
// whatever the input format -- the layout is a property of the entries, and a FASTA build leaves them the same way
static uint32_t preferred_layout(const kmi_index *idx) { return sk_width(idx, SK_ANY_FORMAT); }
static bool sk_rank_count(uint32_t p) { return p == 1u || p == 2u || p == 4u || p == 8u; }

// ---- the workspace every stage shares: per-workgroup histograms and cursors of the coarse groups, and three arrays of kNumCoarse
struct SkGroupWs {
  uint32_t *wg_hist;            // [kPartGroups][kNumCoarse] (WS_WGHIST)
  uint64_t *wg_off;             // [kPartGroups][kNumCoarse] (WS_CURSOR)
  uint64_t *cnt, *base, *cend;  // [kNumCoarse] each (WS_MISC): records, start and end of every group
};
static kmi_status sk_group_ws(kmi_ctx *ctx, SkGroupWs *g) {
  void *p;
  KMI_TRY(ws_get(ctx, WS_WGHIST, sizeof(uint32_t) * kPartGroups * kNumCoarse, &p)); g->wg_hist = (uint32_t *)p;
  KMI_TRY(ws_get(ctx, WS_CURSOR, sizeof(uint64_t) * kPartGroups * kNumCoarse, &p)); g->wg_off = (uint64_t *)p;
  KMI_TRY(ws_get(ctx, WS_MISC, sizeof(uint64_t) * kNumCoarse * 3, &p)); g->cnt = (uint64_t *)p; g->base = g->cnt + kNumCoarse; g->cend = g->base + kNumCoarse;
  return KMI_OK;
}

// Index::build_* on one rank through super-k-mers (kmi_superkmer.h): FASTQ, one-word 2-bit k-mers, k >= 17.
// The super-k-mer build in two halves, so that a build over several ranks can put its exchange between them.
// Front end: FASTQ scan -> window runs -> minimizer items -> 16-byte records grouped by the top 8 bucket bits (WS_KEYS_A),
// the groups of workgroup g at wg_off[g][c]. h_cnt / h_base: records and start of every group.
struct SkFront {
  bool ok = false;                 // false: a run or a tile exceeded its item capacity (the caller takes the k-mer path)
  uint64_t *recs = nullptr;        // WS_KEYS_A
  uint64_t n_records = 0, n_kmers = 0, n_seqs = 0;
  uint64_t h_cnt[kNumCoarse], h_base[kNumCoarse];
  uint64_t *wg_off = nullptr;      // [kPartGroups][kNumCoarse] (WS_CURSOR)
};

template <int W>
static kmi_status sk_front_end(kmi_ctx *ctx, const kmi_config *cfg, const KShape &shape, const FastqScan &sc, uint32_t lp, SkFront *f,
                               uint64_t *out = nullptr, size_t out_cap = 0 /* records: the caller's buffer takes them when they fit */,
                               const FastaScan *fa = nullptr /* FASTA: the compacted character stream instead of the FASTQ scan */) {
  constexpr int NW = 1, BITS = 2;
  f->ok = false;
  uint64_t n = fa ? 0 : sc.n_tuples;   // (FASTA: the run pass counts the windows)
  const uint64_t n_tiles = fa ? (fa->n_chars + 8191) / 8192 : sc.n_tiles;
  const uint32_t k = shape.k;
  PackedInput in;
  if (fa) { in.eol = fa->pk_break; in.stream = fa->pk_stream; in.n_bytes = fa->n_chars; in.n_cover = fa->n_cover; in.n_valid = fa->n_valid; in.brk = nullptr; }
  else { in.eol = sc.pk_eol; in.stream = sc.pk_stream; in.n_bytes = sc.n_bytes; in.n_cover = sc.n_cover; in.n_valid = sc.n_bytes; in.brk = sc.pk_brk; }
  const bool split = !fa && sc.pk_brk != nullptr;
  const bool canonical = cfg->strand != KMI_STRAND_SINGLE;
  using LP = ListPassCfg<NW, BITS>;
  // (a tile of the compacted FASTA stream is all windows: 8192 of them against the 3100 of a FASTQ tile -- twice the item slots)
  const uint32_t seg = sk_segment_of((uint32_t)W), ipt = sk_items_per_tile((uint32_t)W) * (fa ? 2u : 1u);
  const uint32_t stride = fa ? 8192u / seg + 72u : LP::run_stride(k, seg, split);
  void *p;
  KMI_TRY(ws_get(ctx, WS_ENT_LIST, sizeof(uint32_t) * ((size_t)n_tiles * stride + 64), &p)); uint32_t *ent = (uint32_t *)p;
  KMI_TRY(ws_get(ctx, WS_ENT_CNT, sizeof(uint32_t) * (n_tiles + 8), &p)); uint32_t *ent_cnt = (uint32_t *)p;
  KMI_TRY(ws_get(ctx, WS_ENT_BKT, sizeof(uint32_t) * ((size_t)n_tiles * stride + 64), &p)); uint32_t *run_items = (uint32_t *)p;
  KMI_TRY(ws_get(ctx, WS_SK_ITEMS, sizeof(uint32_t) * ((size_t)n_tiles * ipt + 64), &p)); uint32_t *items = (uint32_t *)p;
  SkGroupWs g;
  KMI_TRY(sk_group_ws(ctx, &g));
  KMI_HIP(ctx, hipMemsetAsync(ctx->d_flags + FLAG_SK_DECLINED, 0, sizeof(uint32_t), ctx->stream));
  if (fa) {
    ProfScope ps(ctx, "fasta_runs", fa->n_chars);
    KMI_HIP(ctx, hipMemsetAsync(ctx->d_totals + TOT_SK_KMERS, 0, sizeof(uint64_t), ctx->stream));
    hipLaunchKernelGGL(fasta_runs_kernel, dim3(2048), dim3(256), 0, ctx->stream, reinterpret_cast<const uint32_t *>(fa->pk_break), fa->n_chars, fa->n_valid,
                       fa->n_cover, n_tiles, k, seg, ent, ent_cnt, stride, (unsigned long long *)(ctx->d_totals + TOT_SK_KMERS), ctx->d_flags);
  } else {
    ProfScope ps(ctx, "fastq_list", n);
    const uint32_t wave_lds = LP::wave_lds_bytes(k, split);
    hipLaunchKernelGGL((fastq_list_kernel<NW, BITS, true>), dim3(kListGroups), dim3(kListThreads), wave_lds * (kListThreads / kWave), ctx->stream, in,
                       n_tiles, k, LP::max_runs(k, split), wave_lds, sc.line_base, ctx->d_flags, (void *)ent, ent_cnt, stride, seg);
  }
  {
    ProfScope ps(ctx, "sk_minimizer", n);
    hipLaunchKernelGGL((sk_minimizer_kernel<W>), dim3(kPartGroups), dim3(kSkThreads), 0, ctx->stream, in, n_tiles, k, (const uint32_t *)ent,
                       (const uint32_t *)ent_cnt, stride, ipt, items, run_items, g.wg_hist, ctx->d_flags);
  }
  {
    ProfScope ps(ctx, "sk_offsets", kNumCoarse);
    launch_rank_offsets(ctx->stream, (const uint32_t *)g.wg_hist, (uint32_t)kPartGroups, (uint32_t)kNumCoarse, g.cnt, g.base, g.wg_off);
  }
  KMI_HIP(ctx, hipGetLastError());
  uint64_t h_cnt[2 * kNumCoarse];
  uint32_t h_flags[FLAG_SK_DECLINED + 1] = {0};
  KMI_HIP(ctx, hipMemcpyAsync(h_cnt, g.cnt, sizeof(uint64_t) * 2 * kNumCoarse, hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipMemcpyAsync(h_flags, ctx->d_flags, sizeof(h_flags), hipMemcpyDeviceToHost, ctx->stream));
  if (fa) KMI_HIP(ctx, hipMemcpyAsync(&n, ctx->d_totals + TOT_SK_KMERS, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // the seq / qual length rule rode on the list pass (FLAG_PARSE, bit 2: fastq_length_verdict's): the index stays as it was on a parse error
  if (!fa && (h_flags[FLAG_PARSE] & 4u)) return fastq_length_verdict(ctx);
  const uint32_t h_flag = h_flags[FLAG_SK_DECLINED];
  if (h_flag) return KMI_OK;              // a run with more items than a lane's list holds, or a tile with more than its share
  uint64_t R = 0;
  for (int c = 0; c < kNumCoarse; ++c) { R += h_cnt[c]; f->h_cnt[c] = h_cnt[c]; f->h_base[c] = h_cnt[kNumCoarse + c]; }
  uint64_t *rec_a = out;
  if (!out || R + 64 > out_cap) { KMI_TRY(ws_get(ctx, WS_KEYS_A, (R + 64) * 16, &p)); rec_a = (uint64_t *)p; }   // (64 records of slack behind the last one)
  {
    ProfScope ps(ctx, "sk_scatter", n);
#define KMI_SK_SCATTER(CANON)                                                                                                          \
    hipLaunchKernelGGL(sk_scatter_kernel<CANON>, dim3(kPartGroups), dim3(kSkThreads), 0, ctx->stream, in, n_tiles, k, (const uint32_t *)ent, \
                       (const uint32_t *)ent_cnt, stride, ipt, (const uint32_t *)items, (const uint32_t *)run_items, (const uint64_t *)g.wg_off, rec_a, lp)
    if (canonical) KMI_SK_SCATTER(true); else KMI_SK_SCATTER(false);
#undef KMI_SK_SCATTER
  }
  KMI_HIP(ctx, hipGetLastError());
  f->ok = true; f->recs = rec_a; f->n_records = R; f->n_kmers = n; f->wg_off = g.wg_off;
  return KMI_OK;
}

// a build from host memory whose bytes have not been copied yet (kmi_index_build_host): whoever is about to read the input on the
// context's stream and is not the one-pass front end (which feeds itself, chunk by chunk) queues the whole copy first
static kmi_status feed_flush(kmi_ctx *ctx) {
  if (!ctx->feed_host) return KMI_OK;
  const uint8_t *h = ctx->feed_host;
  ctx->feed_host = nullptr;
  KMI_HIP(ctx, hipMemcpyAsync(ctx->feed_dev, h, ctx->feed_bytes, hipMemcpyHostToDevice, ctx->stream));
  return KMI_OK;
}

// ---- diagnostics of the one-pass front end (timing builds and KMI_FRONT_DEBUG), out of the way of the launch order
static void sk_front_report_clocks(kmi_ctx *ctx) {
#ifdef KMI_FR_TIMING
  unsigned long long t[8];
  hipStreamSynchronize(ctx->stream);
  hipMemcpy(t, ctx->d_flags + FLAG_CLOCKS, sizeof(t), hipMemcpyDeviceToHost);
  fprintf(stderr, "sk_front wave clocks: wait-bytes %llu  eol %llu  lines %llu  load+pack %llu  walk %llu  final %llu  copy-out %llu  rest %llu\n", t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
  hipMemset(ctx->d_flags + FLAG_CLOCKS, 0, sizeof(t));
#endif
}
// when the wavefronts of the (last) launch left the kernel, against the first one's entry: the spread is what a SIMD spends with
// fewer than its three wavefronts. By SIMD (a workgroup's wavefront w runs on SIMD w) and by workgroup order (the three
// workgroups of a CU are its first, second and third arrival: the oldest wavefront of a SIMD is issued first).
static void sk_front_report_leave(kmi_ctx *ctx, bool fed, uint32_t front_launched_waves) {
#ifdef KMI_FR_LEAVE
  hipStreamSynchronize(ctx->stream);
  if (fed) return;
  const uint32_t nw = std::min<uint32_t>(front_launched_waves, kFrTimingWaves);
  std::vector<unsigned long long> wc(2 * (size_t)nw);
  hipMemcpyFromSymbol(wc.data(), HIP_SYMBOL(g_fr_wave_clock), sizeof(unsigned long long) * wc.size());
  unsigned long long first = ~0ull;
  for (uint32_t i = 0; i < nw; ++i) first = std::min(first, wc[2 * i]);
  std::vector<double> leave(nw);
  double by_simd[kFrWaves] = {0}, by_third[3] = {0}, enter_third[3] = {0}; uint32_t n_third[3] = {0};
  for (uint32_t i = 0; i < nw; ++i) {
    leave[i] = (double)(wc[2 * i + 1] - first) * 0.01;   // the wall clock counts at 100 MHz: microseconds
    by_simd[i % kFrWaves] += leave[i] / (nw / kFrWaves);
    const uint32_t th = (uint32_t)((uint64_t)i * 3u / nw);
    by_third[th] += leave[i]; enter_third[th] += (double)(wc[2 * i] - first) * 0.01; ++n_third[th];
  }
  std::vector<double> so(leave);
  std::sort(so.begin(), so.end());
  double mean = 0; for (double v : so) mean += v / nw;
  fprintf(stderr, "sk_front wavefronts leave (us after the first entry): n %u  min %.1f  median %.1f  mean %.1f  max %.1f  | by SIMD %.1f %.1f %.1f %.1f"
                  "  | by workgroup third: leave %.1f %.1f %.1f  enter %.1f %.1f %.1f\n", nw, so[0], so[nw / 2], mean, so[nw - 1], by_simd[0], by_simd[1],
          by_simd[2], by_simd[3], by_third[0] / n_third[0], by_third[1] / n_third[1], by_third[2] / n_third[2], enter_third[0] / n_third[0],
          enter_third[1] / n_third[1], enter_third[2] / n_third[2]);
#endif
}
static void sk_front_report_decline(kmi_ctx *ctx) {
  if (!getenv("KMI_FRONT_DEBUG")) return;
  uint32_t why = 0;
  (void)hipMemcpy(&why, ctx->d_flags + FLAG_SK_WHY, sizeof(why), hipMemcpyDeviceToHost);
  fprintf(stderr, "sk_front declined: reasons 0x%x (2 first byte, 4 crowded lines, 8 inference, 16 marker / length, 32 run queue, 64 run capacity, 128 items per run, 256 item capacity, 512 / 1024 edge records: a read of several runs / a base that is not A C G T; 0 = the chain of line indices)\n", why);
}

// The same front end in one pass over the bytes (kmi_front.h): FASTQ without a sequence filter. *took = false: the fast path
// declined (a shape it does not take, or something in the input it is not sure about) and nothing was changed -- the caller
// runs fastq_scan + sk_front_end, which also words parse errors.
template <int W>
static kmi_status sk_front_fast(kmi_ctx *ctx, const kmi_config *cfg, const KShape &shape, const uint8_t *bytes_dev, size_t n_bytes, uint32_t lp, SkFront *f,
                                bool *took, uint64_t *out = nullptr, size_t out_cap = 0) {
  *took = false;
  f->ok = false;
  const bool fed = ctx->feed_host != nullptr && bytes_dev == ctx->feed_dev && n_bytes == ctx->feed_bytes;
  if (!fed) KMI_TRY(feed_flush(ctx));
  if (!ctx->front_fused || cfg->seq_format != KMI_FMT_FASTQ || cfg->seq_filter != KMI_SEQ_ALL || n_bytes < 64) return feed_flush(ctx);
  const uint32_t k = shape.k;
  const bool canonical = cfg->strand != KMI_STRAND_SINGLE;
  // ranges: one per resident wavefront of the front kernel when the input is large; never below the context's minimum
  if (!ctx->front_waves) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sk_front_kernel<19, false>, kFrThreads, 0) != hipSuccess || per_cu <= 0) per_cu = 2;
    ctx->front_waves = (uint32_t)per_cu * (ctx->n_cus ? ctx->n_cus : 256u) * (uint32_t)kFrWaves;
  }
  // Several ranges per wavefront: the kernel is launched with the resident wavefronts and they take their ranges from a queue,
  // so a SIMD keeps its three wavefronts busy until the input runs out (with one range each the oldest wavefront of a SIMD, which
  // is issued first, left long before the youngest). A range pays for its start (the inferred line index) and its end (it scans
  // on in whole steps until two lines behind its last byte are complete), and its last batch of runs is walked however few of its 64
  // lanes it fills: four per wavefront, 256 KB on 3 GB, measured best of 2 .. 6, 8 and 16 (profiles/r08_a_ab_front_queue.txt).
  // (fed from host memory: sixteen times the ranges -- what runs after the last byte has arrived is one range per wavefront slot,
  // and a range is worked through by one wavefront from end to end: 0.35 ms for 256 KB -- and no queue: the launches of the
  // chunks share the flags, and a counter would hand one launch's numbers to another)
  const uint32_t per_wave = fed ? 16u : ctx->front_ranges_per_wave;
  uint64_t range_bytes = (n_bytes + (uint64_t)ctx->front_waves * per_wave - 1) / ((uint64_t)ctx->front_waves * per_wave);
  range_bytes = (range_bytes + kFrStep - 1) / kFrStep * kFrStep;
  if (range_bytes < ctx->front_min_range) range_bytes = ctx->front_min_range;
  if (range_bytes > (8ull << 20)) range_bytes = 8ull << 20;
  const uint64_t n_ranges64 = (n_bytes + range_bytes - 1) / range_bytes;
  const uint32_t rpg = (uint32_t)((n_ranges64 + kPartGroups - 1) / kPartGroups);
  if (rpg > kFrMaxGroupRanges) return feed_flush(ctx);
  const uint32_t n_ranges = (uint32_t)n_ranges64;
  const uint32_t run_cap = (uint32_t)(range_bytes / 64) + 64u, item_cap = (uint32_t)(range_bytes / 8) + 64u;
  void *p;
  KMI_TRY(ws_get(ctx, WS_TILE_INFO, sizeof(FrRange) * (n_ranges + 1), &p)); FrRange *info = (FrRange *)p;
  KMI_TRY(ws_get(ctx, WS_TILE_BASE, sizeof(uint64_t) * (kPartGroups + 1), &p)); uint64_t *group_runs = (uint64_t *)p;
  KMI_TRY(ws_get(ctx, WS_ENT_LIST, sizeof(uint32_t) * ((size_t)n_ranges * run_cap + 64), &p)); uint32_t *run_items = (uint32_t *)p;
  KMI_TRY(ws_get(ctx, WS_PK_STREAM, sizeof(uint32_t) * kFrRowDw * ((size_t)n_ranges * run_cap + 64), &p)); uint32_t *rows = (uint32_t *)p;
  KMI_TRY(ws_get(ctx, WS_SK_ITEMS, sizeof(uint32_t) * ((size_t)n_ranges * item_cap + 64), &p)); uint32_t *items = (uint32_t *)p;
  SkGroupWs g;
  KMI_TRY(sk_group_ws(ctx, &g));
  // (the front end's flags -- FLAG_FRONT_QUEUE among them --, the k-mer total and the group histograms, in one launch)
  hipLaunchKernelGGL(sk_zero_kernel, dim3(128), dim3(1024), 0, ctx->stream, g.wg_hist, (uint32_t)(kPartGroups * kNumCoarse),
                     reinterpret_cast<uint32_t *>(ctx->d_totals + TOT_SK_KMERS), 2u, (uint32_t *)nullptr, 0u, ctx->d_flags, (uint32_t)FZ_FRONT_0,
                     (uint32_t)FZ_FRONT_1, 0u, 0u);
  // ranges [r0, r1) of the input, from a queue word or (the launches of a host-fed build) without one
  auto launch_front = [&](uint32_t wgs, uint32_t r0, uint32_t r1, uint32_t *queue) {
#define KMI_SK_FRONT(EDGES)                                                                                                            \
    hipLaunchKernelGGL((sk_front_kernel<W, EDGES>), dim3(wgs), dim3(kFrThreads), 0, ctx->stream, bytes_dev, (uint64_t)n_bytes, range_bytes, n_ranges, k, \
                       is_rna(cfg), run_cap, item_cap, rpg, info, run_items, rows, items, g.wg_hist, (unsigned long long *)(ctx->d_totals + TOT_SK_KMERS),  \
                       ctx->d_flags, r0, r1, queue)
    if (ctx->edge_records) KMI_SK_FRONT(true); else KMI_SK_FRONT(false);
#undef KMI_SK_FRONT
  };
  uint32_t front_launched_waves = 0;   // (timing builds report on them)
  if (!fed) {
    ProfScope ps(ctx, "sk_front", n_bytes);
    // as many wavefronts as are resident (or as the context allows), never more than there are ranges; the rest of the ranges
    // go through the queue word, which the launch above has zeroed
    uint32_t waves = ctx->front_max_waves ? std::min(ctx->front_waves, ctx->front_max_waves) : ctx->front_waves;
    waves = std::max<uint32_t>((uint32_t)kFrWaves, waves / (uint32_t)kFrWaves * (uint32_t)kFrWaves);
    const uint32_t wgs = std::min((n_ranges + kFrWaves - 1) / kFrWaves, waves / (uint32_t)kFrWaves);
    front_launched_waves = wgs * (uint32_t)kFrWaves;
    launch_front(wgs, 0u, 0xffffffffu, ctx->d_flags + FLAG_FRONT_QUEUE);
  } else {
    // The input is still in host memory: its copy goes out in chunks on a stream of its own, all of them queued now, and behind every
    // chunk the front end takes the ranges whose bytes have arrived -- a range reads up to kFrOverrun + three steps behind its own end
    // (the lines it owns end there, and the two lines behind them; the next step's prefetch). Only the last chunk's ranges run after
    // the last byte is here; everything else of the front end is hidden behind the copy (BenchmarkKmerIndex.cpp:526-533 times from
    // bytes in host memory).
    ProfScope ps(ctx, "sk_front_fed", n_bytes);
    const uint8_t *host = ctx->feed_host;
    ctx->feed_host = nullptr;
    // chunk sizes: the front end works through a chunk about twenty times faster than the link delivers the next one, so every chunk
    // is a sixteenth of the one before it -- three or four copies in all (sixteen equal chunks cost 1.2 ms more than one copy: a gap
    // behind every copy, and the copies themselves a little slower)
    constexpr size_t kMaxChunks = sizeof(ctx->feed_ev) / sizeof(ctx->feed_ev[0]) - 1;
    size_t cut[kMaxChunks + 1];   // chunk c = bytes [cut[c], cut[c + 1])
    size_t n_chunks = 0;
    {
      size_t ratio = 16;
      if (const char *e = getenv("KMI_FEED_RATIO")) { const long v = atol(e); if (v >= 2 && v <= 64) ratio = (size_t)v; }
      size_t at = 0;
      cut[0] = 0;
      while (n_chunks + 1 < kMaxChunks && n_bytes - at > ctx->feed_min_chunk) {
        size_t len = (n_bytes - at) - (n_bytes - at) / ratio;
        len = len / 4096 * 4096;
        at += len; cut[++n_chunks] = at;
      }
      cut[++n_chunks] = n_bytes;
    }
    if (!ctx->copy_stream) KMI_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (size_t c = 0; c <= n_chunks; ++c) if (!ctx->feed_ev[c]) KMI_HIP(ctx, hipEventCreateWithFlags(&ctx->feed_ev[c], hipEventDisableTiming));
    // (the copy overwrites the input buffer: it starts behind what the build's stream has queued so far)
    KMI_HIP(ctx, hipEventRecord(ctx->feed_ev[n_chunks], ctx->stream));
    KMI_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->feed_ev[n_chunks], 0));
    for (size_t c = 0; c < n_chunks; ++c) {
      KMI_HIP(ctx, hipMemcpyAsync(const_cast<uint8_t *>(bytes_dev) + cut[c], host + cut[c], cut[c + 1] - cut[c], hipMemcpyHostToDevice, ctx->copy_stream));
      KMI_HIP(ctx, hipEventRecord(ctx->feed_ev[c], ctx->copy_stream));
    }
    const uint64_t margin = (uint64_t)kFrOverrun + 3ull * kFrStep;
    uint32_t r_done = 0;
    for (size_t c = 0; c < n_chunks; ++c) {
      KMI_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->feed_ev[c], 0));
      const uint64_t arrived = cut[c + 1];
      uint32_t r_end = n_ranges;
      if (c + 1 < n_chunks) r_end = arrived > margin + range_bytes ? (uint32_t)((arrived - margin) / range_bytes) : 0u;   // ranges [0, r_end) end margin bytes before `arrived`
      if (r_end > n_ranges) r_end = n_ranges;
      if (r_end <= r_done) continue;
      launch_front((r_end - r_done + kFrWaves - 1) / kFrWaves, r_done, r_end, nullptr);
      r_done = r_end;
    }
  }
  {
    ProfScope ps(ctx, "sk_offsets", kNumCoarse);
    sk_front_report_clocks(ctx);
    sk_front_report_leave(ctx, fed, front_launched_waves);
    hipLaunchKernelGGL(sk_front_verify_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const FrRange *)info, n_ranges, rpg, group_runs, ctx->d_totals + TOT_FRONT, ctx->d_flags);
    launch_rank_offsets(ctx->stream, (const uint32_t *)g.wg_hist, (uint32_t)kPartGroups, (uint32_t)kNumCoarse, g.cnt, g.base, g.wg_off);
  }
  KMI_HIP(ctx, hipGetLastError());
  // The scatter pass is queued BEFORE the host looks at the front end's verdict (it checks the flag itself), so the GPU does not
  // idle through the host's round trip: its output then has to be sized by what the front end can produce at most (one item per
  // item slot), which is three times the usual -- done for inputs up to 8 GB, and when the caller did not bring the buffer.
  const uint64_t r_bound = (uint64_t)n_ranges * item_cap;
  bool early = !out && n_bytes <= (8ull << 30);
  uint64_t *rec_a = out;
  if (early) {
    // (the early buffer is sized for the most the front end can produce, three times the usual: where that does not fit -- several
    // indexes in one context, a smaller GPU -- the scatter pass waits for the host to size it by what was produced: ADVICE r3)
    if (ws_get(ctx, WS_KEYS_A, (r_bound + 64) * 16, &p) == KMI_OK) rec_a = (uint64_t *)p; else { early = false; ctx->err.clear(); }
  }
  auto launch_scatter = [&]() {
    ProfScope ps(ctx, "sk_scatter", n_bytes);
#define KMI_SK_SCATTER_ROWS(CANON)                                                                                                     \
    hipLaunchKernelGGL(sk_scatter_rows_kernel<CANON>, dim3(kPartGroups), dim3(kFrScThreads), 0, ctx->stream, (const FrRange *)info, n_ranges, rpg, run_cap, \
                       item_cap, k, (const uint32_t *)run_items, (const uint32_t *)rows, (const uint32_t *)items, (const uint64_t *)g.wg_off, rec_a, lp,         \
                       (const uint32_t *)ctx->d_flags, ctx->edge_records ? 1u : 0u)
    if (canonical) KMI_SK_SCATTER_ROWS(true); else KMI_SK_SCATTER_ROWS(false);
#undef KMI_SK_SCATTER_ROWS
  };
  // what the host needs of the front end comes back into PINNED memory: four copies queued back to back and one synchronisation
  // (into pageable memory every copy was a host round trip of its own: 0.1 ms of an idle GPU per build)
  static_assert(H_MAIL_DECLINED == H_MAIL_CNT + 2 * kNumCoarse, "the mailbox holds the counts and starts of kNumCoarse groups");
  uint64_t *const h = ctx->h_totals;
  const uint64_t *const h_cnt = h + H_MAIL_CNT, *const h_tot = h + H_MAIL_FRONT;
  KMI_HIP(ctx, hipMemcpyAsync(h + H_MAIL_CNT, g.cnt, sizeof(uint64_t) * 2 * kNumCoarse, hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipMemcpyAsync(h + H_MAIL_DECLINED, ctx->d_flags + FLAG_SK_DECLINED, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipMemcpyAsync(h + H_MAIL_FRONT, ctx->d_totals + TOT_FRONT, sizeof(uint64_t) * 3, hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipMemcpyAsync(h + H_MAIL_KMERS, ctx->d_totals + TOT_SK_KMERS, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (early) {
    // the host waits for the read-backs only (an event behind them), not for the scatter pass queued behind that: what it queues
    // next -- the back end's tables and kernels -- is on the stream before the scatter pass has finished
    if (!ctx->ev_mail) KMI_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_mail, hipEventDisableTiming));
    KMI_HIP(ctx, hipEventRecord(ctx->ev_mail, ctx->stream));
    launch_scatter();
    KMI_HIP(ctx, hipEventSynchronize(ctx->ev_mail));
  } else {
    KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  const uint32_t h_flag = *reinterpret_cast<const uint32_t *>(h + H_MAIL_DECLINED);
  const uint64_t n = h[H_MAIL_KMERS];
  if (h_flag) {   // not this path's input (or not well-formed): the general path decides
    sk_front_report_decline(ctx);
    static_assert(FLAG_SK_WHY == FLAG_SK_DECLINED + 1, "cleared together");
    KMI_HIP(ctx, hipMemsetAsync(ctx->d_flags + FLAG_SK_DECLINED, 0, 2 * sizeof(uint32_t), ctx->stream));
    return KMI_OK;
  }
  *took = true;
  uint64_t R = 0;
  for (int c = 0; c < kNumCoarse; ++c) { R += h_cnt[c]; f->h_cnt[c] = h_cnt[c]; f->h_base[c] = h_cnt[kNumCoarse + c]; }
  f->n_records = R; f->n_kmers = n; f->wg_off = g.wg_off; f->recs = nullptr; f->n_seqs = (h_tot[0] + 2) / 4;
  if (n == 0) { f->ok = true; return KMI_OK; }
  if (!early) {
    if (!out || R + 64 > out_cap) { KMI_TRY(ws_get(ctx, WS_KEYS_A, (R + 64) * 16, &p)); rec_a = (uint64_t *)p; }
    launch_scatter();
  }
  KMI_HIP(ctx, hipGetLastError());
  f->ok = true; f->recs = rec_a;
  return KMI_OK;
}

// The door in front of both: one pass over the bytes when the input allows it (kmi_front.h), else the general front end -- scan
// (which words parse errors), list, minimizer. SK_NOT_THIS_PATH: the input exceeds a capacity of the general front end too, or
// the caller wants edge records, which only the one-pass front end makes (the de Bruijn node build): the caller's k-mer / tuple
// pipeline takes the input, nothing was changed.
enum SkDoor { SK_RECORDS, SK_NO_KMERS, SK_NOT_THIS_PATH };
template <int W>
static kmi_status sk_front_door(kmi_ctx *ctx, const kmi_config *cfg, const KShape &shape, const uint8_t *bytes_dev, size_t n_bytes, uint32_t lp, SkFront *f,
                                SkDoor *door, uint64_t *out = nullptr, size_t out_cap = 0) {
  *door = SK_NOT_THIS_PATH;
  bool took = false;
  KMI_TRY((sk_front_fast<W>(ctx, cfg, shape, bytes_dev, n_bytes, lp, f, &took, out, out_cap)));
  if (took && f->ok) { *door = f->n_kmers ? SK_RECORDS : SK_NO_KMERS; return KMI_OK; }
  if (ctx->edge_records) return KMI_OK;
  FastqScan sc;
  KMI_TRY(align_input(ctx, &bytes_dev, n_bytes));   // (the scan's 16-byte loads)
  KMI_TRY(fastq_scan(ctx, cfg, bytes_dev, n_bytes, &sc, false));
  // (no k-mer, so no list pass to carry the length rule: the verdict finds FLAG_PARSE as the scan left it)
  if (sc.n_tuples == 0) { *door = SK_NO_KMERS; return fastq_length_verdict(ctx); }
  KMI_TRY((sk_front_end<W>(ctx, cfg, shape, sc, lp, f, out, out_cap)));
  if (f->ok) *door = SK_RECORDS;
  return KMI_OK;
}

// ---- diagnostics of the back end (KMI_SK_TIMING builds, KMI_SLACK_DEBUG)
static void sk_reduce_report_clocks(kmi_ctx *ctx) {
#ifdef KMI_SK_TIMING
  unsigned long long t[8];
  hipStreamSynchronize(ctx->stream);
  hipMemcpy(t, ctx->d_flags + FLAG_CLOCKS, sizeof(t), hipMemcpyDeviceToHost);
  fprintf(stderr, "sk_reduce wave clocks: A-T1 %llu  A-direct %llu  A-wait %llu  B-work %llu  B-wait %llu  emit %llu  between %llu\n", t[0], t[1], t[2], t[3], t[4], t[5], t[6]);
  hipMemset(ctx->d_flags + FLAG_CLOCKS, 0, sizeof(t));
#endif
}
// how full the fullest fine bucket was
static void sk_slack_report(const uint32_t *fine_cnt, const uint64_t *h_cnt, const uint32_t *h_cap, uint32_t lp, uint64_t R) {
  if (!getenv("KMI_SLACK_DEBUG")) return;
  std::vector<uint32_t> fc(kNumFine);
  (void)hipMemcpy(fc.data(), fine_cnt, sizeof(uint32_t) * kNumFine, hipMemcpyDeviceToHost);
  double worst = 0; uint32_t over = 0;
  for (int f = 0; f < kNumFine; ++f) {
    const double mean = (double)h_cnt[f / kSubPerCoarse] / kSubPerCoarse;
    if (mean > 0 && fc[f] / mean > worst) worst = fc[f] / mean;
    over += fc[f] > h_cap[f / kSubPerCoarse];
  }
  fprintf(stderr, "fine buckets with room: %u of %d outgrew it, the fullest holds %.3f x its coarse bucket's mean (lp %u, %llu records)\n", over,
          (int)kNumFine, worst, lp, (unsigned long long)R);
}

// Back end: records grouped by coarse bucket (rec_a; group c = [h_base[c], h_base[c] + h_cnt[c]), written by kPartGroups
// workgroups at wg_off[g][c]) -> fine buckets -> sk_reduce -> the index (layout W | lp << 8), or added to what it holds.
template <int W>
static kmi_status sk_back_end(kmi_index *idx, const uint64_t *rec_a, uint64_t R, const uint64_t *h_cnt, const uint64_t *h_base, const uint64_t *wg_off,
                              uint64_t n, uint32_t lp, bool exact = false) {
  // exact = false (an index without entries): the fine buckets get room instead of exact offsets, so the records are not read an
  // extra time to be counted (sk_scatter_fine_slack_lines_kernel); a bucket that outgrows its room sends the build through here again
  // with exact = true
  constexpr int NW = 1;
  kmi_ctx *ctx = idx->ctx;
  const bool slack = !exact && ctx->sk_slack && (!idx->has_data || idx->n_entries == 0) && R >= 4096;   // (room_x64 below: <= 6.1 x the records)
  ctx->sk_left.valid = false;
  const uint32_t k = idx->shape.k;
  const bool canonical = idx->cfg.strand != KMI_STRAND_SINGLE;
  void *p;
  SkGroupWs g;
  KMI_TRY(sk_group_ws(ctx, &g));
  uint64_t *const cend = g.cend;
  KMI_TRY(ws_get(ctx, WS_HIST, sizeof(uint32_t) * kNumFine * kFineParts + sizeof(uint64_t) * ((kNumFine + 1) * 2 + kNumFine * kFineParts + kNumCoarse) + 256, &p));
  uint32_t *fine_hist = (uint32_t *)p;
  uint64_t *fine_off = (uint64_t *)((char *)p + sizeof(uint32_t) * kNumFine * kFineParts);
  uint64_t *part_off = fine_off + 2 * (kNumFine + 1);
  uint64_t *coarse_base = part_off + (uint64_t)kNumFine * kFineParts;
  uint64_t h_end[kNumCoarse];
  for (int c = 0; c < kNumCoarse; ++c) h_end[c] = h_base[c] + h_cnt[c];
  KMI_HIP(ctx, hipMemcpyAsync(cend, h_end, sizeof(h_end), hipMemcpyHostToDevice, ctx->stream));   // (h_end outlives the copy: this function synchronises before it returns)
  // the slack layout: every fine bucket of coarse bucket c has room for room_x64 / 64 of c's mean share + 64, in steps of 8 records
  // How uneven minimizer buckets are depends on the minimizer length m = k - W + 1 (few canonical m-mers: a few of them take most
  // minima) and on the rank bits of a build over ranks (a rank's buckets stand for fewer minimizer classes of a larger genome).
  // Fullest fine bucket / its coarse bucket's mean, measured on synthetic reads: m = 11: 1.9 - 2.6, m = 12: 1.63, m >= 13: 1.36 -
  // 1.54; for m = 13 and lp = 0 / 1 / 2 / 3: 1.45 / < 1.6 / 1.79 / 2.27.
  const uint32_t m_len = idx->shape.k - (uint32_t)W + 1u;
  const uint64_t room_m = m_len <= 11u ? 26u : (m_len == 12u ? 18u : 14u);            // in eighths of the mean
  static const uint64_t room_lp[4] = {8, 10, 12, 15};                                   // in eighths
  const uint64_t room_x64 = room_m * room_lp[lp < 4u ? lp : 3u];
  uint64_t h_region[kNumCoarse], total_b = 0;
  uint32_t h_cap[kNumCoarse];
  for (int c = 0; c < kNumCoarse; ++c) {
    const uint64_t cap = ((h_cnt[c] * room_x64 / 64 + kSubPerCoarse - 1) / kSubPerCoarse + 64 + 7) / 8 * 8;
    h_cap[c] = (uint32_t)cap; h_region[c] = total_b; total_b += cap * kSubPerCoarse;
  }
  KMI_TRY(ws_get(ctx, WS_KEYS_B, ((slack ? total_b : R) + 64) * 16, &p)); uint64_t *rec_b = (uint64_t *)p;
  KMI_TRY(ws_get(ctx, WS_SPLIT_OFF, sizeof(uint32_t) * kNumFine * kFineParts + sizeof(uint64_t) * ((kNumFine + 1) + kNumFine * kFineParts + kNumCoarse) + 256, &p));
  uint32_t *fine_kmers = (uint32_t *)p;
  uint64_t *kmer_off = (uint64_t *)((char *)p + sizeof(uint32_t) * kNumFine * kFineParts);
  uint64_t *k_part = kmer_off + (kNumFine + 1), *k_base = k_part + (uint64_t)kNumFine * kFineParts;
  uint64_t *d_region = nullptr; uint32_t *d_cap = nullptr, *fine_cnt = nullptr;
  if (slack) {
    KMI_TRY(ws_get(ctx, WS_BUCKET_OFF, sizeof(uint64_t) * kNumCoarse + sizeof(uint32_t) * kNumCoarse + 64, &p));
    d_region = (uint64_t *)p; d_cap = (uint32_t *)(d_region + kNumCoarse);
    fine_cnt = fine_hist;   // (the first half of the histogram block: records per fine bucket, counted as they are appended)
    KMI_HIP(ctx, hipMemcpyAsync(d_region, h_region, sizeof(h_region), hipMemcpyHostToDevice, ctx->stream));
    KMI_HIP(ctx, hipMemcpyAsync(d_cap, h_cap, sizeof(h_cap), hipMemcpyHostToDevice, ctx->stream));
    // (the append counters, the k-mer counts, the reduce's votes, FLAG_SK_ROOM, FLAG_REDUCE_QUEUE and the spare words behind it)
    hipLaunchKernelGGL(sk_zero_kernel, dim3(96), dim3(1024), 0, ctx->stream, fine_cnt, (uint32_t)kNumFine, fine_kmers, (uint32_t)(kNumFine * kFineParts),
                       (uint32_t *)nullptr, 0u, ctx->d_flags, (uint32_t)FZ_BACK_0, (uint32_t)FZ_BACK_1, (uint32_t)FZ_BACK_2, (uint32_t)FZ_BACK_3);
    {
      ProfScope ps(ctx, "sk_scatter_fine", R);
      // whole lines + pad records
      hipLaunchKernelGGL(sk_scatter_fine_slack_lines_kernel, dim3(kNumCoarse * kFineParts), dim3(kPartThreads), 0, ctx->stream, (const uint64_t *)rec_a, rec_b,
                         (const uint64_t *)wg_off, (const uint64_t *)cend, (uint32_t)kPartGroups, (const uint64_t *)d_region, (const uint32_t *)d_cap,
                         fine_cnt, fine_kmers, ctx->d_flags);
    }
    {
      ProfScope ps(ctx, "fine_offsets", kNumFine);
      launch_fine_offsets(ctx, fine_kmers, kmer_off, k_part, k_base);
    }
  } else {
    {
      ProfScope ps(ctx, "sk_fine_count", R);
      hipLaunchKernelGGL(sk_fine_count_kernel, dim3(kNumCoarse * kFineParts), dim3(1024), 0, ctx->stream, (const uint64_t *)rec_a,
                         (const uint64_t *)wg_off, (const uint64_t *)cend, (uint32_t)kPartGroups, fine_hist, fine_kmers);
    }
    {
      ProfScope ps(ctx, "fine_offsets", kNumFine);
      launch_fine_offsets(ctx, fine_hist, fine_off, part_off, coarse_base);
      launch_fine_offsets(ctx, fine_kmers, kmer_off, k_part, k_base);
    }
    {
      ProfScope ps(ctx, "sk_scatter_fine", R);
      hipLaunchKernelGGL((scatter_fine_kernel<1, 2, 1>), dim3(kNumCoarse * kFineParts), dim3(kPartThreads), 0, ctx->stream, (const uint64_t *)rec_a,
                         rec_b, idx->shape, (const uint64_t *)fine_off, (const uint64_t *)part_off, (const uint64_t *)wg_off,
                         (uint32_t)kPartGroups, (int)BUCKET_REC, 0u);
    }
  }
  // per bucket: as many output slots as it has k-mers (bucket_reduce_kernel's contract), compacted by adopt_tmp
  KMI_TRY(ws_get(ctx, WS_TMP_KEYS, (n + 64) * sizeof(uint64_t), &p)); uint64_t *tmp_keys = (uint64_t *)p;
  KMI_TRY(ws_get(ctx, WS_TMP_VALS, (n + 64) * sizeof(uint32_t), &p)); uint32_t *tmp_vals = (uint32_t *)p;
  KMI_TRY(ws_get(ctx, WS_BUCKET_CNT, sizeof(uint32_t) * kNumFine, &p)); uint32_t *out_cnt = (uint32_t *)p;
  if (!slack) KMI_HIP(ctx, hipMemsetAsync(ctx->d_flags + FLAG_SK_LEVEL0, 0, sizeof(uint32_t) * (FLAG_SK_LEVEL_END - FLAG_SK_LEVEL0), ctx->stream));   // the pass-structure votes of sk_reduce (the slack path has zeroed them)
  {
    const uint32_t nmax = sk_nmax_of(k);
    // persistent workgroups (one per CU: each takes the whole LDS) pull the buckets from a queue word
    uint32_t *queue = ctx->d_flags + FLAG_REDUCE_QUEUE;
    if (!slack) KMI_HIP(ctx, hipMemsetAsync(queue, 0, sizeof(uint32_t) * (FLAG_REDUCE_QUEUE_END - FLAG_REDUCE_QUEUE), ctx->stream));   // (the queue word and the seven spare words behind it)
#ifndef KMI_SK_WGS_PER_CU
#define KMI_SK_WGS_PER_CU 1
#endif
    const uint32_t wgs = (ctx->n_cus ? ctx->n_cus : 256u) * KMI_SK_WGS_PER_CU;
    ProfScope ps(ctx, "sk_reduce", n);
#define KMI_SK_REDUCE(CANON, OWN, SPECIAL)                                                                                               \
    hipLaunchKernelGGL((sk_reduce_kernel<CANON, OWN, SPECIAL>), dim3(wgs), dim3(KMI_SK_NT), 0, ctx->stream, (const uint64_t *)rec_b,        \
                       (const uint64_t *)fine_off, k, (const uint64_t *)kmer_off, tmp_keys, tmp_vals, out_cnt, ctx->d_flags, queue, (uint32_t)kNumFine, \
                       ctx->sk_level_hint, lp, ctx->sk_inv_dup, (const uint64_t *)d_region, (const uint32_t *)d_cap, (const uint32_t *)fine_cnt)
    if (k == 32u) { if (canonical) KMI_SK_REDUCE(true, 64 * 21, true); else KMI_SK_REDUCE(false, 64 * 21, true); }   // (a 32-mer can equal the empty marker)
    else if (nmax <= 21u) { if (canonical) KMI_SK_REDUCE(true, 64 * 21, false); else KMI_SK_REDUCE(false, 64 * 21, false); }
    else if (nmax <= 24u) { if (canonical) KMI_SK_REDUCE(true, 64 * 24, false); else KMI_SK_REDUCE(false, 64 * 24, false); }
    else { if (canonical) KMI_SK_REDUCE(true, 64 * 32, false); else KMI_SK_REDUCE(false, 64 * 32, false); }
#undef KMI_SK_REDUCE
  }
  KMI_HIP(ctx, hipGetLastError());
  sk_reduce_report_clocks(ctx);
  // a fine bucket that outgrew its room? (its records beyond the room were not written: this attempt's result is void; read with
  // the level votes below)
  if (slack) KMI_HIP(ctx, hipMemcpyAsync(ctx->h_totals + H_SK_ROOM, ctx->d_flags + FLAG_SK_ROOM, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  // the level most buckets ended at: where the buckets of the NEXT build (batch, step) of this context start. The copy is queued
  // here and read after the synchronisation adopt_tmp needs anyway (one host round trip less per build).
  KMI_HIP(ctx, hipMemcpyAsync(ctx->h_totals + H_SK_LEVELS /* pinned */, ctx->d_flags + FLAG_SK_LEVEL0, sizeof(uint32_t) * 9, hipMemcpyDeviceToHost, ctx->stream));
  auto read_levels = [&]() {
    const uint32_t *lv = reinterpret_cast<const uint32_t *>(ctx->h_totals + H_SK_LEVELS);
    uint64_t seen = 0; uint32_t best = 0;
    for (uint32_t l = 0; l < 9; ++l) { seen += lv[l]; if (lv[l] > lv[best]) best = l; }
    // (level 0 finishes are only recorded once the hint is non-zero: no record at all means "everything fit at level 0")
    if (seen == 0) ctx->sk_level_hint = 0;
    else if (ctx->sk_level_hint == 0) { uint64_t up = seen; ctx->sk_level_hint = (up * 2 > (uint64_t)kNumFine) ? best : 0u; }
    else ctx->sk_level_hint = best;
  };
  const uint32_t layout = (uint32_t)W | (lp << 8);
  if (!idx->has_data || idx->n_entries == 0) {
    // the index IS the reduce output: entries grouped by minimizer bucket. Queries partition their keys by the same function
    // (fine15_of_key); whatever needs the placement-hash layout converts the entries once (ensure_layout).
    KMI_TRY((adopt_tmp<NW>(idx, tmp_keys, tmp_vals, kmer_off, nullptr, out_cnt, false, n, true)));
    if (slack) sk_slack_report(fine_cnt, h_cnt, h_cap, lp, R);
    if (slack && *reinterpret_cast<const uint32_t *>(ctx->h_totals + H_SK_ROOM)) {
      KMI_TRY(kmi_index_clear(idx));
      return sk_back_end<W>(idx, rec_a, R, h_cnt, h_base, wg_off, n, lp, true);
    }
    read_levels();
    idx->layout_w = layout;
    if (n) ctx->sk_inv_dup = (float)((double)idx->n_entries / (double)n);   // where the buckets of the next build start (sk_reduce_kernel)
    ctx->sk_left.recs = rec_b; ctx->sk_left.rec_off = slack ? nullptr : fine_off; ctx->sk_left.region = d_region; ctx->sk_left.cap = d_cap;
    ctx->sk_left.cnt = fine_cnt; ctx->sk_left.valid = true;
    return KMI_OK;
  }
  // the index holds entries already: the new ones become a scratch index, whose pairs are added to the old
  kmi_index scratch;
  scratch.ctx = ctx; scratch.cfg = idx->cfg; scratch.shape = idx->shape; scratch.val_words = 0; scratch.saturating = idx->saturating;
  kmi_status st = adopt_tmp<NW>(&scratch, tmp_keys, tmp_vals, kmer_off, nullptr, out_cnt);
  if (st == KMI_OK) read_levels();
  if (st == KMI_OK && n) ctx->sk_inv_dup = (float)((double)scratch.n_entries / (double)n);
  if (st == KMI_OK && scratch.n_entries) {
    st = ws_get(ctx, WS_OUTPUT, (scratch.n_entries + 64) * 2 * sizeof(uint64_t), &p);   // (WS_INPUT2 is the re-layout's)
    if (st == KMI_OK) {
      hipLaunchKernelGGL((zip_pairs_kernel<NW>), dim3(2048), dim3(256), 0, ctx->stream, (const uint64_t *)scratch.keys, (const uint32_t *)scratch.vals,
                         scratch.n_entries, (uint64_t *)p);
      st = index_insert_pairs(idx, (const uint64_t *)p, (size_t)scratch.n_entries, false, true);
    }
  }
  (void)hipStreamSynchronize(ctx->stream);
  free_index_arrays(&scratch);
  return st;
}
static kmi_status sk_back(kmi_index *idx, uint32_t w, const SkFront &f, uint32_t lp) {   // a front end's records into the index
  return sk_dispatch_w(w, [&](auto W) { return sk_back_end<W>(idx, f.recs, f.n_records, f.h_cnt, f.h_base, f.wg_off, f.n_kmers, lp); });
}

// ---- Index::build_* on one rank. FASTQ: through the door; an input that is not this path's goes to the k-mer pipeline
static kmi_status index_build_fused(kmi_index *idx, const uint8_t *bytes_dev, size_t n_bytes) {
  if (const uint32_t w = sk_width(idx, SK_FASTQ)) {   // (the caller has a count index and FASTQ: the shape and the context decide)
    SkFront f;
    SkDoor door;
    KMI_TRY(sk_dispatch_w(w, [&](auto W) { return sk_front_door<W>(idx->ctx, &idx->cfg, idx->shape, bytes_dev, n_bytes, 0u, &f, &door); }));
    if (door == SK_RECORDS) return sk_back(idx, w, f, 0u);
    if (door == SK_NO_KMERS) return KMI_OK;
  }
  KMI_DISPATCH(idx->shape, build_fused_impl, idx, bytes_dev, n_bytes);
}

// FASTA count index through super-k-mers: the compacted character stream of kmi_fasta.hip is "FASTQ without line roles", its
// run list comes from the break bitmap (fasta_runs_kernel), everything behind it is the FASTQ build's.
// *done = false: the input does not fit the item capacities (the k-mer pipeline takes over)
static kmi_status sk_build_fasta(kmi_index *idx, uint32_t w, const FastaScan &fa, bool *done) {
  *done = false;
  SkFront f;
  FastqScan none{};
  KMI_TRY(sk_dispatch_w(w, [&](auto W) { return sk_front_end<W>(idx->ctx, &idx->cfg, idx->shape, none, 0u, &f, nullptr, 0, &fa); }));
  if (!f.ok) return KMI_OK;
  *done = true;
  if (f.n_records == 0) return KMI_OK;
  return sk_back(idx, w, f, 0u);
}

// ---- a build over 2^lp ranks through exchanged super-k-mer records ------------------------------------------------------
// produce: the front end; the records leave grouped by owner rank (the owner of a record = the top lp bits of its bucket bits;
// groups of 256 / nranks consecutive coarse buckets), send_counts = records per rank.
static kmi_status sk_produce(kmi_index *idx, uint32_t w, const uint8_t *bytes_dev, size_t n_bytes, uint32_t nranks, const uint64_t **recs_out, uint64_t *n_records,
                             uint64_t *send_counts, int *produced, uint64_t *out, size_t out_cap) {
  *produced = 0; *recs_out = nullptr; *n_records = 0;
  for (uint32_t r = 0; r < nranks; ++r) send_counts[r] = 0;
  if (n_bytes == 0) { *produced = 1; return KMI_OK; }
  const uint32_t lp = 31u - (uint32_t)__builtin_clz(nranks);
  SkFront f;
  SkDoor door;
  KMI_TRY(sk_dispatch_w(w, [&](auto W) { return sk_front_door<W>(idx->ctx, &idx->cfg, idx->shape, bytes_dev, n_bytes, lp, &f, &door, out, out_cap); }));
  if (door != SK_RECORDS) { *produced = door == SK_NO_KMERS; return KMI_OK; }
  const uint32_t per = (uint32_t)kNumCoarse / nranks;
  for (uint32_t c = 0; c < (uint32_t)kNumCoarse; ++c) send_counts[c / per] += f.h_cnt[c];
  *recs_out = f.recs; *n_records = f.n_records; *produced = 1;
  // (the records are being written on the context's stream: whoever reads them is ordered behind it -- a collective on a stream
  // that waits for this one, the library's own exchange, or kmi_copy_on_device)
  return KMI_OK;
}

// consume: what arrived (a flat record array; inside every source's part the records are grouped by the sender's buckets, whose
// low lp bits are not the receiver's coarse bucket bits) is sorted by coarse bucket once, then takes the back end
static kmi_status sk_consume(kmi_index *idx, uint32_t w, const uint64_t *recs_dev, uint64_t R, uint32_t nranks) {
  kmi_ctx *ctx = idx->ctx;
  const uint32_t lp = 31u - (uint32_t)__builtin_clz(nranks);
  if (R == 0) { idx->owner_lp = lp; return KMI_OK; }
  void *p;
  SkGroupWs g;
  KMI_TRY(sk_group_ws(ctx, &g));
  KMI_TRY(ws_get(ctx, WS_KEYS_A, (R + 64) * 16, &p)); uint64_t *rec_a = (uint64_t *)p;
  KMI_HIP(ctx, hipMemsetAsync(ctx->d_totals + TOT_SK_KMERS, 0, sizeof(uint64_t), ctx->stream));
  {
    ProfScope ps(ctx, "sk_recv_hist", R);
    hipLaunchKernelGGL(sk_recv_hist_kernel, dim3(kPartGroups), dim3(kPartThreads), 0, ctx->stream, recs_dev, R, g.wg_hist,
                       (unsigned long long *)(ctx->d_totals + TOT_SK_KMERS));
  }
  {
    ProfScope ps(ctx, "sk_offsets", kNumCoarse);
    launch_rank_offsets(ctx->stream, (const uint32_t *)g.wg_hist, (uint32_t)kPartGroups, (uint32_t)kNumCoarse, g.cnt, g.base, g.wg_off);
  }
  BucketFn fn; fn.mode = BUCKET_REC_COARSE; fn.shape = idx->shape; fn.dist_hash = 0; fn.farm_ndebug = false; fn.nranks = 1; fn.sub = 1;
  {
    ProfScope ps(ctx, "sk_recv_scatter", R);
    hipLaunchKernelGGL((scatter_chunks_kernel<1, 2, 1>), dim3(kPartGroups), dim3(kPartThreads), 0, ctx->stream, recs_dev, R, rec_a, idx->shape, 0u, false, fn,
                       (const uint64_t *)g.wg_off);
  }
  KMI_HIP(ctx, hipGetLastError());
  uint64_t h[2 * kNumCoarse], n_kmers = 0;
  KMI_HIP(ctx, hipMemcpyAsync(h, g.cnt, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipMemcpyAsync(&n_kmers, ctx->d_totals + TOT_SK_KMERS, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  KMI_TRY(sk_dispatch_w(w, [&](auto W) { return sk_back_end<W>(idx, rec_a, R, h, h + kNumCoarse, g.wg_off, n_kmers, lp); }));
  idx->owner_lp = lp;
  return KMI_OK;
}

}  // namespace kmi
