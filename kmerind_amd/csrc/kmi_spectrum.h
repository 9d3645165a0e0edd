// The count spectrum of a count index and its filter by count (no counterpart in the reference beyond export + a host loop):
//   kmi_index_spectrum_*      hist[min(count, n_bins - 1)] += 1 per stored entry, plus the sum / min / max of the counts
//   kmi_index_retain_counts   keeps the entries with lo <= count <= hi, in fresh arrays of exactly the surviving size
// Both are one streaming pass over arrays that already lie in bucket order: the spectrum reads `vals` alone (the flat array of a
// dense index, bucket b = [bucket_off[b], bucket_off[b] + bucket_cnt[b]) of a sparse one, whose leftover slots are never touched);
// the filter counts the survivors per fine bucket, scans the counts into the new bucket_off and copies every bucket's survivors in
// their old order.
//
// Included by kmi_index.hip after kmi_lookup.h.
#pragma once

namespace kmi {

// Bins below kSpecLdsBins are counted in LDS (32-bit words: a workgroup sees far fewer than 2^32 entries -- the grid never has
// fewer than one workgroup per 2^20 of them) and reach the global histogram as one 64-bit atomic per non-empty bin and workgroup;
// bins from kSpecLdsBins on take a global atomic per entry (counts in the thousands are rare in real spectra). Real spectra put
// most entries into the first few bins, where every lane of a wavefront would add to the same LDS word: bins below kSpecHot are
// counted in registers, one counter per lane and bin, and folded once per wavefront at the end.
constexpr int kSpecThreads = 256;
constexpr uint32_t kSpecLdsBins = 4096;
constexpr uint32_t kSpecHot = 4;
// device words of a spectrum call behind the context's WS_SPECTRUM slot: sum of the counts, the largest count, ~(the smallest)
enum { SPEC_SUM = 0, SPEC_MAX = 1, SPEC_NOTMIN = 2, SPEC_SURVIVORS = 3, SPEC_FULLEST = 4, SPEC_WORDS = 8 };

struct SpecAcc {
  uint32_t hot[kSpecHot];
  uint64_t sum;
  uint32_t lo, hi;
};

__device__ __forceinline__ void spec_add(SpecAcc &a, uint32_t c, uint32_t last_bin, uint32_t *s_bins, unsigned long long *hist) {
  a.sum += c;
  a.lo = c < a.lo ? c : a.lo;
  a.hi = c > a.hi ? c : a.hi;
  const uint32_t bin = c < last_bin ? c : last_bin;
  if (bin < kSpecHot) {
#pragma unroll
    for (uint32_t h = 0; h < kSpecHot; ++h) a.hot[h] += bin == h ? 1u : 0u;
  } else if (bin < kSpecLdsBins) {
    atomicAdd(&s_bins[bin], 1u);
  } else {
    atomicAdd(&hist[bin], 1ull);
  }
}

// vals[b, e) by `nt` cooperating threads of which this one is `t`: single words up to the first 16-byte boundary, then four
// counts per load with kSpecBatch loads in flight per lane, then the rest
constexpr int kSpecBatch = 4;
template <typename F>
__device__ __forceinline__ void spec_stream(const uint32_t *__restrict__ vals, uint64_t b, uint64_t e, uint64_t t, uint64_t nt, F &&f) {
  uint64_t body = (b + 3) & ~3ull;
  body = body < e ? body : e;
  for (uint64_t i = b + t; i < body; i += nt) f(vals[i]);
  const uint64_t n4 = (e - body) >> 2;
  const uint4 *__restrict__ v4 = reinterpret_cast<const uint4 *>(vals + body);
  for (uint64_t j0 = t; j0 < n4; j0 += kSpecBatch * nt) {
    uint4 v[kSpecBatch];
#pragma unroll
    for (int u = 0; u < kSpecBatch; ++u) {
      const uint64_t j = j0 + (uint64_t)u * nt;
      if (j < n4) v[u] = v4[j];
    }
#pragma unroll
    for (int u = 0; u < kSpecBatch; ++u) {
      if (j0 + (uint64_t)u * nt < n4) { f(v[u].x); f(v[u].y); f(v[u].z); f(v[u].w); }
    }
  }
  for (uint64_t i = body + 4 * n4 + t; i < e; i += nt) f(vals[i]);
}

// idx_cnt == nullptr: the dense array vals[0, n); else the sparse form, fine bucket by fine bucket
__global__ __launch_bounds__(kSpecThreads) void count_spectrum_kernel(const uint32_t *__restrict__ vals, uint64_t n, const uint64_t *__restrict__ idx_off,
                                                                     const uint32_t *__restrict__ idx_cnt, uint32_t n_bins,
                                                                     unsigned long long *__restrict__ hist, unsigned long long *__restrict__ totals) {
  __shared__ uint32_t s_bins[kSpecLdsBins];
  __shared__ unsigned long long s_sum;
  __shared__ uint32_t s_lo, s_hi;
  const uint32_t last_bin = n_bins - 1u;
  const uint32_t lds_bins = n_bins < kSpecLdsBins ? n_bins : kSpecLdsBins;
  for (uint32_t i = threadIdx.x; i < lds_bins; i += kSpecThreads) s_bins[i] = 0u;
  if (threadIdx.x == 0) { s_sum = 0ull; s_lo = 0xffffffffu; s_hi = 0u; }
  lds_barrier();
  SpecAcc a;
#pragma unroll
  for (uint32_t h = 0; h < kSpecHot; ++h) a.hot[h] = 0u;
  a.sum = 0; a.lo = 0xffffffffu; a.hi = 0u;
  auto add = [&](uint32_t c) { spec_add(a, c, last_bin, s_bins, hist); };
  if (!idx_cnt) {
    spec_stream(vals, 0, n, (uint64_t)blockIdx.x * kSpecThreads + threadIdx.x, (uint64_t)gridDim.x * kSpecThreads, add);
  } else {
    // a wavefront per bucket: a bucket of a few thousand entries is a dozen loads per lane, a workgroup's share would be three
    constexpr uint32_t WAVES = kSpecThreads / kWave;
    for (uint32_t b = blockIdx.x * WAVES + wave_id(); b < (uint32_t)kNumFine; b += gridDim.x * WAVES) {
      const uint64_t ib = idx_off[b];
      spec_stream(vals, ib, ib + idx_cnt[b], lane_id(), kWave, add);
    }
  }
  // one LDS add per wavefront for each hot bin and for the totals
#pragma unroll
  for (uint32_t h = 0; h < kSpecHot; ++h) {
    const uint32_t w = wave_reduce_sum(a.hot[h]);
    if (lane_id() == 0 && w && h < lds_bins) atomicAdd(&s_bins[h], w);
  }
  {
    const uint64_t s = wave_reduce_sum(a.sum);
    uint32_t lo = a.lo, hi = a.hi;
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
      const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, d, kWave), h2 = (uint32_t)__shfl_xor((int)hi, d, kWave);
      lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
    }
    if (lane_id() == 0) { atomicAdd(&s_sum, (unsigned long long)s); atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
  }
  lds_barrier();
  for (uint32_t i = threadIdx.x; i < lds_bins; i += kSpecThreads) {
    const uint32_t c = s_bins[i];
    if (c) atomicAdd(&hist[i], (unsigned long long)c);
  }
  if (threadIdx.x == 0 && s_lo <= s_hi) {   // (a workgroup that saw no entry keeps lo > hi)
    atomicAdd(&totals[SPEC_SUM], s_sum);
    atomicMax(&totals[SPEC_MAX], (unsigned long long)s_hi);
    atomicMax(&totals[SPEC_NOTMIN], (unsigned long long)(~s_lo));
  }
}

// Fine bucket b, one wavefront each: how many of its entries have lo <= count <= hi. fullest: the entry count of the fullest bucket.
constexpr int kRetainCountThreads = 256;
__global__ __launch_bounds__(kRetainCountThreads) void bucket_retain_count_kernel(const uint32_t *__restrict__ vals, const uint64_t *__restrict__ idx_off,
                                                                                 const uint32_t *__restrict__ idx_cnt, uint32_t lo, uint32_t hi,
                                                                                 uint32_t *__restrict__ out_cnt, unsigned long long *__restrict__ fullest) {
  const uint32_t b = blockIdx.x * (kRetainCountThreads / kWave) + wave_id();   // (the grid is kNumFine wavefronts exactly)
  const uint64_t ib = idx_off[b], ie = idx_cnt ? ib + idx_cnt[b] : idx_off[b + 1];
  uint32_t keep = 0;
  spec_stream(vals, ib, ie, lane_id(), kWave, [&](uint32_t c) { keep += (c >= lo && c <= hi) ? 1u : 0u; });
  keep = wave_reduce_sum(keep);
  if (lane_id() == 0) {
    out_cnt[b] = keep;
    if (ie > ib) atomicMax(fullest, (unsigned long long)(ie - ib));
  }
}

// Fine bucket b: its surviving entries, in their old order, to new_off[b] of the new arrays. A tile is one entry per thread; a
// bucket of more entries takes several tiles, each behind the survivors of the ones before it. rows (null for a count index): a
// 32-byte payload per entry, in the order of the keys -- the edge counters of a de Bruijn node map (kmi_dbg_retain_counts) --
// which moves with its entry as two uint4.
constexpr int kRetainTile = 256;
template <int NW>
__global__ __launch_bounds__(kRetainTile) void bucket_retain_compact_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                                           const uint64_t *__restrict__ idx_off, const uint32_t *__restrict__ idx_cnt,
                                                                           uint32_t lo, uint32_t hi, const uint64_t *__restrict__ new_off,
                                                                           uint64_t *__restrict__ new_keys, uint32_t *__restrict__ new_vals,
                                                                           const uint4 *__restrict__ rows, uint4 *__restrict__ new_rows) {
  __shared__ uint32_t s_scan[kRetainTile / kWave + 2];
  const uint32_t b = blockIdx.x;
  uint64_t dst = new_off[b];
  const uint64_t dst_end = new_off[b + 1];
  if (dst == dst_end) return;   // nothing of this bucket survives
  const uint64_t ib = idx_off[b], ie = idx_cnt ? ib + idx_cnt[b] : idx_off[b + 1];
  for (uint64_t t0 = ib; t0 < ie; t0 += kRetainTile) {
    const uint64_t i = t0 + threadIdx.x;
    uint32_t c = 0;
    bool keep = false;
    if (i < ie) { c = vals[i]; keep = c >= lo && c <= hi; }
    uint32_t total;
    const uint32_t pos = block_exclusive_scan<uint32_t>(keep ? 1u : 0u, s_scan, &total);
    if (keep && dst + pos < dst_end) {   // (the bound holds by construction: the count pass saw the same entries)
      const uint64_t o = dst + pos;
#pragma unroll
      for (int w = 0; w < NW; ++w) new_keys[o * NW + w] = keys[i * NW + w];
      new_vals[o] = c;
      if (rows) { new_rows[o * 2u] = rows[i * 2u]; new_rows[o * 2u + 1u] = rows[i * 2u + 1u]; }
    }
    dst += total;
  }
}

// the spectrum of this rank's entries into hist_dev (n_bins words, cleared here); queued on the stream. The totals stay on the
// device (WS_SPECTRUM) for spectrum_totals.
static kmi_status spectrum_run(kmi_index *idx, uint32_t n_bins, uint64_t *hist_dev) {
  kmi_ctx *ctx = idx->ctx;
  void *p;
  KMI_TRY(ws_get(ctx, WS_SPECTRUM, sizeof(uint64_t) * SPEC_WORDS + sizeof(uint32_t) * kNumFine, &p));
  unsigned long long *tot = (unsigned long long *)p;
  KMI_HIP(ctx, hipMemsetAsync(tot, 0, sizeof(uint64_t) * SPEC_WORDS, ctx->stream));
  KMI_HIP(ctx, hipMemsetAsync(hist_dev, 0, sizeof(uint64_t) * n_bins, ctx->stream));
  if (!idx->has_data || idx->n_entries == 0) return KMI_OK;
  const uint64_t n = idx->n_entries;
  // enough workgroups to fill the device, at least sixteen entries per lane, and never more than 2^20 entries per workgroup
  uint64_t blocks = (n + 16 * kSpecThreads - 1) / (16 * kSpecThreads);
  const uint64_t most = (uint64_t)(ctx->n_cus ? ctx->n_cus : 256u) * 8u;
  blocks = blocks < most ? blocks : most;
  const uint64_t least = (n >> 20) + 1;
  blocks = blocks > least ? blocks : least;
  if (idx->bucket_cnt && blocks > (uint64_t)kNumFine / (kSpecThreads / kWave)) blocks = kNumFine / (kSpecThreads / kWave);
  {
    ProfScope ps(ctx, "count_spectrum", n);
    hipLaunchKernelGGL(count_spectrum_kernel, dim3((unsigned)blocks), dim3(kSpecThreads), 0, ctx->stream, (const uint32_t *)idx->vals, n,
                       (const uint64_t *)idx->bucket_off, (const uint32_t *)idx->bucket_cnt, n_bins, (unsigned long long *)hist_dev, tot);
  }
  KMI_HIP(ctx, hipGetLastError());
  return KMI_OK;
}
// waits for the stream
static kmi_status spectrum_totals(kmi_index *idx, kmi_spectrum_totals *totals) {
  kmi_ctx *ctx = idx->ctx;
  uint64_t t[3] = {0, 0, 0};
  KMI_HIP(ctx, hipMemcpyAsync(t, ctx->ws[WS_SPECTRUM].p, sizeof(t), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const bool any = idx->has_data && idx->n_entries;
  totals->n_entries = any ? idx->n_entries : 0;
  totals->sum_counts = t[SPEC_SUM];
  totals->max_count = any ? (uint32_t)t[SPEC_MAX] : 0u;
  totals->min_count = any ? ~(uint32_t)t[SPEC_NOTMIN] : 0u;
  return KMI_OK;
}

// rows / new_rows: the payload of bucket_retain_compact_kernel. *new_rows stays null when nothing leaves (the index and the rows
// stay as they are); else it is a fresh pool block of *new_rows_bytes, the caller's from then on.
template <int NW, int BITS>
static kmi_status retain_counts_impl(kmi_index *idx, uint32_t lo, uint32_t hi, uint64_t *n_erased, const uint32_t *rows, uint32_t **new_rows,
                                     size_t *new_rows_bytes) {
  kmi_ctx *ctx = idx->ctx;
  void *p;
  KMI_TRY(ws_get(ctx, WS_SPECTRUM, sizeof(uint64_t) * SPEC_WORDS + sizeof(uint32_t) * kNumFine, &p));
  uint64_t *tot = (uint64_t *)p;
  uint32_t *out_cnt = (uint32_t *)(tot + SPEC_WORDS);
  uint64_t *new_off = nullptr;
  KMI_HIP(ctx, pool_alloc(ctx, (void **)&new_off, kOffBytes));
  hipError_t e = hipMemsetAsync(tot, 0, sizeof(uint64_t) * SPEC_WORDS, ctx->stream);
  if (e == hipSuccess) {
    {
      ProfScope ps(ctx, "bucket_retain_count", idx->n_entries);
      hipLaunchKernelGGL(bucket_retain_count_kernel, dim3(kNumFine / (kRetainCountThreads / kWave)), dim3(kRetainCountThreads), 0, ctx->stream, (const uint32_t *)idx->vals, (const uint64_t *)idx->bucket_off,
                         (const uint32_t *)idx->bucket_cnt, lo, hi, out_cnt, (unsigned long long *)(tot + SPEC_FULLEST));
    }
    {
      ProfScope ps(ctx, "bucket_offsets", kNumFine);
      hipLaunchKernelGGL(bucket_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t *)out_cnt, new_off, tot, (int)SPEC_SURVIVORS);
    }
    e = hipGetLastError();
  }
  uint64_t t[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(t, tot + SPEC_SURVIVORS, sizeof(t), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { pool_free(ctx, new_off, kOffBytes); return set_err(ctx, KMI_ERR_DEVICE, "retain_counts: %s", hipGetErrorString(e)); }
  const uint64_t total = t[0];
  ctx->retain_fullest = t[1];
  if (total == idx->n_entries) {   // nothing to erase: the index stays exactly as it is (a sparse one sparse)
    pool_free(ctx, new_off, kOffBytes);
    return KMI_OK;
  }
  uint64_t *nk = nullptr; uint32_t *nv = nullptr;
  const size_t kb = (total ? total : 1) * NW * sizeof(uint64_t), vb = (total ? total : 1) * sizeof(uint32_t);
  hipError_t e1 = pool_alloc(ctx, (void **)&nk, kb);
  hipError_t e2 = pool_alloc(ctx, (void **)&nv, vb);
  uint32_t *nr = nullptr;
  const size_t rb = (total ? total : 1) * 8 * sizeof(uint32_t);
  hipError_t e3 = rows ? pool_alloc(ctx, (void **)&nr, rb) : hipSuccess;
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
    if (nk) pool_free(ctx, nk, kb);
    if (nv) pool_free(ctx, nv, vb);
    if (nr) pool_free(ctx, nr, rb);
    pool_free(ctx, new_off, kOffBytes);
    return set_err(ctx, KMI_ERR_NOMEM, "hipMalloc failed for the index arrays");
  }
  if (total) {
    ProfScope ps(ctx, "bucket_retain_compact", idx->n_entries);
    hipLaunchKernelGGL((bucket_retain_compact_kernel<NW>), dim3(kNumFine), dim3(kRetainTile), 0, ctx->stream, (const uint64_t *)idx->keys,
                       (const uint32_t *)idx->vals, (const uint64_t *)idx->bucket_off, (const uint32_t *)idx->bucket_cnt, lo, hi,
                       (const uint64_t *)new_off, nk, nv, (const uint4 *)rows, (uint4 *)nr);
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {   // the index stays as it was
    pool_free(ctx, nk, kb); pool_free(ctx, nv, vb); pool_free(ctx, new_off, kOffBytes);
    if (nr) pool_free(ctx, nr, rb);
    return set_err(ctx, KMI_ERR_DEVICE, "retain_counts: %s", hipGetErrorString(e));
  }
  // the old arrays go back to the pool as in densify_impl; layout_w, owner_lp, saturating and the configuration stay
  pool_free(ctx, idx->keys, idx->keys_bytes);
  pool_free(ctx, idx->vals, idx->vals_bytes);
  pool_free(ctx, idx->bucket_off, kOffBytes);
  if (idx->bucket_cnt) pool_free(ctx, idx->bucket_cnt, sizeof(uint32_t) * kNumFine);
  if (idx->dense_off) pool_free(ctx, idx->dense_off, kOffBytes);
  idx->keys = nk; idx->vals = nv; idx->bucket_off = new_off; idx->bucket_cnt = nullptr; idx->dense_off = nullptr;
  idx->keys_bytes = kb; idx->vals_bytes = vb;
  if (n_erased) *n_erased = idx->n_entries - total;
  idx->n_entries = total;
  if (rows) { *new_rows = nr; *new_rows_bytes = rb; }
  return KMI_OK;
}
static kmi_status index_retain_counts(kmi_index *idx, uint32_t lo, uint32_t hi, uint64_t *n_erased, const uint32_t *rows = nullptr,
                                      uint32_t **new_rows = nullptr, size_t *new_rows_bytes = nullptr) {
  KMI_DISPATCH(idx->shape, retain_counts_impl, idx, lo, hi, n_erased, rows, new_rows, new_rows_bytes);
}

}  // namespace kmi
