// Two count indexes joined on the device (no counterpart in the reference; KMC's `simple` operations and Jellyfish `merge` are the
// precedents):
//   kmi_index_compare   the eight words of kmi_index_overlap: sizes, shared keys, count sums over all and over the shared keys
//   kmi_index_combine   a := a (op) b for the seven KMI_COMBINE_* ops
// Two indexes of one k-mer shape and one layout (layout_w) put a key into the same fine bucket, so bucket b of A only has to meet
// bucket b of B: nothing is partitioned and no tag travels with a key. bucket_join_kernel builds the LDS table of B's bucket -- its
// entries are distinct, so the table's fill and the pass count are known before it is built, as in bucket_lookup_kernel -- and
// streams A's bucket against it once per pass. Compare folds its sums per lane, wavefront and workgroup; intersect / subtract write
// A's surviving entries, with their new counts, into a scratch at A's (dense) bucket offsets, and a scan plus one copy of the
// survivors alone puts them into fresh arrays (bucket_join_compact). The two unions are bucket_merge_kernel with B as the single
// part, whose bucket offsets are the part offsets as they stand.
//
// Included by kmi_index.hip after kmi_spectrum.h.
#pragma once

namespace kmi {

// device words of a compare behind the context's WS_SPECTRUM slot (n_a and n_b are the host's)
enum { OV_SHARED = 0, OV_SUM_A = 1, OV_SUM_B = 2, OV_SUM_A_SHARED = 3, OV_SUM_B_SHARED = 4, OV_SUM_MIN = 5, OV_ACC = 6, OV_SURVIVORS = 6, OV_WORDS = 8 };

struct JoinAcc {
  uint64_t v[OV_ACC];
};

// what becomes of A's entry (count ca) given B's verdict (found, cb; cb = 0 when absent): kept or not, and its new count
__device__ __forceinline__ bool join_verdict(uint32_t op, bool sat, uint32_t ca, bool found, uint32_t cb, uint32_t *v) {
  switch (op) {
    case KMI_COMBINE_INTERSECT_MIN: *v = ca < cb ? ca : cb; return found;
    case KMI_COMBINE_INTERSECT_ADD: { const uint32_t s = ca + cb; *v = (sat && s < ca) ? 0xffffffffu : s; return found; }
    case KMI_COMBINE_INTERSECT_LEFT: *v = ca; return found;
    case KMI_COMBINE_SUBTRACT_KEYS: *v = ca; return !found;
    default: *v = ca - cb; return ca > cb;   // KMI_COMBINE_SUBTRACT_COUNTS
  }
}

// Fine bucket b: table of B's entries (key -> count), then every entry of A's bucket against it. A bucket of B of more entries than
// the table takes runs in passes by pass_of(place_hash), B's entries and A's alike: an entry of A is answered in the pass its hash
// belongs to, hit or miss, so it is seen exactly once per attempt. B's entries are distinct, so an attempt with fewer than
// entries / limit passes cannot fit and is not tried; from there npass doubles, and an attempt that failed leaves nothing behind
// (the lane sums and the bucket's output cursor start again).
// COMPARE: the six sums into totals[OV_*]. Otherwise: A's survivors under `op` to out_keys / out_vals from out_off[b] on, in any
// order, and out_cnt[b] = how many. a_off / b_off == nullptr: that index holds nothing; a_cnt / b_cnt: sparse index (bucket b =
// cnt[b] entries from off[b]); cap_limit: home slots at most (KMI_LOOKUP_CAP).
template <int NW, bool COMPARE>
__global__ __launch_bounds__((QTabCfg<NW>::NT)) void bucket_join_kernel(const uint64_t *__restrict__ a_keys, const uint32_t *__restrict__ a_vals,
                                                                      const uint64_t *__restrict__ a_off, const uint32_t *__restrict__ a_cnt,
                                                                      const uint64_t *__restrict__ b_keys, const uint32_t *__restrict__ b_vals,
                                                                      const uint64_t *__restrict__ b_off, const uint32_t *__restrict__ b_cnt,
                                                                      uint32_t cap_limit, uint32_t op, bool sat, const uint64_t *__restrict__ out_off,
                                                                      uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_vals,
                                                                      uint32_t *__restrict__ out_cnt, unsigned long long *__restrict__ totals,
                                                                      uint32_t *__restrict__ over_limit, uint32_t *__restrict__ max_npass) {
  KMI_TABLE_LDS_CFG(NW, QTabCfg<NW>)
  __shared__ unsigned long long s_acc[OV_ACC];
  uint32_t *s_out = &s_ctl[4];
  const uint32_t b = blockIdx.x;
  const uint64_t ab = a_off ? a_off[b] : 0ull, ae = a_off ? (a_cnt ? ab + a_cnt[b] : a_off[b + 1]) : 0ull;
  const uint64_t bb = b_off ? b_off[b] : 0ull, be = b_off ? (b_cnt ? bb + b_cnt[b] : b_off[b + 1]) : 0ull;
  if (COMPARE ? (ab == ae && bb == be) : ab == ae) {
    if (!COMPARE && threadIdx.x == 0) out_cnt[b] = 0u;
    return;
  }
  const uint64_t na = ae - ab, nb = be - bb;
  const uint64_t o0 = COMPARE ? 0ull : out_off[b];
  {
    // twice B's entries of home slots, at least 512, at most what the knob allows
    uint32_t want = 2u * (uint32_t)(nb < (uint64_t)QTabCfg<NW>::CAP ? nb : (uint64_t)QTabCfg<NW>::CAP);
    want = (want + 255u) & ~255u;
    want = want < 512u ? 512u : want;
    want = want < cap_limit ? want : cap_limit;
    if (want < (uint32_t)QTabCfg<NW>::CAP) { tab.cap = want; tab.slots = want + QTabCfg<NW>::PAD; tab.limit = want * 3u / 4u; }
  }
  if (COMPARE && threadIdx.x < OV_ACC) s_acc[threadIdx.x] = 0ull;   // (behind the first pass's barrier before anyone adds)
  uint32_t npass = 1;
  while ((uint64_t)npass * tab.limit < nb && npass < kMaxPasses) npass *= 2;
  JoinAcc acc;
  while (true) {
#pragma unroll
    for (int j = 0; j < OV_ACC; ++j) acc.v[j] = 0ull;
    if (threadIdx.x == 0) *s_out = 0u;
    bool failed = false;
    for (uint32_t pass = 0; pass < npass && !failed; ++pass) {
      table_clear<NW>(tab);
      lds_barrier();
      for_each_key<NW, BatchOf<NW>::U>(b_keys, bb, be, [&](const uint64_t (&k)[NW], uint64_t i) {
        const uint32_t h = place_hash<NW>(k);
        if (pass_of(h, npass) != pass) return;
        const uint32_t cb = b_vals[i];
        if (COMPARE) acc.v[OV_SUM_B] += cb;
        const int s = table_upsert<NW>(tab, k, h);
        if (s >= 0) tab.vals[s] = cb; else if (s == -2) *tab.special = cb;
      });
      lds_barrier();
      if (*tab.overflow) { failed = true; break; }
      for_each_key<NW, BatchOf<NW>::U>(a_keys, ab, ae, [&](const uint64_t (&k)[NW], uint64_t i) {
        const uint32_t h = place_hash<NW>(k);
        if (pass_of(h, npass) != pass) return;
        const uint32_t ca = a_vals[i];
        const int s = table_find<NW>(tab, k, h);
        const bool found = s >= 0 || s == -2;
        const uint32_t cb = s >= 0 ? tab.vals[s] : (s == -2 ? *tab.special : 0u);
        if (COMPARE) {
          acc.v[OV_SUM_A] += ca;
          if (found) {
            acc.v[OV_SHARED] += 1u; acc.v[OV_SUM_A_SHARED] += ca; acc.v[OV_SUM_B_SHARED] += cb; acc.v[OV_SUM_MIN] += ca < cb ? ca : cb;
          }
        } else {
          uint32_t v;
          const bool keep = join_verdict(op, sat, ca, found, cb, &v);
          const uint32_t pos = wave_alloc(s_out, keep);
          if (keep && pos < na) {   // (the bound holds by construction: an attempt sees every entry of A once)
#pragma unroll
            for (int w = 0; w < NW; ++w) out_keys[(o0 + pos) * NW + w] = k[w];
            out_vals[o0 + pos] = v;
          }
        }
      });
      lds_barrier();
    }
    if (!failed) break;
    npass *= 2;
    if (npass > kMaxPasses) {
      if (threadIdx.x == 0) { atomicOr(over_limit, 1u); *s_out = 0u; }
#pragma unroll
      for (int j = 0; j < OV_ACC; ++j) acc.v[j] = 0ull;
      lds_barrier();
      break;
    }
    lds_barrier();
  }
  if (COMPARE) {
    // per lane -> per wavefront -> per workgroup, then one set of global atomics
#pragma unroll
    for (int j = 0; j < OV_ACC; ++j) {
      const uint64_t w = wave_reduce_sum(acc.v[j]);
      if (lane_id() == 0 && w) atomicAdd(&s_acc[j], (unsigned long long)w);
    }
    lds_barrier();
    if (threadIdx.x < OV_ACC && s_acc[threadIdx.x]) atomicAdd(&totals[threadIdx.x], s_acc[threadIdx.x]);
  }
  if (threadIdx.x == 0) {
    if (!COMPARE) out_cnt[b] = *s_out;
    atomicMax(max_npass, npass > kMaxPasses ? kMaxPasses : npass);
  }
}

static inline uint64_t setops_size(const kmi_index *idx) { return idx->has_data ? idx->n_entries : 0ull; }
static inline uint32_t setops_cap(kmi_ctx *ctx, uint32_t table_cap) {
  uint32_t cap = ctx->lookup_cap ? ctx->lookup_cap : table_cap;
  return cap < 64u ? 64u : (cap > table_cap ? table_cap : cap);
}
// the pass words of the call (the lookup's: every call that uses them clears them first)
static kmi_status setops_begin(kmi_ctx *ctx) {
  ctx->setops_npass = 0;
  KMI_HIP(ctx, hipMemsetAsync(ctx->d_flags + FLAG_LOOKUP_NPASS, 0, 2 * sizeof(uint32_t), ctx->stream));
  return KMI_OK;
}

template <int NW, int BITS>
static kmi_status compare_impl(kmi_index *a, kmi_index *b, kmi_index_overlap *out) {
  kmi_ctx *ctx = a->ctx;
  const uint64_t n_a = setops_size(a), n_b = setops_size(b);
  out->n_a = n_a; out->n_b = n_b;
  if (n_a == 0 && n_b == 0) return KMI_OK;
  // the smaller operand changes over when the layouts differ (its entries stay)
  if (n_a && n_b && a->layout_w != b->layout_w) {
    if (n_a <= n_b) KMI_TRY(ensure_layout(a, b->layout_w)); else KMI_TRY(ensure_layout(b, a->layout_w));
  }
  void *p;
  KMI_TRY(ws_get(ctx, WS_SPECTRUM, sizeof(uint64_t) * SPEC_WORDS + sizeof(uint32_t) * kNumFine, &p));
  unsigned long long *tot = (unsigned long long *)p;
  static_assert(OV_WORDS <= SPEC_WORDS, "the compare's words lie where the spectrum's do");
  KMI_HIP(ctx, hipMemsetAsync(tot, 0, sizeof(uint64_t) * OV_WORDS, ctx->stream));
  KMI_TRY(setops_begin(ctx));
  {
    ProfScope ps(ctx, "bucket_join", n_a + n_b);
    hipLaunchKernelGGL((bucket_join_kernel<NW, true>), dim3(kNumFine), dim3(QTabCfg<NW>::NT), 0, ctx->stream, (const uint64_t *)a->keys,
                       (const uint32_t *)a->vals, (const uint64_t *)(n_a ? a->bucket_off : nullptr), (const uint32_t *)a->bucket_cnt,
                       (const uint64_t *)b->keys, (const uint32_t *)b->vals, (const uint64_t *)(n_b ? b->bucket_off : nullptr),
                       (const uint32_t *)b->bucket_cnt, setops_cap(ctx, (uint32_t)QTabCfg<NW>::CAP), 0u, false, (const uint64_t *)nullptr,
                       (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, tot, ctx->d_flags + FLAG_LOOKUP_OVER,
                       ctx->d_flags + FLAG_LOOKUP_NPASS);
  }
  KMI_HIP(ctx, hipGetLastError());
  uint64_t t[OV_ACC] = {0, 0, 0, 0, 0, 0};
  uint32_t f[2] = {0, 0};
  KMI_HIP(ctx, hipMemcpyAsync(t, tot, sizeof(t), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipMemcpyAsync(f, ctx->d_flags + FLAG_LOOKUP_NPASS, sizeof(f), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->setops_npass = f[0];
  if (f[1]) return set_err(ctx, KMI_ERR_OVERFLOW, "a bucket could not be joined within the pass limit");
  out->n_shared = t[OV_SHARED]; out->sum_a = t[OV_SUM_A]; out->sum_b = t[OV_SUM_B];
  out->sum_a_shared = t[OV_SUM_A_SHARED]; out->sum_b_shared = t[OV_SUM_B_SHARED]; out->sum_min_shared = t[OV_SUM_MIN];
  return KMI_OK;
}
static kmi_status index_compare(kmi_index *a, kmi_index *b, kmi_index_overlap *out) { KMI_DISPATCH(a->shape, compare_impl, a, b, out); }

// intersect / subtract: a non-empty `a` against any b
template <int NW, int BITS>
static kmi_status combine_join_impl(kmi_index *a, kmi_index *b, uint32_t op) {
  kmi_ctx *ctx = a->ctx;
  const uint64_t n_a = a->n_entries, n_b = setops_size(b);
  if (n_b && a->layout_w != b->layout_w) KMI_TRY(ensure_layout(a, b->layout_w));
  // the survivors of bucket b go behind one another from the bucket's offset in the DENSE numbering of a, so the scratch has a's
  // entry count whatever a's form
  const uint64_t *out_off = a->bucket_cnt ? a->dense_off : a->bucket_off;
  void *p;
  KMI_TRY(ws_get(ctx, WS_SPECTRUM, sizeof(uint64_t) * SPEC_WORDS + sizeof(uint32_t) * kNumFine, &p));
  uint64_t *tot = (uint64_t *)p;
  KMI_TRY(ws_get(ctx, WS_TMP_KEYS, n_a * NW * sizeof(uint64_t), &p)); uint64_t *tmp_keys = (uint64_t *)p;
  KMI_TRY(ws_get(ctx, WS_TMP_VALS, n_a * sizeof(uint32_t), &p)); uint32_t *tmp_vals = (uint32_t *)p;
  KMI_TRY(ws_get(ctx, WS_BUCKET_CNT, sizeof(uint32_t) * kNumFine, &p)); uint32_t *out_cnt = (uint32_t *)p;
  KMI_TRY(setops_begin(ctx));
  uint64_t *new_off = nullptr;
  KMI_HIP(ctx, pool_alloc(ctx, (void **)&new_off, kOffBytes));
  {
    ProfScope ps(ctx, "bucket_join", n_a + n_b);
    hipLaunchKernelGGL((bucket_join_kernel<NW, false>), dim3(kNumFine), dim3(QTabCfg<NW>::NT), 0, ctx->stream, (const uint64_t *)a->keys,
                       (const uint32_t *)a->vals, (const uint64_t *)a->bucket_off, (const uint32_t *)a->bucket_cnt, (const uint64_t *)b->keys,
                       (const uint32_t *)b->vals, (const uint64_t *)(n_b ? b->bucket_off : nullptr), (const uint32_t *)b->bucket_cnt,
                       setops_cap(ctx, (uint32_t)QTabCfg<NW>::CAP), op, a->saturating, out_off, tmp_keys, tmp_vals, out_cnt,
                       (unsigned long long *)nullptr, ctx->d_flags + FLAG_LOOKUP_OVER, ctx->d_flags + FLAG_LOOKUP_NPASS);
  }
  {
    ProfScope ps(ctx, "bucket_offsets", kNumFine);
    hipLaunchKernelGGL(bucket_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t *)out_cnt, new_off, tot, (int)OV_SURVIVORS);
  }
  hipError_t e = hipGetLastError();
  uint64_t total = 0;
  uint32_t f[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(&total, tot + OV_SURVIVORS, sizeof(total), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(f, ctx->d_flags + FLAG_LOOKUP_NPASS, sizeof(f), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { pool_free(ctx, new_off, kOffBytes); return set_err(ctx, KMI_ERR_DEVICE, "combine: %s", hipGetErrorString(e)); }
  ctx->setops_npass = f[0];
  if (f[1] || total > n_a) {
    pool_free(ctx, new_off, kOffBytes);
    return set_err(ctx, KMI_ERR_OVERFLOW, "a bucket could not be joined within the pass limit");
  }
  uint64_t *nk = nullptr; uint32_t *nv = nullptr;
  const size_t kb = (total ? total : 1) * NW * sizeof(uint64_t), vb = (total ? total : 1) * sizeof(uint32_t);
  hipError_t e1 = pool_alloc(ctx, (void **)&nk, kb);
  hipError_t e2 = pool_alloc(ctx, (void **)&nv, vb);
  if (e1 != hipSuccess || e2 != hipSuccess) {
    if (nk) pool_free(ctx, nk, kb);
    if (nv) pool_free(ctx, nv, vb);
    pool_free(ctx, new_off, kOffBytes);
    return set_err(ctx, KMI_ERR_NOMEM, "hipMalloc failed for the index arrays");
  }
  if (total) {
    ProfScope ps(ctx, "bucket_join_compact", total);
    hipLaunchKernelGGL((bucket_compact_kernel<NW, uint32_t>), dim3(kNumFine), dim3(256), 0, ctx->stream, (const uint64_t *)tmp_keys,
                       (const uint32_t *)tmp_vals, out_off, (const uint64_t *)nullptr, (const uint64_t *)new_off, nk, nv);
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {   // a stays as it was
    pool_free(ctx, nk, kb); pool_free(ctx, nv, vb); pool_free(ctx, new_off, kOffBytes);
    return set_err(ctx, KMI_ERR_DEVICE, "combine: %s", hipGetErrorString(e));
  }
  // the old arrays go back to the pool as in retain_counts_impl; layout_w, owner_lp, saturating and the configuration stay
  pool_free(ctx, a->keys, a->keys_bytes);
  pool_free(ctx, a->vals, a->vals_bytes);
  pool_free(ctx, a->bucket_off, kOffBytes);
  if (a->bucket_cnt) pool_free(ctx, a->bucket_cnt, sizeof(uint32_t) * kNumFine);
  if (a->dense_off) pool_free(ctx, a->dense_off, kOffBytes);
  a->keys = nk; a->vals = nv; a->bucket_off = new_off; a->bucket_cnt = nullptr; a->dense_off = nullptr;
  a->keys_bytes = kb; a->vals_bytes = vb;
  a->n_entries = total;
  return KMI_OK;
}

// the unions: a non-empty b merged into any a. bucket_merge_kernel reads its part and the index by bucket_off[b] .. bucket_off[b + 1],
// so both operands are dense here.
template <int NW, int BITS>
static kmi_status combine_union_impl(kmi_index *a, kmi_index *b, uint32_t op) {
  kmi_ctx *ctx = a->ctx;
  KMI_TRY(ensure_dense(b));
  KMI_TRY(ensure_dense(a));
  if (a->layout_w != b->layout_w) KMI_TRY(ensure_layout(a, b->layout_w));   // (an empty a just takes the name)
  const uint64_t n_a = setops_size(a), n_b = b->n_entries;
  void *p;
  KMI_TRY(ws_get(ctx, WS_SPLIT_OFF, sizeof(uint64_t) * 2, &p)); uint64_t *base = (uint64_t *)p;   // the single part begins at 0
  const uint64_t cap = n_a + n_b;
  KMI_TRY(ws_get(ctx, WS_TMP_KEYS, cap * NW * sizeof(uint64_t), &p)); uint64_t *tmp_keys = (uint64_t *)p;
  KMI_TRY(ws_get(ctx, WS_TMP_VALS, cap * sizeof(uint32_t), &p)); uint32_t *tmp_vals = (uint32_t *)p;
  KMI_TRY(ws_get(ctx, WS_BUCKET_CNT, sizeof(uint32_t) * kNumFine, &p)); uint32_t *out_cnt = (uint32_t *)p;
  KMI_HIP(ctx, hipMemsetAsync(base, 0, sizeof(uint64_t) * 2, ctx->stream));
  KMI_TRY(setops_begin(ctx));
  const uint64_t *old_off = n_a ? a->bucket_off : nullptr;
  {
    ProfScope ps(ctx, "bucket_merge", n_b);
    hipLaunchKernelGGL((bucket_merge_kernel<NW>), dim3(kNumFine), dim3(TabCfg<NW>::NT), 0, ctx->stream, (const uint64_t *)b->keys,
                       (const uint32_t *)b->vals, 1u, (const uint64_t *)base, (const uint64_t *)b->bucket_off, (const uint64_t *)b->bucket_off,
                       (const uint64_t *)a->keys, (const uint32_t *)a->vals, old_off, tmp_keys, tmp_vals, out_cnt, ctx->d_flags, a->saturating,
                       op == KMI_COMBINE_UNION_MAX, ctx->d_flags + FLAG_LOOKUP_NPASS);
  }
  KMI_HIP(ctx, hipGetLastError());
  KMI_TRY((adopt_tmp<NW>(a, tmp_keys, tmp_vals, b->bucket_off, old_off, out_cnt)));
  uint32_t f = 0;
  KMI_HIP(ctx, hipMemcpyAsync(&f, ctx->d_flags + FLAG_LOOKUP_NPASS, sizeof(f), hipMemcpyDeviceToHost, ctx->stream));
  KMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->setops_npass = f;
  return KMI_OK;
}

template <int NW, int BITS>
static kmi_status combine_impl(kmi_index *a, kmi_index *b, uint32_t op) {
  a->ctx->setops_npass = 0;
  const uint64_t n_a = setops_size(a), n_b = setops_size(b);
  if (op == KMI_COMBINE_UNION_ADD || op == KMI_COMBINE_UNION_MAX) {
    if (n_b == 0) return KMI_OK;
    return combine_union_impl<NW, BITS>(a, b, op);
  }
  if (n_a == 0) return KMI_OK;
  // (an empty b takes no key away; SUBTRACT_COUNTS still drops a's stored zeros -- ca > 0 fails -- and goes the general way)
  if (n_b == 0 && op == KMI_COMBINE_SUBTRACT_KEYS) return KMI_OK;
  return combine_join_impl<NW, BITS>(a, b, op);
}
static kmi_status index_combine(kmi_index *a, kmi_index *b, uint32_t op) { KMI_DISPATCH(a->shape, combine_impl, a, b, op); }

// the operands' rules; nothing is touched
static kmi_status setops_check(kmi_index *a, kmi_index *b, const char *what) {
  kmi_ctx *ctx = a->ctx;
  if (a->val_words || b->val_words) return set_err(ctx, KMI_ERR_INVALID, "%s() is a member of the count index", what);
  if (a->ctx != b->ctx) return set_err(ctx, KMI_ERR_INVALID, "%s: the indexes belong to different contexts", what);
  if (a->cfg.k != b->cfg.k || a->cfg.alphabet != b->cfg.alphabet || a->cfg.strand != b->cfg.strand)
    return set_err(ctx, KMI_ERR_INVALID, "%s: the indexes differ in k, alphabet or strand model", what);
  if (a->owner_lp != b->owner_lp) return set_err(ctx, KMI_ERR_INVALID, "%s: the indexes differ in their owner ranks", what);
  return KMI_OK;
}

}  // namespace kmi
