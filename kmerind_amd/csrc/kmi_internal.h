// kmi_internal.h -- host-side context, workspace and launch helpers (not part of the ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/kmerind_hip.h"
#include "kmi_device.h"

namespace kmi {

// output hits a workgroup of the segmented copy of kmi_query_dist.h owns (kmi_ctx_debug_counter 11: tests make segments cross it)
constexpr int kSegCopyThreads = 256, kSegCopyPerThread = 8, kSegCopyTile = kSegCopyThreads * kSegCopyPerThread;

enum WsSlot {
  WS_TILE_INFO = 0,   // per-tile scan records
  WS_TILE_BASE,       // per-tile line bases
  WS_TILE_OFF,        // per-tile output offsets
  WS_KEYS_A,          // key ping buffer
  WS_KEYS_B,          // key pong buffer
  WS_HIST,            // fine histogram / offsets
  WS_WGHIST,          // per-workgroup coarse histograms
  WS_CURSOR,          // coarse / fine cursors
  WS_TMP_KEYS,        // per-bucket reduce output (keys)
  WS_TMP_VALS,        // per-bucket reduce output (values)
  WS_BUCKET_CNT,      // per-bucket distinct counts
  WS_BUCKET_OFF,      // scanned
  WS_QUERY_A,
  WS_QUERY_B,
  WS_INPUT,           // host-entry staging of input bytes / keys
  WS_OUTPUT,          // host-entry staging of outputs
  WS_OUTPUT2,
  WS_INPUT2,
  WS_MISC,
  WS_TILE_HDR,        // per-tile position of the last record start before the tile
  WS_QUALS,           // k-mer qualities of the extracted tuples
  WS_READS,           // read descriptors for the quality pass
  WS_FA_IDS,          // LongSequenceKmerId of every compacted FASTA character
  WS_PK_EOL,          // EOL bitmap of the scanned input
  WS_PK_STREAM,       // packed complement-code stream of the scanned input
  WS_ENT_BKT,         // rank bucket of the 8 windows of every entry, one byte each (fused extract + route)
  WS_ENT_LIST,        // entry list: runs of <= 8 consecutive windows, per-tile slots (fused build)
  WS_ENT_CNT,         // entries per scan tile
  WS_PK_BRK,          // window-break bitmap (EOL or N) of the scanned input (N_FILTER / N_SPLIT)
  WS_PK_NB,           // N bitmap and pure EOL bitmap of the pre-pass (N_FILTER)
  WS_SPLIT_RANK,      // destination rank of every index entry (split by rank)
  WS_SPLIT_OFF,       // per-part bucket offsets, part totals and bases (split / merge)
  WS_SK_ITEMS,        // super-k-mer items of the minimizer pass (fused build through super-k-mers)
  WS_DIST_A,          // the collectives over ranks (kmi_index_*_dist_*): send / receive / result buffers
  WS_DIST_B,
  WS_DIST_C,
  WS_DIST_D,
  WS_DBG_RECS,        // de Bruijn node build: (k-mer, edge) records of the parsed input
  WS_DBG_OLD,         // ... keys and bucket offsets of the nodes before an insert (their edge counts move to the new order)
  WS_DBG_POS,         // ... entry positions of the nodes a find() hit
  WS_ALIGNED,         // 16-byte aligned copy of an input buffer that arrived at an odd address (a batch inside a larger buffer)
  WS_UNI_TAB,         // unitig compaction (kmi_unitig.h): entry-position table of the neighbour lookups
  WS_UNI_NEXT,        // ... next state of every (node, direction)
  WS_UNI_RANK,        // ... ranking records, two halves (ping-pong; the idle half holds the cycle pass and the scan)
  WS_UNI_NODE,        // ... device scalars, per-node direction and circular flags
  WS_UNI_SCAN,        // unitig compaction over ranks (kmi_unitig_dist.h): (heads, bases) of every node and the scan's tile sums
  WS_UNI_STAGE,       // ... staged 16-byte records of every state before they are grouped by rank; the link requests
  WS_UNI_END,         // ... cycle candidates, then the end k-mer and end occurrences of every state
  WS_UNI_CNT,         // ... records per destination rank, cursors, device scalars
  WS_DBG_TIPS,        // tip clipping (kmi_dbg_tips.h): device scalars, survivors of every fine bucket, per-unitig junctions, per-node masks and classes
  WS_DBG_BUBBLES,     // bubble popping (kmi_dbg_bubbles.h): the same, with two junctions per unitig and a verdict byte beside the class; over ranks (kmi_dbg_bubbles_dist.h) junction words per state and a record index per counter
  WS_LOOKUP_RECS,    // positional lookup / read profile (kmi_lookup.h): (key words, tag) records of the queries or of a batch's k-mers
  WS_LOOKUP_CNT,      // ... the looked-up count of every k-mer of a batch, in file order
  WS_SPECTRUM,        // count spectrum / count filter (kmi_spectrum.h): the call's device scalars, then the survivors of every fine bucket
  WS_LOCATE_POS,      // locate / seed_reads (kmi_locate.h): entry positions of every fine bucket grouped by key, one u32 per index entry
  WS_LOCATE_SCAN,     // ... tile sums of the device-wide scans
  WS_LOCATE_OFF,      // ... offsets[] of a batch's windows, or of the host form's queries
  WS_QD_PERM,         // queries in the caller's order over ranks (kmi_query_dist.h): perm[j] = the query that sits at routed place j
  WS_QD_SLOT,         // ... slot[i] = the routed place of query i (the inverse of perm)
  WS_QD_ANS,          // ... the answers (count / occ, 4 bytes) that came back, in routed order
  WS_QD_OFFS,         // ... routed-order offsets rebuilt from the returned occ
  WS_QD_VALS,         // ... the value words that came back: a CSR in routed order
  WS_QD_RANS,         // ... owner side: count / occ of every received key
  WS_QD_ROFFS,        // ... owner side: offsets over the received keys, all sources concatenated
  WS_QD_RVALS,        // ... owner side: the listed value words of the received keys
  WS_NUM_SLOTS
};

// ---- the device scalars of a context: who owns which word. Every index into d_flags, d_totals and h_totals goes through these names
// (a word a kernel gets as `base + NAME` it indexes from 0: sk_front_verify_kernel's three totals at TOT_FRONT).
// d_flags: FLAG_NUM_WORDS dwords. Kernels raise them with atomics; the host reads a word and clears it where it acts on it.
// Words 0 .. 15 live within ONE call: whoever raises one is read (and answered) before that call returns, so every scan and the
// one-pass front end start by clearing all sixteen ([FZ_SCAN_0, FZ_SCAN_1), [FZ_FRONT_0, FZ_FRONT_1)) -- the words of the reduce
// and of the tuple kernels among them (FLAG_PASS_LIMIT, FLAG_ID_OVERFLOW, FLAG_REDUCE_CHECK, FLAG_OUT_OVERFLOW), on purpose.
enum FlagWord : uint32_t {
  FLAG_PARSE = 0,           // FASTQ record rules, bits 1 / 2 / 4 / 8: the scan kernels and fastq_list_kernel raise them; fastq_scan clears; read_totals, fastq_length_verdict read
  FLAG_OUT_OVERFLOW = 1,    // the extract kernels: more tuples than the output holds; cleared with the scan's words; extract_run reads
  FLAG_PASS_LIMIT = 2,      // bucket_reduce_kernel / sk_reduce_kernel: a bucket went over the pass limit; adopt_tmp reads and clears
  FLAG_ID_OVERFLOW = 3,     // the tuple kernels: a ShortSequenceKmerId increment overflowed; the position builds read and clear
  FLAG_REDUCE_CHECK = 8,    // bucket_reduce_kernel: "a bucket overflowed, later buckets check"; reduce_and_adopt clears before the launch
  FLAG_SK_DECLINED = 9,     // super-k-mer front ends: not this path's input (sk_minimizer, fasta_runs: 1 / 2 a capacity; sk_front, sk_front_verify: 4);
                            // sk_zero_kernel (one-pass) or a fill (general) clears; the front ends read, sk_scatter_rows_kernel reads on the device
  FLAG_SK_WHY = 10,         // sk_front_kernel: the reasons it declined (KMI_FRONT_DEBUG prints them); cleared with FLAG_SK_DECLINED
  FLAG_FRONT_QUEUE = 12,    // sk_front_kernel: the next byte range to hand out; sk_zero_kernel clears before the launch
  FLAG_SK_LEVEL0 = 16,      // sk_reduce_kernel: buckets that ended at level 0 .. 8 (9 words); sk_back_end clears and reads (the next build's hint)
  FLAG_SK_LEVEL_END = 34,   // (words 25 .. 33 are cleared with the votes and unused)
  FLAG_SK_ROOM = 34,        // sk_scatter_fine_slack_lines_kernel: a fine bucket outgrew its room; sk_zero_kernel clears; sk_back_end reads
  FLAG_LOOKUP_NPASS = 36,   // bucket_lookup_kernel, bucket_locate_*_kernel: the largest pass count of the call's buckets; lookup clears and reads
  FLAG_LOOKUP_OVER = 37,    // bucket_lookup_kernel, bucket_locate_*_kernel: a bucket went over the pass limit; lookup clears and reads
  FLAG_REDUCE_QUEUE = 40,   // sk_reduce_kernel: the next fine bucket to hand out (41 .. 47 spare, cleared with it); sk_back_end clears
  FLAG_REDUCE_QUEUE_END = 48,
  FLAG_CLOCKS = 48,         // timing builds (KMI_FR_TIMING, KMI_SK_TIMING): 8 64-bit wave clocks; the reports read and clear them
  FLAG_NUM_WORDS = 64,
  // the flag ranges cleared in one go: by the fill that starts every scan (kmi_extract.hip) [FZ_SCAN_0, FZ_SCAN_1); by sk_zero_kernel
  // the one-pass front end's [FZ_FRONT_0, FZ_FRONT_1), the slack back end's [FZ_BACK_0, FZ_BACK_1) and [FZ_BACK_2, FZ_BACK_3)
  FZ_SCAN_0 = 0, FZ_SCAN_1 = 16, FZ_FRONT_0 = 0, FZ_FRONT_1 = 16, FZ_BACK_0 = 16, FZ_BACK_1 = 35, FZ_BACK_2 = 40, FZ_BACK_3 = 48
};
static_assert(FZ_SCAN_0 == FZ_FRONT_0 && FZ_SCAN_1 == FZ_FRONT_1 && FLAG_REDUCE_CHECK < FZ_SCAN_1,
              "a scan and the one-pass front end clear the same per-call words, and nothing of the back end or the lookup (below)");
static_assert(FZ_FRONT_0 <= FLAG_PARSE && FLAG_SK_DECLINED < FZ_FRONT_1 && FLAG_SK_WHY < FZ_FRONT_1 && FLAG_FRONT_QUEUE < FZ_FRONT_1,
              "the front end's launch clears the parse flags, its verdict words and its range queue");
static_assert(FZ_FRONT_1 <= FLAG_SK_LEVEL0, "... and none of the back end's words");
static_assert(FZ_BACK_0 == FLAG_SK_LEVEL0 && FZ_BACK_1 == FLAG_SK_ROOM + 1 && FLAG_SK_LEVEL_END == FLAG_SK_ROOM,
              "the back end's first range: the level votes and the room flag, nothing else");
static_assert(FZ_BACK_1 <= FLAG_LOOKUP_NPASS && FLAG_LOOKUP_OVER == FLAG_LOOKUP_NPASS + 1 && FLAG_LOOKUP_OVER < FZ_BACK_2,
              "the lookup's two words lie together (one fill, one read-back) and outside both ranges");
static_assert(FZ_BACK_2 == FLAG_REDUCE_QUEUE && FZ_BACK_3 == FLAG_REDUCE_QUEUE_END && FLAG_REDUCE_QUEUE_END <= FLAG_CLOCKS,
              "the back end's second range: the queue word and its spare words, not the clocks");
static_assert(FLAG_SK_LEVEL0 + 9 <= FLAG_SK_LEVEL_END && FLAG_CLOCKS + 16 <= FLAG_NUM_WORDS, "the votes and the clocks fit");

// d_totals: 16 64-bit words, then 256 coarse-bucket totals. h_totals (pinned): their mirror, then the mailbox.
enum TotalWord : uint32_t {
  TOT_LINES = 0,            // FASTQ scan: lines. The scan kernels write words 0 .. 2; read_totals reads them (h_totals mirrors words 0 .. 3 under these names)
  TOT_FA_CHARS = 0,         // FASTA scan: sequence characters (the same word: a context scans one format at a time); fasta_scan reads
  TOT_TUPLES = 1,           // FASTQ scan: k-mer windows
  TOT_FA_DROPPED = 1,       // FASTA scan: records dropped by the filter (the same word: a FASTA scan has no tuple total); fasta_scan clears and reads
  TOT_SEQS = 2,             // sequences / records; the filter count and the quality pass rewrite and read it on the device
  TOT_FA_VALID = 3,         // FASTA compaction: characters whose byte lies in the valid range
  TOT_SCAN_WORDS = 4,       // (words 0 .. 3 come back in one copy: read_totals, fasta_scan)
  TOT_ENTRIES = 4,          // bucket_offsets_kernel: entries of the index after a reduce or an erase; adopt_tmp and the erase read (read_total)
  TOT_RESULTS = 5,          // bucket_offsets_kernel: results of a count / find; the queries read (read_total)
  TOT_SK_KMERS = 6,        // k-mers of a super-k-mer build: sk_front / fasta_runs / sk_recv_hist add; sk_zero_kernel or a fill clears; the front ends read
  TOT_UPDATED = 7,          // update kernels: entries changed; update clears and reads
  TOT_BATCH_END = 8,        // fastq_batch_end_kernel writes; fastq_batch_end reads
  TOT_LOCATE_HITS = 9,      // scan_tile_bases_kernel (kmi_locate.h): the listed hits up to the end of the call's / batch's queries; locate_read_total reads
  TOT_FRONT = 12,           // sk_front_verify_kernel: lines, runs, items (3 words); sk_front_fast reads
  TOT_COARSE = 16,          // fine_totals_kernel: [256] coarse totals of the fine-offset scan (launch_fine_offsets)
  TOT_NUM_WORDS = 16 + 256
};
// one owner per total word: the named words in ascending order with nothing between two of them unaccounted for (10, 11 and 15 are free)
static_assert(TOT_FA_VALID + 1 == TOT_SCAN_WORDS && TOT_SCAN_WORDS == TOT_ENTRIES && TOT_ENTRIES + 1 == TOT_RESULTS &&
              TOT_RESULTS + 1 == TOT_SK_KMERS && TOT_SK_KMERS + 1 == TOT_UPDATED && TOT_UPDATED + 1 == TOT_BATCH_END &&
              TOT_BATCH_END + 1 == TOT_LOCATE_HITS && TOT_LOCATE_HITS < TOT_FRONT && TOT_FRONT + 3 <= TOT_COARSE && TOT_COARSE + 256 == TOT_NUM_WORDS,
              "one owner per total word");
// h_totals: words 0 .. 15 mirror d_totals under the TotalWord names (read_totals, fasta_scan, read_total copy word for word);
// the words below are the host's own
enum HostWord : uint32_t {
  H_BATCH_END = 8,          // mirror of TOT_BATCH_END (read at once, behind a synchronisation)
  H_SK_LEVELS = 8,          // sk_back_end: the 9 level votes, words 8 .. 12 (queued, read after adopt_tmp's synchronisation). Shares word 8 with
                            // H_BATCH_END: both are read before the host thread queues anything else into them
  H_SK_ROOM = 14,           // sk_back_end: FLAG_SK_ROOM
  H_MAIL = 16,              // sk_front_fast's read-backs, one synchronisation for all of them:
  H_MAIL_CNT = H_MAIL,             // [256] records and [256] starts of the coarse groups
  H_MAIL_DECLINED = H_MAIL + 512,  // FLAG_SK_DECLINED
  H_MAIL_FRONT = H_MAIL + 513,     // TOT_FRONT's three words
  H_MAIL_KMERS = H_MAIL + 516,     // TOT_SK_KMERS
  H_NUM_WORDS = 16 + 1024
};
static_assert(H_BATCH_END == (uint32_t)TOT_BATCH_END && H_SK_LEVELS > (uint32_t)TOT_RESULTS && H_SK_LEVELS + 5 <= H_SK_ROOM &&
              H_SK_ROOM < H_MAIL && H_MAIL == (uint32_t)TOT_COARSE && H_MAIL_KMERS < H_NUM_WORDS,
              "the read-backs of a build overlap neither each other nor the mirrored totals a build reads (entries, results)");

struct ProfRec {
  const char *name;
  hipEvent_t e0, e1;
  uint64_t units;
};

struct ProfAgg {
  const char *name;
  double total_ms;
  uint64_t launches, units;
};

}  // namespace kmi

struct kmi_ctx {
  int device = 0, rank = 0, nranks = 1;
  hipStream_t stream = nullptr;
  std::string err;
  struct Buf { void *p = nullptr; size_t cap = 0; } ws[kmi::WS_NUM_SLOTS];
  uint32_t *d_flags = nullptr;   // [FLAG_NUM_WORDS] error / overflow flags, votes, queue words: enum FlagWord names every word and its owner
  uint32_t n_cus = 0;            // compute units of the device (grids of persistent workgroups)
  uint64_t *d_totals = nullptr;  // [16] small device scalars + [256] coarse-bucket totals of the fine-offset scan (enum TotalWord)
  hipEvent_t ev_mail = nullptr;  // marks "the read-backs queued so far have landed" (waited for instead of the whole stream)
  // a build from HOST bytes whose copy has not been queued yet (kmi_index_build_host): the one-pass front end queues it in chunks
  // on copy_stream and starts the byte ranges of a chunk behind it; every other reader of the input calls feed_flush first
  const uint8_t *feed_host = nullptr; uint8_t *feed_dev = nullptr; size_t feed_bytes = 0;
  hipStream_t copy_stream = nullptr;
  hipEvent_t feed_ev[17] = {};
  // the de Bruijn node build through super-k-mers (kmi_debruijn.h): the front end makes records that carry their two outside bases, and
  // the back end leaves word where the fine buckets' records lie (they stay in the workspace until the next build) for the edge pass
  bool edge_records = false;
  bool dbg_superkmer = true;     // KMI_DBG_SUPERKMER=0: the node build always takes the tuple path
  struct { const uint64_t *recs = nullptr, *rec_off = nullptr, *region = nullptr; const uint32_t *cap = nullptr, *cnt = nullptr; bool valid = false; } sk_left;
  bool lines_p2 = true;          // the fine pass of the position builds writes whole lines (scatter_lines_records); KMI_LINES_P2=0: the plain form
  bool host_overlap = true;      // KMI_HOST_OVERLAP=0: one copy on the build's stream, then the build
  size_t host_overlap_min = (size_t)64 << 20;   // ... and inputs below this many bytes always go that way (KMI_HOST_OVERLAP_MIN; tests lower it)
  size_t feed_min_chunk = (size_t)8 << 20;      // a copy chunk is not split further below this (KMI_FEED_MIN_CHUNK)
  uint64_t *h_totals = nullptr;  // pinned mirror: 16 words of totals, then 1024 words for larger read-backs (one synchronisation for all of them; enum HostWord)
  bool prof = false;
  std::vector<kmi::ProfRec> prof_pending;
  std::vector<kmi::ProfAgg> prof_agg;
  std::vector<hipEvent_t> event_pool;
  // released index arrays kept for the next build of the same size (a repeated build / clear cycle then never
  // reaches hipMalloc / hipFree, whose cost on a loaded node is unpredictable)
  struct Spare { void *p; size_t bytes; };
  std::vector<Spare> spare;
  bool fused_superkmer = true;   // fused count-index build through super-k-mers (KMI_FUSED_PATH=kmer in the environment: the k-mer pipeline)
  bool force_dist = false;       // KMI_FORCE_DIST=1: the *_dist_* entry points run their exchange even with one rank (RCCL self exchange: tests)
  uint32_t sk_level_hint = 0;    // sk_reduce: filter bits the buckets of the next build start with (majority of the last build)
  float sk_inv_dup = 0.f;        // sk_reduce: distinct k-mers per k-mer occurrence of the last build (a bucket's expected fill; 0: unknown)
  uint64_t alloc_us = 0, alloc_bytes = 0, alloc_calls = 0, alloc_reused = 0;   // time inside hipMalloc / hipFree, bytes and calls that reached hipMalloc, blocks taken from the process-wide cache (kmi_ctx_debug_counter 1..4)
  uint32_t dist_pool_regrows = 0;     // times a build over ranks had to enlarge its receive pool (kmi_ctx_debug_counter: tests)
  uint64_t unitig_dist_rounds = 0, unitig_dist_exchanges = 0, unitig_dist_bytes = 0;   // the last kmi_dbg_compact_dist_host: jumping rounds, exchanges, bytes this rank sent (kmi_ctx_debug_counter 5..7)
  uint32_t dist_pool_pct = 100;      // the estimate itself, in percent (KMI_DIST_POOL_PCT: tests make it too small)
  uint64_t dist_pool_slack = 65536;   // records a rank's receive pool holds beyond the estimate of its share (KMI_DIST_POOL_SLACK: tests shrink it so that the pool has to grow)
  uint32_t dist_chunks = 4;      // record-aligned chunks of a rank's share in the build over ranks (exchange of one beside the front end of the next; KMI_DIST_CHUNKS)
  bool tuples_from_parse = true; // position / position + quality builds partition their tuples straight from the parse (kmi_tuples.h); KMI_TUPLES=extract: extract, then partition
  bool sk_slack = true;          // fine buckets with room instead of a counting pass (sk_scatter_fine_slack_lines_kernel: whole lines + pad records); KMI_SK_SLACK=0: always count
  bool front_fused = true;       // FASTQ front end of the super-k-mer build in one pass (kmi_front.h); KMI_FRONT=general: scan + list + minimizer
  uint32_t front_waves = 0;      // resident wavefronts of the front kernel (ranges of a large input); 0: not asked yet
  uint64_t front_min_range = 64ull << 10;   // smallest byte range of a wavefront (KMI_FRONT_MIN_RANGE: tests shrink it)
  uint32_t front_ranges_per_wave = 4;       // byte ranges per resident wavefront of a large input: handed out from a queue (KMI_FRONT_RANGES_PER_WAVE)
  uint32_t front_max_waves = 0;             // most wavefronts the front kernel is launched with; 0: as many as are resident (KMI_FRONT_MAX_WAVES: tests make few take many ranges)
  uint64_t sparse_min = 1ull << 26;   // output slots from which a super-k-mer build leaves its index in the sparse form (KMI_SPARSE_MIN)
  int sk_dbg = 0;                // KMI_SK_DBG=7 (test knob): the super-k-mer front end reports a capacity as exceeded
  bool fa_part_set = false;      // kmi_ctx_set_fasta_partition
  kmi_fasta_partition fa_part{};
  uint32_t lookup_cap = 0;       // home slots of the tables of bucket_lookup_kernel, bucket_locate_*_kernel and the set operations (KMI_LOOKUP_CAP: tests reach the multi-pass code with a small index); 0: the table's own
  size_t profile_batch = (size_t)256 << 20;   // input bytes of a batch of kmi_index_profile_reads_* (KMI_PROFILE_BATCH)
  uint64_t lookup_npass = 0;     // the largest pass count a bucket used in the last lookup / profile / locate / seed_reads (kmi_ctx_debug_counter 8)
  uint64_t bubbles_dist_exchanges = 0, bubbles_dist_bytes = 0;   // the last kmi_dbg_pop_bubbles_dist_host: the same (kmi_ctx_debug_counter 16, 17)
  uint64_t bubbles_dist_stage_exchanges = 0, bubbles_dist_stage_bytes = 0;   // ... of which its unitig stages' (18, 19)
  uint64_t tips_dist_exchanges = 0, tips_dist_bytes = 0;   // the last kmi_dbg_clip_tips_dist_host: exchanges, bytes this rank sent, stages included (kmi_ctx_debug_counter 14, 15)
  uint64_t prune_dist_bytes = 0;   // bytes this rank sent in the last kmi_dbg_prune_edges_dist_host (kmi_ctx_debug_counter 13)
  uint64_t retain_fullest = 0;   // entries of the fullest bucket the last kmi_index_retain_counts met (kmi_ctx_debug_counter 9)
  uint64_t setops_npass = 0;     // the largest pass count a bucket used in the last kmi_index_compare / kmi_index_combine (kmi_ctx_debug_counter 10)
  uint64_t qd_answered = 0;      // keys this rank answered as their owner in the last lookup / profile / locate / seed_reads over ranks (kmi_ctx_debug_counter 12)
  int fa_left_carry = -1;        // de Bruijn tuples of a FASTA block (kmi_dbg_build_fasta_range_dist_host): the raw byte of the sequence
                                 // character before the block's first one, the in-edge of its first window; -1: none
};

namespace kmi {

// hipMalloc / hipFree of the library's large blocks, timed, behind a process-wide cache per device (kmi_api.hip): what a context
// gives back when it is destroyed waits there for the next context of the same device instead of going through hipFree and
// hipMalloc again -- on a loaded node a fresh context's first build otherwise pays hundreds of milliseconds for its workspace.
// dev_malloc takes a cached block of at least `bytes` and at most 1.5 x that; *got receives the block's real size.
hipError_t dev_malloc(kmi_ctx *ctx, void **p, size_t bytes, size_t *got = nullptr);
void dev_free(kmi_ctx *ctx, void *p);                       // hipFree, timed
void dev_retire(kmi_ctx *ctx, void *p, size_t bytes);       // into the process-wide cache (hipFree when that is full)

// device blocks of the index arrays: exact-size reuse from the context's spare list, else hipMalloc
inline hipError_t pool_alloc(kmi_ctx *ctx, void **p, size_t bytes) {
  if (bytes == 0) bytes = 256;
  for (size_t i = 0; i < ctx->spare.size(); ++i)
    if (ctx->spare[i].bytes == bytes) { *p = ctx->spare[i].p; ctx->spare.erase(ctx->spare.begin() + (long)i); return hipSuccess; }
  hipError_t e = dev_malloc(ctx, p, bytes);   // (index arrays are asked for by exact size: a cached block must match it)
  if (e != hipSuccess && !ctx->spare.empty()) {   // give the cached blocks back and retry once
    for (auto &b : ctx->spare) dev_free(ctx, b.p);
    ctx->spare.clear();
    e = dev_malloc(ctx, p, bytes);
  }
  return e;
}
inline void pool_free(kmi_ctx *ctx, void *p, size_t bytes) {
  if (!p) return;
  if (bytes == 0) bytes = 256;
  // a few blocks wait here for the next owner (an index's arrays, a workspace slot: ws_get). When the list is full the SMALLEST one
  // goes -- offset / count tables of a few hundred KB come and go with every build and must not push out the multi-GB buffers a
  // sparse index hands back (giving those to hipFree and asking hipMalloc for them again costs hundreds of milliseconds per build)
  constexpr size_t kMaxSpare = 12;
  if (ctx->spare.size() >= kMaxSpare) {
    size_t m = 0;
    for (size_t i = 1; i < ctx->spare.size(); ++i) if (ctx->spare[i].bytes < ctx->spare[m].bytes) m = i;
    if (ctx->spare[m].bytes >= bytes) { dev_free(ctx, p); return; }   // (the newcomer is the smallest)
    dev_free(ctx, ctx->spare[m].p);
    ctx->spare.erase(ctx->spare.begin() + (long)m);
  }
  ctx->spare.push_back({p, bytes});
  // ... and the list never holds more than 32 GB: the OLDEST blocks go first then (the arrays of a multimap that grows batch by
  // batch come back in sizes nobody asks for again)
  constexpr size_t kMaxSpareBytes = 32ull << 30;
  size_t total = 0;
  for (const auto &b : ctx->spare) total += b.bytes;
  while (total > kMaxSpareBytes && !ctx->spare.empty()) {
    total -= ctx->spare.front().bytes;
    dev_free(ctx, ctx->spare.front().p);
    ctx->spare.erase(ctx->spare.begin());
  }
}

inline kmi_status set_err(kmi_ctx *ctx, kmi_status st, const char *fmt, const char *a = "", const char *b = "") {
  if (ctx) {
    char buf[512];
    snprintf(buf, sizeof(buf), fmt, a, b);
    ctx->err = buf;
  }
  return st;
}

#define KMI_HIP(ctx, call)                                                              \
  do {                                                                                  \
    hipError_t e__ = (call);                                                            \
    if (e__ != hipSuccess) return kmi::set_err((ctx), KMI_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e__)); \
  } while (0)

#define KMI_TRY(expr)                       \
  do {                                      \
    kmi_status s__ = (expr);                \
    if (s__ != KMI_OK) return s__;          \
  } while (0)

// workspace slot of at least `bytes` (contents are not preserved when it grows)
kmi_status ws_get(kmi_ctx *ctx, WsSlot slot, size_t bytes, void **out);
void ws_release(kmi_ctx *ctx, WsSlot slot);
bool ws_detach(kmi_ctx *ctx, WsSlot slot, const void *p, size_t *bytes);

// profiling hooks around one kernel launch
void prof_begin(kmi_ctx *ctx, const char *name, uint64_t units);
void prof_end(kmi_ctx *ctx, size_t slot);

struct ProfScope {   // scopes may nest: each closes the record it opened
  kmi_ctx *c;
  size_t slot;
  bool on;
  ProfScope(kmi_ctx *ctx, const char *name, uint64_t units) : c(ctx), slot(0), on(ctx->prof) { if (on) { slot = c->prof_pending.size(); prof_begin(c, name, units); } }
  ~ProfScope() { if (on) prof_end(c, slot); }
};

inline bool valid_config(const kmi_config *cfg, KShape *shape) {
  if (!cfg || cfg->k == 0) return false;
  uint32_t bits = (cfg->alphabet == KMI_ALPHA_DNA || cfg->alphabet == KMI_ALPHA_RNA) ? 2 :
                  ((cfg->alphabet == KMI_ALPHA_DNA5 || cfg->alphabet == KMI_ALPHA_RNA5) ? 3 : (cfg->alphabet == KMI_ALPHA_DNA16 ? 4 : 0));
  if (!bits) return false;
  KShape s = make_shape(cfg->k, bits);
  if (s.n_words > (uint32_t)kMaxWords) return false;
  if (cfg->strand > 2 || cfg->dist_hash > 3 || cfg->store_hash > 3 || cfg->seq_format > 1 || cfg->index_kind > 2 || cfg->seq_filter > 2) return false;
  if (cfg->seq_filter && cfg->seq_format == KMI_FMT_FASTA && cfg->k == 1) return false;   // break bits need k >= 2 there
  if (cfg->seq_filter && cfg->index_kind == KMI_INDEX_POSQUAL) return false;
  if (cfg->dist_trans > 2 || (cfg->dist_trans && cfg->strand != KMI_STRAND_SINGLE)) return false;
  if (shape) *shape = s;
  return true;
}

// RNA alphabets: the byte classifiers see T and U swapped (kmi_device.h swap_tu_dword)
inline bool is_rna(const kmi_config *cfg) { return cfg->alphabet == KMI_ALPHA_RNA || cfg->alphabet == KMI_ALPHA_RNA5; }

// dispatch on (n_words, bits)
#define KMI_DISPATCH(shape, FN, ...)                                                   \
  do {                                                                                 \
    if ((shape).bits == 2) {                                                           \
      switch ((shape).n_words) {                                                       \
        case 1: return FN<1, 2>(__VA_ARGS__);                                          \
        case 2: return FN<2, 2>(__VA_ARGS__);                                          \
        case 3: return FN<3, 2>(__VA_ARGS__);                                          \
        case 4: return FN<4, 2>(__VA_ARGS__);                                          \
      }                                                                                \
    } else if ((shape).bits == 3) {                                                    \
      switch ((shape).n_words) {                                                       \
        case 1: return FN<1, 3>(__VA_ARGS__);                                          \
        case 2: return FN<2, 3>(__VA_ARGS__);                                          \
        case 3: return FN<3, 3>(__VA_ARGS__);                                          \
        case 4: return FN<4, 3>(__VA_ARGS__);                                          \
      }                                                                                \
    } else {                                                                           \
      switch ((shape).n_words) {                                                       \
        case 1: return FN<1, 4>(__VA_ARGS__);                                          \
        case 2: return FN<2, 4>(__VA_ARGS__);                                          \
        case 3: return FN<3, 4>(__VA_ARGS__);                                          \
        case 4: return FN<4, 4>(__VA_ARGS__);                                          \
      }                                                                                \
    }                                                                                  \
    return KMI_ERR_INVALID;                                                            \
  } while (0)

// The byte kernels load 16 bytes per lane: an input that does not start on a 16-byte boundary (a record-aligned batch or
// partition inside a larger device buffer) is copied once to an aligned workspace buffer, device to device.
inline kmi_status align_input(kmi_ctx *ctx, const uint8_t **bytes_dev, size_t n_bytes) {
  if (n_bytes == 0 || (reinterpret_cast<uintptr_t>(*bytes_dev) & 15u) == 0) return KMI_OK;
  void *p;
  KMI_TRY(ws_get(ctx, WS_ALIGNED, n_bytes + 64, &p));
  KMI_HIP(ctx, hipMemcpyAsync(p, *bytes_dev, n_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  *bytes_dev = (const uint8_t *)p;
  return KMI_OK;
}

// ---- the RCCL exchange (kmi_comm.hip)
kmi_status comm_all_to_all_counts(kmi_comm *c, const uint64_t *send_counts, uint64_t *recv_counts);
kmi_status comm_all_to_all_v(kmi_comm *c, const void *send_dev, const uint64_t *send_counts, void *recv_dev, const uint64_t *recv_counts,
                             size_t elem_bytes);
// values[0, n) (host) := their sum (op 0) or maximum (op 1) over the ranks: one callback call of a transport, one ncclAllReduce else
// (more than four words are staged in WS_DIST_A: a caller with that many keeps nothing of its own there)
kmi_status comm_allreduce(kmi_comm *c, uint64_t *values, size_t n, int op);
inline kmi_status comm_allreduce_sum(kmi_comm *c, uint64_t *values, size_t n = 1) { return comm_allreduce(c, values, n, 0); }
kmi_status comm_allgather_words(kmi_comm *c, const uint64_t *mine, size_t n, uint64_t *all);
kmi_status comm_all_to_all_counts2(kmi_comm *c, const uint64_t *send_counts, uint64_t my_largest_bytes, uint64_t *recv_counts, uint64_t *largest_bytes);
kmi_status comm_all_to_all_v_async(kmi_comm *c, const void *send_dev, const uint64_t *send_counts, void *recv_dev, const uint64_t *recv_counts,
                                   size_t elem_bytes, uint64_t largest_bytes);
kmi_status comm_exchange_join(kmi_comm *c);
kmi_status comm_exchange_wait(kmi_comm *c);
kmi_ctx *comm_ctx(kmi_comm *c);
int comm_size(kmi_comm *c);
int comm_rank(kmi_comm *c);

// ---- entry points implemented across the .hip files
// de Bruijn tuples from the extract pass (records of n_words + 1 words): EDGES_NODE -- the key is the smaller strand and the value word
// 1 | edge byte << 32 (node form, what the node build inserts); EDGES_PARSED -- the k-mer as parsed and the edge byte (FASTA only:
// de_bruijn_parser's own output)
enum : uint32_t { EDGES_NONE = 0, EDGES_NODE = 1, EDGES_PARSED = 2 };
kmi_status extract_count(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes_dev, size_t n_bytes,
                         uint64_t *n_tuples, uint64_t *n_seqs);
kmi_status extract_run(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes_dev, size_t n_bytes,
                       uint64_t file_offset, uint64_t *out_kmers_dev, uint64_t *out_ids_dev, size_t out_capacity,
                       bool apply_strand, bool scan_done, uint64_t *n_tuples, uint64_t *n_seqs, float *out_quals_dev = nullptr,
                       uint32_t rec_words = 0, uint32_t edges = EDGES_NONE, struct ReadScan *read_scan = nullptr);
kmi_status upload_quality_lut(kmi_ctx *ctx);

// tile scan of a FASTQ partition; the packed arrays and per-tile line bases stay in the workspace
struct ReadDesc { uint64_t seq_pos, out_off; };   // slot = sequence index of the read; out_off = ~0: the read has no k-mer
// what extract_run leaves for a per-read pass over its tuples (FASTQ, records with ids): a descriptor for EVERY record of the buffer
// (seq_pos = ~0: the record has no sequence line; out_off = ~0: no k-mer), the EOL bitmap of the scan and the buffer's line count
struct ReadScan { const ReadDesc *reads; const uint32_t *eolw; uint64_t n_eol_words, n_lines; };
// end of the record-aligned batch that starts at record start `start`: the last record start in (start, start + batch], or the
// first one behind it when one record is larger than the batch; n_bytes when the rest of the buffer fits (bytes on the device / host)
kmi_status fastq_batch_end(kmi_ctx *ctx, const uint8_t *bytes_dev, size_t n_bytes, uint64_t start, uint64_t batch, uint64_t *end);
uint64_t fastq_batch_end_host(const uint8_t *bytes, size_t n_bytes, uint64_t start, uint64_t batch);
struct FastqScan {
  uint64_t n_tiles, n_tuples, n_seqs, n_bytes, n_cover;
  const uint32_t *line_base;
  const uint64_t *hdr_base;   // [n_tiles] 1 + position of the last record start before the tile (0: none)
  const uint64_t *tile_off;   // [n_tiles + 1] k-mer windows before each scan tile
  const uint8_t *pk_eol, *pk_stream;
  const uint8_t *pk_brk;      // window-break bitmap of a sequence filter, or null
};
// check_lengths = false: the caller runs fastq_list_kernel, which carries the seq/qual length rule, and asks for
// fastq_length_verdict afterwards
kmi_status fastq_scan(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes_dev, size_t n_bytes, FastqScan *out, bool check_lengths = true);
kmi_status fastq_length_verdict(kmi_ctx *ctx);
// the quality values of the scanned input's k-mers in file order (out_quals[t] for tuple t), from the read descriptors a pass over
// the windows has filled (slot = sequence index): fastq_quality_kernel. alloc_reads: a cleared descriptor array for sc.n_seqs reads
kmi_status fastq_quality_reads(kmi_ctx *ctx, const FastqScan &sc, ReadDesc **reads);
kmi_status fastq_quality_launch(kmi_ctx *ctx, const uint8_t *bytes_dev, const FastqScan &sc, uint32_t k, const ReadDesc *reads, float *out_quals);

// FASTA: byte-space passes -> compacted character stream (kmi_fasta.hip)
struct FastaScan {
  uint64_t n_chars, n_seqs, n_cover;
  uint64_t n_valid;            // characters whose byte lies in the valid range: k-mer windows start below this rank
  const uint8_t *pk_break;     // bit r: character r is the first of a record
  const uint8_t *pk_stream;    // BITS per character, complement codes
  const uint64_t *ids_by_rank; // or null
};
kmi_status fasta_scan(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes_dev, size_t n_bytes, uint64_t file_offset, bool want_ids,
                      FastaScan *out);
// kmi_fasta_block_summary_dev, and with carry3 the range's left carry per incoming state (a KMI_FA_CARRY_* word)
enum : uint64_t { KMI_FA_CARRY_PASS = 0, KMI_FA_CARRY_CUT = 1, KMI_FA_CARRY_BYTE = 0x100 };
kmi_status fasta_block_summary(kmi_ctx *ctx, const uint8_t *bytes_dev, size_t n_bytes, bool first_ls, uint64_t *out6, uint64_t *carry3);

}  // namespace kmi
