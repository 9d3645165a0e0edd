/*
 * kmerind_hip.h -- C ABI of libkmerind_hip.so, the MI355X (gfx950) k-mer index core.
 *
 * This is the drop-in boundary for ONE path of ParBLiSS/kmerind:
 *   FASTA/FASTQ bytes -> k-mer tuples -> (strand transform) -> hash / rank ->
 *   bucket partition -> per-bucket reduce -> count / find / erase.
 *
 * The reference exposes that path as C++ templates, not as an FFI
 * (bliss::index::kmer::Index<MapType,KmerParser>, src/index/kmer_index.hpp:98-394).
 * Each entry point below names the reference function(s) it replaces; the C++
 * facade in include/kmerind/ re-creates the reference's class / alias names on
 * top of these calls.
 *
 * Conventions
 *   - every function returns kmi_status (0 = OK); kmi_last_error(ctx) gives text.
 *     The facade maps KMI_ERR_INVALID -> std::invalid_argument,
 *     KMI_ERR_PARSE -> std::logic_error (the exceptions the reference throws,
 *     kmer_index.hpp:245-254, fastq_loader.hpp:350-363).
 *   - plain pointers and sizes only; no C++ or torch types cross the ABI.
 *   - "_host" entry points take/return host memory exactly like the reference's
 *     std::vector based API; "_dev" entry points take device pointers that are
 *     already resident in HBM (what bench.py times).
 *   - k-mers are the reference's Kmer<K,Alphabet,uint64_t> object bytes:
 *     n_words little-endian 64-bit words, data[0] least significant, newest base
 *     in the low bits, pad bits zero (src/common/kmer.hpp:116-177).
 *   - one context = one GPU = one "rank" (replaces mxx::comm); all calls on a
 *     context are issued from one host thread, like one MPI rank.
 *   - there is no CPU fallback: without a usable HIP device every entry point
 *     fails with KMI_ERR_DEVICE.
 */
#ifndef KMERIND_HIP_H
#define KMERIND_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  KMI_OK = 0,
  KMI_ERR_INVALID = 1, /* bad argument / unsupported configuration */
  KMI_ERR_DEVICE = 2,  /* HIP runtime failure, no device */
  KMI_ERR_PARSE = 3,   /* malformed FASTQ/FASTA (reference throws std::logic_error) */
  KMI_ERR_NOMEM = 4,
  KMI_ERR_OVERFLOW = 5, /* id overflow (sequence.hpp:177-183) or capacity exceeded */
  KMI_ERR_PEER = 6      /* a collective ended because ANOTHER rank reported an error (this rank's own state is unchanged or as documented) */
} kmi_status;

enum { KMI_ALPHA_DNA = 0, KMI_ALPHA_DNA5 = 1,                   /* alphabets.hpp:127-185, 212-285 (DNA5 == DNA6) */
       KMI_ALPHA_RNA = 2, KMI_ALPHA_RNA5 = 3,                   /* alphabets.hpp:365-445, 448-530 (RNA5 == RNA6): U for T */
       KMI_ALPHA_DNA16 = 4 };                                   /* alphabets.hpp:648-733: IUPAC, 4 bits, complement = bit reversal */
enum { KMI_STRAND_SINGLE = 0, KMI_STRAND_CANONICAL = 1, KMI_STRAND_BIMOLECULE = 2 }; /* kmer_index.hpp:436-481 */
enum { KMI_HASH_MURMUR = 0, KMI_HASH_FARM = 1,                  /* kmer_hash.hpp:242-311 */
       KMI_HASH_IDENTITY = 2, KMI_HASH_STD = 3 };               /* kmer_hash.hpp:205-230, 154-198 (cpp_std, libstdc++) */
enum { KMI_FMT_FASTQ = 0, KMI_FMT_FASTA = 1 };
enum { KMI_INDEX_COUNT = 0, KMI_INDEX_POSITION = 1, KMI_INDEX_POSQUAL = 2 }; /* kmer_index.hpp:399-411 */
/* the SeqIterType argument of read_file_* / build_* (kmer_index.hpp:239-372): SequencesIterator (every record),
 * NFilterSequencesIterator (records whose sequence holds an 'N' are skipped, filtered_sequence_iterator.hpp:154-165)
 * or NSplitSequencesIterator (sequences are cut at every 'N' / 'n', so no k-mer spans one, :429-440) */
enum { KMI_SEQ_ALL = 0, KMI_SEQ_N_FILTER = 1, KMI_SEQ_N_SPLIT = 2 };
/* DistTrans of SingleStrandHashMapParams ("could be iden, xor, lex_less", kmer_index.hpp:436-450; the benchmark's
 * pDistTrans, BenchmarkKmerIndex.cpp:150-161): what KeyToRank hashes. MODEL = the strand model's own choice (identity for
 * single strand and canonical, lex_less for bimolecule); LEX / XOR (kmer_transform.hpp:90-116,60-88) need
 * KMI_STRAND_SINGLE and make both strands of a k-mer land on one rank while they stay separate keys. */
enum { KMI_DIST_MODEL = 0, KMI_DIST_LEX = 1, KMI_DIST_XOR = 2 };

/* The compile-time parameters of the reference's Index<Map,Parser> as a runtime struct. */
typedef struct {
  uint32_t k;          /* Kmer<K,...>::size */
  uint32_t alphabet;   /* KMI_ALPHA_* */
  uint32_t strand;     /* KMI_STRAND_*: Single / Canonical / Bimolecule HashMapParams */
  uint32_t dist_hash;  /* KMI_HASH_*: DistHash (rank assignment), Prefix=true variant */
  uint32_t store_hash; /* KMI_HASH_*: StoreHash; accepted for API parity, placement on the
                          GPU is internal and does not change results */
  uint32_t index_kind; /* KMI_INDEX_* */
  uint32_t seq_format; /* KMI_FMT_* */
  uint32_t farm_ndebug;/* 0: farmhash as the reference's default RelWithDebInfo build computes it
                          (DebugTweak active, CMakeLists.txt:26,200-204); 1: -DNDEBUG behaviour */
  uint32_t seq_filter; /* KMI_SEQ_*. With a filter, n_seqs counts what the reference's read_block counts: records
                          that pass (N_FILTER) or non-empty pieces (N_SPLIT; FASTA: records). FASTA with a filter
                          needs k >= 2. Quality values (KMI_INDEX_POSQUAL) need KMI_SEQ_ALL. */
  uint32_t dist_trans; /* KMI_DIST_* */
} kmi_config;

typedef struct kmi_ctx kmi_ctx;     /* replaces mxx::comm + per-rank state */
typedef struct kmi_index kmi_index; /* replaces MapType (dsc::counting_*_map etc.) */

/* ---- context ------------------------------------------------------------ */
/* Index(const mxx::comm&) (kmer_index.hpp:115): device = HIP ordinal, rank/nranks =
 * comm.rank()/comm.size(). stream = hipStream_t (NULL = default stream). */
kmi_status kmi_ctx_create(int device, int rank, int nranks, void *stream, kmi_ctx **out);
kmi_status kmi_ctx_destroy(kmi_ctx *ctx);
/* forget what the context learned from its builds so far (the pass structure and the duplication the per-bucket reduce starts
 * from): the next build runs as the first one of a context would, with the workspace blocks still in place */
kmi_status kmi_ctx_reset_hints(kmi_ctx *ctx);
/* counters the library keeps for its tests and for diagnosis (no reference counterpart). which = 0: times a build over ranks had to
 * enlarge its receive pool (kmi_index_build_dist_dev); 1: microseconds this context has spent inside hipMalloc / hipFree; 2: bytes
 * and 3: calls that reached hipMalloc; 4: blocks taken from the process-wide cache instead; 5: pointer-jumping rounds, 6: exchanges
 * and 7: bytes this rank sent in the context's last kmi_dbg_compact_dist_host; 8: the largest number of passes a bucket needed in
 * the context's last kmi_index_lookup_* / kmi_index_profile_reads_* / kmi_index_locate_* / kmi_index_seed_reads_* (1 when every
 * bucket's entries fit one table; 0: no bucket was looked at); 9: the entry count of the fullest bucket the context's last kmi_index_retain_counts / kmi_dbg_retain_counts met (0: the index was empty);
 * 10: the largest number of passes a bucket needed in the context's last kmi_index_compare* / kmi_index_combine (0: no bucket
 * was looked at); 13: bytes this rank sent in the context's last kmi_dbg_prune_edges_dist_host; 14: exchanges and 15: bytes this rank
 * sent in the context's last kmi_dbg_clip_tips_dist_host, those of its unitig stages included; 16 and 17: the same for the context's
 * last kmi_dbg_pop_bubbles_dist_host, and 18 and 19: the share of its unitig stages in them */
kmi_status kmi_ctx_debug_counter(const kmi_ctx *ctx, uint32_t which, uint64_t *value);
/* A destroyed context leaves its large device blocks (workspace, spare index arrays: >= 1 MB each, 96 GB / 64 blocks at most) in a
 * process-wide cache per device, where the next context of that device finds them: its first build then does not wait for
 * hipMalloc ("first build"). This frees them (device < 0: of every device). */
kmi_status kmi_release_cached_memory(int device, uint64_t *bytes_released /* may be NULL */);
const char *kmi_last_error(const kmi_ctx *ctx);
/* derived Kmer shape (padding.hpp:67-90): words per k-mer, hashed byte length */
kmi_status kmi_kmer_shape(const kmi_config *cfg, uint32_t *n_words, uint32_t *n_bits, uint32_t *n_bytes);
void kmi_free_host(void *p);
kmi_status kmi_device_alloc(kmi_ctx *ctx, size_t bytes, void **dptr);
kmi_status kmi_device_free(kmi_ctx *ctx, void *dptr);
kmi_status kmi_copy_to_device(kmi_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
kmi_status kmi_copy_on_device(kmi_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes); /* on the context's stream, completed on return */
kmi_status kmi_copy_to_host(kmi_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
kmi_status kmi_synchronize(kmi_ctx *ctx);

/* ---- FASTA input split over ranks ------------------------------------------------------------------
 * What FASTAParser::init_parser learns about its block from the neighbouring ranks (fasta_loader.hpp:232-456,
 * 485-604) and the valid range / overlap rule of the k-mer parsers (kmer_parser.hpp:112-157, overlap = k - 1,
 * kmer_file_helper.hpp:563), as plain numbers the caller supplies for the NEXT FASTA extract / build calls on this
 * context: the buffer is bytes [file_offset, file_offset + n_bytes) of the file, only k-mers whose first base lies
 * in its first `valid_bytes` bytes are produced (the rest of the buffer is the overlap the last windows read), and
 * the line-kind machine starts in `start_state` instead of "file start". NULL restores whole-file behaviour. */
enum { KMI_FA_OUTSIDE = 0, KMI_FA_HEADER = 1, KMI_FA_SEQUENCE = 2 };
typedef struct {
  uint64_t valid_bytes;     /* k-mers start in [0, valid_bytes) of the buffer */
  uint32_t start_state;     /* KMI_FA_*: kind of the line that byte 0 of the buffer sits on (OUTSIDE = before any header) */
  uint32_t at_line_start;   /* 1: byte 0 is the first byte of a line (file start or the byte before it is '\n') */
  uint64_t records_before;  /* records (header group -> sequence group transitions) that start before the buffer */
  uint32_t index_shift;     /* 1 when the FILE begins with non-header lines (init_parser's k/2 rule), else 0 */
  uint32_t reserved;
} kmi_fasta_partition;
kmi_status kmi_ctx_set_fasta_partition(kmi_ctx *ctx, const kmi_fasta_partition *part);
/* the same bookkeeping computed ON THE DEVICE for every block of an n_parts-way split of a FASTA buffer that sits in HBM (the
 * partition negotiation of file.hpp:1436-1610 + fasta_loader.hpp:202-470): block r = bytes [begin_end_host[2 r], begin_end_host
 * [2 r + 1]) of the buffer -- its nominal range [floor(n r / p), floor(n (r + 1) / p)) plus the overlap that holds k - 1 further
 * sequence characters -- and parts_host[r] what kmi_ctx_set_fasta_partition wants for it. Machine state and record count at a byte
 * come from prefix sums over the scan's tile summaries. */
kmi_status kmi_fasta_partition_dev(kmi_ctx *ctx, const uint8_t *bytes_dev, size_t n_bytes, uint32_t n_parts, uint32_t k,
                                   uint64_t *begin_end_host /* 2 * n_parts */, kmi_fasta_partition *parts_host /* n_parts */);

/* ---- L2: k-mer value ops on arrays (parity surface for kmer.hpp / kmer_transform.hpp) */
/* Kmer::reverse_complement (kmer.hpp:1118-1127) on n k-mers */
kmi_status kmi_revcomp_host(kmi_ctx *ctx, const kmi_config *cfg, const uint64_t *in, size_t n, uint64_t *out);
/* transform::lex_less (kmer_transform.hpp:108-116) */
kmi_status kmi_canonical_host(kmi_ctx *ctx, const kmi_config *cfg, const uint64_t *in, size_t n, uint64_t *out);
/* hash::murmur / farm / identity / cpp_std <Kmer,Prefix> (kmer_hash.hpp:154-311); identity and cpp_std with
 * their default-constructed prefix width (24 / 32 bits); inside KeyToRank they get ceilLog2(nranks) like the reference */
kmi_status kmi_hash_host(kmi_ctx *ctx, const kmi_config *cfg, uint32_t which, int prefix,
                         const uint64_t *in, size_t n, uint64_t *out);
/* KeyToRank (distributed_unordered_map.hpp:148-170): DistHash(DistTrans(k)) % nranks */
kmi_status kmi_key_to_rank_host(kmi_ctx *ctx, const kmi_config *cfg, const uint64_t *in, size_t n,
                                uint32_t nranks, uint32_t *ranks);

/* ---- L3: file bytes -> tuples.  KmerFileHelper::read_file_* / parse_file_data_old /
 * read_block_old (kmer_file_helper.hpp:110-186,441-482,588-633) + the tuple parsers
 * (kmer_parser.hpp:85-294,303-569,577-900,909-1083).
 * `bytes` is a record-aligned partition whose first byte sits at `file_offset`;
 * tuples come back in file order, as parsed (no strand transform), like the reference. */
typedef struct {
  uint64_t n_tuples;
  uint64_t n_seqs;
  uint64_t *kmers;  /* n_tuples * n_words */
  uint64_t *ids;    /* Short/LongSequenceKmerId (sequence.hpp:127-296) or NULL */
  float *quals;     /* k-mer quality (quality_score_iterator.hpp:166-173) or NULL */
} kmi_tuples;

kmi_status kmi_extract_host(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes, size_t n_bytes,
                            uint64_t file_offset, kmi_tuples *out /* buffers malloc'd; kmi_tuples_free */);
void kmi_tuples_free(kmi_tuples *t);
/* read_file_* of one rank of several (kmer_file_helper.hpp:550-579 over partitioned_file, file.hpp:1216-1430), FASTQ: the rank read
 * file bytes [buffer_offset, buffer_offset + n_bytes) -- its nominal byte range (nominal_bytes) plus look-ahead -- and parses the
 * records from the first record start at or after its first byte to the first one at or after the nominal end. *need_more = 1
 * (nothing parsed): the partition's end is not decidable inside the buffer and the buffer does not reach the file's end. */
kmi_status kmi_extract_range_host(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes, size_t n_bytes, uint64_t buffer_offset,
                                  uint64_t nominal_bytes, int reaches_eof, int *need_more, kmi_tuples *out);

/* the same for FASTA (fasta_loader.hpp:202-470 over file.hpp:1436-1610): every rank holds the WHOLE file; the tuples of block
 * `rank` of an equal nranks-way split come back, the block bookkeeping (valid range, machine state, records before) being computed
 * on the device from the whole buffer (kmi_fasta_partition_dev). The union over the ranks is the file's tuples, each once. */
kmi_status kmi_extract_fasta_block_host(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes, size_t n_bytes, uint32_t rank,
                                        uint32_t nranks, kmi_tuples *out);

/* device form: out_kmers_dev capacity in tuples (use kmi_extract_count_dev first, or pass an upper bound n_bytes). bytes_dev
 * may point anywhere (a record-aligned batch inside a larger buffer): an input that is not 16-byte aligned is copied once,
 * device to device, to an aligned workspace buffer. */
kmi_status kmi_extract_count_dev(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes_dev, size_t n_bytes,
                                 uint64_t *n_tuples, uint64_t *n_seqs);
kmi_status kmi_extract_dev(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes_dev, size_t n_bytes,
                           uint64_t file_offset, uint64_t *out_kmers_dev, uint64_t *out_ids_dev,
                           size_t out_capacity, uint64_t *n_tuples, uint64_t *n_seqs);

/* the tuples of the position parsers as records, device to device: n_words key words followed by the value words (id, or
 * id and the quality's float bits in the low half of a second word) -- the object bytes of std::pair<Kmer, ShortSequenceKmerId>
 * / std::pair<Kmer, std::pair<ShortSequenceKmerId, float>> (kmer_parser.hpp:303-569, 577-900): what kmi_route_tuples_dev
 * and kmi_index_insert_tuples_dev take. out_capacity in records (kmi_extract_count_dev gives the number). */
kmi_status kmi_extract_records_dev(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes_dev, size_t n_bytes, uint64_t file_offset,
                                   uint64_t *out_records_dev, size_t out_capacity, uint64_t *n_tuples, uint64_t *n_seqs);

/* record-aligned partition of a FASTQ buffer that already sits in HBM: cuts[r] = first record start at or after byte
 * floor(n_bytes * r / n_parts) by the four-line rule of FASTQParser::find_first_record (fastq_loader.hpp:269-364, as
 * partitioned_file applies it, file.hpp:1216-1430); cuts[n_parts] = n_bytes; the ranges [cuts[r], cuts[r + 1]) tile the
 * buffer. What every rank hands to kmi_index_build_* / kmi_extract_* when one buffer is split between ranks or batches. */
kmi_status kmi_fastq_partition_dev(kmi_ctx *ctx, const uint8_t *bytes_dev, size_t n_bytes, uint32_t n_parts, uint64_t *cuts_host /* n_parts + 1 */);
/* the same rule for explicit positions: starts_host[i] = first record start at or after positions_host[i] in the buffer (n_bytes
 * when the buffer holds none behind it). What a rank that read only ITS byte range of a file (plus some look-ahead) uses to find
 * where its partition begins and ends (file.hpp:1342-1422): both neighbours apply the rule at the same file position. */
kmi_status kmi_fastq_find_records_dev(kmi_ctx *ctx, const uint8_t *bytes_dev, size_t n_bytes, int buffer_starts_file /* byte 0 = the file's first byte */,
                                      const uint64_t *positions_host, uint32_t n_pos, uint64_t *starts_host);

/* ---- L4: the exchange step of imxx::distribute (incremental_mxx.hpp:1039-1109):
 * assign_to_buckets + bucket_to_permutation + permute on the device. Output is the
 * send buffer grouped by destination rank, counts[nranks] on the host. The order INSIDE a rank's message is unspecified (the
 * reference's permutation is stable, incremental_mxx.hpp:324-364, but nothing it feeds -- hash map inserts, query dedup --
 * observes that order). The all-to-all itself is done by the caller (RCCL through
 * torch.distributed in kmerind_amd.dist, or ncclSend/ncclRecv from C++). */
kmi_status kmi_route_dev(kmi_ctx *ctx, const kmi_config *cfg, const uint64_t *keys_dev, size_t n,
                         uint32_t nranks, uint64_t *out_keys_dev, uint64_t *send_counts_host);

/* same for (k-mer, value) records of the position indexes: value_words 64-bit words follow each key */
kmi_status kmi_route_tuples_dev(kmi_ctx *ctx, const kmi_config *cfg, const uint64_t *records_dev, size_t n,
                                uint32_t nranks, uint32_t value_words, uint64_t *out_records_dev, uint64_t *send_counts_host);

/* read_file_* followed by the bucketing half of imxx::distribute, fused (FASTQ): the k-mers of this rank's reads,
 * transformed (InputTrans) and grouped by destination rank = DistHash(DistTrans(k)) % nranks, written straight from
 * the packed input; the tuple array in file order never exists in HBM. Replaces kmi_extract_dev + kmi_route_dev on
 * the multi-GPU build path (kmer_file_helper.hpp:588-633 + incremental_mxx.hpp:1039-1086). */
kmi_status kmi_extract_route_dev(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes_dev, size_t n_bytes, uint32_t nranks,
                                 uint64_t *out_keys_dev, size_t out_capacity, uint64_t *n_tuples, uint64_t *n_seqs,
                                 uint64_t *send_counts_host);

/* the same for the (k-mer, value) tuples of the position indexes (index_kind POSITION / POSQUAL): kmi_extract_records_dev +
 * kmi_route_tuples_dev in one call, records of n_words + value_words words grouped by destination rank in out_records_dev;
 * the tuples in file order never leave the workspace (read_file_* + imxx::distribute of Index::build_* with a multimap,
 * kmer_index.hpp:148-225, distributed_unordered_map.hpp:1466-1515) */
kmi_status kmi_extract_route_records_dev(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes_dev, size_t n_bytes, uint64_t file_offset,
                                         uint32_t nranks, uint64_t *out_records_dev, size_t out_capacity, uint64_t *n_tuples,
                                         uint64_t *n_seqs, uint64_t *send_counts_host);

/* ---- L4/L5: the map behind Index<MapType,Parser> ---------------------------- */
kmi_status kmi_index_create(kmi_ctx *ctx, const kmi_config *cfg, kmi_index **out);
kmi_status kmi_index_destroy(kmi_index *idx);
/* Index::insert(std::vector<Kmer>&) for counting maps on ONE rank: InputTransform +
 * local reduce (distributed_unordered_map.hpp:1697-1745,1826-1884). Keys must already
 * belong to this rank when nranks > 1 (i.e. after the exchange). */
kmi_status kmi_index_insert_host(kmi_index *idx, const uint64_t *kmers, size_t n);
kmi_status kmi_index_insert_dev(kmi_index *idx, const uint64_t *kmers_dev, size_t n);
/* the local_insert half alone (distributed_unordered_map.hpp:1734-1741): keys that already went through the
 * InputTransform -- what kmi_route_dev / kmi_extract_route_dev produce and the exchange delivers -- are reduced as they are */
kmi_status kmi_index_insert_transformed_dev(kmi_index *idx, const uint64_t *kmers_dev, size_t n);
/* Index::insert(std::vector<std::pair<Kmer, T>>&) of the counting / reduction maps (kmer_index.hpp:200-225 ->
 * reduction_unordered_map::local_insert, distributed_unordered_map.hpp:1603-1618: `at() = r(at(), v)` with r = std::plus):
 * every pair's value is ADDED to the key's count. records = n objects of (n_words key words, one value word whose low
 * 32 bits are the count) -- the object bytes of std::pair<Kmer, uint32_t>; the keys go through the InputTransform. */
kmi_status kmi_index_insert_pairs_host(kmi_index *idx, const uint64_t *records, size_t n);
kmi_status kmi_index_insert_pairs_dev(kmi_index *idx, const uint64_t *records_dev, size_t n);
/* Index::build_mmap/build_posix for nranks == 1: read_file + insert fused on the
 * device (kmer_index.hpp:239-372). */
kmi_status kmi_index_build_host(kmi_index *idx, const uint8_t *bytes, size_t n_bytes, uint64_t file_offset);
kmi_status kmi_index_build_dev(kmi_index *idx, const uint8_t *bytes_dev, size_t n_bytes, uint64_t file_offset);
/* MapType::clear() (distributed_map_base.hpp:267-272) */
kmi_status kmi_index_clear(kmi_index *idx);
/* The SeqParser template argument of Index::build_posix / build_mmap / build_mpiio<SeqParser, SeqIterType>
 * (kmer_index.hpp:239-372): which record grammar the next kmi_index_build_* call parses (KMI_FMT_*). A position + quality index
 * reads FASTQ only: KMI_FMT_FASTA gives KMI_ERR_INVALID there and leaves the format as it was (so does kmi_index_create with such
 * a configuration). */
kmi_status kmi_index_set_seq_format(kmi_index *idx, uint32_t seq_format);
/* the SeqIterType template argument of Index::build_* (kmer_index.hpp:239-372): KMI_SEQ_* for the following builds */
kmi_status kmi_index_set_seq_filter(kmi_index *idx, uint32_t seq_filter);
/* MapType::local_size() / size() on one rank (distributed_map_base.hpp:227-245) */
kmi_status kmi_index_local_size(kmi_index *idx, uint64_t *n);
/* MapType::to_vector() (distributed_map_base.hpp:202-217): keys n*n_words, counts n; order unspecified */
kmi_status kmi_index_export_host(kmi_index *idx, uint64_t *keys, uint32_t *counts, size_t capacity, uint64_t *n);

typedef struct {
  uint64_t n;
  uint64_t *keys;   /* n * n_words: the transformed (e.g. canonical) query keys */
  uint64_t *values; /* count(): 0/1 presence (db.count(k)); find(): stored count */
} kmi_results;
void kmi_results_free(kmi_results *r);
/* Index::count (kmer_index.hpp:142-145 -> distributed_unordered_map.hpp:880-983):
 * one entry per DISTINCT transformed query key, value = number of map entries with
 * that key (0 or 1 for a counting map). */
kmi_status kmi_index_count_host(kmi_index *idx, const uint64_t *queries, size_t nq, kmi_results *out);
/* Index::find (kmer_index.hpp:132-135 -> :564-687): (key, stored value) of the
 * distinct transformed query keys that are present. */
kmi_status kmi_index_find_host(kmi_index *idx, const uint64_t *queries, size_t nq, kmi_results *out);
/* Index::erase (kmer_index.hpp:147-149 -> :719-779) */
kmi_status kmi_index_erase_host(kmi_index *idx, const uint64_t *queries, size_t nq, uint64_t *n_erased);
/* device-resident query forms used by bench.py (results stay on the device):
 * out_keys_dev/out_values_dev capacity nq; *n_out distinct results */
kmi_status kmi_index_count_dev(kmi_index *idx, const uint64_t *queries_dev, size_t nq,
                               uint64_t *out_keys_dev, uint64_t *out_values_dev, uint64_t *n_out);
kmi_status kmi_index_find_dev(kmi_index *idx, const uint64_t *queries_dev, size_t nq,
                              uint64_t *out_keys_dev, uint64_t *out_values_dev, uint64_t *n_out);
/* the number of entries kmi_index_find_dev would return for these queries (a multimap returns every entry of a queried key:
 * size the result buffers with this instead of the index's entry count) */
kmi_status kmi_index_find_hits_dev(kmi_index *idx, const uint64_t *queries_dev, size_t nq, uint64_t *n_hits);

/* ---- multimap maps: PositionIndex / PositionQualityIndex (kmer_index.hpp:402-406) over
 * ::dsc::unordered_multimap (distributed_unordered_map.hpp:1466-1515). An index created with
 * index_kind POSITION stores every (k-mer, value) tuple; value = 1 u64 (Short/LongSequenceKmerId),
 * POSQUAL = 2 u64 (id, quality float in the low 32 bits of the second word).
 * kmi_index_build_* on such an index parses with KmerPositionTupleParser semantics.
 * count() returns the multiplicity, find() every (key, value) whose key is queried, erase() removes
 * all of them; kmi_results.values then holds n * value_words words. */
kmi_status kmi_index_insert_tuples_host(kmi_index *idx, const uint64_t *kmers, const uint64_t *values, size_t n);
/* records_dev: n records of (n_words key words, value words), i.e. std::pair<Kmer, value> objects */
kmi_status kmi_index_insert_tuples_dev(kmi_index *idx, const uint64_t *records_dev, size_t n);
kmi_status kmi_index_export_tuples_host(kmi_index *idx, uint64_t *keys, uint64_t *values, size_t capacity, uint64_t *n);

/* ---- combine-first distributed insert of the count index (N > 1 ranks) ------------------------------------
 * The reference's counting maps send every k-mer occurrence through imxx::distribute and reduce at the receiver
 * (distributed_unordered_map.hpp:1715-1745 / distributed_densehash_map.hpp:2584-2610; the local_reduction before
 * the exchange is there but commented out). Integer counts add up associatively, so a rank may reduce its own
 * reads first: it builds a local count index of its partition (kmi_index_build_*), splits the entries by
 * KeyToRank, exchanges (k-mer, count) pairs, and every rank merges what it receives. The resulting distributed
 * index is the reference's (key on rank DistHash(DistTrans(key)) % p, value = occurrences over all ranks); the
 * exchanged volume shrinks by the local coverage.
 *
 * kmi_index_num_buckets(): the fixed number B of placement buckets every index uses (entries of a bucket are
 * contiguous; the placement hash is the same on all ranks).
 * kmi_index_split_by_rank_dev: the entries of `idx` grouped by destination rank (message r starts at the sum of
 * send_counts_host[0..r)), and inside a message ordered by placement bucket; bucket_counts_dev[r * B + b] = entries
 * of message r in bucket b. out buffers hold `capacity` >= kmi_index_local_size entries. `idx` is not changed.
 * kmi_index_merge_parts_dev: kmers_dev / counts_dev = nparts such messages back to back (part s holds
 * sum_b bucket_counts_dev[s * B + b] pairs); their counts are added into `idx`. */
uint32_t kmi_index_num_buckets(void);
kmi_status kmi_index_split_by_rank_dev(kmi_index *idx, uint32_t nranks, uint64_t *out_kmers_dev, uint32_t *out_counts_dev,
                                       size_t capacity, uint32_t *bucket_counts_dev, uint64_t *send_counts_host);
kmi_status kmi_index_merge_parts_dev(kmi_index *idx, uint32_t nparts, const uint64_t *kmers_dev, const uint32_t *counts_dev,
                                     const uint32_t *bucket_counts_dev);

/* ---- more than one rank: the exchange over RCCL (xGMI inside one node) -------------------------------------------
 * One process per GPU (kmi_ctx_create(device, rank, nranks)). A communicator replaces the mxx::comm the reference's maps
 * hold: rank 0 makes an id (kmi_comm_unique_id = ncclGetUniqueId, 128 bytes) and the application hands it to the other
 * ranks (MPI_Bcast in the reference's world), every rank calls kmi_comm_create (ncclCommInitRank; collective).
 * kmi_comm_all_to_all_counts / _v are mxx::all2all / mxx::all2allv of imxx::distribute (incremental_mxx.hpp:1087, 1098):
 * counts on the host, payload in device buffers grouped by destination, received as the concatenation by source rank
 * ascending; grouped ncclSend / ncclRecv on the context's stream, 64-bit counts, peer messages in pieces below 1 GiB, the
 * first exchange of a communicator verified by per-message checksums. nranks == 1 works (self exchange). */
typedef struct kmi_comm kmi_comm;
enum { KMI_COMM_ID_BYTES = 128 };
kmi_status kmi_comm_unique_id(void *id_out /* KMI_COMM_ID_BYTES */);
kmi_status kmi_comm_create(kmi_ctx *ctx, const void *id /* NULL allowed when nranks == 1 */, kmi_comm **out);
/* A communicator over a messenger the APPLICATION brings instead of RCCL: the two collectives imxx::distribute needs
 * (incremental_mxx.hpp:1087 all2all, :1098 all2allv) and the all-reduce behind size() (distributed_map_base.hpp:227-245), as
 * callbacks over HOST buffers -- an MPI communicator (the reference's own mxx::comm: INTEGRATION.md section 4), gloo, sockets.
 * The library stages device buffers through pinned host memory around each call, so everything built on a communicator --
 * kmi_index_*_dist_*, kmi_dbg_*_dist_* -- runs unchanged where RCCL is not an option (ranks sharing one GPU, a cluster without
 * xGMI). Both callbacks are collective and blocking; they return 0 on success. */
typedef struct kmi_transport {
  void *user;
  /* rank r receives send_bytes[r] bytes from this rank (the messages lie back to back in `send`, rank 0's first) and this
   * rank receives recv_bytes[r] bytes from rank r into `recv`, back to back by source rank */
  int (*all_to_all_v)(void *user, const void *send, const uint64_t *send_bytes, void *recv, const uint64_t *recv_bytes);
  /* values[0..n) are replaced by their sum (op 0) or maximum (op 1) over the ranks */
  int (*allreduce_u64)(void *user, uint64_t *values, size_t n, int op);
} kmi_transport;
kmi_status kmi_comm_create_transport(kmi_ctx *ctx, const kmi_transport *transport /* copied */, kmi_comm **out);
kmi_status kmi_comm_destroy(kmi_comm *comm);
kmi_status kmi_comm_all_to_all_counts(kmi_comm *comm, const uint64_t *send_counts_host, uint64_t *recv_counts_host);
kmi_status kmi_comm_all_to_all_v(kmi_comm *comm, const void *send_dev, const uint64_t *send_counts_host, void *recv_dev,
                                 const uint64_t *recv_counts_host, size_t elem_bytes /* multiple of 8 */);
kmi_status kmi_comm_allreduce_sum_u64(kmi_comm *comm, uint64_t *value_host);

/* The collectives of Index<MapType, Parser> with comm.size() > 1, every rank calling with its own (possibly empty) share:
 * insert  (distributed_unordered_map.hpp:1697-1745, :1466-1515): InputTransform, KeyToRank grouping on the device
 *         (kmi_route_dev), all2all(counts) + all2allv(keys), local insert of what arrives;
 * build   (kmer_index.hpp:239-372): this rank's record-aligned partition of the file -> parse -> route -> insert (FASTQ count
 *         index: kmi_extract_route_dev, the tuple array never exists; position indexes: records with their values);
 * count / find / erase (:880-983, :564-687, :719-779): the query keys travel to their owners, every owner answers per source
 *         rank, one return exchange; results are this rank's own queries' answers, as the reference returns them;
 * size    (distributed_map_base.hpp:227-245): allreduce of the local sizes.
 * Device buffers throughout; only the caller's vectors cross PCIe. */
kmi_status kmi_index_insert_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *kmers, size_t n);
kmi_status kmi_index_insert_tuples_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *kmers, const uint64_t *values, size_t n);
kmi_status kmi_index_build_dist_host(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint64_t file_offset);
/* the same with this rank's share already in HBM. The count index of one-word 2-bit k-mers (k >= 17, FASTQ, 2 / 4 / 8 ranks)
 * travels as super-k-mer records in record-aligned chunks (KMI_DIST_CHUNKS, default 4): the records of chunk c are exchanged on
 * the communicator's own stream while the front end of chunk c + 1 runs, the counts of a chunk carry every sender's largest
 * message (so all ranks cut the transfer into the same pieces without another collective) and an exchange whose largest message
 * exceeds every one that carried checksums before is verified on arrival. */
kmi_status kmi_index_build_dist_dev(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes_dev, size_t n_bytes, uint64_t file_offset);
/* Index::build_posix / build_mmap / build_mpiio(filename, comm) with comm.size() > 1 (kmer_index.hpp:239-372 over
 * partitioned_file, file.hpp:1216-1430), FASTQ: `bytes` = what this rank read of the file, file bytes [buffer_offset,
 * buffer_offset + n_bytes) -- its nominal range [buffer_offset, buffer_offset + nominal_bytes) plus look-ahead. The partition
 * begins at the first record start at or after the buffer's first byte (the file's first byte for buffer_offset 0) and ends at the
 * first record start at or after the nominal end (four-line rule, on the device); reaches_eof says that the buffer ends with the
 * file. *need_more = 1 and nothing done when the end cannot be decided inside the buffer: read further and call again (no
 * collective has been entered). Then the collective build of that partition. Works for comm.size() == 1 too. */
kmi_status kmi_index_build_range_dist_host(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint64_t buffer_offset,
                                           uint64_t nominal_bytes, int reaches_eof, int *need_more);
/* the same for a FASTA file: every rank passes the WHOLE file; it keeps block comm.rank() of an equal split (bookkeeping on the
 * device, kmi_fasta_partition_dev) and enters the collective build with it. Works for comm.size() == 1 too. */
kmi_status kmi_index_build_fasta_file_dist_host(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes);
/* ... and with every rank holding only ITS byte range of the file (file.hpp:1436-1610 hands each rank 1/p of the file): bytes =
 * file bytes [buffer_offset, buffer_offset + n_bytes), of which the first nominal_bytes are the rank's block of any tiling of the
 * file in rank order (the blocks' lengths are gathered with their summaries: the equal split, block r = [n r / p, n (r + 1) / p),
 * is one such tiling; blocks may be empty) and the rest look-ahead; prev_byte = the file byte before the buffer, -1 at the file
 * start. What a block cannot know from its own bytes -- the kind of line its first byte sits on, the records that start before it,
 * whether the file opens with a header (fasta_loader.hpp:232-456) -- comes from the ranks' block summaries
 * (kmi_fasta_block_summary_dev), gathered once over the communicator and composed left to right. *need_more = 1 (returned BEFORE
 * anything collective): the k - 1 sequence characters the last windows of the block reach into do not end inside the look-ahead;
 * read further and call again. The union over the ranks is the whole file's tuples, each once, with the ids of a whole-file parse. */
kmi_status kmi_index_build_fasta_range_dist_host(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint64_t buffer_offset,
                                                 uint64_t nominal_bytes, int reaches_eof, int prev_byte, int *need_more);
/* read_file_* of a FASTA file on one rank of several by BYTE RANGE (kmi_extract_fasta_block_host with only the block in memory): the
 * rank brings its block of an equal split of the file plus look-ahead (arguments as kmi_index_build_fasta_range_dist_host); the other
 * blocks' summaries come over comm in one small gather (collective). */
kmi_status kmi_extract_fasta_range_dist_host(kmi_ctx *ctx, const kmi_config *cfg, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes,
                                             uint64_t buffer_offset, uint64_t nominal_bytes, int reaches_eof, int prev_byte, int *need_more,
                                             kmi_tuples *out);
/* the line-kind machine over bytes [0, n_bytes) of a FASTA buffer in HBM as a transfer function: out6 = for the incoming states
 * KMI_FA_OUTSIDE, HEADER, SEQUENCE in turn {state behind the bytes, records that start inside}. first_is_line_start: byte 0 opens a line */
kmi_status kmi_fasta_block_summary_dev(kmi_ctx *ctx, const uint8_t *bytes_dev, size_t n_bytes, int first_is_line_start, uint64_t *out6);
/* weighted insert and update() of the counting maps with comm.size() > 1: the pairs travel to the ranks that own their keys
 * (records: n x (n_words key words, one value word); *n_updated = pairs applied on THIS rank) */
kmi_status kmi_index_insert_pairs_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *records, size_t n);
kmi_status kmi_index_update_pairs_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *records, size_t n, uint32_t op, uint64_t *n_updated);
/* the routing half on its own (imxx::distribute of the pairs, incremental_mxx.hpp:1039-1109): out = the pairs whose keys THIS rank owns,
 * keys as the map stores them, grouped by source rank in rank order; the order inside one source's group is unspecified (out->keys:
 * n_words per pair, out->values: one word; kmi_results_free). update() with a host functor over ranks (distributed_densehash_map.hpp:1975-2030) applies it to these. */
kmi_status kmi_index_route_pairs_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *records, size_t n, kmi_results *out);
kmi_status kmi_index_count_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *queries, size_t nq, kmi_results *out);
kmi_status kmi_index_find_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *queries, size_t nq, kmi_results *out);
kmi_status kmi_index_erase_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *queries, size_t nq, uint64_t *n_erased_local);
kmi_status kmi_index_size_dist(kmi_index *idx, kmi_comm *comm, uint64_t *n);

/* ---- update() of the counting maps with a device-side updater ------------------------
 * distributed_densehash_map.hpp:1975-2003 -> densehash_map.hpp:663-714: for every input pair whose transformed key is
 * stored, op(stored value, pair value); pairs of absent keys are skipped; returns the number of calls. The reference
 * takes any functor (the facade runs those on the host); the arithmetic updaters have a device form: records as for
 * kmi_index_insert_pairs_* (key words + one word whose low 32 bits are the value). Pairs with the same key are applied
 * in input order there: ADD / MAX / MIN do not depend on it, ASSIGN keeps the value of the LAST such pair, as there.
 * One rank's entries only (the caller routes the pairs with kmi_route_tuples_dev first when size() > 1). */
enum { KMI_UPDATE_ADD = 0, KMI_UPDATE_MAX = 1, KMI_UPDATE_MIN = 2, KMI_UPDATE_ASSIGN = 3 };
kmi_status kmi_index_update_pairs_host(kmi_index *idx, const uint64_t *records, size_t n, uint32_t op, uint64_t *n_updated);
kmi_status kmi_index_update_pairs_dev(kmi_index *idx, const uint64_t *records_dev, size_t n, uint32_t op, uint64_t *n_updated);

/* ---- queries in the caller's order (no counterpart in the reference: its count() / find() answer once per distinct transformed
 * key, in no particular order, and it has no per-read query at all)
 * Count indexes only (KMI_INDEX_COUNT); a position index gives KMI_ERR_INVALID. Every k-mer shape a count index takes (one to four
 * words; 2-, 3- and 4-bit alphabets), both layouts (placement hash, and the minimizer layout a super-k-mer build leaves), dense and
 * sparse indexes alike. The index is not changed (a sparse index stays sparse); an empty index answers 0 everywhere. These
 * two answer from this rank's entries; kmi_index_lookup_dist_* / kmi_index_profile_reads_dist_* below answer from all ranks'.
 *
 * lookup: counts[i] = the count stored for InputTransform(queries[i]) (the transform find() applies), 0 when it is not in the
 * index. One answer per query, in query order; a key asked twice is answered twice. nq == 0 is fine.
 * KMI_ERR_OVERFLOW: a bucket of the index could not be looked up within the library's pass limit (as for the other queries). */
kmi_status kmi_index_lookup_dev (kmi_index *idx, const uint64_t *queries_dev, size_t nq, uint32_t *counts_dev);
kmi_status kmi_index_lookup_host(kmi_index *idx, const uint64_t *queries,     size_t nq, uint32_t *counts);

typedef struct {
  uint64_t seq_offset;  /* byte offset, from bytes_dev, of the read's first sequence character (n_bytes when the record has no sequence line) */
  uint64_t sum_counts;  /* sum of the looked-up counts over the read's k-mers */
  uint32_t n_kmers;     /* windows the index's parser yields for this read (KMI_SEQ_ALL) */
  uint32_t n_present;   /* of those, in the index */
  uint32_t n_solid;     /* of those, with count >= solid_threshold */
  uint32_t lowest;      /* min over the read's k-mers, an absent k-mer counting 0; 0 when n_kmers == 0 */
  uint32_t highest;     /* max, likewise */
  uint32_t reserved;    /* 0 */
} kmi_read_profile;     /* 40 bytes */

/* profile_reads: one row per FASTQ record of the record-aligned buffer, in file order (row i = record i, records without a k-mer
 * included).
 *  - Windows. The k-mers of a read are exactly those kmi_extract_dev yields for the same bytes with the index's kmi_config and
 *    KMI_SEQ_ALL (the index's own sequence filter is not consulted); each goes through the index's InputTransform, as for find().
 *  - Format. FASTQ only: an index whose sequence format is FASTA gives KMI_ERR_INVALID. Malformed input gives KMI_ERR_PARSE with the
 *    message the builds give.
 *  - Arguments. solid_threshold == 0 gives KMI_ERR_INVALID. bytes_dev may be unaligned. n_bytes == 0 is fine (*n_reads = 0).
 *  - Capacity. *n_reads is always the number of records; capacity < *n_reads gives KMI_ERR_OVERFLOW, the first `capacity` rows are
 *    written and nothing past them.
 *  - Long reads. A read with a k-mer that starts more than 65535 bytes into its record gives KMI_ERR_OVERFLOW (the extract pass
 *    numbers its tuples with the reference's 16-bit in-record offset and refuses such a record); it never gives wrong rows.
 *  - Batches. The input is worked on in record-aligned batches of at most KMI_PROFILE_BATCH bytes (environment, read when the context
 *    is created; default 256 MiB, at least 4096; a batch grows to hold at least one record), so the workspace is that of one batch
 *    whatever the size of the input. The rows do not depend on the batch size.
 * kmi_ctx_debug_counter 8 tells how many passes the fullest bucket needed; KMI_LOOKUP_CAP (environment, at context creation; 64 ..
 * the table's own size) shrinks the lookup table so that tests reach several passes with a small index. */
kmi_status kmi_index_profile_reads_dev (kmi_index *idx, const uint8_t *bytes_dev, size_t n_bytes, uint32_t solid_threshold,
                                        kmi_read_profile *out_dev, size_t capacity, uint64_t *n_reads);
kmi_status kmi_index_profile_reads_host(kmi_index *idx, const uint8_t *bytes, size_t n_bytes, uint32_t solid_threshold,
                                        kmi_read_profile *out, size_t capacity, uint64_t *n_reads);

/* ---- the position indexes in the caller's order: where does each k-mer occur, and the seeds of reads (no counterpart in the
 * reference: its find() returns the (key, value) pairs of the distinct queried keys in no particular order, and it has no cap on
 * repetitive keys and no per-read query)
 * Position and position + quality indexes only (KMI_INDEX_POSITION, KMI_INDEX_POSQUAL); a count index gives KMI_ERR_INVALID. Every
 * key shape these indexes take (one to four words). This rank's entries, as for lookup (the _dist_ forms below: all ranks'). The index is never changed.
 * Strand. Under the canonical strand model a hit does not tell the orientation of the reference occurrence relative to the query:
 * the index stores the canonical k-mer and the position, not which strand of the reference spelled it.
 *
 * locate:
 *   occ[i]     = number of index entries whose key is InputTransform(queries[i]) (the true multiplicity, never capped)
 *   listed(i)  = occ[i] if occ[i] <= max_occ, else 0 (a key is listed whole or not at all)
 *   offsets[i] = sum of listed(j), j < i; offsets[nq] = *n_hits
 *   values[offsets[i] .. offsets[i+1]) = the value words (1 per hit for POSITION, 2 for POSQUAL) of those entries: one answer per
 *                query in query order, a key asked twice is answered twice. The order of the hits inside one query is unspecified.
 *  - max_occ == 0 gives KMI_ERR_INVALID; KMI_LOCATE_ALL means no cap.
 *  - nq == 0 is fine: offsets[0] = 0, *n_hits = 0, no other buffer is touched. An empty index answers occ = 0 everywhere.
 *  - occ, offsets and *n_hits are always written in full. capacity (in hits) < *n_hits gives KMI_ERR_OVERFLOW and nothing is written
 *    into values. values == NULL with capacity == 0 is the sizing call: KMI_OK, and the fill pass is skipped.
 *  - KMI_ERR_OVERFLOW with the message of the other queries when a bucket cannot be handled within the pass limit.
 * kmi_ctx_debug_counter 8 tells the largest pass count of the call; KMI_LOOKUP_CAP shrinks these tables too. */
enum { KMI_LOCATE_ALL = 0xffffffffu };   /* max_occ: no cap */
kmi_status kmi_index_locate_dev (kmi_index *idx, const uint64_t *queries_dev, size_t nq, uint32_t max_occ,
                                 uint32_t *occ_dev /* nq */, uint64_t *offsets_dev /* nq + 1 */,
                                 uint64_t *values_dev, size_t capacity /* hits */, uint64_t *n_hits);
kmi_status kmi_index_locate_host(kmi_index *idx, const uint64_t *queries, size_t nq, uint32_t max_occ,
                                 uint32_t *occ /* nq */, uint64_t *offsets /* nq + 1 */,
                                 uint64_t *values, size_t capacity /* hits */, uint64_t *n_hits);

typedef struct {
  uint64_t seq_offset;  /* as kmi_read_profile.seq_offset */
  uint64_t first_kmer;  /* index of the read's first window in occ[] / offsets[] (for a read without a window: where it would be) */
  uint32_t n_kmers;     /* windows of the read (KMI_SEQ_ALL) */
  uint32_t n_listed;    /* of those, with at least one listed hit */
  uint64_t n_hits;      /* offsets[first_kmer + n_kmers] - offsets[first_kmer] */
} kmi_read_seeds;       /* 32 bytes */

/* seed_reads: locate for every window of every read of a FASTQ buffer, the seed stage of read mapping.
 *  - Rows. One row per FASTQ record of the record-aligned buffer, in file order, records without a k-mer included.
 *  - Windows. Exactly those of kmi_extract_dev with the index's k, alphabet and strand transform and KMI_SEQ_ALL. Window j of read r
 *    is query rows[r].first_kmer + j of one CSR (occ, offsets, values) over all windows of the buffer, with locate's meaning.
 *  - Format. The reads are always parsed as FASTQ, whatever the index was built from (a FASTA-built index questioned with FASTQ
 *    reads is the expected case). Malformed input gives KMI_ERR_PARSE. The 65535-byte in-record limit applies as for profile_reads.
 *  - Capacities. *n_reads, *n_kmers and *n_hits are always exact. If any capacity is short the call returns KMI_ERR_OVERFLOW;
 *    nothing is written past any capacity and the buffers' contents are otherwise unspecified. offsets takes cap_kmers + 1 words.
 *    All buffers NULL with zero capacities is the sizing call: KMI_OK, only the counting passes run.
 *  - max_occ == 0 gives KMI_ERR_INVALID. n_bytes == 0 is fine (offsets[0] = 0 when offsets is given).
 *  - Batches. Record-aligned batches of at most KMI_PROFILE_BATCH bytes, as for profile_reads; the results do not depend on it. */
kmi_status kmi_index_seed_reads_dev (kmi_index *idx, const uint8_t *bytes_dev, size_t n_bytes, uint32_t max_occ,
                                     kmi_read_seeds *rows_dev, size_t cap_reads,
                                     uint32_t *occ_dev, uint64_t *offsets_dev /* cap_kmers + 1 */, size_t cap_kmers,
                                     uint64_t *values_dev, size_t cap_hits,
                                     uint64_t *n_reads, uint64_t *n_kmers, uint64_t *n_hits);
kmi_status kmi_index_seed_reads_host(kmi_index *idx, const uint8_t *bytes, size_t n_bytes, uint32_t max_occ,
                                     kmi_read_seeds *rows, size_t cap_reads,
                                     uint32_t *occ, uint64_t *offsets /* cap_kmers + 1 */, size_t cap_kmers,
                                     uint64_t *values, size_t cap_hits,
                                     uint64_t *n_reads, uint64_t *n_kmers, uint64_t *n_hits);

/* ---- the queries in the caller's order against an index held over ranks (collective)
 * lookup, profile_reads, locate and seed_reads with the arguments and results of the one-rank calls above, answered from the entries
 * of ALL ranks of `comm`. Every rank of the communicator makes the call, each with its own queries or its own record-aligned FASTQ
 * share; nq == 0 or n_bytes == 0 on some or all ranks is fine. A rank's answers are for its own queries, in its own order. A key
 * lives wholly on the rank that owns it, so occ is the true multiplicity over the whole index and "listed whole or not at all"
 * keeps its meaning; first_kmer, offsets and seq_offset are relative to the rank's own buffer, as on one rank.
 *  - One rank. With a communicator of one rank (and no KMI_FORCE_DIST) the call is the one-rank call.
 *  - Owners. The queries travel to the rank that owns the key under the rule the index was built with: the minimizer-bucket owner
 *    of a build through exchanged super-k-mers (kmi_route_owner_dev), KeyToRank (kmi_route_dev) else. Only the key words travel;
 *    where a query sits in the caller's array stays on its rank. The owner answers everything it received in one pass of the
 *    one-rank code; count / occ come back as 4 bytes per key, the listed values of locate as one message per source.
 *  - Refusals. A wrong index kind, max_occ == 0, solid_threshold == 0, a null buffer, a communicator of another context and an
 *    index whose owner ranks (kmi_index_owner_ranks, when not 1) are not the communicator's size give KMI_ERR_INVALID on that rank
 *    before anything collective.
 *  - Errors. A rank-local verdict is all-reduced before the first exchange of the call -- of every batch round for the reads forms
 *    -- and again behind the owners' pass: a parse error, the 65535-byte record limit and a bucket past the pass limit end the call
 *    on every rank; the failing rank returns its own error, the others KMI_ERR_PEER, and no output is promised.
 *  - Capacities. A short capacity is no such error and changes nothing that is sent or received: that rank takes part in every
 *    round, writes nothing past its capacity and returns KMI_ERR_OVERFLOW with exact totals (for locate: with occ and offsets in
 *    full), its peers return KMI_OK with full answers. The sizing call (all output buffers NULL, zero capacities) is collective too
 *    and runs the same exchanges; the values travel when any rank of the call asked for them.
 *  - Batches. The reads forms work in record-aligned batches of KMI_PROFILE_BATCH bytes, one round per batch; a rank that has run
 *    out of input takes part with zero queries until every rank has. The results do not depend on the batch size.
 * kmi_ctx_debug_counter 8 tells the largest pass count of the buckets this rank answered as an owner; 11 the number of output hits
 * a workgroup of the copy that brings the returned values into query order owns; 12 the keys this rank answered as their owner
 * in the last of these calls. */
kmi_status kmi_index_lookup_dist_dev (kmi_index *idx, kmi_comm *comm, const uint64_t *queries_dev, size_t nq, uint32_t *counts_dev);
kmi_status kmi_index_lookup_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *queries,     size_t nq, uint32_t *counts);
kmi_status kmi_index_profile_reads_dist_dev (kmi_index *idx, kmi_comm *comm, const uint8_t *bytes_dev, size_t n_bytes, uint32_t solid_threshold,
                                             kmi_read_profile *out_dev, size_t capacity, uint64_t *n_reads);
kmi_status kmi_index_profile_reads_dist_host(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint32_t solid_threshold,
                                             kmi_read_profile *out, size_t capacity, uint64_t *n_reads);
kmi_status kmi_index_locate_dist_dev (kmi_index *idx, kmi_comm *comm, const uint64_t *queries_dev, size_t nq, uint32_t max_occ,
                                      uint32_t *occ_dev /* nq */, uint64_t *offsets_dev /* nq + 1 */,
                                      uint64_t *values_dev, size_t capacity /* hits */, uint64_t *n_hits);
kmi_status kmi_index_locate_dist_host(kmi_index *idx, kmi_comm *comm, const uint64_t *queries, size_t nq, uint32_t max_occ,
                                      uint32_t *occ /* nq */, uint64_t *offsets /* nq + 1 */,
                                      uint64_t *values, size_t capacity /* hits */, uint64_t *n_hits);
kmi_status kmi_index_seed_reads_dist_dev (kmi_index *idx, kmi_comm *comm, const uint8_t *bytes_dev, size_t n_bytes, uint32_t max_occ,
                                          kmi_read_seeds *rows_dev, size_t cap_reads,
                                          uint32_t *occ_dev, uint64_t *offsets_dev /* cap_kmers + 1 */, size_t cap_kmers,
                                          uint64_t *values_dev, size_t cap_hits,
                                          uint64_t *n_reads, uint64_t *n_kmers, uint64_t *n_hits);
kmi_status kmi_index_seed_reads_dist_host(kmi_index *idx, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint32_t max_occ,
                                          kmi_read_seeds *rows, size_t cap_reads,
                                          uint32_t *occ, uint64_t *offsets /* cap_kmers + 1 */, size_t cap_kmers,
                                          uint64_t *values, size_t cap_hits,
                                          uint64_t *n_reads, uint64_t *n_kmers, uint64_t *n_hits);

/* ---- the count spectrum, and the filter by count (no counterpart in the reference beyond to_vector() plus a host loop, the way
 * its erase_if(pred) works)
 * Count indexes only (KMI_INDEX_COUNT); a position index gives KMI_ERR_INVALID. Every k-mer shape a count index takes (one to four
 * words; 2-, 3- and 4-bit alphabets), both layouts, dense and sparse indexes alike (the unused slots of a sparse index are never
 * read as entries). One rank's entries unless said otherwise.
 *
 * spectrum: hist[min(count, n_bins - 1)] is incremented once per stored entry: bin c < n_bins - 1 holds the entries whose count is
 * exactly c -- bin 0 included, since update with ASSIGN or MIN can store a 0 -- and the last bin every entry with count >=
 * n_bins - 1. All n_bins words are written (hist_dev is cleared on the context's stream inside the call); the caller need not clear
 * them. n_bins outside 2 .. KMI_SPECTRUM_MAX_BINS gives KMI_ERR_INVALID. The index is not changed (a sparse index stays sparse); an
 * empty index gives all zeros. _dev with totals == NULL only queues its work on the context's stream; with totals it waits.
 *
 * spectrum_dist_host (collective): hist, n_entries and sum_counts summed over the ranks, min_count / max_count reduced over them
 * (ranks without entries abstain). Every key lives on exactly one rank whichever way the index was built (KeyToRank or minimizer-
 * bucket owner), so this is the spectrum of the whole map. A rank whose local pass fails does not leave its peers waiting: they
 * return KMI_ERR_PEER. Works over a one-rank communicator.
 *
 * retain_counts: keeps the entries with lo <= count <= hi and erases the rest; *n_erased = how many left. lo > hi gives
 * KMI_ERR_INVALID and changes nothing. No key travels to the host. The survivors go, in their old order, into fresh arrays of
 * exactly the surviving size (dropping the singletons of a read set gives most of the index's memory back); the result is a dense
 * index in the same layout, with the same owner ranks, saturation setting and configuration, and every later operation works on it
 * as on any index, also when nothing survived. When nothing is erased the index is left exactly as it is (a sparse one sparse).
 * There is no _dist form because there is nothing to exchange: every rank filters its own share, and the union of the shares is
 * the filtered map. kmi_ctx_debug_counter 9 gives the entry count of the fullest bucket the last call met. */
enum { KMI_SPECTRUM_MAX_BINS = 65536 };
typedef struct {
  uint64_t n_entries;   /* entries counted = kmi_index_local_size */
  uint64_t sum_counts;  /* sum of the stored counts, 64-bit, never clamped */
  uint32_t min_count;   /* 0 for an empty index */
  uint32_t max_count;   /* 0 for an empty index */
} kmi_spectrum_totals;  /* 24 bytes */
kmi_status kmi_index_spectrum_dev (kmi_index *idx, uint32_t n_bins, uint64_t *hist_dev, kmi_spectrum_totals *totals /* host; may be NULL */);
kmi_status kmi_index_spectrum_host(kmi_index *idx, uint32_t n_bins, uint64_t *hist,     kmi_spectrum_totals *totals /* may be NULL */);
kmi_status kmi_index_spectrum_dist_host(kmi_index *idx, kmi_comm *comm, uint32_t n_bins, uint64_t *hist, kmi_spectrum_totals *totals /* may be NULL */);
kmi_status kmi_index_retain_counts(kmi_index *idx, uint32_t lo, uint32_t hi, uint64_t *n_erased /* may be NULL */);

/* ---- two count indexes compared and combined (no counterpart in the reference, where this is to_vector() of one map, count() or
 * find() in the other and a host loop; KMC's `simple` operations and Jellyfish `merge` are the precedents)
 * Two indexes of one k-mer shape and one internal layout hold a key in the same bucket, so the join is bucket against bucket on
 * the device: nothing is partitioned and no key travels to the host.
 *
 * Membership is by key. A key whose stored count is 0 is present (update with ASSIGN or MIN can store a 0). "Shared" means the
 * same stored key; both indexes hold keys after the same InputTransform because their configurations must agree (Operands).
 *
 * compare: neither index's entries change. The eight words give
 *   Jaccard = n_shared / (n_a + n_b - n_shared), containment of a in b = n_shared / n_a,
 *   weighted Jaccard = sum_min_shared / (sum_a + sum_b - sum_min_shared);
 * the struct stays integer so that it can be tested exactly. compare(a, a) is allowed and gives n_shared == n_a.
 *
 * combine: a becomes the result, b's entries are unchanged. With ca / cb the stored counts (an absent key counting 0 where the
 * row says so):
 *   KMI_COMBINE_UNION_ADD        keys in a or in b             ca + cb
 *   KMI_COMBINE_UNION_MAX        keys in a or in b             max(ca, cb)
 *   KMI_COMBINE_INTERSECT_MIN    keys in both                  min(ca, cb)
 *   KMI_COMBINE_INTERSECT_ADD    keys in both                  ca + cb
 *   KMI_COMBINE_INTERSECT_LEFT   keys in both                  ca
 *   KMI_COMBINE_SUBTRACT_KEYS    keys in a and not in b        ca
 *   KMI_COMBINE_SUBTRACT_COUNTS  keys in a with ca > cb        ca - cb      (absent from b: cb = 0, so a stored 0 of a leaves)
 * ca + cb follows a's reducer: it wraps by default and stops at 2^32 - 1 after kmi_index_set_saturating(a, 1). The result lies in
 * fresh arrays of exactly its size, in a's layout family; owner ranks, saturation setting and configuration are unchanged, and
 * every later operation works on a as on any index, also when nothing survived. The order of the entries inside the result is
 * not specified. On any error a still holds what it held. An unknown op or a == b gives KMI_ERR_INVALID. *n_entries = the entries
 * of a afterwards. (A call that cannot change a -- a union with an empty b, anything else on an empty a, SUBTRACT_KEYS with an
 * empty b -- leaves a's arrays where they are.)
 *
 * Operands. Anything outside these rules gives KMI_ERR_INVALID with both indexes untouched: both are count indexes (a position
 * index is refused), both belong to the same context, both have the same k, alphabet and strand model, and both have the same
 * kmi_index_owner_ranks.
 *
 * Shapes and forms. Every shape a count index takes (one to four words; 2-, 3- and 4-bit alphabets), dense and sparse indexes
 * alike, either layout held by either operand. The join reads a sparse operand as it is. An operand's INTERNAL FORM may change
 * while its entries do not: when the layouts differ one operand is brought to the other's -- for combine that is a, for compare
 * the smaller one -- and the two unions bring both operands to the dense form first, because the merge reads bucket b as
 * [offset b, offset b + 1).
 *
 * Empty cases. An index that has never been filled counts as empty. Empty against anything is well defined: compare gives zeros
 * but for the other operand's n_ and sum_ words, combine the table's rows.
 *
 * Passes. A bucket of b whose entries do not fit one table is worked on in passes, as in the lookup; KMI_ERR_OVERFLOW when a
 * bucket exceeds the pass limit. KMI_LOOKUP_CAP shrinks this table too. kmi_ctx_debug_counter 10 gives the largest number of
 * passes a bucket needed in the context's last compare or combine, 0 when no bucket was looked at.
 *
 * Ranks. combine needs no _dist form: every key lives on exactly one rank under either ownership rule, so two indexes built over
 * the same communicator with the same owner rule combine share by share, and the union of the shares is the combined map (the
 * equal owner_ranks test guards the rule). compare_dist_host is collective: the eight words summed over the ranks. A rank whose
 * local join fails does not leave its peers waiting: they return KMI_ERR_PEER. Operand errors are every rank's alike and return
 * before anything collective starts. Works over a one-rank communicator.
 *
 * Completion. All three calls are complete on return. */
typedef struct {
  uint64_t n_a, n_b;            /* entries of a and of b (= kmi_index_local_size) */
  uint64_t n_shared;            /* keys stored in both */
  uint64_t sum_a, sum_b;        /* sum of all stored counts, 64-bit, never clamped */
  uint64_t sum_a_shared;        /* sum of a's counts over the shared keys */
  uint64_t sum_b_shared;        /* ... of b's */
  uint64_t sum_min_shared;      /* sum over the shared keys of min(count in a, count in b) */
} kmi_index_overlap;            /* 64 bytes */
enum { KMI_COMBINE_UNION_ADD = 0, KMI_COMBINE_UNION_MAX = 1, KMI_COMBINE_INTERSECT_MIN = 2, KMI_COMBINE_INTERSECT_ADD = 3,
       KMI_COMBINE_INTERSECT_LEFT = 4, KMI_COMBINE_SUBTRACT_KEYS = 5, KMI_COMBINE_SUBTRACT_COUNTS = 6 };
kmi_status kmi_index_compare(kmi_index *a, kmi_index *b, kmi_index_overlap *out);
kmi_status kmi_index_compare_dist_host(kmi_index *a, kmi_index *b, kmi_comm *comm, kmi_index_overlap *out);
kmi_status kmi_index_combine(kmi_index *a, kmi_index *b, uint32_t op, uint64_t *n_entries /* of a afterwards; may be NULL */);

/* ---- a count index over 2, 4 or 8 ranks through exchanged super-k-mers ---------------
 * The reference's distributed insert sends every k-mer to KeyToRank(k-mer) (8 bytes per k-mer over the wire,
 * distributed_unordered_map.hpp:1697-1745). For FASTQ input and one-word DNA k-mers (17 <= k <= 32) the fused build cuts
 * the reads into super-k-mers first (runs of k-mers that share a minimizer: 16 bytes for about nine k-mers), so the
 * exchange can move those instead: the owner of a k-mer is then the rank that owns its MINIMIZER's bucket (the top
 * log2(nranks) bits of the 18 bucket bits), not hash(k-mer) % nranks. Which rank holds a k-mer is not observable through
 * Index (count / find / erase / size are collectives); the union of the ranks' maps is the reference's map, bit for bit.
 *   produce: this rank's FASTQ share -> records grouped by owner rank (2 words per record), send_counts_host[nranks] in
 *            records. They are written to out_records_dev when that buffer (out_capacity records; may be NULL) holds them
 *            all, else to library workspace valid until the next call on the context; *records_dev says where they are.
 *            They are written on the context's stream and the call does not wait for that: read them on that stream, on a
 *            stream ordered behind it (a collective issued from it), or through kmi_copy_on_device. *produced = 0: this
 *            path does not apply (shape, rank count) or an input exceeded a capacity of the fused front end -- EVERY
 *            rank must then take the k-mer route for this input (agree on min(*produced) over ranks first);
 *   (caller: all-to-all of the records, 16-byte elements)
 *   consume: the records that arrived (flat array, any order of sources) -> this rank's part of the index;
 *   kmi_route_owner_dev: query keys (transformed as the index's strand model says) grouped by owner rank, the
 *            counterpart of kmi_route_dev for an index built this way; kmi_index_owner_ranks tells how an index was built
 *            (1 = by kmi_index_build / insert: route with kmi_route_dev); kmi_index_set_owner_ranks declares it for an
 *            index that is filled with k-mers routed by kmi_route_owner_dev only (an input none of whose parts could
 *            be produced as records). */
kmi_status kmi_index_sk_produce_dev(kmi_index *idx, const uint8_t *bytes_dev, size_t n_bytes, uint32_t nranks,
                                    uint64_t *out_records_dev, size_t out_capacity, const uint64_t **records_dev,
                                    uint64_t *n_records, uint64_t *send_counts_host, int *produced);
kmi_status kmi_index_sk_consume_dev(kmi_index *idx, const uint64_t *records_dev, size_t n_records, uint32_t nranks);
kmi_status kmi_route_owner_dev(kmi_ctx *ctx, const kmi_config *cfg, const uint64_t *keys_dev, size_t n, uint32_t nranks,
                               uint64_t *out_keys_dev, uint64_t *send_counts_host);
kmi_status kmi_index_owner_ranks(kmi_index *idx, uint32_t *nranks);
/* *w = the minimizer window W the super-k-mer paths take for this index's FASTQ builds, 0 where they do not apply (multi-word
 * k-mers, 3- / 4-bit alphabets, k < 17, a multimap, a context created with KMI_FUSED_PATH=kmer): callers that choose between
 * the record exchange and another route decide from this, identically on every rank */
kmi_status kmi_index_sk_width(kmi_index *idx, uint32_t *w);
/* the reducer of a counting map: 0 (default) = std::plus<uint32_t>, counts wrap (distributed_unordered_map.hpp:1603-1618);
 * 1 = sat_plus<uint32_t> of saturating_counting_densehash_map (distributed_densehash_map.hpp:2903-2912): a count that would pass
 * 2^32 - 1 stays there. Applies wherever counts are ADDED -- weighted pairs, merging into an index that holds entries, parts
 * received from other ranks. (A single call is assumed to hold fewer than 2^32 occurrences of one key.) */
kmi_status kmi_index_set_saturating(kmi_index *idx, int on);
kmi_status kmi_index_set_owner_ranks(kmi_index *idx, uint32_t nranks);

/* ---- de Bruijn graph nodes ------------------------------------------------------
 * The reference's in-tree consumer of Index: de_bruijn_engine<NodeMap> = Index<NodeMap, de_bruijn_parser>
 * (test/test/debruijn/de_bruijn_construct_engine.hpp:241-245) with NodeMap = de_bruijn_nodes_distributed<Kmer,
 * node::edge_counts<DNA16, int32_t> | node::edge_exists<DNA16>, BimoleculeHashMapParams>
 * (de_bruijn_nodes_distributed.hpp:57-265, de_bruijn_node_trait.hpp:139-336), as
 * test/test/test_de_bruijn_graph_construction.cpp:124-137,195-206 instantiates it.
 * A node = (k-mer, counts[9]): counts[0..3] = out edges A C G T (the base right of the k-mer in a read),
 * counts[4..7] = in edges A C G T (the base left of it), counts[8] = occurrences of the k-mer. Edge bytes are DNA16
 * presence bits (in << 4 | out), so an 'N' neighbour counts for all four. EDGE_EXISTS keeps 0 / 1 per edge and no
 * occurrence count (counts[8] = 0).
 * Orientation: the reference keeps a node under whichever strand reached the map first (an order MPI decides); this
 * library keeps the lexicographically smaller strand and turns the edges with it (reverse_complement_edges,
 * de_bruijn_node_trait.hpp:122-124). The node set is the same, and so is every node up to that flip.
 * Input is FASTQ (what the engine is instantiated with, :96,195) or FASTA (kmi_dbg_set_seq_format; the engine is generic over
 * the sequence type, :108-158), without a sequence filter, on one rank or over ranks; kmi_config.strand, index_kind and dist_trans
 * are not consulted. */
typedef struct kmi_dbg kmi_dbg;
enum { KMI_DBG_EDGE_COUNTS = 0, KMI_DBG_EDGE_EXISTS = 1 };
#define KMI_DBG_VALUE_WORDS 5 /* a node value in kmi_results.values: uint32_t counts[9] + one uint32_t of padding */
kmi_status kmi_dbg_create(kmi_ctx *ctx, const kmi_config *cfg, uint32_t node_kind, kmi_dbg **out);   /* NodeMap(comm) */
/* the SeqParser template argument of the engine's build_* (KMI_FMT_FASTQ / KMI_FMT_FASTA): on FASTA a record's characters are its
 * sequence lines without their EOLs, edges follow the characters across line ends and never across a header */
kmi_status kmi_dbg_set_seq_format(kmi_dbg *g, uint32_t seq_format);
kmi_status kmi_dbg_destroy(kmi_dbg *g);
kmi_status kmi_dbg_clear(kmi_dbg *g);
kmi_status kmi_dbg_local_size(kmi_dbg *g, uint64_t *n);                                               /* local_size() */
/* de_bruijn_parser::operator() over every record of a FASTQ buffer (de_bruijn_construct_engine.hpp:109-157):
 * records of n_words + 1 words, the k-mer as parsed and the edge byte (edge_iterator.hpp:163-177) in the low
 * byte of the last word. out_records_dev == NULL: count only. */
kmi_status kmi_dbg_parse_dev(kmi_ctx *ctx, const kmi_config *cfg, const uint8_t *bytes_dev, size_t n_bytes,
                             uint64_t *out_records_dev, size_t out_capacity, uint64_t *n_tuples);
/* build_posix / build_mmap<FASTQParser> on one rank (kmer_index.hpp:239-372 with the parser above): parse + insert */
kmi_status kmi_dbg_build_dev(kmi_dbg *g, const uint8_t *bytes_dev, size_t n_bytes);
kmi_status kmi_dbg_build_host(kmi_dbg *g, const uint8_t *bytes, size_t n_bytes);
/* insert(std::vector<std::pair<Kmer, uint8_t>>&) (de_bruijn_nodes_distributed.hpp:230-264, local_insert :91-159):
 * records as kmi_dbg_parse_dev emits them, either strand */
kmi_status kmi_dbg_insert_dev(kmi_dbg *g, const uint64_t *records_dev, size_t n);
kmi_status kmi_dbg_insert_host(kmi_dbg *g, const uint64_t *records, size_t n);
/* find(): one (stored k-mer, node) per distinct query key that is a node, KMI_DBG_VALUE_WORDS words per value;
 * a query matches under either strand. count(): 0 / 1 per distinct query key (values: one word each). */
kmi_status kmi_dbg_find_host(kmi_dbg *g, const uint64_t *queries, size_t nq, kmi_results *out);
kmi_status kmi_dbg_find_dev(kmi_dbg *g, const uint64_t *queries_dev, size_t nq, uint64_t *out_keys_dev, uint64_t *out_values_dev,
                            uint64_t *n_out);
kmi_status kmi_dbg_count_host(kmi_dbg *g, const uint64_t *queries, size_t nq, kmi_results *out);
/* the local nodes: keys[n * n_words], counts9[n * 9] (either may be NULL) */
kmi_status kmi_dbg_export_host(kmi_dbg *g, uint64_t *keys, uint32_t *counts9, size_t capacity, uint64_t *n);
/* over the ranks of a communicator: every rank parses its record-aligned share, the tuples travel to the rank
 * KeyToRank gives their canonical k-mer (the distribute step of insert, de_bruijn_nodes_distributed.hpp:243-250) */
kmi_status kmi_dbg_build_dist_host(kmi_dbg *g, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes);
kmi_status kmi_dbg_find_dist_host(kmi_dbg *g, kmi_comm *comm, const uint64_t *queries, size_t nq, kmi_results *out); /* find(): collective */
/* the engine's build_posix / build_mmap(filename) with comm.size() > 1: as kmi_index_build_range_dist_host (FASTQ byte range +
 * look-ahead, cut at record starts on the device, then the collective build) */
kmi_status kmi_dbg_build_range_dist_host(kmi_dbg *g, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint64_t buffer_offset,
                                         uint64_t nominal_bytes, int reaches_eof, int *need_more);
/* ... of a FASTA file (FASTAParser), by BYTE RANGE: arguments as kmi_index_build_fasta_range_dist_host. The block's windows need k
 * sequence characters behind it (the last window's right neighbour), not k - 1; the left neighbour of its first window comes from
 * the blocks before it (their left carries: the last sequence character, or a record start behind it, in the same one gather as the
 * block summaries). *need_more = 1 is returned BEFORE anything collective. Then parse in node form, route, one exchange, insert
 * (collective). Works over a one-rank communicator too. KMI_ERR_INVALID when the graph's sequence format is not FASTA. The union
 * over the ranks is the graph of the whole file. */
kmi_status kmi_dbg_build_fasta_range_dist_host(kmi_dbg *g, kmi_comm *comm, const uint8_t *bytes, size_t n_bytes, uint64_t buffer_offset,
                                               uint64_t nominal_bytes, int reaches_eof, int prev_byte, int *need_more);
/* nodes.erase(keys): the nodes of the query keys (either strand) leave the map with their edge counts (the erase the node map
 * inherits from the distributed map, distributed_unordered_map.hpp:719-779); *n_erased = nodes removed (here / on this rank) */
kmi_status kmi_dbg_erase_host(kmi_dbg *g, const uint64_t *queries, size_t nq, uint64_t *n_erased);
kmi_status kmi_dbg_erase_dist_host(kmi_dbg *g, kmi_comm *comm, const uint64_t *queries, size_t nq, uint64_t *n_erased_local);
kmi_status kmi_dbg_count_dist_host(kmi_dbg *g, kmi_comm *comm, const uint64_t *queries, size_t nq, kmi_results *out); /* count(): collective */
kmi_status kmi_dbg_size_dist(kmi_dbg *g, kmi_comm *comm, uint64_t *n);                                /* size() */

/* ---- unitigs of a node map (no counterpart in the reference: its test/test/debruijn/ ends at the node map)
 * Compaction collapses every non-branching path of the graph below into one unitig. With t = min_edge_count >= 1:
 *  1. Degree of an end. A node v has an out end and an in end, in its stored (lexicographically smaller) orientation. The degree
 *     of an end is the number of bases whose counter at that end is >= t. Only v's own counters count, so an edge to a k-mer that
 *     is not a node (a DNA16 'N' neighbour, a node erased) still counts toward the degree. EDGE_EXISTS counters are 0 / 1.
 *  2. Links. The out end of v, with its single base b, links to the node w = canonical(v[1..k-1] + b) only if w is a node; w != v
 *     (self-loops and hairpins v -> rc(v) never link); the end of w that is entered has degree 1; and its counter for the
 *     reciprocal base is >= t: the in end and base v[0] if w is stored forward, the out end and base comp(v[0]) if w is stored
 *     reverse-complemented. The in end of v works the same way, with w = canonical(c + v[0..k-2]).
 *  3. Palindromes. A node whose k-mer equals its reverse complement (even k only) links to nothing.
 *  4. Components. Links are symmetric and each end has at most one, so the linked components are simple paths and simple cycles.
 *     Each one is a unitig; every node is in exactly one.
 *  5. Spelling. A path of L nodes is its L + k - 1 bases in whichever direction gives the lexicographically smaller string (the
 *     direction whose first oriented k-mer is smaller). A cycle of L nodes is spelled from its node with the smallest canonical
 *     k-mer, in that node's stored orientation, as L + k - 1 bases (the last k - 1 repeat the first), and flagged circular. The
 *     letters are the alphabet's (ACGT; ACGU for RNA).
 *  6. Occurrences. Per unitig, the sum of counts[8] over its nodes (0 for an EDGE_EXISTS map).
 * Unitigs are numbered in the order of the entries of their first nodes. Only 2-bit alphabets (DNA, RNA) are supported, for every
 * k the node map takes; anything else, t = 0, or a map that holds one rank's share of a build over more than one rank
 * (kmi_dbg_build_dist_host / *_range_dist_host with comm size > 1, until kmi_dbg_clear) gives KMI_ERR_INVALID.
 * kmi_dbg_compact runs on the device and keeps the result in the graph; every build, insert, erase or clear drops it. */
kmi_status kmi_dbg_compact(kmi_dbg *g, uint32_t min_edge_count, uint64_t *n_unitigs, uint64_t *n_bases);
/* ... of a map held over the ranks of a communicator (collective). The graph is the union of the ranks' node maps: what a
 * collective build left behind, possibly changed since by kmi_dbg_erase_dist_host / kmi_dbg_insert_*; rules 1-6 above apply to that
 * union unchanged. In addition:
 *  - Ownership. Each unitig is held by exactly one rank: the one whose map holds its first node in spelling order (a path: the node
 *    whose oriented k-mer starts the spelled string; a cycle: its node with the smallest canonical k-mer).
 *  - Order. A rank's unitigs are numbered in the order of the entries of those first nodes in its node map, as above.
 *  - Result. Kept in the graph, read with kmi_dbg_unitigs_export_host (this rank's unitigs), dropped by every build, insert, erase
 *    or clear. *_local: this rank's unitigs and bases; *_total: the sums over the ranks, the same on every rank. Any output may
 *    be NULL.
 *  - One rank. A one-rank communicator gives what kmi_dbg_compact gives (with KMI_FORCE_DIST=1 through the code of several ranks,
 *    the rank being its own peer).
 * KMI_ERR_INVALID: not a 2-bit alphabet, t = 0, a communicator of another context, more than 256 ranks (the limit of the library's
 * routing). KMI_ERR_OVERFLOW: 2^31 - 1 or more nodes on this rank; a global state is rank << 32 | 2 * node + direction, which has
 * room for 2^16 ranks, and distances and occurrence sums are 64-bit, so they do not wrap for any graph that fits. A rank that fails
 * on its own (these, or KMI_ERR_NOMEM for the workspace of its own nodes or for its result) does not leave its peers waiting: the
 * verdict is agreed on by an all-reduce before the first exchange and again before the last, and the peers return KMI_ERR_PEER.
 * (Receive buffers, whose size depends on what the peers send, grow inside an exchange as in the library's other collectives.) The number of pointer-jumping rounds is decided over all ranks (at most
 * ceil(log2(states of all ranks)) + 1); kmi_ctx_debug_counter 5..7 give the rounds, exchanges and bytes sent by this rank for the
 * last call. */
kmi_status kmi_dbg_compact_dist_host(kmi_dbg *g, kmi_comm *comm, uint32_t min_edge_count, uint64_t *n_unitigs_local, uint64_t *n_bases_local,
                                     uint64_t *n_unitigs_total, uint64_t *n_bases_total);
/* the result of the last kmi_dbg_compact / kmi_dbg_compact_dist_host: offsets[n_unitigs + 1] (unitig i is bases[offsets[i], offsets[i + 1])), bases (not
 * NUL-terminated), occurrences[n_unitigs], circular[n_unitigs] (0 / 1). Any output may be NULL. KMI_ERR_INVALID when the map has
 * not been compacted since it last changed; KMI_ERR_OVERFLOW when a capacity is too small. */
kmi_status kmi_dbg_unitigs_export_host(kmi_dbg *g, uint64_t *offsets, char *bases, uint64_t *occurrences, uint8_t *circular,
                                       size_t capacity_unitigs, size_t capacity_bases);

/* ---- cleaning a node map: occurrence spectrum, filter by occurrences, edge pruning (no counterpart in the reference)
 * Sequencing errors show up as nodes seen once or twice. The usual remedy is to drop them and to compact afterwards; rule 1 of the
 * compaction above then still counts every survivor's counter towards a neighbour that has left (or that never was a node: an 'N'
 * neighbour sets all four), and the unitig stops there. kmi_dbg_prune_edges is the explicit step that clears such counters.
 *
 * spectrum: the contract of kmi_index_spectrum_* (hist[min(c, n_bins - 1)], kmi_spectrum_totals, 2 <= n_bins <=
 * KMI_SPECTRUM_MAX_BINS) applied to counts[8] of the nodes this rank holds; _dist_host (collective) sums over the ranks as
 * kmi_index_spectrum_dist_host does. An EDGE_EXISTS map has no occurrence count: KMI_ERR_INVALID.
 *
 * retain_counts: keeps the nodes with lo <= counts[8] <= hi; the rest leave with their edge counters, as in kmi_dbg_erase_host.
 * The survivors keep their eight counters bit for bit and their order, in fresh arrays of exactly the surviving size; the
 * neighbours' counters are not touched (that is prune_edges). *n_erased = nodes that left (may be NULL). lo > hi or an EDGE_EXISTS
 * map: KMI_ERR_INVALID. Local on every rank (a node lives on exactly one rank, so the union over the ranks is filtered when every
 * rank has filtered its share; no _dist form). On any error the map holds what it held, and so does the result of an earlier
 * compaction; a call that succeeds drops it.
 *
 * prune_edges, with t = min_edge_count >= 1. A counter is (v, E, b): v a node in its stored, canonical orientation, E out or in, b
 * a base. Its neighbour k-mer is x = v[1..k-1] + b for E = out and x = b + v[0..k-2] for E = in; w = canonical(x). Its reciprocal
 * counter is at w:
 *      E     w stored as x         w stored as rc(x)
 *      out   (w, in,  v[0])        (w, out, comp(v[0]))
 *      in    (w, out, v[k-1])      (w, in,  comp(v[k-1]))
 * Self-loops and hairpins follow the same formula (a hairpin's counter is its own reciprocal). Counters are read as the compaction
 * reads them: 0 / 1 for an EDGE_EXISTS map. Every counter that is not 0 is judged against the map AS IT WAS WHEN THE CALL BEGAN,
 * by the first rule that applies:
 *  1. Weak. counter < t: cleared.
 *  2. Absent. w is not a node: cleared.
 *  3. Unreciprocated. The reciprocal counter is < t: cleared. Not applied when v or w is its own reverse complement (even k only):
 *     an adjacency of a palindromic node lands in out[b] or in in[comp(b)] depending on the strand it was read from, so no single
 *     counter reciprocates it. Rules 1 and 2 still apply.
 *  4. Kept. Otherwise the counter keeps its value.
 * Consequences: the result is a pure function of the map at the call; a second call with the same t clears nothing (for nodes that
 * are not palindromes the reciprocal of the reciprocal is the counter itself); after prune(t), kmi_dbg_compact gives the same
 * unitigs for every threshold 1..t; nodes are never removed and counts[8] never changes.
 * KMI_ERR_INVALID: t = 0; an alphabet that is not 2-bit (the limit of the compaction); kmi_dbg_prune_edges on a map that holds one
 * rank's share of a build over ranks. An empty map gives zeros. On any error the map holds what it held, and so does the result of
 * an earlier compaction; a call that succeeds drops it. The call is complete on return.
 * _dist_host (collective): the graph is the union of the ranks' maps; a counter whose neighbour lives on another rank is judged by
 * that rank (one request of (n_words + 1) x 8 bytes and one answer of 8 bytes per counter >= t, two exchanges). stats_local: this
 * rank's nodes and counters; stats_total: the sums over the ranks, the same on every rank (either may be NULL). At most 256 ranks;
 * a communicator of another context gives KMI_ERR_INVALID. Argument errors are every rank's alike and return before anything
 * collective; a rank that fails on its own does not leave its peers waiting: the verdict is agreed on by an all-reduce before
 * each of the two exchanges and again before the maps change, and the peers return KMI_ERR_PEER (an error of the transport inside an
 * exchange is not such a failure: it is reported to every rank by the exchange itself). A one-rank communicator gives what
 * kmi_dbg_prune_edges gives (with KMI_FORCE_DIST=1 through the code of several ranks, the rank being its own peer; n_requests then
 * counts the requests it sent itself). kmi_ctx_debug_counter 13 gives the bytes this rank sent. */
typedef struct {
  uint64_t n_nodes;           /* nodes of the map (this rank's; _total: all ranks') */
  uint64_t n_set_before;      /* counters that were not 0 */
  uint64_t n_weak;            /* cleared by rule 1 */
  uint64_t n_absent;          /* cleared by rule 2 */
  uint64_t n_unreciprocated;  /* cleared by rule 3 */
  uint64_t n_set_after;       /* = n_set_before - n_weak - n_absent - n_unreciprocated */
  uint64_t n_isolated;        /* nodes whose eight counters are all 0 afterwards */
  uint64_t n_requests;        /* neighbour requests this rank sent over the communicator: 0 in the one-rank call; under KMI_FORCE_DIST=1 the requests
                                 the one rank sent to itself */
} kmi_dbg_prune_stats;  /* 64 bytes */
kmi_status kmi_dbg_spectrum_host(kmi_dbg *g, uint32_t n_bins, uint64_t *hist, kmi_spectrum_totals *totals /* may be NULL */);
kmi_status kmi_dbg_spectrum_dist_host(kmi_dbg *g, kmi_comm *comm, uint32_t n_bins, uint64_t *hist, kmi_spectrum_totals *totals /* may be NULL */);
kmi_status kmi_dbg_retain_counts(kmi_dbg *g, uint32_t lo, uint32_t hi, uint64_t *n_erased /* may be NULL */);
kmi_status kmi_dbg_prune_edges(kmi_dbg *g, uint32_t min_edge_count, kmi_dbg_prune_stats *stats /* may be NULL */);
kmi_status kmi_dbg_prune_edges_dist_host(kmi_dbg *g, kmi_comm *comm, uint32_t min_edge_count, kmi_dbg_prune_stats *stats_local,
                                         kmi_dbg_prune_stats *stats_total);

/* ---- clipping tips: short dead-end unitigs that hang off a junction (no counterpart in the reference)
 * The count filter and the pruning above remove what is rare; an error near a read's end that is seen often enough to pass the
 * filter survives them as a dead-end chain of a few nodes, and the junction it hangs off splits the true path into three unitigs.
 * kmi_dbg_clip_tips removes such chains. With t = min_edge_count >= 1 and M = max_tip_nodes >= 1; counters are read as the
 * compaction reads them (0 / 1 for an EDGE_EXISTS map); everything is judged against the map AS IT WAS WHEN THE CALL BEGAN, so one
 * call is one round and a pure function of the map:
 *  1. Unitigs. Those of kmi_dbg_compact with threshold t (its rules 1-4). Cycles are never clipped. A path unitig X has two ends:
 *     the ends of its first and of its last node that its links do not use (both ends of the node when X is a single node). The
 *     degree of an end is rule 1's of the compaction.
 *  2. Island. X has at most M nodes and both its ends have degree 0. Counted; removed only with KMI_DBG_CLIP_ISLANDS.
 *  3. Candidate. X has at most M nodes; one end is dead (degree 0); the other end (v, E) has degree exactly 1, with base b; the
 *     neighbour w of the counter (v, E, b) -- the pruning's definition above -- is a node and not a node of X; and the reciprocal
 *     counter (w, E', b') is >= t. That counter is X's junction counter and (w, E') its junction end. X is not linked into w, so on
 *     a pruned map (w, E') has degree >= 2.
 *  4. Verdict. The counters >= t at a junction end are ordered by the key (value, 1 if the counter is NOT the junction counter of a
 *     candidate else 0, -base index). A candidate is clipped if and only if another counter >= t of its junction end has a greater
 *     key. So the greatest branch of every end always stays and a junction is never eroded to nothing; a real continuation beats
 *     a tip of equal weight; of two tips of equal weight the one with the smaller base stays.
 *  5. Effect, as in retain_counts. The nodes of the clipped tips, and of the islands when asked, leave the map; the junction
 *     counter of every clipped tip is cleared, in a node that stays; every other counter and every counts[8] keeps its value bit
 *     for bit; the survivors keep their order, in fresh arrays of exactly the surviving size. When nothing leaves, the map stays
 *     as it is.
 * Consequences. A candidate's junction node never lies in a clipped unitig: the ends of a candidate and of an island have degrees
 * 0 and at most 1, and a clipped tip's junction end has degree >= 2 (its junction counter and the greater one). So on a map where
 * prune_edges(t) clears nothing and no node is its own reverse complement (any odd k), a round leaves no counter that points at a
 * removed node, and prune_edges(t) clears nothing on the result either. (For even k the exemption of the pruning's rule 3 breaks
 * this: a counter beside a palindromic node need not be reciprocated.) A tip longer than M nodes stays; the usual M is 2 k. One
 * round can uncover new tips (a tip on a tip): call again, with prune_edges in between, until n_tips_clipped is 0.
 * KMI_ERR_INVALID: t = 0; M = 0; flag bits other than KMI_DBG_CLIP_ISLANDS; an alphabet that is not 2-bit; a map that holds one
 * rank's share of a build over ranks (as kmi_dbg_compact and kmi_dbg_prune_edges refuse it). KMI_ERR_OVERFLOW: 2^31 - 1 nodes or
 * more. An empty map gives zeros. On any error the map holds what it held, and so does the result of an earlier compaction; a call
 * that succeeds drops it, and the stats are zeroed on an error. The call is complete on return.
 * _dist_host (collective): the graph is the union of the ranks' maps; rules 1-5 apply to that union unchanged, judged against the
 * maps as they were when the call began, and the union afterwards is exactly what kmi_dbg_clip_tips gives on the whole map. Each
 * rank keeps its surviving nodes in their order, rows bit for bit, in fresh arrays of the surviving size. A clipped tip's junction
 * node usually lives on another rank than the tip's nodes, so a rank from which no node leaves can still have a counter cleared: it
 * rewrites its rows; only a rank with nothing leaving and nothing cleared keeps its arrays. The protocol, after the stages of
 * kmi_dbg_compact_dist_host up to its heads (which leave every node with its unitig's two end states and its distances to them):
 *  - end degrees: per path unitig of at most M nodes each end state's owner sends the degree of its end to the other end's owner,
 *    one record of 16 bytes, one exchange (a one-node unitig's record goes to its own rank);
 *  - junction: the degree-1 end of a unitig whose other end is dead sends one request of (n_words + 2) x 8 bytes (the canonical
 *    neighbour k-mer; its own state and the reciprocal counter; the unitig's identity, the smaller of its two end states) to the
 *    owner of the neighbour, which applies rules 3 and 4 from its own rows and answers 16 bytes (state, candidate, clipped): two
 *    exchanges;
 *  - verdict: every node of a path unitig of at most M nodes asks the owners of both end states of its unitig, 16 bytes out and 16
 *    back per end, two exchanges, and leaves when either says so. Nodes of longer unitigs and of cycles send nothing.
 * stats_local: n_nodes, n_nodes_removed and n_counters_cleared count this rank's nodes and the counters cleared in them; n_unitigs
 * the unitigs this rank owns by the ownership rule of kmi_dbg_compact_dist_host; n_islands / n_islands_removed count an island on the
 * rank that holds the smaller of its two end states (rank << 32 | 2 * node + direction); n_candidates / n_tips_clipped count a
 * candidate on the rank that holds its attached node, the one whose end has degree 1. stats_total: the sums over the ranks, the same
 * on every rank. Either may be NULL. Refusals and limits are those of kmi_dbg_prune_edges_dist_host and of kmi_dbg_clip_tips:
 * t = 0, M = 0, unknown flags, an alphabet that is not 2-bit, a communicator of another context and more than 256 ranks give
 * KMI_ERR_INVALID on every rank alike, before anything collective; 2^31 - 1 or more nodes on a rank give KMI_ERR_OVERFLOW. A rank
 * that fails on its own does not leave its peers waiting: the verdict is agreed on by an all-reduce before the first exchange,
 * before each exchange that follows a step of the rank's own, and, with the fresh arrays filled, before the maps change -- all ranks
 * swap or none does -- and the peers return KMI_ERR_PEER. On any error the map and an earlier compaction's result stay and the stats
 * are zeroed; a call that succeeds drops that result on every rank, whether the rank lost a node or not. A one-rank communicator
 * gives what kmi_dbg_clip_tips gives (with KMI_FORCE_DIST=1 through the code of several ranks, the rank being its own peer).
 * kmi_dbg_clip_tips itself keeps refusing a rank's share. kmi_ctx_debug_counter 14 and 15 give the exchanges and the bytes this
 * rank sent. */
enum { KMI_DBG_CLIP_ISLANDS = 1u };
typedef struct {
  uint64_t n_nodes;            /* nodes of the map when the call began */
  uint64_t n_unitigs;          /* unitigs of that map under t (paths and cycles): what kmi_dbg_compact(t) would report */
  uint64_t n_candidates;       /* rule 3 */
  uint64_t n_tips_clipped;     /* candidates removed by rule 4 */
  uint64_t n_islands;          /* rule 2 */
  uint64_t n_islands_removed;  /* = n_islands with KMI_DBG_CLIP_ISLANDS, else 0 */
  uint64_t n_nodes_removed;
  uint64_t n_counters_cleared; /* junction counters of clipped tips, cleared in surviving nodes */
} kmi_dbg_clip_stats;  /* 64 bytes */
kmi_status kmi_dbg_clip_tips(kmi_dbg *g, uint32_t min_edge_count, uint32_t max_tip_nodes, uint32_t flags,
                             kmi_dbg_clip_stats *stats /* may be NULL */);
kmi_status kmi_dbg_clip_tips_dist_host(kmi_dbg *g, kmi_comm *comm, uint32_t min_edge_count, uint32_t max_tip_nodes, uint32_t flags,
                                       kmi_dbg_clip_stats *stats_local, kmi_dbg_clip_stats *stats_total);

/* ---- popping bubbles: parallel unitigs between the same two junction ends (no counterpart in the reference)
 * A substitution in the middle of a read that is seen often enough to pass the filter is not a dead end: it is a second path of
 * about k nodes that leaves a junction and rejoins the true path k nodes later, and each such bubble cuts the true path into three
 * unitigs and adds a fourth. kmi_dbg_pop_bubbles removes the lesser paths. With t = min_edge_count >= 1 and M = max_bubble_nodes
 * >= 1; counters are read as the compaction reads them (0 / 1 for an EDGE_EXISTS map); everything is judged against the map AS IT
 * WAS WHEN THE CALL BEGAN, so one call is one round and a pure function of the map:
 *  1. Unitigs. Those of kmi_dbg_compact with threshold t. Cycles are never branches. Ends and their degrees are those of the tip
 *     clipping's rule 1.
 *  2. Branch. A path unitig X of any length is a branch when both its ends have degree exactly 1; for each end the neighbour w
 *     behind that counter (the pruning's definition) is a node and not a node of X; for each end the reciprocal counter
 *     (w, E', b') is >= t; and the two junction nodes w0 and w1 are different nodes. The two reciprocal counters are X's junction
 *     counters and (w0, E0'), (w1, E1') its junction ends. A loop that leaves and re-enters one node is no branch.
 *  3. Siblings, bubble. Branches with the same unordered pair of junction ends are siblings; a set of two or more siblings is a
 *     bubble. Siblings differ in the base of their junction counter at either end: two counters of one end are two bases.
 *  4. Key. With c0, c1 the values of X's two junction counters, read in the junction nodes, and b the base index of X's junction
 *     counter at the junction node whose canonical k-mer is the smaller of the two (A < C < G < T, as the cycle cut compares
 *     keys): key(X) = (min(c0, c1), max(c0, c1), -b), a total order within a bubble.
 *  5. Verdict. A branch of at most M nodes is popped if and only if a sibling of any length has a greater key. So the greatest
 *     branch of every bubble always stays; a branch longer than M can outweigh others but never leaves; of equal weights the
 *     smaller base at the smaller junction node stays.
 *  6. Effect, as in retain_counts and clip_tips. The nodes of the popped branches leave the map; both junction counters of every
 *     popped branch are cleared, in nodes that stay; every other counter and every counts[8] keeps its value bit for bit; the
 *     survivors keep their order, in fresh arrays of exactly the surviving size. When nothing leaves, the map stays as it is.
 * Consequences. A junction end of a bubble has degree >= 2 and a branch's ends have degree 1, so a junction node never lies in a
 * popped branch. On a map where prune_edges(t) clears nothing and no node is its own reverse complement (any odd k), a round
 * leaves no counter that points at a removed node, and prune_edges(t) clears nothing on the result either; for even k the
 * exemption of the pruning's rule 3 breaks that, as it does for tips. Tips and bubbles do not commute. The intended loop: clip_tips
 * + prune_edges until nothing is clipped, then pop_bubbles + prune_edges until nothing is popped, then again from the top if the
 * last pass removed anything.
 * KMI_ERR_INVALID: t = 0; M = 0; any flag bit (none is defined: flags must be 0); an alphabet that is not 2-bit; a map that holds
 * one rank's share of a build over ranks (a whole map built over a one-rank communicator is accepted). KMI_ERR_OVERFLOW: 2^31 - 1
 * nodes or more. An empty map gives zeros. On any error the map holds what it held, and so does the result of an earlier
 * compaction, and the stats are zeroed; a call that succeeds drops that result. The call is complete on return.
 * _dist_host (collective): the graph is the union of the ranks' maps; rules 1-6 apply to that union unchanged, judged against the
 * maps as they were when the call began, and the union afterwards is exactly what kmi_dbg_pop_bubbles gives on the whole map. Each
 * rank keeps its surviving nodes in their order, rows bit for bit apart from the cleared junction counters, in fresh arrays of the
 * surviving size. A junction node usually lives on another rank than the branch's nodes, so a rank from which no node leaves can
 * still have a counter cleared: it rewrites its rows; only a rank with nothing leaving and nothing cleared keeps its arrays. The
 * protocol, after the stages of kmi_dbg_compact_dist_host up to its heads (kmi_dbg_bubbles_dist.h has the record layouts); the
 * IDENTITY END of a unitig is the smaller of its two end states (rank << 32 | 2 * node + direction):
 *  - junction: every end of degree 1 of a path unitig of any length sends (n_words + 2) x 8 bytes (the canonical neighbour k-mer;
 *    its own state and the reciprocal counter; the unitig's identity) to the owner of the neighbour, which applies rule 2 for that
 *    end from its own rows and answers 16 bytes (junction node, counter, its value): two exchanges;
 *  - pairing: the identity end asks the other end for its junction, 16 bytes out, (n_words + 3) x 8 back (the junction node's k-mer
 *    travels: rule 4 asks which junction node has the smaller one): two exchanges. The branch is assembled at the identity end;
 *  - matching: each branch goes to the owner of its junction node with the smaller k-mer, where its siblings arrive too,
 *    (n_words + 2) x 8 bytes, and gets 16 bytes back (has a sibling, has a greater sibling): two exchanges;
 *  - clears: a popped branch sends one 16-byte record to the owner of either junction node: one exchange;
 *  - telling: every node of a path unitig of at most M nodes asks the owner of its identity end, 16 bytes out and 16 back: two
 *    exchanges. Nodes of longer unitigs and of cycles send nothing.
 * stats_local: n_nodes, n_nodes_removed and n_counters_cleared count this rank's nodes and the counters cleared in them; n_unitigs
 * the unitigs this rank owns by the ownership rule of kmi_dbg_compact_dist_host; n_branches and n_popped count a branch on the rank
 * that holds its identity end; n_bubbles counts a bubble on the rank that holds the junction node with the smaller k-mer of its two,
 * where its greatest branch is judged. stats_total: the sums over the ranks, the same on every rank; each field equals the one-rank
 * call's on the whole map. Either may be NULL. Refusals and limits are those of kmi_dbg_clip_tips_dist_host: t = 0, M = 0, any flag
 * bit, an alphabet that is not 2-bit, a communicator of another context and more than 256 ranks give KMI_ERR_INVALID on every rank
 * alike, before anything collective; 2^31 - 1 or more nodes on a rank give KMI_ERR_OVERFLOW. A rank that fails on its own does not
 * leave its peers waiting: the verdict is agreed on by an all-reduce before the first exchange, before each exchange that follows a
 * step of the rank's own, and, with the fresh arrays filled, before the maps change -- all ranks swap or none does -- and the peers
 * return KMI_ERR_PEER. On any error the map and an earlier compaction's result stay and the stats are zeroed; a call that succeeds
 * drops that result on every rank, whether the rank lost a node or not. A one-rank communicator gives what kmi_dbg_pop_bubbles
 * gives (with KMI_FORCE_DIST=1 through the code of several ranks, the rank being its own peer). kmi_dbg_pop_bubbles itself keeps
 * refusing a rank's share. kmi_ctx_debug_counter 16 and 17 give the exchanges and the bytes this rank sent, stages included. */
typedef struct {
  uint64_t n_nodes;            /* nodes of the map when the call began */
  uint64_t n_unitigs;          /* unitigs of that map under t (paths and cycles): what kmi_dbg_compact(t) would report */
  uint64_t n_branches;         /* rule 2 */
  uint64_t n_bubbles;          /* sibling sets of two or more: the branches that have a sibling and no sibling with a greater key */
  uint64_t n_popped;           /* branches removed by rule 5 */
  uint64_t n_nodes_removed;
  uint64_t n_counters_cleared; /* junction counters of popped branches, cleared in surviving nodes: 2 x n_popped */
  uint64_t reserved;           /* 0 */
} kmi_dbg_pop_stats;  /* 64 bytes */
kmi_status kmi_dbg_pop_bubbles(kmi_dbg *g, uint32_t min_edge_count, uint32_t max_bubble_nodes, uint32_t flags,
                               kmi_dbg_pop_stats *stats /* may be NULL */);
kmi_status kmi_dbg_pop_bubbles_dist_host(kmi_dbg *g, kmi_comm *comm, uint32_t min_edge_count, uint32_t max_bubble_nodes, uint32_t flags,
                                         kmi_dbg_pop_stats *stats_local, kmi_dbg_pop_stats *stats_total);

/* ---- measurement support --------------------------------------------------- */
/* per-kernel HIP-event timing on the context's stream (bench.py roofline leg) */
kmi_status kmi_profile_enable(kmi_ctx *ctx, int on);
kmi_status kmi_profile_reset(kmi_ctx *ctx);
/* writes up to cap records; returns count in *n. name points to static storage. */
typedef struct { const char *name; double total_ms; uint64_t launches; uint64_t units; } kmi_kernel_time;
kmi_status kmi_profile_get(kmi_ctx *ctx, kmi_kernel_time *out, size_t cap, size_t *n);

/* deterministic synthetic inputs of SURVEY.md 8(d) (host side, splitmix64):
 * genome of g bases, r reads of read_len as 4-line FASTQ records with a 9-digit id
 * (315 bytes per 150-bp record). reads [first_read, first_read + n_reads) of the
 * data set defined by (seed, genome_len). Returns bytes written. */
size_t kmi_synth_fastq_bytes(uint64_t n_reads, uint32_t read_len);
kmi_status kmi_synth_fastq(uint64_t seed, uint64_t genome_len, uint32_t read_len, uint64_t first_read,
                           uint64_t n_reads, uint8_t *out, size_t out_capacity, uint32_t threads);

#ifdef __cplusplus
}
#endif
#endif /* KMERIND_HIP_H */
