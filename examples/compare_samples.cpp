// Two read sets joined on the GPU, through kmerind/kmer_index.hpp: build CountIndex<Kmer<k, DNA>> (canonical) from each FASTQ file
// in ONE context, compare them (Index::compare: shared k-mers, Jaccard and weighted Jaccard), and combine them (Index::combine):
// the k-mers private to the first sample, the shared ones, and the two samples merged. No counterpart in the reference beyond
// to_vector() of one map, find() in the other and a host loop.
//
//   compare_samples <a.fastq> <b.fastq> [k=21]        (k = 21 or 31)
//
// Output, one "name<TAB>value" line each: n_a, n_b, n_shared, sum_a, sum_b, sum_a_shared, sum_b_shared, sum_min_shared, jaccard,
// weighted_jaccard (six decimals), then a_only (SUBTRACT_KEYS on a copy of a built again), shared (INTERSECT_MIN), merged
// (UNION_ADD) and merged_sum_counts (the merged index's sum of counts, from its spectrum).
#include <cstdio>
#include <cstdlib>
#include <string>

#include "kmerind/kmer_index.hpp"

template <typename Key> using MapParams = ::bliss::index::kmer::CanonicalHashMapParams<Key>;

template <unsigned K>
static int run(const char *path_a, const char *path_b) {
  using KmerType = bliss::common::Kmer<K, bliss::common::DNA, uint64_t>;
  using CountMap = ::dsc::counting_unordered_map<KmerType, uint32_t, MapParams>;
  using CountIdx = bliss::index::kmer::CountIndex<CountMap>;
  using SameCtx = typename CountIdx::same_context_t;
  kmerind::comm comm(0);
  CountIdx a(comm);
  CountIdx b(a, SameCtx{});   // both operands live in a's context
  a.template build_posix<::bliss::io::FASTQParser, ::bliss::io::SequencesIterator>(path_a);
  b.template build_posix<::bliss::io::FASTQParser, ::bliss::io::SequencesIterator>(path_b);
  const kmi_index_overlap o = a.compare(b);
  std::printf("n_a\t%llu\nn_b\t%llu\nn_shared\t%llu\nsum_a\t%llu\nsum_b\t%llu\nsum_a_shared\t%llu\nsum_b_shared\t%llu\nsum_min_shared\t%llu\n",
              (unsigned long long)o.n_a, (unsigned long long)o.n_b, (unsigned long long)o.n_shared, (unsigned long long)o.sum_a,
              (unsigned long long)o.sum_b, (unsigned long long)o.sum_a_shared, (unsigned long long)o.sum_b_shared,
              (unsigned long long)o.sum_min_shared);
  const uint64_t n_union = o.n_a + o.n_b - o.n_shared, w_union = o.sum_a + o.sum_b - o.sum_min_shared;
  std::printf("jaccard\t%.6f\nweighted_jaccard\t%.6f\n", n_union ? (double)o.n_shared / (double)n_union : 0.0,
              w_union ? (double)o.sum_min_shared / (double)w_union : 0.0);
  {
    CountIdx c(a, SameCtx{});
    c.template build_posix<::bliss::io::FASTQParser, ::bliss::io::SequencesIterator>(path_a);
    std::printf("a_only\t%zu\n", c.combine(b, KMI_COMBINE_SUBTRACT_KEYS));
  }
  {
    CountIdx c(a, SameCtx{});
    c.template build_posix<::bliss::io::FASTQParser, ::bliss::io::SequencesIterator>(path_a);
    const size_t merged = c.combine(b, KMI_COMBINE_UNION_ADD);
    kmi_spectrum_totals t{};
    (void)c.count_spectrum(2, &t);
    std::printf("shared\t%zu\n", a.combine(b, KMI_COMBINE_INTERSECT_MIN));
    std::printf("merged\t%zu\nmerged_sum_counts\t%llu\n", merged, (unsigned long long)t.sum_counts);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3 || argc > 4) { std::fprintf(stderr, "usage: %s <a.fastq> <b.fastq> [k=21]\n", argv[0]); return 2; }
  const long k = argc == 4 ? std::atol(argv[3]) : 21;
  try {
    if (k == 21) return run<21>(argv[1], argv[2]);
    if (k == 31) return run<31>(argv[1], argv[2]);
    std::fprintf(stderr, "error: k is 21 or 31\n");
    return 2;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
