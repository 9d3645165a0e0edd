// The count spectrum of a read set and the error filter read off it, through kmerind/kmer_index.hpp: build
// CountIndex<Kmer<21, DNA>> (canonical) from a FASTQ file, take its spectrum on the GPU (Index::count_spectrum), find the first
// local minimum -- the valley between the sequencing errors, which pile up at count 1, and the genomic k-mers around the coverage --
// and keep the k-mers at or above it (Index::retain_counts). No counterpart in the reference beyond to_vector() and a host loop.
//
//   count_spectrum <reads.fastq> [n_bins]
//
// Output, one "name<TAB>value" line each: bin0 .. bin15 (fewer when n_bins, default 256, is smaller), then entries, sum_counts,
// min_count, max_count, threshold, size_before, erased, size_after. A spectrum that never turns upwards has no valley: the
// threshold is then 1 and nothing is erased.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "kmerind/kmer_index.hpp"

using KmerType = bliss::common::Kmer<21, bliss::common::DNA, uint64_t>;
template <typename Key> using MapParams = ::bliss::index::kmer::CanonicalHashMapParams<Key>;
using CountMap = ::dsc::counting_unordered_map<KmerType, uint32_t, MapParams>;
using CountIdx = bliss::index::kmer::CountIndex<CountMap>;

int main(int argc, char **argv) {
  if (argc < 2 || argc > 3) { std::fprintf(stderr, "usage: %s <reads.fastq> [n_bins]\n", argv[0]); return 2; }
  const long n_bins = argc == 3 ? std::atol(argv[2]) : 256;
  if (n_bins < 2 || n_bins > KMI_SPECTRUM_MAX_BINS) { std::fprintf(stderr, "error: n_bins is 2 .. %d\n", (int)KMI_SPECTRUM_MAX_BINS); return 2; }
  try {
    kmerind::comm comm(0);
    CountIdx idx(comm);
    idx.build_posix<::bliss::io::FASTQParser, ::bliss::io::SequencesIterator>(argv[1]);
    kmi_spectrum_totals t{};
    const std::vector<uint64_t> hist = idx.count_spectrum((uint32_t)n_bins, &t);
    for (size_t c = 0; c < hist.size() && c < 16; ++c) std::printf("bin%zu\t%llu\n", c, (unsigned long long)hist[c]);
    std::printf("entries\t%llu\nsum_counts\t%llu\nmin_count\t%u\nmax_count\t%u\n", (unsigned long long)t.n_entries, (unsigned long long)t.sum_counts,
                t.min_count, t.max_count);
    // the first count c >= 1 whose bin is lower than the one before it and not higher than the one behind it (the open-ended last
    // bin is no candidate)
    uint32_t threshold = 1;
    for (size_t c = 1; c + 2 < hist.size(); ++c)
      if (hist[c] < hist[c - 1] && hist[c] <= hist[c + 1]) { threshold = (uint32_t)c; break; }
    const size_t before = idx.local_size();
    const size_t erased = idx.retain_counts(threshold);
    std::printf("threshold\t%u\nsize_before\t%zu\nerased\t%zu\nsize_after\t%zu\n", threshold, before, erased, idx.local_size());
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
