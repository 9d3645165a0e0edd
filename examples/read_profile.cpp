// k-mer coverage of reads against a count index, through kmerind/kmer_index.hpp: build CountIndex<Kmer<21, DNA>> (canonical) from
// one FASTQ file, profile the reads of a second one against it on the GPU (Index::profile_reads), print one line per read. The
// questions behind read screening, digital normalisation and error detection by k-mer coverage; no counterpart in the reference.
//
//   read_profile <index.fastq> <reads.fastq> [solid_threshold [sequence]]
//
// A header line "#seq_offset n_kmers n_present n_solid lowest highest sum", then per read, tab separated: the byte offset of its
// sequence in the file, its k-mers, how many of them the index holds, how many at least solid_threshold (default 2) times, and the
// lowest, highest and summed count (an absent k-mer counts 0). With a sequence of A, C, G, T on the command line, one more line
// follows: "#lookup" and the count of each of its k-mers, in order (Index::lookup).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "kmerind/kmer_index.hpp"

using KmerType = bliss::common::Kmer<21, bliss::common::DNA, uint64_t>;
template <typename Key> using MapParams = ::bliss::index::kmer::CanonicalHashMapParams<Key>;
using CountMap = ::dsc::counting_unordered_map<KmerType, uint32_t, MapParams>;
using CountIdx = bliss::index::kmer::CountIndex<CountMap>;

int main(int argc, char **argv) {
  if (argc < 3 || argc > 5) { std::fprintf(stderr, "usage: %s <index.fastq> <reads.fastq> [solid_threshold [sequence]]\n", argv[0]); return 2; }
  const long solid = argc >= 4 ? std::atol(argv[3]) : 2;
  if (solid < 1) { std::fprintf(stderr, "error: solid_threshold must be at least 1\n"); return 2; }
  try {
    kmerind::comm comm(0);
    CountIdx idx(comm);
    idx.build_posix<::bliss::io::FASTQParser, ::bliss::io::SequencesIterator>(argv[1]);
    const std::vector<kmi_read_profile> rows = idx.profile_reads(argv[2], (uint32_t)solid);
    std::printf("#seq_offset\tn_kmers\tn_present\tn_solid\tlowest\thighest\tsum\n");
    for (const kmi_read_profile &r : rows)
      std::printf("%llu\t%u\t%u\t%u\t%u\t%u\t%llu\n", (unsigned long long)r.seq_offset, r.n_kmers, r.n_present, r.n_solid, r.lowest, r.highest,
                  (unsigned long long)r.sum_counts);
    if (argc == 5) {
      std::vector<KmerType> q;
      KmerType km;
      size_t n = 0;
      for (const char *c = argv[4]; *c; ++c) {
        const char *at = std::strchr("ACGT", *c);
        if (!at) throw std::invalid_argument("the sequence holds a character other than A, C, G, T");
        km.nextFromChar((unsigned char)(at - "ACGT"));
        if (++n >= KmerType::size) q.push_back(km);
      }
      std::printf("#lookup");
      for (uint32_t c : idx.lookup(q)) std::printf("\t%u", c);
      std::printf("\n");
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
