// seed_reads over ranks, through kmerind/kmer_index.hpp: every rank builds its share of PositionIndex<Kmer<21, DNA>> (canonical)
// from its byte range of a FASTA reference (build_posix with comm.size() > 1), takes its own record-aligned share of a FASTQ file
// and asks, collectively, where every k-mer of its reads occurs in the WHOLE reference (Index::seed_reads ->
// kmi_index_seed_reads_dist_host): the k-mers travel to the ranks that own them, the hits come back in read order. An application
// fills kmerind::comm with its rank, size and either an RCCL id or its own transport. Started on its own the
// program is rank 0 of 1; with KMI_FORCE_DIST=1 in the environment that one rank still goes through the collective code, as its
// own peer.
//
//   seed_reads_ranks <reference.fasta> <reads.fastq> [max_occ]
//
// The table of seed_reads for THIS rank's reads: a header line "#seq_offset n_kmers n_listed n_hits", then per read, tab
// separated: the byte offset of its sequence in the rank's share of the file, its k-mer windows, how many of them have at least one
// listed hit (a k-mer with more than max_occ occurrences over all ranks lists none; default: no cap), and the read's listed hits.
// A last line "#total" gives the rank's reads, windows and hits.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "kmerind/kmer_index.hpp"

using KmerType = bliss::common::Kmer<21, bliss::common::DNA, uint64_t>;
template <typename Key> using MapParams = ::bliss::index::kmer::CanonicalHashMapParams<Key>;
using ValType = bliss::common::LongSequenceKmerId;
using PosMap = ::dsc::unordered_multimap<KmerType, ValType, MapParams>;
using PosIdx = bliss::index::kmer::PositionIndex<PosMap>;

int main(int argc, char **argv) {
  if (argc < 3 || argc > 4) { std::fprintf(stderr, "usage: %s <reference.fasta> <reads.fastq> [max_occ]\n", argv[0]); return 2; }
  const long long cap = argc == 4 ? std::atoll(argv[3]) : (long long)KMI_LOCATE_ALL;
  if (cap < 1 || cap > (long long)KMI_LOCATE_ALL) { std::fprintf(stderr, "error: max_occ must be at least 1\n"); return 2; }
  try {
    kmerind::comm comm(0);
    PosIdx idx(comm);
    idx.build_posix<::bliss::io::FASTAParser, ::bliss::io::SequencesIterator>(argv[1]);   // collective: this rank's block of the file
    const PosIdx::Seeds seeds = idx.seed_reads(argv[2], (uint32_t)cap);                    // collective: this rank's reads
    std::printf("#seq_offset\tn_kmers\tn_listed\tn_hits\n");
    for (const kmi_read_seeds &r : seeds.reads)
      std::printf("%llu\t%u\t%u\t%llu\n", (unsigned long long)r.seq_offset, r.n_kmers, r.n_listed, (unsigned long long)r.n_hits);
    std::printf("#total\t%llu\t%llu\t%llu\n", (unsigned long long)seeds.reads.size(), (unsigned long long)seeds.occ.size(),
                (unsigned long long)seeds.values.size());
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
