// Unitigs of a de Bruijn graph held over ranks, through kmerind/de_bruijn.hpp: every rank builds its share of the node map from its
// byte range of the file (build_posix with comm.size() > 1) and NodeIndex::unitigs() compacts the union of the shares collectively
// (kmi_dbg_compact_dist_host); each rank writes the unitigs it holds, in the format of de_bruijn_unitigs. An application fills
// kmerind::comm with its rank, size and either an RCCL id or its own transport. Started on its own the program is
// rank 0 of 1; with KMI_FORCE_DIST=1 in the environment that one rank still goes through the collective code, as its own peer.
//
//   de_bruijn_unitigs_ranks <file.fastq | file.fasta> <out.fasta> [min_edge_count]
//
// One summary line goes to stdout: "rank <r> of <p> unitigs <n> bases <b> total_unitigs <N> total_bases <B>".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "kmerind/de_bruijn.hpp"

using KmerType = bliss::common::Kmer<31, bliss::common::DNA, uint64_t>;
template <typename K> using MapParams = ::bliss::index::kmer::BimoleculeHashMapParams<K>;
template <typename EdgeEnc>
using CountNodeMapType = bliss::de_bruijn::de_bruijn_nodes_distributed<KmerType, bliss::de_bruijn::node::edge_counts<EdgeEnc, int32_t>, MapParams>;
using Graph = bliss::de_bruijn::de_bruijn_engine<CountNodeMapType>;

template <template <typename> class SeqParser>
static int run(const std::string &in, const std::string &out, uint32_t min_edge_count) {
  kmerind::comm comm(0);
  Graph g(comm);
  g.template build_posix<SeqParser, ::bliss::io::SequencesIterator>(in, comm);
  const std::vector<bliss::de_bruijn::Unitig> u = g.unitigs(min_edge_count);   // collective
  const std::pair<uint64_t, uint64_t> total = g.unitigs_total();
  FILE *f = std::fopen(out.c_str(), "w");
  if (!f) { std::fprintf(stderr, "error: cannot write %s\n", out.c_str()); return 1; }
  uint64_t bases = 0;
  for (size_t i = 0; i < u.size(); ++i) {
    std::fprintf(f, ">u%zu len=%zu occ=%llu circular=%d\n%s\n", i, u[i].sequence.size(), (unsigned long long)u[i].occurrences, u[i].circular ? 1 : 0,
                 u[i].sequence.c_str());
    bases += u[i].sequence.size();
  }
  if (std::fclose(f) != 0) { std::fprintf(stderr, "error: cannot write %s\n", out.c_str()); return 1; }
  std::printf("rank %d of %d unitigs %zu bases %llu total_unitigs %llu total_bases %llu\n", comm.rank(), comm.size(), u.size(), (unsigned long long)bases,
              (unsigned long long)total.first, (unsigned long long)total.second);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 3 && argc != 4) { std::fprintf(stderr, "usage: %s <file.fastq|file.fasta> <out.fasta> [min_edge_count]\n", argv[0]); return 2; }
  const std::string in(argv[1]), out(argv[2]);
  const long t = argc == 4 ? std::atol(argv[3]) : 1;
  if (t < 1) { std::fprintf(stderr, "error: min_edge_count must be at least 1\n"); return 2; }
  try {
    if (::bliss::index::kmer::detail::format_of(in) == KMI_FMT_FASTA) return run<::bliss::io::FASTAParser>(in, out, (uint32_t)t);
    return run<::bliss::io::FASTQParser>(in, out, (uint32_t)t);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
