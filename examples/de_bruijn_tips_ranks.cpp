// Cleaning a de Bruijn graph held over ranks down to its unitigs, through kmerind/de_bruijn.hpp: every rank builds its share of the
// node map from its byte range of the file (build_posix with comm.size() > 1), drops its nodes below a threshold
// (NodeIndex::retain_counts, local), and then, collectively, clears the counters the survivors still hold towards them
// (NodeIndex::prune_edges), clips the short dead ends that hang off junctions (NodeIndex::clip_tips: kmi_dbg_clip_tips_dist_host) and
// prunes again, round after round until a round clips nothing anywhere, and compacts (NodeIndex::unitigs). Each rank writes the
// unitigs it holds, in the format of de_bruijn_unitigs. An application fills kmerind::comm with its rank, size and either an RCCL id
// or its own transport. Started on its own the program is rank 0 of 1; with KMI_FORCE_DIST=1 in the environment
// that one rank still goes through the collective code, as its own peer.
//
//   de_bruijn_tips_ranks <file.fastq | file.fasta> <out.fasta> [min_count [max_tip_nodes]]
//
// min_count and max_tip_nodes as in de_bruijn_tips: 0 (the default) takes the first valley of the spectrum over all ranks; the
// default tip length is 2 k nodes. One summary line per step goes to stdout, each starting "rank <r> of <p> <step>": build,
// retain_counts, prune_edges, clip_tips (one per round, with the pruning behind it; the last round is the one that clips nothing),
// unitigs. Counts named total_* are over all ranks.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "kmerind/de_bruijn.hpp"

using KmerType = bliss::common::Kmer<31, bliss::common::DNA, uint64_t>;
template <typename K> using MapParams = ::bliss::index::kmer::BimoleculeHashMapParams<K>;
template <typename EdgeEnc>
using CountNodeMapType = bliss::de_bruijn::de_bruijn_nodes_distributed<KmerType, bliss::de_bruijn::node::edge_counts<EdgeEnc, int32_t>, MapParams>;
using Graph = bliss::de_bruijn::de_bruijn_engine<CountNodeMapType>;

static unsigned long long cleared(const kmi_dbg_prune_stats &s) { return (unsigned long long)(s.n_set_before - s.n_set_after); }

template <template <typename> class SeqParser>
static int run(const std::string &in, const std::string &out, uint32_t min_count, uint32_t max_tip) {
  kmerind::comm comm(0);
  Graph g(comm);
  const int r = comm.rank(), p = comm.size();
  g.template build_posix<SeqParser, ::bliss::io::SequencesIterator>(in, comm);
  std::printf("rank %d of %d build nodes %zu\n", r, p, g.local_size());
  uint32_t threshold = min_count;
  if (threshold == 0) {   // the first count whose bin is lower than the one before it and not higher than the one behind it
    threshold = 1;
    const std::vector<uint64_t> hist = g.spectrum(256);   // collective: over all ranks
    for (size_t c = 1; c + 2 < hist.size(); ++c)
      if (hist[c] < hist[c - 1] && hist[c] <= hist[c + 1]) { threshold = (uint32_t)c; break; }
  }
  const size_t erased = g.retain_counts(threshold);
  std::printf("rank %d of %d retain_counts threshold %u erased %zu nodes %zu\n", r, p, threshold, erased, g.local_size());
  kmi_dbg_prune_stats pl{};
  kmi_dbg_prune_stats pt = g.prune_edges(1, &pl);   // collective
  std::printf("rank %d of %d prune_edges cleared %llu total_cleared %llu\n", r, p, cleared(pl), cleared(pt));
  unsigned round = 0;
  while (true) {
    ++round;
    kmi_dbg_clip_stats cl{};
    const kmi_dbg_clip_stats ct = g.clip_tips(1, max_tip, 0, &cl);   // collective
    pt = g.prune_edges(1, &pl);
    std::printf("rank %d of %d clip_tips round %u clipped %llu nodes_removed %llu counters_cleared %llu total_candidates %llu total_clipped %llu "
                "total_nodes_removed %llu pruned_behind %llu\n",
                r, p, round, (unsigned long long)cl.n_tips_clipped, (unsigned long long)cl.n_nodes_removed, (unsigned long long)cl.n_counters_cleared,
                (unsigned long long)ct.n_candidates, (unsigned long long)ct.n_tips_clipped, (unsigned long long)ct.n_nodes_removed, cleared(pt));
    if (ct.n_tips_clipped == 0) break;   // (the totals are every rank's alike: all ranks leave the loop together)
  }
  const std::vector<bliss::de_bruijn::Unitig> u = g.unitigs(1);   // collective
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
  std::printf("rank %d of %d unitigs %zu bases %llu total_unitigs %llu total_bases %llu rounds %u nodes %zu\n", r, p, u.size(), (unsigned long long)bases,
              (unsigned long long)total.first, (unsigned long long)total.second, round, g.local_size());
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3 || argc > 5) { std::fprintf(stderr, "usage: %s <file.fastq|file.fasta> <out.fasta> [min_count [max_tip_nodes]]\n", argv[0]); return 2; }
  const std::string in(argv[1]), out(argv[2]);
  const long min_count = argc >= 4 ? std::atol(argv[3]) : 0;
  const long max_tip = argc >= 5 ? std::atol(argv[4]) : 2 * (long)KmerType::size;
  if (min_count < 0 || max_tip < 1) { std::fprintf(stderr, "error: min_count is 0 (the spectrum's first valley) or more, max_tip_nodes 1 or more\n"); return 2; }
  try {
    if (::bliss::index::kmer::detail::format_of(in) == KMI_FMT_FASTA) return run<::bliss::io::FASTAParser>(in, out, (uint32_t)min_count, (uint32_t)max_tip);
    return run<::bliss::io::FASTQParser>(in, out, (uint32_t)min_count, (uint32_t)max_tip);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
