// Cleaning a de Bruijn graph held over ranks down to its unitigs, bubbles included, through kmerind/de_bruijn.hpp: the pipeline of
// examples/de_bruijn_tips_ranks.cpp -- every rank builds its share of the node map from its byte range of the file, drops its nodes
// below a threshold (NodeIndex::retain_counts, local) and then, collectively, prunes (NodeIndex::prune_edges) and clips tips and
// prunes, round after round until a round clips nothing anywhere (NodeIndex::clip_tips) -- followed by rounds of bubble popping and
// pruning until a round pops nothing anywhere (NodeIndex::pop_bubbles: kmi_dbg_pop_bubbles_dist_host), and again from the tips if the
// popping removed anything, as examples/de_bruijn_bubbles.cpp does on one rank: tips and bubbles do not commute. Then it compacts
// (NodeIndex::unitigs) and each rank writes the unitigs it holds, in the format of de_bruijn_unitigs. An application fills
// kmerind::comm with its rank, size and either an RCCL id or its own transport. Started on its own the program is
// rank 0 of 1; with KMI_FORCE_DIST=1 in the environment that one rank still goes through the collective code, as its own peer.
//
//   de_bruijn_bubbles_ranks <file.fastq | file.fasta> <out.fasta> [min_count [max_nodes]]
//
// min_count and max_nodes as in de_bruijn_bubbles: 0 (the default) takes the first valley of the spectrum over all ranks; the
// longest tip that is clipped and the longest branch that is popped have 2 k nodes by default. One summary line per step goes to
// stdout, each starting "rank <r> of <p> <step>": build, retain_counts, prune_edges, then per pass clip_tips (one per round, with
// the pruning behind it; the last round is the one that clips nothing) and pop_bubbles (the same; the last round pops nothing), and
// unitigs. The last pass is the one whose bubble rounds pop nothing. Counts named total_* are over all ranks.
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
static int run(const std::string &in, const std::string &out, uint32_t min_count, uint32_t max_nodes) {
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
  unsigned pass = 0;
  while (true) {   // (the totals are every rank's alike: all ranks leave each loop together)
    ++pass;
    for (unsigned round = 1;; ++round) {
      kmi_dbg_clip_stats cl{};
      const kmi_dbg_clip_stats ct = g.clip_tips(1, max_nodes, 0, &cl);   // collective
      pt = g.prune_edges(1, &pl);
      std::printf("rank %d of %d clip_tips pass %u round %u clipped %llu nodes_removed %llu counters_cleared %llu total_candidates %llu total_clipped %llu "
                  "total_nodes_removed %llu pruned_behind %llu\n",
                  r, p, pass, round, (unsigned long long)cl.n_tips_clipped, (unsigned long long)cl.n_nodes_removed, (unsigned long long)cl.n_counters_cleared,
                  (unsigned long long)ct.n_candidates, (unsigned long long)ct.n_tips_clipped, (unsigned long long)ct.n_nodes_removed, cleared(pt));
      if (ct.n_tips_clipped == 0) break;
    }
    unsigned long long popped = 0;
    for (unsigned round = 1;; ++round) {
      kmi_dbg_pop_stats bl{};
      const kmi_dbg_pop_stats bt = g.pop_bubbles(1, max_nodes, &bl);   // collective
      pt = g.prune_edges(1, &pl);
      std::printf("rank %d of %d pop_bubbles pass %u round %u branches %llu bubbles %llu popped %llu nodes_removed %llu counters_cleared %llu "
                  "total_branches %llu total_bubbles %llu total_popped %llu total_nodes_removed %llu pruned_behind %llu\n",
                  r, p, pass, round, (unsigned long long)bl.n_branches, (unsigned long long)bl.n_bubbles, (unsigned long long)bl.n_popped,
                  (unsigned long long)bl.n_nodes_removed, (unsigned long long)bl.n_counters_cleared, (unsigned long long)bt.n_branches,
                  (unsigned long long)bt.n_bubbles, (unsigned long long)bt.n_popped, (unsigned long long)bt.n_nodes_removed, cleared(pt));
      popped += bt.n_popped;
      if (bt.n_popped == 0) break;
    }
    if (popped == 0) break;
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
  std::printf("rank %d of %d unitigs %zu bases %llu total_unitigs %llu total_bases %llu passes %u nodes %zu\n", r, p, u.size(), (unsigned long long)bases,
              (unsigned long long)total.first, (unsigned long long)total.second, pass, g.local_size());
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3 || argc > 5) { std::fprintf(stderr, "usage: %s <file.fastq|file.fasta> <out.fasta> [min_count [max_nodes]]\n", argv[0]); return 2; }
  const std::string in(argv[1]), out(argv[2]);
  const long min_count = argc >= 4 ? std::atol(argv[3]) : 0;
  const long max_nodes = argc >= 5 ? std::atol(argv[4]) : 2 * (long)KmerType::size;
  if (min_count < 0 || max_nodes < 1) { std::fprintf(stderr, "error: min_count is 0 (the spectrum's first valley) or more, max_nodes 1 or more\n"); return 2; }
  try {
    if (::bliss::index::kmer::detail::format_of(in) == KMI_FMT_FASTA) return run<::bliss::io::FASTAParser>(in, out, (uint32_t)min_count, (uint32_t)max_nodes);
    return run<::bliss::io::FASTQParser>(in, out, (uint32_t)min_count, (uint32_t)max_nodes);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
