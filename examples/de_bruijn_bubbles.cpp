// Popping the bubbles of a de Bruijn graph through kmerind/de_bruijn.hpp: examples/de_bruijn_tips.cpp's pipeline -- build the
// edge-count node map from a FASTQ file, drop the nodes below a threshold (NodeIndex::retain_counts), clear the counters towards
// them (NodeIndex::prune_edges), clip the tips and prune, round after round until a round clips nothing (NodeIndex::clip_tips) --
// followed by rounds of bubble popping and pruning until a round pops nothing (NodeIndex::pop_bubbles), and again from the tips
// if the popping removed anything: tips and bubbles do not commute. No counterpart in the reference, whose de Bruijn sample ends
// at the node map.
//
//   de_bruijn_bubbles <reads.fastq> [min_count [max_nodes]]
//
// min_count: the nodes with fewer occurrences leave; 0 (the default) takes the first valley of the spectrum as
// examples/de_bruijn_clean does. max_nodes: the longest tip that is clipped and the longest branch that is popped, in nodes; the
// default is 2 k.
//
// Output, one "name<TAB>value" line each: nodes_built, unitigs_built, n50_built, threshold, erased, unitigs_filtered, n50_filtered,
// cleared_pruned, unitigs_pruned, n50_pruned, then per pass p = 1, 2, ... its tip rounds r = 1, 2, ...: p<p>_t<r>_candidates,
// _clipped, _nodes_removed, _cleared (by the pruning behind the step), _unitigs, _n50 -- the last round clips nothing -- and its
// bubble rounds: p<p>_b<r>_branches, _bubbles, _popped, _nodes_removed, _cleared, _unitigs, _n50 -- the last round pops nothing.
// The last pass is the one whose bubble rounds pop nothing. Then passes, nodes_final, unitigs_final, n50_final. N50 is over the
// unitigs' lengths in bases.
#include <algorithm>
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

static unsigned long long n50(const std::vector<bliss::de_bruijn::Unitig> &u) {
  std::vector<size_t> len;
  size_t total = 0;
  for (const auto &x : u) { len.push_back(x.sequence.size()); total += x.sequence.size(); }
  std::sort(len.begin(), len.end(), [](size_t a, size_t b) { return a > b; });
  size_t run = 0;
  for (size_t x : len) {
    run += x;
    if (2 * run >= total) return x;
  }
  return 0;
}

static unsigned long long cleared(const kmi_dbg_prune_stats &s) { return (unsigned long long)(s.n_set_before - s.n_set_after); }

int main(int argc, char **argv) {
  if (argc < 2 || argc > 4) { std::fprintf(stderr, "usage: %s <reads.fastq> [min_count [max_nodes]]\n", argv[0]); return 2; }
  const long min_count = argc >= 3 ? std::atol(argv[2]) : 0;
  const long max_nodes = argc >= 4 ? std::atol(argv[3]) : 2 * (long)KmerType::size;
  if (min_count < 0 || max_nodes < 1) { std::fprintf(stderr, "error: min_count is 0 (the spectrum's first valley) or more, max_nodes 1 or more\n"); return 2; }
  try {
    kmerind::comm comm(0);
    Graph g(comm);
    g.build_posix<::bliss::io::FASTQParser, ::bliss::io::SequencesIterator>(std::string(argv[1]), comm);
    std::vector<bliss::de_bruijn::Unitig> u = g.unitigs();
    std::printf("nodes_built\t%zu\nunitigs_built\t%zu\nn50_built\t%llu\n", g.local_size(), u.size(), n50(u));
    uint32_t threshold = (uint32_t)min_count;
    if (threshold == 0) {   // the first count whose bin is lower than the one before it and not higher than the one behind it
      threshold = 1;
      const std::vector<uint64_t> hist = g.spectrum(256);
      for (size_t c = 1; c + 2 < hist.size(); ++c)
        if (hist[c] < hist[c - 1] && hist[c] <= hist[c + 1]) { threshold = (uint32_t)c; break; }
    }
    const size_t erased = g.retain_counts(threshold);
    u = g.unitigs();
    std::printf("threshold\t%u\nerased\t%zu\nunitigs_filtered\t%zu\nn50_filtered\t%llu\n", threshold, erased, u.size(), n50(u));
    kmi_dbg_prune_stats p = g.prune_edges(1);
    u = g.unitigs();
    std::printf("cleared_pruned\t%llu\nunitigs_pruned\t%zu\nn50_pruned\t%llu\n", cleared(p), u.size(), n50(u));
    unsigned pass = 0;
    while (true) {
      ++pass;
      for (unsigned r = 1;; ++r) {
        const kmi_dbg_clip_stats s = g.clip_tips(1, (uint32_t)max_nodes, 0);
        p = g.prune_edges(1);
        u = g.unitigs();
        std::printf("p%u_t%u_candidates\t%llu\np%u_t%u_clipped\t%llu\np%u_t%u_nodes_removed\t%llu\np%u_t%u_cleared\t%llu\np%u_t%u_unitigs\t%zu\np%u_t%u_n50\t%llu\n",
                    pass, r, (unsigned long long)s.n_candidates, pass, r, (unsigned long long)s.n_tips_clipped, pass, r,
                    (unsigned long long)s.n_nodes_removed, pass, r, cleared(p), pass, r, u.size(), pass, r, n50(u));
        if (s.n_tips_clipped == 0) break;
      }
      unsigned long long popped = 0;
      for (unsigned r = 1;; ++r) {
        const kmi_dbg_pop_stats s = g.pop_bubbles(1, (uint32_t)max_nodes);
        p = g.prune_edges(1);
        u = g.unitigs();
        std::printf("p%u_b%u_branches\t%llu\np%u_b%u_bubbles\t%llu\np%u_b%u_popped\t%llu\np%u_b%u_nodes_removed\t%llu\np%u_b%u_cleared\t%llu\n"
                    "p%u_b%u_unitigs\t%zu\np%u_b%u_n50\t%llu\n",
                    pass, r, (unsigned long long)s.n_branches, pass, r, (unsigned long long)s.n_bubbles, pass, r, (unsigned long long)s.n_popped, pass, r,
                    (unsigned long long)s.n_nodes_removed, pass, r, cleared(p), pass, r, u.size(), pass, r, n50(u));
        popped += s.n_popped;
        if (s.n_popped == 0) break;
      }
      if (popped == 0) break;
    }
    std::printf("passes\t%u\nnodes_final\t%zu\nunitigs_final\t%zu\nn50_final\t%llu\n", pass, g.local_size(), u.size(), n50(u));
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
