// Cleaning a de Bruijn graph of sequencing errors through kmerind/de_bruijn.hpp: build the edge-count node map from a FASTQ file,
// take the spectrum of the nodes' occurrences on the GPU (NodeIndex::spectrum), find its first valley as examples/count_spectrum
// does, drop the nodes below it (NodeIndex::retain_counts), clear the counters the survivors still hold towards them
// (NodeIndex::prune_edges) and compact (NodeIndex::unitigs). No counterpart in the reference, whose de Bruijn sample ends at the
// node map.
//
//   de_bruijn_clean <reads.fastq> [n_bins]
//
// Output, one "name<TAB>value" line each: nodes_before, unitigs_before, n50_before, threshold, erased, nodes_after, set_before,
// weak, absent, unreciprocated, set_after, isolated, unitigs_after, n50_after. N50 is over the unitigs' lengths in bases. A spectrum
// that never turns upwards has no valley: the threshold is then 1 and no node leaves.
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

int main(int argc, char **argv) {
  if (argc != 2 && argc != 3) { std::fprintf(stderr, "usage: %s <reads.fastq> [n_bins]\n", argv[0]); return 2; }
  const long n_bins = argc == 3 ? std::atol(argv[2]) : 256;
  if (n_bins < 2 || n_bins > KMI_SPECTRUM_MAX_BINS) { std::fprintf(stderr, "error: n_bins is 2 .. %d\n", (int)KMI_SPECTRUM_MAX_BINS); return 2; }
  try {
    kmerind::comm comm(0);
    Graph g(comm);
    g.build_posix<::bliss::io::FASTQParser, ::bliss::io::SequencesIterator>(std::string(argv[1]), comm);
    std::vector<bliss::de_bruijn::Unitig> u = g.unitigs();
    std::printf("nodes_before\t%zu\nunitigs_before\t%zu\nn50_before\t%llu\n", g.local_size(), u.size(), n50(u));
    const std::vector<uint64_t> hist = g.spectrum((uint32_t)n_bins);
    // the first count c >= 1 whose bin is lower than the one before it and not higher than the one behind it (the open-ended last
    // bin is no candidate)
    uint32_t threshold = 1;
    for (size_t c = 1; c + 2 < hist.size(); ++c)
      if (hist[c] < hist[c - 1] && hist[c] <= hist[c + 1]) { threshold = (uint32_t)c; break; }
    const size_t erased = g.retain_counts(threshold);
    std::printf("threshold\t%u\nerased\t%zu\nnodes_after\t%zu\n", threshold, erased, g.local_size());
    const kmi_dbg_prune_stats s = g.prune_edges(1);
    std::printf("set_before\t%llu\nweak\t%llu\nabsent\t%llu\nunreciprocated\t%llu\nset_after\t%llu\nisolated\t%llu\n", (unsigned long long)s.n_set_before,
                (unsigned long long)s.n_weak, (unsigned long long)s.n_absent, (unsigned long long)s.n_unreciprocated, (unsigned long long)s.n_set_after,
                (unsigned long long)s.n_isolated);
    u = g.unitigs();
    std::printf("unitigs_after\t%zu\nn50_after\t%llu\n", u.size(), n50(u));
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
