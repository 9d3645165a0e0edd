// The reference's de Bruijn sample (test/test/test_de_bruijn_graph_construction.cpp) against kmerind/de_bruijn.hpp: the
// same type aliases, build_posix + find for the edge-count and the edge-existence node maps. Where the reference only
// prints sizes, this prints checksums the test harness compares with its checker. The parser (FASTQParser or FASTAParser)
// follows the file's extension.
//
//   de_bruijn_graph_construction <file.fastq | file.fasta>
//   de_bruijn_graph_construction <file> <rank> <size> <rendezvous_dir>
//
// The second form runs as rank `rank` of `size` processes, one graph over all of them: kmerind::comm.transport is a small host
// messenger over AF_UNIX sockets in rendezvous_dir (rank 0 listens and relays both collectives), the stand-in for the MPI
// communicator of the reference's program. Every rank prints its local_size(), the collective size() and checksums of its nodes.
#include <sys/socket.h>
#include <sys/un.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "kmerind/de_bruijn.hpp"

using WordType = uint64_t;
using Alphabet = bliss::common::DNA;
using KmerType = bliss::common::Kmer<21, Alphabet, WordType>;
using EdgeEncoder = bliss::common::DNA16;

template <typename K> using MapParams = ::bliss::index::kmer::BimoleculeHashMapParams<K>;
template <typename EdgeEnc>
using CountNodeMapType = bliss::de_bruijn::de_bruijn_nodes_distributed<KmerType, bliss::de_bruijn::node::edge_counts<EdgeEnc, int32_t>, MapParams>;
template <typename EdgeEnc>
using ExistNodeMapType = bliss::de_bruijn::de_bruijn_nodes_distributed<KmerType, bliss::de_bruijn::node::edge_exists<EdgeEnc>, MapParams>;

// ---- the socket messenger: rank 0 holds one connection per other rank and does every collective's arithmetic
namespace {
struct SocketMessenger {
  int rank = 0, size = 1;
  std::vector<int> fd;   // rank 0: fd[r] = the connection to rank r; other ranks: fd[0] = the connection to rank 0

  static void put(int s, const void *p, size_t n) {
    const char *c = static_cast<const char *>(p);
    while (n) { const ssize_t w = ::write(s, c, n); if (w <= 0) throw std::runtime_error("socket write"); c += w; n -= (size_t)w; }
  }
  static void get(int s, void *p, size_t n) {
    char *c = static_cast<char *>(p);
    while (n) { const ssize_t r = ::read(s, c, n); if (r <= 0) throw std::runtime_error("socket read"); c += r; n -= (size_t)r; }
  }

  SocketMessenger(int r, int p, const std::string &dir) : rank(r), size(p), fd(p, -1) {
    sockaddr_un a{};
    a.sun_family = AF_UNIX;
    const std::string path = dir + "/kmi_rendezvous.sock";
    if (path.size() >= sizeof(a.sun_path)) throw std::invalid_argument("rendezvous path too long");
    std::snprintf(a.sun_path, sizeof(a.sun_path), "%s", path.c_str());
    if (rank == 0) {
      const int ls = ::socket(AF_UNIX, SOCK_STREAM, 0);
      ::unlink(path.c_str());
      if (ls < 0 || ::bind(ls, (sockaddr *)&a, sizeof(a)) != 0 || ::listen(ls, p) != 0) throw std::runtime_error("cannot listen on " + path);
      for (int i = 1; i < p; ++i) {
        const int s = ::accept(ls, nullptr, nullptr);
        int who = -1;
        if (s < 0) throw std::runtime_error("accept");
        get(s, &who, sizeof(who));
        if (who <= 0 || who >= p || fd[who] >= 0) throw std::runtime_error("bad rank on the rendezvous socket");
        fd[who] = s;
      }
      ::close(ls);
      ::unlink(path.c_str());
    } else {
      const int s = ::socket(AF_UNIX, SOCK_STREAM, 0);
      bool ok = false;
      for (int t = 0; t < 6000 && !ok; ++t) {   // rank 0 may not be listening yet: up to a minute
        ok = ::connect(s, (sockaddr *)&a, sizeof(a)) == 0;
        if (!ok) std::this_thread::sleep_for(std::chrono::milliseconds(10));
      }
      if (!ok) throw std::runtime_error("cannot reach rank 0 at " + path);
      put(s, &rank, sizeof(rank));
      fd[0] = s;
    }
  }
  ~SocketMessenger() { for (int s : fd) if (s >= 0) ::close(s); }

  // kmi_transport::all_to_all_v: every rank's messages go to rank 0, which hands each rank what the others sent it
  static int all_to_all_v(void *user, const void *send, const uint64_t *send_bytes, void *recv, const uint64_t *recv_bytes) {
    SocketMessenger &m = *static_cast<SocketMessenger *>(user);
    const int p = m.size;
    try {
      uint64_t mine = 0, want = 0;
      for (int r = 0; r < p; ++r) { mine += send_bytes[r]; want += recv_bytes[r]; }
      if (m.rank != 0) {
        put(m.fd[0], send_bytes, sizeof(uint64_t) * p);
        put(m.fd[0], send, mine);
        get(m.fd[0], recv, want);
        return 0;
      }
      std::vector<std::vector<uint64_t>> cnt(p, std::vector<uint64_t>(p));
      std::vector<std::vector<char>> msg(p);
      std::copy(send_bytes, send_bytes + p, cnt[0].begin());
      msg[0].assign(static_cast<const char *>(send), static_cast<const char *>(send) + mine);
      for (int s = 1; s < p; ++s) {
        get(m.fd[s], cnt[s].data(), sizeof(uint64_t) * p);
        uint64_t n = 0;
        for (int r = 0; r < p; ++r) n += cnt[s][r];
        msg[s].resize(n);
        get(m.fd[s], msg[s].data(), n);
      }
      for (int d = 0; d < p; ++d) {
        std::vector<char> out;
        for (int s = 0; s < p; ++s) {
          uint64_t off = 0;
          for (int r = 0; r < d; ++r) off += cnt[s][r];
          out.insert(out.end(), msg[s].begin() + off, msg[s].begin() + off + cnt[s][d]);
        }
        if (d == 0) { if (out.size() != want) return 1; std::copy(out.begin(), out.end(), static_cast<char *>(recv)); }
        else put(m.fd[d], out.data(), out.size());
      }
      return 0;
    } catch (const std::exception &) { return 1; }
  }
  // kmi_transport::allreduce_u64: the values to rank 0, the sum (op 0) or maximum (op 1) back to everyone
  static int allreduce_u64(void *user, uint64_t *values, size_t n, int op) {
    SocketMessenger &m = *static_cast<SocketMessenger *>(user);
    try {
      if (m.rank != 0) { put(m.fd[0], values, sizeof(uint64_t) * n); get(m.fd[0], values, sizeof(uint64_t) * n); return 0; }
      std::vector<uint64_t> v(n);
      for (int s = 1; s < m.size; ++s) {
        get(m.fd[s], v.data(), sizeof(uint64_t) * n);
        for (size_t i = 0; i < n; ++i) values[i] = op == 1 ? std::max(values[i], v[i]) : values[i] + v[i];
      }
      for (int s = 1; s < m.size; ++s) put(m.fd[s], values, sizeof(uint64_t) * n);
      return 0;
    } catch (const std::exception &) { return 1; }
  }
};
}  // namespace

template <template <typename> class SeqParser>
static std::vector<KmerType> readForQuery(const std::string &filename, const kmerind::comm &comm) {
  std::vector<KmerType> query;
  ::bliss::io::KmerFileHelper::template read_file_posix<::bliss::index::kmer::KmerParser<KmerType>, SeqParser, ::bliss::io::SequencesIterator>(
      filename, query, comm);
  return query;
}

static uint64_t word_sum(const KmerType &k) { uint64_t s = 0; for (unsigned w = 0; w < KmerType::nWords; ++w) s += k.getData()[w]; return s; }

template <typename NodeMapType, template <typename> class SeqParser>
static void testDeBruijnGraph(const kmerind::comm &comm, const std::string &filename, const char *tag) {
  NodeMapType idx(comm);
  idx.template build_posix<SeqParser, ::bliss::io::SequencesIterator>(filename, comm);
  auto query = readForQuery<SeqParser>(filename, comm);
  if (query.size() > 50) query.resize(query.size() / 2);          // a part of the input's k-mers, repeats included
  auto results = idx.find(query);
  uint64_t edges = 0, self = 0, keys = 0, nbr = 0;
  for (auto &r : results) {
    keys += word_sum(r.first);
    for (int i = 0; i < 8; ++i) edges += (uint64_t)r.second.get_edge_frequency(i) * (uint64_t)(i + 1);
    std::vector<KmerType> out, in;
    bliss::de_bruijn::node::node_utils<KmerType, typename NodeMapType::ValueType>::get_out_neighbors(r.first, r.second, out);
    bliss::de_bruijn::node::node_utils<KmerType, typename NodeMapType::ValueType>::get_in_neighbors(r.first, r.second, in);
    for (auto &k : out) nbr += word_sum(k) % 1000003ull;
    for (auto &k : in) nbr += word_sum(k) % 1000003ull;
  }
  auto all = idx.to_vector();
  for (auto &r : all) self += (uint64_t)r.second.get_edge_frequency(0) + (uint64_t)r.second.get_edge_frequency(7);
  std::printf("%s nodes %zu size %zu found %zu keysum %llu edgesum %llu nbrsum %llu a_out_t_in %llu\n", tag, idx.local_size(), idx.size(),
              results.size(), (unsigned long long)keys, (unsigned long long)edges, (unsigned long long)nbr, (unsigned long long)self);
  // erase (the node map inherits it from the distributed map): every third query key's node leaves
  std::vector<KmerType> victims;
  for (size_t i = 0; i < query.size(); i += 3) victims.push_back(query[i]);
  const size_t erased = idx.erase(victims);
  uint64_t left = 0;
  for (auto &r : idx.to_vector()) left += word_sum(r.first) % 1000003ull;
  std::printf("%s erased %zu left %zu keysum %llu\n", tag, erased, idx.size(), (unsigned long long)left);
}

// one rank of several: the graph over all ranks, this rank's part of it summed up (the sums over the ranks are the whole graph's)
template <typename NodeMapType, template <typename> class SeqParser>
static void rankDeBruijnGraph(const kmerind::comm &comm, const std::string &filename, const char *tag) {
  NodeMapType idx(comm);
  idx.template build_posix<SeqParser, ::bliss::io::SequencesIterator>(filename, comm);
  const size_t total = idx.size();   // collective
  uint64_t keys = 0, edges = 0;
  for (auto &r : idx.to_vector()) {
    keys += word_sum(r.first) % 1000003ull;
    for (int i = 0; i < 8; ++i) edges += (uint64_t)r.second.get_edge_frequency(i) * (uint64_t)(i + 1);
  }
  std::printf("%s rank %d local_size %zu size %zu keysum %llu edgesum %llu\n", tag, comm.rank(), idx.local_size(), total, (unsigned long long)keys,
              (unsigned long long)edges);
}

template <template <typename> class SeqParser>
static void run(const kmerind::comm &comm, const std::string &filename, bool ranks) {
  if (ranks) {
    rankDeBruijnGraph<bliss::de_bruijn::de_bruijn_engine<CountNodeMapType>, SeqParser>(comm, filename, "count");
    rankDeBruijnGraph<bliss::de_bruijn::de_bruijn_engine<ExistNodeMapType>, SeqParser>(comm, filename, "exist");
    return;
  }
  testDeBruijnGraph<bliss::de_bruijn::de_bruijn_engine<CountNodeMapType>, SeqParser>(comm, filename, "count");
  testDeBruijnGraph<bliss::de_bruijn::de_bruijn_engine<ExistNodeMapType>, SeqParser>(comm, filename, "exist");
}

int main(int argc, char **argv) {
  if (argc != 2 && argc != 5) { std::fprintf(stderr, "usage: %s <file.fastq|file.fasta> [rank size rendezvous_dir]\n", argv[0]); return 2; }
  const std::string filename(argv[1]);
  try {
    const bool fasta = ::bliss::index::kmer::detail::format_of(filename) == KMI_FMT_FASTA;
    if (argc == 2) {
      kmerind::comm comm(0);
      if (fasta) run<::bliss::io::FASTAParser>(comm, filename, false);
      else run<::bliss::io::FASTQParser>(comm, filename, false);
      return 0;
    }
    const int rank = std::atoi(argv[2]), size = std::atoi(argv[3]);
    if (size < 1 || rank < 0 || rank >= size) { std::fprintf(stderr, "error: bad rank / size\n"); return 2; }
    SocketMessenger m(rank, size, argv[4]);
    kmerind::comm comm(0, rank, size);
    comm.transport.user = &m;
    comm.transport.all_to_all_v = &SocketMessenger::all_to_all_v;
    comm.transport.allreduce_u64 = &SocketMessenger::allreduce_u64;
    if (fasta) run<::bliss::io::FASTAParser>(comm, filename, true);
    else run<::bliss::io::FASTQParser>(comm, filename, true);
    std::fflush(stdout);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
