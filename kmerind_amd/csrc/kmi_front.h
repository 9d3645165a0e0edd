// kmi_front.h -- the FASTQ front end of the super-k-mer build in ONE pass over the input bytes (included by kmi_index.hip).
//
// What it replaces: fastq_scan_tiles (classify every byte, EOL bitmap, packed stream), fastq_scan_offsets (line bases),
// fastq_list (runs of k-mer windows per tile) and sk_minimizer (the walk) -- i.e. FASTQParser::get_next_record
// (fastq_loader.hpp:389-467) + KmerParser's window loop (kmer_parser.hpp:85-294) of the reference, in the formulation of
// kmi_extract.hip: a line is a maximal run of non-EOL bytes and line index % 4 is its role. Those four kernels spent 3.1 of the
// build's 9 ms issuing instructions on bytes that never become k-mers: every byte was classified into a 2-bit code although 52 %
// of a record are header, '+' and quality, and the line bookkeeping went through three passes over bitmaps.
//
// Here every WAVEFRONT works a byte range at a time, on its own (no workgroup barrier in the kernel; a large input has four ranges
// per resident wavefront, and a wavefront takes its next one from a queue word):
//   produce   64 lanes x 64 bytes: EOL bits only (SWAR), line starts / ends ranked with one DPP scan, their positions into a
//             ring in LDS (line ends alone for an LF text); when 64 complete records wait, one lane per record checks its
//             markers and lengths (a line's role is its index mod 4) and turns its sequence line into runs of windows
//   consume   as soon as 64 runs wait: one lane per run loads the read's own bytes, packs THEM (and nothing else) into 2-bit
//             complement codes -- the run's row, kept for the scatter pass -- and walks the minimizers exactly as
//             sk_minimizer did (rolling canonical m-mer, order hash, sliding minimum over W positions)
// The line index of a range's first line is INFERRED (first line that starts with '@' whose second successor starts with '+':
// the reference's own find_first_record idea, fastq_loader.hpp:269-364) and the ranges are chained afterwards (front_verify):
// the index of range r + 1 must be that of range r plus its lines. Anything the fast path is not sure about -- a marker that
// is not where the role says, sequence and quality lines of different length, an inference without exactly one candidate, a
// chain that does not close, a capacity exceeded -- raises ONE flag and the caller runs the general path (fastq_scan + list +
// minimizer), which also words the error. So this path is exact on well-formed input and silent on everything else.
#pragma once
#include "kmi_front_bytes.h"   // eol_flags, pack_codes4: the dword functions, also run on the host (tests/cpu)

namespace kmi {

constexpr int kFrWaves = 4, kFrThreads = kFrWaves * kWave;
constexpr uint32_t kFrRing = 512;        // line-event words a wavefront keeps (power of two): 512 line ends of an LF file, whose line
                                         // starts follow from them, or 256 (start, end) pairs of any other text
constexpr uint32_t kFrStepLines = 128;   // lines a produce step may add
constexpr uint32_t kFrPendEnds = kFrRing - kFrStepLines - 2u, kFrPendPairs = kFrRing / 2u - kFrStepLines;   // waiting lines that leave a step room
// (A/B knobs, profiles/r12: -DKMI_FR_PASS_RECORDS=1 runs the line pass after every step, -DKMI_FR_PAIRS_ONLY keeps pairs for every text)
#ifndef KMI_FR_PASS_RECORDS
#define KMI_FR_PASS_RECORDS 64
#endif
constexpr uint32_t kFrPassRecords = KMI_FR_PASS_RECORDS;   // complete records that wait before a line pass runs (1 .. 64)
#ifdef KMI_FR_PAIRS_ONLY
constexpr bool kFrEndsOnly = false;
#else
constexpr bool kFrEndsOnly = true;
#endif
constexpr uint32_t kFrRunQ = 256;       // waiting runs (power of two): 64 are taken at a time, a line pass adds what fits
constexpr uint32_t kFrStep = 4096;       // bytes per produce step: 64 lanes x 64
constexpr uint32_t kFrRowDw = 12;        // a run's packed row: 192 bases (a run holds at most 128 + 31)
constexpr uint32_t kFrNone = 0xffu;      // FrRange::l0 of a range that owns no line
constexpr uint32_t kFrOverrun = 256u << 10;   // bytes a range may scan behind its own end before it hands the input over

struct FrRange { uint32_t l0, n_lines, n_runs, n_items; };
struct __attribute__((packed, aligned(1))) FrU4 { uint32_t x, y, z, w; };   // sixteen bytes at any address

// bytes per lane of a run, in dwords: seg + kmax - 1 bases
template <int W> struct FrCfg {
  static constexpr int SEG = W >= 19 ? 127 : (W >= 13 ? 80 : (W >= 11 ? 64 : 44));   // (< 128: window number 127 marks "behind the run" in the walk's entries)
  static constexpr int KMAX = W >= 19 ? 32 : (W >= 13 ? 28 : (W >= 11 ? 22 : 20));
  static constexpr int ND = (SEG + KMAX - 1 + 3) / 4;   // 40, 27, 22, 16
  static constexpr int NR = (ND + 3) / 4;               // packed words that can hold a base: 10, 7, 6, 4
};

// four bases -> four complement codes in the low byte; anything but A C G T (either case) counts as A, like DNA::FROM_ASCII
__device__ __forceinline__ uint32_t pack_dna4(uint32_t w, uint32_t *ok_out = nullptr) {
  const uint32_t x = w & 0xDFDFDFDFu;                          // fold case
  const uint32_t idx = (x >> 1) & 0x03030303u;                 // A 0, C 1, T 2, G 3
  const uint32_t expect = byte_perm(0u, 0x47544341u, idx);     // 'A','C','T','G'
  const uint32_t ok = zero_bytes(x ^ expect);                  // 0x80 per base byte
  if (ok_out) *ok_out = ok;
  const uint32_t lut = byte_perm(0u, 0x01000203u, idx);        // complement codes: A 3, C 2, T 0, G 1
  const uint32_t v1 = ok >> 7, vm = v1 | (v1 << 1);
  const uint32_t cc = (lut & vm) | (0x03030303u & ~vm);
  const uint32_t p1 = cc | (cc >> 6);
  return (p1 | (p1 >> 12)) & 0xFFu;
}

// 0x80 in every byte of w that is one of A C G T (either case)
__device__ __forceinline__ uint32_t dna4_ok(uint32_t w) {
  const uint32_t x = w & 0xDFDFDFDFu;
  const uint32_t idx = (x >> 1) & 0x03030303u;
  return zero_bytes(x ^ byte_perm(0u, 0x47544341u, idx));
}

#if defined(KMI_FR_TIMING) && !defined(KMI_FR_LEAVE)
#define KMI_FR_LEAVE
#endif
#ifdef KMI_FR_LEAVE
// (-DKMI_FR_LEAVE builds; the phase clocks of -DKMI_FR_TIMING cost registers, this does not) when every wavefront of the last launch
// entered and left the kernel: two wall-clock words per wavefront
constexpr uint32_t kFrTimingWaves = 16384;
__device__ unsigned long long g_fr_wave_clock[2 * kFrTimingWaves];
#endif

template <int W, bool EDGES = false>
__global__ __launch_bounds__(kFrThreads) void sk_front_kernel(const uint8_t *__restrict__ bytes, uint64_t n_bytes, uint64_t range_bytes, uint32_t n_ranges,
                                                             uint32_t k, bool rna, uint32_t run_cap, uint32_t item_cap, uint32_t ranges_per_group,
                                                             FrRange *__restrict__ info, uint32_t *__restrict__ run_items, uint32_t *__restrict__ rows,
                                                             uint32_t *__restrict__ items, uint32_t *__restrict__ wg_hist,
                                                             unsigned long long *__restrict__ n_windows, uint32_t *__restrict__ flags,
                                                             uint32_t r_first = 0u, uint32_t r_end = 0xffffffffu, uint32_t *__restrict__ queue = nullptr) {
  constexpr bool edges = EDGES;   // (a kernel of its own: the checks it adds cost the build that does not need them a quarter of this kernel's time)
  // EDGES (the de Bruijn node build, kmi_debruijn.h): a record also carries the base before its first and the base behind its last
  // k-mer (two 3-bit codes in the place of its last three bases: super-k-mers are cut three windows earlier), which the scatter pass
  // takes from the run's row (the bases around the run itself ride in the row's last word) -- and every base has to be one of A C G T
  // (an N is an A inside a k-mer but its own DNA16 code as a neighbour, edge_iterator.hpp:163-177: the general build decides then)
  // r_first / r_end: this launch takes the ranges [r_first, min(r_end, n_ranges)) -- a build from host memory launches the kernel
  // once per arrived chunk of the input, for the ranges whose bytes (and the bytes a range may scan behind its end) are there
  // queue (zero at launch, one launch per zeroing): there are more ranges than wavefronts, and a wavefront that has worked its own
  // range (the one with its number) takes its next one from this counter -- the oldest wavefront of a SIMD is issued first and gets
  // through its bytes well before the youngest, and with equal static shares the SIMD then runs on two wavefronts, then on one.
  // The counter only hands out numbers: no wavefront waits for another. Without a queue (the launches of a host-fed build share
  // the flags) a wavefront takes every n_waves-th range.
  if (r_end > n_ranges) r_end = n_ranges;
  using F = FrCfg<W>;
  constexpr int CAP = kSkListCap;
  constexpr uint32_t INF = 0xffffffffu, RM = kFrRing - 1u, QM = kFrRunQ - 1u;
  __shared__ uint32_t s_ring[kFrWaves][kFrRing], s_rq[kFrWaves][kFrRunQ];
  __shared__ uint32_t s_list[kFrWaves][(CAP + 2) * kWave];   // [slot][lane]; slot 0 takes the opening dummy, slot CAP + 1 what does not fit
  __shared__ uint32_t s_hist[kFrWaves][kNumCoarse];
  // (the wavefront's number as a scalar: from threadIdx.x alone the compiler takes it, the range's number and everything that follows
  // from them -- positions, counts, every `bail` -- for values that differ between lanes, keeps them in vector registers and masks lanes
  // where it could branch)
  const uint32_t lane = lane_id(), wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_id());
  uint32_t *const Rg = s_ring[wv], *const rq = s_rq[wv], *const list = s_list[wv], *const hist = s_hist[wv];
  auto wave_sync = [&]() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); };
  const uint32_t m = k - (uint32_t)W + 1u;
  const uint32_t mmask = (m >= 16u) ? 0xffffffffu : ((1u << (2u * m)) - 1u);
  const uint32_t topsh = 2u * m - 2u;
  const uint32_t nmax = sk_nmax_of(k) - (edges ? kSkEdgeWindows : 0u);
  const uint32_t seg = (uint32_t)F::SEG;
  const uint32_t n_waves = gridDim.x * (uint32_t)kFrWaves;
#ifdef KMI_FR_LEAVE
  const unsigned long long t_enter = wall_clock64();
#endif
#ifdef KMI_FR_TIMING
  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tq = clock64();
#define FQ_MARK(i) { const unsigned long long now_ = clock64(); acc[i] += now_ - tq; tq = now_; }
#else
#define FQ_MARK(i)
#endif
  for (uint32_t r = r_first + blockIdx.x * (uint32_t)kFrWaves + wv; r < r_end;) {   // (uniform per wavefront)
    const uint64_t B = (uint64_t)r * range_bytes;
    const uint32_t len = (uint32_t)((n_bytes - B < range_bytes) ? (n_bytes - B) : range_bytes);
    // the range after this one: asked for now, one range ahead (lane 0's atomic; its answer comes in with the byte before the range,
    // which is waited for anyway, and stays in a scalar register)
    uint32_t q_next = 0;
    if (queue && lane == 0) q_next = atomicAdd(queue, 1u);
    const uint32_t carry0 = (B == 0) ? 1u : (is_eol((uint32_t)__builtin_amdgcn_readfirstlane((int)bytes[B - 1])) ? 1u : 0u);
    const uint32_t r_next = queue ? r_first + n_waves + (uint32_t)__builtin_amdgcn_readfirstlane((int)q_next) : r + n_waves;
    const uint32_t eoff = carry0 ? 0u : 1u;          // the range starts inside a line: that line's end is not ours
    // The line events of a range are kept in one of two forms. `simple`: every EOL byte seen so far stood alone (the ordinary LF
    // file), so a line starts one byte behind its predecessor's end and only the ENDS are written: word e of the ring is end number
    // e of the range. Otherwise (CRLF, blank lines): (start, end) pairs, line j at words 2 j and 2 j + 1. A range begins as simple,
    // and the first step that meets an EOL byte behind another one begins the range again in the other form: nothing a range
    // writes outside its own tables is written before it ends, and a second pass over the same bytes writes the same tables.
    bool simple = kFrEndsOnly;
    for (;;) {
    bool redo = false;
    for (uint32_t i = lane; i < (uint32_t)kNumCoarse; i += kWave) hist[i] = 0;
    uint32_t why = 0; bool bail = false;                               // this range gives up: the caller takes the general path
    uint32_t carry = carry0;                                           // EOL status of the byte before the next step
    uint32_t n_starts = 0, n_ends = 0, n_owned = 0, done = 0, complete = 0, l0 = (r == 0) ? 0u : INF;
    bool fin = false;                                // the range's last line is in the ring: no further step
    if (r == 0 && __builtin_amdgcn_readfirstlane((int)bytes[0]) != (int)'@') { why |= 2u; bail = true; }      // (get_next_record refuses a partition that does not begin with '@')
    uint32_t rq_head = 0, rq_tail = 0, run_count = 0, item_count = 0;
    unsigned long long windows = 0;                  // (lane 0's copy counts)
    uint32_t p = 0;                                  // next step's position inside the range
    bool producing = true;
    // the step's 32 bytes per lane are loaded one step ahead (a step costs a few hundred instructions: without the prefetch
    // every one of them began with a trip to HBM that nothing else in this wavefront could hide)
    FrU4 n0, n1, n2, n3;
    n0.x = n0.y = n0.z = n0.w = 0; n1 = n0; n2 = n0; n3 = n0;
    if (B + 64ull * lane + 64 <= n_bytes) {
      const uint8_t *q = bytes + B + 64ull * lane;
      n0 = *reinterpret_cast<const FrU4 *>(q); n1 = *reinterpret_cast<const FrU4 *>(q + 16);
      n2 = *reinterpret_cast<const FrU4 *>(q + 32); n3 = *reinterpret_cast<const FrU4 *>(q + 48);
    }
    uint32_t mk_hd = (uint32_t)'@', mk_plus = (uint32_t)'+';   // the first bytes of the '@' and the '+' line of the last pass's record
    // where line j of the range starts (j below the lines the ring holds: any value)
    auto line_start = [&](uint32_t j) -> uint32_t { return simple ? (j + eoff ? Rg[(j + eoff - 1u) & RM] + 1u : 0u) : Rg[(2u * j) & RM]; };
    // EOL bits of 32 bytes: the flags (0x80 per EOL byte) of two dwords gathered into one byte by two dot products with bit
    // weights (the product sits 7 bits too high)
    auto eol32 = [](const FrU4 &a, const FrU4 &b) -> uint32_t {
      uint32_t d0 = __builtin_amdgcn_udot4(eol_flags(a.x), 0x08040201u, 0u, false);
      d0 = __builtin_amdgcn_udot4(eol_flags(a.y), 0x80402010u, d0, false);
      uint32_t d1 = __builtin_amdgcn_udot4(eol_flags(a.z), 0x08040201u, 0u, false);
      d1 = __builtin_amdgcn_udot4(eol_flags(a.w), 0x80402010u, d1, false);
      uint32_t d2 = __builtin_amdgcn_udot4(eol_flags(b.x), 0x08040201u, 0u, false);
      d2 = __builtin_amdgcn_udot4(eol_flags(b.y), 0x80402010u, d2, false);
      uint32_t d3 = __builtin_amdgcn_udot4(eol_flags(b.z), 0x08040201u, 0u, false);
      d3 = __builtin_amdgcn_udot4(eol_flags(b.w), 0x80402010u, d3, false);
      return (d0 >> 7) | (d1 << 1) | (d2 << 9) | (d3 << 17);
    };
    while (!bail) {
      // ---------------------------------------------------------------- produce
      // A STEP puts the line events of the next 4 KB into the ring; a LINE PASS takes up to 64 waiting records, one per lane, checks
      // them and queues their runs. The pass runs when 64 complete records wait or the range's last line is in the ring (and
      // whenever the ring has no room for another step's lines, which only pairs come to) -- about once in five steps, with every
      // lane at work, where a pass per step filled 52 lanes of which three in four held a line that makes no run.
      while (producing && rq_tail - rq_head < (uint32_t)kWave && !bail) {
       if (!fin && !(l0 != INF && ((complete - done + ((l0 + done) & 3u)) >> 2) >= kFrPassRecords) &&
           n_starts - done <= (simple ? kFrPendEnds : kFrPendPairs)) {
        const uint64_t g = B + p + 64ull * lane;
        uint32_t eol_lo = 0, eol_hi = 0, in_lo = 0xffffffffu, in_hi = 0xffffffffu;   // in_: the bytes that lie inside the buffer
        const FrU4 v0 = n0, v1 = n1, v2 = n2, v3 = n3;
        {
          const uint64_t gn = g + kFrStep;
          if (gn + 64 <= n_bytes) {
            const uint8_t *q = bytes + gn;
            n0 = *reinterpret_cast<const FrU4 *>(q); n1 = *reinterpret_cast<const FrU4 *>(q + 16);
            n2 = *reinterpret_cast<const FrU4 *>(q + 32); n3 = *reinterpret_cast<const FrU4 *>(q + 48);
          }
        }
        FQ_MARK(0)
        if (g + 64 <= n_bytes) {
          eol_lo = eol32(v0, v1); eol_hi = eol32(v2, v3);
        } else {
          in_lo = in_hi = 0;
#pragma unroll 1
          for (uint32_t i = 0; i < 64u; ++i) {
            const bool in = g + i < n_bytes;
            const bool e = !in || is_eol(bytes[g + i]);   // bytes past the end count as EOL
            if (i < 32u) { eol_lo |= (e ? 1u : 0u) << i; in_lo |= (in ? 1u : 0u) << i; }
            else { eol_hi |= (e ? 1u : 0u) << (i - 32u); in_hi |= (in ? 1u : 0u) << (i - 32u); }
          }
        }
        FQ_MARK(1)
        const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp((int)carry, (int)(eol_hi >> 31), 0x138 /* wave_shr:1 */, 0xf, 0xf, false);   // lane 0 keeps the carry
        const uint32_t before_lo = (eol_lo << 1) | prev, before_hi = (eol_hi << 1) | (eol_lo >> 31);
        // an EOL byte of the buffer behind another EOL byte (the bytes past the buffer's end are not the text's): pairs from here on
        if (simple && __any(((eol_lo & before_lo & in_lo) | (eol_hi & before_hi & in_hi)) != 0u)) { redo = true; bail = true; break; }
        const uint32_t ls_lo = ~eol_lo & before_lo, ls_hi = ~eol_hi & before_hi, le_lo = eol_lo & ~before_lo, le_hi = eol_hi & ~before_hi;
        const uint32_t base = p + 64u * lane;
        const uint32_t ns = (uint32_t)__builtin_popcount(ls_lo) + (uint32_t)__builtin_popcount(ls_hi);
        const uint32_t ne = (uint32_t)__builtin_popcount(le_lo) + (uint32_t)__builtin_popcount(le_hi);
        if (__any(ns > 8u || ne > 8u)) { why |= 4u; bail = true; break; }   // lines of a few bytes: not this path's input (and the packed sums below stay inside their fields)
        // owned line starts: positions below the range's length (whole lanes: a range's length is a multiple of 64 except where the
        // buffer ends, and no line starts behind its end)
        const uint32_t no = base < len ? ns : 0u;
        const uint32_t packed = ns | (ne << 10) | (no << 20);
        const uint32_t inc = wave_inclusive_sum_dpp(packed);
        const uint32_t tot = __builtin_amdgcn_readlane(inc, kWave - 1);
        const uint32_t NS = tot & 1023u, NE = (tot >> 10) & 1023u, NO = tot >> 20;
        if (NS > kFrStepLines || NE > kFrStepLines) { why |= 4u; bail = true; break; }
        // the events go to the ring: one loop over a lane's 64 bits, left when no lane has an event left (a vote per trip; two trips
        // for most steps of a text of reads), starts and ends in the same trip
        uint32_t rs = n_starts + ((inc - packed) & 1023u), re = n_ends + (((inc - packed) >> 10) & 1023u);
        unsigned long long le = ((unsigned long long)le_hi << 32) | le_lo;
        if (simple) {
          while (__any(le != 0ull)) {
            if (le) { Rg[re & RM] = base + (uint32_t)__builtin_ctzll(le); ++re; le &= le - 1ull; }
          }
        } else {
          unsigned long long ls = ((unsigned long long)ls_hi << 32) | ls_lo;
          while (__any((ls | le) != 0ull)) {
            if (ls) { Rg[(2u * rs) & RM] = base + (uint32_t)__builtin_ctzll(ls); ++rs; ls &= ls - 1ull; }
            if (le) {
              if (re >= eoff) Rg[(2u * (re - eoff) + 1u) & RM] = base + (uint32_t)__builtin_ctzll(le);   // (end 0 of a range that starts inside a line is not its line's)
              ++re; le &= le - 1ull;
            }
          }
        }
        n_starts += NS; n_ends += NE; n_owned += NO;
        carry = (uint32_t)__builtin_amdgcn_readlane(eol_hi, kWave - 1) >> 31;   // (the builtin returns a signed int)
        p += kFrStep;
        // a range is done two complete lines behind its last byte; a range that lies inside a line of megabytes (long-read FASTQ)
        // would scan on to that line's end, and so would every other range inside the same line: work without a bound. Past
        // kFrOverrun bytes behind its end the range gives up and the general path takes the input.
        if (p > len + kFrOverrun) { why |= 32u; bail = true; break; }
        const bool at_eof = B + p > n_bytes;                 // (a step that reached past the end has produced the last line's end)
        wave_sync();                                         // the events are in the ring
        // ---- the line index of the first line (once)
        if (l0 == INF && n_starts > 0u) {
          if ((uint32_t)__builtin_amdgcn_readfirstlane((int)line_start(0u)) >= len) l0 = kFrNone;            // the range owns no line: nothing to do here
          else if (at_eof && n_starts < 6u) {
            // the buffer ends here: a well-formed file ends with a quality line, so the lines of this range end on index 3 (mod 4);
            // like every inferred index this one is confirmed by the chain over the ranges
            l0 = (0u - n_starts) & 3u;
          } else if (n_starts >= 6u) {
            const uint32_t nl = 6u;
            uint32_t c = 0;
            if (lane < nl) c = bytes[B + line_start(lane)];
            const uint32_t c2 = __shfl_down(c, 2, kWave);
            const bool cand = lane < 4u && lane + 2u < nl && c == (uint32_t)'@' && c2 == (uint32_t)'+';
            const unsigned long long cm = __ballot(cand);
            if (__popcll(cm) != 1) { why |= 8u; bail = true; break; }   // none, or more than one: the general path decides
            l0 = (4u - (uint32_t)__builtin_ctzll(cm)) & 3u;
          }
        }
        if (l0 == kFrNone) { producing = false; break; }
        if (l0 == INF) {                                     // (fewer than six line starts so far)
          if (at_eof) producing = false;
          wave_sync();
          continue;
        }
        complete = n_ends >= eoff ? (n_starts < n_ends - eoff ? n_starts : n_ends - eoff) : 0u;   // lines whose end is known
        // the last step: the range is scanned and the two lines behind its last one are complete (their quality lines are checked here)
        fin = at_eof || (p >= len && complete >= n_owned + 2u);
       }
        // ---- the line pass: lane i takes the record whose '@' line is line jb + 4 i of the range -- markers, the length rule, runs.
        // A line belongs to the range where it starts: the first record of a range may lack its first lines (l0 of them belong to
        // the range before: the lines below `done` = 0), the records behind the range's end are looked at for the length rule alone,
        // and that rule looks two lines back only if that line is owned.
        const uint32_t jb = done - ((l0 + done) & 3u);       // (below zero, i.e. wrapped, for a first record that lacks lines)
        const uint32_t whole = (complete - jb) >> 2;         // complete records that wait
        if (!fin && whole < kFrPassRecords && n_starts - done <= (simple ? kFrPendEnds : kFrPendPairs)) { wave_sync(); continue; }
        if (fin && done == complete) { producing = false; break; }
        const uint32_t ahead = fin ? complete - jb : 4u * whole;                       // lines from jb on that may be worked ...
        const uint32_t lim = jb + (ahead < 4u * kWave ? ahead : 4u * kWave);          // ... in this pass: those below lim
        const uint32_t n_rec = (lim - jb + 3u) >> 2;
        if (n_rec == 0u) { why |= 32u; bail = true; break; }   // (not reached: without room for a step the ring holds 31 records and more)
        {
          const uint32_t jr = jb + 4u * lane;
          const bool in_pass = lane < n_rec;
          uint32_t s[4], e[4];
          bool v[4];
#pragma unroll
          for (uint32_t t = 0; t < 4u; ++t) v[t] = in_pass && (int32_t)(jr + t - done) >= 0 && (int32_t)(lim - (jr + t)) > 0;
          if (simple) {   // (uniform) five ends: a line starts behind the end before it; line 0 of a range that begins a line, at 0
            uint32_t x[5];
#pragma unroll
            for (uint32_t t = 0; t < 5u; ++t) x[t] = Rg[(jr + eoff - 1u + t) & RM];
#pragma unroll
            for (uint32_t t = 0; t < 4u; ++t) { s[t] = (jr + t + eoff) ? x[t] + 1u : 0u; e[t] = x[t + 1u]; }
          } else {
#pragma unroll
            for (uint32_t t = 0; t < 4u; ++t) { s[t] = Rg[(2u * (jr + t)) & RM]; e[t] = Rg[(2u * (jr + t) + 1u) & RM]; }
          }
          const bool own_hd = v[0] && s[0] < len, own_seq = v[1] && s[1] < len, own_plus = v[2] && s[2] < len;
          // the record's two marker bytes: two loads issued together, compared by the pass after this one (nothing waits for them)
          bool bad = mk_hd != (uint32_t)'@' || mk_plus != (uint32_t)'+';
          mk_hd = (uint32_t)'@'; mk_plus = (uint32_t)'+';
          if (own_hd) mk_hd = bytes[B + s[0]];
          if (own_plus) mk_plus = bytes[B + s[2]];
          const uint32_t L = e[1] - s[1];
          if (v[3] && own_seq) bad = bad || (e[3] - s[3] != L);   // (a quality line that is worked has its sequence line in the same pass)
          if (__any(bad)) { why |= 16u; bail = true; break; }
          uint32_t nr = 0, nwin = 0;
          if (own_seq && L >= k) { nwin = L - k + 1u; nr = (nwin + seg - 1u) / seg; }
          // the records whose runs the queue has room for (a prefix of the lanes: the sums only grow); the others wait for the next
          // pass, after a batch of runs has left the queue
          const uint32_t rinc = wave_inclusive_sum_dpp(nr);
          const uint32_t n_fit = (uint32_t)__popcll(__ballot(in_pass && rinc <= kFrRunQ - (rq_tail - rq_head)));
          // a record with more runs than the queue has room for beside 63 waiting ones (a long read), or a range past 16 MB
          if (n_fit == 0u || __any(nr && (s[1] >> 24))) { why |= 32u; bail = true; break; }
          if (lane < n_fit) {
            const uint32_t o = rq_tail + rinc - nr;
            for (uint32_t i = 0; i < nr; ++i) {
              const uint32_t left = nwin - i * seg;
              rq[(o + i) & QM] = (s[1] + i * seg) | (((left < seg ? left : seg) - 1u) << 24);
            }
          }
          rq_tail += (uint32_t)__builtin_amdgcn_readlane((int)rinc, (int)(n_fit - 1u));
          done = n_fit == n_rec ? lim : jb + 4u * n_fit;
        }
        if (fin && done == complete) producing = false;
        wave_sync();                                         // the queue is written; the ring may be overwritten by the next step
        FQ_MARK(2)
      }
      if (redo) break;
      if (bail) break;
      FQ_MARK(2)
      // ---------------------------------------------------------------- consume
      const uint32_t avail = rq_tail - rq_head;
      if (avail == 0u) { if (!producing) break; continue; }
      const uint32_t take = avail < (uint32_t)kWave ? avail : (uint32_t)kWave;
      const bool mine = lane < take;
      const uint32_t rv = mine ? rq[(rq_head + lane) & QM] : 0u;
      rq_head += take;
      if (run_count + take > run_cap) { why |= 64u; bail = true; break; }
      const uint32_t L = mine ? (rv >> 24) + 1u : 0u;        // windows of the run
      const uint64_t g0 = B + (rv & 0xffffffu);              // its first base
      {
        const uint32_t wsum = __builtin_amdgcn_readlane(wave_inclusive_sum_dpp(L), kWave - 1);
        windows += wsum;
      }
      // ---- the run's bytes -> its packed row (complement codes, base i at bits 2 i)
      uint32_t rw[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) rw[i] = 0;
      uint32_t other = 0;   // edges: 0x80 per byte of the run that is none of A C G T
      // today's exact routine: every byte gets its validity mask, and a byte that is none of A C G T the code of A
      auto pack_exact = [&]() {
#pragma unroll
        for (int q = 0; q < F::NR; ++q) {
          FrU4 v = *reinterpret_cast<const FrU4 *>(bytes + g0 + 16 * q);   // (a read starts at any byte: unaligned 16-byte loads)
          if (rna) { v.x = swap_tu_dword(v.x); v.y = swap_tu_dword(v.y); v.z = swap_tu_dword(v.z); v.w = swap_tu_dword(v.w); }
          uint32_t okd[4];
          rw[q] = pack_dna4(v.x, &okd[0]) | (pack_dna4(v.y, &okd[1]) << 8) | (pack_dna4(v.z, &okd[2]) << 16) | (pack_dna4(v.w, &okd[3]) << 24);
          if (edges) {   // uniform: every byte of the run's nb bases has to be one of A C G T
            const uint32_t nbits = 8u * (L + k - 1u);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const uint32_t at = 8u * (16u * (uint32_t)q + 4u * (uint32_t)e);   // first bit of this dword in the run
              const uint32_t vm = nbits >= at + 32u ? 0x80808080u : (nbits <= at ? 0u : (0x80808080u & ((1u << (nbits - at)) - 1u)));
              other |= ~okd[e] & vm;
            }
          }
        }
      };
      constexpr bool fast_pack = !edges;   // (the edge records need the per-byte mask anyway)
      const bool whole = mine && g0 + 16ull * F::NR <= n_bytes;   // the run's sixteen-byte loads stay inside the buffer
      if (fast_pack) {
        // A read is A C G T and nothing else, nearly always: the codes come from a table lookup and a dot product per dword
        // (pack_codes4), with no validity select. Whether that was right is found out on the side: the differences between the bytes
        // and the letters their codes stand for are OR-ed together over the sixteen-byte groups that lie wholly inside the run's
        // nb = L + k - 1 bases, and the one group that holds the run's last 1 .. 15 bases is looked at again under a byte mask (what
        // lies behind a run's end -- EOLs, '+', quality characters -- must not raise the flag; in the row those bytes leave codes that
        // nothing reads, as before). If any lane of the wavefront saw another byte, the wavefront packs this batch with the exact
        // routine: the rows are today's, bit for bit, wherever a byte is not a base.
        uint32_t bad = 0;
        if (whole) {
          const uint32_t nb = L + k - 1u;
#pragma unroll
          for (int q = 0; q < F::NR; ++q) {
            FrU4 v = *reinterpret_cast<const FrU4 *>(bytes + g0 + 16 * q);
            if (rna) { v.x = swap_tu_dword(v.x); v.y = swap_tu_dword(v.y); v.z = swap_tu_dword(v.z); v.w = swap_tu_dword(v.w); }
            uint32_t d = 0;
            const uint32_t c0 = pack_codes4(v.x, d), c1 = pack_codes4(v.y, d), c2 = pack_codes4(v.z, d), c3 = pack_codes4(v.w, d);
            rw[q] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
            bad |= (16u * (uint32_t)(q + 1) <= nb) ? d : 0u;
          }
          const uint32_t rem = nb & 15u, qt = nb >> 4;   // (rem != 0: qt < NR, sixteen NR bytes hold the longest run)
          if (rem) {
            FrU4 v = *reinterpret_cast<const FrU4 *>(bytes + g0 + 16u * qt);
            if (rna) { v.x = swap_tu_dword(v.x); v.y = swap_tu_dword(v.y); v.z = swap_tu_dword(v.z); v.w = swap_tu_dword(v.w); }
            bad |= dna4_other_in_first(v.x, rem) | dna4_other_in_first(v.y, rem > 4u ? rem - 4u : 0u) |
                   dna4_other_in_first(v.z, rem > 8u ? rem - 8u : 0u) | dna4_other_in_first(v.w, rem > 12u ? rem - 12u : 0u);
          }
          bad &= 0xDFDFDFDFu;
        }
        if (__any(bad != 0u)) { if (whole) pack_exact(); }
      } else if (whole) pack_exact();
      if (mine && !whole) {   // the last reads of the buffer: byte by byte, nothing read past the end
        const uint32_t nb = L + k - 1u;
#pragma unroll 1
        for (uint32_t i = 0; i < nb; ++i) {
          uint32_t c = bytes[g0 + i];
          if (rna) c = swap_tu_dword(c) & 0xffu;
          const uint32_t code = pack_dna4(c | 0x0A0A0A00u) & 3u;
          if (edges) other |= ~dna4_ok(c | 0x41414100u) & 0x80u;
          const uint32_t wi = i >> 4, sh = (i & 15u) * 2u;
#pragma unroll
          for (int q = 0; q < F::NR; ++q) rw[q] |= (wi == (uint32_t)q) ? (code << sh) : 0u;
        }
      }
      if (edges) {   // uniform
        // the bases around the run: the byte before its first base and the byte behind its last one are EOLs where the read begins and
        // ends, and bases where the read goes on in another run; as 1 + base code (0: none) into the last word of the row
        if (mine) {
          const uint32_t nb = L + k - 1u;
          uint32_t lb = bytes[g0 - 1u], rb = g0 + nb < n_bytes ? (uint32_t)bytes[g0 + nb] : (uint32_t)'\n';
          if (rna) { lb = swap_tu_dword(lb) & 0xffu; rb = swap_tu_dword(rb) & 0xffu; }
          const uint32_t lc = is_eol(lb) ? 0u : 4u - (pack_dna4(lb | 0x0A0A0A00u) & 3u), rc = is_eol(rb) ? 0u : 4u - (pack_dna4(rb | 0x0A0A0A00u) & 3u);
          if (!is_eol(lb)) other |= ~dna4_ok(lb | 0x41414100u) & 0x80u;
          if (!is_eol(rb)) other |= ~dna4_ok(rb | 0x41414100u) & 0x80u;
          rw[kFrRowDw - 1] = lc | (rc << 3);
        }
        if (__any(other != 0u)) { why |= 1024u; bail = true; break; }
      }
      FQ_MARK(3)
      // the row leaves now (the walk below consumes its registers): three stores per lane, consecutive rows. Words 10 and 11 hold no
      // base; only the edge records use word 11 (the scatter pass reads nothing of them otherwise), and two registers kept at zero
      // through the whole kernel for them were two registers too many.
      if (mine) {
        const uint64_t ri = (uint64_t)r * run_cap + run_count + lane;
        uint4 *rp = reinterpret_cast<uint4 *>(rows + ri * kFrRowDw);
        rp[0] = make_uint4(rw[0], rw[1], rw[2], rw[3]);
        rp[1] = make_uint4(rw[4], rw[5], rw[6], rw[7]);
        if (edges) rp[2] = make_uint4(rw[8], rw[9], rw[10], rw[11]);
        else *reinterpret_cast<uint2 *>(rp + 2) = make_uint2(rw[8], rw[9]);
      }
      // ---- the walk (sk_minimizer_kernel's). The row is kept ALIGNED to the block being walked: after the first m - 1 bases are
      // shifted out once, the W codes of a block are the low 2 W bits of rw[0..1], and the row moves down by W bases per block
      // (static funnel shifts) -- no indexing of the register array by a run-time value, which the compiler answers with scratch.
      // An entry is written when a super-k-mer OPENS: (low 25 bits of the minimizer's order hash) << 7 | its first window. The walk
      // has no branch: EVERY position stores its (minimizer, window) into the slot behind the last entry, and the slot pointer
      // steps on when the minimizer differs from the one before -- a store that is not followed by a step is overwritten by the
      // next one. Lengths come from the next entry's window afterwards. Positions behind a lane's last window (short reads, the
      // last block) go on writing entries; their window numbers are >= L and the pass below skips them.
      uint32_t cnt = 0;
      {
        const uint32_t nblk = mine ? (L + (uint32_t)W - 2u) / (uint32_t)W + 1u : 0u;   // m-mer positions 0 .. L + W - 2
        uint32_t R = rw[0] & mmask, Fw = sk_fwd_of(rw[0] & mmask, m);
        {
          const uint32_t sh0 = 2u * (m - 1u);   // 4 .. 30 (m <= 16)
#pragma unroll
          for (int i = 0; i < F::NR; ++i) rw[i] = __builtin_amdgcn_alignbit(rw[i + 1], rw[i], sh0);
        }
        uint32_t sprev[W + 1];
#pragma unroll
        for (int j = 0; j <= W; ++j) sprev[j] = INF;
        // (LDS byte addresses: this lane's slot 0; the last slot a pointer may rest on is CAP: what is stored behind it lands in CAP + 1)
        const uint32_t a_first = (uint32_t)(uintptr_t)((lds_u32_t *)list + lane), a_stop = a_first + (uint32_t)CAP * 4u * kWave;
        uint32_t addr = a_first;   // the slot the next entry goes to
        uint32_t prevv = 0;
        const uint32_t nblk_max = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_max_dpp(nblk), kWave - 1);
        auto block = [&](auto first_block, uint32_t wbase /* window that ends at position 0 of the block (b W - (W - 1)) */) {
          constexpr bool FIRST = decltype(first_block)::value;
          const uint32_t clo = rw[0], chi = rw[1];
          {
            constexpr int WS = (2 * W) / 32, BS = (2 * W) % 32;
#pragma unroll
            for (int i = 0; i < F::NR; ++i) rw[i] = __builtin_amdgcn_alignbit(rw[i + WS + 1], rw[i + WS], BS);
          }
          uint32_t hh[W];
          uint32_t pm = INF;
#pragma unroll
          for (int j = 0; j < W; ++j) {
            if (j > 0 || !FIRST) {
              const uint32_t c = (j < 16) ? ((clo >> (2 * (j & 15))) & 3u) : ((chi >> (2 * (j & 15))) & 3u);
              R = (R >> 2) | (c << topsh);
              Fw = ((Fw << 2) | (c ^ 3u)) & mmask;
            }
            const uint32_t h = sk_order_hash(R < Fw ? R : Fw);
            hh[j] = h;
            pm = pm < h ? pm : h;
            if (FIRST && j < W - 1) continue;                     // no window ends before position W - 1
            const uint32_t sp = sprev[j + 1];
            const uint32_t curv = sp < pm ? sp : pm;
            const uint32_t wi = wbase + (uint32_t)j < 127u ? wbase + (uint32_t)j : 127u;   // (the same in every lane)
            *(lds_u32_t *)(uintptr_t)addr = (curv << 7) | wi;
            const uint32_t step = (FIRST || curv != prevv) ? 4u * kWave : 0u;   // (window 0 opens whatever the value)
            addr = addr + step < a_stop ? addr + step : a_stop;
            prevv = curv;
          }
          sprev[W] = INF;
          sprev[W - 1] = hh[W - 1];
#pragma unroll
          for (int j = W - 2; j >= 0; --j) sprev[j] = hh[j] < sprev[j + 1] ? hh[j] : sprev[j + 1];
        };
        if (nblk_max) block(std::true_type{}, 0u - (uint32_t)(W - 1));
        for (uint32_t b = 1; b < nblk_max; ++b) block(std::false_type{}, b * (uint32_t)W - (uint32_t)(W - 1));
        cnt = (addr - a_first) / (4u * kWave);   // entries 0 .. cnt - 1 (those behind the last window included); CAP: maybe more than fit
      }
      FQ_MARK(4)
      if (__any(cnt >= (uint32_t)CAP)) { why |= 128u; bail = true; break; }
      // behind the last entry: one that lies behind every run (window 127), so an entry's successor is read without asking whether
      // there is one (cnt < CAP: the value is 127; made from cnt, it is not a constant that occupies a register through the walk)
      list[cnt * kWave + lane] = cnt | 127u;
      wave_sync();
      // items in their final form ((n - 1) | 27 hash bits << 5: the 18 bucket bits and nine more below them; the items of a run cover
      // its windows without a gap, so an item's first window is the sum of the lengths before it) + the coarse counts.
      // FORWARD, in place, as long as no lane of the wavefront holds a super-k-mer longer than nmax windows: the entries of a lane that
      // lie inside its run are a prefix of its list (windows ascend), entry j's length is the next entry's window (or L) minus its
      // own, and item j goes where entry j was -- straight-line code, one entry per turn, the next two read ahead. The wavefront
      // leaves this loop at the first turn j* in which some lane would need more than one item; items 0 .. j* - 1 are final then
      // (and counted), and the loop below works the entries from j* on.
      const uint32_t cmax = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_max_dpp(cnt), kWave - 1);
      uint32_t jstar = cmax, head = 0;   // head: this lane's items in slots 0 .. head - 1
      {
        // entry J (in CUR) and the one behind it (in NX); leaves the loop when a lane needs more than one item, or when no lane has an
        // entry left. (A macro with its own `break`s: as a lambda that answers "go on" the two uniform exits came out as exec-mask
        // control flow, and a constant marker value or two copy-out loops below cost the kernel two to three registers in the walk.)
#define KMI_FR_TURN(J, CUR, NX)                                                                   \
        {                                                                                         \
          const uint32_t w0 = (CUR) & 127u, wn = (NX) & 127u;                                     \
          const bool valid = (J) < cnt && w0 < L;                                                 \
          const uint32_t n = (wn < L ? wn : L) - w0; /* (the entry behind a lane's last one has window 127) */ \
          if (__any(valid && n > nmax)) { jstar = (J); break; }                                   \
          if (!__any(valid)) break;                                                               \
          if (valid) {                                                                            \
            const uint32_t h27 = sk_bucket_bits27((CUR) >> 7);                                    \
            atomicAdd(&hist[h27 >> 19], 1u);                                                      \
            list[(J) * kWave + lane] = (n - 1u) | (h27 << 5);                                     \
            ++head;                                                                               \
          }                                                                                       \
        }
        // two turns per trip: the two entries behind them are read first (one LDS instruction) and are not needed before the trip's end
        uint32_t e0 = list[lane], e1 = list[kWave + lane];
        for (uint32_t j = 0; j < cmax; j += 2u) {
          const uint32_t e2 = list[(j + 2u) * kWave + lane], e3 = list[(j + 3u) * kWave + lane];   // (slots up to cmax + 2 <= CAP + 1)
          KMI_FR_TURN(j, e0, e1)
          KMI_FR_TURN(j + 1u, e1, e2)
          e0 = e2; e1 = e3;
        }
#undef KMI_FR_TURN
      }
      // The rest (low complexity: one minimizer repeated), entries jstar .. cmax - 1: backwards, written from the top of the list
      // down -- a super-k-mer longer than nmax windows becomes several items, and what is written must not reach what has not been
      // read yet.
      uint32_t top = (uint32_t)CAP + 2u;   // these items end up in slots top .. CAP + 1
      if (jstar < cmax) {
        uint32_t nxt_w = L;
        uint32_t it_nx = list[(cmax - 1u) * kWave + lane];   // (read one turn ahead; a turn writes above the entry it works on)
        for (uint32_t jj = cmax; jj-- > jstar;) {
          const uint32_t it = it_nx;
          if (jj > jstar) it_nx = list[(jj - 1u) * kWave + lane];
          const uint32_t w0 = it & 127u;
          if (jj < cnt && w0 < L) {
            const uint32_t h27 = sk_bucket_bits27(it >> 7);
            uint32_t left = nxt_w - w0;                 // windows of this super-k-mer (>= 1)
            nxt_w = w0;
            while (left) {                               // (one turn unless the super-k-mer is longer than nmax)
              uint32_t n = left;                         // the last piece first: what nmax-window pieces leave over
              while (n > nmax) n -= nmax;
              left -= n;
              if (top <= jj || top <= 2u) { top = 0xffffffffu; left = 0; break; }   // no room (CAP items at most, none over an entry still to be read): checked below
              --top;
              atomicAdd(&hist[h27 >> 19], 1u);
              list[top * kWave + lane] = (n - 1u) | (h27 << 5);
            }
            if (top == 0xffffffffu) break;
          }
        }
      }
      const uint32_t tail = (uint32_t)CAP + 2u - top;   // (no room: top = 0xffffffff makes it CAP + 3)
      if (__any(head + tail > (uint32_t)CAP)) { why |= 128u; bail = true; break; }   // more than CAP items in a run
      cnt = head + tail;
      FQ_MARK(5)
      const uint32_t cinc = wave_inclusive_sum_dpp(cnt);
      const uint32_t ctot = __builtin_amdgcn_readlane(cinc, kWave - 1);
      if (item_count + ctot > item_cap) { why |= 256u; bail = true; break; }
      if (mine) {
        const uint32_t ex = item_count + cinc - cnt;
        uint32_t *dst = items + (uint64_t)r * item_cap + ex;
        if (jstar == cmax) for (uint32_t j = 0; j < cnt; ++j) dst[j] = list[j * kWave + lane];   // (uniform)
        else for (uint32_t j = 0; j < cnt; ++j) dst[j] = list[(j < head ? j : top + j - head) * kWave + lane];   // the two segments, in window order
        const uint64_t ri = (uint64_t)r * run_cap + run_count + lane;
        run_items[ri] = ex | (cnt << 26);
      }
      run_count += take;
      item_count += ctot;
      wave_sync();   // the list is read; the next batch overwrites it
      FQ_MARK(6)
    }
    if (redo) { simple = false; wave_sync(); continue; }   // once more, with (start, end) pairs
    if (!bail && __any(mk_hd != (uint32_t)'@' || mk_plus != (uint32_t)'+')) { why |= 16u; bail = true; }   // the last pass's markers
    if (bail) { if (lane == 0) { atomicOr(&flags[FLAG_SK_DECLINED], 4u); atomicOr(&flags[FLAG_SK_WHY], why); } }
    wave_sync();
    if (lane == 0) {
      FrRange fr; fr.l0 = (l0 == INF) ? kFrNone : l0; fr.n_lines = (l0 == INF || l0 == kFrNone) ? 0u : n_owned; fr.n_runs = run_count; fr.n_items = item_count;
      info[r] = fr;
      if (windows) atomicAdd(n_windows, windows);
    }
    const uint32_t grp = r / ranges_per_group;
    for (uint32_t i = lane; i < (uint32_t)kNumCoarse; i += kWave) {
      const uint32_t c = hist[i];
      if (c) atomicAdd(&wg_hist[(uint64_t)grp * kNumCoarse + i], c);
    }
    wave_sync();
    FQ_MARK(7)
    break;
    }
    r = r_next;
  }
#ifdef KMI_FR_TIMING
  if (lane == 0) for (int i = 0; i < 8; ++i) atomicAdd(&reinterpret_cast<unsigned long long *>(flags + FLAG_CLOCKS)[i], acc[i]);
#endif
#ifdef KMI_FR_LEAVE
  if (lane == 0 && blockIdx.x * (uint32_t)kFrWaves + wv < kFrTimingWaves) {
    g_fr_wave_clock[2u * (blockIdx.x * (uint32_t)kFrWaves + wv)] = t_enter;
    g_fr_wave_clock[2u * (blockIdx.x * (uint32_t)kFrWaves + wv) + 1u] = wall_clock64();
  }
#endif
}

// S for the fused front end: the scatter pass over the runs a group of ranges left (run_items / rows / items at fixed strides per
// range). The round structure, the LDS bucket sort and the copy-out are sk_scatter_kernel's; what differs is where a lane finds
// its run: run number G of the group lies in the range whose prefix of run counts covers it, its row is read as three aligned
// 16-byte loads and starts at the run's first base.
constexpr int kFrRowLds = 11;             // a run's ten packed words (127 + 31 bases) + one: odd stride, rows on different banks
constexpr uint32_t kFrMaxGroupRanges = 128;
constexpr int kFrScThreads = 512;         // runs per round of the scatter pass ...
constexpr int kFrScItems = 7168;          // ... as long as their items fit here (about 13 per run of 120 windows); a round takes fewer runs otherwise
template <bool CANON>
__global__ __launch_bounds__(kFrScThreads, 2) void sk_scatter_rows_kernel(const FrRange *__restrict__ info, uint32_t n_ranges, uint32_t rpg, uint32_t run_cap,
                                                                         uint32_t item_cap, uint32_t k, const uint32_t *__restrict__ run_items,
                                                                         const uint32_t *__restrict__ rows, const uint32_t *__restrict__ items,
                                                                         const uint64_t *__restrict__ wg_off, uint64_t *__restrict__ out, uint32_t lp,
                                                                         const uint32_t *__restrict__ flags, uint32_t edges = 0u) {
  // edges: the record's two outside bases (sk_front_kernel) go to bits 32..37 of word 1 as 1 + base code (A C G T = 0..3 in the
  // record's own orientation; 0: the read ends there), and bit 61 says that the record is the reverse complement of the read's
  // stretch (kRecFlipShift) -- see sk_edge_codes
  // One record format, whether the records go to this GPU's back end or through an exchange: word 1 keeps its 18 bucket bits as
  // the owner will read them, and bits 61..63 are zero -- bits 62 and 63 in an edge record (kmi_superkmer.h: no record's word 1 is
  // all ones).
  // (launched before the host has looked at the front end's verdict: a front end that gave up has left tables nobody may walk)
  if (__hip_atomic_load(&flags[FLAG_SK_DECLINED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  // One lane per run; the round's items are brought into LDS ONCE (sixteen bytes at a time from each run's list) and everything
  // after that -- bucket counts, the bucket sort of (run, item) references, the copy-out that assembles the records -- reads
  // them there. (Kept in registers and re-read from global memory for the copy-out, the items made this kernel wait on the
  // texture addresser: one dword from a different cache line per lane and record.)
  constexpr int NT = kFrScThreads, CAP = kSkListCap, ICAP = kFrScItems;
  static_assert(ICAP >= CAP, "a run's items must fit a round");
  __shared__ uint16_t s_stage[ICAP];
  __shared__ uint32_t s_items[ICAP + 4];    // first window | (n - 1) << 7 | the top 20 hash bits << 12
  __shared__ uint8_t s_xbits[ICAP];         // the low seven hash bits
  __shared__ uint32_t s_row[NT * kFrRowLds + 4];
  __shared__ uint32_t s_ibase[NT];      // first item of every run in s_items
  __shared__ uint8_t s_runw[NT];        // windows of every run (edges)
  __shared__ uint8_t s_runx[NT];        // the bases around every run: 1 + code of the one before | of the one behind << 3 (edges)
  __shared__ uint32_t s_cnt[kNumCoarse];
  __shared__ uint32_t s_cur[kNumCoarse];
  __shared__ uint64_t s_gbase[kNumCoarse];
  __shared__ uint32_t s_part[kNumCoarse / kWave];
  __shared__ uint32_t s_scan[NT / kWave + 2];
  __shared__ uint32_t s_pre[kFrMaxGroupRanges + 1];   // runs before every range of the group
  const bool bl = threadIdx.x < kNumCoarse;   // the lanes that keep a coarse bucket's counters
  uint64_t cursor = bl ? wg_off[(uint64_t)blockIdx.x * kNumCoarse + threadIdx.x] : 0ull;
  if (bl) s_cnt[threadIdx.x] = 0;
  const uint32_t r_first = blockIdx.x * rpg;
  const uint32_t nr = r_first >= n_ranges ? 0u : (n_ranges - r_first < rpg ? n_ranges - r_first : rpg);
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (uint32_t q = 0; q < nr; ++q) { s_pre[q] = acc; acc += info[r_first + q].n_runs; }
    s_pre[nr] = acc;
  }
  lds_barrier();
  const uint32_t total_runs = s_pre[nr];
  const uint32_t *const g_items = items + (uint64_t)r_first * item_cap;
  for (uint32_t rb = 0; rb < total_runs;) {
    // ---- this round's runs: as many of the next NT as their items fit
    const uint32_t G = rb + threadIdx.x;
    uint32_t ri = 0, q = 0;
    uint64_t run = 0;
    if (G < total_runs) {
      // the last range whose runs begin at or before G (the prefix only grows): a binary search, seven probes for up to
      // kFrMaxGroupRanges ranges -- a group holds a few dozen since the front end hands its ranges out from a queue
      static_assert(kFrMaxGroupRanges <= 128u, "seven probes");
#pragma unroll
      for (uint32_t step = 64u; step; step >>= 1) {
        const uint32_t t = q + step;
        if (t < nr && G >= s_pre[t]) q = t;
      }
      run = (uint64_t)(r_first + q) * run_cap + (G - s_pre[q]);
      ri = run_items[run];
    }
    uint32_t cnt = ri >> 26;
    uint32_t total;
    const uint32_t pre = block_exclusive_scan<uint32_t>(cnt, s_scan, &total);
    const bool taken = G < total_runs && pre + cnt <= (uint32_t)ICAP;   // (a prefix of the lanes: the sums only grow)
    const uint32_t n_taken = (uint32_t)__syncthreads_count(taken);     // >= 1: one run's items always fit
    if (!taken) cnt = 0;
    if (taken) {
      const uint4 *rp = reinterpret_cast<const uint4 *>(rows + run * kFrRowDw);
      const uint4 q0 = rp[0], q1 = rp[1], q2 = rp[2];
      uint32_t *row = s_row + threadIdx.x * kFrRowLds;
      row[0] = q0.x; row[1] = q0.y; row[2] = q0.z; row[3] = q0.w; row[4] = q1.x; row[5] = q1.y; row[6] = q1.z; row[7] = q1.w;
      row[8] = q2.x; row[9] = q2.y; row[10] = 0;   // (words 10 and 11 of the row in memory hold no base)
      if (edges) s_runx[threadIdx.x] = (uint8_t)q2.w;   // (... word 11 the two bases around the run, sk_front_kernel)
      // the items: sixteen bytes at a time (a list starts at any dword; what is read behind the run's items is not used). An item's
      // first window is the sum of the lengths before it.
      const uint32_t *src = g_items + (q * item_cap + (ri & 0x3ffffffu));
      uint32_t woff = 0;
#pragma unroll
      for (int v4 = 0; v4 < CAP / 4; ++v4) {
        if ((uint32_t)(4 * v4) < cnt) {
          const FrU4 v = *reinterpret_cast<const FrU4 *>(src + 4 * v4);
          const uint32_t it[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if ((uint32_t)(4 * v4 + e) < cnt) {
              const uint32_t n1 = it[e] & 31u, h27 = it[e] >> 5;
              s_items[pre + 4 * v4 + e] = woff | (n1 << 7) | ((h27 >> 7) << 12);
              s_xbits[pre + 4 * v4 + e] = (uint8_t)(h27 & 127u);
              atomicAdd(&s_cnt[h27 >> 19], 1u);
              woff += n1 + 1u;
            }
        }
      }
    }
    s_ibase[threadIdx.x] = pre;
    if (edges) {   // uniform: the run's windows = the sum of its items' lengths
      uint32_t wsum = 0;
      for (uint32_t j = 0; j < cnt; ++j) wsum += ((s_items[pre + j] >> 7) & 31u) + 1u;
      s_runw[threadIdx.x] = (uint8_t)wsum;
    }
    lds_barrier();
    // ---- bucket offsets of the round
    uint32_t c = 0, inc = 0;
    if (bl) {
      c = s_cnt[threadIdx.x];
      s_cnt[threadIdx.x] = 0;
      inc = wave_inclusive_sum_dpp(c);
      if (lane_id() == kWave - 1) s_part[wave_id()] = inc;
    }
    lds_barrier();
    if (bl) {
      uint32_t wpre = 0;
#pragma unroll
      for (uint32_t w = 0; w < kNumCoarse / kWave; ++w) wpre += (w < wave_id()) ? s_part[w] : 0u;
      const uint32_t lo = wpre + inc - c;
      s_cur[threadIdx.x] = lo;
      s_gbase[threadIdx.x] = cursor - lo;
      cursor += c;
    }
    lds_barrier();
    // ---- references (run << 5 | item) in bucket order
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t item = s_items[pre + j];
      s_stage[atomicAdd(&s_cur[item >> 24], 1u)] = (uint16_t)((threadIdx.x << 5) | j);
    }
    lds_barrier();
    // ---- copy-out: every lane assembles the record of one sorted position
    const uint32_t n_items = pre + cnt;   // (of the last taken lane: the round's total)
    const uint32_t round_items = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cur[kNumCoarse - 1]);   // the last bucket's end = all items of the round
    (void)n_items;
    for (uint32_t s = threadIdx.x; s < round_items; s += NT) {
      const uint32_t e = s_stage[s], rl = e >> 5, j = e & 31u;
      const uint32_t item = s_items[s_ibase[rl] + j];
      const uint32_t h27 = ((item >> 12) << 7) | (uint32_t)s_xbits[s_ibase[rl] + j], n1 = (item >> 7) & 31u;
      // the bucket bits as the owner will read them: the lp rank bits shifted out, further hash bits shifted in below
      const uint32_t hs = ((h27 << lp) & 0x7ffffffu) >> 9;
      uint64_t w0, w1;
      bool flipped = false;
      sk_assemble_row<CANON>(s_row + rl * kFrRowLds, 2u * (item & 127u), k + n1, n1, hs, w0, w1, &flipped);
      if (edges) {   // uniform
        const uint32_t *row = s_row + rl * kFrRowLds;
        const uint32_t wfirst = item & 127u, after = wfirst + n1 + k;   // base index behind the last k-mer
        auto cc = [&](uint32_t i) -> uint32_t { return (row[i >> 4] >> (2u * (i & 15u))) & 3u; };   // complement code of the run's base i
        // (the row holds complement codes in read direction: base code = 3 - cc; a record that travels reverse-complemented sees the
        // complements of its neighbours, on the other side)
        const uint32_t runx = s_runx[rl];
        const uint32_t lc = wfirst ? 1u + (3u - cc(wfirst - 1u)) : (runx & 7u);
        const uint32_t rc = wfirst + n1 + 1u < (uint32_t)s_runw[rl] ? 1u + (3u - cc(after)) : (runx >> 3);
        const uint32_t left = flipped ? (rc ? 5u - rc : 0u) : lc, right = flipped ? (lc ? 5u - lc : 0u) : rc;
        w1 |= ((uint64_t)(left | (right << 3)) << kRecEdgeShift) | ((uint64_t)(flipped ? 1u : 0u) << kRecFlipShift);
      }
      reinterpret_cast<ulonglong2 *>(out)[s_gbase[h27 >> 19] + s] = make_ulonglong2(w0, w1);
    }
    rb += n_taken;
    lds_barrier();   // the stage, the items and the run tables are done with; the counters are clear
  }
}

// the chain of the ranges' line indices: range r + 1 starts where range r ended (mod 4); totals: lines, runs, items
__global__ __launch_bounds__(1024) void sk_front_verify_kernel(const FrRange *__restrict__ info, uint32_t n_ranges, uint32_t ranges_per_group,
                                                             uint64_t *__restrict__ group_runs /* [groups]: runs of every group */,
                                                             uint64_t *__restrict__ totals /* [0] lines [1] runs [2] items */, uint32_t *__restrict__ flags) {
  __shared__ uint64_t s_scan[1024 / 64 + 2];
  __shared__ uint32_t s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  lds_barrier();
  // every thread takes a run of consecutive ranges: their sums first, one scan over the threads, then the chain through its own
  // ranges (a scan per 1024 ranges was 0.1 ms of a single workgroup once the front end cut the input into 12 k ranges and more)
  const uint32_t per = (n_ranges + 1023u) / 1024u;
  const uint32_t r_lo = threadIdx.x * per < n_ranges ? threadIdx.x * per : n_ranges, r_hi = r_lo + per < n_ranges ? r_lo + per : n_ranges;
  uint64_t my_lines = 0, my_runs = 0, my_its = 0;
  for (uint32_t r = r_lo; r < r_hi; ++r) {
    const FrRange fr = info[r];
    my_lines += fr.n_lines; my_runs += fr.n_runs; my_its += fr.n_items;
  }
  uint64_t carry = 0, runs = 0, its = 0;
  uint64_t before = block_exclusive_scan<uint64_t>(my_lines, s_scan, &carry);
  for (uint32_t r = r_lo; r < r_hi; ++r) {
    const FrRange fr = info[r];
    if (fr.l0 != kFrNone && fr.n_lines && ((uint32_t)before & 3u) != fr.l0) s_bad = 1;
    before += fr.n_lines;
  }
  (void)block_exclusive_scan<uint64_t>(my_runs, s_scan, &runs);
  (void)block_exclusive_scan<uint64_t>(my_its, s_scan, &its);
  lds_barrier();
  if (threadIdx.x == 0) {
    totals[0] = carry; totals[1] = runs; totals[2] = its;
    if (s_bad) atomicOr(&flags[FLAG_SK_DECLINED], 4u);
  }
  // runs per group (what a scatter workgroup will walk)
  const uint32_t groups = (n_ranges + ranges_per_group - 1) / ranges_per_group;
  for (uint32_t g = threadIdx.x; g < groups; g += blockDim.x) {
    uint64_t s = 0;
    for (uint32_t r = g * ranges_per_group; r < (g + 1) * ranges_per_group && r < n_ranges; ++r) s += info[r].n_runs;
    group_runs[g] = s;
  }
}

}  // namespace kmi
