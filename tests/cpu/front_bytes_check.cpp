// The dword functions of the one-pass FASTQ front end (kmerind_amd/csrc/kmi_front_bytes.h), run on the host with the header's own
// host definitions of the byte-permute and dot-product instructions, against definitions written byte by byte:
//   eol_flags            0x80 in a byte iff it is '\n' or '\r'
//   pack_codes4          the 2-bit complement code of every byte that is one of A C G T a c g t, at bits 2 i of the result
//                        (A 3, C 2, G 1, T 0), and a difference word that is non-zero under 0xDFDFDFDF iff some byte is none of them
//   dna4_other_in_first  "one of the first n bytes is none of A C G T a c g t", n = 0 .. 4
// over every pair of byte values in every pair of positions of a dword (the other two bytes from a few fillers), and over 2e8
// random dwords (half of them drawn from the bytes a FASTQ file is made of, so that dwords of four bases come up).
// Prints "front_bytes_check: N dwords, 0 mismatches" and returns 0, or the first mismatches and 1.
#include <stdint.h>
#include <stdio.h>

#include "kmi_front_bytes.h"

// byte tables of the definitions: '\n' / '\r', and the complement code of a base (4: not a base)
static uint8_t t_eol[256], t_code[256];
static void make_tables() {
  for (int c = 0; c < 256; ++c) {
    t_eol[c] = (c == 0x0A || c == 0x0D) ? 0x80u : 0u;
    t_code[c] = 4;
  }
  t_code['A'] = t_code['a'] = 3; t_code['C'] = t_code['c'] = 2; t_code['G'] = t_code['g'] = 1; t_code['T'] = t_code['t'] = 0;
}

static unsigned long long n_checked = 0, n_bad = 0;
static void fail(const char *what, uint32_t w, uint32_t got, uint32_t want) {
  if (n_bad++ < 10) fprintf(stderr, "%s: w = 0x%08x got 0x%08x want 0x%08x\n", what, w, got, want);
}

template <bool ALL_N> static inline void check(uint32_t w, uint32_t one_n = 0) {
  ++n_checked;
  const uint32_t b0 = w & 0xffu, b1 = (w >> 8) & 0xffu, b2 = (w >> 16) & 0xffu, b3 = w >> 24;
  const uint32_t want_eol = (uint32_t)t_eol[b0] | ((uint32_t)t_eol[b1] << 8) | ((uint32_t)t_eol[b2] << 16) | ((uint32_t)t_eol[b3] << 24);
  const uint32_t c0 = t_code[b0], c1 = t_code[b1], c2 = t_code[b2], c3 = t_code[b3];
  const uint32_t got_eol = kmi::eol_flags(w);
  if (got_eol != want_eol) fail("eol_flags", w, got_eol, want_eol);
  uint32_t diff = 0;
  const uint32_t packed = kmi::pack_codes4(w, diff);
  // the codes of the bytes that are bases, where they belong; nothing above the low byte
  const uint32_t vmask = (c0 < 4u ? 0x03u : 0u) | (c1 < 4u ? 0x0Cu : 0u) | (c2 < 4u ? 0x30u : 0u) | (c3 < 4u ? 0xC0u : 0u);
  const uint32_t want_codes = ((c0 & 3u) | ((c1 & 3u) << 2) | ((c2 & 3u) << 4) | ((c3 & 3u) << 6)) & vmask;
  if ((packed & vmask) != want_codes || packed > 0xffu) fail("pack_codes4", w, packed, want_codes);
  // the difference word: a byte is zero under the case bit iff it is a base
  const uint32_t d = diff & 0xDFDFDFDFu;
  const uint32_t got_other = ((d & 0xffu) ? 1u : 0u) | ((d & 0xff00u) ? 2u : 0u) | ((d & 0xff0000u) ? 4u : 0u) | ((d & 0xff000000u) ? 8u : 0u);
  const uint32_t want_other = (c0 < 4u ? 0u : 1u) | (c1 < 4u ? 0u : 2u) | (c2 < 4u ? 0u : 4u) | (c3 < 4u ? 0u : 8u);
  if (got_other != want_other) fail("pack_codes4 diff", w, got_other, want_other);
  if (kmi::dna4_diff(w) != diff) fail("dna4_diff", w, kmi::dna4_diff(w), diff);
  // "some byte of the first n is not a base", n = 0 .. 5 (more than four counts as four): every n, or the one the caller names
  for (uint32_t n = ALL_N ? 0u : one_n; n <= (ALL_N ? 5u : one_n); ++n) {
    const uint32_t want = (want_other & ((1u << (n < 4u ? n : 4u)) - 1u)) ? 1u : 0u;
    const uint32_t got = kmi::dna4_other_in_first(w, n) ? 1u : 0u;
    if (got != want) fail("dna4_other_in_first", w, n, want);
  }
}

int main() {
  make_tables();
  // every pair of byte values in every pair of positions
  static const uint32_t fill[] = {0x00u, 0xffu, 'A', 't', '\n', '\r', 'N', 0x80u | 'C'};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      for (uint32_t f = 0; f < sizeof(fill) / sizeof(fill[0]); ++f) {
        const uint32_t base = fill[f] * 0x01010101u & ~((0xffu << (8 * i)) | (0xffu << (8 * j)));
        for (uint32_t a = 0; a < 256; ++a)
          for (uint32_t b = 0; b < 256; ++b) check<true>(base | (a << (8 * i)) | (b << (8 * j)));
      }
  // a dword at the head of each tail length: n bases, then what lies behind a read (EOL, '+', quality characters that are bases)
  static const char *tails[] = {"ACGT", "ACG\n", "AC\n+", "A\n+\n", "\n+\nA", "acgt", "ACGN", "NCGT", "AC\r\n", "TTTI"};
  for (const char *t : tails) check<true>((uint32_t)(uint8_t)t[0] | ((uint32_t)(uint8_t)t[1] << 8) | ((uint32_t)(uint8_t)t[2] << 16) | ((uint32_t)(uint8_t)t[3] << 24));
  // random dwords: uniform, and from the bytes of a FASTQ file (each with one prefix length n, drawn too)
  static const uint8_t alpha[16] = {'A', 'C', 'G', 'T', 'A', 'C', 'G', 'T', 'a', 'c', 'g', 't', 'N', '\n', '\r', 'I'};
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (uint32_t it = 0; it < 100000000u; ++it) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    check<false>((uint32_t)(s >> 32), it % 6u);
    const uint32_t r = (uint32_t)s;
    check<false>((uint32_t)alpha[r & 15u] | ((uint32_t)alpha[(r >> 4) & 15u] << 8) | ((uint32_t)alpha[(r >> 8) & 15u] << 16) | ((uint32_t)alpha[(r >> 12) & 15u] << 24), (r >> 16) % 6u);
  }
  printf("front_bytes_check: %llu dwords, %llu mismatches\n", n_checked, n_bad);
  return n_bad ? 1 : 0;
}
