// kmi_front_bytes.h -- what the one-pass FASTQ front end (kmi_front.h) does to a dword of four input bytes: the EOL test of its
// produce step and the 2-bit packing of its consume step. Pure functions, __host__ __device__ like those of kmi_device.h, with host
// definitions of the two byte instructions they are built on (v_perm_b32, v_dot4_u32_u8) beside the device ones, and nothing
// included but <stdint.h>: tests/cpu/front_bytes_check.cpp runs the very same code, built by any C++ compiler, against a
// byte-by-byte definition.
#pragma once
#include <stdint.h>

#ifndef KMI_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KMI_HD __host__ __device__ __forceinline__
#else
#define KMI_HD inline
#endif
#endif

namespace kmi {

// byte i of the result = byte (sel >> 8 i) & 7 of the eight bytes hi:lo (selectors above 7 are not used here)
KMI_HD uint32_t perm_b32(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const uint64_t tab = ((uint64_t)hi << 32) | lo;
  return (uint32_t)((tab >> (8u * (sel & 7u))) & 0xffu) | ((uint32_t)((tab >> (8u * ((sel >> 8) & 7u))) & 0xffu) << 8) |
         ((uint32_t)((tab >> (8u * ((sel >> 16) & 7u))) & 0xffu) << 16) | ((uint32_t)((tab >> (8u * ((sel >> 24) & 7u))) & 0xffu) << 24);
#endif
}
// 0x80 in every byte of y that is zero (exact: no carry leaves a byte)
KMI_HD uint32_t zero_bytes_b32(uint32_t y) { return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu); }

// the sum of the four byte products of a and b, plus c
KMI_HD uint32_t udot4_u8(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4(a, b, c, false);
#else
  return c + (a & 0xffu) * (b & 0xffu) + ((a >> 8) & 0xffu) * ((b >> 8) & 0xffu) + ((a >> 16) & 0xffu) * ((b >> 16) & 0xffu) + (a >> 24) * (b >> 24);
#endif
}

// 0x80 in every byte of w that is '\n' or '\r' (exact). A table of four bytes is looked up by a byte's low two bits: entry 2 is
// '\n' (0x0A), entry 1 is '\r' (0x0D), entry 0 is 0x01 and entry 3 is 0x00, whose low two bits are not their index -- so a byte
// equals the entry it selects iff it is one of the two (TAB, VT, FF, 0x02, 0x05, 0x0E, ... all differ from theirs). Three
// instructions before zero_bytes, and ONE constant in a register: v_perm_b32 takes no literal, and with the eight-entry table
// over the low three bits (two registers) the kernel went over its register budget.
KMI_HD uint32_t eol_flags(uint32_t w) {
  const uint32_t e = perm_b32(0u, 0x000A0D01u, w & 0x03030303u);
  return zero_bytes_b32(w ^ e);
}

// Four base bytes -> their four complement codes in the low byte (base i at bits 2 i: A 3, C 2, G 1, T 0, either case), and
// `diff` |= w ^ the letters those codes stand for: after any number of calls, (diff & 0xDFDFDFDF) has a non-zero byte where some
// dword held a byte that is none of A C G T a c g t. Such a byte gets the code of the letter it shares bits 1 and 2 with, NOT the
// code of A that pack_dna4 gives it: whoever finds the flag raised packs again with pack_dna4.
KMI_HD uint32_t pack_codes4(uint32_t w, uint32_t &diff) {
  const uint32_t idx = (w >> 1) & 0x03030303u;                 // A 0, C 1, T 2, G 3
  diff |= w ^ perm_b32(0u, 0x47544341u, idx);                 // 'A','C','T','G'
  return udot4_u8(perm_b32(0u, 0x01000203u, idx), 0x40100401u, 0u);
}
// the same difference for one dword alone
KMI_HD uint32_t dna4_diff(uint32_t w) { return w ^ perm_b32(0u, 0x47544341u, (w >> 1) & 0x03030303u); }
// 0xff in the first n bytes of a dword (n >= 4: all of them)
KMI_HD uint32_t first_bytes_mask(uint32_t n) { return n >= 4u ? 0xffffffffu : ((1u << (8u * n)) - 1u); }
// non-zero iff one of the first n bytes of w (n = 0 .. 4, more counts as 4) is none of A C G T a c g t
KMI_HD uint32_t dna4_other_in_first(uint32_t w, uint32_t n) { return dna4_diff(w) & 0xDFDFDFDFu & first_bytes_mask(n); }

}  // namespace kmi
