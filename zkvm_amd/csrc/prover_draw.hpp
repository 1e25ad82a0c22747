// prover_draw.hpp -- prover randomness the library draws itself (seeds == NULL in zkgpu_cloak_prove_batch /
// zkgpu_r1cs_prove_batch, include/zkgpu.h), one derivation for the host and the device.
//
//     seed_i              = the first 32 bytes of SHAKE256(call_seed[32] || "statement" || LE64(i))            (FIPS 202)
//     blinding d of i     = the first 64 bytes of SHAKE256(seed_i || tag_d || LE64(index_d)), reduced mod l    (d < m)
//     rng seed of i       = the first 32 bytes of SHAKE256(seed_i || "rng" || LE64(0))                         (d = m)
//
// call_seed: 32 bytes from the OS (getrandom(2)), taken once per CALL; i: the statement's position in the call, whatever slice
// of the call proves it.  These are R1csProver::derive / derive_scalar applied to seed_i (r1cs_prover.hpp), so a call without
// seeds gives byte for byte what the same call with seeds = seed_0 || seed_1 || ... gives.  A message is 32 + tag + 8 <= 50
// bytes and an output <= 64: both fit the rate of 136, a derivation is ONE Keccak-f[1600] -- the message in lanes 0 .. 6, the
// padding 0x1F right behind it and 0x80 at byte 135 (the top byte of lane 16), the output lanes 0 .. 7.
//
// Everything behind the 32 seed bytes of a message -- tag, index, the 0x1F -- is at most 20 bytes: five little-endian words,
// the TAIL.  The tails of a system's m + 1 derivations (cloak: q_blinding j / f_blinding j interleaved, then rng 0; described
// system: blinding j, then rng 0) are a table the host builds from (tag, index) pairs and hands over as data, eight words an
// entry (five used); the tail of "statement" || LE64(i) is formed where i is known.
//
// Every secret of a proof is a function of seed_i: a call_seed is never reused, is wiped from host memory when the call
// returns, and a call whose seed could not be drawn fails before anything is launched (zkgpu.hip).
//
// Host side: keccak.hpp's keccak_f1600 and sc_dev.hpp's reduction (also what libzkhost's zkhost_prover_draw, the lockstep
// prover and the CPU tests run).  Device side: merlin_dev.hpp's keccak_f1600_halves, the state in registers, the same reduction.
#pragma once
#include "draw_r.hpp"     // DrawSeed, draw_seed, ZK_DRAW_HD
#include "sc_dev.hpp"

#include <vector>

namespace zk {

constexpr size_t PV_DRAW_TAG_MAX = 10;      // "q_blinding"; 32 + 10 + 8 = 50 message bytes
constexpr int PV_DRAW_ENTRY_WORDS = 8;      // a table entry: the five tail words, three words of zero

// the first 64 bytes of SHAKE256(seed[32] || tail bytes before their 0x1F) as sixteen little-endian words
ZK_DRAW_HD inline void pv_derive_words(const uint32_t seed[8], const uint32_t tail[5], uint32_t out[16]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t lo[25], hi[25];
#pragma unroll
  for (int q = 0; q < 25; ++q) lo[q] = hi[q] = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) { lo[q] = seed[2 * q]; hi[q] = seed[2 * q + 1]; }
  lo[4] = tail[0]; hi[4] = tail[1];
  lo[5] = tail[2]; hi[5] = tail[3];
  lo[6] = tail[4];
  hi[16] = 0x80000000u;
  keccak_f1600_halves(lo, hi);
#pragma unroll
  for (int q = 0; q < 8; ++q) { out[2 * q] = lo[q]; out[2 * q + 1] = hi[q]; }
#else
  uint64_t s[25] = {0};
  for (int q = 0; q < 4; ++q) s[q] = (uint64_t)seed[2 * q] | (uint64_t)seed[2 * q + 1] << 32;
  s[4] = (uint64_t)tail[0] | (uint64_t)tail[1] << 32;
  s[5] = (uint64_t)tail[2] | (uint64_t)tail[3] << 32;
  s[6] = tail[4];
  s[16] = 0x80ull << 56;
  keccak_f1600(s);
  for (int q = 0; q < 8; ++q) { out[2 * q] = (uint32_t)s[q]; out[2 * q + 1] = (uint32_t)(s[q] >> 32); }
#endif
}

// the tail of "statement" || LE64(p): nine tag bytes, the position from byte 9 on, 0x1F at byte 17
ZK_DRAW_HD inline void pv_statement_tail(uint64_t p, uint32_t tail[5]) {
  tail[0] = 0x74617473u;                                  // "stat"
  tail[1] = 0x6e656d65u;                                  // "emen"
  tail[2] = 0x74u | (uint32_t)(p & 0xffffffu) << 8;       // "t", p bits 0 .. 23
  tail[3] = (uint32_t)(p >> 24);
  tail[4] = (uint32_t)(p >> 56) | 0x1Fu << 8;
}

// seed_p as eight words
ZK_DRAW_HD inline void pv_statement_seed_words(const DrawSeed& call_seed, uint64_t p, uint32_t out[8]) {
  uint32_t tail[5], w[16];
  pv_statement_tail(p, tail);
  pv_derive_words(call_seed.w, tail, w);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int q = 0; q < 8; ++q) out[q] = w[q];
}

// One derivation of statement p: its seed, then the entry's message -- two permutations.  scalar: 64 bytes reduced mod l,
// canonical plain words (PvBatch::blindings); otherwise the first 32 bytes as they are (PvBatch::rng_seed).
ZK_DRAW_HD inline void pv_draw_one(const DrawSeed& call_seed, uint64_t p, const uint32_t tail[5], bool scalar, uint32_t out[8]) {
  uint32_t seed[8], w[16];
  pv_statement_seed_words(call_seed, p, seed);
  pv_derive_words(seed, tail, w);
  if (scalar) {
    scm_to_words(out, scm_from_wide(w));
  } else {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < 8; ++q) out[q] = w[q];
  }
}

// ---- host: the table, and the draws as bytes -------------------------------------------------------------------------------
// tag || LE64(index) || 0x1F as an entry; false: the tag is empty or longer than PV_DRAW_TAG_MAX
inline bool pv_draw_entry(const char* tag, size_t tag_len, uint64_t index, uint32_t entry[PV_DRAW_ENTRY_WORDS]) {
  for (int q = 0; q < PV_DRAW_ENTRY_WORDS; ++q) entry[q] = 0;
  if (tag_len == 0 || tag_len > PV_DRAW_TAG_MAX) return false;
  uint8_t b[20] = {0};
  memcpy(b, tag, tag_len);
  for (int k = 0; k < 8; ++k) b[tag_len + k] = (uint8_t)(index >> (8 * k));
  b[tag_len + 8] = 0x1F;
  for (int q = 0; q < 5; ++q)
    entry[q] = (uint32_t)b[4 * q] | (uint32_t)b[4 * q + 1] << 8 | (uint32_t)b[4 * q + 2] << 16 | (uint32_t)b[4 * q + 3] << 24;
  return true;
}

inline void pv_draw_table_put(std::vector<uint32_t>& t, const char* tag, uint64_t index) {
  uint32_t e[PV_DRAW_ENTRY_WORDS];
  (void)pv_draw_entry(tag, strlen(tag), index, e);
  t.insert(t.end(), e, e + PV_DRAW_ENTRY_WORDS);
}
// the cloak's 2 nv commitments (quantity, flavor per value) and its rng seed: 2 nv + 1 entries
inline std::vector<uint32_t> pv_draw_table_cloak(size_t nv) {
  std::vector<uint32_t> t;
  for (size_t j = 0; j < nv; ++j) { pv_draw_table_put(t, "q_blinding", j); pv_draw_table_put(t, "f_blinding", j); }
  pv_draw_table_put(t, "rng", 0);
  return t;
}
// a described system's m commitments and its rng seed: m + 1 entries
inline std::vector<uint32_t> pv_draw_table_desc(size_t m) {
  std::vector<uint32_t> t;
  for (size_t j = 0; j < m; ++j) pv_draw_table_put(t, "blinding", j);
  pv_draw_table_put(t, "rng", 0);
  return t;
}

inline void pv_words_to_bytes(const uint32_t w[8], uint8_t out[32]) {
  for (int q = 0; q < 8; ++q)
    for (int b = 0; b < 4; ++b) out[4 * q + b] = (uint8_t)(w[q] >> (8 * b));
}

// seed_p as bytes (the lockstep prover hands it to R1csProver as the statement's seed)
inline void pv_statement_seed(const uint8_t call_seed[32], uint64_t p, uint8_t out[32]) {
  uint32_t w[8];
  pv_statement_seed_words(draw_seed(call_seed), p, w);
  pv_words_to_bytes(w, out);
}

// statements first .. first + count - 1 over a table of m + 1 entries: per statement m blindings of 32 bytes (canonical,
// little endian), then the 32 bytes of the rng seed
inline void pv_draw_bytes(const uint8_t call_seed[32], uint64_t first, size_t count, const uint32_t* table, size_t m, uint8_t* out) {
  const DrawSeed s = draw_seed(call_seed);
  for (size_t i = 0; i < count; ++i)
    for (size_t d = 0; d <= m; ++d) {
      uint32_t w[8];
      pv_draw_one(s, first + i, table + PV_DRAW_ENTRY_WORDS * d, d < m, w);
      pv_words_to_bytes(w, out + 32 * ((m + 1) * i + d));
    }
}

#if defined(__HIPCC__)
// One lane per (statement, derivation): derivations d0 .. m of statements first .. first + count - 1 (d0 = m: the caller
// brought the blindings, only the rng seeds are drawn).  The 50 state words in registers, no LDS, no scratch; a lane's 32
// bytes leave as two uint4 -- blindings and rng_seed are regions of a context's own input area, at multiples of 32 bytes, and
// table is 16-byte aligned.  `lanes` = count (m + 1 - d0); lanes past it leave before they touch memory.
__global__ void __launch_bounds__(64)
k_pv_draw(DrawSeed call_seed, uint64_t first, uint64_t lanes, uint32_t m, uint32_t d0, const uint32_t* __restrict__ table,
          uint32_t* __restrict__ blindings, uint32_t* __restrict__ rng_seed) {
  const uint64_t g = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= lanes) return;
  const uint32_t per = m + 1 - d0;
  const uint64_t i = g / per;
  const uint32_t d = d0 + (uint32_t)(g - i * per);
  const uint4 t4 = *(const uint4*)(table + PV_DRAW_ENTRY_WORDS * (uint64_t)d);
  const uint32_t tail[5] = {t4.x, t4.y, t4.z, t4.w, table[PV_DRAW_ENTRY_WORDS * (uint64_t)d + 4]};
  uint32_t w[8];
  pv_draw_one(call_seed, first + i, tail, d < m, w);
  uint4* o = (uint4*)(d < m ? blindings + (i * m + d) * 8 : rng_seed + i * 8);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]);
  o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
#endif

}  // namespace zk
