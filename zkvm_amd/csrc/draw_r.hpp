// draw_r.hpp -- verifier randomness the library draws itself, one derivation for the host and the device.
//
//     r(seed, p) = the first 64 bytes of SHAKE256(seed[32] || LE64(p))                                   (FIPS 202)
//
// seed: 32 bytes from the OS (getrandom(2)), taken once per device batch; p: the statement's position in that batch.  40 bytes in
// and 64 bytes out fit the rate of 136, so a draw is ONE Keccak-f[1600]: the message in lanes 0 .. 4, the padding 0x1F at byte 40
// (lane 5) and 0x80 at byte 135 (the top byte of lane 16), the output lanes 0 .. 7.  The same construction as the host draws of
// session.hpp (a block's transactions, a host ticket), written once here so that a caller who keeps its proofs in HBM need not
// produce and upload 64 bytes of CSPRNG output per statement (include/zkgpu.h: d_r == NULL).
//
// r is the soundness parameter of the group checks (rho = r^2 weights a statement inside its group): a seed is never reused, and
// a draw that could not be made fails the batch (zkgpu.hip, session.hpp) -- stale bytes are never an r.
//
// Host side: keccak.hpp's keccak_f1600 (also what libzkhost's zkhost_draw_r and the CPU tests run).  Device side: merlin_dev.hpp's
// keccak_f1600_halves, the state in registers.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include "merlin_dev.hpp"
#define ZK_DRAW_HD __host__ __device__
#else
#define ZK_DRAW_HD
#endif
#include "keccak.hpp"

namespace zk {

struct DrawSeed { uint32_t w[8]; };      // the 32 seed bytes as little-endian words (a kernel argument, by value)

inline DrawSeed draw_seed(const uint8_t bytes[32]) {
  DrawSeed s;
  for (int q = 0; q < 8; ++q)
    s.w[q] = (uint32_t)bytes[4 * q] | (uint32_t)bytes[4 * q + 1] << 8 | (uint32_t)bytes[4 * q + 2] << 16 | (uint32_t)bytes[4 * q + 3] << 24;
  return s;
}

// out: the 64 bytes of r(seed, p) as sixteen little-endian words
ZK_DRAW_HD inline void draw_r_words(const DrawSeed& seed, uint64_t p, uint32_t out[16]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t lo[25], hi[25];
#pragma unroll
  for (int q = 0; q < 25; ++q) lo[q] = hi[q] = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) { lo[q] = seed.w[2 * q]; hi[q] = seed.w[2 * q + 1]; }
  lo[4] = (uint32_t)p; hi[4] = (uint32_t)(p >> 32);
  lo[5] = 0x1Fu;
  hi[16] = 0x80000000u;
  keccak_f1600_halves(lo, hi);
#pragma unroll
  for (int q = 0; q < 8; ++q) { out[2 * q] = lo[q]; out[2 * q + 1] = hi[q]; }
#else
  uint64_t s[25] = {0};
  for (int q = 0; q < 4; ++q) s[q] = (uint64_t)seed.w[2 * q] | (uint64_t)seed.w[2 * q + 1] << 32;
  s[4] = p;
  s[5] = 0x1Full;
  s[16] = 0x80ull << 56;
  keccak_f1600(s);
  for (int q = 0; q < 8; ++q) { out[2 * q] = (uint32_t)s[q]; out[2 * q + 1] = (uint32_t)(s[q] >> 32); }
#endif
}

// host: r(seed, first) .. r(seed, first + count - 1) as bytes, 64 each
inline void draw_r_bytes(const uint8_t seed[32], uint64_t first, size_t count, uint8_t* out) {
  const DrawSeed s = draw_seed(seed);
  for (size_t i = 0; i < count; ++i) {
    uint32_t w[16];
    draw_r_words(s, first + i, w);
    for (int q = 0; q < 16; ++q)
      for (int b = 0; b < 4; ++b) out[64 * i + 4 * q + b] = (uint8_t)(w[q] >> (8 * b));
  }
}

#if defined(__HIPCC__)
// One lane per statement, the 50 state words in registers (no LDS, no scratch), the lane's 64 bytes written as four uint4 --
// out is 16-byte aligned: a context's own buffer, at a multiple of 64 bytes.  Lanes past `count` leave before they touch memory.
__global__ void __launch_bounds__(64)
k_draw_r(DrawSeed seed, uint64_t first, uint32_t count, uint4* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  uint32_t w[16];
  draw_r_words(seed, first + i, w);
  uint4* o = out + 4 * (uint64_t)i;
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}
#endif

}  // namespace zk
