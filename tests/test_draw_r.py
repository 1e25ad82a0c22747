"""Verifier randomness the library draws itself (zkvm_amd/csrc/draw_r.hpp): r(seed, p) = the first 64 bytes of
SHAKE256(seed || LE64(p)), one Keccak-f per draw -- the host side of the function k_draw_r runs on the device, through
libzkhost.so (zkhost_draw_r) against hashlib, and once more as a stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (bytes(32), hashlib.sha256(b"draw_r seed").digest())
POSITIONS = (0, 1, 63, 64, 2**32 - 1, 2**32, 2**63)


def want(seed: bytes, p: int) -> bytes:
    return hashlib.shake_256(seed + p.to_bytes(8, "little")).digest(64)


@pytest.fixture(scope="module")
def draw():
    from zkvm_amd import build
    build.build()
    lib = C.CDLL(os.path.join(ROOT, "zkvm_amd", "lib", "libzkhost.so"))
    lib.zkhost_draw_r.restype = None
    lib.zkhost_draw_r.argtypes = [C.c_char_p, C.c_uint64, C.c_size_t, C.c_char_p]

    def call(seed, first, count):
        out = C.create_string_buffer(64 * count)
        lib.zkhost_draw_r(seed, first, count, out)
        return out.raw
    return call


@pytest.mark.parametrize("seed", SEEDS, ids=("zero seed", "hashed seed"))
def test_draw_equals_shake256_of_seed_and_position(draw, seed):
    for p in POSITIONS:
        assert draw(seed, p, 1) == want(seed, p), p


def test_a_run_of_draws_is_one_draw_per_position(draw):
    """count > 1: positions first .. first + count - 1, across the 2^32 boundary, each 64 bytes of its own"""
    seed, first, count = SEEDS[1], 2**32 - 3, 70
    got = draw(seed, first, count)
    assert got == b"".join(want(seed, first + i) for i in range(count))
    assert len({got[64 * i: 64 * i + 64] for i in range(count)}) == count


SAN_MAIN = r"""
// draw_r.hpp's host side against keccak.hpp's byte-wise sponge, which pads and squeezes by its own code
#include "draw_r.hpp"
#include <cstdio>
#include <vector>
int main() {
  const uint64_t firsts[] = {0, 63, 0xfffffffdull, 0x7ffffffffffffff0ull, 0xfffffffffffffff0ull};
  for (int s = 0; s < 2; ++s) {
    uint8_t seed[32];
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(s * (31 * i + 7));
    for (uint64_t first : firsts) {
      const size_t count = 9;
      std::vector<uint8_t> out(64 * count);
      zk::draw_r_bytes(seed, first, count, out.data());
      for (size_t i = 0; i < count; ++i) {
        uint8_t in[40], ref[64];
        memcpy(in, seed, 32);
        for (int q = 0; q < 8; ++q) in[32 + q] = (uint8_t)((first + i) >> (8 * q));
        zk::Sponge sp = zk::shake256_sponge();
        sp.absorb(in, 40);
        sp.squeeze(ref, 64);
        if (memcmp(ref, &out[64 * i], 64) != 0) { printf("differs: seed %d first %llu + %zu\n", s, (unsigned long long)first, i); return 1; }
      }
    }
  }
  printf("draw ok\n");
  return 0;
}
"""


@pytest.mark.timeout(300)
def test_shared_function_under_asan_ubsan_as_a_standalone_program(tmp_path):
    have = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(have) and os.path.exists(have)):
        pytest.skip("gcc has no libasan here")
    main = tmp_path / "main.cpp"
    main.write_text(SAN_MAIN)
    exe = tmp_path / "draw_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "zkvm_amd", "csrc"), str(main), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=200, env=env)
    assert p.returncode == 0 and "draw ok" in p.stdout and "Sanitizer" not in p.stderr, (p.stdout[-1500:], p.stderr[-4000:])
