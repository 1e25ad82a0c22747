"""Prover randomness the library draws itself (zkvm_amd/csrc/prover_draw.hpp; seeds == NULL in the two provers):

    seed_i          = SHAKE256(call_seed || "statement" || LE64(i))[:32]
    blinding d of i = SHAKE256(seed_i || tag_d || LE64(index_d))[:64] mod l
    rng seed of i   = SHAKE256(seed_i || "rng" || LE64(0))[:32]

one Keccak-f per derivation -- the host side of the function k_pv_draw runs on the device, through libzkhost.so
(zkhost_prover_draw) against hashlib and Python integers, and once more as a stand-alone program under AddressSanitizer +
UBSan against keccak.hpp's byte-wise sponge."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 2**252 + 27742317777372353535851937790883648493
SEEDS = (bytes(32), hashlib.sha256(b"prover draw seed").digest())
POSITIONS = (0, 1, 63, 64, 2**32 - 1, 2**32, 2**63)
MS = (0, 1, 4, 8)


def cloak_table(m):
    """m = 2 nv commitments: (q_blinding j, f_blinding j) per value, then the rng seed"""
    t = []
    for j in range(m // 2):
        t += [(b"q_blinding", j), (b"f_blinding", j)]
    if m % 2:                                   # (an odd m is no cloak; the table is data all the same)
        t.append((b"q_blinding", m // 2))
    return t + [(b"rng", 0)]


def desc_table(m):
    return [(b"blinding", j) for j in range(m)] + [(b"rng", 0)]


TABLES = {"cloak": cloak_table, "described": desc_table}


def derive(seed, tag, index, n):
    return hashlib.shake_256(seed + tag + index.to_bytes(8, "little")).digest(n)


def want(call_seed, p, table):
    seed = derive(call_seed, b"statement", p, 32)
    out = b""
    for tag, index in table[:-1]:
        out += (int.from_bytes(derive(seed, tag, index, 64), "little") % L).to_bytes(32, "little")
    tag, index = table[-1]
    return out + derive(seed, tag, index, 32)


@pytest.fixture(scope="module")
def draw():
    from zkvm_amd import build
    build.build()
    lib = C.CDLL(os.path.join(ROOT, "zkvm_amd", "lib", "libzkhost.so"))
    lib.zkhost_prover_draw.restype = C.c_int
    lib.zkhost_prover_draw.argtypes = [C.c_char_p, C.c_uint64, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p]

    def call(seed, first, count, table):
        m = len(table) - 1
        rec = b"".join(tag.ljust(16, b"\0") + index.to_bytes(8, "little") for tag, index in table)
        out = C.create_string_buffer(32 * (m + 1) * count)
        rc = lib.zkhost_prover_draw(seed, first, count, rec, m, out)
        return rc, out.raw
    return call


@pytest.mark.parametrize("kind", sorted(TABLES))
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("seed", SEEDS, ids=("zero seed", "hashed seed"))
def test_draw_equals_shake256_and_integers_mod_l(draw, seed, m, kind):
    table = TABLES[kind](m)
    for p in POSITIONS:
        rc, got = draw(seed, p, 1, table)
        assert rc == 0 and got == want(seed, p, table), (p, m, kind)
        for d in range(m):
            assert int.from_bytes(got[32 * d: 32 * d + 32], "little") < L, (p, d)


@pytest.mark.parametrize("kind", sorted(TABLES))
def test_a_run_of_positions_is_one_draw_per_position(draw, kind):
    """count > 1: positions first .. first + count - 1, across the 2^32 boundary, each the single draw of its position"""
    seed, first, count, table = SEEDS[1], 2**32 - 3, 70, TABLES[kind](8)
    rc, got = draw(seed, first, count, table)
    assert rc == 0
    per = 32 * len(table)
    singles = [draw(seed, first + i, 1, table)[1] for i in range(count)]
    assert got == b"".join(singles) == b"".join(want(seed, first + i, table) for i in range(count))
    assert len({got[per * i + 32 * d: per * i + 32 * d + 32] for i in range(count) for d in range(len(table))}) == count * len(table)


def test_a_tag_the_message_cannot_hold_is_refused(draw):
    """32 + tag + 8 <= 50: a tag of eleven bytes (or none) would leave the one-permutation form"""
    assert draw(SEEDS[1], 0, 1, [(b"elevenbytes", 0), (b"rng", 0)])[0] == -1
    assert draw(SEEDS[1], 0, 1, [(b"", 0), (b"rng", 0)])[0] == -1
    assert draw(SEEDS[1], 0, 1, [(b"tenbytes__", 0), (b"rng", 0)])[0] == 0


SAN_MAIN = r"""
// prover_draw.hpp's host side against keccak.hpp's byte-wise sponge, which pads and squeezes by its own code, and
// scalar.hpp's reduction
#include "prover_draw.hpp"
#include "scalar.hpp"
#include <cstdio>
#include <string>
#include <vector>
static void shake(const uint8_t seed[32], const std::string& tag, uint64_t i, uint8_t* out, size_t n) {
  std::vector<uint8_t> in(seed, seed + 32);
  in.insert(in.end(), tag.begin(), tag.end());
  for (int q = 0; q < 8; ++q) in.push_back((uint8_t)(i >> (8 * q)));
  zk::Sponge sp = zk::shake256_sponge();
  sp.absorb(in.data(), in.size());
  sp.squeeze(out, n);
}
int main() {
  const uint64_t firsts[] = {0, 63, 0xfffffffdull, 0x7ffffffffffffff0ull, 0xfffffffffffffff0ull};
  const size_t ms[] = {0, 1, 4, 8};
  for (int s = 0; s < 2; ++s) {
    uint8_t call_seed[32];
    for (int i = 0; i < 32; ++i) call_seed[i] = (uint8_t)(s * (31 * i + 7));
    for (int kind = 0; kind < 2; ++kind)
      for (size_t m : ms) {
        if (kind == 0 && m % 2) continue;
        const std::vector<uint32_t> table = kind == 0 ? zk::pv_draw_table_cloak(m / 2) : zk::pv_draw_table_desc(m);
        if (table.size() != (m + 1) * zk::PV_DRAW_ENTRY_WORDS) { printf("table size\n"); return 1; }
        for (uint64_t first : firsts) {
          const size_t count = 5;
          std::vector<uint8_t> out(32 * (m + 1) * count);
          zk::pv_draw_bytes(call_seed, first, count, table.data(), m, out.data());
          for (size_t i = 0; i < count; ++i) {
            uint8_t seed[32], mine[32];
            shake(call_seed, "statement", first + i, seed, 32);
            zk::pv_statement_seed(call_seed, first + i, mine);
            if (memcmp(seed, mine, 32) != 0) { printf("statement seed differs: %d %llu + %zu\n", s, (unsigned long long)first, i); return 1; }
            for (size_t d = 0; d <= m; ++d) {
              uint8_t ref[64], want[32];
              const std::string tag = d == m ? "rng" : kind == 1 ? "blinding" : d % 2 ? "f_blinding" : "q_blinding";
              const uint64_t index = d == m ? 0 : kind == 1 ? d : d / 2;
              shake(seed, tag, index, ref, 64);
              if (d < m) zk::Scalar::from_wide(ref).to_bytes(want); else memcpy(want, ref, 32);
              if (memcmp(want, &out[32 * ((m + 1) * i + d)], 32) != 0) {
                printf("differs: seed %d kind %d m %zu first %llu + %zu derivation %zu\n", s, kind, m, (unsigned long long)first, i, d);
                return 1;
              }
            }
          }
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
    exe = tmp_path / "pv_draw_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I", os.path.join(ROOT, "zkvm_amd", "csrc"), str(main), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=200, env=env)
    assert p.returncode == 0 and "draw ok" in p.stdout and "Sanitizer" not in p.stderr, (p.stdout[-1500:], p.stderr[-4000:])
