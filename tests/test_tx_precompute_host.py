"""ZKGPU_TXFORMAT_PRECOMPUTE_ONLY (0x2000) on the CPU tier: the first half of upstream's Tx::verify alone -- the VM, the
transaction ID and the log, nothing verified.

  1. the format word: the validity rule over the full cross product, decoded by the library's own header (csrc/tx_out.hpp);
  2. the side table of the hash tape walked by dependency level (csrc/tx_hash_levels.hpp) is a topological order of every
     shape's jobs, and gives each job its place in the transaction's byte run;
  3. the level interpreter -- the function k_tx_hash_levels runs per lane -- run on the host lane by lane and level by level,
     with T and T / 2 lanes per transaction, leaves the slots and IDs tx_hash_run leaves, and the IDs are the oracle's;
  4. the scheduler of a transaction call (csrc/tx_call.hpp) under the flag over a stand-in device: no key, proof or signature
     operation is asked for; statuses, IDs and records are as constructed; an error of the stand-in leaves 1 and zeros;
  5. tools/tx_precompute_check.cpp, a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer.
"""
import ctypes as C
import os
import random
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_tx_hash_tape import host, wrapped  # noqa: E402,F401
from tx_log_util import area_bytes, check_accepted, record_bytes, split_area  # noqa: E402

PRE = 0x2000
T = 4                                                     # csrc/tx_hash_levels.hpp: TAPE_LEVEL_LANES
LEVEL_SHAPES = [(1, 1), (2, 2), (3, 1), (1, 3), (4, 4), (8, 8), (1, 16)]
GUARD = 64


def _offsets(txs):
    n = len(txs)
    return (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:i + 1]) for i in range(n)]))


# ---- 1. the format word ------------------------------------------------------------------------------------------------------
def _decode(host, word):
    out = (C.c_int64 * 7)(*([-7] * 7))
    assert host.zkhost_tx_out_layout(C.c_int(0), (C.c_int64 * 1)(word), None, None, None, None, out) == 0
    return list(out)


def _valid_without_the_flag(base, hash_, sign, ids, log_k):
    """the rule of the parent commit (tests/test_tx_out_layout.py holds the library against its own table of it)"""
    if base == 0:
        return not (hash_ or sign or ids or log_k)
    return not (sign and not hash_) and not (log_k and not ids)


def test_format_decoding_over_the_full_cross_product(host):
    seen_valid = 0
    for base in (0, 1, 2):
        for hash_ in (0, 0x100):
            for sign in (0, 0x200):
                for ids in (0, 0x400):
                    for k in (0, 1, 4, 255):
                        plain = base | hash_ | sign | ids | ((0x800 | (k << 16)) if k else 0)
                        ok = _valid_without_the_flag(base, hash_, sign, ids, k)
                        got = _decode(host, plain)
                        assert got[0] == int(ok), hex(plain)
                        if ok:
                            assert got[1:7] == [base, int(bool(hash_)), int(bool(sign)), int(bool(ids)), k, 0], hex(plain)
                        # ... and with the flag: valid exactly when the word without it is, the base is 1 or 2, 0x400 is set, 0x200 is not
                        want = ok and base in (1, 2) and bool(ids) and not sign
                        got = _decode(host, plain | PRE)
                        assert got[0] == int(want), hex(plain | PRE)
                        if want:
                            seen_valid += 1
                            assert got[1:7] == [base, int(bool(hash_)), 0, 1, k, 1], hex(plain | PRE)
    assert seen_valid == 2 * 2 * 4
    for word in (PRE, PRE | 0x400, PRE | 1, PRE | 2, PRE | 0x101, PRE | 0x701, PRE | 0x401 | 0x1000, PRE | 0x401 | 0x4000, PRE | 0x401 | (1 << 24),
                 PRE | 0x401 | (4 << 16), PRE | 0xC01, PRE | 3 | 0x400):
        assert _decode(host, word)[0] == 0, hex(word)
    # a window alone, the flag's neighbours alone: as on the parent
    for word in (0x1000, 0x4000, 0x8000, 0x401 | 0x1000, 0x401 | 0x4000):
        assert _decode(host, word)[0] == 0, hex(word)


def test_the_constants_are_mirrored_everywhere_and_the_abi_is_what_it_was():
    read = lambda *p: open(os.path.join(ROOT, *p)).read()      # noqa: E731
    header = dict((n, int(v)) for n, v in re.findall(r"#define\s+(ZKGPU_[A-Z0-9_]+)\s+(-?\d+)\b", read("include", "zkgpu.h")))
    rust = dict((n, int(v)) for n, v in re.findall(r"pub const (ZKGPU_[A-Z0-9_]+): c_int = (-?\d+);", read("rust", "zkgpu-sys", "src", "lib.rs")))
    import zkvm_amd
    from zkvm_amd import native
    from zkvm_amd.verifier import BlockVerifier
    for name, value in {"ZKGPU_TXFORMAT_PRECOMPUTE_ONLY": 8192, "ZKGPU_TXSTATUS_PRECOMPUTED": 3}.items():
        short = name[len("ZKGPU_"):]
        assert header.get(name) == value == rust.get(name), name
        assert getattr(native, short) == getattr(zkvm_amd, short) == getattr(BlockVerifier, short) == value, name
    wrapper = read("rust", "zkgpu", "src", "lib.rs")
    assert "sys::ZKGPU_TXFORMAT_PRECOMPUTE_ONLY" in wrapper and "pub fn precompute(" in wrapper
    from test_capi_symbols import _declared, _hooks_declared
    assert len(_declared()) == 90 and len(_hooks_declared()) == 25
    assert "return 3;" in re.search(r"int zkgpu_abi_version\(void\)\s*\{[^}]*\}", read("zkvm_amd", "csrc", "zkgpu.hip")).group(0)


def test_the_python_wrapper_refuses_before_it_calls_the_library():
    from zkvm_amd.verifier import BlockVerifier
    bv = BlockVerifier.__new__(BlockVerifier)
    with pytest.raises(ValueError):                          # (the format in force is not a precompute-only one)
        bv.precompute_txs([b"x"])
    bv._tx_return_ids = True
    with pytest.raises(ValueError):
        bv.precompute_txs([b"x"])
    bv._tx_precompute = True
    with pytest.raises(ValueError):                          # (a verifying call under a precompute-only format would read 3 as "rejected")
        bv.verify_txs([b"x"])


# ---- 2, 3. the side table and the level walk ---------------------------------------------------------------------------------
def _levels(host, txs, lanes):
    n = len(txs)
    host.zkhost_tx_hash_levels.restype = C.c_longlong
    cap = 1 << 18
    status = C.create_string_buffer(n)
    block, table, sizes = (C.c_uint32 * cap)(), (C.c_uint32 * cap)(), (C.c_uint64 * 4)()
    by_levels, by_run = C.create_string_buffer(32 * n), C.create_string_buffer(32 * n)
    rc = host.zkhost_tx_hash_levels(b"".join(txs), _offsets(txs), C.c_size_t(n), C.c_int(2), C.c_uint32(lanes), status, block, C.c_size_t(cap),
                                    table, C.c_size_t(cap), sizes, by_levels, by_run)
    return dict(rc=rc, status=status.raw, block=list(block[: sizes[0]]), table=list(table[: sizes[1]]), slot_words_differ=sizes[3],
                by_levels=[by_levels.raw[32 * i: 32 * i + 32] for i in range(n)], by_run=[by_run.raw[32 * i: 32 * i + 32] for i in range(n)])


@pytest.fixture(scope="module")
def shaped(oracle):
    """three payments of every shape in a drawn order, one truncated (not on the tape)"""
    txs = [wrapped(oracle, a, b, 4000 + 100 * a + 10 * b + c) for a, b in LEVEL_SHAPES for c in range(3)]
    random.Random(11).shuffle(txs)
    txs[4] = txs[4][:-1]
    return txs


def _head(block):
    names = "magic n_lanes n_tx n_shapes shapes jobs pieces lanes txs data n_jobs n_pieces data_bytes n_slots words zero".split()
    return dict(zip(names, block[:16]))


def test_the_side_table_is_a_topological_order_of_every_shape(host, shaped):
    out = _levels(host, shaped, T)
    assert out["rc"] == len(shaped) - 1
    b, tab, h = out["block"], out["table"], _head(out["block"])
    assert h["n_shapes"] == len(LEVEL_SHAPES) and tab[1] == h["n_shapes"] and tab[2] == len(tab)
    widest, most = 0, 0
    for s in range(h["n_shapes"]):
        job0, n_jobs, n_slots, _root = b[h["shapes"] + 4 * s: h["shapes"] + 4 * s + 4]
        at = tab[4 + s]
        L, J = tab[at], tab[at + 1]
        first = tab[at + 2: at + 2 + L + 1]
        order = tab[at + 2 + L + 1: at + 2 + L + 1 + 2 * J]
        assert J == n_jobs and first[0] == 0 and first[L] == J and all(first[q] < first[q + 1] for q in range(L))
        level, offset = {}, {}
        for lv in range(L):
            for q in range(first[lv], first[lv + 1]):
                assert order[2 * q] not in level
                level[order[2 * q]], offset[order[2 * q]] = lv, order[2 * q + 1]
        assert sorted(level) == list(range(J))
        producer, cursor = {}, 0
        for j in range(J):
            _w0, out_slot, p0, n_p = b[h["jobs"] + 4 * (job0 + j): h["jobs"] + 4 * (job0 + j) + 4]
            assert offset[j] == cursor, (s, j)               # the cursor tx_hash_run would have reached
            need = 0
            for p in range(p0, p0 + n_p):
                w0, ln, _msg, slot = b[h["pieces"] + 4 * p: h["pieces"] + 4 * p + 4]
                if w0 >> 8 == 1:                             # TAPE_SLOT
                    assert slot < n_slots
                    if slot in producer:
                        assert level[producer[slot]] < level[j], (s, j, slot)     # every slot piece's producer has a lower level
                        need = max(need, level[producer[slot]] + 1)
                else:
                    cursor += ln
            assert level[j] == need, (s, j)                  # ... and the job stands at the lowest level they allow
            assert out_slot not in producer
            producer[out_slot] = j
        widest = max(widest, max(first[q + 1] - first[q] for q in range(L)))
        most = max(most, L)
    assert widest > T, "no shape has a level wider than T: the rounds of a level are not exercised"
    assert tab[3] == most


@pytest.mark.parametrize("lanes", [T, T // 2])
def test_the_level_walk_leaves_what_tx_hash_run_leaves_and_the_oracles_ids(host, oracle, shaped, lanes):
    out = _levels(host, shaped, lanes)
    assert out["rc"] == len(shaped) - 1 and out["slot_words_differ"] == 0
    assert out["by_levels"] == out["by_run"]
    for i, t in enumerate(shaped):
        if i == 4:
            assert out["status"][i] == 1 and out["by_levels"][i] == bytes(32)
            continue
        rc, want, _, _ = oracle.tx_id(t)
        assert rc == 0 and out["status"][i] == 0 and out["by_levels"][i] == want, i


# ---- 4. TxCall under the flag over a stand-in device -------------------------------------------------------------------------
def _call(host, txs, hashing, reasons, k, threads=4, chunk=0, seed=1, hash_fail_at=-1, slots=2):
    n = len(txs)
    size = area_bytes(n, k) if k else 33 * n
    bm = C.create_string_buffer(b"\xff" * ((n + 7) // 8), (n + 7) // 8)
    st = C.create_string_buffer(b"\xa5" * (size + GUARD), size + GUARD)
    out = (C.c_uint64 * 6)()
    rc = host.zkhost_txcall_precompute_selftest(C.c_int(hashing), C.c_int(reasons), C.c_size_t(k), C.c_size_t(n), b"".join(txs), _offsets(txs),
                                                C.c_int(threads), C.c_size_t(chunk), C.c_uint32(seed), C.c_int(hash_fail_at), C.c_int(slots), bm, st, out)
    assert st.raw[size:] == b"\xa5" * GUARD, "guard bytes overwritten"
    if k:
        status, ids, recs = split_area(st.raw, n, k)
    else:
        status, ids, recs = st.raw[:n], [st.raw[n + 32 * i: n + 32 * i + 32] for i in range(n)], [b""] * n
    names = ("chunks", "stage_ops", "host_hashed", "device_hashed", "precomputed", "dirty")
    return rc, bm.raw, status, ids, recs, dict(zip(names, out))


CORPUS_SHAPES = [(1, 1), (2, 2), (3, 2), (2, 3)]          # 2, 4, 5, 5 log entries


def _non_canonical_s(tx):
    """the signature's scalar s (the last 32 of the 64 bytes behind the program) set to 2^256 - 1"""
    at = 28 + int.from_bytes(tx[24:28], "little")
    return tx[: at + 32] + b"\xff" * 32 + tx[at + 64:]


@pytest.fixture(scope="module")
def corpus(oracle):
    """valid payments of four shapes, and among them: outside the subset (a later version), VM-invalid (truncated; mintime after
    maxtime), a non-canonical s, and -- what a precompute-only call must NOT see -- a forged signature and a corrupt proof.
    -> transactions, the status a format-1 call writes, the status a format-2 call writes"""
    n = 60
    txs = [wrapped(oracle, *CORPUS_SHAPES[i % 4], 5000 + i) for i in range(n)]
    v1, v2 = bytearray([3] * n), bytearray([3] * n)
    t = bytearray(txs[9]); t[0] = 2; txs[9] = bytes(t)                       # outside the subset
    v1[9] = v2[9] = 2
    txs[13] = txs[13][:-1]                                                   # truncated
    txs[26] = txs[26][:8] + (2 ** 63).to_bytes(8, "little") + txs[26][16:]   # mintime after maxtime
    for i in (13, 26):
        v1[i], v2[i] = 1, 16
    txs[31] = _non_canonical_s(txs[31])
    v1[31], v2[31] = 1, 21
    at = 28 + int.from_bytes(txs[40][24:28], "little")
    txs[40] = txs[40][: at + 3] + bytes([txs[40][at + 3] ^ 1]) + txs[40][at + 4:]      # R of the signature: still 3
    txs[47] = txs[47][:-3] + bytes([txs[47][-3] ^ 0x55]) + txs[47][-2:]                # a proof byte: still 3
    return txs, bytes(v1), bytes(v2)


@pytest.mark.parametrize("hashing", [0, 1])
@pytest.mark.parametrize("reasons", [0, 1])
def test_a_precompute_call_asks_for_no_stage_and_writes_what_was_constructed(host, oracle, corpus, hashing, reasons):
    txs, v1, v2 = corpus
    n, want = len(txs), (v2 if reasons else v1)
    first = {}
    for k in (0, 8, 4):                                      # no log; every shape fits; the five-entry shapes read the count alone
        for chunk, threads in ((0, 4), (3, 1), (24, 4)):
            rc, bm, st, ids, recs, c = _call(host, txs, hashing, reasons, k, threads=threads, chunk=chunk, seed=3 * k + chunk)
            assert rc == 0 and bm == bytes((n + 7) // 8), (k, chunk)             # the bitmap is written, and all zero
            assert st == want and 0 not in st, (k, chunk, list(st))
            assert c["stage_ops"] == 0 and c["dirty"] == 0
            assert c["precomputed"] == want.count(3)
            on_tape = sum(1 for s in want if s == 3)                           # (a non-canonical s is found before the plan is finished)
            assert (c["host_hashed"], c["device_hashed"]) == ((0, on_tape) if hashing else (n, 0))
            for i, t in enumerate(txs):
                if want[i] != 3:
                    assert ids[i] == bytes(32) and recs[i] == bytes(len(recs[i])), i
                elif k:
                    count = check_accepted(oracle, t, ids[i], recs[i], k)
                    assert count == sum(CORPUS_SHAPES[i % 4])
                    if count > k:
                        assert recs[i] == bytes([count]) + bytes(33 * k)
                else:
                    assert ids[i] == oracle.tx_id(t)[1]
            assert first.setdefault(k, (ids, recs)) == (ids, recs)
    assert first[0][0] == first[8][0] == first[4][0]


def test_the_host_pass_and_the_tape_give_identical_bytes(host, corpus):
    txs = corpus[0]
    a = _call(host, txs, 0, 1, 5, chunk=16)
    b = _call(host, txs, 1, 1, 5, chunk=16, slots=1)
    assert a[:5] == b[:5]


def test_an_error_of_the_stand_in_leaves_one_and_zeros(host, corpus):
    txs, v1, v2 = corpus
    n, failures = len(txs), 0
    for reasons, want in ((0, v1), (1, v2)):
        k = 0
        while True:
            rc, bm, st, ids, recs, c = _call(host, txs, 1, reasons, 5, chunk=16, threads=2, seed=70 + k, hash_fail_at=k)
            assert c["stage_ops"] == 0
            if rc == 0:
                assert st == want
                break
            failures += 1
            assert bm == bytes((n + 7) // 8) and c["dirty"] == 0 and c["precomputed"] == 0
            assert ids == [bytes(32)] * n and recs == [bytes(record_bytes(5))] * n
            assert all(g == 1 or (g == 2 and w == 2) for g, w in zip(st, want)), (k, list(st))
            k += 1
            assert k < 50
        assert k >= 4                                         # four chunks of 16: an enqueue and a collect each, at least
    assert failures >= 8


# ---- 5. the stand-alone sanitizer program ------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_the_side_table_and_the_level_walk_under_sanitizers(tmp_path):
    """tools/tx_precompute_check.cpp: a program of its own (no Python in the process) builds the side table and walks the same
    seven shapes by level, then hands the interpreter a truncated tape, truncated tables and an oversized tape in exact-size
    heap copies, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    r = subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + r.stderr.strip()[-300:])
    exe = tmp_path / "tx_precompute_check"
    subprocess.run([cxx] + flags + ["-I" + os.path.join(ROOT, "zkvm_amd", "csrc"), os.path.join(ROOT, "tools", "tx_precompute_check.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), "5"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok:") and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
