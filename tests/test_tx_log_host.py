"""ZKGPU_TXFORMAT_RETURN_LOG on the CPU tier: the constants are in the header, the Rust declarations and the Python binding,
and came through entry points that exist (90 exports, 25 hooks, ABI 3); the scheduler of
a transaction call (csrc/tx_call.hpp) hands back the Input / Output entries of every accepted transaction's log and of
nothing else over each of the three stand-in devices of libzkhost -- records filled by the host VM's second pass, by a
hashing stage whose gather is the kernel's own code (csrc/tx_log.hpp: tx_log_gather_lane), by the same behind a chained
signature stage -- laid out and fail-closed as the library does it (zkhost_txcall_log_selftest); and a stand-alone program
gives it status arrays of exactly the size the layout asks for under AddressSanitizer; the second pass that fills the records
on the host (tx_prepare_many_logged) leaves the statements tx_prepare_many leaves.

NOT tested here: the validity table of the format value.  zkgpu_verifier_set_tx_format needs a verifier, and a verifier needs
a device, so the table below (valid_formats / INVALID_FORMATS) is only DATA on this tier; tests/test_gpu_tx_log.py::
test_format_values holds the library against it.

What pins a record needs nothing new in the oracle (tests/tx_log_util.py): the transaction ID is the Merkle root over the
header and the entries, so the root recomputed from a record must be oracle.tx_id's; and an input's ID is the contract ID of
the contract its program pushed.
"""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_tx_hash_tape import SHAPES, host, wrapped  # noqa: E402,F401
from tx_log_util import area_bytes, check_accepted, record_bytes, split_area  # noqa: E402

KINDS = (0, 1, 2)                                        # HostTxDevice, HostHashingTxDevice, HostChainingTxDevice
ENTRIES = [a + b for a, b in SHAPES]                     # log entries of the four shapes
GUARD = 64


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_constants_are_mirrored_everywhere_and_the_abi_is_what_it_was():
    header = dict((n, int(v)) for n, v in re.findall(r"#define\s+(ZKGPU_[A-Z0-9_]+)\s+(-?\d+)\b", _read("include", "zkgpu.h")))
    rust = dict((n, int(v)) for n, v in re.findall(r"pub const (ZKGPU_[A-Z0-9_]+): c_int = (-?\d+);", _read("rust", "zkgpu-sys", "src", "lib.rs")))
    import zkvm_amd
    from zkvm_amd import native
    from zkvm_amd.verifier import BlockVerifier
    want = {"ZKGPU_TXFORMAT_RETURN_LOG": 2048, "ZKGPU_TXFORMAT_LOG_SHIFT": 16, "ZKGPU_TXLOG_INPUT": 1, "ZKGPU_TXLOG_OUTPUT": 2}
    for name, value in want.items():
        short = name[len("ZKGPU_"):]
        assert header.get(name) == value == rust.get(name), name
        assert getattr(native, short) == getattr(zkvm_amd, short) == getattr(BlockVerifier, short) == value, name
    wrapper = _read("rust", "zkgpu", "src", "lib.rs")
    assert "sys::ZKGPU_TXFORMAT_RETURN_LOG" in wrapper and "pub enum TxLogEntry" in wrapper
    assert "pub fn enable_recollected_tx_format_returning_log(" in wrapper and "pub fn verify_txs_with_log(" in wrapper
    from test_capi_symbols import _declared, _hooks_declared
    assert len(_declared()) == 90
    assert len(_hooks_declared()) == 25
    assert "return 3;" in re.search(r"int zkgpu_abi_version\(void\)\s*\{[^}]*\}", _read("zkvm_amd", "csrc", "zkgpu.hip")).group(0)


def valid_formats():
    """every value valid before the flag existed, and each of those with 0x400 also with 0x800 | K << 16 for K in 1, 4, 255"""
    old = [0] + [base | hs | f for base in (1, 2) for hs in (0, 0x100, 0x300) for f in (0, 0x400)]
    return old + [fmt | 0x800 | (k << 16) for fmt in old if fmt & 0x400 for k in (1, 4, 255)]


INVALID_FORMATS = [0x801, 0x1401, 0xC01, 1 | (4 << 16), 0xC01 | (4 << 16) | 0x1000, 0xC01 | (1 << 24),
                   0x400, 0x403, 0x600, 0x601, 0x800 | (4 << 16), 0x801 | (4 << 16), 0xC00 | (4 << 16), 0xE01 | (4 << 16), 0xC01 | (4 << 16) | 0x8000,
                   0xC01 | (4 << 16) | (1 << 30), -1]


def test_log_true_without_the_flag_raises():
    """(no device needed: the wrapper refuses before it calls the library)"""
    from zkvm_amd.verifier import BlockVerifier
    bv = BlockVerifier.__new__(BlockVerifier)
    with pytest.raises(ValueError):
        bv.verify_txs([b"x"], log=True)
    bv._tx_return_ids = True                             # (0x400 alone is not enough)
    with pytest.raises(ValueError):
        bv.verify_txs([b"x"], log=True)
    bv.__dict__["_tx_calls"] = {7: (b"", None, 1, True, 0), 8: (b"", None, 1, True)}
    for cid in (7, 8):
        with pytest.raises(ValueError):
            bv.wait_txs(cid, log=True)
    with pytest.raises(ValueError):                      # (a window in the format AND as log_k: refused before the library is called)
        bv.set_tx_format(0x402 | 0x800 | (4 << 16), log_k=5)
    with pytest.raises(ValueError):
        bv.set_tx_format(0x402 | (4 << 16), log_k=4)
    with pytest.raises(ValueError):
        bv.set_tx_format(0x402, log_k=256)
    assert BlockVerifier._tx_status_bytes(10, False, 0) == 10 and BlockVerifier._tx_status_bytes(10, True, 0) == 330
    assert BlockVerifier._tx_status_bytes(10, True, 4) == area_bytes(10, 4) == 10 * (33 + 1 + 132)


def test_a_saturated_count_reads_as_a_number_not_as_entries():
    """count saturates at 255: under K = 255 a record of 255 with zero kinds means "255 or more, not listed", and the decoder
    must not hand back 255 entries of kind 0 (a listed entry never has kind 0)"""
    import ctypes
    from zkvm_amd.verifier import BlockVerifier
    bv = BlockVerifier.__new__(BlockVerifier)
    k, one = 255, bytes([7]) * 32
    listed = bytes([2, 1, 2]) + bytes(k - 2) + one + one + bytes(32 * (k - 2))
    saturated = bytes([255]) + bytes(33 * k)
    raw = bytes(3) + bytes(32 * 3) + listed + saturated + bytes(record_bytes(k))
    st = ctypes.create_string_buffer(raw, len(raw))
    bm = ctypes.create_string_buffer(b"\x07", 1)
    out = bv._tx_result(bm, st, 3, True, False, k, True)
    assert out[3] == [[("input", one), ("output", one)], 255, []]


def test_the_logged_second_pass_leaves_the_statements_of_the_plain_one(host, oracle):
    """tx_prepare_many_logged and tx_prepare_many are two sets of parameters of one second pass (zkvm_tx.hpp: tx_run_group);
    this guards what must not differ between them: both over the same groups of eight, statement by statement -- groups of one shape (hashed in lockstep where the
    CPU can) and mixed ones, with a truncated transaction and one outside the subset among them"""
    host.zkhost_tx_prepare_logged_compare.restype = C.c_longlong
    uniform = [wrapped(oracle, 2, 2, 2100 + k) for k in range(24)] + [wrapped(oracle, 3, 2, 2200 + k) for k in range(8)]
    mixed = [wrapped(oracle, *SHAPES[k % 4], 2300 + k) for k in range(29)]
    mixed[5] = mixed[5][:-1]
    t = bytearray(mixed[9]); t[0] = 2; mixed[9] = bytes(t)
    for txs, lockstep in ((uniform, 4), (mixed, 0), (uniform[:3] + mixed, None)):
        groups = C.c_uint64(99)
        for k in (1, 4, 255):
            assert host.zkhost_tx_prepare_logged_compare(b"".join(txs), _offsets(txs), C.c_size_t(len(txs)), C.c_size_t(k), C.byref(groups)) == 0
        if lockstep is not None:
            assert groups.value == lockstep


def _offsets(txs):
    n = len(txs)
    return (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:i + 1]) for i in range(n)]))


def _log_call(host, kind, txs, proof_ok, k, k_b=0, split=0, threads=4, chunk=0, seed=1, fail_at=-1, fail_stage=0, slots=2):
    """-> rc, bitmap, status bytes, ids, records (each with the window of its caller), counters.  The status arrays are of
    exactly the size the layout asks for plus GUARD bytes, which must come back untouched."""
    n = len(txs)
    na, nb = (split or n), (n - split if split else 0)
    kb = k_b or k
    bm = C.create_string_buffer((n + 7) // 8 + 1)
    sa = C.create_string_buffer(b"\xa5" * (area_bytes(na, k) + GUARD), area_bytes(na, k) + GUARD)
    sb = C.create_string_buffer(b"\xa5" * (area_bytes(nb, kb) + GUARD), area_bytes(nb, kb) + GUARD)
    out = (C.c_uint64 * 6)()
    rc = host.zkhost_txcall_log_selftest(C.c_int(kind), C.c_size_t(k), C.c_size_t(k_b), C.c_size_t(n), C.c_size_t(split), b"".join(txs), _offsets(txs),
                                         proof_ok, C.c_int(threads), C.c_size_t(chunk), C.c_uint32(seed), C.c_int(fail_at), C.c_int(fail_stage),
                                         C.c_int(slots), bm, sa, sb, out)
    assert sa.raw[area_bytes(na, k):] == b"\xa5" * GUARD and sb.raw[area_bytes(nb, kb):] == b"\xa5" * GUARD, "guard bytes overwritten"
    st_a, ids_a, rec_a = split_area(sa.raw, na, k)
    st_b, ids_b, rec_b = split_area(sb.raw, nb, kb)
    names = ("chunks", "leaked", "host_hashed", "device_hashed", "device_logged", "dirty")
    return rc, bm.raw[: (n + 7) // 8], st_a + st_b, ids_a + ids_b, rec_a + rec_b, dict(zip(names, out))


def _block(oracle, n):
    """wrapped payments of the four shapes (2, 4, 5, 5 log entries) with a wrong mintime (the signature fails: its entries
    exist and must be withheld), a truncated transaction, a later version (outside the subset) and a proof the stand-in's
    table rejects"""
    txs = [wrapped(oracle, *SHAPES[k % 4], 1300 + k) for k in range(n)]
    txs[7] = txs[7][:8] + b"\x00" * 8 + txs[7][16:]
    txs[13] = txs[13][:-1]
    t = bytearray(txs[18]); t[0] = 2; txs[18] = bytes(t)
    proof_ok = bytearray([1] * n)
    proof_ok[21] = 0
    want = bytearray(n)
    want[7] = want[13] = want[21] = 1
    want[18] = 2
    return txs, bytes(proof_ok), bytes(want)


@pytest.fixture(scope="module")
def block60(oracle):
    return _block(oracle, 60)


def _check_records(oracle, txs, want, ids, recs, windows):
    """every record beside status 0 passes the Merkle check and the input check (or, past its window, reads the count alone);
    every other record is all zero"""
    for i, t in enumerate(txs):
        k = windows[i]
        if want[i] == 0:
            assert check_accepted(oracle, t, ids[i], recs[i], k) == ENTRIES[i % 4], i
        else:
            assert recs[i] == bytes(record_bytes(k)) and ids[i] == bytes(32), i


@pytest.mark.parametrize("kind", KINDS)
def test_records_of_accepted_transactions_and_of_nothing_else(host, oracle, block60, kind):
    """K = 5: the five-entry shapes fit exactly; K = 8: zero padding; K = 4: they read count = 5 and nothing else"""
    txs, proof_ok, want = block60
    n = len(txs)
    bitmap = bytes(sum((want[8 * b + q] == 0) << q for q in range(8) if 8 * b + q < n) for b in range((n + 7) // 8))
    first = {}
    for k in (5, 8, 4):
        for chunk, threads in ((0, 4), (3, 1), (24, 4), (0, 1)):          # (chunk 3: cut to multiples of eight -- and a remainder)
            rc, bm, st, ids, recs, c = _log_call(host, kind, txs, proof_ok, k, chunk=chunk, threads=threads, seed=7 * k + chunk)
            assert (rc, bm, st) == (0, bitmap, want), (k, chunk, threads)
            assert c["leaked"] == 0 and c["dirty"] == 0
            _check_records(oracle, txs, want, ids, recs, [k] * n)
            if k == 4:
                assert all(recs[i][0] == 5 and recs[i][1:] == bytes(33 * 4) for i in range(n) if want[i] == 0 and ENTRIES[i % 4] == 5)
            assert first.setdefault(k, (ids, recs)) == (ids, recs), (k, chunk, threads)
            hashed = [i for i in range(n) if want[i] != 2 and i != 13]     # what reaches the second pass: the tape's transactions
            if kind == 0:
                assert c["host_hashed"] == n and c["device_logged"] == 0
            else:
                assert c["host_hashed"] == 0 and c["device_hashed"] == len(hashed)
                assert c["device_logged"] == sum(ENTRIES[i % 4] for i in hashed if ENTRIES[i % 4] <= k)
    # the entries do not depend on the window: K = 8 is K = 5 with zero padding
    assert [r[0] for r in first[5][1]] == [r[0] for r in first[8][1]]


def test_the_three_stand_ins_return_identical_bytes(host, block60):
    txs, proof_ok, _ = block60
    got = [_log_call(host, kind, txs, proof_ok, 5, chunk=16, seed=3)[1:5] for kind in KINDS]
    assert got[0] == got[1] == got[2]


@pytest.mark.parametrize("kind", KINDS)
def test_two_callers_in_one_merged_call_have_an_area_and_a_window_each(host, oracle, block60, kind):
    txs, proof_ok, want = block60
    n = len(txs)
    for split, chunk, k, k_b in ((40, 0, 5, 0), (8, 24, 8, 4), (24, 3, 4, 8)):
        rc, bm, st, ids, recs, c = _log_call(host, kind, txs, proof_ok, k, k_b=k_b, split=split, chunk=chunk, slots=1)
        assert rc == 0 and st == want and c["leaked"] == 0, (split, chunk)
        _check_records(oracle, txs, want, ids, recs, [k] * split + [k_b or k] * (n - split))


@pytest.mark.parametrize("kind", KINDS)
def test_an_error_at_any_operation_of_any_stage_leaves_no_record(host, oracle, kind):
    """fail_at walks over every operation of every stage the stand-in has, for a lone call of two chunks and for a merged one:
    an error return always leaves all-zero ID and record areas -- and had left them all-zero before the caller fail-closed them
    --, a zero bitmap and status 1 or 2"""
    txs, proof_ok, want = _block(oracle, 24)
    n = len(txs)
    failures = 0
    for stage in range(kind + 1):
        for split in (0, 16):
            k = 0
            while True:
                rc, bm, st, ids, recs, c = _log_call(host, kind, txs, proof_ok, 5, split=split, chunk=16, threads=2, seed=50 + k, fail_at=k, fail_stage=stage)
                assert c["leaked"] == 0, (stage, split, k)
                if rc == 0:
                    assert st == want, (stage, split, k)
                    _check_records(oracle, txs, want, ids, recs, [5] * n)
                    break
                failures += 1
                assert ids == [bytes(32)] * n and recs == [bytes(record_bytes(5))] * n and c["dirty"] == 0, (stage, split, k)
                assert bm == bytes((n + 7) // 8), (stage, split, k)
                assert all(g == 1 or (g == 2 and s == 2) for g, s in zip(st, want)), (stage, split, k, list(st))
                k += 1
                assert k < 200
            assert k >= 4, (stage, split, k)
    assert failures >= 8 * (kind + 1)


@pytest.mark.timeout(900)
def test_no_write_past_a_status_array_of_exactly_the_size_the_layout_asks_for(tmp_path):
    """tools/tx_log_overrun_check.cpp: a program of its own (no Python in the process) drives TxCall over the three stand-in
    devices with heap arrays of exactly batch * (33 + 1 + 33 K) bytes, for a lone call and for two merged pieces with windows
    of their own, clean and with a fault at every operation, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    r = subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + r.stderr.strip()[-300:])
    exe = tmp_path / "tx_log_overrun_check"
    subprocess.run([cxx] + flags + [os.path.join(ROOT, "tools", "tx_log_overrun_check.cpp"), os.path.join(ROOT, "zkvm_amd", "csrc", "hostlib.cpp"),
                                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok:") and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
