"""ZKGPU_TXFORMAT_RETURN_IDS on the CPU tier: the flag is a constant of the header, mirrored in the Rust declarations and the
Python binding, and came through entry points that exist (no new export, hook or struct, no new ABI version); the scheduler
of a transaction call (csrc/tx_call.hpp) hands back the ID of every accepted transaction and of nothing else, over each of
the three stand-in devices of libzkhost -- IDs hashed by the host VM, by a hashing stage, by a hashing stage whose IDs a
chained signature stage reads in place -- laid out and fail-closed as the library does it (zkhost_txcall_ids_selftest); and
a stand-alone program gives it status arrays of exactly the size the layout asks for under AddressSanitizer.
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

ZERO = bytes(32)
KINDS = (0, 1, 2)                                        # HostTxDevice, HostHashingTxDevice, HostChainingTxDevice


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_flag_is_mirrored_everywhere_and_the_abi_is_what_it_was():
    header = dict((n, int(v)) for n, v in re.findall(r"#define\s+(ZKGPU_[A-Z0-9_]+)\s+(-?\d+)\b", _read("include", "zkgpu.h")))
    rust = dict((n, int(v)) for n, v in re.findall(r"pub const (ZKGPU_[A-Z0-9_]+): c_int = (-?\d+);", _read("rust", "zkgpu-sys", "src", "lib.rs")))
    import zkvm_amd
    from zkvm_amd import native
    from zkvm_amd.verifier import BlockVerifier
    assert header.get("ZKGPU_TXFORMAT_RETURN_IDS") == 1024 == rust.get("ZKGPU_TXFORMAT_RETURN_IDS")
    assert native.TXFORMAT_RETURN_IDS == zkvm_amd.TXFORMAT_RETURN_IDS == BlockVerifier.TXFORMAT_RETURN_IDS == 1024
    wrapper = _read("rust", "zkgpu", "src", "lib.rs")
    assert "sys::ZKGPU_TXFORMAT_RETURN_IDS" in wrapper
    assert "pub fn enable_recollected_tx_format_returning_ids(" in wrapper and "pub fn verify_txs_with_ids(" in wrapper
    from test_capi_symbols import _declared, _hooks_declared
    assert len(_declared()) == 90
    assert len(_hooks_declared()) == 25
    assert "return 3;" in re.search(r"int zkgpu_abi_version\(void\)\s*\{[^}]*\}", _read("zkvm_amd", "csrc", "zkgpu.hip")).group(0)


def test_ids_true_without_the_flag_raises():
    """(no device needed: the wrapper refuses before it calls the library)"""
    from zkvm_amd.verifier import BlockVerifier
    bv = BlockVerifier.__new__(BlockVerifier)
    with pytest.raises(ValueError):
        bv.verify_txs([b"x"], ids=True)
    bv.__dict__["_tx_calls"] = {7: (b"", None, 1, False)}
    with pytest.raises(ValueError):
        bv.wait_txs(7, ids=True)


def _offsets(txs):
    n = len(txs)
    return (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:i + 1]) for i in range(n)]))


def _prepare_txid(host, tx):
    """zkhost_tx_prepare -> the transaction ID, or None where the host VM does not accept the transaction"""
    txid, com, sc, pt = C.create_string_buffer(32), C.create_string_buffer(64 * 32), C.create_string_buffer(32 * 40), C.create_string_buffer(32 * 40)
    a, b, n_sig, po, pl = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    rc = host.zkhost_tx_prepare(tx, C.c_size_t(len(tx)), txid, C.byref(a), C.byref(b), com, C.c_size_t(64 * 32), sc, pt, C.c_size_t(40), C.byref(n_sig),
                                C.byref(po), C.byref(pl))
    return txid.raw if rc == 0 else None


def _ids_call(host, kind, txs, proof_ok, flag=True, split=0, threads=4, chunk=0, seed=1, fail_at=-1, fail_stage=0, slots=2):
    """-> rc, bitmap, status bytes, IDs (a list, or None without the flag), the selftest's counters.  The status arrays are of
    exactly the size the layout asks for."""
    n = len(txs)
    na, nb, per = (split or n), (n - split if split else 0), (33 if flag else 1)
    bm = C.create_string_buffer((n + 7) // 8 + 1)
    sa, sb = C.create_string_buffer(per * na), C.create_string_buffer(max(per * nb, 1))
    out = (C.c_uint64 * 6)()
    rc = host.zkhost_txcall_ids_selftest(C.c_int(kind), C.c_int(int(flag)), C.c_size_t(n), C.c_size_t(split), b"".join(txs), _offsets(txs), proof_ok,
                                         C.c_int(threads), C.c_size_t(chunk), C.c_uint32(seed), C.c_int(fail_at), C.c_int(fail_stage), C.c_int(slots),
                                         bm, sa, sb, out)
    status = sa.raw[:na] + sb.raw[:nb]
    ids = None
    if flag:
        area = sa.raw[na: 33 * na] + sb.raw[nb: 33 * nb]
        ids = [area[32 * i: 32 * i + 32] for i in range(n)]
    names = ("chunks", "leaked", "id_asks", "host_hashed", "device_hashed", "dirty")
    return rc, bm.raw[: (n + 7) // 8], status, ids, dict(zip(names, out))


def _unflagged(host, kind, txs, proof_ok, chunk, threads):
    """the selftest of that kind as it was before the flag existed -> rc, bitmap, status bytes"""
    n = len(txs)
    bm, st = C.create_string_buffer((n + 7) // 8 + 1), C.create_string_buffer(n)
    nc, ns, leaked, hashed, signed = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0), C.c_uint64(0)
    head = (C.c_size_t(n), b"".join(txs), _offsets(txs), proof_ok, C.c_int(threads), C.c_size_t(chunk), C.c_uint32(3), C.c_int(-1))
    if kind == 0:
        rc = host.zkhost_txcall_selftest(*head, bm, st, C.byref(nc), C.byref(ns), C.byref(leaked))
    elif kind == 1:
        rc = host.zkhost_txcall_hashing_selftest(*head, C.c_int(2), bm, st, C.byref(nc), C.byref(leaked), C.byref(hashed))
    else:
        rc = host.zkhost_txcall_chaining_selftest(*head, C.c_int(2), bm, st, C.byref(nc), C.byref(ns), C.byref(leaked), C.byref(hashed), C.byref(signed))
    return rc, bm.raw[: (n + 7) // 8], st.raw


def _block(oracle, n):
    """wrapped payments of the four shapes with a wrong mintime (the signature fails: its ID exists and must be withheld), a
    truncated transaction, a later version (outside the subset) and a proof the stand-in's table rejects"""
    txs = [wrapped(oracle, *SHAPES[k % 4], 900 + k) for k in range(n)]
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
def block100(host, oracle):
    """-> transactions, the proofs' table, expected status bytes, expected IDs (the oracle's AND zkhost_tx_prepare's beside
    status 0, zeros elsewhere)"""
    txs, proof_ok, want = _block(oracle, 100)
    ids = []
    for t, s in zip(txs, want):
        rc, txid, _, _ = oracle.tx_id(t)
        if s == 0:
            assert rc == 0 and txid == _prepare_txid(host, t) and txid != ZERO
        ids.append(txid if s == 0 else ZERO)
    assert _prepare_txid(host, txs[7]) not in (None, ZERO) and _prepare_txid(host, txs[21]) not in (None, ZERO)     # (IDs that exist, withheld)
    return txs, proof_ok, want, ids


@pytest.mark.parametrize("kind", KINDS)
def test_ids_of_accepted_transactions_and_of_nothing_else(host, block100, kind):
    txs, proof_ok, want, ids = block100
    n = len(txs)
    bitmap = bytes(sum((want[8 * b + q] == 0) << q for q in range(8) if 8 * b + q < n) for b in range((n + 7) // 8))
    for chunk in (0, 64, 1):
        for threads in (1, 4):
            plain = _unflagged(host, kind, txs, proof_ok, chunk, threads)
            assert plain == (0, bitmap, want), (chunk, threads)
            rc, bm, st, got, c = _ids_call(host, kind, txs, proof_ok, chunk=chunk, threads=threads, seed=10 * chunk + threads)
            assert (rc, bm, st) == plain, (chunk, threads)
            assert got == ids, (chunk, threads, [i for i in range(n) if got[i] != ids[i]])
            assert c["leaked"] == 0 and c["dirty"] == 0
            chunks = {0: 1, 64: 2, 1: 13}[chunk]
            assert c["chunks"] == chunks
            if kind == 0:                                # the VM's second pass hashed every ID; no device was asked
                assert c["host_hashed"] == n and c["id_asks"] == 0
            else:                                        # the device hashed them, once per chunk it was asked for them, the host hashed none
                assert c["host_hashed"] == 0 and c["device_hashed"] == n - 2 and c["id_asks"] == chunks
            # the same call without the flag, on an array of n bytes: same verdicts; a chaining device is never asked for IDs
            rc, bm, st, none, c = _ids_call(host, kind, txs, proof_ok, flag=False, chunk=chunk, threads=threads)
            assert (rc, bm, st) == plain and none is None
            assert c["id_asks"] == (chunks if kind == 1 else 0)


@pytest.mark.parametrize("kind", KINDS)
def test_two_callers_in_one_merged_call_have_an_id_area_each(host, block100, kind):
    txs, proof_ok, want, ids = block100
    for split, chunk in ((72, 0), (8, 64), (40, 1)):
        rc, bm, st, got, c = _ids_call(host, kind, txs, proof_ok, split=split, chunk=chunk, slots=1)
        assert rc == 0 and st == want and got == ids, (split, chunk)
        assert c["leaked"] == 0 and c["host_hashed"] == (len(txs) if kind == 0 else 0)


@pytest.mark.parametrize("kind", KINDS)
def test_an_error_at_any_operation_of_any_stage_leaves_no_id(host, oracle, kind):
    """fail_at walks over every operation of every stage the stand-in has (0: keys, proofs, unchained signatures; 1: the hashing
    stage; 2: the chained signature stage), for a lone call of two chunks and for a merged one: an error return always leaves
    an all-zero ID area -- and had left it all-zero before the caller fail-closed it --, a zero bitmap and status 1 or 2 (2 only
    beside the transaction outside the subset, and only if the call had looked at it before it failed)"""
    txs, proof_ok, want = _block(oracle, 24)
    n = len(txs)
    ids = [oracle.tx_id(t)[1] if s == 0 else ZERO for t, s in zip(txs, want)]
    failures = 0
    for stage in range(kind + 1):
        for split in (0, 16):
            k = 0
            while True:
                rc, bm, st, got, c = _ids_call(host, kind, txs, proof_ok, split=split, chunk=16, threads=2, seed=50 + k, fail_at=k, fail_stage=stage)
                assert c["leaked"] == 0, (stage, split, k)
                if rc == 0:
                    assert st == want and got == ids, (stage, split, k)
                    break
                failures += 1
                assert got == [ZERO] * n and c["dirty"] == 0, (stage, split, k)
                assert bm == bytes((n + 7) // 8), (stage, split, k)
                # (1 everywhere inside the subset; outside it 2 if the staging thread had reached the transaction when the call
                # failed, else still 1 -- never a 0, and never a 2 beside a transaction inside the subset)
                assert all(g == 1 or (g == 2 and s == 2) for g, s in zip(st, want)), (stage, split, k, list(st))
                k += 1
                assert k < 200
            assert k >= 4, (stage, split, k)             # an enqueue and a collect per chunk could fail, at the least
    assert failures >= 8 * (kind + 1)


@pytest.mark.timeout(900)
def test_no_write_past_a_status_array_of_exactly_the_size_the_layout_asks_for(tmp_path):
    """tools/tx_ids_overrun_check.cpp: a program of its own (no Python in the process) drives TxCall over the three stand-in
    devices with heap arrays of exactly batch bytes without the flag and 33 * batch with it, for a lone call and for two
    merged pieces, clean and with a fault at every operation, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    r = subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + r.stderr.strip()[-300:])
    exe = tmp_path / "tx_ids_overrun_check"
    subprocess.run([cxx] + flags + [os.path.join(ROOT, "tools", "tx_ids_overrun_check.cpp"), os.path.join(ROOT, "zkvm_amd", "csrc", "hostlib.cpp"),
                                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok:") and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
