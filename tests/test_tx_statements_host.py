"""ZKGPU_TXFORMAT_STATEMENTS_V1 (4, and 4 | 0x200) on the CPU tier: upstream's PrecomputedTx::verify behind the caller's own VM.

  1. the format word: decoding over the full cross product (csrc/tx_out.hpp through zkhost_tx_out_layout), the constants
     mirrored, the ABI what it was;
  2. the parser (csrc/tx_statements.hpp) against this file's own model of the framing, every buffer followed by guard bytes;
  3. musig_row (csrc/tx_musig_rows.hpp), the function k_musig_rows runs per lane, against coefficients computed with the
     oracle's Merlin transcript; the recipe recorded for the device against the VM's plan; the host's eight-wide jobs;
  4. the scheduler (csrc/tx_call.hpp: step_statements) on the stand-in device of hostlib.cpp, both modes;
  5. tools/tx_statements_check.cpp, a program of its own under AddressSanitizer / UndefinedBehaviorSanitizer and under
     ThreadSanitizer.
"""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess

import pytest

from test_tx_hash_tape import SHAPES, built, wrapped
from tx_statements_util import L, Signer, bits, csr, fields_of_payment, musig_coefficients, pack, record_of_payment, signature_holds, u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATEMENTS, SIGN = 4, 0x200
KEY_COUNTS = list(range(1, 18)) + [32, 64]
GUARD = b"\xa5" * 64


@pytest.fixture(scope="module")
def host():
    from zkvm_amd.build import build, HOST_OUT
    build()
    return C.CDLL(HOST_OUT)


# ---------------------------------------------------------------- 1. the format word
def _decode(host, word):
    out = (C.c_int64 * 7)()
    assert host.zkhost_tx_out_layout(0, (C.c_int64 * 1)(word), None, None, None, None, out) == 0
    return list(out)


def test_base_4_takes_the_signing_flag_alone(host):
    valid = []
    for hash_ in (0, 0x100):
        for sign in (0, 0x200):
            for ids in (0, 0x400):
                for log in (0, 0x800):
                    for pre in (0, 0x2000):
                        for k in (0, 1, 255):
                            word = STATEMENTS | hash_ | sign | ids | log | pre | (k << 16)
                            got = _decode(host, word)
                            if got[0]:
                                valid.append(word)
                                assert got == [1, 4, 0, int(bool(sign)), 0, 0, 0], hex(word)
    assert valid == [4, 0x204]
    # what was invalid stays invalid, what was valid decodes as it did
    for word in (3, 5, 6, 7, 8, 0x200, 0x201, 0x202, 0x300, 0x100, 0x400, 0x2000, 0x2401 | 0x200, 0x801, 0x10401, -1, 3 | 0x100, 4 | 0x1000, 4 | 0x4000, 4 | (1 << 24)):
        assert _decode(host, word)[0] == 0, hex(word)
    assert _decode(host, 0) == [1, 0, 0, 0, 0, 0, 0]
    assert _decode(host, 0x301) == [1, 1, 1, 1, 0, 0, 0] and _decode(host, 0x102) == [1, 2, 1, 0, 0, 0, 0]
    assert _decode(host, 0x2401) == [1, 1, 0, 0, 1, 0, 1] and _decode(host, 2 | 0x400 | 0x800 | (7 << 16)) == [1, 2, 0, 0, 1, 7, 0]


def test_the_constant_is_mirrored_everywhere_and_the_abi_is_what_it_was():
    from test_capi_symbols import _declared, _hooks_declared
    read = lambda *p: open(os.path.join(ROOT, *p)).read()      # noqa: E731
    header = dict((n, int(v)) for n, v in re.findall(r"#define\s+(ZKGPU_[A-Z0-9_]+)\s+(-?\d+)\b", read("include", "zkgpu.h")))
    rust = dict((n, int(v)) for n, v in re.findall(r"pub const (ZKGPU_[A-Z0-9_]+): c_int = (-?\d+);", read("rust", "zkgpu-sys", "src", "lib.rs")))
    assert header["ZKGPU_TXFORMAT_STATEMENTS_V1"] == rust["ZKGPU_TXFORMAT_STATEMENTS_V1"] == STATEMENTS
    import zkvm_amd
    from zkvm_amd import native
    from zkvm_amd.verifier import BlockVerifier
    assert native.TXFORMAT_STATEMENTS_V1 == zkvm_amd.TXFORMAT_STATEMENTS_V1 == BlockVerifier.TXFORMAT_STATEMENTS_V1 == STATEMENTS
    wrapper = read("rust", "zkgpu", "src", "lib.rs")
    assert "sys::ZKGPU_TXFORMAT_STATEMENTS_V1" in wrapper and "pub fn verify_precomputed(" in wrapper
    assert len(_declared()) == 90 and len(_hooks_declared()) == 25
    assert "int zkgpu_abi_version(void) { return 3; }" in read("zkvm_amd", "csrc", "zkgpu.hip")
    assert "the framing is this library's own" in read("include", "zkgpu.h").lower().replace("\n * ", " ")


def test_pack_statement_is_the_framing_and_the_wrapper_refuses_before_it_calls_the_library():
    import zkvm_amd
    from zkvm_amd.verifier import BlockVerifier
    f = dict(txid=b"\x01" * 32, R=b"\x02" * 32, s=b"\x03" * 32, keys=[b"\x04" * 32, b"\x05" * 32], n_in=1, n_out=2, commitments=b"\x06" * 192, proof=b"\x07" * 9)
    assert zkvm_amd.pack_statement(**f) == pack(**f)
    for bad in (dict(f, txid=b"\x01" * 31), dict(f, keys=[b"\x04" * 33]), dict(f, commitments=b"\x06" * 191), dict(f, n_in=2)):
        with pytest.raises(ValueError):
            zkvm_amd.pack_statement(**bad)
    bv = BlockVerifier.__new__(BlockVerifier)                 # (no library behind it: a call that got through would raise AttributeError)
    for bad in (b"one record, not a list", "text", [b"ok", "text"], [None], 7):
        with pytest.raises(TypeError):
            bv.verify_statements(bad)
        with pytest.raises(TypeError):
            bv.submit_statements(bad, on_device=True)


# ---------------------------------------------------------------- 2. the parser
def _parse(host, rec):
    buf = C.create_string_buffer(rec + GUARD, len(rec) + len(GUARD))
    u = (C.c_uint32 * 5)()
    why = C.create_string_buffer(64 + 64)
    txid = C.create_string_buffer(bytes(32) + GUARD, 96)
    cap_com, cap_terms = 64 * 128, 66
    com = C.create_string_buffer(bytes(cap_com) + GUARD, cap_com + 64)
    sc = C.create_string_buffer(bytes(32 * cap_terms) + GUARD, 32 * cap_terms + 64)
    pt = C.create_string_buffer(bytes(32 * cap_terms) + GUARD, 32 * cap_terms + 64)
    status = host.zkhost_tx_statement_parse(buf, C.c_size_t(len(rec)), u, why, txid, com, C.c_size_t(cap_com), sc, pt, C.c_size_t(cap_terms))
    assert buf.raw[len(rec):] == GUARD and txid.raw[32:] == GUARD and com.raw[cap_com:] == GUARD and sc.raw[32 * cap_terms:] == GUARD and pt.raw[32 * cap_terms:] == GUARD
    return dict(status=status, n_in=u[0], n_out=u[1], terms=u[2], proof_at=u[3], proof_len=u[4], why=why.value.decode(), txid=txid.raw[:32],
                com=com.raw[:cap_com], sc=sc.raw[: 32 * cap_terms], pt=pt.raw[: 32 * cap_terms])


def _model(rec):
    """-> (status, reason code) of a record by this file's reading of the framing: 0 ok, 16, 21, 2"""
    if len(rec) < 96:
        return 16
    if int.from_bytes(rec[64:96], "little") >= L:
        return 21
    at = 96
    rd = lambda: int.from_bytes(rec[at: at + 4], "little")      # noqa: E731
    if len(rec) < at + 4:
        return 16
    k = rd(); at += 4
    if k == 0 or len(rec) < at + 32 * k + 8:
        return 16
    at += 32 * k
    n_in = rd(); at += 4
    n_out = rd(); at += 4
    if len(rec) < at + 64 * (n_in + n_out) + 4:
        return 16
    at += 64 * (n_in + n_out)
    p = rd(); at += 4
    if len(rec) != at + p:
        return 16
    if k > 64 or not 1 <= n_in <= 64 or not 1 <= n_out <= 64:
        return 2
    return 0


def _fields(k=1, n_in=1, n_out=1, s=None, p=5, tag=b"f"):
    h = lambda t, n: hashlib.shake_256(tag + t).digest(n)      # noqa: E731
    return dict(txid=h(b"id", 32), R=h(b"R", 32), s=(s if s is not None else (L - 1 - k)).to_bytes(32, "little"), keys=[h(b"k%d" % i, 32) for i in range(k)],
                n_in=n_in, n_out=n_out, commitments=h(b"com", 64 * (n_in + n_out)), proof=h(b"proof", p))


CODE = {16: (1, "record malformed"), 21: (1, "signature scalar not canonical"), 2: (2, None)}


def _check_against_model(host, rec, f=None):
    got, want = _parse(host, rec), _model(rec)
    if want:
        assert got["status"] == CODE[want][0] and (CODE[want][1] is None or got["why"] == CODE[want][1]), (want, got["status"], got["why"])
        assert got["terms"] == 0 and got["proof_len"] == 0 and got["n_in"] == 0 and got["txid"] == bytes(32)
        return want
    assert got["status"] == 0 and f is not None
    k = len(f["keys"])
    assert (got["n_in"], got["n_out"], got["terms"], got["proof_len"]) == (f["n_in"], f["n_out"], 2 + k, len(f["proof"]))
    assert got["txid"] == f["txid"] and got["com"][: len(f["commitments"])] == f["commitments"]
    assert rec[got["proof_at"]: got["proof_at"] + got["proof_len"]] == f["proof"]
    # term 0 = (s, B: filled in later), term 1 = (-1, R), terms 2.. = (a_i: not hashed by the parser, X_i)
    assert got["sc"][: 32 * (2 + k)] == f["s"] + (L - 1).to_bytes(32, "little") + bytes(32 * k)
    assert got["pt"][32: 32 * (2 + k)] == f["R"] + b"".join(f["keys"])
    return 0


def test_the_parser_against_the_model(host):
    f = _fields(k=2, n_in=2, n_out=3, p=40)
    assert _check_against_model(host, pack(**f), f) == 0
    one = _fields()
    rec = pack(**one)
    assert [_check_against_model(host, rec[:cut]) for cut in range(len(rec))] == [16] * len(rec)      # every truncation point of a 1 x 1 record
    assert _check_against_model(host, rec + b"\x00") == 16                                                # a trailing byte
    for k, want in ((0, 16), (1, 0), (64, 0), (65, 2)):
        f = _fields(k=k, tag=b"k%d" % k)
        assert _check_against_model(host, pack(**f), f) == want, k
    for n_in, n_out, want in ((0, 1, 2), (1, 0, 2), (64, 1, 0), (1, 64, 0), (64, 64, 0), (65, 1, 2), (1, 65, 2), (0, 0, 2)):
        f = _fields(n_in=n_in, n_out=n_out, tag=b"n%d %d" % (n_in, n_out))
        assert _check_against_model(host, pack(**f), f) == want, (n_in, n_out)
    f = _fields(s=L - 1)
    assert _check_against_model(host, pack(**f), f) == 0
    assert _check_against_model(host, pack(**_fields(s=L))) == 21
    assert _check_against_model(host, pack(**_fields(s=2 ** 256 - 1))) == 21
    # s is looked at before the rest of the record: not canonical beside k = 0 and beside a count the library does not serve
    assert _check_against_model(host, pack(**_fields(k=0, s=L))) == 21 and _check_against_model(host, pack(**_fields(k=65, s=L))) == 21
    rec = pack(**one)
    for p in (len(one["proof"]) + 1, 2 ** 32 - 1, 2 ** 31):                                              # a p that overruns
        assert _check_against_model(host, rec[: -len(one["proof"]) - 4] + u32(p) + one["proof"]) == 16
    big = pack(**dict(one, keys=[]))                                                                      # counts that overrun: k, n_in, n_out of 2^32 - 1
    assert _check_against_model(host, big[:96] + u32(2 ** 32 - 1) + big[100:]) == 16
    assert _check_against_model(host, rec[:132] + u32(2 ** 32 - 1) + rec[136:]) == 16 and _check_against_model(host, rec[:136] + u32(2 ** 32 - 1) + rec[140:]) == 16


# ---------------------------------------------------------------- 3. musig_row, the recipe, the host's jobs
def _musig_rows(host, rows, skip):
    """rows: lists of keys -> (per row the coefficients musig_row wrote, the trace)"""
    pts = b"".join((b"\x11" * 32) * skip + b"".join(keys) for keys in rows)
    offs = [0]
    for keys in rows:
        offs.append(offs[-1] + skip + len(keys))
    sc = C.create_string_buffer(b"\xee" * (32 * offs[-1]) + GUARD, 32 * offs[-1] + 64)
    tr = (C.c_uint32 * 3)()
    assert host.zkhost_musig_rows(sc, pts + GUARD, (C.c_uint64 * len(offs))(*offs), C.c_size_t(len(rows)), C.c_uint32(skip), tr) == 0
    assert sc.raw[32 * offs[-1]:] == GUARD
    out = []
    for r, keys in enumerate(rows):
        assert sc.raw[32 * offs[r]: 32 * (offs[r] + skip)] == b"\xee" * (32 * skip)      # (the leading terms are not touched)
        out.append(sc.raw[32 * (offs[r] + skip): 32 * offs[r + 1]])
    return out, list(tr)


@pytest.mark.parametrize("skip", [0, 1])
def test_musig_row_against_the_oracles_transcript(host, oracle, skip):
    """every k from 1 to 17, then 32 and 64, as rows of one stage.  At 41 absorbed bytes per key against a rate of 166 these counts
    put the rate boundary inside an operation header, inside a label and its length, and inside a key: asserted from the
    function's own position counter"""
    rows = [[hashlib.sha256(b"musig %d %d" % (k, i)).digest() for i in range(k)] for k in KEY_COUNTS]
    got, trace = _musig_rows(host, rows, skip)
    for keys, g in zip(rows, got):
        assert g == b"".join(a.to_bytes(32, "little") for a in musig_coefficients(keys)), len(keys)
    assert all(t >= 1 for t in trace), trace
    # a row's coefficients do not depend on its neighbours or its place
    alone, _ = _musig_rows(host, [rows[5]], skip)
    assert alone[0] == got[5]


def test_the_recipe_recorded_for_the_device_is_the_vms_plan(host, oracle):
    host.zkhost_musig_recipe_compare.restype = C.c_longlong
    for n_in, n_out in SHAPES:
        tx = wrapped(oracle, n_in, n_out, 70 + n_in)
        assert host.zkhost_musig_recipe_compare(tx, C.c_size_t(len(tx))) == n_in
    assert host.zkhost_musig_recipe_compare(tx[:-1], C.c_size_t(len(tx) - 1)) == -2


@pytest.mark.parametrize("lockstep", [0, 1])
def test_the_hosts_jobs_give_the_oracles_coefficients(host, oracle, lockstep):
    """eight records of three keys (one shape: hashed eight-wide where the CPU can), then a mixed group with a refused record"""
    for ks in ([3] * 8, [1, 2, 17, 64, 0, 2, 2, 5]):
        fs = [_fields(k=k, tag=b"g%d %d" % (i, k)) for i, k in enumerate(ks)]
        blob, offs = csr([pack(**f) for f in fs])
        status, sc = C.create_string_buffer(8), C.create_string_buffer(32 * 66 * 8)
        host.zkhost_tx_statements_group(blob, offs, C.c_size_t(8), C.c_int(lockstep), status, sc)
        for i, f in enumerate(fs):
            k = len(f["keys"])
            assert status.raw[i] == (0 if k else 1)
            if k:
                want = f["s"] + (L - 1).to_bytes(32, "little") + b"".join(a.to_bytes(32, "little") for a in musig_coefficients(f["keys"]))
                assert sc.raw[32 * 66 * i: 32 * 66 * i + len(want)] == want, (i, k)


# ---------------------------------------------------------------- 4. the scheduler on the stand-in
@pytest.fixture(scope="module")
def corpus(oracle):
    """100 records of signed payments of the four shapes, some damaged -> (records, proof_ok, expected status bytes)"""
    txs = [wrapped(oracle, *SHAPES[k % 4], 800 + k) for k in range(100)]
    fs = [fields_of_payment(oracle, t) for t in txs]
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]      # noqa: E731
    fs[3]["txid"] = flip(fs[3]["txid"], 0)
    fs[10]["keys"] = fs[10]["keys"][::-1]                    # (2 x 2: two keys, permuted)
    fs[17]["s"] = ((int.from_bytes(fs[17]["s"], "little") + 1) % L).to_bytes(32, "little")
    fs[21]["keys"][0] = b"\xff" * 32                         # no encoding
    fs[33]["R"] = b"\xff" * 32
    fs[40]["s"] = L.to_bytes(32, "little")
    recs = [pack(**f) for f in fs]
    recs[50] = recs[50][:-1]
    recs[61] = pack(**dict(fs[61], n_in=65, commitments=bytes(64 * (65 + fs[61]["n_out"]))))
    proof_ok = bytearray([1] * 100)
    proof_ok[8] = proof_ok[21] = 0
    want = []
    for i, rec in enumerate(recs):
        m = _model(rec)
        if m:
            want.append(m)
            continue
        sig = signature_holds(oracle, fs[i]["txid"], fs[i]["R"], fs[i]["s"], fs[i]["keys"])
        want.append(19 if not proof_ok[i] else 20 if sig == "key" else 21 if sig == "signature" else 0)
    assert [want[i] for i in (3, 8, 10, 17, 21, 33, 40, 50, 61)] == [21, 19, 21, 21, 19, 21, 21, 16, 2] and want.count(0) == 91
    return recs, bytes(proof_ok), bytes(want)


def _call(host, recs, proof_ok, on_device, chunk=0, seed=1, slots=2, fail_at=-1, threads=4, with_status=True, reasons=1):
    n = len(recs)
    blob, offs = csr(recs)
    bm = C.create_string_buffer(b"\xff" * ((n + 7) // 8 + 1) + GUARD, (n + 7) // 8 + 65)
    st = C.create_string_buffer(b"\xff" * n + GUARD, n + 64)
    out = (C.c_uint64 * 5)()
    rc = host.zkhost_txcall_statements_selftest(C.c_int(on_device), C.c_int(reasons), C.c_size_t(n), blob + GUARD, offs, proof_ok, C.c_int(threads), C.c_size_t(chunk),
                                                C.c_uint32(seed), C.c_int(fail_at), C.c_int(slots), bm, st if with_status else None, out)
    assert st.raw[n:] == GUARD and bm.raw[(n + 7) // 8 + 1:] == GUARD
    return dict(rc=rc, bits=bm.raw[: (n + 7) // 8], status=st.raw[:n], chunks=out[0], leaked=out[1], hash_asks=out[2], host_hashed=out[3], formed=out[4])


@pytest.mark.parametrize("on_device", [0, 1])
def test_a_statements_call_asks_for_no_tape_and_writes_what_was_constructed(host, corpus, on_device):
    recs, proof_ok, want = corpus
    n = len(recs)
    for chunk, seed, slots, threads in ((0, 1, 2, 4), (8, 2, 2, 4), (16, 3, 1, 4), (24, 4, 2, 1), (64, 5, 1, 2)):
        got = _call(host, recs, proof_ok, on_device, chunk, seed, slots, threads=threads)
        assert got["rc"] == 0 and got["status"] == want, (chunk, got["rc"], list(got["status"]))
        assert bits(got["bits"], n) == [int(w == 0) for w in want]
        assert got["hash_asks"] == 0 and got["host_hashed"] == 0 and got["leaked"] == 0      # no tape, no second pass
        assert got["formed"] == (97 if on_device else 0)                                     # (every record the parser let through: 100 - {40, 50, 61})
        if chunk == 8:
            assert got["chunks"] == 13
    # status == NULL stays legal; a device without reasons writes 1 beside every clear bit inside what it serves
    got = _call(host, recs, proof_ok, on_device, 16, 6, with_status=False)
    assert got["rc"] == 0 and bits(got["bits"], n) == [int(w == 0) for w in want] and got["status"] == b"\xff" * n
    got = _call(host, recs, proof_ok, on_device, 16, 7, reasons=0)
    assert got["rc"] == 0 and got["status"] == bytes(w if w in (0, 2) else 1 for w in want)


def test_the_two_modes_give_identical_bytes(host, corpus):
    recs, proof_ok, want = corpus
    a = _call(host, recs, proof_ok, 0, chunk=16, seed=11)
    b = _call(host, recs, proof_ok, 1, chunk=16, seed=12, slots=1)
    assert (a["rc"], a["bits"], a["status"]) == (b["rc"], b["bits"], b["status"]) == (0, a["bits"], want)


def test_an_error_of_the_stand_in_leaves_one_and_zeros(host, corpus):
    recs, proof_ok, want = corpus
    recs, proof_ok, want = recs[:64], proof_ok[:64], want[:64]
    n = len(recs)
    for on_device in (0, 1):
        failures = 0
        for k in range(200):
            got = _call(host, recs, proof_ok, on_device, chunk=16, seed=100 + k, fail_at=k)
            if got["rc"] == 0:
                assert got["status"] == want
                break
            failures += 1
            assert got["rc"] == -3 and got["bits"] == bytes((n + 7) // 8) and got["leaked"] == 0, (on_device, k)
            # (1 everywhere; a record the library does not serve reads 2 if its chunk had been parsed when the call ended, else 1)
            assert all(s == 1 or (s == 2 and w == 2) for s, w in zip(got["status"], want)), (on_device, k)
        assert failures >= 12, (on_device, failures)         # (4 chunks: an enqueue and a collect of keys, proofs and signatures each)


# ---------------------------------------------------------------- 5. sanitizers
@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_parser_rows_and_scheduler_under_sanitizers(tmp_path, sanitizer):
    """tools/tx_statements_check.cpp: a program of its own (no Python in the process, nothing preloaded) runs the parser over
    exact-size copies of every truncation, musig_row, tx_sig_row and the stand-in scheduler in both modes"""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-O1", "-std=c++17", "-pthread", "-fsanitize=" + sanitizer, "-fno-omit-frame-pointer"] + (["-fno-sanitize-recover=all"] if "address" in sanitizer else [])
    r = subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + r.stderr.strip()[-300:])
    exe = tmp_path / "tx_statements_check"
    subprocess.run([cxx] + flags + ["-I" + os.path.join(ROOT, "zkvm_amd", "csrc"), os.path.join(ROOT, "tools", "tx_statements_check.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe), "17"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok:") and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
