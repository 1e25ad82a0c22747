"""ZKGPU_TXFORMAT_RETURN_ROOT on the CPU: the format word with flag 16, the layout with 32 more bytes, the host fold of
csrc/tx_root.hpp and the hand-out of a merged round with roots, through libzkhost (zkhost_tx_root).

The reference tree is written here, top-down and recursive as oracle/zkvm_tx.c's root_of is (the RFC 6962 split: the left
subtree takes the largest power of two below the count), over the oracle's Merlin transcript -- an independent formulation of
the bottom-up fold the library runs.  tests/test_gpu_tx_root.py imports it.
"""
import ctypes as C
import hashlib
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_tx_hash_tape import host  # noqa: E402,F401
from test_tx_out_layout import model_valid, words  # noqa: E402
from tx_log_util import area_bytes  # noqa: E402

HASH, SIGN, IDS, LOG, PRE, SHIFT, RETURN_ROOT = 0x100, 0x200, 0x400, 0x800, 0x2000, 16, 16
REJECTED, OUTSIDE, PRECOMPUTED = 1, 2, 3
GUARD = 64
DEFAULT_SPAN = 7
LABEL = b"ZkVM.txroot"


def reference_root(ids):
    """MerkleTree::root over the IDs, as recalled: the transaction ID's own tree under the label ZkVM.txroot"""
    from oracle.binding import MerlinTranscript
    t = MerlinTranscript(LABEL)
    if not ids:
        return t.challenge_bytes(b"merkle.empty", 32)
    if len(ids) == 1:
        t.append_message(b"txid", ids[0])
        return t.challenge_bytes(b"merkle.leaf", 32)
    k = 1
    while 2 * k < len(ids):
        k *= 2
    t.append_message(b"L", reference_root(ids[:k]))
    t.append_message(b"R", reference_root(ids[k:]))
    return t.challenge_bytes(b"merkle.node", 32)


def some_ids(n, tag=b""):
    return [hashlib.sha256(b"txroot id %d " % i + tag).digest() for i in range(n)]


def call(host, op, ints, data=None, bitmap=None, area=None, out_bits=None, out_area=None, n_out=8):
    arr = (C.c_int64 * max(len(ints), 1))(*ints)
    out = (C.c_int64 * n_out)(*([-7] * n_out))
    rc = host.zkhost_tx_root(C.c_int(op), arr, data, bitmap, area, out_bits, out_area, out)
    return rc, list(out)


def fold(host, ids, span=0, threads=1):
    out = C.create_string_buffer(32)
    rc, o = call(host, 6, [len(ids), span, threads], b"".join(ids) if ids else None, out_area=out)
    assert rc == 0
    return out.raw, o[0]


def guarded(n, fill=0xA5):
    return C.create_string_buffer(bytes([fill]) * n + bytes([0x5A]) * GUARD, n + GUARD)


def intact(buf, n):
    return buf.raw[n:] == bytes([0x5A]) * GUARD


def model_valid_with_root(word):
    """a word with 16: valid if and only if the word without it is valid, has the IDs, and its base is 1 or 2"""
    old = word & ~RETURN_ROOT
    return word >= 0 and model_valid(old) and bool(old & IDS) and (old & 15) in (1, 2)


def test_words_with_and_without_the_flag(host):
    n_flagged = 0
    for w in words() + [w | PRE for w in words() if w >= 0] + [4, 4 | SIGN]:
        rc_old, old = call(host, 0, [w])
        assert rc_old == 0
        if w >= 0 and not w & RETURN_ROOT:
            rc, out = call(host, 0, [w | RETURN_ROOT])
            assert rc == 0
            valid = bool(old[0]) and bool(w & IDS) and (w & 15) in (1, 2)
            assert out[0] == int(valid), hex(w | RETURN_ROOT)
            if not w & PRE:
                assert valid == model_valid_with_root(w | RETURN_ROOT), hex(w)
            if valid:
                n_flagged += 1
                assert out[1:7] == old[1:7] and out[7] == 1, hex(w)          # the decoded fields of the flagless word are unchanged
        if old[0]:
            assert old[7] == 0, hex(w)
    # {1, 2} x {0, 0x100, 0x300} x 0x400 x {no log, 3 windows}, and the same under 0x2000 without 0x200
    assert n_flagged == 2 * 3 * 4 + 2 * 2 * 4
    for w in (RETURN_ROOT, RETURN_ROOT | 1, RETURN_ROOT | 2 | HASH, RETURN_ROOT | IDS, 4 | RETURN_ROOT, 4 | SIGN | RETURN_ROOT, 4 | IDS | RETURN_ROOT,
              RETURN_ROOT | 1 | LOG | (4 << SHIFT), 3 | IDS | RETURN_ROOT, 1 | IDS | RETURN_ROOT | 0x20, 1 | IDS | RETURN_ROOT | 0x1000):
        assert call(host, 0, [w])[1][0] == 0, hex(w)


@pytest.mark.parametrize("k", (0, 1, 255))
def test_layout_is_the_old_one_and_32_bytes(host, k):
    for batch in (0, 1, 7, 8, 9):
        old = area_bytes(batch, k) if k else 33 * batch
        rc, out = call(host, 1, [1, k, 1, batch])
        assert rc == 0 and out[:3] == [old + 32, old, old], (k, batch, out)
        rc, out = call(host, 1, [1, k, 0, batch])
        assert rc == 0 and out[:3] == [old, -1, -1]
        size, nb = old + 32, (batch + 7) // 8
        bm, area = guarded(nb, 0xFF), guarded(size)
        assert call(host, 2, [1, k, 1, batch], None, bm, area)[0] == 0                    # begin
        assert bm.raw[:nb] == bytes(nb) and area.raw[:size] == bytes([REJECTED]) * batch + bytes(size - batch)
        assert intact(bm, nb) and intact(area, size)
        area = guarded(size)
        assert call(host, 3, [1, k, 1, batch], None, None, area)[0] == 0                  # nothing in the subset
        assert area.raw[:size] == bytes([OUTSIDE]) * batch + bytes(size - batch) and intact(area, size)
        dirty = bytes(batch) + bytes([0xEE]) * (size - batch)
        bm, area = guarded(nb, 0xFF), C.create_string_buffer(dirty + bytes([0x5A]) * GUARD, size + GUARD)
        assert call(host, 4, [1, k, 1, batch], None, bm, area)[0] == 0                    # fail-closed
        assert bm.raw[:nb] == bytes(nb) and area.raw[:size] == bytes([REJECTED]) * batch + bytes(size - batch)
        assert intact(bm, nb) and intact(area, size)


SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 129)
S = 1 << DEFAULT_SPAN


@pytest.fixture(scope="module")
def references():
    ns = sorted(set(SIZES) | {S - 1, S, S + 1, 2 * S + 1})
    return {n: reference_root(some_ids(n)) for n in ns}


@pytest.mark.parametrize("threads", (1, 3))
def test_the_host_fold_is_the_recursive_tree(host, references, threads):
    for n in SIZES:
        got, passes = fold(host, some_ids(n), 0, threads)
        assert got == references[n], n
        assert passes == (0 if n <= 1 else 1 if n <= S else 2)
    for n in (S - 1, S, S + 1, 2 * S + 1):                                        # around the default span
        assert fold(host, some_ids(n), DEFAULT_SPAN, threads)[0] == references[n], n
    for span in (1, 2):                                                           # many passes
        for n in (n for n in SIZES if n <= 65):
            got, passes = fold(host, some_ids(n), span, threads)
            assert got == references[n], (span, n)
            if n == 65:
                assert passes == (7 if span == 1 else 4)
    # the tree is over the IDs in ORDER
    assert fold(host, list(reversed(some_ids(5))))[0] != references[5]
    assert fold(host, some_ids(5, b"other"))[0] != references[5]


def hand_out(host, calls, status, ok, roots):
    """calls: (batch, ids, K, root) each; status: the round's status bytes; -> per call (bits, area)"""
    total = sum(c[0] for c in calls)
    round_bits = bytearray((total + 7) // 8 + 1)
    for g, s in enumerate(status):
        round_bits[g // 8] |= (1 if s == 0 else 0) << (g % 8)
    sizes = [(area_bytes(b, k) if k else 33 * b if ids else b) + (32 if root else 0) for b, ids, k, root in calls]
    n_bits = sum((c[0] + 7) // 8 for c in calls)
    # (every call's ID and record parts hold what the round's verdicts wrote there; the root area is still zero, as begin left it)
    filled = b"".join(bytes([0xA5]) * b + bytes([0xC3]) * (size - b - (32 if root else 0)) + bytes(32 if root else 0) for (b, _, _, root), size in zip(calls, sizes))
    out_bits, out_area = guarded(n_bits), C.create_string_buffer(filled + bytes([0x5A]) * GUARD, len(filled) + GUARD)
    ints = [len(calls), ok] + [x for b, ids, k, root in calls for x in (ids, k, root, b)]
    rb, rs = C.create_string_buffer(bytes(round_bits), len(round_bits)), C.create_string_buffer(bytes(status), max(total, 1))
    assert call(host, 5, ints, b"".join(roots), rb, rs, out_bits, out_area)[0] == 0
    assert intact(out_bits, n_bits) and intact(out_area, len(filled))
    got, at = [], 0
    for size in sizes:
        got.append(out_area.raw[at: at + size])
        at += size
    return got


def test_a_round_hands_every_call_its_own_root(host):
    calls = [(5, 1, 0, 1), (64, 1, 4, 0), (1, 1, 0, 1)]                           # two of the three carry the flag
    roots = [fold(host, some_ids(b, b"call %d" % c))[0] for c, (b, _, _, _) in enumerate(calls)]
    total = 70
    whole = hand_out(host, calls, [0] * total, 1, roots)
    assert whole[0][:5] == bytes(5) and whole[0][-32:] == roots[0] and len(whole[0]) == 33 * 5 + 32
    assert len(whole[1]) == area_bytes(64, 4)                                     # no root area: nothing appended, nothing moved
    assert whole[2][-32:] == roots[2] and len(whole[2]) == 33 + 32
    # one transaction of the first call not accepted: its root is zero, the others keep theirs
    status = [0] * total
    status[3] = 19
    short = hand_out(host, calls, status, 1, roots)
    assert short[0][:5] == bytes([0, 0, 0, 19, 0]) and short[0][-32:] == bytes(32) and short[0][5:-32] == whole[0][5:-32]
    assert short[1] == whole[1] and short[2] == whole[2]
    # ... of the last call
    status = [0] * total
    status[69] = OUTSIDE
    short = hand_out(host, calls, status, 1, roots)
    assert short[0] == whole[0] and short[2][-32:] == bytes(32)
    # a precompute-only round: every status byte 3
    pre = hand_out(host, calls, [PRECOMPUTED] * total, 1, roots)
    assert pre[0][-32:] == roots[0] and pre[2][-32:] == roots[2]
    mixed = hand_out(host, calls, [PRECOMPUTED] * 4 + [0] + [PRECOMPUTED] * 65, 1, roots)
    assert mixed[0][-32:] == bytes(32)
    # a failed round: all zeros
    failed = hand_out(host, calls, [0] * total, 0, roots)
    for (b, _, _, _), got in zip(calls, failed):
        assert got == bytes([REJECTED]) * b + bytes(len(got) - b)


def test_fold_and_clears_under_sanitizers(tmp_path):
    """tools/tx_root_check.cpp: a program of its own (no Python in the process) drives the host fold of tx_root.hpp and the
    layout's clears over heap arrays of exactly the size they are given, at n = 0, 1 and 65, under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    r = subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + r.stderr.strip()[-300:])
    exe = tmp_path / "tx_root_check"
    subprocess.run([cxx] + flags + [os.path.join(ROOT, "tools", "tx_root_check.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok") and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
