"""csrc/tx_out.hpp on the CPU: the header in which the library lays out what a transaction call hands its caller -- the format
word decoded and validated, the status argument  status[batch] | id[batch][32] | record[batch][1 + 33 K]  as a value, the
three moments that write it wholesale (begin, nothing-in-the-subset, fail-closed) and the hand-out of a merged round to its
calls.  libzkgpu and libzkhost compile the same header; zkhost_tx_out_layout is its entry for this test, and the self-tests
of tests/test_tx_ids_host.py and tests/test_tx_log_host.py run a scheduler over it.

The model is independent of the header: the five validity rules are written out below, sizes and offsets are those of
tests/tx_log_util.py (area_bytes / split_area), and the hand-out is a few lines of Python over lists.

NOT tested here: zkgpu_verifier_set_tx_format's own answer (it needs a verifier, hence a device); the GPU tests hold it
against the same table of values (tests/test_gpu_tx_log.py::test_format_values).
"""
import ctypes as C
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_tx_hash_tape import host  # noqa: E402,F401
from tx_log_util import area_bytes, record_bytes, split_area  # noqa: E402

HASH, SIGN, IDS, LOG, SHIFT = 0x100, 0x200, 0x400, 0x800, 16
REJECTED, OUTSIDE = 1, 2
GUARD = 64
BATCHES = (0, 1, 7, 8, 9, 64)


def call(host, op, ints, bitmap=None, area=None, out_bits=None, out_area=None, n_out=8):
    arr = (C.c_int64 * max(len(ints), 1))(*ints)
    out = (C.c_int64 * n_out)(*([-7] * n_out))
    rc = host.zkhost_tx_out_layout(C.c_int(op), arr, bitmap, area, out_bits, out_area, out)
    return rc, list(out)


def model_valid(word):
    """the five rules of zkgpu_verifier_set_tx_format"""
    if word < 0:                                                           # format >= 0
        return False
    k, log = (word >> SHIFT) & 255, bool(word & LOG)
    base = word & ~(HASH | SIGN | IDS | LOG | (255 << SHIFT))
    if log != (k != 0):                                                    # the log flag if and only if K != 0
        return False
    if log and not word & IDS:                                             # the log only beside the IDs
        return False
    if word & SIGN and not word & HASH:                                    # signing on the device only beside hashing there
        return False
    return word == 0 or base in (1, 2)                                     # flags (or anything else) only beside a base format


def words():
    out = [base | (HASH if h else 0) | (SIGN if s else 0) | (IDS if i else 0) | (LOG if l else 0) | (k << SHIFT)
           for base in (0, 1, 2) for h in (0, 1) for s in (0, 1) for i in (0, 1) for l in (0, 1) for k in (0, 1, 4, 255)]
    return out + [-1, -(2 ** 31), 0xC01 | (4 << SHIFT) | (1 << 30), 1 | (1 << 24), 3, 0x1001, 0xC01 | (4 << SHIFT) | 0x8000]


def layouts():
    return [(0, 0), (1, 0), (1, 1), (1, 4), (1, 255)]


def test_decoding_follows_the_five_rules(host):
    n_valid = 0
    for w in words():
        rc, out = call(host, 0, [w])
        assert rc == 0 and out[0] == int(model_valid(w)), hex(w)
        if not model_valid(w):
            continue
        n_valid += 1
        assert out[1:6] == [w & 255, int(bool(w & HASH)), int(bool(w & SIGN)), int(bool(w & IDS)), (w >> SHIFT) & 255], hex(w)
    # 0 | 2 bases x (hash, sign) in 3 valid pairs x (no ids | ids | ids + log with 3 windows)
    assert n_valid == 1 + 2 * 3 * (1 + 1 + 3)


@pytest.mark.parametrize("ids,k", layouts())
def test_sizes_and_offsets_are_the_tests_own_model(host, ids, k):
    for batch in BATCHES:
        for i in sorted({0, max(batch - 1, 0)}):
            rc, out = call(host, 1, [ids, k, batch, i])
            assert rc == 0
            if k:
                raw = bytes(range(256)) * (area_bytes(batch, k) // 256 + 1)
                raw = raw[: area_bytes(batch, k)]
                assert out[0] == len(raw)
                if batch:
                    st, idl, recs = split_area(raw, batch, k)
                    assert raw[out[1]: out[1] + 1] == st[i: i + 1] and out[1] == i
                    assert raw[out[2]: out[2] + 32] == idl[i] and out[2] == batch + 32 * i
                    assert raw[out[3]: out[3] + record_bytes(k)] == recs[i] and out[3] == 33 * batch + record_bytes(k) * i
                assert out[4:7] == [batch, 33 * batch, k]
            else:
                assert out[0] == (33 * batch if ids else batch)
                assert out[1:4] == [i, batch + 32 * i if ids else -1, -1]
                assert out[4:7] == [batch if ids else -1, -1, 0]


def guarded(n, fill=0xA5):
    """n bytes of 0xA5 and a guard behind them"""
    return C.create_string_buffer(bytes([fill]) * n + bytes([0x5A]) * GUARD, n + GUARD)


def intact(buf, n):
    return buf.raw[n:] == bytes([0x5A]) * GUARD


@pytest.mark.parametrize("ids,k", layouts())
def test_begin_nothing_in_the_subset_and_fail_closed(host, ids, k):
    rng = random.Random(1000 * ids + k)
    for batch in BATCHES:
        size = (33 + record_bytes(k) if k else 33 if ids else 1) * batch
        nb = (batch + 7) // 8
        # begin: no bit, every status "rejected", zeros behind
        bm, area = guarded(nb), guarded(size)
        assert call(host, 2, [ids, k, batch], bm, area)[0] == 0
        assert bm.raw[:nb] == bytes(nb) and area.raw[:size] == bytes([REJECTED]) * batch + bytes(size - batch)
        assert intact(bm, nb) and intact(area, size)
        # nothing in the subset, on the area that has begun: every status "outside the subset", zeros behind
        assert call(host, 3, [ids, k, batch], None, area)[0] == 0
        assert area.raw[:size] == bytes([OUTSIDE]) * batch + bytes(size - batch) and intact(area, size)
        # fail-closed over a mix: accepted, outside the subset, a reason, and IDs / records that are not zero
        status = bytes(rng.choice((0, 2, 17)) for _ in range(batch))
        dirty = status + bytes(rng.randrange(1, 256) for _ in range(size - batch))
        bm = guarded(nb, 0xFF)
        area = C.create_string_buffer(dirty + bytes([0x5A]) * GUARD, size + GUARD)
        assert call(host, 4, [ids, k, batch], bm, area)[0] == 0
        assert bm.raw[:nb] == bytes(nb) and intact(bm, nb) and intact(area, size)
        assert area.raw[:size] == bytes(OUTSIDE if s == OUTSIDE else REJECTED for s in status) + bytes(size - batch)
        # a caller without a status argument: the bitmap alone
        for op in (2, 4):
            bm = guarded(nb, 0xFF)
            assert call(host, op, [ids, k, batch], bm, None)[0] == 0
            assert bm.raw[:nb] == bytes(nb) and intact(bm, nb)
        assert call(host, 3, [ids, k, batch], None, None)[0] == 0


HAND_OUTS = [[(13, 0, 0), (11, 1, 4)],                          # (batch, ids, K) per call: sizes that are no multiple of 8 after the first
             [(8, 1, 0), (5, 1, 255), (19, 0, 0)],
             [(3, 1, 1), (7, 1, 4), (9, 1, 0)]]


@pytest.mark.parametrize("calls", HAND_OUTS)
@pytest.mark.parametrize("ok", (1, 0))
def test_a_rounds_hand_out(host, calls, ok):
    rng = random.Random(len(calls) * 2 + ok)
    total = sum(b for b, _, _ in calls)
    bits = [rng.randrange(2) for _ in range(total)]
    status = [0 if b else rng.choice((1, 2, 17, 21)) for b in bits]
    round_bits = bytearray((total + 7) // 8 + 1)
    for g, b in enumerate(bits):
        round_bits[g // 8] |= b << (g % 8)
    sizes = [(33 + record_bytes(k) if k else 33 if ids else 1) * b for b, ids, k in calls]
    # (every call's ID and record parts hold what the round's verdicts wrote there: bytes that are not zero)
    behind = [bytes(rng.randrange(1, 256) for _ in range(size - b)) for size, (b, _, _) in zip(sizes, calls)]
    areas = b"".join(bytes([0xA5]) * b + rest for (b, _, _), rest in zip(calls, behind))
    n_bits = sum((b + 7) // 8 for b, _, _ in calls)
    out_bits, out_area = guarded(n_bits), C.create_string_buffer(areas + bytes([0x5A]) * GUARD, len(areas) + GUARD)
    ints = [len(calls), ok] + [x for b, ids, k in calls for x in (ids, k, b)]
    rb, rs = C.create_string_buffer(bytes(round_bits), len(round_bits)), C.create_string_buffer(bytes(status), max(total, 1))
    assert call(host, 5, ints, rb, rs, out_bits, out_area)[0] == 0
    assert intact(out_bits, n_bits) and intact(out_area, len(areas))
    at = at_bits = at_area = 0
    for (b, ids, k), size, rest in zip(calls, sizes, behind):
        want_bits = bytearray((b + 7) // 8)
        for i in range(b):
            want_bits[i // 8] |= (bits[at + i] if ok else 0) << (i % 8)
        assert out_bits.raw[at_bits: at_bits + len(want_bits)] == bytes(want_bits)
        got = out_area.raw[at_area: at_area + size]
        if ok:
            assert got == bytes(status[at: at + b]) + rest
        else:
            assert got == bytes(OUTSIDE if s == OUTSIDE else REJECTED for s in status[at: at + b]) + bytes(size - b)
        at, at_bits, at_area = at + b, at_bits + len(want_bits), at_area + size


PRE, STATEMENTS = 0x2000, 4
ROUND_WORDS = [0, 1, 2, 1 | HASH, 2 | HASH | SIGN, 1 | IDS, 2 | HASH | IDS | PRE, 1 | IDS | PRE, STATEMENTS, STATEMENTS | SIGN]


def model_round_key(word):
    """a submitted call's kind and what it is keyed by: precompute-only by (base, hashing), statements by (signing), anything
    else verifies -- one key whatever its word"""
    if word & PRE:
        return ("precompute", word & 7, bool(word & HASH))
    if word & 7 == STATEMENTS:
        return ("statements", bool(word & SIGN))
    return ("verify",)


def model_round_format(first, now):
    """-> [base, hash, sign, precompute-only, reasons] of the round whose first call was submitted under `first`, started under `now`"""
    kind = model_round_key(first)[0]
    if kind == "precompute":                                # as its calls were queued; never signs on the device
        return [first & 7, int(bool(first & HASH)), 0, 1, int(first & 7 == 2)]
    if kind == "statements":                                # base 4 and the signing switch its calls were queued under
        return [STATEMENTS, 0, int(bool(first & SIGN)), 0, 1]
    word = first if now & 7 == STATEMENTS else now          # the format in force now -- its bytes are transactions, though
    return [word & 7, int(bool(word & HASH)), int(bool(word & SIGN)), 0, int(word & 7 == 2)]


def test_the_round_rule_of_calls_in_flight(host):
    """tx_round_mates / tx_round_format (what the engine of zkgpu_tx_verify_submit asks) over every triple of words -- the round's
    first call's, the one in force when the round starts, a candidate's -- against the rule written out above"""
    assert all(model_valid(w & ~PRE) for w in ROUND_WORDS if w & 7 != STATEMENTS)
    for first in ROUND_WORDS:
        for now in ROUND_WORDS:
            for candidate in ROUND_WORDS:
                rc, out = call(host, 6, [first, now, candidate])
                assert rc == 0, (hex(first), hex(now), hex(candidate))
                assert out[0] == int(model_round_key(candidate) == model_round_key(first)), (hex(first), hex(candidate))
                assert out[1:6] == model_round_format(first, now), (hex(first), hex(now))
    assert call(host, 6, [1, 2, SIGN | 1])[0] == -1         # (a word the format refuses)
