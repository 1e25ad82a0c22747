"""ZKGPU_TXFORMAT_RETURN_LOG: the Input / Output entries of every accepted transaction's log handed back with the verdicts and
the transaction IDs -- what a node needs to apply a verified block to its UTXO set.  With the flag and a window K the status
argument of a transaction call is batch * (33 + 1 + 33 K) bytes: status bytes, IDs, then one record count | kind[K] | id[K][32]
per transaction.

Checked on the device: bitmap, status bytes and IDs are those of the same format without the flag; every record beside an
accepted transaction reproduces the oracle's transaction ID as the Merkle root over the header and its entries, and its inputs
are the contract IDs of the contracts the program pushed (tests/tx_log_util.py); every other record is zero; the three
arrangements -- records filled by the host VM (0x402), gathered by k_tx_log_gather behind the device's tape (0x502), the same
behind a chained signature stage (0x702) -- return identical bytes, whatever the chunking, the host threads or the round a
submitted call was merged into; the device counter moves by the entries the gather handed back; an unflagged call launches
what it launched; a call keeps the layout it was queued under; nothing leaks beside a signature that fails; and a failure of
any runtime call leaves the whole area zero.

The inputs are the 150-transaction block of tests/test_gpu_tx_device_hashing.py with the undecodable key of
tests/test_gpu_tx_sign_on_device.py and, added here, a proof whose version byte is flipped (80 transactions of one shape -- two
wavefronts of it on the tape -- and 15 to 40 of the others; every verdict 16, 17, 18, 19, 20, 21 and 2: the `block` fixture
asserts it), and the committed fixture.
"""
import ctypes as C
import struct

import pytest

from gpu_util import bits, load_tx_fixture
from test_gpu_tx_device_hashing import _hashed, _inside_second_pass, _verifier, block150, ctx, gens, mintime_flipped  # noqa: F401
from test_gpu_tx_reasons import ACCEPTED, KEY, OUTSIDE, PROOF_FORMAT, REJECTED, SIGNATURE, TX_INVALID, _bitmap, _v1, version_flipped
from test_gpu_tx_sign_on_device import _signed, r_flipped
from test_gpu_tx_sign_on_device import block as block_with_key  # noqa: F401
from test_tx_log_host import INVALID_FORMATS, valid_formats
from tx_log_util import _opcodes, area_bytes, check_accepted, record_bytes, split_area

pytestmark = pytest.mark.gpu
HASH, SIGN, IDS, LOG = 0x100, 0x200, 0x400, 0x800
ZERO = bytes(32)


@pytest.fixture(scope="module")
def block(block_with_key, oracle):
    """the block of the signing tests with one more damage, at an accepted position: the proof's version byte flipped -> status
    17, the one verdict that block lacks.  -> (transactions, expected status bytes of format 2), every verdict kind among them"""
    txs, want = block_with_key
    txs, want = list(txs), bytearray(want)
    i = next(i for i in range(len(txs) - 1, -1, -1) if want[i] == ACCEPTED)
    txs[i] = version_flipped(txs[i])
    want[i] = PROOF_FORMAT
    assert oracle.tx_verify(txs[i], bytes(range(64))) == _v1(bytes([PROOF_FORMAT]))[0]
    assert {2, 16, 17, 18, 19, 20, 21} <= set(want)
    return txs, bytes(want)


def _fmt(base, k):
    return base | LOG | (k << 16)


def _logged(ctx):
    return struct.unpack("<Q", ctx.debug_read("tx_logged_on_device", 8))[0]


def _entries(tx):
    return sum(1 for op in _opcodes(tx) if op in (0x1b, 0x1c))


def _offs(txs):
    n = len(txs)
    return (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:k + 1]) for k in range(n)]))


def _raw_call(ctx, bv, txs, k, threads=4):
    """zkgpu_tx_verify_batch on an array of exactly the layout's size and 64 guard bytes -> rc, bitmap, status, ids, records"""
    n = len(txs)
    size = area_bytes(n, k)
    bm = C.create_string_buffer(b"\xff" * ((n + 7) // 8), (n + 7) // 8)
    st = C.create_string_buffer(b"\xa5" * (size + 64), size + 64)
    rc = ctx.lib.zkgpu_tx_verify_batch(bv.h, n, b"".join(txs), _offs(txs), threads, bm, st)
    assert st.raw[size:] == b"\xa5" * 64, "guard bytes overwritten"
    return (rc, bm.raw) + split_area(st.raw, n, k)


def _records_of(log, k):
    """what verify_txs(log=True) hands back -> the records' bytes again (None: all zero)"""
    names = {"input": 1, "output": 2}
    out = []
    for entry in log:
        if entry is None:
            out.append(bytes(record_bytes(k)))
        elif isinstance(entry, int):
            out.append(bytes([entry]) + bytes(33 * k))
        else:
            kinds = bytes(names[a] for a, _ in entry)
            out.append(bytes([len(entry)]) + kinds.ljust(k, b"\0") + b"".join(i for _, i in entry).ljust(32 * k, b"\0"))
    return out


def test_format_values(ctx, gens):
    from zkvm_amd import TXFORMAT_LOG_SHIFT, TXFORMAT_RETURN_LOG
    assert (TXFORMAT_RETURN_LOG, TXFORMAT_LOG_SHIFT) == (LOG, 16)
    bv = _verifier(ctx, gens, 0)
    try:
        for fmt in valid_formats():
            assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, fmt) == 0, hex(fmt)
        for fmt in INVALID_FORMATS:
            assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, fmt) == -1, hex(fmt)
    finally:
        bv.close()


def test_three_arrangements_chunks_one_host_thread_and_two_calls_in_a_round(ctx, gens, oracle, block):
    """every window in turn in ONE test, so that the checks across windows and across arrangements never depend on which other
    tests ran: `seen` holds, per window, the records the first arrangement returned"""
    txs, want = block
    assert {2, 16, 17, 18, 19, 20, 21} <= set(want)
    seen = {}
    for k in (4, 5, 8):
        _arrangements(ctx, gens, oracle, txs, want, seen, k)
    assert any(r[0] == 5 and r[1:] == bytes(33 * 4) for r in seen[4])                       # the five-entry shapes read the count alone
    # K = 8 is K = 5 with zero padding
    assert [(r[0], r[1:1 + r[0]], r[6:6 + 32 * r[0]]) for r in seen[5]] == [(r[0], r[1:1 + r[0]], r[9:9 + 32 * r[0]]) for r in seen[8]]
    assert any(r[0] == 5 for r in seen[5])


def _arrangements(ctx, gens, oracle, txs, want, seen, k):
    n = len(txs)
    counts = [_entries(t) if s == ACCEPTED else 0 for t, s in zip(txs, want)]
    assert {2, 4, 5} <= set(counts)
    got = {}
    for base in (0x402, 0x502, 0x702):
        bv = _verifier(ctx, gens, base)
        try:
            plain = bv.verify_txs(txs, host_threads=4, ids=True)                            # the same format without 0x800
            assert plain[:2] == (_bitmap(want), want)
            bv.set_tx_format(base, log_k=k)
            out = bv.verify_txs(txs, host_threads=4, log=True)
            assert out[:3] == plain
            recs = _records_of(out[3], k)
            # the C layout, byte for byte, on an array of exactly the size it asks for
            rc, bm, st, ids, raw = _raw_call(ctx, bv, txs, k)
            assert (rc, bm, st, ids) == (0,) + plain and raw == recs
            if k not in seen:                                                               # (checked once per window: the rest must equal it)
                for i, t in enumerate(txs):
                    if want[i] == ACCEPTED:
                        assert check_accepted(oracle, t, ids[i], raw[i], k) == counts[i], i
                        assert isinstance(out[3][i], int) == (counts[i] > k)
                    else:
                        assert raw[i] == bytes(record_bytes(k)) and out[3][i] is None, i
                seen[k] = raw
            assert raw == seen[k], [i for i in range(n) if raw[i] != seen[k][i]]
            assert bv.verify_txs(txs, host_threads=4) == plain[:2]                          # (no change of arity without log=True)
            assert bv.verify_txs(txs, host_threads=4, ids=True) == plain
            bv.set_tx_chunk(64)                                                             # three chunks, the last a remainder
            assert bv.verify_txs(txs, host_threads=4, log=True) == out
            bv.set_tx_chunk(0)
            assert bv.verify_txs(txs, host_threads=1, log=True) == out
            a, b = bv.submit_txs(txs[:70], host_threads=2), bv.submit_txs(txs[70:], host_threads=2)
            rb, ra = bv.wait_txs(b, log=True), bv.wait_txs(a, log=True)                     # waited in reverse order, a buffer each
            assert ra == (_bitmap(want[:70]), want[:70], out[2][:70], out[3][:70])
            assert rb == (_bitmap(want[70:]), want[70:], out[2][70:], out[3][70:])
            bv.set_tx_format(base)
            with pytest.raises(ValueError):
                bv.verify_txs(txs, host_threads=4, log=True)
            got[base] = out
        finally:
            bv.close()
    assert got[0x702] == got[0x502] == got[0x402]


def test_the_counters(ctx, gens, block):
    """tx_logged_on_device moves by the entries of the rows the tape hashed (those that fit the window), only under 0x100;
    tx_hashed_on_device and tx_signed_on_device move as without the flag"""
    txs, want = block
    hashed = [t for t, s in zip(txs, want) if s not in (OUTSIDE, TX_INVALID)]
    rows = len(hashed)
    assert rows == _inside_second_pass(want)
    for base, k in ((0x702, 8), (0x702, 4), (0x502, 4), (0x402, 8)):
        bv = _verifier(ctx, gens, _fmt(base, k))
        try:
            assert (_logged(ctx), _hashed(ctx), _signed(ctx)) == (0, 0, 0)
            bv.verify_txs(txs, host_threads=4, log=True)
            fit = sum(e for e in map(_entries, hashed) if e <= k)
            print(hex(base), "K", k, "entries handed back", _logged(ctx), "of", sum(map(_entries, hashed)))
            assert _logged(ctx) == (fit if base & HASH else 0)
            assert _hashed(ctx) == (rows if base & HASH else 0) and _signed(ctx) == (rows if base & SIGN else 0)
            bv.set_tx_format(base)
            bv.verify_txs(txs, host_threads=4, ids=True)
            assert _logged(ctx) == (fit if base & HASH else 0)                              # (0 without the flag)
            assert _hashed(ctx) == (2 * rows if base & HASH else 0) and _signed(ctx) == (2 * rows if base & SIGN else 0)
        finally:
            bv.close()


def test_the_kernel_sets(ctx, gens):
    """0x701 and its flagged form differ by exactly k_tx_log_gather; 0x401 and its flagged form launch the same kernels"""
    txs = load_tx_fixture()[:128]
    n = len(txs)
    names = {}
    for fmt in (0x701, _fmt(0x701, 5), 0x401, _fmt(0x401, 5)):
        bv = _verifier(ctx, gens, fmt)
        try:
            ctx.profile(True)
            ctx.profile_reset()
            out = bv.verify_txs(txs, host_threads=4)
            assert bits(out[0], n) == [1] * n
            names[fmt] = set(ctx.profile_read())
        finally:
            ctx.profile(False)
            ctx.profile_reset()
            bv.close()
    print("kernels the flag adds to 0x701:", sorted(names[_fmt(0x701, 5)] - names[0x701]))
    assert names[_fmt(0x701, 5)] - names[0x701] == {"k_tx_log_gather"} and names[0x701] <= names[_fmt(0x701, 5)]
    assert names[0x401] == names[_fmt(0x401, 5)] and "k_tx_log_gather" not in names[0x401]


def test_the_layout_of_a_submitted_call_is_the_one_it_was_queued_under(ctx, gens, oracle, block):
    """queued under the flag and waited for after it was dropped: the large layout all the same; queued without the flag
    and waited for under it: the small layout, and the guard bytes behind it are intact"""
    txs, want = block
    txs, want = txs[:40], want[:40]
    n, k = len(txs), 5
    blob, offs = b"".join(txs), _offs(txs)
    bv = _verifier(ctx, gens, _fmt(0x702, k))
    try:
        cid = C.c_uint64(0)
        assert ctx.lib.zkgpu_tx_verify_submit(bv.h, n, blob, offs, 2, C.byref(cid)) == 0
        bv.set_tx_format(0x702)                                                 # (waits for the round: the format is the verifier's)
        size = area_bytes(n, k)
        bm, st = C.create_string_buffer((n + 7) // 8), C.create_string_buffer(b"\xa5" * (size + 64), size + 64)
        assert ctx.lib.zkgpu_tx_verify_wait(bv.h, cid.value, bm, st) == 0
        status, ids, recs = split_area(st.raw, n, k)
        assert (bm.raw, status) == (_bitmap(want), want) and st.raw[size:] == b"\xa5" * 64
        for i, t in enumerate(txs):
            if want[i] == ACCEPTED:
                check_accepted(oracle, t, ids[i], recs[i], k)
            else:
                assert ids[i] == ZERO and recs[i] == bytes(record_bytes(k)), i
        assert ctx.lib.zkgpu_tx_verify_submit(bv.h, n, blob, offs, 2, C.byref(cid)) == 0
        bv.set_tx_format(0x702, log_k=k)
        bm, st = C.create_string_buffer((n + 7) // 8), C.create_string_buffer(b"\xa5" * (33 * n + 64), 33 * n + 64)
        assert ctx.lib.zkgpu_tx_verify_wait(bv.h, cid.value, bm, st) == 0
        assert (bm.raw, st.raw[:n]) == (_bitmap(want), want) and st.raw[n: 33 * n] == b"".join(ids) and st.raw[33 * n:] == b"\xa5" * 64
    finally:
        bv.close()


def test_entries_the_device_computed_for_a_signature_that_fails_are_not_handed_back(ctx, gens, oracle):
    """a bit of mintime in one transaction, a bit of R in another: the device computed both transactions' contract IDs, and
    both read SIGNATURE with an all-zero record while their neighbours pass the Merkle check"""
    txs = load_tx_fixture()[:96]
    txs[10] = mintime_flipped(txs[10])
    txs[77] = r_flipped(txs[77])
    want = bytes(SIGNATURE if i in (10, 77) else ACCEPTED for i in range(96))
    k = 5
    for base in (0x702, 0x402):
        bv = _verifier(ctx, gens, _fmt(base, k))
        try:
            rc, bm, st, ids, recs = _raw_call(ctx, bv, txs, k)
            assert (rc, bm, st) == (0, _bitmap(want), want)
            if base & HASH:                                                     # (all 96 went through the tape and the gather)
                assert _hashed(ctx) == 96 and _logged(ctx) == sum(e for e in map(_entries, txs) if e <= k)
            for i, t in enumerate(txs):
                if i in (10, 77):
                    assert ids[i] == ZERO and recs[i] == bytes(record_bytes(k)), i
                else:
                    check_accepted(oracle, t, ids[i], recs[i], k)
        finally:
            bv.close()


def test_a_failure_of_any_runtime_call_leaves_the_whole_area_zero(ctx, gens, block):
    """zkgpu_debug_fail_after makes the n-th runtime call of the library answer "failed" on the host (nothing faults on the
    device).  n walks through every runtime call of a warm flagged 12-transaction call: EVERY one of them, failed, ends the call
    with a nonzero return, a zero bitmap and a status area that is zero but for status 1 inside the subset and 2 where it was --
    the library tolerates no failed runtime call on this path, so none may be swallowed: the gate must have fired exactly once
    and the call must have failed, for every n --; the clean call after each failure is right"""
    txs, want = block
    pick = list(dict.fromkeys([i for i, s in enumerate(want) if s in (OUTSIDE, KEY)] + list(range(10))))[:12]
    txs, want = [txs[i] for i in pick], bytes(want[i] for i in pick)
    n, k = len(txs), 5
    assert n == 12 and OUTSIDE in want and ACCEPTED in want
    bv = _verifier(ctx, gens, _fmt(0x702, k))
    try:
        good = _raw_call(ctx, bv, txs, k, threads=2)
        assert good[:3] == (0, _bitmap(want), want) and good == _raw_call(ctx, bv, txs, k, threads=2)     # (warm)
        assert any(r[0] for r in good[4])
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 10 ** 9, None)
        assert _raw_call(ctx, bv, txs, k, threads=2) == good
        calls = int(ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None))
        assert calls >= 40
        named = []
        for q in range(1, calls + 1):
            ctx.lib.zkgpu_debug_fail_after(ctx.h, q, None)
            out = _raw_call(ctx, bv, txs, k, threads=2)
            fired = C.c_longlong(-1)
            ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, C.byref(fired))
            assert fired.value == 1, (q, fired.value)                           # (the q-th call exists and was answered "failed")
            assert out[0] != 0, q
            assert out[1] == bytes((n + 7) // 8), q
            assert out[2] == bytes(OUTSIDE if s == OUTSIDE else REJECTED for s in want), q
            assert out[3] == [ZERO] * n and out[4] == [bytes(record_bytes(k))] * n, q
            if b"transaction-ID hashing stage" in ctx.lib.zkgpu_verifier_last_error(bv.h):
                named.append(q)
            assert _raw_call(ctx, bv, txs, k, threads=2) == good, q
        print("runtime calls of a clean call:", calls, "those of the hashing stage:", named)
        # the stage's copy up, launch, event for the chain, ID copy, table copy, gather, log copy, and the wait: at the least
        assert len(named) >= 8
    finally:
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None)
        bv.close()
