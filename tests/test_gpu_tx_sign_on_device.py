"""ZKGPU_TXFORMAT_SIGN_ON_DEVICE: the challenge of a transaction's signature formed by k_tx_sig_rows (csrc/tx_sig_rows.hpp)
from the transaction ID and the aggregated key where the device left them, instead of on the host between two device stages.
Verdicts and status bytes must be those of the same call without the flag, and the oracle's;
zkgpu_debug_read("tx_signed_on_device") tells the device path from a silent host fallback.

The block is the 150-transaction block of tests/test_gpu_tx_device_hashing.py (four shapes, three key counts, every shape's
run part padding, more than one wavefront) with its seven damages, plus one undecodable KEY.
"""
import ctypes as C
import struct

import pytest

from gpu_util import bits, load_tx_fixture
from test_gpu_tx_device_hashing import _hashed, _inside_second_pass, _verifier, block150, ctx, gens, mintime_flipped  # noqa: F401
from test_gpu_tx_reasons import ACCEPTED, KEY, OUTSIDE, REJECTED, SIGNATURE, _bitmap, _parts, _put, _undecodable, _v1

pytestmark = pytest.mark.gpu
HASH, SIGN = 0x100, 0x200


def _signed(ctx):
    return struct.unpack("<Q", ctx.debug_read("tx_signed_on_device", 8))[0]


def key_undecodable(tx):
    """the predicate of the FIRST contract the program pushes (push:n: anchor:32 predicate:32 ...): a key the signature covers"""
    assert tx[28] == 0x00
    return _put(tx, 28 + 1 + 4 + 32, _undecodable())


def r_flipped(tx):
    sig_at, _ = _parts(tx)
    return _put(tx, sig_at + 3, bytes([tx[sig_at + 3] ^ 0x10]))


@pytest.fixture(scope="module")
def block(block150, oracle):
    """the block of the hashing tests with one more damage: an undecodable key at an accepted position -> status 20"""
    txs, want = block150
    txs, want = list(txs), bytearray(want)
    i = next(i for i in range(60, 150) if want[i] == ACCEPTED)
    txs[i] = key_undecodable(txs[i])
    want[i] = KEY
    assert oracle.tx_verify(txs[i], bytes(range(64))) == REJECTED
    return txs, bytes(want)


def test_format_values(ctx, gens):
    from zkvm_amd import TXFORMAT_HASH_ON_DEVICE, TXFORMAT_SIGN_ON_DEVICE
    from zkvm_amd.verifier import BlockVerifier
    assert TXFORMAT_SIGN_ON_DEVICE == BlockVerifier.TXFORMAT_SIGN_ON_DEVICE == SIGN and TXFORMAT_HASH_ON_DEVICE == HASH
    bv = _verifier(ctx, gens, 0)
    try:
        for fmt in (0x301, 0x302, 0x101, 0x102, 1, 2, 0):
            assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, fmt) == 0, hex(fmt)
        for fmt in (0x200, 0x201, 0x202, 0x300, 0x303, 0x100, 0x103):
            assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, fmt) == -1, hex(fmt)
    finally:
        bv.close()


def test_a_lone_call_chunks_one_host_thread_and_two_calls_in_a_round(ctx, gens, block):
    """the flagged verifier first (its counters are read), then 0x102 and 2 on the same context (the new counter stays 0)"""
    txs, want = block
    rows = _inside_second_pass(want)                                          # every transaction the VM accepted has a signature row
    got = {}
    for fmt in (0x302, 0x102, 2):
        bv = _verifier(ctx, gens, fmt)
        try:
            assert _signed(ctx) == 0 and _hashed(ctx) == 0
            got[fmt] = bv.verify_txs(txs, host_threads=4)
            print(hex(fmt), "status", list(got[fmt][1]))
            assert got[fmt] == (_bitmap(want), want)
            assert _signed(ctx) == (rows if fmt & SIGN else 0)
            assert _hashed(ctx) == (rows if fmt & HASH else 0)
            bv.set_tx_format(fmt - 1)                                         # 0x301 against 1
            assert bv.verify_txs(txs, host_threads=4) == (_bitmap(want), _v1(want))
            bv.set_tx_format(fmt)
            bv.set_tx_chunk(64)                                               # three chunks, the last a remainder
            assert bv.verify_txs(txs, host_threads=4) == got[fmt]
            bv.set_tx_chunk(0)
            assert bv.verify_txs(txs, host_threads=1) == got[fmt]
            before = _signed(ctx)
            a, b = bv.submit_txs(txs[:70], host_threads=2), bv.submit_txs(txs[70:], host_threads=2)
            rb, ra = bv.wait_txs(b), bv.wait_txs(a)                           # waited in reverse order
            assert ra == (_bitmap(want[:70]), want[:70]) and rb == (_bitmap(want[70:]), want[70:])
            assert _signed(ctx) - before == (rows if fmt & SIGN else 0)
        finally:
            bv.close()
    assert got[0x302] == got[0x102] == got[2]


def test_the_committed_fixture(ctx, gens):
    txs = load_tx_fixture()
    out = {}
    for fmt in (0x301, 1):
        bv = _verifier(ctx, gens, fmt)
        try:
            out[fmt] = bv.verify_txs(txs, host_threads=4)
            assert _signed(ctx) == (len(txs) if fmt & SIGN else 0)
        finally:
            bv.close()
    assert out[0x301] == out[1] and bits(out[1][0], len(txs)) == [1] * len(txs)


def test_damage_that_only_the_challenge_sees(ctx, gens):
    """a bit of mintime (the ID changes) in one transaction, a bit of R in another: both read SIGNATURE while their neighbours
    are accepted -- a challenge kernel that ignored one of its inputs would accept them"""
    txs = load_tx_fixture()[:96]
    txs[10] = mintime_flipped(txs[10])
    txs[77] = r_flipped(txs[77])
    want = bytes(SIGNATURE if i in (10, 77) else ACCEPTED for i in range(96))
    bv = _verifier(ctx, gens, 0x302)
    try:
        assert bv.verify_txs(txs, host_threads=4) == (_bitmap(want), want)
        bv.set_tx_format(2)
        assert bv.verify_txs(txs, host_threads=4) == (_bitmap(want), want)
    finally:
        bv.close()


def test_an_error_of_the_new_step_fails_the_call_closed(ctx, gens, block):
    """zkgpu_debug_fail_after makes the n-th runtime call of the library answer "failed" on the host (nothing faults on the
    device).  n walks through a warm 24-transaction 0x302 call: for EVERY n either the call is right, or it returns an error
    with a zero bitmap, status 1 inside the subset and 2 left alone; some n names the new step; a clean call afterwards is right."""
    txs, want = block
    pick = list(dict.fromkeys([i for i, s in enumerate(want) if s in (OUTSIDE, KEY)] + list(range(22))))
    txs, want = [txs[i] for i in pick], bytes(want[i] for i in pick)
    n = len(txs)
    blob = b"".join(txs)
    offs = (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:i + 1]) for i in range(n)]))
    bv = _verifier(ctx, gens, 0x302)

    def call():
        bm = C.create_string_buffer(b"\xff" * ((n + 7) // 8), (n + 7) // 8)
        st = C.create_string_buffer(b"\x00" * n, n)
        return ctx.lib.zkgpu_tx_verify_batch(bv.h, n, blob, offs, 2, bm, st), bm.raw, st.raw

    try:
        good = (0, _bitmap(want), want)
        assert call() == good and call() == good                             # (warm: every buffer of the stages exists)
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 10 ** 9, None)
        assert call() == good
        calls = int(ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None))
        named = []
        for k in range(1, calls + 1):
            ctx.lib.zkgpu_debug_fail_after(ctx.h, k, None)
            rc, bm, st = call()
            ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None)
            if rc == 0:
                assert (rc, bm, st) == good, k
                continue
            assert bm == bytes((n + 7) // 8) and st == bytes(OUTSIDE if s == OUTSIDE else REJECTED for s in want), k
            if b"signature challenge stage" in ctx.lib.zkgpu_verifier_last_error(bv.h):
                named.append(k)
        print("runtime calls of a clean call:", calls, "those of the new step:", named)
        assert named
        assert call() == good
    finally:
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None)
        bv.close()


def test_an_unflagged_call_launches_nothing_new(ctx, gens):
    txs = load_tx_fixture()[:128]
    names = {}
    for fmt in (0x101, 0x301):
        bv = _verifier(ctx, gens, fmt)
        try:
            ctx.profile(True)
            ctx.profile_reset()
            out = bv.verify_txs(txs, host_threads=4)
            assert bits(out[0], len(txs)) == [1] * len(txs)
            names[fmt] = set(ctx.profile_read())
            assert _signed(ctx) == (len(txs) if fmt & SIGN else 0)
        finally:
            ctx.profile(False)
            ctx.profile_reset()
            bv.close()
    assert "k_tx_sig_rows" not in names[0x101] and "k_tx_sig_rows" in names[0x301], names
