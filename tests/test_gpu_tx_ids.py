"""ZKGPU_TXFORMAT_RETURN_IDS: the transaction ID of every accepted transaction handed back with the verdicts -- the Ok side
of upstream's Result<VerifiedTx, VMError>.  With the flag the status argument of a transaction call is 33 * batch bytes: the
status bytes, then 32 bytes per transaction that hold the ID beside status 0 and zeros beside everything else.

Checked on the device: bitmap and status bytes are those of the same format without the flag; every ID is the oracle's
(oracle/zkvm_tx.c, written separately) whichever of the three hashing arrangements produced it -- the host VM (0x402), the
device's tape (0x502), the tape with the IDs left on the device for the challenge (0x702: the one arrangement where the flag
adds a copy); a transaction whose ID the device computed but whose signature failed hands back zeros; the device counters
move as without the flag; and a call without the flag launches and writes nothing new.  The fail-closed paths are covered
on the CPU (tests/test_tx_ids_host.py).

The inputs are the 150-transaction block of tests/test_gpu_tx_device_hashing.py with the undecodable key of
tests/test_gpu_tx_sign_on_device.py, and the committed fixture.
"""
import ctypes as C

import pytest

from gpu_util import bits, load_tx_fixture
from test_gpu_tx_device_hashing import _hashed, _inside_second_pass, _verifier, block150, ctx, gens, mintime_flipped  # noqa: F401
from test_gpu_tx_reasons import ACCEPTED, KEY, OUTSIDE, SIGNATURE, _bitmap
from test_gpu_tx_sign_on_device import _signed, block, r_flipped  # noqa: F401

pytestmark = pytest.mark.gpu
HASH, SIGN, IDS = 0x100, 0x200, 0x400
ZERO = bytes(32)


@pytest.fixture(scope="module")
def block_ids(block, oracle):
    """-> (transactions, expected status bytes of format 2, expected IDs: the oracle's beside status 0, zeros elsewhere)"""
    txs, want = block
    ids = []
    for t, s in zip(txs, want):
        if s == ACCEPTED:
            rc, txid, _, _ = oracle.tx_id(t)
            assert rc == 0 and txid != ZERO
            ids.append(txid)
        else:
            ids.append(ZERO)
    assert set(want) >= {16, 19, 18, 20, 21, 2}                               # every kind of verdict that must read zeros
    return txs, want, ids


def test_format_values(ctx, gens):
    from zkvm_amd import TXFORMAT_RETURN_IDS
    from zkvm_amd.verifier import BlockVerifier
    assert TXFORMAT_RETURN_IDS == BlockVerifier.TXFORMAT_RETURN_IDS == IDS
    bv = _verifier(ctx, gens, 0)
    try:
        valid = [base | hs | f for base in (1, 2) for hs in (0, 0x100, 0x300) for f in (0, IDS)]
        assert len(valid) == 12
        for fmt in valid + [0]:
            assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, fmt) == 0, hex(fmt)
        for fmt in (0x400, 0x403, 0x600, 0x601, 0x801, 0x1401):
            assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, fmt) == -1, hex(fmt)
    finally:
        bv.close()


def test_a_lone_call_chunks_one_host_thread_and_two_calls_in_a_round(ctx, gens, block_ids):
    txs, want, ids = block_ids
    rows = _inside_second_pass(want)
    got = {}
    for fmt in (0x702, 0x502, 0x402):
        bv = _verifier(ctx, gens, fmt)
        try:
            assert _signed(ctx) == 0 and _hashed(ctx) == 0
            got[fmt] = bv.verify_txs(txs, host_threads=4, ids=True)
            print(hex(fmt), "status", list(got[fmt][1]), "ids that differ", [i for i in range(len(txs)) if got[fmt][2][i] != ids[i]])
            assert got[fmt] == (_bitmap(want), want, ids)
            assert bv.verify_txs(txs, host_threads=4) == (_bitmap(want), want)              # (no change of arity without ids=True)
            assert _signed(ctx) == (2 * rows if fmt & SIGN else 0)                          # the counters move as without the flag
            assert _hashed(ctx) == (2 * rows if fmt & HASH else 0)
            bv.set_tx_format(fmt - IDS)                                                     # the same format without the flag
            assert bv.verify_txs(txs, host_threads=4) == got[fmt][:2]
            with pytest.raises(ValueError):
                bv.verify_txs(txs, host_threads=4, ids=True)
            bv.set_tx_format(fmt)
            bv.set_tx_chunk(64)                                                             # three chunks, the last a remainder
            assert bv.verify_txs(txs, host_threads=4, ids=True) == got[fmt]
            bv.set_tx_chunk(0)
            assert bv.verify_txs(txs, host_threads=1, ids=True) == got[fmt]
            before = _signed(ctx), _hashed(ctx)
            a, b = bv.submit_txs(txs[:70], host_threads=2), bv.submit_txs(txs[70:], host_threads=2)
            rb, ra = bv.wait_txs(b, ids=True), bv.wait_txs(a, ids=True)                     # waited in reverse order, a buffer each
            assert ra == (_bitmap(want[:70]), want[:70], ids[:70])
            assert rb == (_bitmap(want[70:]), want[70:], ids[70:])
            assert _signed(ctx) - before[0] == (rows if fmt & SIGN else 0)
            assert _hashed(ctx) - before[1] == (rows if fmt & HASH else 0)
        finally:
            bv.close()
    assert got[0x702] == got[0x502] == got[0x402]


def test_an_id_the_device_computed_for_a_signature_that_fails_is_not_handed_back(ctx, gens, oracle):
    """a bit of mintime in one transaction (its ID changes: the device hashes the new one), a bit of R in another (its ID is
    untouched): both read SIGNATURE with zero IDs, while their neighbours carry the oracle's"""
    txs = load_tx_fixture()[:96]
    txs[10] = mintime_flipped(txs[10])
    txs[77] = r_flipped(txs[77])
    want = bytes(SIGNATURE if i in (10, 77) else ACCEPTED for i in range(96))
    ids = [ZERO if i in (10, 77) else oracle.tx_id(t)[1] for i, t in enumerate(txs)]
    assert oracle.tx_id(txs[10])[0] == 0 and oracle.tx_id(txs[77])[0] == 0      # (both HAVE an ID: it is withheld, not missing)
    for fmt in (0x702, 0x402):
        bv = _verifier(ctx, gens, fmt)
        try:
            out = bv.verify_txs(txs, host_threads=4, ids=True)
            assert out[:2] == (_bitmap(want), want)
            assert out[2][10] == ZERO and out[2][77] == ZERO
            assert out[2] == ids
        finally:
            bv.close()


def test_one_transaction_none_and_no_status_array(ctx, gens, block_ids):
    txs, want, ids = block_ids
    i = next(i for i in range(150) if want[i] == ACCEPTED)
    j = next(i for i in range(150) if want[i] == KEY)
    bv = _verifier(ctx, gens, 0x702)
    try:
        assert bv.verify_txs([txs[i]], host_threads=2, ids=True) == (b"\x01", bytes([ACCEPTED]), [ids[i]])
        assert bv.verify_txs([txs[j]], host_threads=2, ids=True) == (b"\x00", bytes([KEY]), [ZERO])
        assert bv.verify_txs([], host_threads=2, ids=True) == (b"", b"", [])
        # batch == 0 through the C interface: nothing of the status argument is touched
        guard = C.create_string_buffer(b"\xa5" * 40, 40)
        bm = C.create_string_buffer(1)
        assert ctx.lib.zkgpu_tx_verify_batch(bv.h, 0, None, None, 2, bm, guard) == 0 and guard.raw == b"\xa5" * 40
        # status == NULL stays legal: the bitmap alone
        n = len(txs)
        blob = b"".join(txs)
        offs = (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:k + 1]) for k in range(n)]))
        bm = C.create_string_buffer(b"\xff" * ((n + 7) // 8), (n + 7) // 8)
        assert ctx.lib.zkgpu_tx_verify_batch(bv.h, n, blob, offs, 4, bm, None) == 0 and bm.raw == _bitmap(want)
        cid = C.c_uint64(0)
        assert ctx.lib.zkgpu_tx_verify_submit(bv.h, n, blob, offs, 4, C.byref(cid)) == 0
        bm = C.create_string_buffer(b"\xff" * ((n + 7) // 8), (n + 7) // 8)
        assert ctx.lib.zkgpu_tx_verify_wait(bv.h, cid.value, bm, None) == 0 and bm.raw == _bitmap(want)
    finally:
        bv.close()


def test_the_layout_of_a_submitted_call_is_the_one_it_was_queued_under(ctx, gens, block_ids):
    """queued under 0x702 and waited for under 0x302: 33 bytes per transaction all the same; queued under 0x302 and waited for
    under 0x702: the status bytes alone, and the guard bytes behind them are intact"""
    txs, want, ids = block_ids
    txs, want, ids = txs[:40], want[:40], ids[:40]
    n = len(txs)
    blob = b"".join(txs)
    offs = (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:k + 1]) for k in range(n)]))
    bv = _verifier(ctx, gens, 0x702)
    try:
        cid = C.c_uint64(0)
        assert ctx.lib.zkgpu_tx_verify_submit(bv.h, n, blob, offs, 2, C.byref(cid)) == 0
        bv.set_tx_format(0x302)                                                 # (waits for the round: the format is the verifier's)
        bm, st = C.create_string_buffer((n + 7) // 8), C.create_string_buffer(b"\xa5" * (33 * n + 64), 33 * n + 64)
        assert ctx.lib.zkgpu_tx_verify_wait(bv.h, cid.value, bm, st) == 0
        assert (bm.raw, st.raw[:n]) == (_bitmap(want), want)
        assert st.raw[n: 33 * n] == b"".join(ids) and st.raw[33 * n:] == b"\xa5" * 64
        assert ctx.lib.zkgpu_tx_verify_submit(bv.h, n, blob, offs, 2, C.byref(cid)) == 0
        bv.set_tx_format(0x702)
        bm, st = C.create_string_buffer((n + 7) // 8), C.create_string_buffer(b"\xa5" * (n + 64), n + 64)
        assert ctx.lib.zkgpu_tx_verify_wait(bv.h, cid.value, bm, st) == 0
        assert (bm.raw, st.raw[:n]) == (_bitmap(want), want) and st.raw[n:] == b"\xa5" * 64
    finally:
        bv.close()


def test_a_call_without_the_flag_launches_and_writes_nothing_new(ctx, gens):
    txs = load_tx_fixture()[:128]
    n = len(txs)
    names = {}
    for fmt in (0x301, 0x701):
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
    print("kernels of 0x301:", sorted(names[0x301]))
    assert names[0x301] == names[0x701] and "k_tx_sig_rows" in names[0x301], names
    # an unflagged call given batch status bytes and 64 guard bytes behind them
    blob = b"".join(txs)
    offs = (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:k + 1]) for k in range(n)]))
    bv = _verifier(ctx, gens, 0x301)
    try:
        bm, st = C.create_string_buffer((n + 7) // 8), C.create_string_buffer(b"\xa5" * (n + 64), n + 64)
        assert ctx.lib.zkgpu_tx_verify_batch(bv.h, n, blob, offs, 4, bm, st) == 0
        assert st.raw[:n] == bytes(n) and st.raw[n:] == b"\xa5" * 64
    finally:
        bv.close()
