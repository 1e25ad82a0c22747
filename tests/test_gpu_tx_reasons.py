"""WHY a serialized transaction was rejected (include/zkgpu.h: ZKGPU_TXFORMAT_RECOLLECTED_V1_REASONS, ZKGPU_TXSTATUS_*).

Upstream's Tx::verify returns Result<VerifiedTx, VMError>; with format 2 the status bytes of zkgpu_tx_verify_batch and
zkgpu_tx_verify_submit / _wait carry the reason.  The transactions are built as tests/test_zkvm_tx.py builds them (the
committed fixtures, the product's and the oracle's builders); the oracle only GENERATES -- every expected status byte is
known by construction from the bytes that were damaged:

    truncated transaction                                16   the transaction itself (host)
    proof version byte flipped                           17   R1CSProof malformed
    a proof scalar set to l                              17
    T_1 zeroed (an identity upstream forbids)            17
    a proof point replaced by an undecodable encoding    18   a point does not decode
    a commitment replaced by another valid point         19   the verification equation fails
    t_x incremented                                      19
    R made undecodable                                   21   the signature
    s incremented                                        21
    a bad t_x AND a bad s                                19   precedence: the lowest code
    an opcode outside the subset                          2   not an error of the transaction
"""
import ctypes as C
import hashlib
import json
import os
import struct

import pytest

from gpu_util import L, built_transactions, load_cloak_fixture, load_mixed_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCEPTED, REJECTED, OUTSIDE, TX_INVALID, PROOF_FORMAT, PROOF_POINT, PROOF_EQUATION, KEY, SIGNATURE = 0, 1, 2, 16, 17, 18, 19, 20, 21
CALL = 21                                   # which slice of the proof fixture built_transactions wraps


def _undecodable():
    """an encoding RFC 9496 DECODE rejects, from the committed vectors (canonical as a field element, no point behind it)"""
    with open(os.path.join(ROOT, "tests", "golden", "ristretto255.json")) as f:
        enc = [bytes.fromhex(e["enc"]) for e in json.load(f)["valid_encoding"] if not e["valid"]]
    return next(e for e in enc if e[31] < 0x7f and not e[0] & 1)


def _parts(tx):
    """-> (offset of R | s, offset of the proof bytes)"""
    prog_len = struct.unpack("<I", tx[24:28])[0]
    sig_at = 28 + prog_len
    return sig_at, sig_at + 64 + 4


def _put(tx, at, data):
    return tx[:at] + data + tx[at + len(data):]


def _inc(tx, at):
    v = int.from_bytes(tx[at: at + 32], "little") + 1
    assert v < L
    return _put(tx, at, v.to_bytes(32, "little"))


def truncated(tx):
    return tx[:-1]


def version_flipped(tx):
    _, po = _parts(tx)
    return _put(tx, po, bytes([tx[po] ^ 1]))


def scalar_is_l(tx):                         # t_x_blinding = l: not canonical
    _, po = _parts(tx)
    return _put(tx, po + 1 + 32 * 12, L.to_bytes(32, "little"))


def t1_zeroed(tx):
    _, po = _parts(tx)
    return _put(tx, po + 1 + 32 * 6, bytes(32))


def point_undecodable(tx):                   # T_3
    _, po = _parts(tx)
    return _put(tx, po + 1 + 32 * 7, _undecodable())


def commitment_swapped(tx, mine, other):
    """the first commitment of the cloak (it lies in the program) replaced by another transaction's: a valid point, another
    statement"""
    at = tx.find(mine)
    sig_at, _ = _parts(tx)
    assert 28 <= at < sig_at and mine != other
    return _put(tx, at, other)


def tx_incremented(tx):
    _, po = _parts(tx)
    return _inc(tx, po + 1 + 32 * 11)


def r_undecodable(tx):
    sig_at, _ = _parts(tx)
    return _put(tx, sig_at, _undecodable())


def s_incremented(tx):
    sig_at, _ = _parts(tx)
    return _inc(tx, sig_at + 32)


def unknown_opcode(tx):
    prog_len = struct.unpack("<I", tx[24:28])[0]
    return tx[:24] + struct.pack("<I", prog_len + 1) + tx[28: 28 + prog_len] + b"\x15" + tx[28 + prog_len:]


def _bitmap(status):
    out = bytearray((len(status) + 7) // 8)
    for i, s in enumerate(status):
        if s == ACCEPTED:
            out[i // 8] |= 1 << (i % 8)
    return bytes(out)


def _v1(status):
    return bytes(s if s in (ACCEPTED, OUTSIDE) else REJECTED for s in status)


@pytest.fixture(scope="module")
def ctx():
    from zkvm_amd import Context
    c = Context(0)
    yield c
    c.lib.zkgpu_debug_fail_after(c.h, 0, None)
    c.close()


@pytest.fixture(scope="module")
def gens(ctx):
    from zkvm_amd.verifier import BulletproofGens
    g = BulletproofGens(ctx, 512, table_bits=8)          # (every shape up to 4x4)
    yield g
    g.close()


@pytest.fixture(scope="module")
def block48():
    """48 transactions of 2-in/2-out.  The device sees the ones the VM passes, in order, in groups of 16: transactions 0 .. 15
    are clean, 16 .. 31 hold a single culprit, 32 .. 45 several culprits with different reasons; the two the host itself
    answers (truncated, outside the subset) come last.  -> (transactions, expected status bytes of format 2)"""
    txs, _ = built_transactions(48, call=CALL, bad_every=0)
    recs = load_cloak_fixture()[0]
    com = lambda i: recs[(i + 131 * CALL) % len(recs)][0][:32]                  # noqa: E731
    want = [ACCEPTED] * 48
    damage = {21: (tx_incremented, PROOF_EQUATION),
              33: (version_flipped, PROOF_FORMAT), 34: (scalar_is_l, PROOF_FORMAT), 36: (t1_zeroed, PROOF_FORMAT),
              37: (point_undecodable, PROOF_POINT), 39: (lambda t: commitment_swapped(t, com(39), com(40)), PROOF_EQUATION),
              40: (r_undecodable, SIGNATURE), 42: (s_incremented, SIGNATURE),
              43: (lambda t: s_incremented(tx_incremented(t)), PROOF_EQUATION),
              46: (truncated, TX_INVALID), 47: (unknown_opcode, OUTSIDE)}
    for i, (f, code) in damage.items():
        txs[i] = f(txs[i])
        want[i] = code
    return txs, bytes(want)


def _verifier(ctx, gens, fmt, lanes=3):
    from zkvm_amd.verifier import BlockVerifier
    bv = BlockVerifier(ctx, gens, batches_in_flight=lanes)
    bv.set_tx_format(fmt)
    return bv


def _each_lane(bv, f):
    for i in range(bv.lanes()):
        f(bv.lane(i))


def test_every_rejection_reads_the_reason_its_damage_gives(ctx, gens, block48):
    """(1) the exact status array; the bitmap is format 1's on the same input; 0 stands exactly beside a set bit; the Python
    helper turns the bytes into upstream's error variants"""
    from zkvm_amd.verifier import BlockVerifier, InvalidR1CSProof, InvalidSignature, TxFormatError, tx_errors
    txs, want = block48
    bv = _verifier(ctx, gens, BlockVerifier.TXFORMAT_RECOLLECTED_V1_REASONS)
    try:
        bm, st = bv.verify_txs(txs, host_threads=4)
        print("status", list(st))
        assert st == want
        assert bm == _bitmap(want)
        assert all((s == ACCEPTED) == bool((bm[i // 8] >> (i % 8)) & 1) for i, s in enumerate(st))
        bv.set_tx_format(BlockVerifier.TXFORMAT_RECOLLECTED_V1)
        bm1, st1 = bv.verify_txs(txs, host_threads=4)
        assert bm1 == bm and st1 == _v1(want)
        errs = tx_errors(st)
        assert errs[0] is None and isinstance(errs[46], TxFormatError) and isinstance(errs[40], InvalidSignature)
        assert isinstance(errs[37], InvalidR1CSProof) and errs[37].reason == PROOF_POINT and errs[21].reason == PROOF_EQUATION
        # a call without a status array is the format-1 call: the same bitmap
        bv.set_tx_format(BlockVerifier.TXFORMAT_RECOLLECTED_V1_REASONS)
        blob = b"".join(txs)
        offs = (C.c_uint64 * 49)(*([0] + [sum(len(t) for t in txs[:i + 1]) for i in range(48)]))
        bm2 = C.create_string_buffer(6)
        assert ctx.lib.zkgpu_tx_verify_batch(bv.h, 48, blob, offs, 4, bm2, None) == 0 and bm2.raw == bm
    finally:
        bv.close()


def test_format_1_is_unchanged(ctx, gens, block48):
    """(2) the same input under format 1: only 0, 1 and 2, as before -- synchronous and through submit / wait"""
    from zkvm_amd.verifier import BlockVerifier
    txs, want = block48
    bv = _verifier(ctx, gens, BlockVerifier.TXFORMAT_RECOLLECTED_V1)
    try:
        bm, st = bv.verify_txs(txs, host_threads=4)
        assert set(st) <= {0, 1, 2} and st == _v1(want) and bm == _bitmap(want)
        bm, st = bv.wait_txs(bv.submit_txs(txs, host_threads=4))
        assert st == _v1(want) and bm == _bitmap(want)
    finally:
        bv.close()


def test_reasons_do_not_depend_on_how_the_call_was_batched(ctx, gens, block48):
    """(3) chunks of 16; group checks of 1 and 16; failed groups located (both forms), re-checked one by one, and the
    ungrouped re-run of a batch whose located transaction is made not to account for its group; three calls of 16
    submitted while a round is running and merged by the engine: the same status bytes every time"""
    from zkvm_amd.verifier import BlockVerifier
    txs, want = block48
    bv = _verifier(ctx, gens, BlockVerifier.TXFORMAT_RECOLLECTED_V1_REASONS)
    try:
        def run(label):
            bm, st = bv.verify_txs(txs, host_threads=4)
            print(label, list(st))
            assert st == want and bm == _bitmap(want), label
        bv.set_tx_chunk(16)
        run("chunks of 16")
        bv.set_tx_chunk(0)
        for group in (1, 16):
            _each_lane(bv, lambda c: c.set_group_size(group))
            run("group size %d" % group)
        for mode in (1, 2, 3):
            _each_lane(bv, lambda c: c.set_locate_mode(mode))
            run("locate mode %d" % mode)
        _each_lane(bv, lambda c: c.set_locate_mode(2))
        before = sum(bv.lane(i).force_regroup(True) for i in range(bv.lanes()))
        run("ungrouped re-run")
        after = sum(bv.lane(i).force_regroup(False) for i in range(bv.lanes()))
        assert after > before                                  # (the re-run path was taken, and its reasons are the re-run's)
        _each_lane(bv, lambda c: c.set_locate_mode(0))
        # Three calls of 16 submitted while a round is running (the whole block, submitted first, keeps the engine busy): they
        # wait in the queue together and the engine merges them -- four calls leave in at most two rounds, and every call
        # reads its own part of the round it was merged into.  (Which rounds they turn out to be is the engine's business;
        # a slow host may split them further, so this is tried a few times before it counts as "never merged".)
        merged = False
        for _ in range(4):
            r0, c0 = bv.tx_stats()
            first = bv.submit_txs(txs, host_threads=2)
            ids = [bv.submit_txs(txs[16 * k: 16 * k + 16], host_threads=2) for k in range(3)]
            assert bv.wait_txs(first) == (_bitmap(want), want)
            for k, cid in enumerate(ids):
                bm, st = bv.wait_txs(cid)
                assert st == want[16 * k: 16 * k + 16] and bm == _bitmap(want[16 * k: 16 * k + 16]), ("submit", k)
            r1, c1 = bv.tx_stats()
            assert c1 - c0 == 4
            print("rounds for four calls:", r1 - r0)
            if r1 - r0 <= 2:
                merged = True
                break
        assert merged
    finally:
        _each_lane(bv, lambda c: (c.set_group_size(16), c.set_locate_mode(0), c.force_regroup(False)))
        bv.close()


def test_a_block_of_mixed_arity(ctx, gens, oracle):
    """(4) 1x1, 2x2, 3x3 and 4x4 (the largest shape of the committed fixture) in one call, one damage of each proof reason
    among them and one of the signature's"""
    from zkvm_amd.verifier import BlockVerifier
    fix = load_mixed_fixture()
    shapes = [(1, 1), (2, 2), (3, 3), (4, 4)]
    txs, want = [], []
    for k in range(20):
        a, b = shapes[k % 4]
        com, proof = fix[(a, b)][k // 4]
        txs.append(oracle.tx_wrap_payment(a, b, com, proof, hashlib.sha256(b"reasons mixed %d" % k).digest(), 5, 10 ** 9))
        want.append(ACCEPTED)
    for i, (f, code) in {4: (version_flipped, PROOF_FORMAT), 6: (point_undecodable, PROOF_POINT), 7: (tx_incremented, PROOF_EQUATION),
                         11: (scalar_is_l, PROOF_FORMAT), 13: (s_incremented, SIGNATURE), 14: (t1_zeroed, PROOF_FORMAT)}.items():
        txs[i] = f(txs[i])
        want[i] = code
    want = bytes(want)
    bv = _verifier(ctx, gens, BlockVerifier.TXFORMAT_RECOLLECTED_V1_REASONS)
    try:
        bm, st = bv.verify_txs(txs, host_threads=4)
        print("mixed", list(st))
        assert st == want and bm == _bitmap(want)
        bv.set_tx_format(BlockVerifier.TXFORMAT_RECOLLECTED_V1)
        bm1, st1 = bv.verify_txs(txs, host_threads=4)
        assert bm1 == bm and st1 == _v1(want)
    finally:
        bv.close()


def test_an_error_is_never_a_reason(ctx, gens, block48):
    """(5) fail-closed: ONE runtime call in the middle of a format-2 call is made to report a failure (the library's own
    error-injection gate, zkgpu_debug_fail_after): the call returns an error, every transaction inside the subset reads 1 --
    no reason, no 0 -- and the bitmap is zero; the same verifier then gives the right answer again"""
    from zkvm_amd.verifier import BlockVerifier
    txs, want = block48
    n = len(txs)
    blob = b"".join(txs)
    offs = (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:i + 1]) for i in range(n)]))
    bv = _verifier(ctx, gens, BlockVerifier.TXFORMAT_RECOLLECTED_V1_REASONS)

    def call():
        bm = C.create_string_buffer(b"\xff" * ((n + 7) // 8), (n + 7) // 8)
        st = C.create_string_buffer(b"\x00" * n, n)
        return ctx.lib.zkgpu_tx_verify_batch(bv.h, n, blob, offs, 4, bm, st), bm.raw, st.raw

    try:
        assert call() == (0, _bitmap(want), want)              # (warm: workspaces, stage contexts and arenas exist)
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 10 ** 9, None)   # count a clean call's runtime calls
        assert call() == (0, _bitmap(want), want)
        calls = int(ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None))
        assert calls > 20
        ctx.lib.zkgpu_debug_fail_after(ctx.h, calls // 2, None)
        rc, bm, st = call()
        fired = C.c_longlong(0)
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, C.byref(fired))
        print("runtime calls of a clean call:", calls, "failed call:", calls // 2, "rc", rc, "status", list(st))
        assert fired.value == 1 and rc != 0
        assert bm == bytes((n + 7) // 8)
        assert st == bytes(OUTSIDE if s == OUTSIDE else REJECTED for s in want)
        assert call() == (0, _bitmap(want), want)
    finally:
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None)
        bv.close()
