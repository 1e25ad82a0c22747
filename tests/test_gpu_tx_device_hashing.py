"""ZKGPU_TXFORMAT_HASH_ON_DEVICE: the contract IDs, anchor ratchets and transaction-ID trees of a transaction call computed by
k_tx_hash (csrc/tx_hash_kernels.hpp) instead of on the host's threads.  Verdicts and status bytes must be those of the same
call without the flag, and the oracle's; zkgpu_debug_read("tx_hashed_on_device") tells the device path from a silent host
fallback (it counts on the context, from 0 for every verifier made on it).

The call: 150 transactions of 1-in/1-out, 2-in/2-out, 3-in/2-out and 2-in/3-out in a drawn order -- four shapes, so every
shape's run of lanes is part padding, and more than one wavefront runs -- with, at drawn positions, the damages below.
Expected status bytes are known by construction and held against the oracle's Tx::verify once.
"""
import ctypes as C
import hashlib
import random
import struct
from concurrent.futures import ThreadPoolExecutor

import pytest

from gpu_util import bits, load_cloak_fixture, load_mixed_fixture, load_tx_fixture
from test_gpu_tx_reasons import (ACCEPTED, OUTSIDE, PROOF_EQUATION, PROOF_POINT, REJECTED, SIGNATURE, TX_INVALID, _bitmap, _parts, _put,
                                 _undecodable, _v1, s_incremented, tx_incremented, unknown_opcode)

pytestmark = pytest.mark.gpu
FLAG = 0x100
N = 150


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
    g = BulletproofGens(ctx, 512, table_bits=8)
    yield g
    g.close()


def predicate_flipped(tx):
    """a byte of the LAST output predicate pushed (it ends 5 bytes before the program does: push:32:pred output:1)"""
    sig_at, _ = _parts(tx)
    at = sig_at - 5 - 7
    return _put(tx, at, bytes([tx[at] ^ 0x40]))


def mintime_flipped(tx):
    return _put(tx, 8, bytes([tx[8] ^ 1]))


def commitment_undecodable(tx, com32):
    at = tx.find(com32)
    assert 28 <= at < _parts(tx)[0]
    return _put(tx, at, _undecodable())


def program_truncated(tx):
    return tx[:60]


@pytest.fixture(scope="module")
def block150(oracle):
    """-> (transactions, expected status bytes of format 2)"""
    rng = random.Random(150)
    fix = load_mixed_fixture()
    recs22 = load_cloak_fixture()[0]
    proved = {}
    for shape in ((3, 2), (2, 3)):
        com, proofs = oracle.cloak_prove_batch(8, shape[0], shape[1], hashlib.sha256(b"hashing %d%d" % shape).digest(), threads=8)
        w = 64 * sum(shape)
        proved[shape] = [(com[w * i: w * (i + 1)], proofs[i]) for i in range(8)]
    shapes = [(1, 1)] * 40 + [(2, 2)] * 80 + [(3, 2)] * 15 + [(2, 3)] * 15
    rng.shuffle(shapes)
    txs, coms = [], []
    for k, (a, b) in enumerate(shapes):
        pool = recs22 if (a, b) == (2, 2) else fix[(1, 1)] if (a, b) == (1, 1) else proved[(a, b)]
        com, proof = pool[k % len(pool)][:2]
        txs.append(oracle.tx_wrap_payment(a, b, com, proof, hashlib.sha256(b"hashing tx %d" % k).digest(), 5 + k, 10 ** 9))
        coms.append(com[:32])
    want = [ACCEPTED] * N
    where = rng.sample(range(N), 7)
    damage = [(predicate_flipped, SIGNATURE), (mintime_flipped, SIGNATURE), (s_incremented, SIGNATURE), (tx_incremented, PROOF_EQUATION),
              (None, PROOF_POINT), (program_truncated, TX_INVALID), (unknown_opcode, OUTSIDE)]
    for i, (f, code) in zip(where, damage):
        txs[i] = f(txs[i]) if f else commitment_undecodable(txs[i], coms[i])
        want[i] = code
    want = bytes(want)
    with ThreadPoolExecutor(8) as pool:
        verdicts = list(pool.map(lambda t: oracle.tx_verify(t, bytes(range(64))), txs))
    assert bytes(verdicts) == _v1(want)
    return txs, want


def _verifier(ctx, gens, fmt):
    from zkvm_amd.verifier import BlockVerifier
    bv = BlockVerifier(ctx, gens, batches_in_flight=3)
    bv.set_tx_format(fmt)
    return bv


def _hashed(ctx):
    return struct.unpack("<Q", ctx.debug_read("tx_hashed_on_device", 8))[0]


def _inside_second_pass(want):
    return sum(1 for s in want if s not in (OUTSIDE, TX_INVALID))


def test_format_values(ctx, gens):
    from zkvm_amd import TXFORMAT_HASH_ON_DEVICE
    from zkvm_amd.verifier import BlockVerifier
    assert TXFORMAT_HASH_ON_DEVICE == BlockVerifier.TXFORMAT_HASH_ON_DEVICE == FLAG
    bv = _verifier(ctx, gens, 0)
    try:
        for fmt in (0x101, 0x102, 1, 2, 0):
            assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, fmt) == 0, hex(fmt)
        for fmt in (0x100, 0x103, 0x201, 3):
            assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, fmt) == -1, hex(fmt)
    finally:
        bv.close()


def test_a_lone_call_chunks_one_host_thread_and_two_calls_in_a_round(ctx, gens, block150):
    """the flagged verifier first (its counter is read), then the unflagged one on the same context (its counter stays 0)"""
    txs, want = block150
    got = {}
    for fmt in (0x102, 2):
        bv = _verifier(ctx, gens, fmt)
        try:
            assert _hashed(ctx) == 0
            got[fmt] = bv.verify_txs(txs, host_threads=4)
            print(hex(fmt), "status", list(got[fmt][1]))
            assert got[fmt] == (_bitmap(want), want)
            live = _inside_second_pass(want)
            assert _hashed(ctx) == (live if fmt & FLAG else 0)
            bv.set_tx_format(fmt - 1)                                         # 0x101 against 1
            assert bv.verify_txs(txs, host_threads=4) == (_bitmap(want), _v1(want))
            bv.set_tx_format(fmt)
            bv.set_tx_chunk(64)                                               # three chunks, the last a remainder
            assert bv.verify_txs(txs, host_threads=4) == got[fmt]
            bv.set_tx_chunk(0)
            assert bv.verify_txs(txs, host_threads=1) == got[fmt]
            before = _hashed(ctx)
            a, b = bv.submit_txs(txs[:70], host_threads=2), bv.submit_txs(txs[70:], host_threads=2)
            rb, ra = bv.wait_txs(b), bv.wait_txs(a)                           # waited in reverse order
            assert ra == bv.verify_txs(txs[:70], host_threads=2) == (_bitmap(want[:70]), want[:70])
            assert rb == bv.verify_txs(txs[70:], host_threads=2) == (_bitmap(want[70:]), want[70:])
            assert _hashed(ctx) - before == (2 * live if fmt & FLAG else 0)
        finally:
            bv.close()
    assert got[0x102] == got[2]


def test_the_committed_fixture(ctx, gens):
    txs = load_tx_fixture()
    out = {}
    for fmt in (0x101, 1):
        bv = _verifier(ctx, gens, fmt)
        try:
            out[fmt] = bv.verify_txs(txs, host_threads=4)
            assert _hashed(ctx) == (len(txs) if fmt & FLAG else 0)
        finally:
            bv.close()
    assert out[0x101] == out[1] and bits(out[1][0], len(txs)) == [1] * len(txs)


def test_an_error_of_the_hashing_stage_fails_the_call_closed(ctx, gens, block150):
    """zkgpu_debug_fail_after makes the n-th runtime call of the library answer "failed" on the host (nothing faults on the
    device).  n walks through a warm 24-transaction call until the failing call is one of the hashing stage (the verifier's
    error text names the stage).  For EVERY n: an error gives a zero bitmap, status 1 for every transaction inside the subset
    and 2 left alone; no error gives the right answer.  Then a clean call on the same verifier is right."""
    txs, want = block150
    pick = list(dict.fromkeys([i for i, s in enumerate(want) if s == OUTSIDE] + list(range(23))))
    txs, want = [txs[i] for i in pick], bytes(want[i] for i in pick)
    n = len(txs)
    blob = b"".join(txs)
    offs = (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:i + 1]) for i in range(n)]))
    bv = _verifier(ctx, gens, 0x102)

    def call():
        bm = C.create_string_buffer(b"\xff" * ((n + 7) // 8), (n + 7) // 8)
        st = C.create_string_buffer(b"\x00" * n, n)
        return ctx.lib.zkgpu_tx_verify_batch(bv.h, n, blob, offs, 2, bm, st), bm.raw, st.raw

    try:
        good = (0, _bitmap(want), want)
        assert call() == good and call() == good                             # (warm: every buffer of the stage exists)
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 10 ** 9, None)
        assert call() == good
        calls = int(ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None))
        hit = None
        for k in range(1, calls + 1):
            ctx.lib.zkgpu_debug_fail_after(ctx.h, k, None)
            rc, bm, st = call()
            ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None)
            if rc == 0:
                assert (rc, bm, st) == good, k
                continue
            assert bm == bytes((n + 7) // 8) and st == bytes(OUTSIDE if s == OUTSIDE else REJECTED for s in want), k
            if b"transaction-ID hashing stage" in ctx.lib.zkgpu_verifier_last_error(bv.h):
                hit = k
                break
        print("runtime calls of a clean call:", calls, "the hashing stage's first:", hit)
        assert hit is not None
        assert call() == good
    finally:
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None)
        bv.close()
