"""ZKGPU_TXFORMAT_PRECOMPUTE_ONLY (0x2000) on the device: upstream's Tx::precompute -- the VM, the transaction ID and the log,
NOTHING verified.  The accept bitmap is written and all zero; a transaction the VM ran to the end reads status 3 beside its ID
and its log record, and a 3 is not a verdict.

  1. equality with verifying calls: 2-in/2-out payments around the proofs of tests/golden/cloak_2x2_proofs.bin at call sizes
     1, 5, 63, 64, 65, 130 under 0x2401 (the host hashes; the device is not touched) and 0x2501 (one hashing launch);
  2. both hashing kernels over a call of mixed shapes, in fresh processes chosen by ZKGPU_TX_HASH_LEVELS: byte-identical, equal
     to the host path, and pinned by the oracle through tests/tx_log_util.py;
  3. what a precompute call does not look at -- signature, key, proof, commitment -- and what it does;
  4. submitted calls: precompute-only and verifying calls queued alternately from two threads, each under the layout and the
     format it was queued with, and never two in a round; a NULL status argument;
  5. fail-closed at every runtime call of a 0x2501 call (the software gate zkgpu_debug_fail_after: nothing faults).
"""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys
import threading

import pytest

from gpu_util import bits, load_cloak_fixture
from test_gpu_tx_reasons import _parts, _put, _undecodable, tx_incremented, unknown_opcode, version_flipped
from test_gpu_tx_sign_on_device import key_undecodable, r_flipped
from tx_log_util import check_accepted, record_bytes
from tx_precompute_child import MIXED_SHAPES, PER_SHAPE, WINDOWS, mixed_corpus, raw_precompute

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE, HASH, IDS = 0x2000, 0x100, 0x400
PRECOMPUTED, ZERO = 3, bytes(32)
SIZES = (1, 5, 63, 64, 65, 130)


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
    g = BulletproofGens(ctx, 256, table_bits=8)              # (the smallest the 2-in/2-out fixtures allow)
    yield g
    g.close()


@pytest.fixture(scope="module")
def payments(oracle):
    """130 valid signed 2-in/2-out payments around the committed proofs, and the oracle's ID of each (computed once)"""
    recs = load_cloak_fixture("cloak_2x2_proofs.bin")[0]
    txs = [oracle.tx_wrap_payment(2, 2, recs[k % len(recs)][0], recs[k % len(recs)][1], hashlib.sha256(b"precompute %d" % k).digest(), 3 + k, 10 ** 9)
           for k in range(max(SIZES))]
    ids = []
    for t in txs:
        rc, txid, _, _ = oracle.tx_id(t)
        assert rc == 0
        ids.append(txid)
    return txs, ids


def _verifier(ctx, gens, fmt, log_k=0):
    from zkvm_amd.verifier import BlockVerifier
    bv = BlockVerifier(ctx, gens, batches_in_flight=3)
    bv.set_tx_format(fmt, log_k=log_k)
    return bv


def _read(ctx, what):
    return struct.unpack("<Q", ctx.debug_read(what, 8))[0]


def _profiled(ctx, call):
    ctx.profile(True)
    ctx.profile_reset()
    try:
        out = call()
        return out, set(ctx.profile_read())
    finally:
        ctx.profile(False)
        ctx.profile_reset()


def test_the_flag_is_accepted_exactly_where_the_rule_says(ctx, gens):
    """(fails on the parent commit, where every word with 0x2000 is ZKGPU_EINVAL)"""
    bv = _verifier(ctx, gens, 0)
    try:
        for fmt in (0x2401, 0x2402, 0x2501, 0x2502, 0x2401 | 0x800 | (4 << 16), 0x2502 | 0x800 | (255 << 16)):
            assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, fmt) == 0, hex(fmt)
        for fmt in (0x2000, 0x2400, 0x2001, 0x2101, 0x2701, 0x2601, 0x2403, 0x2401 | (4 << 16), 0x2001 | 0x800 | (4 << 16), 0x3401, 0x6401):
            assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, fmt) == -1, hex(fmt)
    finally:
        bv.close()


def test_ids_equal_those_of_verifying_calls_and_the_oracle(ctx, gens, payments):
    txs, want_ids = payments
    bv = _verifier(ctx, gens, 0x2501)
    try:
        bv.precompute_txs(txs[:8], host_threads=4)                                         # (warm: the stage contexts are made)
        assert (_read(ctx, "tx_precomputed"), _read(ctx, "tx_hashed_on_device")) == (8, 8)
        done = hashed = 8
        for n in SIZES:
            part, got = txs[:n], {}
            for fmt in (0x2401, 0x2501):
                bv.set_tx_format(fmt)
                (rc, bm, st, ids, _), kernels = _profiled(ctx, lambda: raw_precompute(ctx, bv, part, 0))
                assert rc == 0 and bm == bytes((n + 7) // 8) and st == bytes([PRECOMPUTED]) * n, (n, hex(fmt), list(st))
                assert ids == want_ids[:n], (n, hex(fmt))
                # the launches: under 0x2501 the one hashing kernel, under 0x2401 none at all
                assert len(kernels) == (1 if fmt & HASH else 0) and kernels <= {"k_tx_hash", "k_tx_hash_levels"}, (n, hex(fmt), kernels)
                done += n
                hashed += n if fmt & HASH else 0
                assert (_read(ctx, "tx_precomputed"), _read(ctx, "tx_hashed_on_device")) == (done, hashed), (n, hex(fmt))
                got[fmt] = (st, ids)
                assert bv.precompute_txs(part, host_threads=1) == (st, ids, None)                # (the Python method: the same)
                done += n
                hashed += n if fmt & HASH else 0
            assert got[0x2401] == got[0x2501]
            for fmt in (0x401, 0x501):                                                          # the same bytes, verified
                bv.set_tx_format(fmt)
                bm, st, ids = bv.verify_txs(part, host_threads=4, ids=True)
                assert st == bytes(n) and ids == want_ids[:n], (n, hex(fmt))
                hashed += n if fmt & HASH else 0
            assert (_read(ctx, "tx_precomputed"), _read(ctx, "tx_hashed_on_device")) == (done, hashed), n
    finally:
        bv.close()


def test_both_kernels_over_mixed_shapes_in_fresh_processes(ctx, gens, oracle, tmp_path):
    """tests/tx_precompute_child.py, once with k_tx_hash_levels and once with k_tx_hash: the same bytes; here, the host path"""
    txs = mixed_corpus(oracle)
    n = len(txs)
    assert n == len(MIXED_SHAPES) * PER_SHAPE
    got = {}
    for levels in ("1", "0"):
        out = tmp_path / ("levels%s.json" % levels)
        env = dict(os.environ, ZKGPU_TX_HASH_LEVELS=levels)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tx_precompute_child.py"), str(out)], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (levels, r.stdout[-1000:], r.stderr[-3000:])
        got[levels] = json.load(open(out))
    for k in WINDOWS:
        a, b = got["1"][str(k)], got["0"][str(k)]
        assert a["kernels"] == ["k_tx_hash_levels", "k_tx_log_gather"] and b["kernels"] == ["k_tx_hash", "k_tx_log_gather"], (a["kernels"], b["kernels"])
        assert {q: a[q] for q in a if q != "kernels"} == {q: b[q] for q in b if q != "kernels"}, k
        assert a["rc"] == 0 and bytes.fromhex(a["bitmap"]) == bytes((n + 7) // 8) and bytes.fromhex(a["status"]) == bytes([PRECOMPUTED]) * n
    bv = _verifier(ctx, gens, 0x2401)
    try:
        counts = set()
        for k in WINDOWS:
            bv.set_tx_format(0x2401, log_k=k)
            rc, bm, st, ids, recs = raw_precompute(ctx, bv, txs, k)                           # the host path
            a = got["1"][str(k)]
            assert (rc, bm.hex(), st.hex(), [i.hex() for i in ids], [r.hex() for r in recs]) == (0, a["bitmap"], a["status"], a["ids"], a["records"]), k
            for i, t in enumerate(txs):
                count = check_accepted(oracle, t, ids[i], recs[i], k)
                counts.add(count)
                if count > k:
                    assert recs[i] == bytes([count]) + bytes(33 * k)                           # the count alone
        assert counts == {a + b for a, b in MIXED_SHAPES} and max(counts) == 17
    finally:
        bv.close()


def commitment_undecodable(tx, com32):
    at = tx.find(com32)
    assert 28 <= at < _parts(tx)[0]
    return _put(tx, at, _undecodable())


def test_what_a_precompute_call_does_not_look_at(ctx, gens, oracle, payments):
    txs, want_ids = payments
    txs, want_ids = list(txs[:24]), list(want_ids[:24])
    recs = load_cloak_fixture("cloak_2x2_proofs.bin")[0]
    # what only verification sees: still 3.  Signature and proof lie outside what the ID covers: the ID is unchanged;
    # a key and a commitment lie in the program: the ID is the oracle's for the damaged bytes
    unseen = {2: (r_flipped, (21,)), 5: (key_undecodable, (20,)), 9: (version_flipped, (17,)), 11: (tx_incremented, (19,)),
              14: (lambda t: commitment_undecodable(t, recs[14 % len(recs)][0][:32]), (17, 18, 19))}
    for i, (damage, _) in unseen.items():
        txs[i] = damage(txs[i])
        rc, txid, _, _ = oracle.tx_id(txs[i])
        assert rc == 0 and (txid == want_ids[i]) == (i in (2, 9, 11)), i
        want_ids[i] = txid
    # what the host VM finds: a truncated program, time bounds the wrong way round, a non-canonical s; and outside the subset
    txs[3] = txs[3][:60]
    txs[7] = _put(txs[7], 8, (2 ** 63).to_bytes(8, "little"))
    sig_at = _parts(txs[16])[0]
    txs[16] = _put(txs[16], sig_at + 32, b"\xff" * 32)
    txs[20] = unknown_opcode(txs[20])
    n = len(txs)
    host_found = {3: 16, 7: 16, 16: 21}
    bv = _verifier(ctx, gens, 0x2402)
    try:
        for fmt in (0x2402, 0x2502, 0x2401, 0x2501):
            bv.set_tx_format(fmt)
            rc, bm, st, ids, _ = raw_precompute(ctx, bv, txs, 0)
            assert rc == 0 and bm == bytes((n + 7) // 8)
            for i in range(n):
                if i in host_found:
                    assert st[i] == (host_found[i] if fmt & 2 else 1) and ids[i] == ZERO, (hex(fmt), i, st[i])
                elif i == 20:
                    assert st[i] == 2 and ids[i] == ZERO, (hex(fmt), i)
                else:
                    assert st[i] == PRECOMPUTED and ids[i] == want_ids[i], (hex(fmt), i, st[i])
        bv.set_tx_format(0x402)                                                               # the same transactions, verified
        bm, st, ids = bv.verify_txs(txs, host_threads=4, ids=True)
        for i in range(n):
            if i in unseen:
                assert st[i] in unseen[i][1] and ids[i] == ZERO, (i, st[i])
            elif i in host_found:
                assert st[i] == host_found[i], (i, st[i])
            elif i == 20:
                assert st[i] == 2
            else:
                assert st[i] == 0 and ids[i] == want_ids[i], (i, st[i])
    finally:
        bv.close()


def test_submitted_calls_of_both_kinds_from_two_threads(ctx, gens, payments):
    """one thread queues precompute-only calls (0x2501 with a window of 5), the other verifying ones (0x401), in STRICT alternation
    P, V, P, V, ... -- a turn counter under a condition: each thread sets its format and submits only on its turn (the format is
    the verifier's).  Whatever is queued at any moment therefore alternates in kind, and an engine that takes only calls of one
    kind into a round can never put two of them together: zkgpu_tx_verify_stats must show as many rounds as calls.  An engine
    that mixed kinds would show fewer -- and hand a call the other kind's outputs.  Every call comes back under the layout and
    the kind it was queued with"""
    txs, want_ids = payments
    bv = _verifier(ctx, gens, 0x401)
    parts = [(0, 40), (40, 65), (65, 130), (10, 74)]
    try:
        rounds0, calls0 = bv.tx_stats()
        done0 = _read(ctx, "tx_precomputed")
        turn, state, queued, errors = threading.Condition(), {"next": 0}, {"pre": [], "ver": []}, []

        def submit(kind, parity):
            try:
                for q, (lo, hi) in enumerate(parts):
                    with turn:
                        assert turn.wait_for(lambda: state["next"] == 2 * q + parity or errors, timeout=60)
                        if errors:
                            return
                        if kind == "pre":
                            bv.set_tx_format(0x2501, log_k=5)
                        else:
                            bv.set_tx_format(0x401)
                        queued[kind].append((bv.submit_txs(txs[lo:hi], host_threads=2), lo, hi, state["next"]))
                        state["next"] += 1
                        turn.notify_all()
            except BaseException as e:                                                        # noqa: BLE001
                with turn:
                    errors.append(e)
                    turn.notify_all()

        threads = [threading.Thread(target=submit, args=(kind, parity)) for parity, kind in enumerate(("pre", "ver"))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        # the order of submission was P, V, P, V, ...
        assert [q[3] for q in queued["pre"]] == [0, 2, 4, 6] and [q[3] for q in queued["ver"]] == [1, 3, 5, 7]
        for cid, lo, hi, _ in queued["ver"]:
            with pytest.raises(ValueError):
                bv.wait_precomputed(cid)
            bm, st, ids = bv.wait_txs(cid, ids=True)
            assert bits(bm, hi - lo) == [1] * (hi - lo)
            assert st == bytes(hi - lo) and ids == want_ids[lo:hi]
        for cid, lo, hi, _ in queued["pre"]:
            with pytest.raises(ValueError):
                bv.wait_txs(cid)
            st, ids, logs = bv.wait_precomputed(cid)
            assert st == bytes([PRECOMPUTED]) * (hi - lo) and ids == want_ids[lo:hi]
            assert all(isinstance(e, list) and sorted(a for a, _ in e) == ["input", "input", "output", "output"] for e in logs)
        rounds, calls = bv.tx_stats()
        assert calls - calls0 == 2 * len(parts)
        assert rounds - rounds0 == calls - calls0, "a round held two calls: of kinds that alternate, so it held both kinds"
        assert _read(ctx, "tx_precomputed") - done0 == sum(hi - lo for lo, hi in parts)
    finally:
        bv.close()


def test_a_submitted_precompute_call_keeps_the_format_it_was_queued_under(ctx, gens, payments):
    """queued under 0x2502 and the format changed to 0x401 at once -- before or after the engine starts the round, whichever
    thread is quicker --: the call still reports format 2's codes (16, 21), still verifies nothing, and its IDs still come from
    the device"""
    txs, want_ids = payments
    txs, want_ids = list(txs[:20]), list(want_ids[:20])
    txs[4] = txs[4][:60]
    txs[11] = _put(txs[11], _parts(txs[11])[0] + 32, b"\xff" * 32)
    want = bytes(16 if i == 4 else 21 if i == 11 else PRECOMPUTED for i in range(20))
    bv = _verifier(ctx, gens, 0x2502)
    try:
        for _ in range(3):
            bv.set_tx_format(0x2502)
            hashed0 = _read(ctx, "tx_hashed_on_device")
            cid = bv.submit_txs(txs, host_threads=2)
            bv.set_tx_format(0x401)
            st, ids, logs = bv.wait_precomputed(cid)
            assert st == want and logs is None
            assert ids == [ZERO if i in (4, 11) else want_ids[i] for i in range(20)]
            assert _read(ctx, "tx_hashed_on_device") - hashed0 == 18
    finally:
        bv.close()


def test_no_status_argument_only_zeroes_the_bitmap(ctx, gens, payments):
    """status == NULL stays legal under the flag: there is nowhere to put what the call computes, so a lone call zeroes the bitmap
    and computes nothing (the counter does not move); a submitted call waited for without one gets its zero bitmap"""
    txs = payments[0][:21]
    n = len(txs)
    offs = (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:i + 1]) for i in range(n)]))
    blob = b"".join(txs)
    for fmt in (0x2401, 0x2502):
        bv = _verifier(ctx, gens, fmt)
        try:
            done0 = _read(ctx, "tx_precomputed")
            bm = C.create_string_buffer(b"\xff" * 3, 3)
            assert ctx.lib.zkgpu_tx_verify_batch(bv.h, n, blob, offs, 2, bm, None) == 0
            assert bm.raw == bytes(3) and _read(ctx, "tx_precomputed") == done0
            cid = C.c_uint64(0)
            assert ctx.lib.zkgpu_tx_verify_submit(bv.h, n, blob, offs, 2, C.byref(cid)) == 0
            bm = C.create_string_buffer(b"\xff" * 3, 3)
            assert ctx.lib.zkgpu_tx_verify_wait(bv.h, cid.value, bm, None) == 0
            assert bm.raw == bytes(3)
        finally:
            bv.close()


def test_a_failure_of_any_runtime_call_fails_the_call_closed(ctx, gens, payments):
    """zkgpu_debug_fail_after makes the n-th runtime call of the library answer "failed" on the host (nothing faults on the
    device).  n walks through every runtime call of a warm 0x2501 call of 65 transactions with a window of 5: every one of them,
    failed, ends the call with an error, a zero bitmap, status 1 everywhere, no ID, no record; the clean call after it is right"""
    txs, want_ids = payments
    txs, want_ids = txs[:65], want_ids[:65]
    n, k = 65, 5
    bv = _verifier(ctx, gens, 0x2501, log_k=k)
    try:
        good = raw_precompute(ctx, bv, txs, k, threads=2)
        assert good[:4] == (0, bytes((n + 7) // 8), bytes([PRECOMPUTED]) * n, want_ids) and good == raw_precompute(ctx, bv, txs, k, threads=2)   # (warm)
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 10 ** 9, None)
        assert raw_precompute(ctx, bv, txs, k, threads=2) == good
        calls = int(ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None))
        # the tape up, the launch, the IDs down, the table up, the gather, the records down, the wait: at the least
        assert 7 <= calls <= 40, calls
        for q in range(1, calls + 1):
            ctx.lib.zkgpu_debug_fail_after(ctx.h, q, None)
            out = raw_precompute(ctx, bv, txs, k, threads=2)
            fired = C.c_longlong(-1)
            ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, C.byref(fired))
            assert fired.value == 1, (q, fired.value)
            assert out[0] != 0 and out[1] == bytes((n + 7) // 8) and out[2] == bytes([1]) * n, q
            assert out[3] == [ZERO] * n and out[4] == [bytes(record_bytes(k))] * n, q
            assert raw_precompute(ctx, bv, txs, k, threads=2) == good, q                      # the verifier is usable afterwards
        print("runtime calls of a clean precompute-only call with device hashing:", calls)
    finally:
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None)
        bv.close()
