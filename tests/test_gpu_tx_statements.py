"""ZKGPU_TXFORMAT_STATEMENTS_V1 (4) and 4 | ZKGPU_TXFORMAT_SIGN_ON_DEVICE (0x204) on the device: upstream's PrecomputedTx::verify
behind the caller's own VM -- records of (txid, R, s, keys, commitments, proof) in, verdicts out.  Under 0x204 the MuSig
coefficients come from k_musig_rows (csrc/tx_musig_rows.hpp) and the challenge from k_tx_sig_rows; no transcript runs on the host.

  1. the word is accepted exactly where the rule says, and a refused word leaves the format in force;
  2. parity: 65 payments, damaged where a record carries the bytes, as transactions under format 2 and as records under 4 and
     0x204 -- the same bits and status bytes, and the oracle's verdicts; the counters move by the row count under 0x204 only;
  3. many keys, independent of the product's VM: records this file signs itself around one fixture proof, 1 .. 17, 32 and 64
     keys, calls of 1, 63, 64, 65 and 129 records, seven kinds of damage per call, expected verdicts from the oracle's primitives;
  4. malformed and unservable records inside a good call; status == NULL;
  5. submitted calls from two threads interleaved with format-2 calls: each keeps what it was queued under, rounds never mix;
     neighbours under one word are merged, a call under the other word runs alone;
  6. fail-closed at every runtime call of one 0x204 call (the software gate zkgpu_debug_fail_after: nothing faults).
"""
import ctypes as C
import hashlib
import struct
import threading

import pytest

from gpu_util import bits, load_mixed_fixture
from test_gpu_tx_reasons import (_parts, _put, _undecodable, commitment_swapped, point_undecodable, r_undecodable, s_incremented, scalar_is_l, t1_zeroed,
                                 tx_incremented, version_flipped)
from tx_statements_util import L, Signer, fields_of_payment, pack, signature_holds

pytestmark = pytest.mark.gpu
STATEMENTS, SIGN = 4, 0x200
KEY_COUNTS = list(range(1, 18)) + [32, 64]
SHAPES = [(1, 1), (2, 2), (1, 2)]
R_BYTES = bytes(range(64))


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


def _verifier(ctx, gens, fmt=0):
    from zkvm_amd.verifier import BlockVerifier
    bv = BlockVerifier(ctx, gens, batches_in_flight=3)
    bv.set_tx_format(fmt)
    return bv


def _read(ctx, what):
    return struct.unpack("<Q", ctx.debug_read(what, 8))[0]


def key_undecodable(tx):                     # the predicate of the first input's contract: push:133:(anchor:32 key:32 ...)
    return _put(tx, 28 + 5 + 32, _undecodable())


def s_is_l(tx):
    return _put(tx, _parts(tx)[0] + 32, L.to_bytes(32, "little"))


@pytest.fixture(scope="module")
def payments(oracle):
    """65 signed payments of 1x1, 2x2 and 1x2 around the committed proofs -- one more than a 64-lane block --, some damaged in
    bytes a record carries (proof, commitment, key, R, s) -> (transactions, their records, the oracle's verdict of each)"""
    fx = load_mixed_fixture()
    txs = []
    for k in range(65):
        n_in, n_out = SHAPES[k % 3]
        com, proof = fx[(n_in, n_out)][(k // 3) % len(fx[(n_in, n_out)])]
        txs.append(oracle.tx_wrap_payment(n_in, n_out, com, proof, hashlib.sha256(b"statements %d" % k).digest(), 3 + k, 10 ** 9))
        assert txs[-1]
    first_com = lambda k: fx[SHAPES[k % 3]][(k // 3) % len(fx[SHAPES[k % 3]])][0][:32]      # noqa: E731
    damage = {5: tx_incremented, 9: version_flipped, 13: scalar_is_l, 20: t1_zeroed, 22: point_undecodable,
              27: lambda t: commitment_swapped(t, first_com(27), first_com(30)), 31: r_undecodable, 38: s_incremented, 41: key_undecodable,
              44: s_is_l, 50: lambda t: s_incremented(tx_incremented(t)), 57: lambda t: key_undecodable(r_undecodable(t)), 64: s_incremented}
    for i, f in damage.items():
        txs[i] = f(txs[i])
    recs = [pack(**fields_of_payment(oracle, t)) for t in txs]
    verdicts = [oracle.tx_verify(t, R_BYTES) for t in txs]
    assert [i for i, v in enumerate(verdicts) if v] == sorted(damage) and all(v in (0, 1) for v in verdicts)
    return txs, recs, verdicts


def test_the_word_is_accepted_exactly_where_the_rule_says(ctx, gens, payments):
    from zkvm_amd import ZkGpuError
    txs, recs, _ = payments
    bv = _verifier(ctx, gens)
    try:
        for fmt in (STATEMENTS, STATEMENTS | SIGN):
            bv.set_tx_format(fmt)
        for base, probe, lengths in ((STATEMENTS | SIGN, recs[0], [len(recs[0])]), (2, txs[0], [len(txs[0])])):
            bv.set_tx_format(base)
            for bad in (STATEMENTS | 0x100, STATEMENTS | 0x300, STATEMENTS | 0x400, STATEMENTS | 0x400 | 0x800 | (3 << 16), STATEMENTS | (1 << 16), STATEMENTS | 0x2000,
                        STATEMENTS | 0x2400, 3, 5, 6, 0x200, 0x201):
                with pytest.raises(ZkGpuError):
                    bv._check(bv.lib.zkgpu_verifier_set_tx_format(bv.h, bad))
                bm, st = bv._tx_call(probe, lengths, 2)      # the format in force is the one set last: its bytes are still accepted
                assert st.raw[:1] == b"\x00" and bm.raw[0] == 1, (hex(base), hex(bad))
    finally:
        bv.close()


def test_records_read_what_format_2_reads_for_their_transactions(ctx, gens, payments):
    txs, recs, verdicts = payments
    n = len(txs)
    bv = _verifier(ctx, gens, 2)
    try:
        bm2, st2 = bv.verify_txs(txs, host_threads=4)
        print("status", list(st2))
        assert [int(s != 0) for s in st2] == verdicts and bits(bm2, n) == [1 - v for v in verdicts]
        assert [st2[i] for i in (5, 9, 13, 20, 22, 27, 31, 38, 41, 44, 50, 57, 64)] == [19, 17, 17, 17, 18, 19, 21, 21, 20, 21, 19, 20, 21]
        for on_device in (False, True):
            musig0, signed0 = _read(ctx, "tx_musig_on_device"), _read(ctx, "tx_signed_on_device")
            bm, st = bv.verify_statements(recs, host_threads=4, on_device=on_device)
            assert (bm, st) == (bm2, st2), (on_device, list(st))
            # (rows: every record the host lets through -- all but the one whose s is not canonical)
            moved = (_read(ctx, "tx_musig_on_device") - musig0, _read(ctx, "tx_signed_on_device") - signed0)
            assert moved == ((n - 1, n - 1) if on_device else (0, 0)), (on_device, moved)
            # one stage per chunk and several chunks: the same bytes
            bv.set_tx_chunk(16)
            assert bv.verify_statements(recs, host_threads=2, on_device=on_device) == (bm2, st2)
            bv.set_tx_chunk(0)
            # verify_statements put the format back: transactions are still read as transactions
            assert bv.verify_txs(txs[:7], host_threads=2) == (bytes([bm2[0] & 0x7f]), st2[:7])
    finally:
        bv.close()


@pytest.fixture(scope="module")
def signed(oracle):
    """129 records this file signs itself around ONE 1x1 fixture proof, record i under KEY_COUNTS[i % 19] keys -> (fields, signers)"""
    com, proof = load_mixed_fixture()[(1, 1)][0]
    signers = {k: Signer(oracle, b"%d" % k, k) for k in KEY_COUNTS}
    fs = []
    for i in range(129):
        k = KEY_COUNTS[i % len(KEY_COUNTS)]
        txid = hashlib.sha256(b"signed record %d" % i).digest()
        R, s = signers[k].sign(txid, i)
        fs.append(dict(txid=txid, R=R, s=s, keys=list(signers[k].X), n_in=1, n_out=1, commitments=com, proof=proof))
    return fs, signers


def test_many_keys_signed_by_the_test_itself(ctx, gens, oracle, signed):
    fs, signers = signed
    spare = Signer(oracle, b"spare", 2)
    clean = {}

    def expected(f):
        why = signature_holds(oracle, f["txid"], f["R"], f["s"], f["keys"])
        return 0 if why is None else 20 if why == "key" else 21

    bv = _verifier(ctx, gens)
    try:
        for n in (1, 63, 64, 65, 129):
            call = [dict(f, keys=list(f["keys"])) for f in fs[:n]]
            # one of each per call, at places that move with the call's size; a call of one record takes the first kind only
            at = lambda q: (n * (2 * q + 1)) // 15      # noqa: E731
            if n > 1:
                i = next(j for j in range(at(0), n) if len(call[j]["keys"]) >= 2)
                call[i]["keys"] = call[i]["keys"][1:] + call[i]["keys"][:1]                      # keys permuted
                call[at(1)]["keys"][-1] = spare.X[0]                                              # one key swapped for another valid key
                call[at(2)]["txid"] = bytes([call[at(2)]["txid"][0] ^ 1]) + call[at(2)]["txid"][1:]      # one txid bit flipped
                call[at(3)]["s"] = ((int.from_bytes(call[at(3)]["s"], "little") + 1) % L).to_bytes(32, "little")
                call[at(4)]["R"] = spare.X[1]                                                     # R replaced by a valid other point
                call[at(5)]["keys"][0] = _undecodable()                                           # a key that is no encoding -> 20
                call[at(6)]["R"] = _undecodable()                                                 # an R that is none -> 21
                damaged = {i} | {at(q) for q in range(1, 7)}
                assert len(damaged) == 7
            else:
                call[0]["keys"][0] = _undecodable()
                damaged = {0}
            want = []
            for j, f in enumerate(call):
                if j in damaged:
                    want.append(expected(f))
                else:
                    if j not in clean:
                        clean[j] = expected(f)
                    want.append(clean[j])
            assert sum(1 for w in want if w) == len(damaged) and (n == 1 or (want[at(5)], want[at(6)]) == (20, 21))
            recs = [pack(**f) for f in call]
            for on_device in (False, True):
                bm, st = bv.verify_statements(recs, host_threads=4, on_device=on_device)
                assert st == bytes(want), (n, on_device, [(j, s, w) for j, (s, w) in enumerate(zip(st, want)) if s != w])
                assert bits(bm, n) == [int(w == 0) for w in want]
    finally:
        bv.close()


def test_malformed_and_unservable_records_inside_a_good_call(ctx, gens, payments):
    _, recs, verdicts = payments
    good = [r for r, v in zip(recs, verdicts) if v == 0][:20]
    f = dict(txid=bytes(32), R=bytes(32), s=bytes(32), keys=[bytes(32)], n_in=1, n_out=1, commitments=bytes(128), proof=b"\x01" * 30)
    odd = {2: (good[2][:-1], 16), 5: (good[5] + b"\x00", 16), 7: (pack(**dict(f, keys=[])), 16), 8: (b"", 16), 11: (good[11][:64] + L.to_bytes(32, "little") + good[11][96:], 21),
           13: (pack(**dict(f, keys=[bytes(32)] * 65)), 2), 14: (pack(**dict(f, n_in=0, commitments=bytes(64))), 2), 16: (pack(**dict(f, n_out=65, commitments=bytes(64 * 66))), 2),
           19: (good[19][:50], 16)}
    call = [odd[i][0] if i in odd else good[i] for i in range(20)]
    want = bytes(odd[i][1] if i in odd else 0 for i in range(20))
    bv = _verifier(ctx, gens)
    try:
        for fmt in (STATEMENTS, STATEMENTS | SIGN):
            bm, st = bv.verify_statements(call, host_threads=2, on_device=bool(fmt & SIGN))
            assert st == want and bits(bm, 20) == [int(w == 0) for w in want], (hex(fmt), list(st))
            # status == NULL: the same bits
            blob = b"".join(call)
            offs = (C.c_uint64 * 21)(*([0] + [sum(len(t) for t in call[:i + 1]) for i in range(20)]))
            raw = C.create_string_buffer(b"\xff" * 3, 3)
            bv.set_tx_format(fmt)                            # (verify_statements put back the format it found: none)
            assert ctx.lib.zkgpu_tx_verify_batch(bv.h, 20, blob, offs, 2, raw, None) == 0 and raw.raw == bm
    finally:
        bv.close()


def test_submitted_calls_interleaved_with_format_2_calls_from_two_threads(ctx, gens, payments):
    """one thread queues statements calls (under 4 and under 0x204 in turn), the other format-2 calls on the transactions, in STRICT
    alternation S, T, S, T, ... (a turn counter under a condition: the format is the verifier's).  What is queued alternates in kind,
    so an engine that never mixes kinds in a round runs as many rounds as calls; every call comes back with the verdicts of the
    synchronous call, whatever the format says when its round starts"""
    txs, recs, verdicts = payments
    parts = [(0, 40), (40, 65), (0, 65), (10, 64)]
    bv = _verifier(ctx, gens, 2)
    try:
        bm2, st2 = bv.verify_txs(txs, host_threads=4)
        rounds0, calls0 = bv.tx_stats()
        musig0 = _read(ctx, "tx_musig_on_device")
        turn, state, queued, errors = threading.Condition(), {"next": 0}, {"rec": [], "tx": []}, []

        def submit(kind, parity):
            try:
                for q, (lo, hi) in enumerate(parts):
                    with turn:
                        assert turn.wait_for(lambda: state["next"] == 2 * q + parity or errors, timeout=60)
                        if errors:
                            return
                        if kind == "rec":
                            cid = bv.submit_statements(recs[lo:hi], host_threads=2, on_device=bool(q % 2))
                        else:
                            bv.set_tx_format(2)
                            cid = bv.submit_txs(txs[lo:hi], host_threads=2)
                        queued[kind].append((cid, lo, hi, q))
                        state["next"] += 1
                        turn.notify_all()
            except BaseException as e:                                                        # noqa: BLE001
                with turn:
                    errors.append(e)
                    turn.notify_all()

        threads = [threading.Thread(target=submit, args=(kind, parity)) for parity, kind in enumerate(("rec", "tx"))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for kind in ("tx", "rec"):
            for cid, lo, hi, q in queued[kind]:
                bm, st = bv.wait_statements(cid) if kind == "rec" else bv.wait_txs(cid)
                assert st == st2[lo:hi] and bits(bm, hi - lo) == [1 - v for v in verdicts[lo:hi]], (kind, q)
        rounds, calls = bv.tx_stats()
        assert calls - calls0 == 2 * len(parts)
        assert rounds - rounds0 == calls - calls0, "a round held two calls: of kinds that alternate, so it held both kinds"
        # (the calls queued under 0x204 -- parts 1 and 3 -- had their coefficients formed on the device, the others not)
        assert _read(ctx, "tx_musig_on_device") - musig0 == sum(hi - lo - sum(1 for i in range(lo, hi) if i == 44) for q, (lo, hi) in enumerate(parts) if q % 2)
    finally:
        bv.close()


def test_neighbours_under_one_word_share_a_round_and_a_call_under_the_other_word_runs_alone(ctx, gens, payments):
    """a long call is submitted under 4 and, while its round runs, two short ones are queued back to back through the library's
    own submit (the format is not touched: setting it waits for the verifier, which a round in flight holds).  Both under 4 (the
    control): the engine merges them -- two rounds for the three calls, so it does merge what the queue holds.  Then the same
    with the third call under 0x204, whose format change can only be made between rounds: three rounds, the right verdicts for
    each, every call under the word it was queued with -- tx_musig_on_device moves by the rows of the 0x204 call alone, although
    0x204 is the format in force while the calls queued under 4 are waited for"""
    _, recs, verdicts = payments
    clean = [r for r, v in zip(recs, verdicts) if v == 0]
    long_call, a, b = clean * 8, clean[:20], clean[20:50]
    packed = lambda call: (b"".join(call), [len(r) for r in call], 2)      # noqa: E731
    bv = _verifier(ctx, gens, STATEMENTS)
    try:
        bv.verify_statements(long_call, host_threads=2)      # (warm: buffers and contexts are made)
        for other_word, want_rounds in ((False, 2), (True, 3)):
            rounds0, calls0 = bv.tx_stats()
            musig0 = _read(ctx, "tx_musig_on_device")
            bv.set_tx_format(STATEMENTS)
            ids = [bv.submit_txs_packed(*packed(long_call)), bv.submit_txs_packed(*packed(a))]
            if other_word:
                bv.set_tx_format(STATEMENTS | SIGN)
            ids.append(bv.submit_txs_packed(*packed(b)))
            for cid, call in zip(ids, (long_call, a, b)):
                bm, st = bv.wait_txs(cid)
                assert st == bytes(len(call)) and bits(bm, len(call)) == [1] * len(call)
            rounds, calls = bv.tx_stats()
            assert calls - calls0 == 3 and rounds - rounds0 == want_rounds, (other_word, rounds - rounds0)
            assert _read(ctx, "tx_musig_on_device") - musig0 == (len(b) if other_word else 0)
    finally:
        bv.close()


def test_a_failure_of_any_runtime_call_fails_the_call_closed(ctx, gens, payments):
    """zkgpu_debug_fail_after makes the n-th runtime call of the library answer "failed" on the host (nothing faults on the
    device).  n walks through every runtime call of a warm 0x204 call of 65 records: every one of them, failed, ends the call
    with an error, a zero bitmap and status 1 everywhere; the clean call after it is right"""
    _, recs, verdicts = payments
    n = len(recs)
    blob = b"".join(recs)
    offs = (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in recs[:i + 1]) for i in range(n)]))
    bv = _verifier(ctx, gens, STATEMENTS | SIGN)

    def raw():
        bm, st = C.create_string_buffer(b"\xff" * ((n + 7) // 8), (n + 7) // 8), C.create_string_buffer(b"\xff" * n, n)
        return ctx.lib.zkgpu_tx_verify_batch(bv.h, n, blob, offs, 2, bm, st), bm.raw, st.raw

    try:
        good = raw()
        assert good[0] == 0 and bits(good[1], n) == [1 - v for v in verdicts] and good == raw()      # (warm)
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 10 ** 9, None)
        assert raw() == good
        calls = int(ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None))
        assert 10 <= calls <= 400, calls
        for q in range(1, calls + 1):
            ctx.lib.zkgpu_debug_fail_after(ctx.h, q, None)
            out = raw()
            fired = C.c_longlong(-1)
            ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, C.byref(fired))
            assert fired.value == 1, (q, fired.value)
            assert out[0] != 0 and out[1] == bytes((n + 7) // 8) and out[2] == bytes([1]) * n, q
            assert raw() == good, q                                                                  # the verifier is usable afterwards
        print("runtime calls of a clean 0x204 call of 65 records:", calls)
    finally:
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None)
        bv.close()
