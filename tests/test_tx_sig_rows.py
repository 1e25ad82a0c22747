"""The signature challenge of a transaction call with ZKGPU_TXFORMAT_SIGN_ON_DEVICE (csrc/tx_sig_rows.hpp), on the CPU.

libzkhost's zkhost_tx_sig_rows treats a chunk the way a chaining call does -- the taped second pass, the tape interpreted (IDs
in the tape's order), the aggregated keys, the signature rows with the MuSig coefficients a_i in place, the row -> tape map --
and runs tx_sig_row over every row: the function the kernel k_tx_sig_rows runs per lane, built for the host.  Checked here:
(a) every scalar it writes equals what tx_finish_signature writes for the same statement, byte for byte; (b) the challenge
itself equals an independent restatement with the oracle's Merlin transcript over (the oracle's transaction ID, the aggregated
key, R), which gives -c a_i mod l in Python integers.

Then csrc/tx_call.hpp with a device that chains, on the stand-in device of tests/test_tx_hash_tape.py extended to chain.
"""
import ctypes as C

import pytest

from test_tx_hash_tape import SHAPES, built, wrapped

L = 2 ** 252 + 27742317777372353535851937790883648493
CAP = 4


@pytest.fixture(scope="module")
def host():
    from zkvm_amd.build import build, HOST_OUT
    build()
    return C.CDLL(HOST_OUT)


def run_rows(host, txs, threads=2):
    n = len(txs)
    blob = b"".join(txs)
    offs = (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:i + 1]) for i in range(n)]))
    status = C.create_string_buffer(n)
    n_keys = (C.c_uint32 * n)()
    txid, agg, R = (C.create_string_buffer(32 * n) for _ in range(3))
    a_in, rows, hostside = (C.create_string_buffer(32 * CAP * n) for _ in range(3))
    host.zkhost_tx_sig_rows.restype = C.c_longlong
    rc = host.zkhost_tx_sig_rows(blob, offs, C.c_size_t(n), C.c_int(threads), C.c_size_t(CAP), status, n_keys, txid, agg, R, a_in, rows, hostside)
    cut = lambda b, w: [b.raw[w * i: w * (i + 1)] for i in range(n)]      # noqa: E731
    return dict(rc=rc, status=status.raw, n_keys=list(n_keys), txid=cut(txid, 32), agg=cut(agg, 32), R=cut(R, 32), a=cut(a_in, 32 * CAP),
                rows=cut(rows, 32 * CAP), host=cut(hostside, 32 * CAP))


def check(oracle, txs, out, live, keys_of):
    from oracle.binding import MerlinTranscript
    assert out["rc"] == len(live)
    for i, tx in enumerate(txs):
        if i not in live:
            assert out["status"][i] != 0 and out["n_keys"][i] == 0 and out["rows"][i] == bytes(32 * CAP)
            continue
        k = out["n_keys"][i]
        assert out["status"][i] == 0 and k == keys_of(i), (i, k)
        # (a) byte for byte what tx_finish_signature writes
        assert out["rows"][i] == out["host"][i], ("tx_finish_signature", i)
        assert out["rows"][i][: 32 * k] != out["a"][i][: 32 * k] and out["rows"][i][32 * k:] == bytes(32 * (CAP - k))
        # (b) the challenge, restated
        rc, want_id, _, _ = oracle.tx_id(tx)
        assert rc == 0 and out["txid"][i] == want_id, ("txid", i)
        t = MerlinTranscript(b"ZkVM.signtx")
        t.append_message(b"txid", want_id)
        t.append_message(b"dom-sep", b"schnorr-signature v1")
        t.append_message(b"X", out["agg"][i])
        t.append_message(b"R", out["R"][i])
        c = t.challenge_scalar(b"c")
        for j in range(k):
            a = int.from_bytes(out["a"][i][32 * j: 32 * j + 32], "little")
            assert a < L
            assert out["rows"][i][32 * j: 32 * j + 32] == ((-c * a) % L).to_bytes(32, "little"), ("-c a_i", i, j)


@pytest.mark.parametrize("shape", SHAPES)
def test_one_built_payment_of_every_shape(host, oracle, shape):
    """1, 2, 3 and 2 keys: the loop over a row's extent"""
    tx = built(oracle, shape[0], shape[1], 10 * shape[0] + shape[1])
    out = run_rows(host, [tx])
    check(oracle, [tx], out, [0], lambda i: shape[0])
    assert out["agg"][0] != bytes(32)


def test_a_scrambled_chunk_of_wrapped_payments(host, oracle):
    """100 of the four shapes in a drawn order, one the VM rejects and one outside the subset among them: the rows are fewer than
    the transactions and lie in another order than the tape's lanes, so the map from row to tape position is exercised"""
    import random
    rng = random.Random(9)
    shapes = [SHAPES[rng.randrange(4)] for _ in range(100)]
    txs = [wrapped(oracle, a, b, 900 + k) for k, (a, b) in enumerate(shapes)]
    txs[11] = txs[11][:-1]
    t = bytearray(txs[52]); t[0] = 2; txs[52] = bytes(t)
    live = [i for i in range(100) if i not in (11, 52)]
    out = run_rows(host, txs, threads=4)
    check(oracle, txs, out, live, lambda i: shapes[i][0])
    one = run_rows(host, txs, threads=1)
    assert one["rows"] == out["rows"]


def test_scheduling_of_a_chaining_call_on_a_stand_in_device(host, oracle):
    """csrc/tx_call.hpp with a device that chains, on the CPU: the hashing stand-in plus a signature stage that waits on a thread
    of its own for the slot's key stage and tape, forms the challenges with tx_sig_row and checks the rows.  Several chunks
    (more than ring slots, a ragged last one), one chunk, one stage slot: bits and status bytes are the unchained call's, there
    is one signature stage per chunk, and every row's challenge came from the stand-in.  Then the n-th operation of the
    chained signature stage fails, for every n: an error, zero bits, status 1 inside the subset and 2 left alone, nothing
    leaked, no hang."""
    txs = [wrapped(oracle, *SHAPES[k % 4], 500 + k) for k in range(100)]
    txs[7] = txs[7][:8] + b"\x00" * 8 + txs[7][16:]                         # another mintime: the ID changes, the signature fails
    txs[30] = txs[30][:-1]                                                  # rejected by the host
    t = bytearray(txs[61]); t[0] = 2; txs[61] = bytes(t)                    # a later version: outside the subset
    t = bytearray(txs[44]); t[-687] ^= 1; txs[44] = bytes(t)                # a byte of R (R:32 s:32 n:4 and the 641 proof bytes end the transaction)
    n = len(txs)
    proof_ok = bytes([1] * n)
    blob = b"".join(txs)
    offs = (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:i + 1]) for i in range(n)]))

    def plain(chunk, seed):
        bm, st = C.create_string_buffer((n + 7) // 8 + 1), C.create_string_buffer(n)
        nc, ns, leaked = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        rc = host.zkhost_txcall_selftest(C.c_size_t(n), blob, offs, proof_ok, C.c_int(4), C.c_size_t(chunk), C.c_uint32(seed), C.c_int(-1), bm, st,
                                         C.byref(nc), C.byref(ns), C.byref(leaked))
        return rc, bm.raw[: (n + 7) // 8], st.raw

    def chained(chunk, seed, slots=2, fail_at=-1, threads=4):
        bm, st = C.create_string_buffer((n + 7) // 8 + 1), C.create_string_buffer(n)
        nc, ns, leaked, hashed, signed = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0), C.c_uint64(0)
        rc = host.zkhost_txcall_chaining_selftest(C.c_size_t(n), blob, offs, proof_ok, C.c_int(threads), C.c_size_t(chunk), C.c_uint32(seed),
                                                  C.c_int(fail_at), C.c_int(slots), bm, st, C.byref(nc), C.byref(ns), C.byref(leaked),
                                                  C.byref(hashed), C.byref(signed))
        return rc, bm.raw[: (n + 7) // 8], st.raw, nc.value, ns.value, leaked.value, hashed.value, signed.value

    want = plain(0, 1)
    assert want[0] == 0 and want[2][7] == 1 and want[2][44] == 1 and want[2][30] == 1 and want[2][61] == 2 and want[2].count(0) == n - 4
    for chunk, seed, slots, threads in ((0, 1, 2, 4), (8, 2, 2, 4), (16, 3, 1, 4), (24, 4, 2, 1), (64, 5, 1, 2)):
        rc, bm, st, nc, ns, leaked, hashed, signed = chained(chunk, seed, slots, threads=threads)
        assert (rc, bm, st) == want, (chunk, rc)
        assert ns == nc and leaked == 0 and hashed == n - 2 and signed == n - 2, (chunk, nc, ns, hashed, signed)
        if chunk == 8:
            assert nc == 13
    for chunk, slots in ((16, 2), (16, 1), (0, 2)):
        k = 0
        while True:
            rc, bm, st, nc, ns, leaked, hashed, signed = chained(chunk, 100 + k, slots=slots, fail_at=k)
            if rc == 0:
                assert (rc, bm, st) == want
                break
            assert rc == -3 and bm == bytes((n + 7) // 8) and leaked == 0, (chunk, k)
            assert st == bytes(2 if s == 2 else 1 for s in want[2]), (chunk, k)
            k += 1
            assert k < 100
        assert k == (2 * 7 if chunk else 2), (chunk, k)                     # an enqueue and a collect per chunk could fail
