"""The hash tape of a transaction call with ZKGPU_TXFORMAT_HASH_ON_DEVICE (csrc/tx_hash_tape.hpp), on the CPU.

libzkhost's zkhost_tx_hash_tape runs the VM's structure pass over a chunk, flattens the hash plans into the block the
kernel k_tx_hash indexes, and interprets the block with tx_hash_run -- the function the kernel runs per lane, built for
the host.  Checked here: every slot the interpreter writes equals what run_plan writes for the same plan; every
transaction ID equals the oracle's (oracle/zkvm_tx.c, written separately); the lane table is the one a model of the
ordering rule gives (grouped by shape, every run padded to 64 with idle lanes, every transaction once).

Transactions are the oracle builder's (as tests/test_zkvm_tx.py builds them) for one of every shape; the bulk of a mixed
chunk wraps arbitrary commitment and proof bytes (the ID does not depend on whether the proof verifies).
"""
import ctypes as C
import hashlib
import random

import pytest

IDLE = 0xFFFFFFFF
RATE = 166
SHAPES = [(1, 1), (2, 2), (3, 2), (2, 3)]            # (3, 2) and (2, 3): six log entries, a Merkle tree with an odd split


@pytest.fixture(scope="module")
def host():
    from zkvm_amd.build import build, HOST_OUT
    build()
    return C.CDLL(HOST_OUT)


def built(oracle, n_in, n_out, seed):
    """a real payment: proved and signed by the oracle's builder"""
    rng = random.Random(seed)
    fl = rng.randrange(2 ** 250).to_bytes(32, "little")
    q_in = [rng.randrange(1, 2 ** 40) for _ in range(n_in)]
    tot = sum(q_in)
    q_out = [tot // 3] * (n_out - 1)
    q_out.append(tot - sum(q_out))
    tx = oracle.tx_build_payment(n_in, n_out, q_in + q_out, [fl] * (n_in + n_out), hashlib.sha256(b"tape %d" % seed).digest(), 0, 2 ** 40)
    assert tx
    return tx


def wrapped(oracle, n_in, n_out, seed):
    """a signed payment around arbitrary statement bytes: everything the ID covers is there"""
    h = lambda tag, n: b"".join(hashlib.sha256(b"%s %d %d" % (tag, seed, i)).digest() for i in range(n))      # noqa: E731
    tx = oracle.tx_wrap_payment(n_in, n_out, h(b"com", 2 * (n_in + n_out)), h(b"proof", 20) + b"\x01", hashlib.sha256(b"wrap %d" % seed).digest(),
                                seed % 1000, 10 ** 9 + seed)
    assert tx
    return tx


def run_tape(host, txs, threads=2):
    n = len(txs)
    blob = b"".join(txs)
    offs = (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:i + 1]) for i in range(n)]))
    lanes_cap, slots_cap, pieces_cap = 64 * (n + 8), 64 * n + 64, 1 << 16
    status = C.create_string_buffer(n)
    head = (C.c_uint32 * 16)()
    pieces = (C.c_uint32 * (4 * pieces_cap))()
    lanes = (C.c_uint32 * lanes_cap)()
    shape = (C.c_uint32 * n)()
    slot0 = (C.c_uint64 * n)()
    txid = C.create_string_buffer(32 * n)
    s_tape, s_plan, kept = C.create_string_buffer(32 * slots_cap), C.create_string_buffer(32 * slots_cap), C.create_string_buffer(slots_cap)
    host.zkhost_tx_hash_tape.restype = C.c_longlong
    rc = host.zkhost_tx_hash_tape(blob, offs, C.c_size_t(n), C.c_int(threads), status, head, pieces, C.c_size_t(pieces_cap), lanes,
                                  C.c_size_t(lanes_cap), shape, slot0, txid, s_tape, s_plan, kept, C.c_size_t(slots_cap))
    names = ["magic", "n_lanes", "n_tx", "n_shapes", "shapes", "jobs", "pieces", "lanes", "txs", "data", "n_jobs", "n_pieces", "data_bytes",
             "n_slots", "words", "contractid_pos"]
    hd = dict(zip(names, head))
    return dict(rc=rc, status=status.raw, head=hd, lanes=list(lanes[: hd["n_lanes"]]), shape=list(shape), slot0=list(slot0), txid=txid.raw,
                slots_tape=s_tape.raw[: 32 * hd["n_slots"]], slots_plan=s_plan.raw[: 32 * hd["n_slots"]], kept=kept.raw[: hd["n_slots"]],
                pieces=[tuple(pieces[4 * i: 4 * i + 4]) for i in range(hd["n_pieces"])])


def check(oracle, txs, out, live=None):
    n = len(txs)
    live = list(range(n)) if live is None else live
    assert out["rc"] == len(live), out["rc"]
    hd = out["head"]
    assert hd["n_tx"] == len(live) and hd["n_lanes"] % 64 == 0
    # (1) slot by slot against run_plan, on the slots the three protocols write; the others are left alone
    assert sum(out["kept"]) > 0
    for s in range(hd["n_slots"]):
        a, b = out["slots_tape"][32 * s: 32 * s + 32], out["slots_plan"][32 * s: 32 * s + 32]
        assert (a == b) if out["kept"][s] else (a == bytes(32)), ("slot", s)
    # (2) the IDs against the oracle's
    for i in range(n):
        rc, want, _, _ = oracle.tx_id(txs[i])
        assert rc == out["status"][i]
        if i in live:
            assert rc == 0 and out["txid"][32 * i: 32 * i + 32] == want, ("txid", i)
        else:
            assert rc != 0 and out["shape"][i] == IDLE
    # (3) the lane table against a model of the ordering: transactions numbered in chunk order, grouped by shape in the
    # order of the shape table, positions ascending inside a shape, every run padded to 64 with idle lanes
    number = {i: t for t, i in enumerate(live)}
    model = []
    for s in range(hd["n_shapes"]):
        run = [number[i] for i in live if out["shape"][i] == s]
        assert run, ("a shape nobody has", s)
        model += run + [IDLE] * (-len(run) % 64)
    assert out["lanes"] == model
    assert sorted(t for t in out["lanes"] if t != IDLE) == list(range(len(live)))          # every transaction once
    for w in range(0, hd["n_lanes"], 64):                                                  # a wavefront runs one shape
        assert len({out["shape"][live[t]] for t in out["lanes"][w: w + 64] if t != IDLE}) <= 1
    return hd


@pytest.mark.parametrize("shape", SHAPES)
def test_one_built_payment_of_every_shape(host, oracle, shape):
    tx = built(oracle, shape[0], shape[1], 10 * shape[0] + shape[1])
    hd = check(oracle, [tx], run_tape(host, [tx]))
    assert hd["n_lanes"] == 64 and hd["n_shapes"] == 1


def test_a_message_crosses_the_rate_boundary_inside_a_continuation_piece(host, oracle):
    """An output's new contract is hashed as ONE message of several pieces (anchor slot | predicate | count | item heads |
    items).  Following the STROBE position through the piece records of the tape -- each message opens with meta-AD
    framing (2 + label + 4 bytes) and an AD header (2 bytes) -- at least one continuation piece (label 0) must straddle a
    multiple of the rate, 166: that is where streaming a message piece by piece differs from assembling it first.  The
    IDs are right all the same."""
    tx = built(oracle, 2, 2, 22)
    out = run_tape(host, [tx])
    check(oracle, [tx], out)
    pieces = out["pieces"]
    straddles = 0
    for first, p in enumerate(pieces):
        if (p[0] & 0xFF) == 0 or p[1] == p[2]:
            continue                                             # not the first piece of a message in several pieces
        last = first + 1
        while last < len(pieces) and (pieces[last][0] & 0xFF) == 0:
            last += 1
        # This message is the first of its contract-ID transcript, which starts at head.contractid_pos.  The length of its
        # label's text is not known here (1 .. 15 bytes: the label table's format), so a piece counts only if it straddles
        # the boundary for EVERY possible length.
        def inside(label_len):
            pos = out["head"]["contractid_pos"] + 2 + label_len + 4 + 2
            hit = False
            for q in range(first, last):
                ln = pieces[q][1]
                if q > first and pos % RATE != 0 and pos // RATE != (pos + ln - 1) // RATE:
                    hit = True
                pos += ln
            return hit
        straddles += all(inside(n) for n in range(1, 16))
    assert straddles >= 1


def test_a_mixed_chunk_in_scrambled_order(host, oracle):
    """150 transactions of the four shapes in a drawn order, with one the VM rejects and one outside the subset among them:
    more than one wavefront, every run part padding; one thread and four give the same block contents"""
    rng = random.Random(5)
    txs = [built(oracle, a, b, 100 + 10 * a + b) for a, b in SHAPES]
    txs += [wrapped(oracle, *SHAPES[rng.randrange(4)], k) for k in range(146)]
    rng.shuffle(txs)
    txs[17] = txs[17][:-1]                                                   # truncated: rejected by the host
    t = txs[40]
    prog_len = int.from_bytes(t[24:28], "little")
    txs[40] = t[:24] + (prog_len + 1).to_bytes(4, "little") + t[28: 28 + prog_len] + b"\x15" + t[28 + prog_len:]     # unknown opcode
    live = [i for i in range(150) if i not in (17, 40)]
    out = run_tape(host, txs, threads=4)
    hd = check(oracle, txs, out, live)
    assert hd["n_shapes"] == 4 and hd["n_lanes"] == 4 * 64
    one = run_tape(host, txs, threads=1)
    check(oracle, txs, one, live)
    assert one["txid"] == out["txid"]


def test_scheduling_of_a_flagged_call_on_a_stand_in_device(host, oracle):
    """csrc/tx_call.hpp with a device that hashes, on the CPU: the stand-in of tests/test_zkvm_tx.py (keys and signature
    equations with the reference arithmetic, proofs by a table) plus a hashing stage that interprets every chunk's tape with
    tx_hash_run on a thread of its own after a random delay.  One chunk and many (more chunks than ring slots, a ragged last
    one), two stage slots and one: bits and status bytes are those of the unflagged stand-in call, and every transaction
    the VM accepted got its ID from the stand-in's hashing stage.  Then the n-th operation of the hashing stage fails, for
    every n: an error, zero bits, status 1 inside the subset and 2 left alone, nothing leaked, no hang."""
    txs = [wrapped(oracle, *SHAPES[k % 4], 500 + k) for k in range(100)]
    txs[7] = txs[7][:8] + b"\x00" * 8 + txs[7][16:]                         # another mintime: the ID changes, the signature fails
    txs[30] = txs[30][:-1]                                                  # rejected by the host
    t = bytearray(txs[61]); t[0] = 2; txs[61] = bytes(t)                    # a later version: outside the subset
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

    def flagged(chunk, seed, slots=2, fail_at=-1, threads=4):
        bm, st = C.create_string_buffer((n + 7) // 8 + 1), C.create_string_buffer(n)
        nc, leaked, hashed = C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        rc = host.zkhost_txcall_hashing_selftest(C.c_size_t(n), blob, offs, proof_ok, C.c_int(threads), C.c_size_t(chunk), C.c_uint32(seed),
                                                 C.c_int(fail_at), C.c_int(slots), bm, st, C.byref(nc), C.byref(leaked), C.byref(hashed))
        return rc, bm.raw[: (n + 7) // 8], st.raw, nc.value, leaked.value, hashed.value

    want = plain(0, 1)
    assert want[0] == 0 and want[2][7] == 1 and want[2][30] == 1 and want[2][61] == 2 and want[2].count(0) == n - 3
    for chunk, seed, slots, threads in ((0, 1, 2, 4), (8, 2, 2, 4), (16, 3, 1, 4), (24, 4, 2, 1), (64, 5, 1, 2)):
        rc, bm, st, nc, leaked, hashed = flagged(chunk, seed, slots, threads=threads)
        assert (rc, bm, st) == want, (chunk, rc)
        assert leaked == 0 and hashed == n - 2, (chunk, hashed)             # everything the VM accepted, from the hashing stage
        if chunk == 8:
            assert nc == 13
    for chunk in (16, 0):
        k = 0
        while True:
            rc, bm, st, nc, leaked, hashed = flagged(chunk, 100 + k, fail_at=k)
            if rc == 0:
                assert (rc, bm, st) == want
                break
            assert rc == -3 and bm == bytes((n + 7) // 8) and leaked == 0, (chunk, k)
            assert st == bytes(2 if s == 2 else 1 for s in want[2]), (chunk, k)
            k += 1
            assert k < 100
        assert k == (2 * 7 if chunk else 2), (chunk, k)                     # an enqueue and a collect per chunk could fail
