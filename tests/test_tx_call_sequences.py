"""What a transaction call ASKS of its device (csrc/tx_call.hpp over the stand-ins of csrc/hostlib.cpp, through the recording
wrapper behind zkhost_txcall_trace) is what tests/golden/tx_call_sequences.json holds: recorded by
tools/record_tx_call_sequences.py from the commit the file names, before the call's mode became one value and the scheduler's
twin steps were shared, and never regenerated from the code under test.  No GPU.

The other CPU self-tests pin what a call hands back; this pins the schedule.  Per scenario -- a format word, a chunk size, the
stage slots -- and per KIND of operation the ordered list of [slot or ring slot, rows, detail]: across the two threads of a call
only the order within a kind is fixed, so that is what is recorded (two recordings under different delay seeds agreed on every
kind of every scenario).  Beside them the planned chunks and signature stages.  One relation the lists cannot express is
asserted from the same traces: a call of several chunks queues a chunk's keys before its proofs, a call of one chunk its proofs
first (words of base 1 / 2 that do not sign on the device)."""
import ctypes as C
import json
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tx_call_sequences.json")
KINDS = ["keys_enqueue", "keys_enqueue_formed", "keys_collect", "proofs_stage", "proofs_start", "proofs_finish", "sigs_enqueue", "sigs_collect",
         "hash_enqueue", "hash_collect"]                    # (the order of TracingTxDevice::Op)
HASH, SIGN, IDS, LOG, PRE = 0x100, 0x200, 0x400, 0x800, 0x2000
WORDS = [1, 2, 1 | HASH, 1 | HASH | SIGN, 1 | HASH | SIGN | IDS, 2 | HASH | IDS | LOG | 4 << 16, 1 | IDS | PRE, 2 | HASH | IDS | PRE, 4, 4 | SIGN]
CHUNKS = [0, 16, 64]                                        # one chunk (proofs first); ten, more than the ring of 6, ragged last; three
SLOTS = [2, 1]
SEEDS = [11, 12, 13]


def _inputs(oracle):
    """the 150 transactions of test_zkvm_tx.py::test_scheduling_of_a_transaction_call_on_a_stand_in_device -- damaged ones, two
    other shapes, one outside the subset -- with the stand-in's proof table; and, for the statements words, the records their VM
    would leave (tx_statements_util), the one outside the subset as a record with more inputs than the library serves"""
    from gpu_util import built_transactions
    from test_zkvm_tx import payment
    from tx_statements_util import fields_of_payment, pack
    txs, _ = built_transactions(150, call=9, bad_every=8)
    clean, _ = built_transactions(150, call=9, bad_every=0)
    proof_ok = [1] * len(txs)
    for i, (a, b) in enumerate(zip(txs, clean)):
        plen = struct.unpack("<I", b[24:28])[0]
        if a[28 + plen + 64:] != b[28 + plen + 64:]:
            proof_ok[i] = 0
    txs[5] = clean[5] = payment(oracle, 1, 2, 77)
    txs[77] = clean[77] = payment(oracle, 3, 2, 78, two_flavors=True)
    txs[100] = txs[100][:8] + b"\x00" * 8 + txs[100][16:]
    t = bytearray(txs[120]); t[0] = 2; txs[120] = bytes(t)
    recs = []
    for i, (tx, ok) in enumerate(zip(txs, clean)):
        try:
            f = fields_of_payment(oracle, tx)
        except AssertionError:                              # (damaged where the walk or the oracle's ID stops: the undamaged fields)
            f = fields_of_payment(oracle, ok)
        if i == 120:
            f = dict(f, n_in=65, commitments=bytes(64 * (65 + f["n_out"])))
        recs.append(pack(**f))
    return txs, recs, bytes(proof_ok)


def _trace(host, word, slots, chunk, items, proof_ok, seed):
    offs = (C.c_uint64 * (len(items) + 1))()
    for i, it in enumerate(items):
        offs[i + 1] = offs[i] + len(it)
    cap = 4096
    out, plan = (C.c_int64 * (4 * cap))(), (C.c_uint64 * 2)()
    host.zkhost_txcall_trace.restype = C.c_longlong
    n = host.zkhost_txcall_trace(C.c_int(word), C.c_int(slots), C.c_size_t(chunk), C.c_size_t(len(items)), b"".join(items) + bytes(64), offs, proof_ok,
                                 C.c_int(4), C.c_uint32(seed), out, C.c_size_t(cap), plan)
    assert n >= 0, (hex(word), slots, chunk, n)
    return [tuple(out[4 * i: 4 * i + 4]) for i in range(n)], list(plan)


def scenario_name(word, chunk, slots):
    return "word %#x, chunk %d, %d slot%s" % (word, chunk, slots, "s" if slots > 1 else "")


def _tx_call_sequences(host, inputs, seed, words=WORDS):
    """-> {scenario: {"chunks", "sig_stages", "kinds": {kind: [[slot, rows, detail] ...]}, "trace": the operations as they arrived}}"""
    txs, recs, proof_ok = inputs
    got = {}
    for word in words:
        for chunk in CHUNKS:
            for slots in SLOTS:
                trace, plan = _trace(host, word, slots, chunk, recs if word & 7 == 4 else txs, proof_ok, seed)
                got[(word, chunk, slots)] = {
                    "chunks": plan[0], "sig_stages": plan[1], "trace": trace,
                    "kinds": {k: [list(e[1:]) for e in trace if e[0] == q] for q, k in enumerate(KINDS)}}
    return got


@pytest.fixture(scope="module")
def host():
    from zkvm_amd.build import build, HOST_OUT
    build()
    return C.CDLL(HOST_OUT)


@pytest.fixture(scope="module")
def inputs(oracle):
    return _inputs(oracle)


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


@pytest.fixture(scope="module", params=[(seed, word) for seed in SEEDS for word in WORDS], ids=lambda p: "seed %d, word %#x" % p)
def got(host, inputs, request):
    """the scenarios of one word under one delay seed (one case each: a call over a stand-in takes a good part of a second)"""
    return _tx_call_sequences(host, inputs, request.param[0], [request.param[1]])


def test_the_recording_holds_every_scenario(gold):
    assert len(gold["recorded_from"]) == 40
    assert sorted(gold["scenarios"]) == sorted(scenario_name(w, c, n) for w in WORDS for c in CHUNKS for n in SLOTS)


def test_what_the_device_is_asked_is_the_recording(got, gold):
    assert len(got) == len(CHUNKS) * len(SLOTS)
    for key, have in got.items():
        name = scenario_name(*key)
        rec = gold["scenarios"][name]
        assert (have["chunks"], have["sig_stages"]) == (rec["chunks"], rec["sig_stages"]), name
        assert sorted(rec["kinds"]) == sorted(KINDS), name   # (no kind was left out of the recording: every one was deterministic)
        for kind in KINDS:
            assert have["kinds"][kind] == rec["kinds"][kind], (name, kind)


def test_keys_before_proofs_unless_the_call_is_one_chunk(got):
    """words of base 1 or 2 without 0x200: with several chunks proofs_start of chunk c comes after keys_enqueue of chunk c, with
    one chunk before it (every chunk of these inputs has transactions the VM accepts, so the c-th of either is chunk c's; a
    precompute-only word asks for neither)"""
    for (word, chunk, slots), have in got.items():
        if word & 7 not in (1, 2) or word & SIGN:
            continue
        keys = [i for i, e in enumerate(have["trace"]) if e[0] == KINDS.index("keys_enqueue")]
        proofs = [i for i, e in enumerate(have["trace"]) if e[0] == KINDS.index("proofs_start")]
        n = have["chunks"]
        assert n == {0: 1, 16: 10, 64: 3}[chunk] and len(keys) == len(proofs) == (0 if word & PRE else n), (hex(word), chunk, slots)
        for c, (k, p) in enumerate(zip(keys, proofs)):
            assert (p > k) if n > 1 else (p < k), (hex(word), chunk, slots, c)
