"""What the verifier's ticket engine (csrc/session.hpp) queues, lane by lane, for a fixed set of small scenarios -- device
tickets merged into two device batches whose three pieces are interleaved, tickets that bring no verifier randomness, a
lone ticket, host-memory tickets, a block of several shapes, a proof length no plan serves, a reserve followed by a cold
first run, a transaction call that asks for reasons, tickets in buffers that are not 16-byte aligned -- is what
tests/golden/ticket_sequences.json holds: recorded by tools/record_ticket_sequences.py from the commit the file names,
before the engine was rearranged over a call value, and never regenerated from the code under test.

Per scenario: the verdict bits (held against the oracle here, so a sequence that verifies nothing is never recorded or
compared), every lane's profile entries [name, launches] in the order they were first queued, and the number of gated
runtime calls (csrc/fault_gate.hpp) of a warm run with profiling off -- of the FIRST run where the scenario says so."""
import ctypes as C
import hashlib
import json
import os

import pytest

from gpu_util import bits, load_cloak_fixture, load_mixed_fixture, oracle_block_bits

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ticket_sequences.json")
IN_FLIGHT, MERGE, EACH = 2, 32, 16


def _ticket_sequences(ctx, oracle, lanes=None):
    """-> {"lanes": lanes of a verifier, "scenarios": {name: {"bits", "lanes", "runtime_calls"}}}.  `lanes`: what every
    verifier made here must report (None: whatever the first one reports)."""
    import test_gpu_tx_reasons as txr
    from gpu_util import built_transactions
    from zkvm_amd.verifier import BlockVerifier, BulletproofGens, CloakTx
    lib = ctx.lib
    out = {"lanes": lanes, "scenarios": {}}
    gens = BulletproofGens(ctx, 256, table_bits=10)
    held = []                                               # device buffers: (pointer handed out, pointer to free)

    def to_device(data, skew=0):
        p = C.c_void_p()
        ctx._check(lib.zkgpu_malloc(ctx.h, len(data) + skew, C.byref(p)))
        ctx._check(lib.zkgpu_upload(ctx.h, C.c_void_p(p.value + skew), data, len(data)))
        held.append(p.value)
        return p.value + skew

    def verifier(chunk=0):
        bv = BlockVerifier(ctx, gens, batches_in_flight=IN_FLIGHT, chunk=chunk)
        bv.set_merge(MERGE)
        if out["lanes"] is None:
            out["lanes"] = bv.lanes()
        assert bv.lanes() == out["lanes"], (bv.lanes(), out["lanes"])
        return bv

    def counted(run, want, name):
        lib.zkgpu_debug_fail_after(ctx.h, 1 << 60, None)    # counts, never fires
        try:
            got = run()
        finally:
            fired = C.c_longlong(0)
            seen = int(lib.zkgpu_debug_fail_after(ctx.h, 0, C.byref(fired)))
        assert got == want and fired.value == 0, name
        return seen

    def record(name, bv, run, want, first_run=False):
        lanes_ = [bv.lane(i) for i in range(bv.lanes())]
        calls = counted(run, want, name) if first_run else None
        for c in lanes_:
            c.profile(True)
            c.profile_reset()
        try:
            got = run()
            seqs = [[[k, v[0]] for k, v in c.profile_read().items()] for c in lanes_]
        finally:
            for c in lanes_:
                c.profile(False)
                c.profile_reset()
        assert got == want, name
        if calls is None:
            assert run() == want, name                      # (once more with profiling off: the counted run is a warm one)
            calls = counted(run, want, name)
        out["scenarios"][name] = {"bits": got, "lanes": seqs, "runtime_calls": calls}

    fix, n_in, n_out, plen = load_cloak_fixture()
    n = 4 * EACH
    coms, proofs = [fix[i][0] for i in range(n)], [bytearray(fix[i][1]) for i in range(n)]
    proofs[21][1 + 32 * 11 + 5] ^= 4                        # t_x of one proof (second ticket, first device batch)
    proofs = [bytes(p) for p in proofs]
    r = hashlib.shake_256(b"ticket sequences").digest(64 * n)
    want = list(oracle.cloak_verify_batch(b"".join(coms), n_in, n_out, b"".join(proofs), plen, r, threads=16))
    assert want.count(0) == 1 and want[21] == 0
    h_com = [b"".join(coms[EACH * k: EACH * (k + 1)]) for k in range(4)]            # the four tickets' inputs
    h_proofs = [b"".join(proofs[EACH * k: EACH * (k + 1)]) for k in range(4)]
    h_r = [r[64 * EACH * k: 64 * EACH * (k + 1)] for k in range(4)]
    try:
        d_com, d_proofs, d_r = [[to_device(x) for x in xs] for xs in (h_com, h_proofs, h_r)]
        skew_com, skew_r = [to_device(x, 8) for x in h_com], [to_device(x, 8) for x in h_r]
        assert all(p % 16 == 8 for p in skew_com + skew_r)

        def tickets(bv, com, rr, proof_len=plen):
            def run():
                t = bv.submit_many_dev(n_in, n_out, EACH, com, d_proofs, proof_len, rr)
                return [b for k in t for b in bits(bv.wait(k), EACH)]
            return run

        def lone(bv, rr):
            def run():
                return bits(bv.wait(bv.submit_dev(n_in, n_out, EACH, d_com[1], d_proofs[1], plen, rr)), EACH)
            return run

        def scenario(name, make, want_, chunk=0, before=None, first_run=False):
            bv = verifier(chunk)
            try:
                if before:
                    before(bv)
                record(name, bv, make(bv), want_, first_run)
            finally:
                bv.close()

        scenario("device tickets", lambda bv: tickets(bv, d_com, d_r), want)
        scenario("tickets without r", lambda bv: tickets(bv, d_com, [d_r[0], None, d_r[2], None]), want)
        scenario("a lone ticket", lambda bv: lone(bv, d_r[1]), want[EACH: 2 * EACH])
        scenario("a lone ticket without r", lambda bv: lone(bv, None), want[EACH: 2 * EACH])

        def host(bv):
            def run():
                t = bv.submit_many(n_in, n_out, EACH, h_com[:2], h_proofs[:2], plen, h_r[:2])
                return [b for k in t for b in bits(bv.wait(k), EACH)]
            return run
        scenario("host tickets", host, want[: 2 * EACH])

        # a block of three shapes the 256 generators serve, in requests of 16: 40 of 2x2 (three requests merged into one device
        # batch), 20 of 1x2 (two requests), 16 of 1x1 (one request) -- three device batches on two lanes
        mixed = load_mixed_fixture()
        txs = []
        for i in range(40):
            for shape, count in (((2, 2), 40), ((1, 2), 20), ((1, 1), 16)):
                if i < count:
                    txs.append((shape[0], shape[1]) + mixed[shape][i % len(mixed[shape])])
        bad = bytearray(txs[7][3]); bad[-40] ^= 1; txs[7] = txs[7][:3] + (bytes(bad),)
        txs[30] = txs[30][:3] + (txs[30][3][:-32],)         # truncated: a proof length its shape's plan does not serve
        r_blk = hashlib.shake_256(b"ticket sequences, block").digest(64 * len(txs))
        want_blk = list(oracle_block_bits(oracle, txs, r_blk))
        assert want_blk.count(0) == 2

        def block(bv):
            def run():
                b = bv.block([CloakTx(*t) for t in txs], r_blk)
                try:
                    return bits(bv.verify_block(b), len(txs))
                finally:
                    b.close()
            return run
        scenario("a mixed-shape block", block, want_blk, chunk=EACH)

        scenario("a wrong proof length", lambda bv: tickets(bv, d_com, d_r, plen - 32), [0] * n)
        assert all(seq == [] for seq in out["scenarios"]["a wrong proof length"]["lanes"])

        scenario("reserve, then a cold first run", lambda bv: tickets(bv, d_com, d_r), want,
                 before=lambda bv: bv.reserve(n_in, n_out, MERGE), first_run=True)

        # one synchronous transaction call of 16 in the reasons format; the damage is tests/test_gpu_tx_reasons.py's
        tx16, _ = built_transactions(EACH, call=txr.CALL, bad_every=0)
        damage = {3: (txr.tx_incremented, txr.PROOF_EQUATION), 6: (txr.point_undecodable, txr.PROOF_POINT),
                  9: (txr.version_flipped, txr.PROOF_FORMAT), 12: (txr.s_incremented, txr.SIGNATURE)}
        want_st = [txr.ACCEPTED] * EACH
        for i, (f, code) in damage.items():
            tx16[i] = f(tx16[i])
            want_st[i] = code
        want_tx = [int(s == txr.ACCEPTED) for s in want_st]
        assert [int(oracle.tx_verify(t, r[:64]) == 0) for t in tx16] == want_tx

        def tx_call(bv):
            def run():
                bm, st = bv.verify_txs(tx16, host_threads=4)
                assert st == bytes(want_st)
                return bits(bm, EACH)
            return run
        scenario("a transaction call with reasons", tx_call, want_tx,
                 before=lambda bv: bv.set_tx_format(BlockVerifier.TXFORMAT_RECOLLECTED_V1_REASONS))

        # the merge's fallback: commitments and randomness 8 bytes off a 16-byte boundary go through plain copies
        scenario("unaligned device tickets", lambda bv: tickets(bv, skew_com, skew_r), want)
    finally:
        lib.zkgpu_debug_fail_after(ctx.h, 0, None)
        for p in held:
            ctx.free_device(p)
        gens.close()
    return out


@pytest.fixture(scope="module")
def ctx():
    from zkvm_amd import Context
    c = Context(0)
    yield c
    c.lib.zkgpu_debug_fail_after(c.h, 0, None)
    c.close()


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got(ctx, oracle, gold):
    return _ticket_sequences(ctx, oracle, lanes=gold["lanes"])


def test_the_scenarios_are_the_recorded_ones(got, gold):
    assert got["lanes"] == gold["lanes"] and sorted(got["scenarios"]) == sorted(gold["scenarios"])


@pytest.mark.parametrize("name", ["device tickets", "tickets without r", "a lone ticket", "a lone ticket without r", "host tickets",
                                  "a mixed-shape block", "a wrong proof length", "reserve, then a cold first run",
                                  "a transaction call with reasons", "unaligned device tickets"])
def test_ticket_sequences_are_the_recorded_ones(got, gold, name):
    """bits, per-lane launch sequences and gated runtime calls of one scenario = the recording's"""
    have, rec = got["scenarios"][name], gold["scenarios"][name]
    print(name, "runtime calls", have["runtime_calls"], "recorded", rec["runtime_calls"])
    assert have["bits"] == rec["bits"]
    for i, (a, b) in enumerate(zip(have["lanes"], rec["lanes"])):
        assert a == b, (name, "lane", i)
    assert len(have["lanes"]) == len(rec["lanes"])
    assert have["runtime_calls"] == rec["runtime_calls"]
