"""Prover randomness the library draws itself (seeds == NULL in zkgpu_cloak_prove_batch / zkgpu_r1cs_prove_batch;
zkvm_amd/csrc/prover_draw.hpp, k_pv_draw): the call takes ONE seed from the OS, statement i of the CALL gets

    seed_i = SHAKE256(call_seed || "statement" || LE64(i))[:32]

and the call then gives byte for byte what the same call with seeds = seed_0 || seed_1 || ... gives -- whatever the slicing
and the prover mode.  The hook zkgpu_debug_read "prover_seed" hands the call's seed to the test, which recomputes seed_i with
hashlib and holds the library's commitments and proofs against the ORACLE's prover on that seed.  Generators for 2-in/2-out,
tables at 8 bits; a batch of 70 crosses a 64-lane block of k_pv_draw and is no multiple of it."""
import ctypes as C
import hashlib
from concurrent.futures import ThreadPoolExecutor

import pytest

from gpu_util import GADGET_LABEL, L, bits, describe_range, gadget_witness

pytestmark = pytest.mark.gpu
OK = 0
BATCH = 70
STRIDE = 1 + 32 * (16 + 2 * 16)
FLAVOR = bytes([3]) + bytes(31)


def statement_seed(call_seed: bytes, i: int) -> bytes:
    return hashlib.shake_256(call_seed + b"statement" + i.to_bytes(8, "little")).digest(32)


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
    g = BulletproofGens(ctx, 256, table_bits=8)
    yield g
    g.close()


def quantities(n_in, n_out, batch=BATCH):
    """balanced statements of one flavor, every one different"""
    if (n_in, n_out) == (2, 2):
        return [[5 + i, 9, 4 + i, 10] for i in range(batch)]
    assert (n_in, n_out) == (1, 1)
    return [[7 + i, 7 + i] for i in range(batch)]


def cloak_call(c, gens, n_in, n_out, qs, seeds, host_threads=3):
    """the C entry point itself, outputs pre-filled with 0xff -> (status, commitments, proofs, proof_len)"""
    nv, batch = n_in + n_out, len(qs)
    qa = (C.c_uint64 * (batch * nv))(*[q for row in qs for q in row])
    com = C.create_string_buffer(b"\xff" * (64 * nv * batch), 64 * nv * batch)
    proofs = C.create_string_buffer(b"\xff" * (STRIDE * batch), STRIDE * batch)
    plen = C.c_size_t(12345)
    st = c.lib.zkgpu_cloak_prove_batch(c.h, gens.points.h, gens.gens_capacity, batch, n_in, n_out, qa, FLAVOR * (nv * batch),
                                       None if seeds is None else b"".join(seeds), host_threads, com, proofs, STRIDE, C.byref(plen))
    return st, com.raw, proofs.raw, plen.value


def split(n_in, n_out, com, proofs, plen):
    nv = n_in + n_out
    n = len(com) // (64 * nv)
    return [(com[64 * nv * i: 64 * nv * (i + 1)], proofs[STRIDE * i: STRIDE * i + plen]) for i in range(n)]


def oracle_cloak(oracle, n_in, n_out, qs, seeds):
    """the oracle's prover on every statement and its seed -> [(commitments, proof)]"""
    def one(i):
        rc, com, proof, _ = oracle.cloak_prove(qs[i], [FLAVOR] * (n_in + n_out), n_in, n_out, seeds[i])
        assert rc == 0, i
        return com, proof
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(one, range(len(qs))))


def null_call_against_oracle(c, gens, oracle, n_in, n_out, label):
    """one call without seeds on c: OK, a seed was drawn, every statement equals the oracle's on seed_i -> (call seed, statements)"""
    qs = quantities(n_in, n_out)
    st, com, proofs, plen = cloak_call(c, gens, n_in, n_out, qs, None)
    assert st == OK, (label, st, c.lib.zkgpu_last_error(c.h))
    call_seed = c.prover_seed()
    assert call_seed != bytes(32), label
    got = split(n_in, n_out, com, proofs, plen)
    seeds = [statement_seed(call_seed, i) for i in range(BATCH)]
    want = oracle_cloak(oracle, n_in, n_out, qs, seeds)
    for i in range(BATCH):
        assert got[i] == want[i], (label, "statement", i)
    return call_seed, seeds, got


def test_a_cloak_call_without_seeds_equals_the_oracle_on_the_derived_seeds(ctx, gens, oracle):
    """(1) fails before the feature (ZKGPU_EINVAL).  seeds=None through the Python layer: every proof verifies under the
    oracle's verifier, equals the oracle's prover on seed_i, and equals the library's own call with those seeds spelled out."""
    from zkvm_amd.verifier import Prover
    qs = quantities(2, 2)
    fs = [[FLAVOR] * 4] * BATCH
    pv = Prover(ctx, gens, host_threads=3)
    made = pv.prove(2, 2, qs, fs)                          # seeds=None is the default
    assert len(made) == BATCH
    call_seed = ctx.prover_seed()
    assert call_seed != bytes(32)
    seeds = [statement_seed(call_seed, i) for i in range(BATCH)]
    want = oracle_cloak(oracle, 2, 2, qs, seeds)
    r = hashlib.shake_256(b"prover draw r").digest(64 * BATCH)
    with ThreadPoolExecutor(8) as ex:
        ok = list(ex.map(lambda i: oracle.cloak_verify(made[i].commitments, 2, 2, made[i].proof, r[64 * i: 64 * i + 64]), range(BATCH)))
    assert all(ok), ok
    for i, t in enumerate(made):
        assert (t.commitments, t.proof) == want[i], i
    again = pv.prove(2, 2, qs, fs, seeds)
    assert [(t.commitments, t.proof) for t in again] == want
    # the packed form: the batch size comes from the other arguments
    qa = (C.c_uint64 * (BATCH * 4))(*[q for row in qs for q in row])
    com, proofs, plen = pv.prove_packed(2, 2, BATCH, qa, FLAVOR * (4 * BATCH))
    s2 = ctx.prover_seed()
    assert s2 not in (bytes(32), call_seed)
    assert split(2, 2, com.raw, proofs.raw, plen) == oracle_cloak(oracle, 2, 2, qs, [statement_seed(s2, i) for i in range(BATCH)])


@pytest.mark.parametrize("mode, slices", [(16 + 3, 3), (16 + 1, 1), (1, None)], ids=("three slices", "one slice", "host lockstep"))
def test_positions_are_those_of_the_call_in_every_slicing_and_mode(gens, oracle, mode, slices):
    """(2) cuts at 23 and 46: a slice that numbered its statements from 0 would repeat the seeds of statements 0 .. 22"""
    from zkvm_amd import Context
    c = Context(0)
    try:
        c.set_prover_mode(mode)
        null_call_against_oracle(c, gens, oracle, 2, 2, "mode %d" % mode)
        if slices is not None:
            assert int.from_bytes(c.debug_read("prover_slices", 4), "little") == slices
    finally:
        c.close()


def test_equal_statements_get_different_blindings_and_calls_different_seeds(ctx, gens):
    """(3) seventy times the same values and flavors: 70 distinct commitments per value; a second call: another seed, other
    commitments; after a call that brings its seeds the hook reads zero"""
    qs = [[5, 9, 4, 10]] * BATCH
    st, com, _, _ = cloak_call(ctx, gens, 2, 2, qs, None)
    assert st == OK
    s1 = ctx.prover_seed()
    assert s1 != bytes(32)
    for slot in range(8):                                  # (quantity, flavor) commitments of the four values
        assert len({com[256 * i + 32 * slot: 256 * i + 32 * slot + 32] for i in range(BATCH)}) == BATCH, slot
    st, com2, _, _ = cloak_call(ctx, gens, 2, 2, qs, None)
    assert st == OK
    s2 = ctx.prover_seed()
    assert s2 not in (bytes(32), s1)
    assert not {com[32 * k: 32 * k + 32] for k in range(8 * BATCH)} & {com2[32 * k: 32 * k + 32] for k in range(8 * BATCH)}
    st, _, _, _ = cloak_call(ctx, gens, 2, 2, qs, [hashlib.sha256(b"own seed %d" % i).digest() for i in range(BATCH)])
    assert st == OK and ctx.prover_seed() == bytes(32)


def test_described_system_without_seeds_with_and_without_blindings(ctx, gens, oracle):
    """(4) zkgpu_r1cs_prove_batch on the 8-bit range statement (m = 1): blindings NULL -- everything derived, the oracle's
    gadget prover on seed_i gives the same bytes; blindings given -- only the rng seed is derived: the library's call with
    seed_i spelled out gives the same bytes and the oracle's verifier accepts them"""
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import R1csProver
    desc = R1csDescription(GADGET_LABEL, *describe_range(8))
    values = [[(17 * i + 3) % 256] for i in range(BATCH)]
    mult_def = gadget_witness(1, 8, values[0])[0]
    given = [gadget_witness(1, 8, v)[1] for v in values]
    pv = R1csProver(ctx, gens, desc, mult_def, host_threads=3)
    coms, proofs = pv.prove(values, given)
    call_seed = ctx.prover_seed()
    assert call_seed != bytes(32)
    for i in range(BATCH):
        rc, want_com, want_proof = oracle.gadget_prove(1, 8, values[i], statement_seed(call_seed, i))
        assert rc == 0 and (coms[i], proofs[i]) == (want_com, want_proof), i
    blind = [[int.from_bytes(hashlib.sha512(b"given blinding %d" % i).digest(), "little") % L] for i in range(BATCH)]
    coms, proofs = pv.prove(values, given, None, blind)
    call_seed = ctx.prover_seed()
    assert call_seed != bytes(32)
    seeds = [statement_seed(call_seed, i) for i in range(BATCH)]
    assert (coms, proofs) == pv.prove(values, given, seeds, blind)
    assert ctx.prover_seed() == bytes(32)
    r = hashlib.shake_256(b"prover draw gadget r").digest(64 * BATCH)
    assert all(oracle.gadget_verify(1, 8, coms[i], proofs[i], r[64 * i: 64 * i + 64]) for i in range(BATCH))
    assert len(set(coms)) == BATCH


def test_one_in_one_out_cloak_without_seeds(ctx, gens, oracle):
    """(4, second shape) m = 4: five derivations per statement, 350 lanes"""
    null_call_against_oracle(ctx, gens, oracle, 1, 1, "1-in/1-out")


@pytest.mark.timeout(600, method="thread")
def test_a_call_without_seeds_fails_closed_at_every_runtime_call(ctx, gens, oracle):
    """(5) zkgpu_debug_fail_after (csrc/fault_gate.hpp: the n-th HIP runtime call REPORTS failure without being made, the
    device is not touched): every runtime call of one warm call without seeds in three slices fails in turn.  A nonzero
    status leaves every commitment and proof byte zero and *proof_len 0; a fault that was absorbed leaves a call that
    verifies; and the next clean call without seeds verifies (device verifier on every one, the oracle's on the last)."""
    from zkvm_amd import Context
    from zkvm_amd.verifier import CloakTx, Verifier
    qs = quantities(2, 2)
    v = Verifier(ctx, gens, host_threads=2)
    pc = Context(0)                           # the slices' helper contexts are made by its first call

    def verified(com, proofs, plen):
        txs = [CloakTx(2, 2, a, b) for a, b in split(2, 2, com, proofs, plen)]
        return txs, bits(v.verify_bitmap_gpu(txs), BATCH) == [1] * BATCH

    def arm(n):
        ctx.lib.zkgpu_debug_fail_after(ctx.h, n, None)

    def disarm():
        fired = C.c_longlong(0)
        seen = ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, C.byref(fired))
        return int(seen), int(fired.value)

    try:
        pc.set_prover_mode(16 + 3)
        st, com, proofs, plen = cloak_call(pc, gens, 2, 2, qs, None)      # cold: workspaces, helper contexts
        assert st == OK and verified(com, proofs, plen)[1]
        arm(1 << 60)                                                      # counts, never fires
        st, com, proofs, plen = cloak_call(pc, gens, 2, 2, qs, None)
        n_calls, fired = disarm()
        assert st == OK and fired == 0 and n_calls >= 30, (st, fired, n_calls)
        surfaced = 0
        txs = None
        for n in range(1, n_calls + 1):
            arm(n)
            st, com, proofs, plen = cloak_call(pc, gens, 2, 2, qs, None)
            _, fired = disarm()
            if st != OK:
                assert fired, (n, "an error without a fault")
                assert com == bytes(len(com)) and proofs == bytes(len(proofs)) and plen == 0, (n, st)
                surfaced += 1
            else:
                assert 0 < plen <= STRIDE and verified(com, proofs, plen)[1], (n, "status OK but the proofs do not verify")
            st, com, proofs, plen = cloak_call(pc, gens, 2, 2, qs, None)  # clean, same contexts
            assert st == OK and pc.prover_seed() != bytes(32), (n, st, pc.lib.zkgpu_last_error(pc.h))
            txs, good = verified(com, proofs, plen)
            assert good, (n, "the clean call after the fault")
        assert surfaced >= n_calls // 2, (surfaced, n_calls)
        r = hashlib.shake_256(b"prover draw faults r").digest(64 * BATCH)
        with ThreadPoolExecutor(8) as ex:
            assert all(ex.map(lambda i: oracle.cloak_verify(txs[i].commitments, 2, 2, txs[i].proof, r[64 * i: 64 * i + 64]), range(BATCH)))
        print("prover without seeds: %d runtime calls in a warm call of three slices, %d faults surfaced as errors" % (n_calls, surfaced))
    finally:
        disarm()
        pc.close()
        v.close()
