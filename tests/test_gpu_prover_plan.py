"""Which kernels a device prover call queues, in which order and how often, and how many HIP runtime calls a warm call
makes -- held against tests/golden/prover_launch_sequences.json, which was recorded before prove_device was rearranged to
walk a PvCallPlan (zkvm_amd/csrc/prover_call_plan.hpp) and is never regenerated from the code under test.  Five statements
per call, tables at 8 bits, generators for the next power of two at or above n: the smallest shapes that take every guard
of the plan's step list both ways (m = 0 aside, which no proof of these gadgets has)."""
import hashlib
import json
import os

import pytest

from gpu_util import GADGET_LABEL, L, describe_range, describe_shuffle, gadget_witness

pytestmark = pytest.mark.gpu
BATCH = 5
FLAVOR = bytes([3]) + bytes(31)


def _statement_seed(call_seed: bytes, i: int) -> bytes:
    return hashlib.shake_256(call_seed + b"statement" + i.to_bytes(8, "little")).digest(32)


def prover_launch_sequences(oracle):
    """Every call on one fresh context, profiled on its own -> {call: [[profile entry, launches], ...]} in the order the
    entries were first queued (three slices: sorted by name, the slices' profiles are merged), plus the count of gated
    runtime calls of a warm range call.  Every proof is held against the oracle prover's bytes here, so a sequence that
    proves nothing is never recorded or compared."""
    import ctypes as C
    import random
    from zkvm_amd import Context
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import BulletproofGens, Prover, R1csProver
    out = {}
    ctx = Context(0)
    ctx.profile(True)
    ctx.set_prover_mode(0)

    def profiled(name, fn, in_order=True):
        ctx.profile_reset()
        fn()
        got = [[k, v[0]] for k, v in ctx.profile_read().items()]
        out[name] = got if in_order else sorted(got)

    def described(kind, param, values):
        m, n1, n, labels, cons = describe_range(param) if kind == 1 else describe_shuffle(param)
        cap = 1
        while cap < max(n, 1):
            cap *= 2
        gens = BulletproofGens(ctx, cap, table_bits=8)
        desc = R1csDescription(GADGET_LABEL, m, n1, n, labels, cons)
        seeds = [hashlib.sha256(b"prover plan %d %d %d" % (kind, param, i)).digest() for i in range(BATCH)]
        mult_def = gadget_witness(kind, param, values[0])[0]
        given = [gadget_witness(kind, param, v)[1] for v in values]
        pv = R1csProver(ctx, gens, desc, mult_def, host_threads=2)

        def call():
            coms, proofs = pv.prove(values, given, seeds)
            for i in range(BATCH):
                rc, want_com, want_proof = oracle.gadget_prove(kind, param, values[i], seeds[i])
                assert rc == 0 and (coms[i], proofs[i]) == (want_com, want_proof), (kind, param, i)
        return call, gens

    def cloak(gens, label):
        qs = [[5 + i, 9, 4 + i, 10] for i in range(BATCH)]
        made = Prover(ctx, gens, host_threads=2).prove(2, 2, qs, [[FLAVOR] * 4] * BATCH)       # seeds=None: drawn
        call_seed = ctx.prover_seed()
        assert call_seed != bytes(32), label
        for i, t in enumerate(made):
            rc, com, proof, _ = oracle.cloak_prove(qs[i], [FLAVOR] * 4, 2, 2, _statement_seed(call_seed, i))
            assert rc == 0 and (t.commitments, t.proof) == (com, proof), (label, i)

    gens = None
    try:
        call, gens = described(1, 8, [[(17 * i + 3) % 256] for i in range(BATCH)])
        profiled("range 8", call)
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 1 << 60, None)                       # counts, never fires
        call()
        fired = C.c_longlong(0)
        seen = int(ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, C.byref(fired)))
        assert fired.value == 0
        out["range 8, warm: runtime calls"] = seen
        gens.close()
        rng = random.Random(2)
        values = []
        for _ in range(BATCH):
            xs = [rng.randrange(L) for _ in range(2)]
            values.append(xs + sorted(xs))
        call, gens = described(2, 2, values)
        profiled("shuffle 2", call)
        gens.close()
        gens = BulletproofGens(ctx, 256, table_bits=8)
        profiled("cloak 2x2, seeds drawn", lambda: cloak(gens, "one slice"))
        ctx.set_prover_mode(16 + 3)
        profiled("cloak 2x2, seeds drawn, three slices", lambda: cloak(gens, "three slices"), in_order=False)
        assert int.from_bytes(ctx.debug_read("prover_slices", 4), "little") == 3
    finally:
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None)
        if gens is not None:
            gens.close()
        ctx.close()
    return out


def test_prover_launch_sequences_and_warm_runtime_calls_are_the_recorded_ones(oracle):
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "prover_launch_sequences.json")))
    got = prover_launch_sequences(oracle)
    assert sorted(got) == sorted(gold)
    for name in gold:
        assert got[name] == gold[name], name
