"""zkgpu_r1cs_verify_mixed / zkgpu_r1cs_verify_mixed_submit: statements of different constraint systems -- described
systems of every kind the tests know (single and two phase, random systems with challenges, the 1032-constraint program)
and cloak shapes -- verified together in one device call.  Every bit equals the per-plan calls of
zkgpu_r1cs_verify_batch_gpu on the same statements and randomness, and the oracle's verdict wherever it has the statement."""
import ctypes as C
import hashlib
import random

import pytest

from gpu_util import GADGET_LABEL, L, bits, describe_range, describe_ranges, describe_shuffle, gadget_witness, load_cloak_fixture, random_system

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    from zkvm_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gens(ctx):
    from zkvm_amd.verifier import BulletproofGens
    g = BulletproofGens(ctx, 512, table_bits=8)         # padded n up to 512: the 1032-constraint program
    yield g
    g.close()


def _prove(ctx, gens, desc, mult_def, vals, givens, tag):
    from zkvm_amd.verifier import R1csProver
    seeds = [hashlib.sha256(b"mixed %s %d" % (tag, i)).digest() for i in range(len(vals))]
    return R1csProver(ctx, gens, desc, mult_def, host_threads=8).prove(vals, givens, seeds)


@pytest.fixture(scope="module")
def suite(ctx, gens, oracle):
    """Eight plans and valid statements for each: (plan handles, statements, the MixedR1csVerifier over the eight plans);
    a statement is (plan, commitments, proof, oracle check or None)."""
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import MixedR1csVerifier, R1csVerifier
    rng = random.Random(2024)
    plans, keep, stmts = [], [], []

    def gadget(kind, param, count):
        m, n1, n, labels, cons = describe_range(param) if kind == 1 else describe_shuffle(param) if kind == 2 else describe_ranges(param)
        desc = R1csDescription(GADGET_LABEL, m, n1, n, labels, cons)
        v = R1csVerifier(ctx, gens, desc)
        keep.append(v)
        vals, givens = [], []
        mult_def = None
        for _ in range(count):
            if kind == 1:
                values = [rng.randrange(1 << param)]
            elif kind == 3:
                values = [rng.randrange(1 << 64) for _ in range(param)]
            else:
                xs = [rng.randrange(L) for _ in range(param)]
                values = xs + sorted(xs)
            mult_def, given = gadget_witness(kind, param, values)
            vals.append(values)
            givens.append(given)
        coms, proofs = _prove(ctx, gens, desc, mult_def, vals, givens, b"g %d %d" % (kind, param))
        p = len(plans)
        plans.append(v)
        stmts.extend((p, coms[i], proofs[i], ("gadget", kind, param)) for i in range(count))

    def system(m, n1, n2, n_chal, count, label):
        (m, n1, n, labels, cons), mult_def, values, given = random_system(rng, m, n1, n2, n_chal)
        desc = R1csDescription(label, m, n1, n, labels, cons)
        v = R1csVerifier(ctx, gens, desc)
        keep.append(v)
        coms, proofs = _prove(ctx, gens, desc, mult_def, [values] * count, [given] * count, label)
        p = len(plans)
        plans.append(v)
        stmts.extend((p, coms[i], proofs[i], None) for i in range(count))

    gadget(1, 8, 150)                       # 0: range(8), single phase, k = 3
    gadget(1, 64, 100)                      # 1: range(64)
    gadget(2, 5, 60)                        # 2: shuffle(5), two phases
    gadget(3, 8, 12)                        # 3: the 1032-constraint program, padded n = 512
    system(1, 4, 3, 2, 40, b"mixed system A")   # 4: challenges; m = 1 and padded n = 8 like plan 0
    system(2, 9, 4, 3, 40, b"mixed system B")   # 5
    fix, n_in, n_out, _ = load_cloak_fixture()
    assert (n_in, n_out) == (2, 2)
    plans.append((2, 2))                    # 6: cloak 2x2 (committed fixture)
    stmts.extend((6, c, p, ("cloak", 2, 2)) for c, p in fix[:200])
    plans.append((3, 2))                    # 7: cloak 3x2 (oracle prover)
    com, proofs = oracle.cloak_prove_batch(24, 3, 2, b"mixed 3x2".ljust(32, b"\0"), threads=8)
    stmts.extend((7, com[320 * i: 320 * (i + 1)], proofs[i], ("cloak", 3, 2)) for i in range(24))
    mv = MixedR1csVerifier(ctx, gens, plans)
    yield mv.handles, stmts, mv
    mv.close()
    for v in keep:
        v.close()


def _oracle_bit(oracle, chk, com, proof, r):
    if chk is None:
        return None
    if chk[0] == "gadget":
        return int(oracle.gadget_verify(chk[1], chk[2], com, proof, r))
    return int(oracle.cloak_verify(com, chk[1], chk[2], proof, r))


def _per_plan(ctx, gens, plans, idx, coms, proofs, r):
    """the reference: one zkgpu_r1cs_verify_batch_gpu call per (plan, proof length)"""
    out = [None] * len(idx)
    groups = {}
    for i, p in enumerate(idx):
        groups.setdefault((p, len(proofs[i])), []).append(i)
    for (p, plen), members in groups.items():
        n = len(members)
        bm = C.create_string_buffer((n + 7) // 8)
        rc = ctx.lib.zkgpu_r1cs_verify_batch_gpu(ctx.h, gens.points.h, C.c_void_p(plans[p]), n, b"".join(coms[i] for i in members),
                                                 b"".join(proofs[i] for i in members), plen,
                                                 b"".join(r[64 * i: 64 * i + 64] for i in members), bm)
        assert rc == 0
        for j, i in enumerate(members):
            out[i] = bits(bm.raw, n)[j]
    return out


def test_mixed_batch_equals_per_plan_calls_and_oracle(ctx, gens, oracle, suite):
    """~630 statements over 8 plans (single / two phase, random systems with challenges, the 1032-constraint program,
    cloak 2x2 and 3x2) in shuffled order with ~5 % corrupted: flipped bytes, swapped commitments, wrong lengths,
    non-canonical scalars, and a valid proof filed under another plan of the same proof length."""
    plans, stmts, mv = suite
    rng = random.Random(7)
    order = list(range(len(stmts)))
    rng.shuffle(order)
    idx = [stmts[k][0] for k in order]
    coms = [bytearray(stmts[k][1]) for k in order]
    proofs = [bytearray(stmts[k][2]) for k in order]
    chks = [stmts[k][3] for k in order]
    n = len(idx)
    bad = rng.sample(range(n), 32)
    for j, i in enumerate(list(bad)):
        kind = j % 5
        if kind == 0:                                   # a byte of T_1 .. T_6, t_x, t_x_blinding (either wire form)
            proofs[i][1 + 32 * (6 + j % 7) + (j % 31)] ^= 1 << (j % 8)
        elif kind == 1:                                 # commitments of two statements of the same plan swapped
            o = next(x for x in range(n) if x != i and idx[x] == idx[i] and x not in bad)
            if coms[o] == coms[i]:                      # (the random systems commit the same values: corrupt instead)
                coms[i][5] ^= 4
            else:
                coms[i], coms[o] = coms[o], coms[i]
                bad.append(o)
        elif kind == 2:                                 # wrong length
            proofs[i] = proofs[i][:-32]
        elif kind == 3:                                 # t_x not canonical (>= l): element 11, or 8 in the one-phase wire form
            at = 1 + 32 * (11 if proofs[i][0] == 1 else 8)
            proofs[i][at: at + 32] = (L + 5).to_bytes(32, "little")
        else:                                           # a valid range(8) proof filed under system A (same m, same length)
            src = next(k for k in range(len(stmts)) if stmts[k][0] == 0)
            idx[i], coms[i], proofs[i], chks[i] = 4, bytearray(stmts[src][1]), bytearray(stmts[src][2]), None
    coms = [bytes(c) for c in coms]
    proofs = [bytes(p) for p in proofs]
    r = hashlib.shake_256(b"mixed r").digest(64 * n)
    got = bits(mv.verify(idx, coms, proofs, r), n)
    want = _per_plan(ctx, gens, plans, idx, coms, proofs, r)
    assert got == want
    for i in range(n):
        o = _oracle_bit(oracle, chks[i], coms[i], proofs[i], r[64 * i: 64 * i + 64])
        assert o is None or o == got[i], i
    assert sum(got) >= n - len(bad) and sum(got) <= n - 25          # the corruptions are rejected, the rest accepted
    for i in set(bad):
        assert got[i] == 0, i


def test_one_plan_equals_the_homogeneous_call(ctx, gens, oracle):
    """n_plans = 1 over the full 1024-statement cloak fixture: the bitmap of zkgpu_cloak_verify_batch_gpu"""
    from zkvm_amd.verifier import MixedR1csVerifier, Verifier
    fix, n_in, n_out, plen = load_cloak_fixture()
    coms = [c for c, _ in fix]
    proofs = [bytearray(p) for _, p in fix]
    for i in range(3, len(proofs), 97):
        proofs[i][1 + 32 * 12 + 3] ^= 2
    proofs = [bytes(p) for p in proofs]
    n = len(proofs)
    r = hashlib.shake_256(b"one plan").digest(64 * n)
    cv = Verifier(ctx, gens)
    want = cv.verify_packed_gpu(n_in, n_out, n, b"".join(coms), b"".join(proofs), plen, r)
    mv = MixedR1csVerifier(ctx, gens, [(n_in, n_out)])
    got = mv.verify([0] * n, coms, proofs, r)
    mv.close()
    cv.close()
    assert got == want
    assert bits(got, n).count(0) == len(range(3, n, 97))


def _profiled(ctx, mv, idx, coms, proofs, r):
    ctx.profile(True)
    ctx.profile_reset()
    try:
        bm = mv.verify(idx, coms, proofs, r)
        return bm, {k: v[0] for k, v in ctx.profile_read().items()}
    finally:
        ctx.profile(False)


def test_launch_count_does_not_depend_on_the_number_of_plans(ctx, gens, suite):
    """the same batch size over 2 distinct plans and over 8: the same launches, kernel by kernel -- one per stage, the scalar
    preparation once per LDS class present (the 1032-constraint program takes a CU's LDS alone, the others share it)"""
    plans, stmts, mv = suite
    by_plan = {}
    for s in stmts:
        by_plan.setdefault(s[0], []).append(s)
    batch = 192
    two = [by_plan[p][i % len(by_plan[p])] for i, p in zip(range(batch), [0, 3] * batch)]
    eight = [by_plan[p][i // 8 % len(by_plan[p])] for i, p in zip(range(batch), list(range(8)) * batch)]
    small = [by_plan[p][i % len(by_plan[p])] for i, p in zip(range(batch), [0, 6] * batch)]
    r = hashlib.shake_256(b"launches").digest(64 * batch)
    counts = []
    for sel in (two, eight, small):
        bm, prof = _profiled(ctx, mv, [s[0] for s in sel], [s[1] for s in sel], [s[2] for s in sel], r)
        assert bits(bm, batch) == [1] * batch
        counts.append(prof)
    assert counts[0] == counts[1]
    assert counts[0]["k_mx_prepare"] == 2 and counts[0]["k_mx_proof_unpack"] == 1 and counts[0]["k_mx_transcript_coop"] == 1
    assert counts[2]["k_mx_prepare"] == 1                                     # small plans only: one LDS class
    assert {k: v for k, v in counts[2].items() if k != "k_mx_prepare"} == {k: v for k, v in counts[0].items() if k != "k_mx_prepare"}
    assert not any(k in counts[0] for k in ("k_prepare", "k_transcript", "k_challenges"))   # the homogeneous stages stay out


def test_submit_wait_and_os_randomness(ctx, gens, suite):
    """submit + zkgpu_verify_wait = the synchronous call; a synchronous call while a batch is submitted is refused with
    ZKGPU_EINVAL and a zero bitmap; r_bytes = NULL accepts every valid statement"""
    plans, stmts, mv = suite
    sel = stmts[::5]
    n = len(sel)
    idx, coms = [s[0] for s in sel], [s[1] for s in sel]
    proofs = [bytearray(s[2]) for s in sel]
    proofs[3][1 + 32 * 9] ^= 1
    proofs = [bytes(p) for p in proofs]
    r = hashlib.shake_256(b"submit").digest(64 * n)
    want = mv.verify(idx, coms, proofs, r)
    assert bits(want, n) == [0 if i == 3 else 1 for i in range(n)]
    mv.submit(idx, coms, proofs, r)
    bm = C.create_string_buffer(b"\xff" * ((n + 7) // 8))
    ia = (C.c_uint32 * n)(*idx)
    offs = [0]
    for p in proofs:
        offs.append(offs[-1] + len(p))
    oa = (C.c_uint64 * (n + 1))(*offs)
    rc = ctx.lib.zkgpu_r1cs_verify_mixed(ctx.h, gens.points.h, mv._plans, len(plans), n, ia, b"".join(coms), b"".join(proofs), oa, r, bm)
    assert rc == EINVAL and bm.raw[: (n + 7) // 8] == bytes((n + 7) // 8)
    assert mv.wait() == want
    assert bits(mv.verify(idx, coms, proofs, None), n) == bits(want, n)          # getrandom
    assert mv.verify([], [], [], None) == b""                                    # batch 0


def test_argument_errors_zero_the_bitmap_and_leave_the_context_usable(ctx, gens, suite):
    """plan index out of range, a NULL plan, a plan needing more generators than the set holds, bad offsets:
    ZKGPU_EINVAL and a zero bitmap before any device work; the context then verifies a correct batch as usual"""
    from zkvm_amd.native import R1csDescription
    plans, stmts, mv = suite
    sel = [stmts[0], stmts[200], stmts[400], stmts[-1]]
    n = len(sel)
    idx, coms, proofs = [s[0] for s in sel], b"".join(s[1] for s in sel), [s[2] for s in sel]
    offs = [0]
    for p in proofs:
        offs.append(offs[-1] + len(p))
    r = hashlib.shake_256(b"errors").digest(64 * n)
    m, n1, nm, labels, cons = describe_range(8)
    big = C.c_void_p()
    desc = R1csDescription(GADGET_LABEL, m, n1, nm, labels, cons)
    assert ctx.lib.zkgpu_r1cs_plan_create(ctx.h, C.byref(desc.struct), 1024, C.byref(big)) == 0     # 2 + 2 x 1024 generators
    try:
        def call(plan_list, index, offsets):
            pa = (C.c_void_p * len(plan_list))(*plan_list)
            bm = C.create_string_buffer(b"\xff" * ((n + 7) // 8))
            rc = ctx.lib.zkgpu_r1cs_verify_mixed(ctx.h, gens.points.h, pa, len(plan_list), n, (C.c_uint32 * n)(*index), coms,
                                                 b"".join(proofs), (C.c_uint64 * (n + 1))(*offsets), r, bm)
            return rc, bm.raw[: (n + 7) // 8]
        zero = bytes((n + 7) // 8)
        assert call(plans, idx[:3] + [len(plans)], offs) == (EINVAL, zero)
        assert call(plans[:-1] + [None], idx, offs) == (EINVAL, zero)
        assert call(plans + [big.value], idx, offs) == (EINVAL, zero)
        assert call(plans, idx, [0, offs[2], offs[1]] + offs[3:]) == (EINVAL, zero)
        assert call(plans, idx, [1] + offs[1:]) == (EINVAL, zero)
        rc, bm = call(plans, idx, offs)
        assert rc == 0 and bits(bm, n) == [1] * n
        assert mv.verify(idx, [s[1] for s in sel], proofs, r) == bm
    finally:
        ctx.lib.zkgpu_r1cs_plan_destroy(big)


def test_one_lane_transcript_equals_per_plan_calls_and_oracle(ctx, gens, oracle, suite):
    """the one-lane-per-statement transcript (what a call above 1536 statements takes) with its per-plan runs padded to whole
    wavefronts: runs of lengths that are no multiple of 64, in shuffled order, with corruptions -- the verdicts of the
    per-plan calls and of the oracle, and k_mx_transcript is what ran"""
    plans, stmts, mv = suite
    rng = random.Random(11)
    by_plan = {}
    for s_ in stmts:
        by_plan.setdefault(s_[0], []).append(s_)
    sel = []
    for p, take in zip(range(8), (97, 65, 33, 7, 1, 40, 130, 24)):
        sel += by_plan[p][:take]
    rng.shuffle(sel)
    n = len(sel)
    idx, coms, chks = [s_[0] for s_ in sel], [s_[1] for s_ in sel], [s_[3] for s_ in sel]
    proofs = [bytearray(s_[2]) for s_ in sel]
    bad = rng.sample(range(n), 20)
    for j, i in enumerate(bad):
        if j % 3 == 0:
            proofs[i][1 + 32 * (6 + j % 7) + j] ^= 0x20
        elif j % 3 == 1:
            at = 1 + 32 * (12 if proofs[i][0] == 1 else 9)      # t_x_blinding not canonical
            proofs[i][at: at + 32] = (L + 1).to_bytes(32, "little")
        else:
            proofs[i] = proofs[i] + b"\0"
    proofs = [bytes(p) for p in proofs]
    r = hashlib.shake_256(b"one lane").digest(64 * n)
    ctx.set_transcript_mode(1)
    try:
        bm, prof = _profiled(ctx, mv, idx, coms, proofs, r)
    finally:
        ctx.set_transcript_mode(0)
    assert prof.get("k_mx_transcript") == 1 and "k_mx_transcript_coop" not in prof
    got = bits(bm, n)
    assert got == _per_plan(ctx, gens, plans, idx, coms, proofs, r)
    for i in range(n):
        o = _oracle_bit(oracle, chks[i], coms[i], proofs[i], r[64 * i: 64 * i + 64])
        assert o is None or o == got[i], i
    assert [i for i in range(n) if not got[i]] == sorted(bad)
    assert bits(mv.verify(idx, coms, proofs, r), n) == got                    # the cooperative form: the same bits


def test_bindings_check_commitment_sizes_and_plan_indices(ctx, gens, suite):
    """the library reads 32 m bytes of commitments per statement, m from its plan: the binding refuses anything else (and
    out-of-range plan indices, and plans that have been closed) before the call"""
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import MixedR1csVerifier, R1csVerifier
    plans, stmts, mv = suite
    sel = [stmts[0], stmts[300], stmts[-1]]
    idx, coms, proofs = [s_[0] for s_ in sel], [s_[1] for s_ in sel], [s_[2] for s_ in sel]
    with pytest.raises(ValueError):
        mv.verify(idx, [coms[0][:-32]] + coms[1:], proofs)                     # one commitment short
    with pytest.raises(ValueError):
        mv.verify(idx, coms[:2] + [coms[2] + bytes(32)], proofs)               # one too many
    with pytest.raises(ValueError):
        mv.verify(idx[:2] + [len(plans)], coms, proofs)
    with pytest.raises(ValueError):
        mv.submit(idx, [coms[0][:-1]] + coms[1:], proofs)
    m, n1, n, labels, cons = describe_range(8)
    v = R1csVerifier(ctx, gens, R1csDescription(GADGET_LABEL, m, n1, n, labels, cons))
    own = MixedR1csVerifier(ctx, gens, [v])
    assert bits(own.verify([0], [stmts[0][1]], [stmts[0][2]]), 1) == [1]
    v.close()
    with pytest.raises(ValueError):
        own.verify([0], [stmts[0][1]], [stmts[0][2]])                          # its plan is gone
    assert bits(mv.verify(idx, coms, proofs), 3) == [1, 1, 1]
