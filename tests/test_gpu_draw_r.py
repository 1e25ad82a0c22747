"""Verifier randomness drawn by the library on the device paths (d_r == NULL; zkvm_amd/csrc/draw_r.hpp, k_draw_r): every
entry point that takes device pointers, on batches of 70 statements -- one full wavefront and a partial one, four groups of
16 and a remainder of 6 -- with three corrupted statements, two of them in one group.

What the device drew is read back through what the verifier made of it: slot 7 of zkgpu_debug_read("challenges") is
Scalar::from_wide(r) in Montgomery form, r * 2^260 mod l, and must equal from_wide(SHAKE256(seed || LE64(i))[:64]) * 2^260
for the seed zkgpu_debug_read("r_seed") reports -- the definition, computed here with hashlib."""
import ctypes as C
import hashlib

import pytest

from gpu_util import BAD_POINT, GADGET_LABEL, L, bits, describe_range, load_cloak_fixture

pytestmark = pytest.mark.gpu
OK = 0
BATCH = 70
BAD = {20: 0, 27: 1, 40: 2}           # position -> kind (gpu_util.benched_step's three); 20 and 27 share group 1 (one left out of the sum, one culprit)
R260 = pow(2, 260, L)


def draw(seed: bytes, p: int) -> bytes:
    return hashlib.shake_256(seed + p.to_bytes(8, "little")).digest(64)


def mont(r64: bytes) -> int:
    return int.from_bytes(r64, "little") % L * R260 % L


def statements(first: int, count: int, bad):
    """`count` statements of the 2-in/2-out fixture from record `first` on, those at the positions of `bad` corrupted -> (com, proofs, expected bits)"""
    fixture, n_in, n_out, _ = load_cloak_fixture("cloak_2x2_1024.bin")
    coms, proofs, expected = [], [], []
    for i in range(count):
        com, proof = fixture[(first + i) % len(fixture)]
        kind = bad.get(i)
        if kind == 0:        # a commitment that is not a ristretto255 encoding
            com = com[:96] + BAD_POINT + com[128:]
        elif kind == 1:      # IPA scalar a off by one (still canonical)
            a = (int.from_bytes(proof[-64:-32], "little") + 1) % L
            proof = proof[:-64] + a.to_bytes(32, "little") + proof[-32:]
        elif kind == 2:      # a valid proof of a different statement
            proof = fixture[(first + i + 1) % len(fixture)][1]
        coms.append(com); proofs.append(proof); expected.append(0 if kind is not None else 1)
    return b"".join(coms), b"".join(proofs), expected


def bitmap(expected):
    bm = bytearray((len(expected) + 7) // 8)
    for i, b in enumerate(expected):
        bm[i // 8] |= b << (i % 8)
    return bytes(bm)


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


@pytest.fixture(scope="module")
def batch70(ctx, oracle):
    """the batch every cloak test below verifies, resident in HBM, its expected bits held against the oracle's verifier once"""
    _, n_in, n_out, plen = load_cloak_fixture("cloak_2x2_1024.bin")
    com, proofs, expected = statements(100, BATCH, BAD)
    r = hashlib.shake_256(b"draw_r oracle").digest(64 * BATCH)
    assert list(oracle.cloak_verify_batch(com, n_in, n_out, proofs, plen, r, threads=8)) == expected
    d_com, d_proofs = ctx.to_device(com), ctx.to_device(proofs)
    yield dict(n_in=n_in, n_out=n_out, plen=plen, com=com, proofs=proofs, expected=expected, d_com=d_com, d_proofs=d_proofs)
    ctx.free_device(d_com)
    ctx.free_device(d_proofs)


def slot7(c, slots: int, batch: int):
    ch = c.debug_read("challenges", batch * slots * 32)
    assert len(ch) == batch * slots * 32
    return [int.from_bytes(ch[(i * slots + 7) * 32: (i * slots + 7) * 32 + 32], "little") for i in range(batch)], ch


def test_synchronous_call_draws_r_from_a_fresh_seed_and_equals_the_call_with_those_bytes(ctx, gens, batch70):
    from zkvm_amd.verifier import Verifier
    b = batch70
    v = Verifier(ctx, gens)
    try:
        slots = v.plan_layout(b["n_in"], b["n_out"])["slots"]
        bm = v.verify_packed_gpu_dev(b["n_in"], b["n_out"], BATCH, b["d_com"], b["d_proofs"], b["plen"], None)
        assert bits(bm, BATCH) == b["expected"]
        seed = ctx.debug_read("r_seed", 32)
        assert len(seed) == 32 and seed != bytes(32)
        got, ch = slot7(ctx, slots, BATCH)
        r = b"".join(draw(seed, i) for i in range(BATCH))
        assert got == [mont(r[64 * i: 64 * i + 64]) for i in range(BATCH)]
        # the same statements with those 64-byte strings as the caller's d_r: the same bytes everywhere
        d_r = ctx.to_device(r)
        try:
            assert v.verify_packed_gpu_dev(b["n_in"], b["n_out"], BATCH, b["d_com"], b["d_proofs"], b["plen"], d_r) == bm
            assert ctx.debug_read("challenges", len(ch)) == ch
            assert ctx.debug_read("r_seed", 32) == bytes(32)          # (that batch brought its own r)
        finally:
            ctx.free_device(d_r)
        assert bits(v.verify_packed_gpu_dev(b["n_in"], b["n_out"], BATCH, b["d_com"], b["d_proofs"], b["plen"]), BATCH) == b["expected"]
        again = ctx.debug_read("r_seed", 32)
        assert again != bytes(32) and again != seed
        assert slot7(ctx, slots, BATCH)[0] == [mont(draw(again, i)) for i in range(BATCH)]
    finally:
        v.close()


def test_submitted_batch_keeps_its_drawn_r_through_the_ungrouped_rerun(ctx, gens, batch70):
    from zkvm_amd.verifier import Verifier
    b = batch70
    v = Verifier(ctx, gens)
    try:
        slots = v.plan_layout(b["n_in"], b["n_out"])["slots"]
        ctx.set_locate_mode(2)              # a failed group's culprit is located (the default from 2048 statements on): what the hook makes "unresolved"
        before = ctx.force_regroup(True)
        v.submit_packed_gpu_dev(b["n_in"], b["n_out"], BATCH, b["d_com"], b["d_proofs"], b["plen"], None)
        seed = ctx.debug_read("r_seed", 32)
        assert seed != bytes(32)
        assert bits(ctx.verify_wait(), BATCH) == b["expected"]
        assert ctx.force_regroup(False) == before + 1                  # the batch was run again, ungrouped, from the same r
        assert ctx.debug_read("r_seed", 32) == seed
        assert slot7(ctx, slots, BATCH)[0] == [mont(draw(seed, i)) for i in range(BATCH)]
    finally:
        ctx.force_regroup(False)
        ctx.set_locate_mode(0)
        v.close()


def test_described_plan_submitted_without_r(ctx, gens, oracle):
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import R1csVerifier
    n, bad = 5, 3
    rv = R1csVerifier(ctx, gens, R1csDescription(GADGET_LABEL, *describe_range(8)))
    coms, proofs = [], []
    for i in range(n):
        rc, com, proof = oracle.gadget_prove(1, 8, [17 + i], hashlib.sha256(b"draw_r range %d" % i).digest())
        assert rc == 0
        if i == bad:
            a = (int.from_bytes(proof[-64:-32], "little") + 1) % L
            proof = proof[:-64] + a.to_bytes(32, "little") + proof[-32:]
        coms.append(com); proofs.append(proof)
    plen = len(proofs[0])
    assert all(len(p) == plen for p in proofs)
    r = hashlib.shake_256(b"draw_r range oracle").digest(64 * n)
    expected = [int(oracle.gadget_verify(1, 8, coms[i], proofs[i], r[64 * i: 64 * i + 64])) for i in range(n)]
    assert expected == [0 if i == bad else 1 for i in range(n)]
    d_com, d_proofs = ctx.to_device(b"".join(coms)), ctx.to_device(b"".join(proofs))
    try:
        slots = rv.info()["slots"]
        ctx._check(ctx.lib.zkgpu_r1cs_verify_submit_dev(ctx.h, gens.points.h, rv.h, n, d_com, d_proofs, plen, None))
        ctx._pending_batch = n
        assert bits(ctx.verify_wait(), n) == expected
        seed = ctx.debug_read("r_seed", 32)
        assert seed != bytes(32)
        assert slot7(ctx, slots, n)[0] == [mont(draw(seed, i)) for i in range(n)]
    finally:
        ctx.free_device(d_com)
        ctx.free_device(d_proofs)
        rv.close()


@pytest.fixture(scope="module")
def tickets96(ctx, oracle, batch70):
    """three tickets of 32 statements in HBM, A's randomness among them; the expected bits held against the oracle's verifier once"""
    n_in, n_out, plen = batch70["n_in"], batch70["n_out"], batch70["plen"]
    each = 32
    sets = [statements(300 + 40 * k, each, {3 + k: k, 17: 1} if k != 1 else {9: 2}) for k in range(3)]
    r_a = hashlib.shake_256(b"draw_r ticket A").digest(64 * each)
    for com, proofs, expected in sets:
        assert list(oracle.cloak_verify_batch(com, n_in, n_out, proofs, plen, r_a, threads=8)) == expected
    dev = [[ctx.to_device(com), ctx.to_device(proofs)] for com, proofs, _ in sets]
    d_ra = ctx.to_device(r_a)
    yield dict(each=each, expected=[e for _, _, e in sets], dev=dev, r_a=r_a, d_ra=d_ra)
    for d in dev:
        for x in d:
            ctx.free_device(x)
    ctx.free_device(d_ra)


def _drawing_lane(bv):
    """the one lane of the verifier whose last device batch drew randomness -> (its context view, the seed)"""
    found = [(c, c.debug_read("r_seed", 32)) for c in (bv.lane(i) for i in range(bv.lanes()))]
    found = [(c, s) for c, s in found if s != bytes(32)]
    assert len(found) == 1
    return found[0]


@pytest.mark.parametrize("how", ["submit_dev", "submit_many_dev, one NULL entry", "submit_many_dev, NULL array"])
def test_tickets_with_and_without_r_in_one_device_batch(ctx, gens, batch70, tickets96, how):
    """merge target 96, three tickets of 32 -> ONE device batch: A brings its r, B and C get r(seed, 32 ..) and r(seed, 64 ..)"""
    from zkvm_amd.verifier import BlockVerifier, Verifier
    n_in, n_out, plen = batch70["n_in"], batch70["n_out"], batch70["plen"]
    each, dev, r_a, d_ra = tickets96["each"], tickets96["dev"], tickets96["r_a"], tickets96["d_ra"]
    v = Verifier(ctx, gens)
    slots = v.plan_layout(n_in, n_out)["slots"]
    v.close()
    bv = BlockVerifier(ctx, gens, batches_in_flight=2)
    try:
        bv.set_merge(3 * each)
        all_null = how == "submit_many_dev, NULL array"
        if how == "submit_dev":
            ts = [bv.submit_dev(n_in, n_out, each, dev[k][0], dev[k][1], plen, d_ra if k == 0 else None) for k in range(3)]
        else:
            ts = bv.submit_many_dev(n_in, n_out, each, [d[0] for d in dev], [d[1] for d in dev], plen, None if all_null else [d_ra, None, None])
        for k in range(3):
            assert bits(bv.wait(ts[k]), each) == tickets96["expected"][k], k
        lane, seed = _drawing_lane(bv)
        got, _ = slot7(lane, slots, 3 * each)
        first_drawn = 0 if all_null else each
        if not all_null:
            assert got[:each] == [mont(r_a[64 * i: 64 * i + 64]) for i in range(each)]
        assert got[first_drawn:] == [mont(draw(seed, i)) for i in range(first_drawn, 3 * each)]
    finally:
        bv.close()


def test_lone_ticket_without_r_is_drawn_into_the_lane(ctx, gens, batch70):
    """one ticket below the merge target, waited for at once: it leaves unmerged, and its r is the lane's, not the caller's"""
    from zkvm_amd.verifier import BlockVerifier, Verifier
    b = batch70
    v = Verifier(ctx, gens)
    slots = v.plan_layout(b["n_in"], b["n_out"])["slots"]
    v.close()
    bv = BlockVerifier(ctx, gens, batches_in_flight=2)
    try:
        bv.set_merge(96)
        seeds = []
        for _ in range(2):
            t = bv.submit_dev(b["n_in"], b["n_out"], BATCH, b["d_com"], b["d_proofs"], b["plen"], None)
            assert bits(bv.wait(t), BATCH) == b["expected"]
            lane, seed = _drawing_lane(bv)
            assert slot7(lane, slots, BATCH)[0] == [mont(draw(seed, i)) for i in range(BATCH)]
            seeds.append(seed)
        assert seeds[0] != seeds[1]
    finally:
        bv.close()


@pytest.mark.timeout(300, method="thread")
def test_call_without_r_fails_closed_at_every_runtime_call(ctx, gens):
    """zkgpu_debug_fail_after at every runtime call of a 16-statement d_r == NULL call in turn (the gate answers "failed" without
    touching the device): a nonzero status and an all-zero bitmap every time, and the next clean call on the same context is right"""
    from zkvm_amd.verifier import Verifier
    _, n_in, n_out, plen = load_cloak_fixture("cloak_2x2_1024.bin")
    n = 16
    com, proofs, expected = statements(500, n, {2: 1, 11: 2})
    want = bitmap(expected)
    d_com, d_proofs = ctx.to_device(com), ctx.to_device(proofs)
    lib = ctx.lib
    v = Verifier(ctx, gens)
    plan = v._plan(n_in, n_out)

    def call():
        bm = C.create_string_buffer(b"\xff" * len(want), len(want))
        st = lib.zkgpu_cloak_verify_batch_gpu_dev(ctx.h, gens.points.h, plan, n, d_com, d_proofs, plen, None, bm)
        return st, bm.raw

    try:
        assert call() == (OK, want)                       # (workspaces exist from here on)
        lib.zkgpu_debug_fail_after(ctx.h, 1 << 60, None)  # counts, never fires
        assert call() == (OK, want)
        n_calls = int(lib.zkgpu_debug_fail_after(ctx.h, 0, None))
        assert n_calls >= 10
        for k in range(1, n_calls + 1):
            lib.zkgpu_debug_fail_after(ctx.h, k, None)
            st, bm = call()
            fired = C.c_longlong(0)
            lib.zkgpu_debug_fail_after(ctx.h, 0, C.byref(fired))
            assert fired.value == 1, k
            assert st != OK and bm == bytes(len(want)), (k, st, lib.zkgpu_last_error(ctx.h).decode())
            assert call() == (OK, want), k
        print("fail-closed without r: %d runtime calls, each failed in turn" % n_calls)
    finally:
        lib.zkgpu_debug_fail_after(ctx.h, 0, None)
        v.close()
        ctx.free_device(d_com)
        ctx.free_device(d_proofs)
