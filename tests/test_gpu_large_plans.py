"""Statements whose scalar preparation does not fit a CU's LDS (large_prep.hpp): cloak shapes from 12x12 up to the 64x64
maximum and described programs past 160 KiB get a plan, and every device path -- homogeneous calls (pipelined and
synchronous), mixed calls, the zkgpu_verifier blocks and tickets -- gives the oracle's and the host-prepared path's bits.
ZKGPU_TEST_LARGE_PREP=1 (a test hook) sends small plans down the same path: their scalars must not change by a byte."""
import ctypes as C
import hashlib
import random

import pytest

from gpu_util import GADGET_LABEL, L, bits, describe_ranges, describe_shuffle, load_cloak_fixture

pytestmark = pytest.mark.gpu

EINVAL = -1
LARGE_KERNELS = ("k_lp_head", "k_lp_flatten", "k_lp_gens", "k_lp_tail")


@pytest.fixture(scope="module")
def ctx():
    from zkvm_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gens(ctx):
    from zkvm_amd.verifier import BulletproofGens
    g = BulletproofGens(ctx, 2048, table_bits=8)
    yield g
    g.close()


def _cloak(oracle, count, n_in, n_out, tag):
    from zkvm_amd.verifier import CloakTx
    com, proofs = oracle.cloak_prove_batch(count, n_in, n_out, hashlib.sha256(tag).digest(), threads=16)
    w = 64 * (n_in + n_out)
    return [CloakTx(n_in, n_out, com[w * i: w * (i + 1)], proofs[i]) for i in range(count)]


def _corrupt(txs, rng, n_bad):
    """flipped proof scalar, swapped commitments, non-canonical t_x, identity T_1, the IPA's b flipped; -> positions"""
    from zkvm_amd.verifier import CloakTx
    bad = rng.sample(range(len(txs)), n_bad)
    for j, i in enumerate(bad):
        t = txs[i]
        p, cm = bytearray(t.proof), t.commitments
        kind = j % 5
        if kind == 0:
            p[1 + 32 * 12 + 3] ^= 0x10                                   # t_x_blinding
        elif kind == 1:
            o = (i + 1) % len(txs)
            cm = txs[o].commitments if txs[o].commitments != cm else bytes(64) + cm[64:]
        elif kind == 2:
            p[1 + 32 * 11: 1 + 32 * 12] = (L + 5).to_bytes(32, "little")  # t_x not canonical
        elif kind == 3:
            p[1 + 32 * 6: 1 + 32 * 7] = bytes(32)                         # T_1 = identity
        else:
            p[-20] ^= 1                                                  # b
        txs[i] = CloakTx(t.n_in, t.n_out, cm, bytes(p))
    return bad


def _want(oracle, txs, r):
    return [int(oracle.cloak_verify(t.commitments, t.n_in, t.n_out, t.proof, r[64 * i: 64 * i + 64])) for i, t in enumerate(txs)]


def _profiled(ctx, fn):
    ctx.profile(True)
    ctx.profile_reset()
    try:
        out = fn()
        return out, {k: v[0] for k, v in ctx.profile_read().items()}
    finally:
        ctx.profile(False)


def _plan_rc(ctx, n_in, n_out, cap):
    h = C.c_void_p()
    rc = ctx.lib.zkgpu_cloak_plan_create(ctx.h, n_in, n_out, cap, C.byref(h))
    info = None
    if rc == 0:
        vals = [C.c_uint32() for _ in range(5)]
        assert ctx.lib.zkgpu_cloak_plan_info(h, *[C.byref(v) for v in vals]) == 0
        info = [v.value for v in vals]
        ctx.lib.zkgpu_cloak_plan_destroy(h)
    return rc, info


def test_plans_past_the_lds_limit_are_made(ctx):
    """12x12 .. 64x64: a plan over enough generators, with the multipliers and padded n of upstream's gadget; over too few
    generators still ZKGPU_EINVAL (the reference's InvalidGeneratorsLength)"""
    for (n_in, n_out), (mult, pn) in {(12, 12): (960, 1024), (1, 16): (1192, 2048), (16, 16): (1284, 2048),
                                      (32, 32): (2580, 4096), (64, 64): (5172, 8192)}.items():
        rc, info = _plan_rc(ctx, n_in, n_out, pn)
        assert rc == 0, (n_in, n_out)
        assert info[0] == mult and info[1] == pn, (n_in, n_out, info)
        assert _plan_rc(ctx, n_in, n_out, pn - 1) == (EINVAL, None), (n_in, n_out)


@pytest.mark.parametrize("shape", [(16, 16), (1, 16)])
def test_homogeneous_batches_equal_oracle_and_host(ctx, gens, oracle, shape):
    """96 statements, ~6 % corrupted at drawn positions: the device head (both transcript forms, groups of 16 and
    statements alone) gives the oracle's bits and those of the host-prepared zkgpu_cloak_verify_batch; the large path ran.
    A block call (zkgpu_verifier) with one more proof of the wrong length rejects that one alone."""
    from zkvm_amd.verifier import CloakTx, Verifier
    n_in, n_out = shape
    rng = random.Random(n_in * 100 + n_out)
    txs = _cloak(oracle, 96, n_in, n_out, b"large %d %d" % shape)
    bad = _corrupt(txs, rng, 6)
    r = hashlib.shake_256(b"large r %d %d" % shape).digest(64 * len(txs))
    want = _want(oracle, txs, r)
    assert [i for i, w in enumerate(want) if not w] == sorted(bad)
    v = Verifier(ctx, gens, host_threads=0)
    assert bits(v.verify_bitmap(txs, r), len(txs)) == want
    plen = len(txs[0].proof)
    com, proofs = b"".join(t.commitments for t in txs), b"".join(t.proof for t in txs)
    try:
        for mode in (2, 1):
            ctx.set_transcript_mode(mode)
            for group in (16, 1):
                ctx.set_group_size(group)
                got, prof = _profiled(ctx, lambda: v.verify_packed_gpu(n_in, n_out, len(txs), com, proofs, plen, r))
                assert bits(got, len(txs)) == want, (mode, group)
                assert all(prof.get(k) == 1 for k in LARGE_KERNELS) and "k_prepare" not in prof, prof
    finally:
        ctx.set_transcript_mode(0)
        ctx.set_group_size(16)
    short = next(i for i in range(len(txs)) if i not in bad)
    txs[short] = CloakTx(n_in, n_out, txs[short].commitments, txs[short].proof[:-32])          # wrong length
    want = _want(oracle, txs, r)
    assert [i for i, w in enumerate(want) if not w] == sorted(bad + [short])
    assert bits(v.verify_bitmap_gpu(txs, r), len(txs)) == want                 # zkgpu_verifier (block)
    assert bits(v.verify_bitmap(txs, r), len(txs)) == want
    v.close()


def test_synchronous_path_and_64x64(ctx, oracle):
    """generators without tables take the synchronous device path: a 16x16 batch and 64x64 statements (the documented
    maximum, 8192 generators) -- valid gives 1, corrupted 0, as the oracle says.  800 64x64 statements (a valid and a
    corrupted one, repeated) need more than one slice of the 512 MiB workspace: prepared in two rounds, the same bits"""
    from zkvm_amd.verifier import BulletproofGens, Verifier
    g = BulletproofGens(ctx, 8192, table_bits=0)
    v = Verifier(ctx, g)
    try:
        for shape, count in (((16, 16), 6), ((64, 64), 2)):
            txs = _cloak(oracle, count, *shape, b"sync %d %d" % shape)
            _corrupt(txs, random.Random(count), 1)
            r = hashlib.shake_256(b"sync r").digest(64 * count)
            want = _want(oracle, txs, r)
            assert want.count(0) == 1
            com, proofs = b"".join(t.commitments for t in txs), b"".join(t.proof for t in txs)
            got, prof = _profiled(ctx, lambda: v.verify_packed_gpu(shape[0], shape[1], count, com, proofs, len(txs[0].proof), r))
            assert bits(got, count) == want, shape
            assert prof.get("k_lp_gens") == 1 and "k_prepare" not in prof
        n = 800
        com = b"".join(txs[i % 2].commitments for i in range(n))
        proofs = b"".join(txs[i % 2].proof for i in range(n))
        r = hashlib.shake_256(b"sync r 800").digest(64 * n)
        got, prof = _profiled(ctx, lambda: v.verify_packed_gpu(64, 64, n, com, proofs, len(txs[0].proof), r))
        assert bits(got, n) == [want[i % 2] for i in range(n)]
        assert prof.get("k_lp_head") == 2 and prof.get("k_lp_tail") == 2
    finally:
        v.close()
        g.close()


def _cprime(ch, n2, pn, rho=1):
    cp = rho * pow(ch[n2], pn - 1, L) % L
    for u in ch[n2 + 5:]:
        cp = cp * u * u % L
    return cp


def _check_scalars(ctx, lay, batch, i, want_st, want_dy, cp):
    st = ctx.debug_read("static_scalars", batch * lay["n_static"] * 32)
    dy = ctx.debug_read("dyn_scalars", batch * lay["n_dyn"] * 32)
    for got, wantb, cnt in ((st, want_st, lay["n_static"]), (dy, want_dy, lay["n_dyn"])):
        assert len(wantb) == 32 * cnt
        for j in range(cnt):
            g = int.from_bytes(got[(i * cnt + j) * 32: (i * cnt + j + 1) * 32], "little")
            assert g == int.from_bytes(wantb[32 * j: 32 * j + 32], "little") * cp % L, (i, j)


def test_large_path_scalars_equal_oracle_times_cprime(ctx, gens, oracle):
    """zkgpu_debug_read after a batch: every static and dynamic scalar of a 16x16 cloak (alone and in groups, rho = r^2) and
    of a two-phase shuffle past the limit is the oracle's times c' = rho y^(pn-1) prod u_j^2"""
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import R1csVerifier, Verifier
    txs = _cloak(oracle, 3, 16, 16, b"scalars")
    r = hashlib.shake_256(b"scalars r").digest(64 * 3)
    v = Verifier(ctx, gens)
    lay = v.plan_layout(16, 16)
    com, proofs = b"".join(t.commitments for t in txs), b"".join(t.proof for t in txs)
    try:
        for group in (1, 16):
            ctx.set_group_size(group)
            assert bits(v.verify_packed_gpu(16, 16, 3, com, proofs, len(txs[0].proof), r), 3) == [1, 1, 1]
            for i, t in enumerate(txs):
                ds, _, ss, pn = oracle.cloak_verify_prepare(t.commitments, 16, 16, t.proof, r[64 * i: 64 * i + 64])
                ch = oracle.cloak_verify_challenges(t.commitments, 16, 16, t.proof, r[64 * i: 64 * i + 64])
                rr = int.from_bytes(r[64 * i: 64 * i + 64], "little") % L
                _check_scalars(ctx, lay, 3, i, ss, ds, _cprime(ch, lay["n_chal2"], pn, rr * rr % L if group > 1 else 1))
    finally:
        ctx.set_group_size(16)
    # a shuffle of 400 pairs: 798 multipliers, 800 commitments, one second-phase challenge
    k = 400
    rv = R1csVerifier(ctx, gens, R1csDescription(GADGET_LABEL, *describe_shuffle(k)))
    info = rv.info()
    rng = random.Random(5)
    coms, prs = [], []
    for i in range(2):
        xs = [rng.randrange(L) for _ in range(k)]
        rc, c_, p_ = oracle.gadget_prove(2, k, xs + sorted(xs), hashlib.sha256(b"shuffle %d" % i).digest())
        assert rc == 0 and len(p_) == info["proof_len"]
        coms.append(c_); prs.append(p_)
    r = hashlib.shake_256(b"shuffle r").digest(128)
    got, prof = _profiled(ctx, lambda: rv.verify_gpu(2, b"".join(coms), b"".join(prs), info["proof_len"], r))
    assert bits(got, 2) == [1, 1] and prof.get("k_lp_head") == 1
    for i in range(2):
        ds, _, ss, pn, ch = oracle.gadget_verify_prepare(2, k, coms[i], prs[i], r[64 * i: 64 * i + 64])
        assert pn == info["padded_n"]
        _check_scalars(ctx, info, 2, i, ss, ds, _cprime(ch, info["n_chal2"], pn))
    rv.close()


def _ranges(ctx, gens, oracle, count, n_stmt, tag):
    """describe_ranges(count) (64-bit ranges, one phase), its R1csVerifier and oracle proofs -> (verifier, coms, proofs)"""
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import R1csVerifier
    rv = R1csVerifier(ctx, gens, R1csDescription(GADGET_LABEL, *describe_ranges(count)))
    rng = random.Random(count)
    coms, prs = [], []
    for i in range(n_stmt):
        rc, c_, p_ = oracle.gadget_prove(3, count, [rng.randrange(1 << 64) for _ in range(count)], hashlib.sha256(tag + b"%d" % i).digest())
        assert rc == 0
        coms.append(c_); prs.append(p_)
    return rv, coms, prs


def test_described_ranges_past_the_limit(ctx, gens, oracle):
    """20 64-bit ranges (1280 multipliers, padded n 2048) in both wire forms: the oracle's bits and the host-prepared
    zkgpu_r1cs_verify_batch's, through the large path"""
    rv, coms, prs = _ranges(ctx, gens, oracle, 20, 12, b"ranges")
    info = rv.info()
    prs = [bytearray(p) for p in prs]
    prs[3][1 + 32 * 9 + 2] ^= 8                                       # T_5
    coms[7] = coms[8]
    r = hashlib.shake_256(b"ranges r").digest(64 * len(prs))
    want = [int(oracle.gadget_verify(3, 20, coms[i], bytes(prs[i]), r[64 * i: 64 * i + 64])) for i in range(len(prs))]
    assert [i for i, w in enumerate(want) if not w] == [3, 7]
    for form in ("one", "two"):
        if form == "two":                                           # the oracle's encoding: A_I2 A_O2 S2 = identity, version 1
            pb = [bytes(p) for p in prs]
            assert pb[0][0] == 1 and pb[0][1 + 96: 1 + 192] == bytes(96) and len(pb[0]) == 1 + 32 * (16 + 2 * 11)
        else:                                                       # the same proofs without the three points, version 0
            pb = [b"\x00" + bytes(p[1: 1 + 96]) + bytes(p[1 + 192:]) for p in prs]
        plen = len(pb[0])
        com_b, proof_b = b"".join(coms), b"".join(pb)
        got, prof = _profiled(ctx, lambda: rv.verify_gpu(len(pb), com_b, proof_b, plen, r))
        assert bits(got, len(pb)) == want, form
        assert prof.get("k_lp_tail") == 1 and "k_prepare" not in prof
        assert bits(rv.verify_host_prepared(len(pb), com_b, proof_b, plen, r, host_threads=0), len(pb)) == want, form
    assert info["padded_n"] == 2048
    rv.close()


def test_mixed_call_with_large_and_small_plans(ctx, gens, oracle):
    """a shuffled mixed call over three small plans and two large ones: per-plan calls' and the oracle's bits; the large
    path's launches do not depend on how many large plans the call holds, and a call without one makes none"""
    from zkvm_amd.verifier import MixedR1csVerifier
    small_rv, s_coms, s_prs = _ranges(ctx, gens, oracle, 2, 16, b"small ranges")
    big_rv, b_coms, b_prs = _ranges(ctx, gens, oracle, 20, 8, b"big ranges")
    fix, _, _, _ = load_cloak_fixture()
    c16 = _cloak(oracle, 10, 16, 16, b"mixed 16")
    c32 = _cloak(oracle, 10, 3, 2, b"mixed 3x2")
    plans = [small_rv, (2, 2), (3, 2), (16, 16), big_rv]
    stmts = [(0, s_coms[i], s_prs[i], ("gadget", 3, 2)) for i in range(16)] \
        + [(1, c, p, ("cloak", 2, 2)) for c, p in fix[:40]] \
        + [(2, t.commitments, t.proof, ("cloak", 3, 2)) for t in c32] \
        + [(3, t.commitments, t.proof, ("cloak", 16, 16)) for t in c16] \
        + [(4, b_coms[i], b_prs[i], ("gadget", 3, 20)) for i in range(8)]
    rng = random.Random(9)
    rng.shuffle(stmts)
    n = len(stmts)
    proofs = [bytearray(s[2]) for s in stmts]
    bad = rng.sample(range(n), 6)
    for i in bad:
        proofs[i][1 + 32 * 7 + 1] ^= 4                                  # T_3 (either wire form)
    proofs = [bytes(p) for p in proofs]
    idx, coms = [s[0] for s in stmts], [s[1] for s in stmts]
    r = hashlib.shake_256(b"mixed large r").digest(64 * n)
    mv = MixedR1csVerifier(ctx, gens, plans)
    try:
        got, prof = _profiled(ctx, lambda: mv.verify(idx, coms, proofs, r))
        got = bits(got, n)
        for i, s in enumerate(stmts):
            kind, a, b = s[3]
            o = oracle.gadget_verify(a, b, coms[i], proofs[i], r[64 * i: 64 * i + 64]) if kind == "gadget" else \
                oracle.cloak_verify(coms[i], a, b, proofs[i], r[64 * i: 64 * i + 64])
            assert got[i] == int(o), i
        assert sorted(i for i in range(n) if not got[i]) == sorted(bad)
        # per-plan calls on the same statements and randomness
        for p, h in enumerate(mv.handles):
            members = [i for i in range(n) if idx[i] == p]
            for plen in {len(proofs[i]) for i in members}:
                mm = [i for i in members if len(proofs[i]) == plen]
                bm = C.create_string_buffer((len(mm) + 7) // 8)
                rc = ctx.lib.zkgpu_r1cs_verify_batch_gpu(ctx.h, gens.points.h, C.c_void_p(h), len(mm), b"".join(coms[i] for i in mm),
                                                         b"".join(proofs[i] for i in mm), plen, b"".join(r[64 * i: 64 * i + 64] for i in mm), bm)
                assert rc == 0 and bits(bm.raw, len(mm)) == [got[i] for i in mm], p
        assert all(prof.get(k) == 1 for k in LARGE_KERNELS), prof
        # one large plan instead of two: the same launches; no large plan: none of them, k_mx_prepare as before
        one = [i for i in range(n) if idx[i] != 4]
        _, prof1 = _profiled(ctx, lambda: mv.verify([idx[i] for i in one], [coms[i] for i in one], [proofs[i] for i in one],
                                                     b"".join(r[64 * i: 64 * i + 64] for i in one)))
        assert {k: prof1.get(k) for k in LARGE_KERNELS + ("k_mx_prepare",)} == {k: prof.get(k) for k in LARGE_KERNELS + ("k_mx_prepare",)}
        none = [i for i in range(n) if idx[i] < 3]
        got0, prof0 = _profiled(ctx, lambda: mv.verify([idx[i] for i in none], [coms[i] for i in none], [proofs[i] for i in none],
                                                       b"".join(r[64 * i: 64 * i + 64] for i in none)))
        assert bits(got0, len(none)) == [got[i] for i in none]
        assert not any(k in prof0 for k in LARGE_KERNELS) and prof0["k_mx_prepare"] == 1
    finally:
        mv.close()
        small_rv.close()
        big_rv.close()


def test_verifier_accepts_valid_large_payouts(ctx, gens, oracle):
    """zkgpu_verifier over 2048 generators: a block mixing 2x2 and 1x16 transactions and 1x16 tickets give valid 1x16
    transactions bit 1 (the plan used to be refused and every one of them rejected) and corrupted ones bit 0, as the oracle"""
    from zkvm_amd.verifier import BlockVerifier, CloakTx
    fix, _, _, _ = load_cloak_fixture()
    big = _cloak(oracle, 24, 1, 16, b"payout")
    bad = _corrupt(big, random.Random(3), 3)
    txs = [CloakTx(2, 2, c, p) for c, p in fix[:24]] + big
    random.Random(4).shuffle(txs)
    r = hashlib.shake_256(b"payout r").digest(64 * len(txs))
    want = _want(oracle, txs, r)
    assert want.count(0) == len(bad)
    bv = BlockVerifier(ctx, gens)
    try:
        assert bits(bv.verify(txs, r), len(txs)) == want
        rb = hashlib.shake_256(b"payout ticket r").digest(64 * len(big))
        t = bv.submit(1, 16, len(big), b"".join(x.commitments for x in big), b"".join(x.proof for x in big), len(big[0].proof), rb)
        assert bits(bv.wait(t), len(big)) == _want(oracle, big, rb)
    finally:
        bv.close()


def test_forced_large_path_equals_k_prepare(ctx, gens, oracle, monkeypatch):
    """ZKGPU_TEST_LARGE_PREP=1 at plan creation: the 2x2 and 4x4 cloaks, the 1032-constraint program and a two-phase
    shuffle prepared by large_prep.hpp write the very bytes k_prepare writes, and give the same bits"""
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import R1csVerifier, Verifier
    fix, _, _, plen = load_cloak_fixture()
    com22, pr22 = b"".join(c for c, _ in fix[:40]), [bytearray(p) for _, p in fix[:40]]
    pr22[5][1 + 32 * 12] ^= 1
    pr22 = b"".join(bytes(p) for p in pr22)
    t44 = _cloak(oracle, 6, 4, 4, b"forced 4x4")
    rng = random.Random(8)
    shuf = []
    for i in range(4):
        xs = [rng.randrange(L) for _ in range(6)]
        rc, c_, p_ = oracle.gadget_prove(2, 6, xs + sorted(xs), hashlib.sha256(b"forced sh %d" % i).digest())
        shuf.append((c_, p_))
    rv8, r_coms, r_prs = _ranges(ctx, gens, oracle, 8, 4, b"forced ranges")
    rv8.close()

    def run(forced):
        if forced:
            monkeypatch.setenv("ZKGPU_TEST_LARGE_PREP", "1")
        else:
            monkeypatch.delenv("ZKGPU_TEST_LARGE_PREP", raising=False)
        out = []
        v = Verifier(ctx, gens)
        for group in (16, 1):
            ctx.set_group_size(group)
            for (n_in, n_out), com, pr, pl, b in (((2, 2), com22, pr22, plen, 40),
                                                  ((4, 4), b"".join(t.commitments for t in t44), b"".join(t.proof for t in t44), len(t44[0].proof), 6)):
                lay = v.plan_layout(n_in, n_out)
                got, prof = _profiled(ctx, lambda: v.verify_packed_gpu(n_in, n_out, b, com, pr, pl, r_all[: 64 * b]))
                out.append((got, ctx.debug_read("static_scalars", b * lay["n_static"] * 32),
                            ctx.debug_read("dyn_scalars", b * lay["n_dyn"] * 32)))
                assert ("k_lp_head" in prof) == forced and ("k_prepare" in prof) != forced
        ctx.set_group_size(16)
        for kind, desc, items in ((2, describe_shuffle(6), shuf), (3, describe_ranges(8), list(zip(r_coms, r_prs)))):
            rv = R1csVerifier(ctx, gens, R1csDescription(GADGET_LABEL, *desc))
            info = rv.info()
            b = len(items)
            got = rv.verify_gpu(b, b"".join(c for c, _ in items), b"".join(p for _, p in items), len(items[0][1]), r_all[: 64 * b])
            out.append((got, ctx.debug_read("static_scalars", b * info["n_static"] * 32),
                        ctx.debug_read("dyn_scalars", b * info["n_dyn"] * 32)))
            rv.close()
        v.close()
        return out

    r_all = hashlib.shake_256(b"forced r").digest(64 * 40)
    try:
        base, forced = run(False), run(True)
    finally:
        ctx.set_group_size(16)
    assert bits(base[0][0], 40).count(0) == 1
    for a, b in zip(base, forced):
        assert a == b


def _wide(n_cons):
    """one committed value v and 8 multipliers, each (v, 1, v): n_cons - 2 copies of a_L0 - V_0 = 0, then a_R0 - 1 = 0 and
    a_O0 - V_0 = 0 -- a small statement (padded n 8) with as many constraints as asked"""
    K_COMMITTED, K_LEFT, K_RIGHT, K_OUT, K_ONE = range(5)
    cons = [[(K_LEFT, 0, 1, -1, 0), (K_COMMITTED, 0, -1, -1, 0)]] * (n_cons - 2)
    cons += [[(K_RIGHT, 0, 1, -1, 0), (K_ONE, 0, -1, -1, 0)], [(K_OUT, 0, 1, -1, 0), (K_COMMITTED, 0, -1, -1, 0)]]
    return 1, 8, 8, [], cons


def test_constraint_count_bound(ctx, gens, oracle):
    """65536 constraints (the z power tables' reach) verify on the device as on the host-prepared path; 65537 are refused
    at plan creation with ZKGPU_EINVAL"""
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import R1csProver, R1csVerifier
    over = R1csDescription(GADGET_LABEL, *_wide(65537))
    h = C.c_void_p()
    assert ctx.lib.zkgpu_r1cs_plan_create(ctx.h, C.byref(over.struct), 2048, C.byref(h)) == EINVAL
    desc = R1csDescription(GADGET_LABEL, *_wide(65536))
    rv = R1csVerifier(ctx, gens, desc)
    assert rv.info()["constraints"] == 65536
    vals = [[5 + i] for i in range(4)]
    givens = [[(5 + i, 1)] * 8 for i in range(4)]
    seeds = [hashlib.sha256(b"wide %d" % i).digest() for i in range(4)]
    coms, proofs = R1csProver(ctx, gens, desc, [0xFFFFFFFF] * 16, host_threads=8).prove(vals, givens, seeds)
    proofs = [bytearray(p) for p in proofs]
    proofs[2][1 + 32 * 9 + 3] ^= 2
    proofs = [bytes(p) for p in proofs]
    plen = len(proofs[0])
    r = hashlib.shake_256(b"wide r").digest(64 * 4)
    com_b, proof_b = b"".join(coms), b"".join(proofs)
    got, prof = _profiled(ctx, lambda: rv.verify_gpu(4, com_b, proof_b, plen, r))
    assert bits(got, 4) == [1, 1, 0, 1] and prof.get("k_lp_head") == 1
    assert bits(rv.verify_host_prepared(4, com_b, proof_b, plen, r, host_threads=0), 4) == [1, 1, 0, 1]
    rv.close()
