"""Group checks in zkgpu_r1cs_verify_mixed: statements whose plans have the same generator key (padded n, generator
capacity) are checked in groups of up to zkgpu_set_group_size members whatever their constraint systems; the members of a
group that fails are re-checked alone on the device.  Every bitmap equals the one of the same call with group_size = 1, of
the per-plan calls and of the oracle; zkgpu_debug_read "mixed_groups" (groups formed, statements in them, groups failed,
statements re-checked) equals what the grouping rule gives, computed here from zkgpu_cloak_plan_info's padded n.

The model of the rule (`_model_groups`): statements in the order (plan by first appearance, position in the call), cut per
padded n into runs of group_size; a run of one statement is no group.  (The library orders by LDS class before plan; no two
plans of one padded n differ in class here, so the class does not show inside a key.)"""
import ctypes as C
import hashlib
import random

import pytest

from gpu_util import GADGET_LABEL, L, bits, describe_range, describe_ranges, describe_shuffle, gadget_witness, load_cloak_fixture, random_system

pytestmark = pytest.mark.gpu

RANGE8, SHUFFLE5, SYSTEM_A, CLOAK22, RANGES8X64, RANGE64 = range(6)


@pytest.fixture(scope="module")
def ctx():
    from zkvm_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gens(ctx):
    from zkvm_amd.verifier import BulletproofGens
    g = BulletproofGens(ctx, 512, table_bits=8)
    yield g
    g.close()


def _prove(ctx, gens, desc, mult_def, vals, givens, tag):
    from zkvm_amd.verifier import R1csProver
    seeds = [hashlib.sha256(b"mixed groups %s %d" % (tag, i)).digest() for i in range(len(vals))]
    return R1csProver(ctx, gens, desc, mult_def, host_threads=8).prove(vals, givens, seeds)


def _descriptions():
    """(description tuple, label, oracle check or None, kind, param) per plan except the cloak"""
    rng = random.Random(99)
    (sa, mult_def_a, values_a, given_a) = random_system(rng, 1, 4, 3, 2)
    return {RANGE8: (describe_range(8), GADGET_LABEL, ("gadget", 1, 8)), SHUFFLE5: (describe_shuffle(5), GADGET_LABEL, ("gadget", 2, 5)),
            SYSTEM_A: (sa, b"groups system A", None, mult_def_a, values_a, given_a),
            RANGES8X64: (describe_ranges(8), GADGET_LABEL, ("gadget", 3, 8)), RANGE64: (describe_range(64), GADGET_LABEL, ("gadget", 1, 64))}


def _make_verifiers(ctx, gens):
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import R1csVerifier
    out = {}
    for p, d in _descriptions().items():
        m, n1, n, labels, cons = d[0]
        out[p] = (R1csVerifier(ctx, gens, R1csDescription(d[1], m, n1, n, labels, cons)), R1csDescription(d[1], m, n1, n, labels, cons))
    return out


@pytest.fixture(scope="module")
def suite(ctx, gens):
    """six plans -- range(8), shuffle(5) (two phases), a random system with challenges (these three: m or constraints
    differ, padded n = 8 alike), cloak 2x2, the 1032-constraint program (LDS class 1), range(64) -- and valid statements:
    -> (MixedR1csVerifier, {plan: [(commitments, proof, oracle check)]}, {plan: padded n})"""
    from zkvm_amd.verifier import MixedR1csVerifier
    rng = random.Random(4242)
    vs = _make_verifiers(ctx, gens)
    descs = _descriptions()
    pool = {}
    for p, count in ((RANGE8, 40), (SHUFFLE5, 16), (SYSTEM_A, 20), (RANGES8X64, 8), (RANGE64, 16)):
        d = descs[p]
        if p == SYSTEM_A:
            mult_def, vals, givens = d[3], [d[4]] * count, [d[5]] * count
        else:
            kind, param = d[2][1], d[2][2]
            vals, givens, mult_def = [], [], None
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
        coms, proofs = _prove(ctx, gens, vs[p][1], mult_def, vals, givens, b"p%d" % p)
        pool[p] = [(coms[i], proofs[i], d[2]) for i in range(count)]
    fix, n_in, n_out, _ = load_cloak_fixture()
    assert (n_in, n_out) == (2, 2)
    pool[CLOAK22] = [(c, p, ("cloak", 2, 2)) for c, p in fix[:64]]
    plans = [vs[RANGE8][0], vs[SHUFFLE5][0], vs[SYSTEM_A][0], (2, 2), vs[RANGES8X64][0], vs[RANGE64][0]]
    mv = MixedR1csVerifier(ctx, gens, plans)
    pn = {p: _padded_n(ctx, h) for p, h in enumerate(mv.handles)}
    assert pn[RANGE8] == pn[SHUFFLE5] == pn[SYSTEM_A] == 8 and pn[CLOAK22] == 256 and pn[RANGES8X64] == 512 and pn[RANGE64] == 64
    yield mv, pool, pn
    mv.close()
    for v, _ in vs.values():
        v.close()


def _padded_n(ctx, handle):
    vals = [C.c_uint32() for _ in range(5)]
    assert ctx.lib.zkgpu_cloak_plan_info(C.c_void_p(handle), *[C.byref(v) for v in vals]) == 0
    return vals[1].value


def _model_groups(idx, pn, gs):
    """the grouping rule (module docstring) -> the groups of two or more, as lists of positions"""
    if gs <= 1:
        return []
    first, by_key = {}, {}
    for p in idx:
        first.setdefault(p, len(first))
    for i in sorted(range(len(idx)), key=lambda i: (first[idx[i]], i)):
        by_key.setdefault(pn[idx[i]], []).append(i)         # (every plan here has the same generator capacity)
    groups = []
    for mem in by_key.values():
        groups += [mem[k: k + gs] for k in range(0, len(mem), gs) if len(mem[k: k + gs]) >= 2]
    return groups


def _formed(idx, pn, gs):
    g = _model_groups(idx, pn, gs)
    return len(g), sum(len(x) for x in g)


def _take(pool, spec, rng=None):
    """spec: [(plan, count)] -> idx, coms, proofs, checks; shuffled with rng"""
    sel = [(p,) + pool[p][i % len(pool[p])] for p, count in spec for i in range(count)]
    if rng:
        rng.shuffle(sel)
    return [s[0] for s in sel], [s[1] for s in sel], [s[2] for s in sel], [s[3] for s in sel]


def _run(ctx, mv, gs, idx, coms, proofs, r):
    ctx.set_group_size(gs)
    try:
        bm = mv.verify(idx, coms, proofs, r)
        return bits(bm, len(idx)), ctx.mixed_group_stats()
    finally:
        ctx.set_group_size(16)


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


def _flip_scalar(proof):
    """t_x_blinding off by a bit: still canonical, every point still decodes -- the equation alone fails"""
    p = bytearray(proof)
    p[1 + 32 * (12 if p[0] == 1 else 9) + 3] ^= 0x10
    return bytes(p)


def test_groups_form_across_plans(ctx, suite):
    """20 range(8) + 20 of the random system (padded n = 8 both) + 5 cloak 2x2, shuffled: 3 groups of the padded-8 key
    (16, 16, 8) whatever the plan, one group of the 5 cloaks; nothing fails; group_size = 1: no group, the same bits"""
    mv, pool, pn = suite
    idx, coms, proofs, _ = _take(pool, [(RANGE8, 20), (SYSTEM_A, 20), (CLOAK22, 5)], random.Random(1))
    n = len(idx)
    r = hashlib.shake_256(b"groups across plans").digest(64 * n)
    got, stats = _run(ctx, mv, 16, idx, coms, proofs, r)
    assert got == [1] * n
    assert _formed(idx, pn, 16) == (-(-40 // 16) + 1, 45)
    assert sorted(len(g) for g in _model_groups(idx, pn, 16)) == [5, 8, 16, 16]
    assert stats == (4, 45, 0, 0)
    got1, stats1 = _run(ctx, mv, 1, idx, coms, proofs, r)
    assert got1 == got and stats1 == (0, 0, 0, 0)


def test_smallest_shapes(ctx, suite):
    """batch 1; batch 2 of one plan and of two keys; 17 of one plan (16 + one alone); group sizes 2, 5 and 64 on a
    70-statement batch of two keys, one statement corrupted: the stats of the rule, the bits of group_size = 1"""
    mv, pool, pn = suite
    for spec, gs in (([(RANGE8, 1)], 16), ([(RANGE8, 2)], 16), ([(RANGE8, 1), (CLOAK22, 1)], 16), ([(SHUFFLE5, 17)], 16),
                     ([(RANGE8, 37), (RANGE64, 33)], 2), ([(RANGE8, 37), (RANGE64, 33)], 5), ([(RANGE8, 37), (RANGE64, 33)], 64)):
        idx, coms, proofs, _ = _take(pool, spec, random.Random(len(spec) + gs))
        n = len(idx)
        if n == 70:
            proofs[11] = _flip_scalar(proofs[11])
        r = hashlib.shake_256(b"smallest %d %d" % (n, gs)).digest(64 * n)
        got, stats = _run(ctx, mv, gs, idx, coms, proofs, r)
        want, _ = _run(ctx, mv, 1, idx, coms, proofs, r)
        assert got == want == [0 if (n == 70 and i == 11) else 1 for i in range(n)], (spec, gs)
        groups = _model_groups(idx, pn, gs)
        hit = [g for g in groups if n == 70 and 11 in g]
        assert stats == (len(groups), sum(len(g) for g in groups), len(hit), sum(len(g) for g in hit)), (spec, gs)
    assert _formed([0], {0: 8}, 16) == (0, 0) and _formed([0, 0], {0: 8}, 16) == (1, 2) and _formed([0, 1], {0: 8, 1: 256}, 16) == (0, 0)
    assert _formed([0] * 17, {0: 8}, 16) == (1, 16)


def test_verdict_parity_under_corruption(ctx, gens, oracle, suite):
    """~250 statements over a single-phase gadget, a two-phase one, a random system with challenges, cloak 2x2 and the
    1032-constraint program, ~8 % corrupted: a group with one bad statement, one with three, one whose members are all
    bad, a wrong length, a non-canonical t_x, an undecodable commitment (an RFC 9496 reject vector), a valid proof filed
    under another plan of the same key, r = 0 for a valid and for a bad statement.  The bitmap of group_size = 1, of the
    per-plan calls and of the oracle; failed groups = those with a bad member that is still inside its group (malformed and
    undecodable statements are left out before the sums), re-checked = the members of those groups that are inside."""
    from decode_corpus import corpus
    mv, pool, pn = suite
    rng = random.Random(31)
    idx, coms, proofs, chks = _take(pool, [(RANGE8, 80), (SHUFFLE5, 40), (SYSTEM_A, 43), (CLOAK22, 70), (RANGES8X64, 20)], rng)
    n = len(idx)
    r = bytearray(hashlib.shake_256(b"groups parity").digest(64 * n))
    live_bad, left_out = set(), set()
    # a valid range(8) proof filed under the random system (same key, same m, same proof length)
    i = next(k for k in range(n) if idx[k] == RANGE8)
    idx[i], chks[i] = SYSTEM_A, None
    live_bad.add(i)
    groups = _model_groups(idx, pn, 16)
    free = [g for g in groups if i not in g]
    rng.shuffle(free)
    smallest = min(free, key=len)
    free.remove(smallest)
    picked = []

    def pick(pred=lambda g: True):
        g = next(g for g in free if g not in picked and len(g) >= 4 and pred(g))
        picked.append(g)
        return g
    undecodable = pick(lambda g: idx[g[0]] == CLOAK22)
    one, three, malformed, noncanon, r_zero = pick(), pick(), pick(), pick(), pick()
    for k in [one[2]] + three[:3] + list(smallest):                        # the equation alone fails
        proofs[k] = _flip_scalar(proofs[k])
        live_bad.add(k)
    proofs[malformed[1]] = proofs[malformed[1]][:-32]                      # wrong length
    at = 1 + 32 * (11 if proofs[noncanon[1]][0] == 1 else 8)               # t_x >= l
    proofs[noncanon[1]] = proofs[noncanon[1]][:at] + (L + 5).to_bytes(32, "little") + proofs[noncanon[1]][at + 32:]
    reject = next(e for e, label, _ in corpus() if label == "nonsquare")
    coms[undecodable[1]] = reject + coms[undecodable[1]][32:]
    left_out |= {malformed[1], noncanon[1], undecodable[1]}
    r[64 * r_zero[0]: 64 * r_zero[0] + 64] = bytes(64)                     # r = 0, valid statement
    r[64 * three[0]: 64 * three[0] + 64] = bytes(64)                       # r = 0, bad statement
    others = [k for k in range(n) if k not in live_bad | left_out and not any(k in g for g in picked + [smallest])]
    for k in rng.sample(others, 20 - len(live_bad | left_out)):            # up to ~8 %
        proofs[k] = _flip_scalar(proofs[k])
        live_bad.add(k)
    r = bytes(r)
    got, stats = _run(ctx, mv, 16, idx, coms, proofs, r)
    alone, stats1 = _run(ctx, mv, 1, idx, coms, proofs, r)
    assert got == alone and stats1 == (0, 0, 0, 0)
    assert got == _per_plan(ctx, gens, mv.handles, idx, coms, proofs, r)
    for k in range(n):
        o = _oracle_bit(oracle, chks[k], coms[k], proofs[k], r[64 * k: 64 * k + 64])
        assert o is None or o == got[k], k
    assert [k for k in range(n) if not got[k]] == sorted(live_bad | left_out)
    failed = [g for g in groups if live_bad & set(g)]
    assert smallest in failed and one in failed and three in failed
    assert not any(g in failed for g in (malformed, noncanon, undecodable, r_zero))
    assert stats == (len(groups), sum(len(g) for g in groups), len(failed), sum(len(set(g) - left_out) for g in failed))


def _planner_counts(ctx, gens, handles, idx, proofs, gs):
    """what the host's planner (csrc/mixed_plan.hpp through libzkhost's zkhost_mixed_plan, the hook tests/test_mixed_plan.py
    drives) makes of this call -> (checks of two or more members, statements in them).  The plans' rows and keys are what
    zkgpu_cloak_plan_info / _layout give; LDS class and transcript form, which they do not give, order the statements inside
    a key and leave the counts alone"""
    import os
    import zkvm_amd
    host = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(zkvm_amd.__file__)), "lib", "libzkhost.so"))
    host.zkhost_mixed_plan.restype = C.c_longlong
    rows = []
    for h in handles:
        lay = (C.c_uint32 * 8)()
        assert ctx.lib.zkgpu_cloak_plan_layout(C.c_void_p(h), lay) == 0
        # id | proof_words m n_ch n_ch_ext n_seg n_dyn n_static pn h_base n_targets | lds_bytes large lp_slots
        rows += [h, (16 + 2 * lay[5]) * 8, lay[6], lay[1], lay[0], 1, lay[3], lay[4], _padded_n(ctx, h), 2 + gens.gens_capacity, 0, 0, 0, 0]
    offs = [0]
    for p in proofs:
        offs.append(offs[-1] + len(p))
    summary, uniq, err = (C.c_uint64 * 35)(), (C.c_uint32 * len(handles))(), C.create_string_buffer(128)
    size = host.zkhost_mixed_plan((C.c_uint64 * len(rows))(*rows), C.c_size_t(len(handles)), (C.c_uint32 * len(idx))(*idx),
                                  (C.c_uint64 * len(offs))(*offs), C.c_size_t(len(idx)), 1, C.c_uint32(gs), 1, C.c_size_t(256), None,
                                  C.c_size_t(0), summary, uniq, err, C.c_size_t(128))
    assert size > 0, err.value
    return summary[23], summary[20]


def test_the_call_runs_the_planner_the_cpu_tests_drive(ctx, gens, suite):
    """5 statements over 3 plans of 2 generator keys (range(8) and the random system: padded n = 8; range(64)), group_size 2:
    the counters of the call are those of zkhost_mixed_plan for the same call -- 2 checks of two, 4 statements in them, none
    failed, none re-checked -- and the bitmap is the per-plan calls'"""
    mv, pool, pn = suite
    idx, coms, proofs, _ = _take(pool, [(RANGE8, 2), (RANGE64, 2), (SYSTEM_A, 1)], random.Random(12))
    n = len(idx)
    r = hashlib.shake_256(b"groups planner").digest(64 * n)
    predicted = _planner_counts(ctx, gens, mv.handles, idx, proofs, 2)
    assert predicted == (2, 4) == _formed(idx, pn, 2)
    got, stats = _run(ctx, mv, 2, idx, coms, proofs, r)
    assert stats == predicted + (0, 0)
    assert got == _per_plan(ctx, gens, mv.handles, idx, coms, proofs, r) == [1] * n


def _profiled(ctx, fn):
    ctx.profile(True)
    ctx.profile_reset()
    try:
        out = fn()
        return out, {k: v[0] for k, v in ctx.profile_read().items()}
    finally:
        ctx.profile(False)


def test_every_route_through_the_call(ctx, gens, suite, monkeypatch):
    """the one-lane transcript, the large-plan preparation forced on small plans, submit + wait, r_bytes = NULL and a
    point set without tables (statements alone there): the bits of group_size = 1 on the default route"""
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import BulletproofGens, MixedR1csVerifier, R1csVerifier
    mv, pool, pn = suite
    idx, coms, proofs, _ = _take(pool, [(RANGE8, 40), (SHUFFLE5, 19), (SYSTEM_A, 21), (CLOAK22, 23), (RANGES8X64, 5)], random.Random(5))
    n = len(idx)
    bad = [3, 4, 50, 77]
    for k in bad:
        proofs[k] = _flip_scalar(proofs[k])
    proofs[9] = proofs[9] + b"\0"
    want = [0 if k in bad + [9] else 1 for k in range(n)]
    r = hashlib.shake_256(b"groups routes").digest(64 * n)
    alone, _ = _run(ctx, mv, 1, idx, coms, proofs, r)
    assert alone == want
    groups = _model_groups(idx, pn, 16)
    failed = [g for g in groups if set(bad) & set(g)]
    expect = (len(groups), sum(len(g) for g in groups), len(failed), sum(len(set(g) - {9}) for g in failed))
    got, prof = _profiled(ctx, lambda: mv.verify(idx, coms, proofs, r))
    assert bits(got, n) == want and ctx.mixed_group_stats() == expect
    assert prof.get("k_mx_group_scalars") == 1 and prof.get("k_mx_group_combine") == 1 and prof.get("k_recheck_fused") == 1
    ctx.set_transcript_mode(1)
    try:
        got, prof = _profiled(ctx, lambda: mv.verify(idx, coms, proofs, r))
    finally:
        ctx.set_transcript_mode(0)
    assert prof.get("k_mx_transcript") == 1 and "k_mx_transcript_coop" not in prof and prof.get("k_mx_group_combine") == 1
    assert bits(got, n) == want and ctx.mixed_group_stats() == expect
    # submit + zkgpu_verify_wait: the counters are those of the call FINISHED last
    mv.verify(idx[:1], coms[:1], proofs[:1], r[:64])
    mv.submit(idx, coms, proofs, r)
    assert ctx.mixed_group_stats() == (0, 0, 0, 0)
    assert bits(mv.wait(), n) == want and ctx.mixed_group_stats() == expect
    # r_bytes = NULL: every valid statement accepted
    vi, vc, vp, _ = _take(pool, [(RANGE8, 30), (SYSTEM_A, 9), (CLOAK22, 10)], random.Random(6))
    assert bits(mv.verify(vi, vc, vp, None), len(vi)) == [1] * len(vi)
    assert ctx.mixed_group_stats() == _formed(vi, pn, 16) + (0, 0)
    # plans made with the large-plan preparation forced on
    monkeypatch.setenv("ZKGPU_TEST_LARGE_PREP", "1")
    descs = _descriptions()
    forced = []
    for p in (RANGE8, SHUFFLE5, SYSTEM_A, RANGES8X64):
        m, n1, nm, labels, cons = descs[p][0]
        forced.append(R1csVerifier(ctx, gens, R1csDescription(descs[p][1], m, n1, nm, labels, cons)))
    lv = MixedR1csVerifier(ctx, gens, forced[:3] + [(2, 2)] + forced[3:])
    monkeypatch.delenv("ZKGPU_TEST_LARGE_PREP")
    try:
        got, prof = _profiled(ctx, lambda: lv.verify(idx, coms, proofs, r))
        assert prof.get("k_lp_head") == 1 and "k_mx_prepare" not in prof
        assert bits(got, n) == want and ctx.mixed_group_stats() == expect
    finally:
        lv.close()
        for v in forced:
            v.close()
    # a point set without tables: the synchronous route, statements alone
    plain = BulletproofGens(ctx, 512, table_bits=0)
    vs = _make_verifiers(ctx, plain)
    pv = MixedR1csVerifier(ctx, plain, [vs[RANGE8][0], vs[SHUFFLE5][0], vs[SYSTEM_A][0], (2, 2), vs[RANGES8X64][0], vs[RANGE64][0]])
    try:
        assert bits(pv.verify(idx, coms, proofs, r), n) == want and ctx.mixed_group_stats() == (0, 0, 0, 0)
    finally:
        pv.close()
        for v, _ in vs.values():
            v.close()
        plain.close()


def test_launch_sequence_depends_on_the_call_only(ctx, suite):
    """192 valid statements over 2 plans, over 6 and over 2 small plans, each right after a call with corrupted
    statements (failed groups): the same launches kernel by kernel (k_mx_prepare: once per LDS class present)"""
    mv, pool, pn = suite
    batch = 192
    r = hashlib.shake_256(b"groups launches").digest(64 * batch)
    counts = []
    for plans in ((RANGE8, RANGES8X64), tuple(range(6)), (RANGE8, CLOAK22)):
        sel = [(p,) + pool[p][(i // len(plans)) % len(pool[p])] for i, p in zip(range(batch), plans * batch)]
        idx, coms, proofs = [s[0] for s in sel], [s[1] for s in sel], [s[2] for s in sel]
        spoiled = [_flip_scalar(p) if i % 7 == 0 else p for i, p in enumerate(proofs)]
        assert bits(mv.verify(idx, coms, spoiled, r), batch) == [0 if i % 7 == 0 else 1 for i in range(batch)]
        assert ctx.mixed_group_stats()[2] > 0
        bm, prof = _profiled(ctx, lambda: mv.verify(idx, coms, proofs, r))
        assert bits(bm, batch) == [1] * batch and ctx.mixed_group_stats()[2:] == (0, 0)
        counts.append(prof)
    assert counts[0] == counts[1]
    assert counts[0]["k_mx_prepare"] == 2 and counts[2]["k_mx_prepare"] == 1
    assert {k: v for k, v in counts[2].items() if k != "k_mx_prepare"} == {k: v for k, v in counts[0].items() if k != "k_mx_prepare"}
    assert all(v == 1 for k, v in counts[0].items() if k != "k_mx_prepare"), counts[0]


def test_homogeneous_calls_are_untouched(ctx, gens, oracle, suite):
    """a homogeneous cloak batch with failures after a mixed call with failed groups, and a mixed call after it: the
    oracle's bits, and the homogeneous call launches what it launches on a fresh context in the same state (the mixed call
    neither reads nor writes what steers the homogeneous Horner arrangement)"""
    from zkvm_amd import Context
    from zkvm_amd.verifier import BulletproofGens, Verifier
    mv, pool, pn = suite
    fix, n_in, n_out, plen = load_cloak_fixture()
    n = 96
    hc = [c for c, _ in fix[100: 100 + n]]
    hp = [_flip_scalar(p) if i in (5, 40) else p for i, (_, p) in enumerate(fix[100: 100 + n])]
    hr = hashlib.shake_256(b"groups homogeneous").digest(64 * n)
    want = [int(oracle.cloak_verify(hc[i], n_in, n_out, hp[i], hr[64 * i: 64 * i + 64])) for i in range(n)]
    assert want == [0 if i in (5, 40) else 1 for i in range(n)]
    idx, coms, proofs, chks = _take(pool, [(RANGE8, 30), (CLOAK22, 30)], random.Random(8))
    proofs[7] = _flip_scalar(proofs[7])
    mr = hashlib.shake_256(b"groups mixed beside").digest(64 * len(idx))
    mwant = [0 if k == 7 else 1 for k in range(len(idx))]

    def homogeneous(c, g):
        v = Verifier(c, g)
        try:
            clean = v.verify_packed_gpu(n_in, n_out, n, b"".join(hc), b"".join(p for _, p in fix[100: 100 + n]), plen, hr)
            assert bits(clean, n) == [1] * n                 # (the state: the batch finished last had no failed group)
            return _profiled(c, lambda: v.verify_packed_gpu(n_in, n_out, n, b"".join(hc), b"".join(hp), plen, hr))
        finally:
            v.close()
    fresh = Context(0)
    fg = BulletproofGens(fresh, 512, table_bits=8)
    try:
        ref_bm, ref_prof = homogeneous(fresh, fg)
    finally:
        fg.close()
        fresh.close()
    v = Verifier(ctx, gens)
    try:
        clean = v.verify_packed_gpu(n_in, n_out, n, b"".join(hc), b"".join(p for _, p in fix[100: 100 + n]), plen, hr)
        assert bits(clean, n) == [1] * n
        assert bits(mv.verify(idx, coms, proofs, mr), len(idx)) == mwant and ctx.mixed_group_stats()[2] == 1
        bm, prof = _profiled(ctx, lambda: v.verify_packed_gpu(n_in, n_out, n, b"".join(hc), b"".join(hp), plen, hr))
    finally:
        v.close()
    assert bits(bm, n) == want == bits(ref_bm, n)
    assert prof == ref_prof
    got = bits(mv.verify(idx, coms, proofs, mr), len(idx))
    assert got == mwant
    for k in range(len(idx)):
        o = _oracle_bit(oracle, chks[k], coms[k], proofs[k], mr[64 * k: 64 * k + 64])
        assert o is None or o == got[k], k
