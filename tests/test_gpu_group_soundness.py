"""Group checks against crafted statements whose errors cancel or line up (tests/forgery_corpus.py; its controls, on the
CPU, are tests/test_forgery_corpus.py).  Every bitmap is held against the oracle's per-statement verdicts with the same r,
every counter against the integers the corpus' model gives:

    homogeneous cloak call   every C, A and R case under group sizes 1, 2, 3, 16, 64 x locate modes 1, 2, 3 x Horner modes
                             0, 1, 2 x tail modes 0, 1; zkgpu_debug_force_regroup's counter before and after each call --
                             an A case that names an innocent statement, or a bad one that is not alone, is the first input
                             that raises status[0] bit 2 and takes the ungrouped re-run by DATA -- and rho (slot 13 of the
                             "challenges" buffer) of every statement: r^2, 1 where r reduces to 0
    independent-r paths      submit + wait, device pointers with r drawn on the device, scalars prepared on the host
    tickets                  the halves of a pair in two tickets merged into one device batch, r given and drawn
    described systems        R1csVerifier.verify_gpu and MixedR1csVerifier.verify with zkgpu_debug_read "mixed_groups"
"""
import hashlib

import pytest

import forgery_corpus as F
from gpu_util import GADGET_LABEL, L, bits, describe_range, load_cloak_fixture

pytestmark = pytest.mark.gpu
R260 = pow(2, 260, L)
CLOAK = F.cloak_cases()
CLOAK_C = [c for c in CLOAK if c.family == "C"]
_WANT = {}


def bitmap(accept) -> bytes:
    bm = bytearray((len(accept) + 7) // 8)
    for i, b in enumerate(accept):
        bm[i // 8] |= (1 if b else 0) << (i % 8)
    return bytes(bm)


def packed(case):
    return b"".join(c for c, _ in case.members), b"".join(p for _, p in case.members), len(case.members[0][1])


def want_of(oracle, case, r=None):
    """the oracle's accept bytes for the case's statements, each alone, with the case's r (computed once) or the r given"""
    key = None if r is not None else case.name + case.system
    if key is None or key not in _WANT:
        com, proofs, plen = packed(case)
        rr = r if r is not None else case.r
        if case.system == "cloak":
            acc = list(oracle.cloak_verify_batch(com, 2, 2, proofs, plen, rr, threads=16))
        else:
            acc = [int(oracle.gadget_verify(1, 8, c, p, rr[64 * i: 64 * i + 64])) for i, (c, p) in enumerate(case.members)]
        if key is None:
            return acc
        assert acc == case.expected(), case
        _WANT[key] = acc
    return _WANT[key]


def draw(seed: bytes, p: int) -> bytes:
    return hashlib.shake_256(seed + p.to_bytes(8, "little")).digest(64)


def mont(x: int) -> int:
    return x % L * R260 % L


def slot(ch: bytes, slots: int, i: int, j: int) -> int:
    return int.from_bytes(ch[(i * slots + j) * 32: (i * slots + j) * 32 + 32], "little")


@pytest.fixture(scope="module")
def ctx():
    from zkvm_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gens(ctx):
    from zkvm_amd.verifier import BulletproofGens
    g = BulletproofGens(ctx, 256, table_bits=8)
    yield g
    g.close()


@pytest.fixture(scope="module")
def verifier(ctx, gens):
    from zkvm_amd.verifier import Verifier
    v = Verifier(ctx, gens)
    yield v
    v.close()


@pytest.fixture(scope="module")
def clean(oracle):
    """21 valid statements no case uses, with their own r -> (commitments, proofs, proof length, r, bitmap)"""
    fix, _, _, plen = load_cloak_fixture()
    com, proofs = b"".join(c for c, _ in fix[100:121]), b"".join(p for _, p in fix[100:121])
    r = hashlib.shake_256(b"forgery clean batch").digest(64 * 21)
    acc = list(oracle.cloak_verify_batch(com, 2, 2, proofs, plen, r, threads=16))
    assert acc == [1] * 21
    return com, proofs, plen, r, bitmap(acc)


def _reset(ctx):
    ctx.set_group_size(16); ctx.set_locate_mode(0); ctx.set_horner_mode(0); ctx.set_tail_mode(0)
    ctx.force_regroup(False)


@pytest.mark.parametrize("case", CLOAK, ids=lambda c: c.name)
def test_homogeneous_cloak_call(ctx, verifier, oracle, clean, case):
    com, proofs, plen = packed(case)
    want = bitmap(want_of(oracle, case))
    slots = verifier.plan_layout(2, 2)["slots"]
    rs = [int.from_bytes(case.chunk(i), "little") % L for i in range(case.n)]
    seen = {}
    try:
        for gs in F.GROUP_SIZES:
            reruns = F.reruns(oracle, case, gs)
            if gs == case.group:
                assert reruns == (1 if case.family == "A" and case.hit is not None else 0)
            ctx.set_group_size(gs)
            for tail in (0, 1):
                ctx.set_tail_mode(tail)
                for horner in (0, 1, 2):
                    ctx.set_horner_mode(horner)
                    for locate in (1, 2, 3):
                        ctx.set_locate_mode(locate)
                        before = ctx.force_regroup(False)
                        got = verifier.verify_packed_gpu(2, 2, case.n, com, proofs, plen, case.r)
                        after = ctx.force_regroup(False)
                        where = (gs, tail, horner, locate)
                        assert got == want, where
                        assert after - before == (reruns if locate != 1 else 0), where
                        seen[after - before] = seen.get(after - before, 0) + 1
                        if locate == 1 and tail == 0 and horner == 0:
                            # the weights the call used: rho = r^2 inside a group (1 where r = 0), 1 for a statement alone
                            ch = ctx.debug_read("challenges", case.n * slots * 32)
                            assert len(ch) == case.n * slots * 32
                            assert [slot(ch, slots, i, 7) for i in range(case.n)] == [mont(r) for r in rs], where
                            rho = [mont((r * r % L or 1) if gs > 1 else 1) for r in rs]
                            assert [slot(ch, slots, i, 13) for i in range(case.n)] == rho, where
                        if after != before:                  # the batch after an ungrouped re-run
                            assert verifier.verify_packed_gpu(2, 2, 21, clean[0], clean[1], clean[2], clean[3]) == clean[4], where
                            assert ctx.force_regroup(False) == after
            assert verifier.verify_packed_gpu(2, 2, 21, clean[0], clean[1], clean[2], clean[3]) == clean[4], gs
    finally:
        _reset(ctx)
    print("regroup counter deltas (delta: calls) %s: %s" % (case.name, sorted(seen.items())))


@pytest.mark.parametrize("case", CLOAK_C, ids=lambda c: c.name)
def test_independent_r_paths(ctx, gens, verifier, oracle, case):
    from zkvm_amd.verifier import CloakTx
    com, proofs, plen = packed(case)
    want = bitmap(want_of(oracle, case))
    d_com = d_proofs = None
    try:
        ctx.set_group_size(case.group)
        before = ctx.force_regroup(False)
        verifier.submit_packed_gpu(2, 2, case.n, com, proofs, plen, case.r)
        assert ctx.verify_wait() == want
        d_com, d_proofs = ctx.to_device(com), ctx.to_device(proofs)
        got = verifier.verify_packed_gpu_dev(2, 2, case.n, d_com, d_proofs, plen, None)
        seed = ctx.debug_read("r_seed", 32)
        assert len(seed) == 32 and seed != bytes(32)
        drawn = b"".join(draw(seed, i) for i in range(case.n))
        assert got == bitmap(want_of(oracle, case, drawn)) == want
        txs = [CloakTx(2, 2, c, p) for c, p in case.members]
        assert verifier.verify_bitmap(txs, case.r) == want
        assert ctx.force_regroup(False) == before
    finally:
        for d in (d_com, d_proofs):
            if d is not None:
                ctx.free_device(d)
        _reset(ctx)


@pytest.mark.parametrize("how", ["submit, r given", "submit_dev, r given", "submit_dev, r drawn"])
def test_halves_in_two_tickets_of_one_device_batch(ctx, gens, verifier, oracle, how):
    """two tickets of 8 at a merge target of 16: the +d half is statement 3 of the first, the -d half statement 4 of the
    second, so they are positions 4 and 13 of one group of 16 -- shown by slot 7 of the lane's 16-statement batch"""
    from zkvm_amd import ZkGpuError
    from zkvm_amd.verifier import BlockVerifier
    fix, _, _, plen = load_cloak_fixture()
    each = 8
    members = [list(fix[130: 130 + each]), list(fix[140: 140 + each])]
    members[0][3] = (fix[0][0], F.moved(fix[0][1], "a", 1))
    members[1][4] = (fix[0][0], F.moved(fix[0][1], "a", -1))
    coms = [b"".join(c for c, _ in m) for m in members]
    proofs = [b"".join(p for _, p in m) for m in members]
    r = hashlib.shake_256(b"forgery tickets").digest(64 * 2 * each)
    given = how.endswith("given")
    slots = verifier.plan_layout(2, 2)["slots"]
    bv = BlockVerifier(ctx, gens, batches_in_flight=2)
    dev = []
    try:
        bv.set_merge(2 * each)
        before = sum(bv.lane(i).force_regroup(False) for i in range(bv.lanes()))
        if how.startswith("submit_dev"):
            dev = [ctx.to_device(x) for x in coms + proofs + ([r[:64 * each], r[64 * each:]] if given else [])]
            ts = [bv.submit_dev(2, 2, each, dev[k], dev[2 + k], plen, dev[4 + k] if given else None) for k in range(2)]
        else:
            ts = [bv.submit(2, 2, each, coms[k], proofs[k], plen, r[64 * each * k: 64 * each * (k + 1)]) for k in range(2)]
        got = [bv.wait(t) for t in ts]
        if not given:
            found = [(c, c.debug_read("r_seed", 32)) for c in (bv.lane(i) for i in range(bv.lanes()))]
            found = [(c, s) for c, s in found if s != bytes(32)]
            assert len(found) == 1
            r = b"".join(draw(found[0][1], i) for i in range(2 * each))
        merged = 0
        for i in range(bv.lanes()):                       # one lane ran ONE batch of 16 with these r: the tickets were merged
            try:
                ch = bv.lane(i).debug_read("challenges", 2 * each * slots * 32)
            except ZkGpuError:                            # a lane that has run nothing yet
                continue
            if len(ch) == 2 * each * slots * 32:
                rr = [int.from_bytes(r[64 * k: 64 * k + 64], "little") % L for k in range(2 * each)]
                merged += [slot(ch, slots, k, 7) for k in range(2 * each)] == [mont(x) for x in rr] and \
                    [slot(ch, slots, k, 13) for k in range(2 * each)] == [mont(x * x % L or 1) for x in rr]
        assert merged == 1
        for k in range(2):
            acc = list(oracle.cloak_verify_batch(coms[k], 2, 2, proofs[k], plen, r[64 * each * k: 64 * each * (k + 1)], threads=8))
            assert acc == [0 if i == (3, 4)[k] else 1 for i in range(each)]
            assert got[k] == bitmap(acc), k
        assert sum(bv.lane(i).force_regroup(False) for i in range(bv.lanes())) == before
    finally:
        bv.close()
        for d in dev:
            ctx.free_device(d)


# ---- described systems and mixed calls -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def described(ctx, gens, oracle):
    """two plans of ONE description (range(8): the same generator key) and the cloak 2x2 ->
    (R1csVerifier, MixedR1csVerifier over [range(8), range(8) again, cloak 2x2], {name: case})"""
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import MixedR1csVerifier, R1csVerifier
    m, n1, n, labels, cons = describe_range(8)
    rv = [R1csVerifier(ctx, gens, R1csDescription(GADGET_LABEL, m, n1, n, labels, cons)) for _ in range(2)]
    mv = MixedR1csVerifier(ctx, gens, rv + [(2, 2)])
    cases = {c.name: c for c in F.corpus(oracle) if c.system == "range8"}
    assert len(cases) == 3
    yield rv[0], mv, cases
    mv.close()
    for v in rv:
        v.close()


RANGE8_CASES = ("C pair a, batch 2", "C pair a, check of 16", "C pair a, malformed third")


@pytest.mark.parametrize("name", RANGE8_CASES)
def test_described_system_call(ctx, oracle, described, name):
    rv, _, cases = described
    case = cases[name]
    com, proofs, plen = packed(case)
    want = bitmap(want_of(oracle, case))
    try:
        for gs in (1, 2, 16):
            ctx.set_group_size(gs)
            for locate in (1, 2):
                ctx.set_locate_mode(locate)
                before = ctx.force_regroup(False)
                assert rv.verify_gpu(case.n, com, proofs, plen, case.r) == want, (gs, locate)
                assert F.reruns(oracle, case, gs) == 0 and ctx.force_regroup(False) == before, (gs, locate)
    finally:
        _reset(ctx)


def _checks(idx, key, gs):
    """the mixed call's checks of two or more (test_gpu_r1cs_mixed_groups.py's rule): statements ordered by (plan by first
    appearance, position), cut per generator key into runs of gs"""
    if gs <= 1:
        return []
    first, by_key = {}, {}
    for p in idx:
        first.setdefault(p, len(first))
    for i in sorted(range(len(idx)), key=lambda i: (first[idx[i]], i)):
        by_key.setdefault(key[idx[i]], []).append(i)
    return [mem[k: k + gs] for mem in by_key.values() for k in range(0, len(mem), gs) if len(mem[k: k + gs]) >= 2]


def _mixed(ctx, oracle, mv, idx, members, r, forged, left_out):
    """one call per group size: the oracle's bits; checks formed, statements in them, checks that hold a forged statement,
    and the members of those checks (the left-out ones aside) re-checked"""
    n = len(idx)
    acc = []
    for i, (c, p) in enumerate(members):
        ri = r[64 * i: 64 * i + 64]
        acc.append(int(oracle.cloak_verify(c, 2, 2, p, ri) if idx[i] == 2 else oracle.gadget_verify(1, 8, c, p, ri)))
    assert acc == [0 if i in forged | left_out else 1 for i in range(n)]
    try:
        for gs in (16, 2, 3, 1):
            ctx.set_group_size(gs)
            checks = _checks(idx, {0: 8, 1: 8, 2: 256}, gs)
            failed = [g for g in checks if forged & set(g)]
            got = mv.verify(idx, [c for c, _ in members], [p for _, p in members], r)
            assert got == bitmap(acc), gs
            assert ctx.mixed_group_stats() == (len(checks), sum(len(g) for g in checks), len(failed), sum(len(set(g) - left_out) for g in failed)), gs
    finally:
        ctx.set_group_size(16)


@pytest.mark.parametrize("name", RANGE8_CASES)
def test_mixed_call_one_plan(ctx, oracle, described, name):
    _, mv, cases = described
    case = cases[name]
    _mixed(ctx, oracle, mv, [0] * case.n, case.members, case.r, set(case.forged), set(case.left_out))


def test_mixed_call_halves_under_two_plans_of_one_key(ctx, oracle, described):
    """the +d half under plan 0 and the -d half under plan 1 (the same description: one generator key, one check), two
    clean statements under each, and beside them a cloak pair with two clean cloaks under the third plan"""
    _, mv, cases = described
    pool = F.range8_statements(oracle, 20)
    fix, _, _, _ = load_cloak_fixture()
    members = [(pool[0][0], F.moved(pool[0][1], "b", 1)), (pool[0][0], F.moved(pool[0][1], "b", -1)), pool[1], pool[2], pool[3], pool[4],
               fix[150], (fix[0][0], F.moved(fix[0][1], "a", 1)), fix[151], (fix[0][0], F.moved(fix[0][1], "a", -1))]
    idx = [0, 1, 0, 1, 0, 1, 2, 2, 2, 2]
    r = hashlib.shake_256(b"forgery two plans").digest(64 * len(idx))
    _mixed(ctx, oracle, mv, idx, members, r, {0, 1, 7, 9}, set())
    assert _checks(idx, {0: 8, 1: 8, 2: 256}, 16) == [[0, 2, 4, 1, 3, 5], [6, 7, 8, 9]]
