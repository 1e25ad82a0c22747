"""The cloak provers at the edges of quantities and flavors, on the CPU (cloak_witness_corpus.py): the corpus is what its
names claim; the witness queue of the product (cloak::gadget_witness, as pv_cloak_given hands it to the device prover)
means what the mix gadget demands, checked with Python integers; the oracle's prover, the host lockstep prover and the
device prover's functions on the host agree byte for byte, and the oracle's verifier says what the corpus expects.

Before run totals were carried past 64 bits, test_cpu_provers_agree_and_verify_as_expected failed for exactly the
balanced statements with a run total >= 2^64 (every prover returned success and the same bytes; the verifier said 0):
    (2, 2)  run_total:2^64, run_total:2^65-2, filler:0
    (3, 2)  run_total:2^64, run_total:2^65-2, filler:1, filler:2
    (3, 3)  run_total:2^64, run_total:2^65-2, run_total:3(2^64-1), run_total:2^64_beside_second_flavor
(the three fillers are the ones whose random totals pass 2^64), and the witness-queue test for the same statements and
for the unbalanced ones whose 64-bit sums wrap."""
import ctypes as C
import os

import pytest

import cloak_witness_corpus as corpus
from cloak_witness_corpus import L, U, SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 256


@pytest.fixture(scope="module")
def host():
    from zkvm_amd import build
    build.build()
    lib = C.CDLL(os.path.join(ROOT, "zkvm_amd", "lib", "libzkhost.so"))
    lib.zkhost_cloak_given.restype = C.c_size_t
    return lib


@pytest.fixture(scope="module")
def gens(oracle):
    B, Bb = oracle.pedersen_gens()
    return B + Bb + b"".join(oracle.bulletproof_gens(CAP, "G")) + b"".join(oracle.bulletproof_gens(CAP, "H"))


def _sides(st):
    _, n_in, _, q, f, _ = st
    vals = [(a, int.from_bytes(b, "little")) for a, b in zip(q, f)]
    return vals[:n_in], vals[n_in:]


def _res(vals):
    return [f % L for _, f in vals]


def _one_flavor_total(st, total):
    ins, outs = _sides(st)
    return len(set(_res(ins + outs))) == 1 and sum(q for q, _ in ins) == total == sum(q for q, _ in outs)


def _has_run(vals, r):
    return _res(vals).count(r) >= 2


def _own_zero(vals):
    """flavors (mod l, nonzero) that one value of quantity 0 has to itself on this side"""
    return {f % L for q, f in vals if q == 0 and f % L and _res(vals).count(f % L) == 1}


def _differ_in(st, lo_bit, hi_bit):
    fl = sorted({f for _, f in sum(_sides(st), [])})
    return len(fl) == 2 and fl[1] < L and (fl[0] ^ fl[1]) % (1 << lo_bit) == 0 and (fl[0] ^ fl[1]) >> hi_bit == 0


def _single(value):
    return lambda st: all(f == value for _, f in sum(_sides(st), []))


def _totals(vals):
    return corpus.totals([q for q, _ in vals], [f.to_bytes(32, "little") for _, f in vals])


def _zero_one_side(zero_flavor):
    """a value of quantity 0 whose flavor (0 mod l or not, as asked) the other side lacks, in a statement whose nonzero
    totals balance: only the flavor's presence differs"""
    def check(st):
        ins, outs = _sides(st)
        nonzero = lambda vals: {r: t for r, t in _totals(vals).items() if t}
        lone = [v for mine, other in ((ins, outs), (outs, ins)) for v in mine
                if v[0] == 0 and (v[1] % L == 0) == zero_flavor and v[1] % L not in _res(other)]
        return bool(lone) and nonzero(ins) == nonzero(outs)
    return check


# what a name claims, re-derived from the statement with Python integers
CLAIMS = {
    "run_total:2^64-1": lambda st: _one_flavor_total(st, 2**64 - 1),
    "run_total:2^64": lambda st: _one_flavor_total(st, 2**64),
    "run_total:2^65-2": lambda st: _one_flavor_total(st, 2**65 - 2),
    "run_total:3(2^64-1)": lambda st: _one_flavor_total(st, 3 * U) and all(v[0][0] + v[1][0] > U for v in _sides(st)),
    "run_total:2^64_beside_second_flavor": lambda st: all(len(_totals(v)) == 2 and max(_totals(v).values()) == 2**64
                                                         and 0 < min(_totals(v).values()) < 2**64 for v in _sides(st)),
    "quantity:all_zero": lambda st: not any(st[3]),
    "quantity:all_max_distinct_flavors": lambda st: all(q == U for q in st[3]) and all(len(set(_res(v))) == len(v) for v in _sides(st)),
    "quantity:zero_with_own_flavor": lambda st: bool(_own_zero(_sides(st)[0]) & _own_zero(_sides(st)[1])),
    "quantity:identical_pairs": lambda st: any(len(set(v)) < len(v) for v in _sides(st)),
    "flavor:f_and_f+l": lambda st: (lambda fl: len(fl) == 2 and fl[1] - fl[0] == L
                                    and (st[1:3] == (1, 1) or any({f for _, f in v} == set(fl) for v in _sides(st))))(
                                        sorted({f for _, f in sum(_sides(st), [])})),
    "flavor:zero_flavor_beside_merge": lambda st: any(any(q and f % L == 0 for q, f in v) and any(r and _has_run(v, r) for r in _res(v))
                                                      for v in _sides(st)),
    "flavor:differ_top_word": lambda st: _differ_in(st, 192, 256),
    "flavor:differ_bottom_word": lambda st: _differ_in(st, 0, 64),
    "flavor:descending_inputs": lambda st: (lambda r: r == sorted(r, reverse=True) and r[0] != r[-1])(_res(_sides(st)[0])),
    "flavor:interleaved_runs": lambda st: (lambda r: r[0] == r[2] != r[1])(_res(_sides(st)[0])),
    "flavor:zero_quantity_of_flavor_0_on_one_side": _zero_one_side(True),
    "unbalanced:outputs_exceed_by_1": lambda st: len(set(_res(sum(_sides(st), [])))) == 1 and sum(st[3][st[1]:]) - sum(st[3][:st[1]]) == 1,
    "unbalanced:outputs_exceed_by_2^64": lambda st: len(set(_res(sum(_sides(st), [])))) == 1 and sum(st[3][st[1]:]) - sum(st[3][:st[1]]) == 2**64,
    "unbalanced:inputs_exceed_by_2^64": lambda st: len(set(_res(sum(_sides(st), [])))) == 1 and sum(st[3][:st[1]]) - sum(st[3][st[1]:]) == 2**64,
    "unbalanced:same_totals_other_flavor": lambda st: sum(st[3][:st[1]]) == sum(st[3][st[1]:]) > 0
                                                      and not set(_res(_sides(st)[0])) & set(_res(_sides(st)[1])),
    "unbalanced:zero_quantity_flavor_on_one_side": _zero_one_side(False),
}
CLAIMS.update({"flavor:single_" + n: _single(v) for n, v in corpus.FLAVOR_SINGLES})
CLAIMS.update({"filler:%d" % k: lambda st: True for k in range(3)})


def test_corpus_is_what_it_claims():
    """every name in every shape it lists and in no other; every statement well-formed; every name's property and every
    `expect` re-derived with Python integers"""
    assert set(CLAIMS) == set(corpus.ADMITS)
    classes = {name.split(":")[0] for name in corpus.ADMITS}
    assert classes == {"run_total", "quantity", "flavor", "unbalanced", "filler"}
    for shape in SHAPES:
        sts = corpus.statements(shape)
        names = [st[0] for st in sts]
        assert len(set(names)) == len(names) and 15 <= len(names) <= 32, shape
        assert set(names) == {n for n, shapes in corpus.ADMITS.items() if shape in shapes}, shape
        for st in sts:
            name, n_in, n_out, q, f, expect = st
            assert (n_in, n_out) == shape and len(q) == len(f) == n_in + n_out, (shape, name)
            assert all(0 <= a <= U for a in q) and all(len(b) == 32 for b in f), (shape, name)
            assert CLAIMS[name](st), (shape, name)
            assert expect == int(corpus.satisfiable(n_in, q, f)), (shape, name)
            assert expect == (0 if name.startswith("unbalanced:") else 1), (shape, name)
            past = corpus.run_totals_past_2_64(n_in, q, f)
            if name.startswith("run_total:") and name != "run_total:2^64-1":
                assert past and past[-1] >= 2**64, (shape, name)
            elif not name.startswith(("filler:", "unbalanced:inputs_exceed", "unbalanced:outputs_exceed_by_2^64")):
                assert not past, (shape, name)
        assert corpus.statements(shape) == sts                       # deterministic
    # the shapes a class is built in are the ones that admit it: a total of 2^64 needs two values on both sides ...
    assert set(corpus.ADMITS["run_total:2^64"]) == {s for s in SHAPES if min(s) >= 2}
    assert set(corpus.ADMITS["run_total:2^64-1"]) == {s for s in SHAPES if max(s) >= 2}
    assert set(corpus.ADMITS["run_total:3(2^64-1)"]) == {s for s in SHAPES if min(s) >= 3}
    # ... and the fillers do put totals past 2^64 among the ordinary lanes
    assert any(corpus.run_totals_past_2_64(st[1], st[3], st[4]) for shape in SHAPES for st in corpus.statements(shape)
               if st[0].startswith("filler:"))


def _given(host, st):
    _, n_in, n_out, q, f, _ = st
    qa = (C.c_uint64 * len(q))(*q)
    cap = 3 * (n_in + n_out) + 3 + 64 * n_out
    buf = C.create_string_buffer(64 * cap)
    n = host.zkhost_cloak_given(n_in, n_out, qa, b"".join(f), buf, C.c_size_t(cap))
    assert n <= cap
    word = lambda i: int.from_bytes(buf.raw[32 * i: 32 * i + 32], "little")
    return [(word(2 * i), word(2 * i + 1)) for i in range(n)]


def _check_mix(queue, at, vals, tag):
    """one k_mix's allocations queue[at:] for the side `vals` [(q, f mod l)] against the mix gadget's definition;
    -> (the position after them, the quantities of its mid values, of its merged values)"""
    k = len(vals)
    if k <= 1:
        return at, [], []
    grouped, mid, merged = queue[at: at + k], queue[at + k: at + 2 * k - 2], queue[at + 2 * k - 2: at + 3 * k - 2]
    assert len(merged) == k, tag
    assert sorted(grouped) == sorted(vals), tag                                    # a permutation of the side's values
    a = grouped[0]
    for i in range(k - 1):                                                         # mix (A, B) -> (C, D), chained through D
        b, c = grouped[i + 1], merged[i]
        d = merged[k - 1] if i + 2 == k else mid[i]
        assert (c, d) == (a, b) or (a[1] == b[1] and c == (0, 0) and d == (a[0] + b[0], a[1])), (tag, i)   # the sum unreduced
        a = d
    # what the merge leaves: one value per flavor with the flavor's total (and the (0, 0) of the freed slots)
    left = sorted(v for v in merged if v != (0, 0))
    assert left == sorted((q, r) for r, q in _totals(vals).items()), tag
    return at + 3 * k - 2, [q for q, _ in mid], [q for q, _ in merged]


@pytest.mark.parametrize("shape", SHAPES)
def test_witness_queue_means_what_the_mix_gadget_demands(host, shape):
    for st in corpus.statements(shape):
        name, n_in, n_out, q, f, _ = st
        tag = (shape, name)
        queue = _given(host, st)
        assert all(l < L and r < L for l, r in queue), tag                         # canonical
        vals = [(a, int.from_bytes(b, "little") % L) for a, b in zip(q, f)]
        at, mid_in, merged_in = _check_mix(queue, 0, vals[:n_in], tag + ("in",))
        at, mid_out, merged_out = _check_mix(queue, at, vals[n_in:], tag + ("out",))
        pad = abs(n_in - n_out)
        assert queue[at: at + pad] == [(0, 0)] * pad, tag                          # the shorter side's shuffle padding
        at += pad
        for j in range(n_out):                                                     # 64 bit multipliers per output
            bit_pairs = queue[at: at + 64]
            assert len(bit_pairs) == 64, tag
            assert all((a + b) % L == 1 and a * b % L == 0 for a, b in bit_pairs), (tag, j)
            assert sum(b << i for i, (_, b) in enumerate(bit_pairs)) == q[n_in + j], (tag, j)
            at += 64
        assert at == len(queue), tag
        # quantities past 2^64: as merged values exactly the totals the corpus names; between two mixes only the running sum
        # of a side that has such a total, and never more than it
        assert sorted(x for x in merged_in + merged_out if x > U) == corpus.run_totals_past_2_64(n_in, q, f), tag
        for mid, side in ((mid_in, vals[:n_in]), (mid_out, vals[n_in:])):
            assert all(x <= max(_totals(side).values()) for x in mid if x > U), tag


@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_provers_agree_and_verify_as_expected(host, oracle, gens, shape):
    """oracle prover == host lockstep prover == the device prover's functions on the host (whole phases, and stage by
    stage), byte for byte; the oracle's verifier accepts exactly the statements the corpus built to hold"""
    from concurrent.futures import ThreadPoolExecutor
    n_in, n_out = shape
    sts = corpus.statements(shape)

    def prove(job):                                     # -> (rc, commitments, proof, multipliers or None)
        which, (name, _, _, q, f, _) = job
        seed = corpus.seed_of(name, shape)
        if which == "oracle":
            return oracle.cloak_prove(q, f, n_in, n_out, seed)
        qa = (C.c_uint64 * len(q))(*q)
        com, proof = C.create_string_buffer(64 * len(q)), C.create_string_buffer(4096)
        plen, nm = C.c_size_t(0), C.c_size_t(0)
        if which == "host":
            rc = host.zkhost_cloak_prove(n_in, n_out, qa, b"".join(f), seed, gens, C.c_size_t(CAP), com, proof, C.c_size_t(4096),
                                         C.byref(plen), C.byref(nm))
            return rc, com.raw, proof.raw[: plen.value], nm.value
        rc = host.zkhost_prove_dev_cloak(n_in, n_out, qa, b"".join(f), seed, gens, C.c_size_t(CAP), com, proof, C.c_size_t(4096),
                                         C.byref(plen))
        return rc, com.raw, proof.raw[: plen.value], None

    # the provers share nothing but the switch between the device prover's two readings: one pass of calls per setting,
    # the statements of a pass on a few threads (a proof over the test library's reference multiplication takes a second)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        jobs = [(which, st) for which in ("oracle", "host", "dev") for st in sts]
        out = dict(zip([(w, st[0]) for w, st in jobs], pool.map(prove, jobs)))
        host.zkhost_set_pv_staged(1)
        try:
            out.update(zip([("staged", st[0]) for st in sts], pool.map(prove, [("dev", st) for st in sts])))
        finally:
            host.zkhost_set_pv_staged(0)
    wrong = []
    for name, _, _, q, f, expect in sts:
        rc, want_com, want_proof, want_n = out["oracle", name]
        assert rc == 0, name
        for which in ("host", "dev", "staged"):
            rc, com, proof, nm = out[which, name]
            assert rc == 0 and nm in (None, want_n), (name, which)
            assert com == want_com and proof == want_proof, (name, which)
        got = int(oracle.cloak_verify(want_com, n_in, n_out, want_proof, bytes(range(64))))
        print("%s %s: verifier %d, expected %d" % (shape, name, got, expect))
        if got != expect:
            wrong.append((name, got, expect))
    assert not wrong, wrong
