"""The arithmetic layers of the device code on their own, against Python integers:
GF(2^255-19) on 26+25-bit limb pairs (field.hpp) and the integers mod l in both device forms (sc_dev.hpp: canonical
Montgomery words, lazy ten-limb form), including the edge values of every representation."""
import random

import pytest

pytestmark = pytest.mark.gpu
P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493


@pytest.fixture(scope="module")
def ctx():
    from zkvm_amd import Context
    c = Context(0)
    yield c
    c.close()


def _vals(rng, mod, n):
    edge = [0, 1, 2, mod - 1, mod - 2, (mod - 1) // 2, 2 ** 255 - 1, 2 ** 256 - 1, 2 ** 252, 2 ** 252 - 1, mod, mod + 1, 19, 2 ** 51 - 1,
            2 ** 26 - 1, 2 ** 26, (1 << 255) - 20, sum(((1 << 26) - 1) << (26 * i) for i in range(10)) % 2 ** 256]
    out = [e % 2 ** 256 for e in edge]
    while len(out) < n:
        out.append(rng.getrandbits(256))
    return out[:n]


def _run(ctx, op, xs, ys):
    a = b"".join(x.to_bytes(32, "little") for x in xs)
    b = b"".join(y.to_bytes(32, "little") for y in ys)
    raw = ctx.debug_arith(op, a, b)
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(len(xs))]


def test_field_arithmetic_vs_python_integers(ctx):
    rng = random.Random(255)
    n = 4096
    xs, ys = _vals(rng, P, n), list(reversed(_vals(rng, P, n)))
    fx = [(x % 2 ** 255) % P for x in xs]                       # bit 255 is ignored on input
    fy = [(y % 2 ** 255) % P for y in ys]
    assert _run(ctx, 0, xs, ys) == [a * b % P for a, b in zip(fx, fy)]
    assert _run(ctx, 1, xs, ys) == [a * a % P for a in fx]
    assert _run(ctx, 2, xs, ys) == [pow(a, P - 2, P) for a in fx]
    assert _run(ctx, 3, xs, ys) == [2 * a % P for a in fx]
    assert _run(ctx, 4, xs, ys) == [pow(a, (P - 5) // 8, P) for a in fx]


def test_scalar_arithmetic_in_both_forms_vs_python_integers(ctx):
    rng = random.Random(252)
    n = 4096
    xs, ys = _vals(rng, L, n), list(reversed(_vals(rng, L, n)))
    sx, sy = [x % L for x in xs], [y % L for y in ys]
    want_mul = [a * b % L for a, b in zip(sx, sy)]
    assert _run(ctx, 10, xs, ys) == want_mul
    assert _run(ctx, 11, xs, ys) == want_mul
    assert _run(ctx, 12, xs, ys) == [((a - b) * (a + b) + 16 * a * b - b) % L for a, b in zip(sx, sy)]
    want_inv = [pow(a, L - 2, L) for a in sx]
    assert _run(ctx, 13, xs[:512], ys[:512]) == want_inv[:512]
    assert _run(ctx, 14, xs[:512], ys[:512]) == want_inv[:512]
    assert _run(ctx, 16, xs[:512], ys[:512]) == want_inv[:512]          # the fixed chain of the lane-per-proof kernels
    assert _run(ctx, 16, [0, 1, L - 1], [0, 0, 0]) == [0, 1, L - 1]
    assert _run(ctx, 15, xs, ys) == sy


# ---- the field layer on raw limb vectors (zkgpu_debug_fe_raw): the non-canonical and loose representations that DECODE and
# ---- the group law hand to the predicates and products, at the limb bounds field.hpp documents ---------------------------
START = (0, 26, 51, 77, 102, 128, 153, 179, 204, 230)       # fe_from_words: limb k starts at bit ceil(25.5 k)
M26, M25 = 2 ** 26 - 1, 2 ** 25 - 1
P_LIMBS = [M26 - 18] + [M25 if k & 1 else M26 for k in range(1, 10)]
# exclusive limb maxima (even, odd) of field.hpp's contracts
TIGHT = (2 ** 26 + 2 ** 18, 2 ** 25 + 2 ** 18)
LOOSE = (int(2 ** 27.7) + 1, int(2 ** 26.7) + 1)            # fe_mul / fe_sq operands: one fe_add / fe_sub of tight values
SUB4 = (2 ** 28 + 2 ** 26 + 2 ** 18, 2 ** 27 + 2 ** 25 + 2 ** 18)   # fe_sub4_loose output: a first operand of fe_mul only


def _value(v):
    return sum(x << START[k] for k, x in enumerate(v))


def _limbs(x):
    """canonical split of 0 <= x < 2^255 + 2^230 (limb 9 may exceed 25 bits)"""
    return [(x >> START[k]) & (M25 if k & 1 else M26) for k in range(9)] + [x >> START[9]]


def _bounded(rng, bound, n):
    """n vectors with limbs below bound = (even, odd): all-maximal, single-limb and alternating maxima first, then random"""
    top = [bound[k & 1] - 1 for k in range(10)]
    out = [top, [0] * 10, [top[k] if k & 1 else 0 for k in range(10)], [0 if k & 1 else top[k] for k in range(10)]]
    out += [[top[k] if k == j else 0 for k in range(10)] for j in range(10)]
    out += [[top[k] if k != j else 0 for k in range(10)] for j in range(10)]
    out += [[top[k] - rng.randrange(4) for k in range(10)] for _ in range(32)]
    while len(out) < n:
        out.append([rng.randrange(bound[k & 1]) for k in range(10)])
    return out[:n]


def _within(v, bound):
    return all(x < bound[k & 1] for k, x in enumerate(v))


def _fe_run(ctx, op, a, b=None):
    return ctx.debug_fe_raw(op, a, b if b is not None else [[0] * 10] * len(a))


def _noncanonical_representations():
    """representations of 0, 1, p - 1 and of values in [p, 2^255 + small) as the decoder and the group law meet them"""
    reps = []
    for m in range(4):                                               # m p + c, as far as the loose bound reaches
        for c in (0, 1, P - 1, 2, 19, P - 19):
            v = [m * P_LIMBS[k] for k in range(10)]
            cl = _limbs(c)
            rep = [v[k] + cl[k] for k in range(10)]
            if _within(rep, LOOSE):
                reps.append(rep)
    reps += [_limbs(x) for x in list(range(P, 2 ** 255)) + [2 ** 255 + j for j in range(0, 40, 3)]]
    reps.append([M26 if k % 2 == 0 else M25 for k in range(9)] + [M25 + 1])   # 2^255 + 2^230 - 1: limb 9 above 25 bits
    return reps


def test_field_predicates_on_noncanonical_limb_vectors(ctx):
    """fe_canon / fe_to_words / fe_is_negative / fe_is_zero / fe_eq on non-canonical and loose inputs"""
    rng = random.Random(2551)
    a = _noncanonical_representations()
    a += [v for v in _bounded(rng, LOOSE, 2048) if _within(v, LOOSE)]
    a += _bounded(rng, TIGHT, 512)
    assert all(_within(v, LOOSE) for v in a)
    vals = [_value(v) % P for v in a]
    # b: the same value in another representation (canonical, + p, + 2p), or a value off by one
    b = []
    for i, x in enumerate(vals):
        kind = i % 4
        if kind == 3:
            b.append(_limbs((x + 1) % P))
        else:
            c = _limbs(x)
            b.append([c[k] + kind * P_LIMBS[k] for k in range(10)])
    for op in (0, 1):                                               # r = a as given / r = fe_canon(a)
        out = _fe_run(ctx, op, a, b)
        for i, (v, x) in enumerate(zip(a, vals)):
            o = out[i]
            words = sum(w << (32 * q) for q, w in enumerate(o[10:18]))
            flags = (x & 1) | (x == 0) << 1 | (i % 4 != 3) << 2
            assert (words, o[18]) == (x, flags), (op, i, v, o)
            if op == 1:
                assert o[:10] == _limbs(x), (i, v, o)
            else:
                assert o[:10] == v


def test_field_carry_and_subtractions_at_their_limb_bounds(ctx):
    rng = random.Random(2552)
    n = 2048
    loose = _bounded(rng, LOOSE, n)
    tight = _bounded(rng, TIGHT, n)
    tight_b = list(reversed(_bounded(rng, TIGHT, n)))
    two_tight = [[x + y for x, y in zip(u, w)] for u, w in zip(tight, tight_b)]    # fe_add of two tight values
    loose_b = list(reversed(loose))

    def check(op, a, b, exact, bound):
        out = _fe_run(ctx, op, a, b)
        for i, (u, w) in enumerate(zip(a, b)):
            r = out[i][:10]
            assert _value(r) % P == exact(_value(u), _value(w)) % P, (op, i, u, w, r)
            assert _within(r, bound), (op, i, u, w, r)
            words = sum(q << (32 * j) for j, q in enumerate(out[i][10:18]))
            assert words == _value(r) % P
        return out

    check(2, loose, loose, lambda u, w: u, TIGHT)                                  # fe_carry: loose -> tight
    out = check(5, tight, tight_b, lambda u, w: u + w, LOOSE)                      # fe_add: tight + tight -> loose
    assert [o[:10] for o in out] == two_tight
    for f in (tight, [[0] * 10] * n):                                              # fe_sub: f tight, g tight -> loose, exact limbs
        out = check(6, f, tight_b, lambda u, w: u - w, LOOSE)
        assert [o[:10] for o in out] == [[u[k] + 2 * P_LIMBS[k] - w[k] for k in range(10)] for u, w in zip(f, tight_b)]
    check(7, loose, loose_b, lambda u, w: u - w, TIGHT)                            # fe_sub_c: f, g loose -> tight
    check(7, [[0] * 10] * n, loose_b, lambda u, w: u - w, TIGHT)
    for f in (tight, [[0] * 10] * n):                                              # fe_sub4_loose: f tight, g two tight
        out = check(8, f, two_tight, lambda u, w: u - w, SUB4)
        assert [o[:10] for o in out] == [[u[k] + 4 * P_LIMBS[k] - w[k] for k in range(10)] for u, w in zip(f, two_tight)]


def test_field_products_with_operands_at_their_limb_bounds(ctx):
    """fe_mul / fe_sq at the largest limbs their contract admits: tight, loose, and fe_sub4_loose output (ge_double,
    quad_double) as a first operand with a tight second operand"""
    rng = random.Random(2553)
    n = 2048
    tight, loose, sub4 = _bounded(rng, TIGHT, n), _bounded(rng, LOOSE, n), _bounded(rng, SUB4, n)
    cases = [(tight, list(reversed(tight))), (loose, list(reversed(loose))), (sub4, tight), (sub4, list(reversed(tight))),
             (loose, tight), (tight, loose)]
    for a, b in cases:
        out = _fe_run(ctx, 3, a, b)
        for i, (u, w) in enumerate(zip(a, b)):
            r = out[i][:10]
            assert _value(r) % P == _value(u) * _value(w) % P and _within(r, TIGHT), (i, u, w, r)
    for a in (tight, loose):
        out = _fe_run(ctx, 4, a)
        for i, u in enumerate(a):
            r = out[i][:10]
            assert _value(r) % P == _value(u) ** 2 % P and _within(r, TIGHT), (i, u, r)
