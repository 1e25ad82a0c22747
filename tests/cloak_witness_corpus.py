"""Cloak statements at the edges of their quantities and flavors, for every prover of the project (the oracle's, the host
lockstep prover, the device prover and its CPU emulation); plain Python, host only.

A statement is (name, n_in, n_out, quantities, flavors, expect): n_in + n_out quantities below 2^64, as many 32-byte
flavors (any 256-bit string: a prover reduces it mod l), and expect = 1 when a correct prover's proof verifies.  `expect`
is fixed by construction, never taken from a prover.  The rule (`satisfiable`): a side's values merge into one
(total, flavor mod l) per flavor, the total an unreduced sum of Python ints, and into (0, 0) placeholders for the slots
the merge freed; the two sides' merged values must be the same multiset once the shorter side is padded with (0, 0).
So a statement holds exactly when both sides have the same map flavor -> total -- where a flavor that is present with
total 0 still counts as present, unless the flavor itself is 0 mod l: (0, 0) is what a placeholder looks like.

A name is "class:variant"; ADMITS lists the shapes every name is built in.  Classes:
    run_total   one flavor whose merged total sits around 2^64 (a 64-bit accumulator wraps from 2^64 on)
    quantity    all 0, all 2^64 - 1, a zero with a flavor of its own, equal (q, f) pairs
    flavor      edge values, two byte strings of one residue, values that differ in one 64-bit word, orders that make the
                stable sort work
    unbalanced  expect = 0, the reason in the name
    filler      seeded random balanced statements with full-range quantities and flavors"""

L = 2**252 + 27742317777372353535851937790883648493
U = 2**64 - 1
SHAPES = ((1, 1), (2, 2), (3, 2), (1, 3), (3, 1), (3, 3))
S11, S22, S32, S13, S31, S33 = SHAPES
_ALL = SHAPES
_PAIR = (S22, S32, S13, S31, S33)          # a side with two values or more: something merges or splits
_BOTH = (S22, S32, S33)                    # two or more on both sides

# ordinary values: F < G < H < l, all words nonzero; A + B + 7 < 2^64
F = 0x03a1c5e2977b40d86f21a4c3e5b7d9f00123456789abcdef0fedcba987654321
G = 0x07f3b2a1908e7d6c5b4a39281706f5e4d3c2b1a0918273645546372819a0b1c2
H = 0x0c0ffee0ddba11ad0be5e1f1ed5ca1ab1e0b5e55ed0ddba11c0c0a0de1e7edf1
A = 0x0123456789abcdef
B = 0x0fedcba987654321
T = A + B + 7
FLAVOR_SINGLES = (("0", 0), ("1", 1), ("l-1", L - 1), ("l", L), ("2^255", 2**255), ("2^256-1", 2**256 - 1))


def fb(x: int) -> bytes:
    return x.to_bytes(32, "little")


def spread(total: int, n: int):
    """total (< 2^64) as n quantities: a third of what is left each, the rest last"""
    out = []
    for _ in range(n - 1):
        out.append(total // 3)
        total -= out[-1]
    return out + [total]


def totals(quantities, flavors):
    """{flavor mod l: unreduced total} of one side; the placeholder-like (0, 0) left out"""
    t = {}
    for q, f in zip(quantities, flavors):
        r = int.from_bytes(f, "little") % L
        t[r] = t.get(r, 0) + q
    return {r: q for r, q in t.items() if (q, r) != (0, 0)}


def satisfiable(n_in, quantities, flavors) -> bool:
    return totals(quantities[:n_in], flavors[:n_in]) == totals(quantities[n_in:], flavors[n_in:])


# ---- builders: shape -> (quantities, flavors as ints, expect) --------------------------------------------------------
def _one_flavor(parts_in, parts_out, f=F, expect=1):
    return list(parts_in) + list(parts_out), [f] * (len(parts_in) + len(parts_out)), expect


def _run_max(shape):                       # 2^64 - 1 = (2^64 - 2) + 1: the largest total without a carry
    part = {1: [U], 2: [U - 1, 1], 3: [U - 1, 1, 0]}
    return _one_flavor(part[shape[0]], part[shape[1]][::-1])


def _run_2_64(shape):                      # 2^64 = 2^63 + 2^63; of three: 2^63 + 2^62 + 2^62 (only the last step carries)
    part = {2: [2**63, 2**63], 3: [2**63, 2**62, 2**62]}
    return _one_flavor(part[shape[0]], part[shape[1]][::-1])


def _run_2_65(shape):                      # 2^65 - 2 = (2^64 - 1) + (2^64 - 1)
    part = {2: [U, U], 3: [U, U, 0]}
    return _one_flavor(part[shape[0]], part[shape[1]][::-1])


def _run_three(shape):                     # 3 (2^64 - 1): carries twice, the value between the two mixes exceeds 2^64 too
    return _one_flavor([U, U, U], [U, U, U])


def _run_beside(shape):
    return [2**63, 5, 2**63, 2**63, 2**63, 5], [F, G, F, F, F, G], 1


def _all_zero(shape):
    return _one_flavor([0] * shape[0], [0] * shape[1])


def _all_max(shape):
    fl = [F, G, H][:shape[0]]
    return [U] * (2 * shape[0]), fl + fl[::-1], 1


def _zero_own_flavor(shape):
    return {S22: ([A, 0, 0, A], [F, G, G, F], 1),
            S32: ([A, 0, B, A + B, 0], [F, G, F, F, G], 1),
            S33: ([A, 0, B, 0, B, A], [F, G, F, G, F, F], 1)}[shape]


def _identical_pairs(shape):
    c = 0x00123456789abcd
    return _one_flavor([shape[1] * c] * shape[0], [shape[0] * c] * shape[1])


def _single(value):
    return lambda shape: _one_flavor(spread(T, shape[0]), spread(T, shape[1])[::-1], value)


def _alias(shape):                         # F and F + l alternate: one flavor, two byte strings
    q, _, _ = _single(F)(shape)
    n_in, n_out = shape
    return q, [F + L * (i & 1) for i in range(n_in)] + [F + L * (1 - (i & 1)) for i in range(n_out)], 1


def _zero_flavor_beside_merge(shape):      # (9, 0) is a real value; the merge of the two F leaves a (0, 0) beside it
    return {S32: ([A, B, 9, 9, A + B], [F, F, 0, 0, F], 1),
            S33: ([A, 9, B, A + B - 4, 4, 9], [F, 0, F, F, F, 0], 1)}[shape]


def _two_flavors(f1, f2):
    def build(shape):
        return {S22: ([A, B, B, A], [f1, f2, f2, f1], 1),
                S32: ([A, B, 7, B, A + 7], [f1, f2, f1, f2, f1], 1),
                S33: ([A, B, 7, B - 1, A + 7, 1], [f1, f2, f1, f2, f1, f2], 1)}[shape]
    return build


def _descending(shape):
    return {S22: ([A, B, A, B], [H, G, H, G], 1),
            S32: ([A, B, 7, B + 7, A], [H, G, G, G, H], 1),
            S33: ([A, B, 7, 7, B, A], [H, G, F, F, G, H], 1)}[shape]


def _interleaved(shape):
    return {S32: ([A, B, 7, A + 7, B], [F, G, F, F, G], 1),
            S33: ([A, B, 7, 3, B, A + 4], [F, G, F, F, G, F], 1)}[shape]


def _one_sided_zero(g, expect):            # a zero quantity whose flavor g the other side does not have
    def build(shape):
        if shape == S11:
            return [0, 0], [F, g], expect
        return {S22: ([A, 0, A - 3, 3], [F, g, F, F], expect),
                S32: ([A, 0, B, A, B], [F, g, F, F, F], expect),
                S13: ([A, A - 3, 0, 3], [F, F, g, F], expect),
                S31: ([A - 3, 0, 3, A], [F, g, F, F], expect),
                S33: ([A, 0, B, A, B - 1, 1], [F, g, F, F, F, F], expect)}[shape]
    return build


def _out_plus_one(shape):
    q, f, _ = _single(F)(shape)
    q[-1] += 1
    return q, f, 0


def _out_plus_2_64(shape):                 # a 64-bit sum of the outputs wraps to the inputs' 0
    return _one_flavor([0] * shape[0], [2**63, 2**63, 0][:shape[1]], expect=0)


def _in_plus_2_64(shape):
    return _one_flavor([2**63, 2**63, 0][:shape[0]], [0] * shape[1], expect=0)


def _other_flavor(shape):
    q, _, _ = _single(F)(shape)
    return q, [F] * shape[0] + [G] * shape[1], 0


def _filler(k):
    def build(shape):
        import random
        n_in, n_out = shape
        rng = random.Random(f"cloak filler {n_in} {n_out} {k}")
        d = rng.randrange(1, min(n_in, n_out) + 1)
        fl = [rng.getrandbits(256) for _ in range(d)]

        def slots(n):                      # every flavor at least once
            s = list(range(d)) + [rng.randrange(d) for _ in range(n - d)]
            rng.shuffle(s)
            return s

        def split(total, n):               # n quantities <= 2^64 - 1 with that sum
            out = []
            for i in range(n - 1):
                rest = (n - 1 - i) * U
                out.append(rng.randint(max(0, total - rest), min(U, total)))
                total -= out[-1]
            return out + [total]
        s_in, s_out = slots(n_in), slots(n_out)
        q = [0] * (n_in + n_out)
        for j in range(d):
            at_in = [i for i, s in enumerate(s_in) if s == j]
            at_out = [n_in + i for i, s in enumerate(s_out) if s == j]
            total = rng.randint(0, min(len(at_in), len(at_out)) * U)
            for at in (at_in, at_out):
                for i, part in zip(at, split(total, len(at))):
                    q[i] = part
        return q, [fl[s] for s in s_in + s_out], 1
    return build


# name -> (shapes it is built in, builder)
_TABLE = [
    ("run_total:2^64-1", _PAIR, _run_max),
    ("run_total:2^64", _BOTH, _run_2_64),
    ("run_total:2^65-2", _BOTH, _run_2_65),
    ("run_total:3(2^64-1)", (S33,), _run_three),
    ("run_total:2^64_beside_second_flavor", (S33,), _run_beside),
    ("quantity:all_zero", _ALL, _all_zero),
    ("quantity:all_max_distinct_flavors", (S11, S22, S33), _all_max),
    ("quantity:zero_with_own_flavor", _BOTH, _zero_own_flavor),
    ("quantity:identical_pairs", _PAIR, _identical_pairs),
] + [("flavor:single_" + n, _ALL, _single(v)) for n, v in FLAVOR_SINGLES] + [
    ("flavor:f_and_f+l", _ALL, _alias),
    ("flavor:zero_flavor_beside_merge", (S32, S33), _zero_flavor_beside_merge),
    ("flavor:differ_top_word", _BOTH, _two_flavors(F, F ^ (1 << 200))),
    ("flavor:differ_bottom_word", _BOTH, _two_flavors(F, F ^ 1)),
    ("flavor:descending_inputs", _BOTH, _descending),
    ("flavor:interleaved_runs", (S32, S33), _interleaved),
    ("flavor:zero_quantity_of_flavor_0_on_one_side", _PAIR, _one_sided_zero(0, 1)),
    ("unbalanced:outputs_exceed_by_1", _ALL, _out_plus_one),
    ("unbalanced:outputs_exceed_by_2^64", (S22, S32, S13, S33), _out_plus_2_64),
    ("unbalanced:inputs_exceed_by_2^64", (S22, S32, S31, S33), _in_plus_2_64),
    ("unbalanced:same_totals_other_flavor", _ALL, _other_flavor),
    ("unbalanced:zero_quantity_flavor_on_one_side", _ALL, _one_sided_zero(G, 0)),
] + [("filler:%d" % k, _ALL, _filler(k)) for k in range(3)]
ADMITS = {name: shapes for name, shapes, _ in _TABLE}


def statements(shape):
    """-> [(name, n_in, n_out, quantities, flavors (32 B each), expect)] of one shape, in a fixed order"""
    out = []
    for name, shapes, build in _TABLE:
        if tuple(shape) in shapes:
            q, f, expect = build(tuple(shape))
            out.append((name, shape[0], shape[1], list(q), [fb(x) for x in f], expect))
    return out


def seed_of(name: str, shape) -> bytes:
    """the 32-byte prover seed a statement is proved under wherever a test gives seeds"""
    import hashlib
    return hashlib.sha256(b"cloak witness corpus %d %d " % tuple(shape) + name.encode()).digest()


def run_totals_past_2_64(n_in, quantities, flavors):
    """the merged totals >= 2^64 of a statement, both sides, as a sorted list"""
    return sorted(t for side in ((quantities[:n_in], flavors[:n_in]), (quantities[n_in:], flavors[n_in:]))
                  for t in totals(*side).values() if t > U)
