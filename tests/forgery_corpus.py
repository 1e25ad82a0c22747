"""Crafted statements whose errors cancel or line up inside a group check, built deterministically from the committed
cloak fixture (statement 0 of cloak_2x2_1024.bin) and from oracle.gadget_prove (range(8)); host only.

The last two proof scalars (the inner-product a, b) enter the transcript after every challenge, so a statement's
verification equation E is linear in each of them: a copy of a valid statement with a + m d (d = D) has E = m d X for a
point X that depends on neither m nor the verifier randomness r (a and b sit in the half of the equation that r does not
multiply).  Copies with moves that add up to zero therefore CANCEL in an unweighted sum, and copies under one weight are
COLLINEAR: with moves m_t at the 1-based positions i_t of a group, S2 = sum i_t E_t is (sum i_t m_t / sum m_t) S1.

Families (Case.family):
    C   cancelling sets under independent r: a correct verifier rejects every forged member, accepts the rest, and never
        needs the ungrouped re-run
    A   aligned sets: the forged copies share one 64-byte r chunk (equal rho, whatever the map r -> rho), every other
        statement has its own.  Case.hit = the position the locating step names (an innocent statement, or a bad one that
        is not alone), or None where the position is left out of the group / lies outside it
    R   r chunks that reduce to 0, 1 and l - 1 (rho = 1 for all three: prep_kernels.hpp turns rho = 0 into 1), for valid
        statements, for one half of a C pair and for a forged statement that is alone in its group.  k_transcript reduces
        the 64 bytes as a 512-bit little-endian integer mod l (scm_from_wide; oracle.sc_reduce_wide is the same map), so
        each residue is written as itself, plus l, and as the largest 64-byte integer of its class; 2^512 - 1 itself is
        the tenth chunk.  (No homogeneous-path test gives any of these to the device: test_gpu_r1cs_mixed_groups.py's
        parity test has all-zero chunks, on the mixed call only.  Nothing is skipped.)

`model` is the group check written over the oracle's rows in Python integers: the controls of test_forgery_corpus.py and
the expected counters of test_gpu_group_soundness.py come from it.  Its weights are a hash of the r chunk -- equal chunks,
equal weights -- and the corpus never puts forged members with different chunks but equal rho into one group, so what it
says about cancelling and locating is what any correct map r -> rho gives."""
import hashlib

from gpu_util import BAD_POINT, L, load_cloak_fixture

D = 0x1234567
TOP = 2 ** 512 - 1
GROUP_SIZES = (1, 2, 3, 16, 64)


def moved(proof: bytes, which: str, m: int) -> bytes:
    """the proof with a (or b) + m d, canonical"""
    at = len(proof) - (64 if which == "a" else 32)
    v = (int.from_bytes(proof[at: at + 32], "little") + m * D) % L
    return proof[:at] + v.to_bytes(32, "little") + proof[at + 32:]


def undecodable(com: bytes) -> bytes:
    return com[:32] + BAD_POINT + com[64:]


def malformed(proof: bytes) -> bytes:
    """t_x_blinding = l: not canonical"""
    at = 1 + 32 * (12 if proof[0] == 1 else 9)
    return proof[:at] + L.to_bytes(32, "little") + proof[at + 32:]


def edge_chunks():
    """-> [(name, residue mod l, 64 bytes)]"""
    out = []
    for name, res in (("0", 0), ("1", 1), ("l-1", L - 1)):
        out += [(name, res, res), (name + "+l", res, res + L), (name + " top", res, TOP - (TOP - res) % L)]
    out.append(("2^512-1", TOP % L, TOP))
    return [(n, res, v.to_bytes(64, "little")) for n, res, v in out]


class Case:
    def __init__(self, name, family, system, members, r, group, forged, left_out=(), cancel=(), hit=None, hit_group=None):
        self.name, self.family, self.system = name, family, system
        self.members = members                    # [(commitments, proof)] in batch order
        self.r = bytes(r)                         # 64 bytes per member
        self.group = group                        # the group size the case is meant for
        self.forged = tuple(sorted(forged))       # rejected by their equation
        self.left_out = tuple(sorted(left_out))   # rejected before the sums (undecodable point, malformed proof)
        self.cancel = tuple(cancel)               # C: index sets whose unweighted sum is the identity
        self.hit, self.hit_group = hit, hit_group  # A: 1-based position named in group hit_group (None: no hit)

    def __repr__(self):
        return self.name

    @property
    def n(self):
        return len(self.members)

    def chunk(self, i):
        return self.r[64 * i: 64 * i + 64]

    def expected(self):
        return [0 if i in self.forged or i in self.left_out else 1 for i in range(self.n)]


# ---- the statements --------------------------------------------------------------------------------------------------
_RANGE8 = None


def range8_statements(oracle, count=20):
    """valid range(8) statements of the oracle's prover -> [(commitments, proof)]"""
    global _RANGE8
    if _RANGE8 is None or len(_RANGE8) < count:
        out = []
        for i in range(count):
            rc, com, proof = oracle.gadget_prove(1, 8, [(37 * i + 5) % 256], hashlib.sha256(b"forgery corpus range8 %d" % i).digest())
            assert rc == 0
            out.append((com, proof))
        _RANGE8 = out
    return _RANGE8[:count]


def _build(name, family, system, pool, n, group, moves, out=None, shared=False, chunks=None, cancel=(), hit=None, hit_group=None):
    """pool[0] is the statement the forged copies are made of, pool[1:] the clean members; moves: {index: (which, m)};
    out: {index: "point" | "scalar"}; shared: the forged members take the first one's r chunk; chunks: {index: 64 bytes}"""
    members = [pool[1 + i] for i in range(n)]
    r = bytearray(hashlib.shake_256(b"zkvm_amd forgery corpus|" + name.encode()).digest(64 * n))
    for i, (which, m) in moves.items():
        members[i] = (pool[0][0], moved(pool[0][1], which, m))
    for i, kind in (out or {}).items():
        com, proof = members[i]
        members[i] = (undecodable(com), proof) if kind == "point" else (com, malformed(proof))
    idx = sorted(moves)
    if shared:
        for i in idx[1:]:
            r[64 * i: 64 * i + 64] = r[64 * idx[0]: 64 * idx[0] + 64]
    for i, c in (chunks or {}).items():
        r[64 * i: 64 * i + 64] = c
    forged = [i for i in idx if i not in (out or {})]
    return Case(name, family, system, members, r, group, forged, sorted(out or {}), cancel, hit, hit_group)


def _cases(system, pool):
    """the cases of one system; `pool`: 54 or more distinct valid statements (the described system gets the small ones)"""
    big = system == "cloak"
    mk = lambda *a, **k: _build(a[0], a[1], system, pool, *a[2:], **k)                    # noqa: E731
    pair = lambda w, i, j: {i: (w, 1), j: (w, -1)}                                      # noqa: E731
    out = [
        mk("C pair a, batch 2", "C", 2, 2, pair("a", 0, 1), cancel=[(0, 1)]),
        mk("C pair a, check of 16", "C", 16, 16, pair("a", 0, 15), cancel=[(0, 15)]),
        mk("C pair a, malformed third", "C", 16, 16, pair("a", 1, 3), out={2: "scalar"}, cancel=[(1, 3)]),
    ]
    if not big:
        return out
    e = edge_chunks()
    out += [
        mk("C pair b, batch 2", "C", 2, 2, pair("b", 0, 1), cancel=[(0, 1)]),
        mk("C pair a, first and last of group 1 of 16", "C", 37, 16, pair("a", 16, 31), cancel=[(16, 31)]),
        mk("C pair b, first and last of the ragged group", "C", 37, 16, pair("b", 32, 36), cancel=[(32, 36)]),
        mk("C triple a, group of 3", "C", 8, 3, {3: ("a", 1), 4: ("a", 3), 5: ("a", -4)}, cancel=[(3, 4, 5)]),
        mk("C triple b, ragged group of 5 after 3 x 16", "C", 53, 16, {48: ("b", 1), 50: ("b", 3), 52: ("b", -4)}, cancel=[(48, 50, 52)]),
        mk("C pair a, undecodable between", "C", 21, 16, pair("a", 3, 5), out={4: "point"}, cancel=[(3, 5)]),
        mk("C pair b, malformed between", "C", 21, 16, pair("b", 16, 18), out={17: "scalar"}, cancel=[(16, 18)]),
        mk("C pair a, halves in groups 0 and 1 of 16", "C", 37, 16, pair("a", 15, 16), cancel=[(15, 16)]),
        mk("C pair b, halves in groups 0 and 1 of 2", "C", 5, 2, pair("b", 1, 2), cancel=[(1, 2)]),
        mk("C pair a, first and last of group 1 of 3", "C", 7, 3, pair("a", 3, 5), cancel=[(3, 5)]),
        mk("C pair b, one group of 53 under 64", "C", 53, 64, pair("b", 0, 52), cancel=[(0, 52)]),
        mk("C two pairs a and b in one group", "C", 16, 16, {2: ("a", 1), 9: ("a", -1), 4: ("b", 1), 12: ("b", -1)}, cancel=[(2, 9), (4, 12)]),
        # aligned: 1-based positions inside the group
        mk("A equal moves at 4 and 6", "A", 21, 16, {3: ("a", 1), 5: ("a", 1)}, shared=True, hit=5, hit_group=0),
        mk("A moves d, 3d at 2 and 6 of group 1", "A", 37, 16, {17: ("a", 1), 21: ("a", 3)}, shared=True, hit=5, hit_group=1),
        mk("A three equal moves at 3, 5, 7", "A", 16, 16, {2: ("b", 1), 4: ("b", 1), 6: ("b", 1)}, shared=True, hit=5, hit_group=0),
        mk("A named position is left out", "A", 21, 16, {3: ("a", 1), 5: ("a", 1)}, out={4: "point"}, shared=True, hit=None, hit_group=0),
        mk("A d, -2d at 1 and 5 of a ragged group of 5", "A", 21, 16, {16: ("a", 1), 20: ("a", -2)}, shared=True, hit=None, hit_group=1),
        mk("A d, -2d at 1 and 16 of a full group", "A", 16, 16, {0: ("b", 1), 15: ("b", -2)}, shared=True, hit=None, hit_group=0),
        mk("A equal moves at 1 and 3 of a group of 3", "A", 6, 3, {3: ("a", 1), 5: ("a", 1)}, shared=True, hit=2, hit_group=1),
        mk("A equal moves at 10 and 30 of 53 under 64", "A", 53, 64, {9: ("b", 1), 29: ("b", 1)}, shared=True, hit=20, hit_group=0),
        # weights at their edges: every chunk on a valid statement, two to a group
        mk("R every edge chunk on valid statements", "R", 21, 16, {}, chunks={2 * i + 1: c for i, (_, _, c) in enumerate(e)}),
    ]
    for name, _, c in e:
        # one half of a pair (group 0), a valid statement beside it, and a forged statement alone in the ragged group
        out.append(mk("R chunk " + name, "R", 21, 16, {2: ("a", 1), 9: ("a", -1), 18: ("b", 1)}, chunks={2: c, 5: c, 18: c, 20: c},
                      cancel=[(2, 9)]))
    return out


_CORPUS = {}


def corpus(oracle=None):
    """-> the cloak cases (C, A, R) and, with the oracle's prover at hand, the range(8) ones (C)"""
    if "cloak" not in _CORPUS:
        fix, n_in, n_out, _ = load_cloak_fixture()
        assert (n_in, n_out) == (2, 2)
        _CORPUS["cloak"] = _cases("cloak", fix[:64])
    if oracle is not None and "range8" not in _CORPUS:
        _CORPUS["range8"] = _cases("range8", range8_statements(oracle, 20))
    return _CORPUS["cloak"] + _CORPUS.get("range8", [])


def cloak_cases():
    return [c for c in corpus() if c.system == "cloak"]


# ---- the model -------------------------------------------------------------------------------------------------------
_GENS = {}


def _generators(oracle, pn):
    if pn not in _GENS:
        enc = list(oracle.pedersen_gens()) + oracle.bulletproof_gens(pn, "G") + oracle.bulletproof_gens(pn, "H")
        _GENS[pn] = [oracle.decode(e) for e in enc]
    return _GENS[pn]


def row(oracle, case, i):
    """the oracle's prepared row of member i (None: malformed) -> (scalars as ints, encoded points)"""
    com, proof = case.members[i]
    if case.system == "cloak":
        prep = oracle.cloak_verify_prepare(com, 2, 2, proof, case.chunk(i))
    else:
        prep = oracle.gadget_verify_prepare(1, 8, com, proof, case.chunk(i))
    if prep is None:
        return None
    ds, dp, ss, pn = prep[:4]
    assert len(ss) == 32 * (2 + 2 * pn)
    sc = [int.from_bytes(x[32 * j: 32 * j + 32], "little") for x in (ds, ss) for j in range(len(x) // 32)]
    return sc, [dp[32 * j: 32 * j + 32] for j in range(len(dp) // 32)], pn


def accepts(oracle, case, i):
    """the oracle's verdict for member i alone, with the case's r"""
    com, proof = case.members[i]
    if case.system == "cloak":
        return bool(oracle.cloak_verify(com, 2, 2, proof, case.chunk(i)))
    return bool(oracle.gadget_verify(1, 8, com, proof, case.chunk(i)))


def weight(chunk: bytes) -> int:
    """the model's weight of an r chunk: equal chunks, equal weights; nothing else is assumed"""
    return int.from_bytes(hashlib.shake_256(b"forgery model weight|" + chunk).digest(64), "little") % L or 1


def joined_check(oracle, case, idx, weights):
    """the rows of members idx, scalars multiplied by their weight mod l, joined into one row -> oracle.verify_batch's bit"""
    sc, pt = b"", b""
    for i, w in zip(idx, weights):
        s, dyn, pn = row(oracle, case, i)
        sc += b"".join((x * w % L).to_bytes(32, "little") for x in s)
        pt += b"".join(dyn) + b"".join(oracle.encode(g) for g in _generators(oracle, pn))
    return oracle.verify_batch(sc, pt, [0, len(sc) // 32])[0] & 1


def equation(oracle, case, i):
    """E_i = the multiscalar multiplication of member i's row, as a point (cached on the case)"""
    cache = case.__dict__.setdefault("_eq", {})
    if i not in cache:
        s, dyn, pn = row(oracle, case, i)
        cache[i] = oracle.msm_points("vartime", s, [oracle.decode(p) for p in dyn] + _generators(oracle, pn))
    return cache[i]


def is_identity(oracle, p):
    return oracle.encode(p) == bytes(32)


def same(oracle, p, q):
    return oracle.encode(p) == oracle.encode(q)


def group_sums(oracle, case, members, weights=None):
    """members: [(1-based position, index)] of the forged members of one group -> (S1, S2) under the model's weights (or
    `weights`: {index: w})"""
    terms = [(pos, (weights[i] if weights else weight(case.chunk(i))), equation(oracle, case, i)) for pos, i in members]
    s1 = oracle.msm_points("vartime", [w for _, w, _ in terms], [e for _, _, e in terms])
    s2 = oracle.msm_points("vartime", [pos * w % L for pos, w, _ in terms], [e for _, _, e in terms])
    return s1, s2


def locate(oracle, case, gs):
    """what the locating step does with the case under group size gs: per failed group (group index, position named or
    None, whether the named statement accounts for its group: S1 - E_k the identity).  Groups are runs of gs batch
    positions; positions count left-out members, which can never be named."""
    out = []
    if gs <= 1:
        return out
    for g0 in range(0, case.n, gs):
        members = [(i - g0 + 1, i) for i in range(g0, min(g0 + gs, case.n)) if i in case.forged]
        if not members:
            continue
        s1, s2 = group_sums(oracle, case, members)
        assert not is_identity(oracle, s1), "forged members cancel under the weights of their r: outside what the corpus may hold"
        named, accounts = None, False
        for i in range(g0, min(g0 + gs, case.n)):
            k = i - g0 + 1
            if i in case.left_out or not same(oracle, oracle.scalarmult(k, s1), s2):
                continue
            named = k
            rest = s1
            if i in case.forged:
                rest = oracle.msm_points("vartime", [1, L - weight(case.chunk(i))], [s1, equation(oracle, case, i)])
            accounts = is_identity(oracle, rest)
            break
        out.append((g0 // gs, named, accounts))
    return out


def reruns(oracle, case, gs):
    """ungrouped re-runs a call takes under the locating modes: one when some named statement does not account for its group"""
    return 1 if any(named is not None and not accounts for _, named, accounts in locate(oracle, case, gs)) else 0
