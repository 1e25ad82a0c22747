"""The control of tests/forgery_corpus.py, on the CPU: every case does to a group check what its name says, shown with a
model of the check in Python integers over the oracle's rows (forgery_corpus.row / joined_check / group_sums).  A case that
misses its control has no place in the corpus; test_gpu_group_soundness.py gives the same cases to the device."""
import pytest

import forgery_corpus as F
from gpu_util import L


@pytest.fixture(scope="module")
def cases(oracle):
    return F.corpus(oracle)


def _by_family(cases, family):
    out = [c for c in cases if c.family == family]
    assert out
    return out


def test_corpus_holds_what_the_issue_lists(cases):
    count = {(c.system, c.family): 0 for c in cases}
    for c in cases:
        count[(c.system, c.family)] += 1
        assert c.n <= 16 * 3 + 5 and c.group in F.GROUP_SIZES and len(c.r) == 64 * c.n
        assert not set(c.forged) & set(c.left_out)
    assert count == {("cloak", "C"): 15, ("cloak", "A"): 8, ("cloak", "R"): 11, ("range8", "C"): 3}
    assert len({c.name + c.system for c in cases}) == len(cases)
    assert {c.group for c in _by_family(cases, "C")} == {2, 3, 16, 64} and {c.n for c in cases} >= {2, 53}
    for c in cases:                                       # clean members are distinct statements, forged ones copies of one
        clean = [c.members[i] for i in range(c.n) if i not in c.forged and i not in c.left_out]
        assert len(set(clean)) == len(clean)
        assert len({c.members[i][0] for i in c.forged}) <= 1
        own = [c.chunk(i) for i in range(c.n) if i not in c.forged]
        if c.family != "R":
            assert len(set(own)) == len(own)


def test_edge_chunks_reduce_as_named(oracle):
    e = F.edge_chunks()
    assert len(e) == 10 and len({c for _, _, c in e}) == 10
    for name, res, chunk in e:
        assert oracle.sc_reduce_wide(chunk) == res == int.from_bytes(chunk, "little") % L, name
    assert [res for _, res, _ in e[:9]] == [0] * 3 + [1] * 3 + [L - 1] * 3
    assert e[0][2] == bytes(64) and e[1][2] == L.to_bytes(64, "little") and e[9][2] == b"\xff" * 64
    for _, res, chunk in e[2:9:3]:                          # the largest of its class: one more l does not fit
        assert int.from_bytes(chunk, "little") + L > F.TOP


def test_oracle_rejects_every_forged_member_alone_and_accepts_every_clean_one(oracle, cases):
    for c in cases:
        for i in range(c.n):
            assert F.accepts(oracle, c, i) == (i not in c.forged and i not in c.left_out), (c, i)
        for i in c.left_out:                                # known bad before the sums: no row, or a point that does not decode
            r = F.row(oracle, c, i)
            assert r is None or any(oracle.decode(c.members[i][0][32 * j: 32 * j + 32]) is None for j in range(len(c.members[i][0]) // 32)), (c, i)
        for i in c.forged:                                  # every point decodes, every scalar is canonical: the equation alone fails
            assert F.row(oracle, c, i) is not None and not F.is_identity(oracle, F.equation(oracle, c, i)), (c, i)


def test_cancelling_sets_cancel_unweighted_and_not_under_distinct_weights(oracle, cases):
    """weight 1 for all: the sum of the set's rows is the identity although every member's r is its own; weights
    w_t = t + 2: it is not; nor is any proper subset's (a d, 3d pair does not cancel)"""
    sets = [(c, s) for c in cases for s in c.cancel]
    assert len(sets) >= len(_by_family(cases, "C"))
    for c, s in sets:
        s = list(s)
        if c.family != "R":
            assert len({c.chunk(i) for i in s}) == len(s), c
        assert F.joined_check(oracle, c, s, [1] * len(s)) == 1, c
        assert F.joined_check(oracle, c, s, [t + 2 for t in range(len(s))]) == 0, c
        assert F.joined_check(oracle, c, s[:-1], [1] * (len(s) - 1)) == 0, c
        s1, _ = F.group_sums(oracle, c, [(1, i) for i in s], {i: 1 for i in s})
        assert F.is_identity(oracle, s1), c
    # a and b moved together do not cancel: the equation is linear in each, not in both
    c = cases[0]
    com, proof = c.members[0]
    both = F.Case("a and b together", "C", c.system, [(com, F.moved(F.moved(proof, "b", 1), "a", 2)), (com, F.moved(F.moved(proof, "b", -1), "a", 0))],
                  c.r, 2, (0, 1))
    assert F.joined_check(oracle, both, [0, 1], [1, 1]) == 0


def test_cancelling_sets_locate_nobody(oracle, cases):
    """under independent weights no position fits S2 = k S1: the group is re-checked member by member, whatever the group size"""
    for c in _by_family(cases, "C"):
        for gs in F.GROUP_SIZES:
            assert all(named is None or accounts for _, named, accounts in F.locate(oracle, c, gs)), (c, gs)
            assert F.reruns(oracle, c, gs) == 0, (c, gs)
        at = F.locate(oracle, c, c.group)
        together = len({i // c.group for i in c.forged}) == 1
        assert [named for _, named, _ in at] == ([None] if together else [(i % c.group) + 1 for i in c.forged]), c


def test_aligned_sets_name_the_position_stated(oracle, cases):
    """S1 is not the identity; S2 = k S1 for exactly the k the case states among 1 .. group, or for none"""
    for c in _by_family(cases, "A"):
        assert len({c.chunk(i) for i in c.forged}) == 1, c
        g0 = c.hit_group * c.group
        assert all(g0 <= i < g0 + c.group for i in c.forged), c
        s1, s2 = F.group_sums(oracle, c, [(i - g0 + 1, i) for i in c.forged])
        assert not F.is_identity(oracle, s1), c
        ks = [k for k in range(1, c.group + 1) if F.same(oracle, oracle.scalarmult(k, s1), s2)]
        in_group = min(c.group, c.n - g0)
        if c.hit is not None:
            assert ks == [c.hit] and c.hit <= in_group and g0 + c.hit - 1 not in c.left_out, (c, ks)
            # the statement named is innocent, or bad but not alone: S1 - E_k is not the identity
            assert F.locate(oracle, c, c.group) == [(c.hit_group, c.hit, False)], c
            assert F.reruns(oracle, c, c.group) == 1, c
        else:
            assert not ks or ks[0] > in_group or g0 + ks[0] - 1 in c.left_out, (c, ks)
            assert F.locate(oracle, c, c.group) == [(c.hit_group, None, False)], c
            assert F.reruns(oracle, c, c.group) == 0, c
        assert F.reruns(oracle, c, 1) == 0


def test_edge_weight_cases_are_ordinary_to_the_model(oracle, cases):
    """the R cases: the pair cancels unweighted (above), its halves have different chunks, the forged statement beside
    them is alone in its group at the case's group size and is named there -- and accounts for its group"""
    for c in _by_family(cases, "R"):
        if not c.forged:
            continue
        assert c.forged == (2, 9, 18) and c.chunk(2) == c.chunk(18) != c.chunk(9), c
        assert F.locate(oracle, c, c.group) == [(0, None, False), (1, 3, True)], c
        for gs in F.GROUP_SIZES:
            assert F.reruns(oracle, c, gs) == 0, (c, gs)
