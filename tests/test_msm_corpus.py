"""The multiscalar-multiplication corpus (tests/msm_corpus.py) is what it claims: under plain-Python models of the two
recodings the digits re-sum to the scalar, every named edge really occurs, and the C oracle that the GPU tests compare
with agrees with the big-integer reference on corpus rows -- scalars >= l and the identity point included."""
import pytest

import msm_corpus as mc


@pytest.mark.parametrize("w", mc.WIDTHS)
def test_signed_digits_resum_and_stay_in_range(w):
    half = 1 << (w - 1)
    for name, s in mc.all_scalars(w):
        d = mc.signed_digits(s, w)
        assert len(d) == 255 // w + 1
        assert sum(x << (w * t) for t, x in enumerate(d)) == s, name
        assert all(-half < x <= half for x in d), name


@pytest.mark.parametrize("w", mc.WIDTHS)
def test_every_named_edge_of_the_signed_recoding_occurs(w):
    sc = dict(mc.width_scalars(w))
    W, half = mc.n_windows(w), 1 << (w - 1)
    dig = {k: mc.signed_digits(v, w) for k, v in sc.items()}
    assert dig["0"] == [0] * W
    assert dig["half"] == [half] + [0] * (W - 1)                       # digit +half, no carry
    assert dig["half+1"] == [-(half - 1), 1] + [0] * (W - 2)           # digit -(half - 1), carry
    whole = sum(1 for t in range(W) if w * t + w <= 255)
    assert whole >= W - 2
    assert dig["every window half"] == [half] * whole + [0] * (W - whole)
    # a carry chain to the top: the first digit is -(half - 1), every further one -(half - 2), and the carry out of the last whole
    # window (W - 2 where the top window holds bits of the scalar) lands in an empty window as +1
    assert dig["every window half+1"] == [-(half - 1)] + [-(half - 2)] * (whole - 1) + [1] + [0] * (W - whole - 1)
    top = 254 // w
    assert dig["top window"] == [0] * top + [1] + [0] * (W - top - 1) and top >= W - 2
    assert dig["bottom window"] == [-1, 1] + [0] * (W - 2)
    # 2^255 - 1: -1, zeros with a carry through every window, and the carry out of window W - 2 makes the top window a power of
    # two: exactly +half where w divides 256 (at w = 16 that is 32768, which a 16-bit digit array stores wrapped)
    top_bits = 255 - w * (W - 1)
    assert dig["2^255-1"] == [-1] + [0] * (W - 2) + [1 << top_bits]
    assert (dig["2^255-1"][-1] == half) == (w in (2, 4, 8, 16))
    assert sc["l"] >= mc.L and sc["2^255-19"] > mc.L and sc["l-1"] < mc.L


def test_small_path_recoding_resums_and_its_edges_occur():
    seen_wrap = seen_zero_row = False
    for w in (4, 16):
        for name, s in mc.all_scalars(w):
            sp, d = mc.small_recode(s)
            assert sum(x << (4 * t) for t, x in enumerate(d)) == s, name
            assert all(-8 <= x <= 7 for x in d[:63]) and 0 <= d[63] <= 8, name
            wrapped = s + mc.EIGHTS >= 1 << 256
            assert wrapped == (s >= int("7" * 63 + "8", 16)) == (sp >> 252 == 0) == (d[63] == 8), name
            seen_wrap |= wrapped
            seen_zero_row |= d == [0] * 64
    assert seen_wrap and seen_zero_row
    sm = dict(mc.small_scalars())
    assert mc.small_recode(sm["7777..77"]) == (int("F" * 64, 16), [7] * 64)
    assert mc.small_recode(sm["7777..78"]) == (0, [-8] * 63 + [8])
    assert mc.small_recode(sm["0777..78"]) == (9 << 252, [-8] * 63 + [1])
    assert mc.small_recode(sm["7FFF..FF"])[0] == int("0" + "8" * 62 + "7", 16)          # wrapped, top nibble 0
    assert mc.small_recode(sm["7888..88"])[1][63] == 8 and mc.small_recode(sm["0888..8"])[1][63] == 1
    for nibble in (7, 8, 9):
        for p in (0, 17, 62):
            d = mc.small_recode(sm["nibble %d at %d" % (nibble, p)])[1]
            want = [0] * 64
            want[p] = nibble if nibble < 8 else nibble - 16
            want[p + 1] = 0 if nibble < 8 else 1
            assert d == want, (nibble, p)
    assert mc.small_recode(sm["nibble 7 at 63"])[1] == [0] * 63 + [7]
    assert mc.small_recode((1 << 255) - 1)[1] == [-1] + [0] * 62 + [8]


def test_corpus_rows_have_the_points_they_claim(oracle, pyref):
    e = mc.edge_points(oracle)
    assert pyref.pt_is_identity(pyref.decode(e["identity"]))
    assert e["base"] == pyref.encode(pyref.BASE)
    p, q = pyref.decode(e["p"]), pyref.decode(e["neg_p"])
    assert pyref.pt_is_identity(pyref.pt_add(p, q)) and e["p"] != e["neg_p"]
    assert len(set(e["uniform"] + [e["p"], e["base"], e["identity"]])) == 7
    terms = mc.corpus_terms(oracle, 7)
    assert len(terms) == 109
    pts = [t[1] for t in terms]
    assert pts.count(e["identity"]) >= 9 and pts.count(e["p"]) >= 30 and e["neg_p"] in pts
    assert terms[-8:] == [terms[-1]] * 8                                # one point eight times under one scalar


@pytest.mark.parametrize("w", (2, 9, 16))
def test_the_c_oracle_agrees_with_the_big_integer_reference_on_corpus_rows(oracle, pyref, w):
    """oracle.msm is the reference of the GPU tests; pyref is ~40 lines of modular arithmetic.  One round of the corpus per
    width (47 terms), whole and term by term for the scalars >= l and the identity point."""
    terms = mc.corpus_terms(oracle, w, rounds=1)
    dec = {enc: pyref.decode(enc) for enc in {t[1] for t in terms}}
    assert all(v is not None for v in dec.values())
    sc, pt = mc.corpus_row(oracle, w, rounds=1)
    rc, got, _ = oracle.msm(sc, pt)
    assert rc == 0 and got == pyref.encode(pyref.msm([k % mc.L for k, _ in terms], [dec[p] for _, p in terms]))
    e = mc.edge_points(oracle)
    for k in (mc.L, mc.L + 1, (1 << 255) - 19, (1 << 255) - 1, int("7" * 63 + "8", 16)):
        for enc in (e["identity"], e["base"], e["p"]):
            rc, got, _ = oracle.msm(k.to_bytes(32, "little"), enc)
            assert rc == 0 and got == pyref.encode(pyref.pt_mul(k % mc.L, dec.get(enc) or pyref.decode(enc))), (hex(k), enc.hex())
    # P and -P under one scalar: the identity's all-zero encoding
    rc, got, _ = oracle.msm(mc.sc_bytes([mc.L - 1, mc.L - 1]), e["p"] + e["neg_p"])
    assert rc == 0 and got == bytes(32)
