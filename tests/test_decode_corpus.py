"""The edge-encoding corpus of ristretto255 DECODE (tests/decode_corpus.py) on the CPU: its labels against oracle/pyref.py and
the C oracle, and proof that it holds, for every check of DECODE, entries that only that check rejects -- the inputs on which
tests/test_gpu_decode_edges.py holds every device decoder to the RFC."""
import decode_corpus as DC
from oracle import pyref as R

P = R.P


def test_corpus_labels_agree_with_pyref_and_the_c_oracle(oracle):
    entries = DC.corpus()
    assert len({e for e, _, _ in entries}) == len(entries) and all(len(e) == 32 for e, _, _ in entries)
    for e, lbl, origin in entries:
        assert (lbl == "valid") == (R.decode(e) is not None), (e.hex(), lbl, origin)
        assert (lbl == "valid") == (oracle.decode(e) is not None), (e.hex(), lbl, origin)
    got = oracle.decode_batch(b"".join(e for e, _, _ in entries))
    assert list(got) == [int(lbl == "valid") for _, lbl, _ in entries]
    # valid entries decode to the point they encode
    for e, lbl, _ in entries:
        if lbl == "valid":
            assert R.encode(R.decode(e)) == e


def test_constructed_encodings_carry_the_label_of_the_first_rfc_step_that_rejects_them():
    entries = DC.corpus()
    by_enc = {e: lbl for e, lbl, _ in entries}
    valid = sorted(int.from_bytes(e, "little") for e, lbl, _ in entries if lbl == "valid")
    assert by_enc[DC.enc(0)] == "valid"                                   # the identity
    assert by_enc[DC.enc(P - 1)] == "y_zero"                              # the only even canonical s with u1 = 0
    assert by_enc[DC.enc(1)] == "negative"
    assert by_enc[DC.enc(R.SQRT_M1)] in ("nonsquare", "negative")         # u2 = 0: v u2^2 = 0 is no square of 1 / (v u2^2)
    assert [by_enc[DC.enc(s + P)] for s in range(19)] == ["noncanonical"] * 19
    assert [DC.checks(DC.enc(s + P))[1] for s in range(19)] == [s % 2 == 0 for s in range(19)]   # s + p is odd for even s
    with_bit = [s for s in valid if DC.enc(s | 1 << 255) in by_enc]
    assert len(with_bit) >= 32 and all(by_enc[DC.enc(s | 1 << 255)] == "noncanonical" for s in with_bit)
    negated = [s for s in valid if s and DC.enc(P - s) in by_enc]
    assert len(negated) >= 31 and all(by_enc[DC.enc(P - s)] == "negative" for s in negated)
    for e, lbl, origin in entries:
        if origin == "random even s":
            assert lbl in ("valid", "nonsquare", "t_negative") and int.from_bytes(e, "little") < P
    # limb patterns: every limb boundary and the values just below 2^255 and p
    ints = {int.from_bytes(e, "little") for e in by_enc}
    for start in DC.LIMB_START[1:10]:
        assert {(1 << start) - 1, 1 << start, (1 << start) + 1} <= ints
    assert set(range(P, 2 ** 255)) <= ints and 2 ** 255 - 1 - 23 in ints


def test_corpus_drives_every_branch_of_decode():
    """each class holds enough members, and for every check enough entries that ONLY that check rejects: a decoder that left
    the check out, or got it wrong, would accept them"""
    entries = DC.corpus()
    counts = {c: 0 for c in DC.MIN_MEMBERS}
    for _, lbl, _ in entries:
        counts[lbl] += 1
    assert all(counts[c] >= m for c, m in DC.MIN_MEMBERS.items()), counts
    sole = DC.sole_rejects(entries)
    assert all(sole[c] >= m for c, m in DC.MIN_SOLE.items()), sole
    # the label is the first failing check, and "valid" means none fails
    for e, lbl, _ in entries:
        bad = DC.checks(e)
        assert lbl == ("valid" if not any(bad) else DC.CLASSES[bad.index(True)])
