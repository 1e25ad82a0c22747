"""Edge encodings of ristretto255 DECODE (RFC 9496 sec 4.3.1), built deterministically from oracle/pyref.py.

Every device decoder (curve.hpp ristretto_decode_affine, and kernels.hpp dec_front + k_decompress_post of the split
path) makes five checks.  Each entry of the corpus carries the name of the FIRST check that rejects it, in the RFC's
order ("valid" when none does):

    noncanonical   the 32 bytes, read as an integer, are >= p (bit 255 set included)
    negative       the low bit of the encoding is set
    nonsquare      v * u2^2 is not a square (SQRT_RATIO_M1(1, v u2^2) fails; 0 included)
    t_negative     t = x y is negative
    y_zero         y = 0

`checks` evaluates the five predicates the way the device reads an encoding: the sign is the encoding's low bit, and the
arithmetic runs on the low 255 bits reduced mod p.  So a non-canonical encoding also has an answer for the four later
checks, and the corpus can prove that it holds, for every check, entries that ONLY that check rejects: a decoder
without that check would accept them."""
import hashlib
import json
import os

from oracle import pyref as R

P = R.P
HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = ("noncanonical", "negative", "nonsquare", "t_negative", "y_zero")
# limb k of field.hpp starts at bit ceil(25.5 k): 26-bit even limbs, 25-bit odd limbs
LIMB_START = (0, 26, 51, 77, 102, 128, 153, 179, 204, 230, 255)


def enc(x: int) -> bytes:
    return (x % 2 ** 256).to_bytes(32, "little")


def checks(e: bytes):
    """-> the five predicates (True = the check rejects), in CLASSES order"""
    raw = int.from_bytes(e, "little")
    s = (raw % 2 ** 255) % P
    ss = s * s % P
    u1 = (1 - ss) % P
    u2 = (1 + ss) % P
    u2_sqr = u2 * u2 % P
    v = (-(R.D * u1 % P * u1) - u2_sqr) % P
    was_square, invsqrt = R.sqrt_ratio_m1(1, v * u2_sqr % P)
    den_x = invsqrt * u2 % P
    den_y = invsqrt * den_x % P * v % P
    x = R.ct_abs(2 * s * den_x % P)
    y = u1 * den_y % P
    return (raw >= P, bool(raw & 1), not was_square, R.is_neg(x * y % P), y == 0)


def label(e: bytes) -> str:
    for name, bad in zip(CLASSES, checks(e)):
        if bad:
            return name
    return "valid"


def _limb_patterns():
    """s values whose 26/25-bit limbs sit at all-ones or zero patterns near 2^255, p and the limb boundaries"""
    ones = [(1 << (LIMB_START[k + 1] - LIMB_START[k])) - 1 for k in range(10)]
    out = []
    for k in range(10):
        lo = LIMB_START[k]
        out += [ones[k] << lo,                                   # one limb all ones
                (1 << LIMB_START[k + 1]) - 1,                    # limbs 0..k all ones
                (2 ** 255 - 1) ^ (ones[k] << lo),                 # every limb all ones but limb k
                (1 << lo) - 1, 1 << lo, (1 << lo) + 1,            # around a limb boundary
                P - (1 << lo), P + (1 << lo) if k < 9 else P + 1]
    even = sum(ones[k] << LIMB_START[k] for k in range(0, 10, 2))
    odd = sum(ones[k] << LIMB_START[k] for k in range(1, 10, 2))
    out += [even, odd, even | 1, odd | 1]
    out += [2 ** 255 - 1 - j for j in range(24)]                 # [p, 2^255): every non-canonical value of 255 bits, and below p
    out += [P - 1 - j for j in range(8)] + [2 ** 254 + j for j in range(-2, 3)]
    return sorted({x for x in out if 0 <= x < 2 ** 255})


def _random_even(tag: bytes, count: int):
    raw = hashlib.shake_256(b"zkvm_amd decode corpus|" + tag).digest(32 * count)
    return [(int.from_bytes(raw[32 * i: 32 * i + 32], "little") % P) & ~1 for i in range(count)]


_CORPUS = None


def corpus():
    """-> [(32-byte encoding, label, origin)], no encoding twice, in a fixed order"""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    golden = json.load(open(os.path.join(HERE, "golden", "ristretto255.json")))
    items = []
    for v in golden["valid_encoding"]:
        items.append((bytes.fromhex(v["enc"]), "libsodium valid_encoding"))
    for v in golden["noncanonical"]:
        items.append((bytes.fromhex(v["enc"]), "libsodium noncanonical"))
    for h in golden["rfc_only_reject"]:
        items.append((bytes.fromhex(h), "libsodium rfc_only_reject"))
    # canonical even s drawn until every class that random even s reach has enough members
    want = {"valid": 48, "nonsquare": 24, "t_negative": 24}
    got = {k: 0 for k in want}
    valid_s = [int.from_bytes(e, "little") for e, _ in items if label(e) == "valid"]
    for s in _random_even(b"even s", 512):
        c = label(enc(s))
        if c in got and got[c] < want[c]:
            got[c] += 1
            items.append((enc(s), "random even s"))
            if c == "valid":
                valid_s.append(s)
    assert got == want, got
    valid_s = sorted(set(valid_s))
    small_valid = [s for s in range(19) if label(enc(s)) == "valid" or label(enc(P - s)) == "valid"]
    for s in range(19):                                          # s + p < 2^255: non-canonical; even when s is odd
        items.append((enc(s + P), "s + p, s <= 18" + (" (s or p - s valid)" if s in small_valid else "")))
    for s in valid_s[:32]:
        items.append((enc(s | 1 << 255), "valid with bit 255 set"))
        if s:
            items.append((enc(P - s), "p - s of valid s"))
    items.append((enc(0), "s = 0: the identity"))
    items.append((enc(P - 1), "s = p - 1: u1 = 0"))
    items.append((enc(1), "s = 1: u1 = 0, odd"))
    i = R.SQRT_M1
    items += [(enc(i), "s^2 = -1: u2 = 0"), (enc(P - i), "s^2 = -1: u2 = 0")]
    for s in _limb_patterns():
        items.append((enc(s), "limb pattern"))
        if s < P and not s & 1 and label(enc(s)) == "valid":
            items.append((enc(s | 1 << 255), "limb pattern, valid with bit 255 set"))
    seen, out = set(), []
    for e, origin in items:
        if e not in seen:
            seen.add(e)
            out.append((e, label(e), origin))
    _CORPUS = out
    return out


# fewest members of each class, and of each class that ONLY its own check rejects (a decoder without that check accepts them)
MIN_MEMBERS = {"valid": 64, "noncanonical": 48, "negative": 48, "nonsquare": 24, "t_negative": 24, "y_zero": 1}
MIN_SOLE = {"noncanonical": 16, "negative": 16, "nonsquare": 8, "t_negative": 8, "y_zero": 1}


def sole_rejects(entries):
    """-> {check: number of entries that this check alone rejects}"""
    out = {c: 0 for c in CLASSES}
    for e, _, _ in entries:
        bad = checks(e)
        if sum(bad) == 1:
            out[CLASSES[bad.index(True)]] += 1
    return out
