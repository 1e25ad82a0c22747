"""Edge inputs of the multiscalar multiplication, shared by tests/test_msm_corpus.py (which proves on the CPU that they are
what their names claim) and tests/test_gpu_msm_routes.py (which sends them through every route of the device code).

Scalars are integers with bit 255 clear -- what the ABI accepts, canonical or not.  Two recodings are modelled here in plain
Python, independent of the kernels: the bucket pipeline's signed radix-2^w digits (kernels.hpp, for_each_digit: digits in
(-2^(w-1), 2^(w-1)], least significant window first, 255 // w + 1 windows) and the per-point-table path's carry-free
s' = s + 0x88..8 mod 2^256 (k_small_tables / k_small_accumulate: digit t = nibble t of s' minus 8, the top nibble of a wrapped
s' read as +8)."""
L = 2**252 + 27742317777372353535851937790883648493
EIGHTS = int("8" * 64, 16)
WIDTHS = tuple(range(2, 17))


def n_windows(w: int) -> int:
    return 255 // w + 1


def signed_digits(s: int, w: int):
    """-> [d_0 .. d_{W-1}] with s = sum d_t 2^(w t), -2^(w-1) < d_t <= 2^(w-1)"""
    assert 0 <= s < 1 << 255
    half, out, carry = 1 << (w - 1), [], 0
    for t in range(n_windows(w)):
        v = ((s >> (w * t)) & ((1 << w) - 1)) + carry
        carry = 1 if v > half else 0
        out.append(v - (carry << w))
    assert carry == 0
    return out


def small_recode(s: int):
    """-> (s', [d_0 .. d_63]): the 4-bit path's recoding, s = sum d_t 16^t with -8 <= d_t <= 8"""
    assert 0 <= s < 1 << 255
    sp = (s + EIGHTS) % (1 << 256)
    nib = [(sp >> (4 * t)) & 15 for t in range(64)]
    return sp, [n - 8 for n in nib[:63]] + [nib[63] + 8 if nib[63] < 8 else nib[63] - 8]


def width_scalars(w: int):
    """[(name, value)]: the edges of the signed recoding at window width w"""
    W, half, mask = n_windows(w), 1 << (w - 1), (1 << w) - 1
    whole = [t for t in range(W) if w * t + w <= 255]          # windows that lie below bit 255 entirely
    top = 254 // w                                              # the highest window that holds a bit of the scalar
    return [("0", 0), ("1", 1), ("2", 2),
            ("half", half), ("half+1", half + 1),
            ("every window half", sum(half << (w * t) for t in whole)),
            ("every window half+1", sum((half + 1) << (w * t) for t in whole)),
            ("top window", 1 << (w * top)),
            ("bottom window", mask),
            ("2^252", 1 << 252), ("l-1", L - 1), ("l", L), ("l+1", L + 1),
            ("2^255-19", (1 << 255) - 19), ("2^255-1", (1 << 255) - 1)]


def small_scalars():
    """[(name, value)]: the edges of s' = s + 0x88..8, the wrap range s >= 0x7777..78 included"""
    out = [("0888..8", int("0" + "8" * 63, 16)),
           ("0777..78", int("0" + "7" * 62 + "8", 16)),          # s' = 0x9000..0: a zero nibble (digit -8) everywhere but the top
           ("7777..77", int("7" * 64, 16)),                      # s' = 0xFF..F: every digit +7
           ("7777..78", int("7" * 63 + "8", 16)),                # s' = 0 (wrapped): digits -8 .. -8 and +8 on top
           ("7888..88", int("7" + "8" * 63, 16)),
           ("7FFF..FF", int("7" + "F" * 63, 16))]
    for nibble, positions in ((7, (0, 17, 62, 63)), (8, (0, 17, 62)), (9, (0, 17, 62))):
        out += [("nibble %d at %d" % (nibble, p), nibble << (4 * p)) for p in positions]
    return out


def all_scalars(w: int):
    return width_scalars(w) + small_scalars()


def sc_bytes(values) -> bytes:
    return b"".join(v.to_bytes(32, "little") for v in values)


_POINTS = {}


def edge_points(oracle):
    """{"identity", "base", "p", "neg_p", "uniform": [4 encodings]} as 32-byte encodings"""
    if not _POINTS:
        import hashlib
        uni = [oracle.from_uniform_bytes(hashlib.shake_256(b"msm corpus point %d" % i).digest(64)) for i in range(5)]
        p = uni[4]
        _POINTS.update(identity=bytes(32), base=oracle.encode(oracle.basepoint()), p=p,
                       neg_p=oracle.encode(oracle.scalarmult(L - 1, oracle.decode(p))), uniform=uni[:4])
    return _POINTS


def corpus_terms(oracle, w: int, rounds: int = 3):
    """[(scalar, point encoding)]: every scalar of all_scalars(w) `rounds` times, each time on another of the edge points (the
    identity, the base point, one point again and again, from_uniform_bytes points); then P and -P under one scalar for four
    scalars (a bin that is flagged non-empty and sums to the identity) and one point eight times under one scalar (a bin
    that doubles through the unified addition).  rounds = 3: 109 terms."""
    e = edge_points(oracle)
    cycle = [e["identity"], e["base"], e["p"], e["uniform"][0], e["p"], e["uniform"][1], e["p"], e["uniform"][2], e["uniform"][3]]
    sc = [v for _, v in all_scalars(w)]
    terms = [(k, cycle[(i + 4 * r) % len(cycle)]) for r in range(rounds) for i, k in enumerate(sc)]
    for k in (1, sc[3], L - 1, (1 << 255) - 1):
        terms += [(k, e["p"]), (k, e["neg_p"])]
    terms += [(sc[4], e["uniform"][0])] * 8
    return terms


def corpus_row(oracle, w: int, rounds: int = 3):
    """-> (scalars, points) of corpus_terms as the ABI takes them"""
    terms = corpus_terms(oracle, w, rounds)
    return sc_bytes(k for k, _ in terms), b"".join(p for _, p in terms)
