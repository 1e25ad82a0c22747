"""Helpers of the statements tests (ZKGPU_TXFORMAT_STATEMENTS_V1): packing a record, turning a payment of DESIGN.md sec 4.5
into the record its VM would leave, and signing records with the oracle's primitives -- nothing here goes through the
product's VM or its hashing.

A payment, as the oracle's builder lays it out (oracle/zkvm_tx.c):
  version:u64 mintime:u64 maxtime:u64 | n:u32 program | R:32 s:32 | p:u32 proof
  program: per input   push:133:(anchor:32 key:32 k=1:u32 0x02 qty:32 flavor:32)  input  signtx
           per output  push:32:qty var  push:32:flavor var
           cloak:m:n
           per output  push:32:predicate  output:1
"""
import hashlib

L = 2 ** 252 + 27742317777372353535851937790883648493
RATE = 166


def u32(x):
    return int(x).to_bytes(4, "little")


def pack(txid, R, s, keys, n_in, n_out, commitments, proof):
    """the record, field by field (the test's own statement of the framing; zkvm_amd.pack_statement is compared with it)"""
    return b"".join([txid, R, s, u32(len(keys))] + list(keys) + [u32(n_in), u32(n_out), commitments, u32(len(proof)), proof])


def fields_of_payment(oracle, tx):
    """-> dict(txid, R, s, keys, n_in, n_out, commitments, proof) of a payment the oracle built or wrapped, by walking its
    layout; the ID is the oracle's"""
    rd = lambda at: int.from_bytes(tx[at: at + 4], "little")      # noqa: E731
    pl = rd(24)
    prog, at = tx[28: 28 + pl], 0
    keys, com_in, halves = [], [], []
    while prog[at] == 0x00 and int.from_bytes(prog[at + 1: at + 5], "little") == 133:
        contract = prog[at + 5: at + 5 + 133]
        assert contract[64:69] == u32(1) + b"\x02" and prog[at + 138: at + 140] == b"\x1b\x20"
        keys.append(contract[32:64])
        com_in.append(contract[69:133])
        at += 140
    while prog[at] == 0x00:
        assert int.from_bytes(prog[at + 1: at + 5], "little") == 32 and prog[at + 37] == 0x06
        halves.append(prog[at + 5: at + 37])
        at += 38
    assert prog[at] == 0x18
    n_in, n_out = int.from_bytes(prog[at + 1: at + 5], "little"), int.from_bytes(prog[at + 5: at + 9], "little")
    assert n_in == len(keys) and 2 * n_out == len(halves)
    sig = 28 + pl
    p = rd(sig + 64)
    assert sig + 68 + p == len(tx)
    rc, txid, a, b = oracle.tx_id(tx)
    assert rc == 0 and (a, b) == (n_in, n_out)
    return dict(txid=txid, R=tx[sig: sig + 32], s=tx[sig + 32: sig + 64], keys=keys, n_in=n_in, n_out=n_out,
                commitments=b"".join(com_in) + b"".join(halves), proof=tx[sig + 68:])


def record_of_payment(oracle, tx):
    return pack(**fields_of_payment(oracle, tx))


def musig_coefficients(keys):
    """a_i = H("Musig.aggregated-key": n, X_0 .. X_{n-1}, then i), one fresh transcript per key -- with the oracle's Merlin"""
    from oracle.binding import MerlinTranscript
    out = []
    for i in range(len(keys)):
        t = MerlinTranscript(b"Musig.aggregated-key")
        t.append_u64(b"n", len(keys))
        for k in keys:
            t.append_message(b"X", k)
        t.append_u64(b"i", i)
        out.append(t.challenge_scalar(b"a_i"))
    return out


def challenge(txid, X, R):
    from oracle.binding import MerlinTranscript
    t = MerlinTranscript(b"ZkVM.signtx")
    t.append_message(b"txid", txid)
    t.append_message(b"dom-sep", b"schnorr-signature v1")
    t.append_message(b"X", X)
    t.append_message(b"R", R)
    return t.challenge_scalar(b"c")


def secret(tag, i):
    return int.from_bytes(hashlib.sha512(b"%s %d" % (tag, i)).digest(), "little") % L


class Signer:
    """k secret keys and their public encodings, made once per k (a scalar multiplication of the oracle takes a millisecond)"""

    def __init__(self, oracle, tag, k):
        self.oracle = oracle
        self.B = oracle.basepoint()
        self.x = [secret(b"key " + tag, i) for i in range(k)]
        self.X = [oracle.encode(oracle.scalarmult(x, self.B)) for x in self.x]
        a = musig_coefficients(self.X)
        self.agg_secret = sum(ai * xi for ai, xi in zip(a, self.x)) % L
        self.agg = oracle.encode(oracle.scalarmult(self.agg_secret, self.B))

    def sign(self, txid, nonce_tag):
        r = secret(b"nonce", nonce_tag)
        R = self.oracle.encode(self.oracle.scalarmult(r, self.B))
        c = challenge(txid, self.agg, R)
        return R, ((r + c * self.agg_secret) % L).to_bytes(32, "little")


def signature_holds(oracle, txid, R, s, keys):
    """every key decodes (else "key"), then s canonical, R decodes and s B = R + c sum a_i X_i (else "signature") -> None when it
    holds; computed from the oracle's group and transcript alone"""
    pts = [oracle.decode(k) for k in keys]
    s_int = int.from_bytes(s, "little")
    if s_int >= L:
        return "signature"
    if any(p is None for p in pts):
        return "key"
    Rp = oracle.decode(R)
    if Rp is None:
        return "signature"
    a = musig_coefficients(keys)
    X = oracle.msm_points("naive", a, pts) if len(pts) > 1 else oracle.scalarmult(a[0], pts[0])
    c = challenge(txid, oracle.encode(X), R)
    lhs = oracle.scalarmult(s_int, oracle.basepoint())
    rhs = oracle.add(Rp, oracle.scalarmult(c, X))
    return None if oracle.encode(lhs) == oracle.encode(rhs) else "signature"


def csr(items):
    import ctypes as C
    offs = [0]
    for it in items:
        offs.append(offs[-1] + len(it))
    return b"".join(items), (C.c_uint64 * len(offs))(*offs)


def bits(bm, n):
    return [(bm[i // 8] >> (i % 8)) & 1 for i in range(n)]
