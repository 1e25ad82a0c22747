"""The device provers at the edges no other GPU test reaches: the cloak witness corpus (cloak_witness_corpus.py: run totals
around 2^64, flavors >= l, flavor 0, ties, orders, unbalanced statements) through zkgpu_cloak_prove_batch in every prover
mode against the oracle's prover and verifier, and zkgpu_r1cs_prove_batch with values, given assignments and blinding
factors that are not canonical -- the kernels take them as raw 32-byte strings (pv_from_plain), the lockstep provers
reduce them with Scalar::from_wide."""
import ctypes as C
import hashlib

import pytest

import cloak_witness_corpus as corpus
from cloak_witness_corpus import SHAPES
from gpu_util import GADGET_LABEL, K_COMMITTED, K_OUT, L, bits, describe_range, random_system

pytestmark = pytest.mark.gpu
TOP = 2**256 - 1
STRIDE = 1 + 32 * (16 + 2 * 16)


@pytest.fixture(scope="module")
def ctx():
    from zkvm_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gens(ctx):
    from zkvm_amd.verifier import BulletproofGens
    g = BulletproofGens(ctx, 256, table_bits=8)
    yield g
    g.close()


@pytest.fixture(scope="module")
def oracle_proofs(oracle):
    """shape -> [(commitments, proof)] of the oracle's prover for the corpus under corpus.seed_of; made once per shape"""
    from concurrent.futures import ThreadPoolExecutor
    made = {}

    def get(shape):
        if shape not in made:
            with ThreadPoolExecutor(max_workers=8) as pool:
                res = list(pool.map(lambda st: oracle.cloak_prove(st[3], st[4], st[1], st[2], corpus.seed_of(st[0], shape)),
                                    corpus.statements(shape)))
            assert all(rc == 0 for rc, _, _, _ in res), shape
            made[shape] = [(com, proof) for _, com, proof, _ in res]
        return made[shape]
    return get


def _verdicts(ctx, gens, oracle, txs, tag):
    """the device verifier's bits at group sizes 16 and 1, checked against the oracle's verifier"""
    from zkvm_amd.verifier import Verifier
    r = hashlib.shake_256(b"prover edges " + tag).digest(64 * len(txs))
    want = [int(oracle.cloak_verify(t.commitments, t.n_in, t.n_out, t.proof, r[64 * i: 64 * i + 64])) for i, t in enumerate(txs)]
    v = Verifier(ctx, gens)
    try:
        for group in (16, 1):
            ctx.set_group_size(group)
            assert bits(v.verify_bitmap_gpu(txs, r), len(txs)) == want, (tag, group)
    finally:
        ctx.set_group_size(16)
        v.close()
    return want


@pytest.mark.parametrize("shape", SHAPES)
def test_cloak_corpus_through_the_device_provers(ctx, gens, oracle, oracle_proofs, shape):
    """the whole corpus of a shape in one call, seeds given: host threads in lockstep, the whole proof on the device, the same
    in three slices -- every commitment and proof byte is the oracle prover's; the device verifier (in groups and alone)
    and the oracle's verifier accept exactly what the corpus built to hold"""
    from zkvm_amd.verifier import Prover
    n_in, n_out = shape
    sts = corpus.statements(shape)
    want = oracle_proofs(shape)
    qs, fs, seeds = [st[3] for st in sts], [st[4] for st in sts], [corpus.seed_of(st[0], shape) for st in sts]
    try:
        for mode in (1, 0, 16 + 3):
            ctx.set_prover_mode(mode)
            txs = Prover(ctx, gens, host_threads=8).prove(n_in, n_out, qs, fs, seeds)
            for st, tx, (com, proof) in zip(sts, txs, want):
                assert tx.commitments == com and tx.proof == proof, (mode, st[0])
    finally:
        ctx.set_prover_mode(0)
    assert _verdicts(ctx, gens, oracle, txs, b"seeded %d %d" % shape) == [st[5] for st in sts]


@pytest.mark.parametrize("shape", SHAPES)
def test_cloak_corpus_without_seeds(ctx, gens, oracle, shape):
    """seeds = None (the randomness drawn on the device): the verdicts are the corpus's, and no two commitments of the call
    are equal -- equal (quantity, flavor) pairs abound in the corpus, inside a statement and across statements"""
    from zkvm_amd.verifier import Prover
    n_in, n_out = shape
    sts = corpus.statements(shape)
    txs = Prover(ctx, gens, host_threads=8).prove(n_in, n_out, [st[3] for st in sts], [st[4] for st in sts], None)
    assert _verdicts(ctx, gens, oracle, txs, b"drawn %d %d" % shape) == [st[5] for st in sts]
    values = [(q, f) for st in sts for q, f in zip(st[3], st[4])]
    coms = [t.commitments[32 * j: 32 * j + 32] for t in txs for j in range(2 * (n_in + n_out))]
    assert len(set(values)) < len(values)                       # there are equal pairs
    assert len(set(coms)) == len(coms)


# ---- described systems with inputs that are not canonical ---------------------------------------------------------------
def _forms(x):
    """the 32-byte integers congruent to x (< l): x, x + l, and the largest one"""
    return [x, x + L, x + (TOP - x) // L * L]


def _range8_statements():
    """(values, given, blindings) per statement, as integers below 2^256: describe_range(8) for v = 0, 1, 0x5a, 255 in
    every form of v, of the bits 0 and 1 and of the blinding factor -- l (for 0), l - 1 and 2^256 - 1 among them"""
    blind = [0, L, L - 1, TOP, 12345 + L, TOP - L, 1, L + 1, 2**252, 7 + 15 * L, 2**255, L - 1 + L]
    out = []
    for i, v in enumerate([0, 0, 0, 1, 1, 0x5a, 0x5a, 0x5a, 255, 255, 255, 0x33]):
        form = i % 3
        given = []
        for k in range(8):
            bit = (v >> k) & 1
            given.append((_forms(1 - bit)[(form + k) % 3], _forms(bit)[(form + k + 1) % 3]))
        out.append(([_forms(v)[form]], given, [blind[i]]))
    return out


def _random_system_statements(values, given):
    """the witness of one random system in three forms per value, with edge blinding factors"""
    blind = [0, L, L - 1, TOP, TOP - L, 2**255]
    out = []
    for s in range(6):
        out.append(([_forms(x)[(s + j) % 3] for j, x in enumerate(values)],
                    [(_forms(a)[(s + j) % 3], _forms(b)[(s + j + 1) % 3]) for j, (a, b) in enumerate(given)],
                    [blind[(s + j) % 6] for j in range(len(values))]))
    return out


def _edge_product_system():
    """two multipliers, both given: o_0 - V_0 = 0 and o_1 = 0 -- so that 2^256 - 1, l - 1 and l can BE given assignments:
    (2^256 - 1) (l - 1) = V_0 and l * 0 = 0"""
    desc = (1, 2, 2, [], [[(K_OUT, 0, 1, -1, 0), (K_COMMITTED, 0, -1, -1, 0)], [(K_OUT, 1, 1, -1, 0)]])
    v0 = TOP * (L - 1) % L
    sts = [([_forms(v0)[s % 3]], [(TOP, L - 1), (L, 0)] if s < 2 else [(L - 1, TOP), (0, L)], [b])
           for s, b in enumerate([TOP, L, L - 1, 0])]
    return desc, [0xFFFFFFFF] * 4, sts


def _prove_raw(ctx, gens, desc, mult_def, sts, seeds, reduce):
    """zkgpu_r1cs_prove_batch on the statements' integers as 32-byte strings -- as they are, or reduced mod l here"""
    red = (lambda x: x % L) if reduce else (lambda x: x)
    enc = lambda x: red(x).to_bytes(32, "little")
    batch, m, n_given = len(sts), desc.m, len(sts[0][1])
    vb = b"".join(enc(x) for vals, _, _ in sts for x in vals)
    gb = b"".join(enc(a) + enc(b) for _, giv, _ in sts for a, b in giv)
    bb = b"".join(enc(x) for _, _, bl in sts for x in bl)
    md = (C.c_uint32 * len(mult_def))(*mult_def)
    com, proofs, plen = C.create_string_buffer(32 * m * batch), C.create_string_buffer(STRIDE * batch), C.c_size_t(0)
    ctx._check(ctx.lib.zkgpu_r1cs_prove_batch(ctx.h, gens.points.h, C.byref(desc.struct), md, gens.gens_capacity, batch, vb, bb, gb,
                                              n_given, b"".join(seeds), 4, com, proofs, STRIDE, C.byref(plen)))
    return ([com.raw[32 * m * i: 32 * m * (i + 1)] for i in range(batch)],
            [proofs.raw[STRIDE * i: STRIDE * i + plen.value] for i in range(batch)])


@pytest.mark.parametrize("system", ["range8", "random", "edge_product"])
def test_described_prover_reduces_what_is_not_canonical(ctx, gens, oracle, system):
    """values, given assignments and blinding factors as x + l, the largest 32-byte integer of a class, 2^256 - 1, l, l - 1
    and 0: in every prover mode the call's output is, byte for byte, that of the same call with every input reduced mod l
    beforehand; the commitments are v B + b B_blinding of the reduced integers; the device verifier accepts every proof"""
    import random
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import R1csVerifier
    if system == "range8":
        label, described, sts = GADGET_LABEL, describe_range(8), _range8_statements()
        mult_def = [0xFFFFFFFF] * 16
    elif system == "random":
        described, mult_def, values, given = random_system(random.Random(20260), 3, 6, 3, 2)
        assert given and len(values) == 3
        label, sts = b"random system", _random_system_statements(values, given)
    else:
        label = b"edge product"
        described, mult_def, sts = _edge_product_system()
    flat = [x for vals, giv, bl in sts for x in list(vals) + [y for ab in giv for y in ab] + list(bl)]
    assert all(0 <= x <= TOP for x in flat) and any(x >= L for x in flat)
    if system != "random":
        assert {0, L, L - 1, TOP} <= set(flat)
    desc = R1csDescription(label, *described)
    seeds = [hashlib.sha256(b"prover edges %s %d" % (system.encode(), i)).digest() for i in range(len(sts))]
    out = {}
    try:
        for mode in (1, 0, 16 + 2):
            ctx.set_prover_mode(mode)
            for reduce in (True, False):
                out[mode, reduce] = _prove_raw(ctx, gens, desc, mult_def, sts, seeds, reduce)
    finally:
        ctx.set_prover_mode(0)
    for key, got in out.items():
        assert got == out[1, True], key
    coms, proofs = out[0, False]
    B, Bb = (oracle.decode(p) for p in oracle.pedersen_gens())
    for i, (vals, _, bl) in enumerate(sts):
        for j, (v, b) in enumerate(zip(vals, bl)):
            want = oracle.encode(oracle.add(oracle.scalarmult(v % L, B), oracle.scalarmult(b % L, Bb)))
            assert coms[i][32 * j: 32 * j + 32] == want, (i, j)
    r = hashlib.shake_256(b"prover edges r " + system.encode()).digest(64 * len(sts))
    v = R1csVerifier(ctx, gens, desc)
    try:
        assert bits(v.verify_gpu(len(sts), b"".join(coms), b"".join(proofs), len(proofs[0]), r), len(sts)) == [1] * len(sts)
    finally:
        v.close()
