"""Every device DECODE (RFC 9496 sec 4.3.1) on the edge-encoding corpus of tests/decode_corpus.py, bit for bit against
oracle/pyref.py.  There are two device decoders: the one-kernel k_decompress (curve.hpp ristretto_decode_affine) and the
split k_decompress_pre -> k_pow22523 -> k_decompress_post (kernels.hpp dec_front), which the MSM pipeline takes from
131072 points on.  Both profile as "k_decompress", so every test reads the context's decode-route counters
(zkgpu_debug_decode_routes) to prove which decoder it ran.

An accept decision is only visible where the candidate point cancels out: a verdict-level test rejects a proof with a bad
point whether the decoder refused it or accepted it and got a wrong equation.  So the MSM tests put each candidate E in a row
of its own as (k, E) + (l - k, E), plus cancelling pairs of valid padding points: the row's ok bit is exactly "E decoded"."""
import random

import pytest

import decode_corpus as DC
from gpu_util import L, bits, points

pytestmark = pytest.mark.gpu
SPLIT_FROM = 131072                 # n_dyn from which run_to_windows takes the split decoder


@pytest.fixture(scope="module")
def ctx():
    from zkvm_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    return DC.corpus()


def _mismatches(entries, got, want):
    return [(i, entries[i][2], entries[i][1], entries[i][0].hex()) for i in range(len(want)) if got[i] != want[i]][:8]


def _routes_delta(ctx, before):
    now = ctx.decode_routes()
    return tuple(a - b for a, b in zip(now, before))


def test_one_kernel_decoder_on_the_edge_corpus(ctx, corpus):
    """(a) zkgpu_decode_check: k_decompress alone, one ok byte per encoding"""
    want = [int(lbl == "valid") for _, lbl, _ in corpus]
    before = ctx.decode_routes()
    got = list(ctx.decode_check(b"".join(e for e, _, _ in corpus)))
    assert got == want, _mismatches(corpus, got, want)
    assert _routes_delta(ctx, before) == (1, len(corpus), 0, 0)


def _batch(corpus, oracle, pad_pairs, tag):
    """Rows of zkgpu_msm_batch: one per corpus entry E, (k, E) + (l - k, E) + pad_pairs cancelling pairs (expected ok bit:
    E is valid; value: the identity); then one per VALID entry, (k, E) + the pairs (ok; value encode(k * decode(E))).
    -> (scalars, points, offsets, expected ok bits, expected values or None)"""
    from oracle import pyref as R
    rng = random.Random("decode rows|" + tag)
    pads = [points(oracle, "decode pads|" + tag, 8)[32 * j: 32 * j + 32] for j in range(8)]
    sc, pt, offs, ok, vals = [], [], [0], [], []

    def pad():
        for _ in range(pad_pairs):
            k, p = rng.randrange(1, L), pads[rng.randrange(8)]
            sc.extend([k, L - k])
            pt.extend([p, p])

    for e, lbl, _ in corpus:
        k = rng.randrange(1, L)
        sc.extend([k, L - k])
        pt.extend([e, e])
        pad()
        offs.append(len(sc))
        ok.append(int(lbl == "valid"))
        vals.append(bytes(32) if lbl == "valid" else None)
    for e, lbl, _ in corpus:
        if lbl != "valid":
            continue
        k = rng.randrange(1, L)
        sc.append(k)
        pt.append(e)
        pad()
        offs.append(len(sc))
        ok.append(1)
        vals.append(R.encode(R.pt_mul(k, R.decode(e))))
    return b"".join(k.to_bytes(32, "little") for k in sc), b"".join(pt), offs, ok, vals


def _check_batch(ctx, corpus, oracle, pad_pairs, tag):
    sc, pt, offs, ok, vals = _batch(corpus, oracle, pad_pairs, tag)
    before = ctx.decode_routes()
    out, bm = ctx.msm_batch(sc, pt, offs)
    routes = _routes_delta(ctx, before)
    got = bits(bm, len(ok))
    n = len(corpus)
    assert got[:n] == ok[:n], _mismatches(corpus, got[:n], ok[:n])
    assert got[n:] == ok[n:]
    bad = [i for i, v in enumerate(vals) if v is not None and out[32 * i: 32 * i + 32] != v]
    assert not bad, [(i, out[32 * i: 32 * i + 32].hex(), vals[i].hex()) for i in bad[:4]]
    return routes, offs


def test_small_row_batch_decoder_on_the_edge_corpus(ctx, corpus, oracle):
    """(b) zkgpu_msm_batch with rows of at most 256 terms, n_dyn <= 64 B and B >= 64: the small-row path, one-kernel decoder"""
    routes, offs = _check_batch(ctx, corpus, oracle, 1, "small")
    B, n = len(offs) - 1, offs[-1]
    assert B >= 64 and n <= 64 * B and max(b - a for a, b in zip(offs, offs[1:])) <= 256
    assert routes == (1, n, 0, 0)


def test_split_decoder_on_the_edge_corpus_one_row_per_candidate(ctx, corpus, oracle):
    """(c) zkgpu_msm_batch with rows of more than 256 terms and 131072 or more in all: the bucket pipeline, split decoder"""
    routes, offs = _check_batch(ctx, corpus, oracle, 129, "split")
    n = offs[-1]
    assert n >= SPLIT_FROM and min(b - a for a, b in zip(offs, offs[1:])) > 256
    assert routes == (0, 0, 1, n)


def test_split_decoder_single_msm_reports_the_lowest_invalid_position(ctx, corpus, oracle):
    """(d) zkgpu_msm of 131072 terms: invalid corpus encodings at chosen positions raise ZKGPU_EINVALID_POINT with the lowest
    one's index, for every reject class (entries that only that class's check rejects); the valid corpus equals the oracle"""
    from zkvm_amd import ZkGpuError
    n = SPLIT_FROM
    valid = [e for e, lbl, _ in corpus if lbl == "valid"]
    rng = random.Random("decode single msm")
    sc = b"".join(rng.randrange(L).to_bytes(32, "little") for _ in range(n))
    pt = b"".join(valid[i % len(valid)] for i in range(n))
    before = ctx.decode_routes()
    rc, want, _ = oracle.msm(sc, pt)
    assert rc == 0
    assert ctx.msm(sc, pt) == want
    sole = {c: [e for e, _, _ in corpus if sum(DC.checks(e)) == 1 and DC.checks(e)[DC.CLASSES.index(c)]] for c in DC.CLASSES}
    calls = 1
    for j, where in enumerate([[0], [n - 1], [n // 2], [n // 3 + 1, 2 * n // 3]]):
        for c in DC.CLASSES:
            bad = bytearray(pt)
            for q, pos in enumerate(where):
                bad[32 * pos: 32 * pos + 32] = sole[c][(j + q) % len(sole[c])]
            with pytest.raises(ZkGpuError) as e:
                ctx.msm(sc, bytes(bad))
            assert (e.value.code, e.value.index) == (-2, min(where)), (c, where)
            calls += 1
    assert _routes_delta(ctx, before) == (0, 0, calls, calls * n)
