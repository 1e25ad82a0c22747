"""The failed-group tail after its sums are folded in LDS (k_locate_fused, k_recheck_fused): verdicts of batches that take the
locating path, fused against unfused tail and both against the oracle; and sums whose first term is loaded instead of added
to the identity (static_row_share, k_small_accumulate, the per-point tables), by value against the oracle."""
import hashlib

import pytest

import msm_corpus as mc
from gpu_util import L, bits, load_cloak_fixture, scalars

pytestmark = pytest.mark.gpu
GROUP = 16
N_FULL, N_RAGGED = 2048, 2048 + 5          # LOCATE_MIN_BATCH (pipe_plan.hpp): the smallest batch whose failed groups are located


@pytest.fixture(scope="module")
def ctx():
    from zkvm_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def planted(oracle):
    """2053 transactions (the 1024 golden 2-in/2-out proofs, twice and five more) with damage planted by group, and the
    oracle's verdict of each one: computed once, shared by the cases (the first 2048 are a batch of their own)."""
    fix, n_in, n_out, plen = load_cloak_fixture()
    n = N_RAGGED
    coms = [bytearray(fix[i % len(fix)][0]) for i in range(n)]
    proofs = [bytearray(fix[i % len(fix)][1]) for i in range(n)]

    def bad_scalar(i): proofs[i][1 + 32 * 11 + (i % 29)] ^= 1 << (i % 8)          # t_x: only the sum can tell
    def bad_a(i):
        a = (int.from_bytes(proofs[i][-64:-32], "little") + 1) % L
        proofs[i][-64:-32] = a.to_bytes(32, "little")
    def bad_point(i): coms[i][32:64] = bytes.fromhex("01" + "00" * 31)             # undecodable: left out before the sums
    bad = {}
    bad_a(GROUP * 1 + 0); bad["first"] = [GROUP * 1]                               # first position of its group
    bad_scalar(GROUP * 2 + 15); bad["last"] = [GROUP * 2 + 15]                     # last position
    bad_scalar(GROUP * 3 + 2); bad_a(GROUP * 3 + 9); bad["two"] = [GROUP * 3 + 2, GROUP * 3 + 9]      # no single culprit: all queued
    bad_point(GROUP * 6 + 15); bad_scalar(GROUP * 6 + 4); bad["left out"] = [GROUP * 6 + 4, GROUP * 6 + 15]   # last member left out
    bad_scalar(GROUP * 127 + 8); bad["far"] = [GROUP * 127 + 8]                    # the last full group of the batch
    bad_scalar(N_RAGGED - 1); bad["short"] = [N_RAGGED - 1]                        # the short group (5 members), its last
    r = hashlib.shake_256(b"tail fold").digest(64 * n)
    com_b, proof_b = b"".join(bytes(c) for c in coms), b"".join(bytes(p) for p in proofs)
    want = list(oracle.cloak_verify_batch(com_b, n_in, n_out, proof_b, plen, r, threads=16))
    rejected = sorted(i for v in bad.values() for i in v)
    assert [i for i, b in enumerate(want) if not b] == rejected
    return n_in, n_out, plen, com_b, proof_b, r, want


@pytest.fixture(scope="module")
def verifier(ctx):
    from zkvm_amd.verifier import BulletproofGens, Verifier
    gens = BulletproofGens(ctx, 256, table_bits=10)
    v = Verifier(ctx, gens)
    yield v
    v.close()
    gens.close()


@pytest.mark.parametrize("n", (N_FULL, N_RAGGED))
def test_located_verdicts_fused_and_unfused_against_the_oracle(ctx, verifier, planted, n):
    """Groups of 16 in a batch of 2048 (and of 2048 + 5: a short last group whose only damaged member is its last): a culprit
    in the first and in the last position, two in one group (nobody is named, the group is queued whole), a group whose last
    member is left out beforehand with another one damaged.  Every bitmap is the oracle's, under the fused tail (the sums
    folded in LDS) and under the unfused one (launches of their own, the same code after the fold): equal bitmaps, and the
    locating kernels really ran."""
    n_in, n_out, plen, com_b, proof_b, r, want = planted
    com_b, proof_b, r, want = com_b[: len(com_b) // N_RAGGED * n], proof_b[: plen * n], r[: 64 * n], want[:n]
    got = {}
    ctx.set_group_size(GROUP)
    ctx.profile(True)
    try:
        for tail, kernel in ((0, "k_locate_fused"), (1, "k_locate_combine")):
            ctx.set_tail_mode(tail)
            ctx.profile_reset()
            got[tail] = bits(verifier.verify_packed_gpu(n_in, n_out, n, com_b, proof_b, plen, r), n)
            assert ctx.profile_read().get(kernel, (0,))[0] == 1, (tail, kernel)
            assert got[tail] == want, (n, tail, [i for i in range(n) if got[tail][i] != want[i]])
        assert got[0] == got[1]
    finally:
        ctx.profile(False)
        ctx.set_tail_mode(0)
        ctx.set_group_size(16)


def test_first_term_of_a_sum_loaded_not_added(ctx, oracle):
    """Rows of three terms through the per-point tables (k_small_tables, k_small_accumulate), whose FIRST scalar has digit 0,
    -8 and +7 in the lowest window and digit 0, +7 and +8 in the top one: the first non-zero digit of a lane starts its sum
    from the table entry itself (negated for a negative digit), a zero digit leaves the start to a later term.  In the
    recoding s' = s + 0x88..8 a digit +8 exists only in the top window (the wrap range s >= 0x77..78) and -8 only below it.
    By value against the oracle."""
    e = mc.edge_points(oracle)
    top7, wrap = 7 << 252, int("7" * 63 + "8", 16)
    first = [0x10, 0x18, 0x17, 0, 8, 7,                            # lowest digit 0 / -8 / +7 (with and without anything above)
             top7 | 0x10, top7 | 0x18, top7 | 0x17,                # top digit +7
             wrap, wrap + 0x08, wrap + 0x10, int("7" + "8" * 63, 16),     # wrapped: +8 on top, lowest -8 / 0 / -8; every digit 0 but the top
             (1 << 252) | 0x18, int("0" + "8" * 63, 16)]
    for s in first:
        assert s < 1 << 255
    assert mc.small_recode(first[0])[1][0] == 0 and mc.small_recode(first[1])[1][0] == -8 and mc.small_recode(first[2])[1][0] == 7
    assert mc.small_recode(first[3])[1][63] == 0 and mc.small_recode(first[6])[1][63] == 7 and mc.small_recode(wrap)[1][63] == 8
    rnd = scalars("tail fold small", 2 * 64)
    pts = [e["p"], e["base"], e["neg_p"]] + e["uniform"]
    rows = []
    for i in range(64):                                             # 64 rows: the smallest batch that takes the per-point tables
        sc = mc.sc_bytes([first[i % len(first)]]) + rnd[64 * i: 64 * i + 64]
        rows.append((sc, pts[i % 7] + pts[(i + 1 + i // 7) % 7] + pts[(i + 3) % 7]))
    sc, pt, offs = b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), [3 * i for i in range(65)]
    before = ctx.msm_routes()["small"]
    out, ok = ctx.msm_batch(sc, pt, offs)
    assert ctx.msm_routes()["small"] == before + 1
    assert bits(ok, 64) == [1] * 64
    for i, (rs, rp) in enumerate(rows):
        rc, enc, _ = oracle.msm(rs, rp)
        assert rc == 0 and out[32 * i: 32 * i + 32] == enc, (i, hex(first[i % len(first)]))
