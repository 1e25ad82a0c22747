"""Helper of tests/test_gpu_tx_root.py, run as a fresh process (python tx_root_child.py OUT.json): one call of 65 payments under
0x502 | 16 in a process whose ZKGPU_TX_ROOT_SPAN the parent chose -- the library reads the variable once, when it is loaded.
Writes the status array as hex and, from a second, profiled call, how often each root kernel was launched.  Also holds what the
parent and the child share: the payments and the raw call on an array of exactly the layout's size."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(1, 1), (2, 2), (1, 2)]
RETURN_ROOT = 16
GUARD = 64


def payments(oracle, n):
    """n signed, valid payments of 1x1, 2x2 and 1x2 in turn around the committed proofs: the tape orders them by shape, the call does not"""
    from gpu_util import load_mixed_fixture
    fx = load_mixed_fixture()
    txs = []
    for k in range(n):
        n_in, n_out = SHAPES[k % 3]
        com, proof = fx[(n_in, n_out)][(k // 3) % len(fx[(n_in, n_out)])]
        txs.append(oracle.tx_wrap_payment(n_in, n_out, com, proof, hashlib.sha256(b"txroot payment %d" % k).digest(), 3 + k, 10 ** 9))
        assert txs[-1]
    return txs


def old_bytes(word, n):
    k = (word >> 16) & 255
    return n * ((33 if word & 0x400 else 1) + (1 + 33 * k if k else 0))


def raw_call(ctx, bv, word, txs, threads=4):
    """zkgpu_tx_verify_batch under `word` (set here) on an array of exactly the layout's size -> rc, bitmap, everything the flagless
    word lays out, the root (None without the flag)"""
    n = len(txs)
    bv.set_tx_format(word)
    size = old_bytes(word, n) + (32 if word & RETURN_ROOT else 0)
    offs = (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:i + 1]) for i in range(n)]))
    bm = C.create_string_buffer(b"\xff" * max((n + 7) // 8, 1), max((n + 7) // 8, 1))
    st = C.create_string_buffer(b"\xa5" * (size + GUARD), size + GUARD)
    rc = ctx.lib.zkgpu_tx_verify_batch(bv.h, n, b"".join(txs), offs, threads, bm, st)
    assert st.raw[size:] == b"\xa5" * GUARD, "guard bytes overwritten"
    return rc, bm.raw[: (n + 7) // 8], st.raw[: old_bytes(word, n)], (st.raw[size - 32: size] if word & RETURN_ROOT else None)


def main(out_path):
    from oracle import binding as oracle
    from zkvm_amd import Context
    from zkvm_amd.verifier import BlockVerifier, BulletproofGens
    oracle.load()
    txs = payments(oracle, 65)
    ctx = Context(0)
    gens = BulletproofGens(ctx, 256, table_bits=8)
    bv = BlockVerifier(ctx, gens, batches_in_flight=2)
    try:
        rc, bm, area, root = raw_call(ctx, bv, 0x502 | RETURN_ROOT, txs)
        ctx.profile(True)
        ctx.profile_reset()
        again = raw_call(ctx, bv, 0x502 | RETURN_ROOT, txs)
        launches = {k: v[0] for k, v in ctx.profile_read().items() if k.startswith("k_tx_root")}
        ctx.profile(False)
        out = dict(rc=rc, bitmap=bm.hex(), area=area.hex(), root=root.hex(), same=again == (rc, bm, area, root), launches=launches)
    finally:
        bv.close()
        gens.close()
        ctx.close()
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1])
