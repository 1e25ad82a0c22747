"""Helper of tests/test_gpu_tx_precompute.py, run as a fresh process (python tx_precompute_child.py OUT.json): one precompute-only
call with device hashing (0x2501) over the mixed-shape corpus below, with the log's window K = 4 and K = 255, in a process whose
ZKGPU_TX_HASH_LEVELS the parent chose -- the variable picks the kernel that hashes the tape, and is read when a call starts.
Writes, per window, the status bytes, the IDs and the records as hex, and the kernels the profiled call launched."""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MIXED_SHAPES = [(1, 1), (2, 2), (3, 1), (4, 4), (8, 8), (1, 16)]
PER_SHAPE = 5
WINDOWS = (4, 255)


def mixed_corpus(oracle):
    """five payments of each shape around arbitrary statement bytes, in a drawn order: every shape's run is shorter than a
    wavefront, 8x8 has a level wider than the kernel's four lanes, and 1x16 logs 17 entries -- more than K = 4"""
    from test_tx_hash_tape import wrapped
    txs = [wrapped(oracle, a, b, 7000 + 100 * a + 10 * b + c) for a, b in MIXED_SHAPES for c in range(PER_SHAPE)]
    random.Random(21).shuffle(txs)
    return txs


def raw_precompute(ctx, bv, txs, k, threads=4):
    """zkgpu_tx_verify_batch under a precompute-only format on an array of exactly the layout's size -> rc, bitmap, status, ids, records"""
    import ctypes as C
    from tx_log_util import area_bytes, split_area
    n = len(txs)
    size = area_bytes(n, k) if k else 33 * n
    offs = (C.c_uint64 * (n + 1))(*([0] + [sum(len(t) for t in txs[:i + 1]) for i in range(n)]))
    bm = C.create_string_buffer(b"\xff" * ((n + 7) // 8), (n + 7) // 8)
    st = C.create_string_buffer(b"\xa5" * (size + 64), size + 64)
    rc = ctx.lib.zkgpu_tx_verify_batch(bv.h, n, b"".join(txs), offs, threads, bm, st)
    assert st.raw[size:] == b"\xa5" * 64, "guard bytes overwritten"
    if k:
        return (rc, bm.raw) + split_area(st.raw, n, k)
    return rc, bm.raw, st.raw[:n], [st.raw[n + 32 * i: n + 32 * i + 32] for i in range(n)], [b""] * n


def main(out_path):
    from oracle import binding as oracle
    from zkvm_amd import Context
    from zkvm_amd.verifier import BlockVerifier, BulletproofGens
    oracle.load()
    txs = mixed_corpus(oracle)
    ctx = Context(0)
    gens = BulletproofGens(ctx, 256, table_bits=8)
    bv = BlockVerifier(ctx, gens, batches_in_flight=2)
    out = {}
    try:
        for k in WINDOWS:
            bv.set_tx_format(0x2501, log_k=k)
            ctx.profile(True)
            ctx.profile_reset()
            rc, bm, st, ids, recs = raw_precompute(ctx, bv, txs, k)
            names = sorted(ctx.profile_read())
            ctx.profile(False)
            out[str(k)] = dict(rc=rc, bitmap=bm.hex(), status=st.hex(), ids=[i.hex() for i in ids], records=[r.hex() for r in recs], kernels=names)
    finally:
        bv.close()
        gens.close()
        ctx.close()
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1])
