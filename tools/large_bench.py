"""Statements past a CU's LDS (large_prep.hpp): the device head (zkgpu_cloak_verify_batch_gpu / zkgpu_r1cs_verify_batch_gpu:
transcript, scalar preparation and multiscalar multiplications on the GPU) against the host-prepared path
(zkgpu_cloak_verify_batch / zkgpu_r1cs_verify_batch: transcript and scalars on host threads, the multiplications on the GPU),
on the same proof bytes and randomness.  One JSON line per configuration: median ms per call of each path, statements per
second, and the large path's four kernels (profiled call, ms summed over the call's launches).

Proofs come from the oracle prover: `--distinct` different statements per shape, repeated to fill the batch (a repeated
statement costs the verifier what a new one does).

    python tools/large_bench.py [--reps 5] [--distinct 32] [--host-threads 0]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("ZKGPU_TEST_HOOKS", "1")            # the per-kernel profile is a hook (include/zkgpu_hooks.h)

LARGE_KERNELS = ("k_lp_head", "k_lp_flatten", "k_lp_gens", "k_lp_tail")


def _median_ms(fn, reps):
    fn()                                                   # warm-up: plan, workspace, pinned buffers
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def _kernels(ctx, fn):
    ctx.profile(True)
    ctx.profile_reset()
    try:
        fn()
        prof = ctx.profile_read()
    finally:
        ctx.profile(False)
    return {k: round(prof[k][1], 3) for k in LARGE_KERNELS if k in prof}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--host-threads", type=int, default=0)
    args = ap.parse_args()
    from gpu_util import GADGET_LABEL, bits, describe_ranges
    from oracle import binding as oracle
    from zkvm_amd import Context
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import BulletproofGens, CloakTx, R1csVerifier, Verifier
    oracle.load()
    ctx = Context(0)
    gens = BulletproofGens(ctx, 2048, table_bits=8)
    v = Verifier(ctx, gens, host_threads=args.host_threads)
    for (n_in, n_out), batch in (((16, 16), 256), ((16, 16), 1024), ((1, 16), 1024)):
        com, proofs = oracle.cloak_prove_batch(args.distinct, n_in, n_out, hashlib.sha256(b"large bench %d %d" % (n_in, n_out)).digest(),
                                               threads=16)
        w = 64 * (n_in + n_out)
        base = [CloakTx(n_in, n_out, com[w * i: w * (i + 1)], proofs[i]) for i in range(args.distinct)]
        txs = [base[i % args.distinct] for i in range(batch)]
        plen = len(txs[0].proof)
        com_b, proof_b = b"".join(t.commitments for t in txs), b"".join(t.proof for t in txs)
        r = hashlib.shake_256(b"large bench r").digest(64 * batch)
        dev = lambda: v.verify_packed_gpu(n_in, n_out, batch, com_b, proof_b, plen, r)      # noqa: E731
        host = lambda: v.verify_bitmap(txs, r)                                              # noqa: E731
        assert dev() == host() and bits(dev(), batch) == [1] * batch
        d_ms, h_ms = _median_ms(dev, args.reps), _median_ms(host, args.reps)
        print(json.dumps({"config": "cloak %dx%d" % (n_in, n_out), "batch": batch, "device_ms": round(d_ms, 2),
                          "host_prepared_ms": round(h_ms, 2), "device_tx_per_s": round(batch / d_ms * 1e3, 1),
                          "host_prepared_tx_per_s": round(batch / h_ms * 1e3, 1), "speedup": round(h_ms / d_ms, 2),
                          "large_kernels_ms": _kernels(ctx, dev), "host_threads": args.host_threads}), flush=True)
    # a described program past the limit: 20 64-bit ranges (1280 multipliers, padded n 2048), one phase
    count, batch = 20, 256
    rv = R1csVerifier(ctx, gens, R1csDescription(GADGET_LABEL, *describe_ranges(count)))
    rng = random.Random(1)
    coms, prs = [], []
    for i in range(args.distinct):
        rc, c_, p_ = oracle.gadget_prove(3, count, [rng.randrange(1 << 64) for _ in range(count)], hashlib.sha256(b"rb %d" % i).digest())
        assert rc == 0
        coms.append(c_); prs.append(p_)
    com_b = b"".join(coms[i % args.distinct] for i in range(batch))
    proof_b = b"".join(prs[i % args.distinct] for i in range(batch))
    plen = len(prs[0])
    r = hashlib.shake_256(b"large bench ranges r").digest(64 * batch)
    dev = lambda: rv.verify_gpu(batch, com_b, proof_b, plen, r)                                          # noqa: E731
    host = lambda: rv.verify_host_prepared(batch, com_b, proof_b, plen, r, host_threads=args.host_threads)   # noqa: E731
    assert dev() == host() and bits(dev(), batch) == [1] * batch
    d_ms, h_ms = _median_ms(dev, args.reps), _median_ms(host, args.reps)
    print(json.dumps({"config": "ranges 20 x 64 bit", "batch": batch, "device_ms": round(d_ms, 2), "host_prepared_ms": round(h_ms, 2),
                      "device_tx_per_s": round(batch / d_ms * 1e3, 1), "host_prepared_tx_per_s": round(batch / h_ms * 1e3, 1),
                      "speedup": round(h_ms / d_ms, 2), "large_kernels_ms": _kernels(ctx, dev), "host_threads": args.host_threads}),
          flush=True)
    rv.close()
    v.close()
    gens.close()
    ctx.close()


if __name__ == "__main__":
    main()
