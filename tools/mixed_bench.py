#!/usr/bin/env python3
"""Statements of 8 different constraint systems verified in ONE zkgpu_r1cs_verify_mixed call, against the same statements
sent as one zkgpu_r1cs_verify_batch_gpu call per plan (wall time of the synchronous calls, inputs in host memory for both).

    python tools/mixed_bench.py [--batches 1024,8192] [--reps 5] [--once N] [--group N]

--once N: a single mixed call of N statements (for a kernel trace of one call).
--group N: group size of the mixed call (default: the library's 16; 1: every statement alone); the counters of
zkgpu_debug_read "mixed_groups" are printed with each result.
--per-plan-group 1: the per-plan calls check every statement alone, as the mixed call does (default: groups of 16).
Plans: range(8), range(64), shuffle(5), the 1032-constraint program, two random systems with challenges, cloak 2x2 and
3x2; statements are dealt round-robin over the plans (64 distinct valid proofs per plan, repeated)."""
import os as _os; _os.environ.setdefault("ZKGPU_TEST_HOOKS", "1")   # the group-size hook (include/zkgpu_hooks.h) is not an export
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


def make_plans(ctx, gens, per_plan):
    from gpu_util import GADGET_LABEL, L, describe_range, describe_ranges, describe_shuffle, gadget_witness, random_system
    from oracle import binding as oracle
    from zkvm_amd.native import R1csDescription
    from zkvm_amd.verifier import R1csProver, R1csVerifier
    rng = random.Random(5)
    plans, pool, names, keep = [], [], [], []

    def add(name, desc, mult_def, vals, givens):
        v = R1csVerifier(ctx, gens, desc)
        keep.append(v)
        seeds = [hashlib.sha256(b"mixed bench %s %d" % (name.encode(), i)).digest() for i in range(len(vals))]
        coms, proofs = R1csProver(ctx, gens, desc, mult_def, host_threads=8).prove(vals, givens, seeds)
        plans.append(v)
        pool.append(list(zip(coms, proofs)))
        names.append(name)

    for kind, param, name in ((1, 8, "range8"), (1, 64, "range64"), (2, 5, "shuffle5"), (3, 8, "ranges8x64")):
        m, n1, n, labels, cons = describe_range(param) if kind == 1 else describe_shuffle(param) if kind == 2 else describe_ranges(param)
        vals, givens, mult_def = [], [], None
        for _ in range(per_plan):
            if kind == 1:
                values = [rng.randrange(1 << param)]
            elif kind == 3:
                values = [rng.randrange(1 << 64) for _ in range(param)]
            else:
                xs = [rng.randrange(L) for _ in range(param)]
                values = xs + sorted(xs)
            mult_def, given = gadget_witness(kind, param, values)
            vals.append(values)
            givens.append(given)
        add(name, R1csDescription(GADGET_LABEL, m, n1, n, labels, cons), mult_def, vals, givens)
    for shape, name in (((1, 4, 3, 2), "systemA"), ((2, 9, 4, 3), "systemB")):
        (m, n1, n, labels, cons), mult_def, values, given = random_system(rng, *shape)
        add(name, R1csDescription(name.encode(), m, n1, n, labels, cons), mult_def, [values] * per_plan, [given] * per_plan)
    for n_in, n_out in ((2, 2), (3, 2)):
        com, proofs = oracle.cloak_prove_batch(per_plan, n_in, n_out, b"mixed bench cloak".ljust(32, b"\0"), threads=16)
        w = 64 * (n_in + n_out)
        plans.append((n_in, n_out))
        pool.append([(com[w * i: w * (i + 1)], proofs[i]) for i in range(per_plan)])
        names.append("cloak%dx%d" % (n_in, n_out))
    return plans, pool, names, keep


def per_plan_call(ctx, gens, plan, coms, proofs, r):
    import ctypes as C
    n = len(coms)
    bm = C.create_string_buffer((n + 7) // 8)
    rc = ctx.lib.zkgpu_r1cs_verify_batch_gpu(ctx.h, gens.points.h, C.c_void_p(plan), n, b"".join(coms), b"".join(proofs),
                                             len(proofs[0]), r, bm)
    assert rc == 0
    return bm.raw


def timed(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--lds-case", type=int, default=0,
                    help="N range(8) statements alone, then the same with one 1032-constraint statement added: the cost of "
                         "the large plan's LDS to the small statements (k_mx_prepare time from the profiling hook)")
    ap.add_argument("--group", type=int, default=0,
                    help="group size of the mixed call (0: the library's default of 16; 1: every statement checked alone)")
    ap.add_argument("--per-plan-group", type=int, default=0,
                    help="group size of the per-plan calls (0: the library's default; 1: every statement checked alone, as "
                         "the mixed call does)")
    a = ap.parse_args()
    from zkvm_amd import Context
    from zkvm_amd.verifier import BulletproofGens, MixedR1csVerifier
    ctx = Context(0)
    gens = BulletproofGens(ctx, 512, table_bits=12)
    plans, pool, names, keep = make_plans(ctx, gens, 64)
    mv = MixedR1csVerifier(ctx, gens, plans)
    handles = mv.handles
    P = len(plans)
    mixed_group = a.group or 16

    def mixed_call(idx, coms, proofs, r):
        ctx.set_group_size(mixed_group)
        try:
            return mv.verify(idx, coms, proofs, r)
        finally:
            ctx.set_group_size(16)
    if a.lds_case:
        n = a.lds_case
        small = [pool[0][i % len(pool[0])] for i in range(n)]
        for label, idx, st in (("range8 alone", [0] * n, small), ("range8 + one ranges8x64", [0] * n + [3], small + [pool[3][0]])):
            coms, proofs = [x[0] for x in st], [x[1] for x in st]
            r = hashlib.shake_256(b"lds case").digest(64 * len(idx))
            t = timed(lambda: mv.verify(idx, coms, proofs, r), a.reps)
            ctx.profile(True)
            ctx.profile_reset()
            bm = mv.verify(idx, coms, proofs, r)
            prof = ctx.profile_read()
            ctx.profile(False)
            assert sum(bin(b).count("1") for b in bm) == len(idx)
            print(json.dumps({"lds_case": label, "statements": len(idx), "call_ms": round(1e3 * t, 3),
                              "k_mx_prepare_launches": prof["k_mx_prepare"][0], "k_mx_prepare_ms": round(prof["k_mx_prepare"][1], 4)}))
    for batch in ([] if a.lds_case else [a.once] if a.once else [int(x) for x in a.batches.split(",")]):
        idx = [i % P for i in range(batch)]
        st = [pool[p][(i // P) % len(pool[p])] for i, p in enumerate(idx)]
        coms, proofs = [s[0] for s in st], [s[1] for s in st]
        r = hashlib.shake_256(b"mixed bench r %d" % batch).digest(64 * batch)
        if a.once:
            bm = mixed_call(idx, coms, proofs, r)
            print(json.dumps({"once": batch, "group": mixed_group, "accepted": sum(bin(b).count("1") for b in bm),
                              "mixed_groups": list(ctx.mixed_group_stats())}))
            continue
        groups = [[i for i in range(batch) if idx[i] == p] for p in range(P)]
        bm = mixed_call(idx, coms, proofs, r)
        assert sum(bin(b).count("1") for b in bm) == batch, "every statement is valid"
        t_mixed = timed(lambda: mixed_call(idx, coms, proofs, r), a.reps)
        stats = list(ctx.mixed_group_stats())
        if a.per_plan_group:
            ctx.set_group_size(a.per_plan_group)
        t_plan = []
        for p in range(P):
            g = groups[p]
            rp = b"".join(r[64 * i: 64 * i + 64] for i in g)
            gc, gp = [coms[i] for i in g], [proofs[i] for i in g]
            t_plan.append(timed(lambda: per_plan_call(ctx, gens, handles[p], gc, gp, rp), a.reps))
        ctx.set_group_size(16)
        print(json.dumps({"batch": batch, "plans": P, "group": mixed_group, "mixed_groups": stats,
                          "per_plan_group": a.per_plan_group or 16, "mixed_ms": round(1e3 * t_mixed, 3),
                          "per_plan_sum_ms": round(1e3 * sum(t_plan), 3),
                          "per_plan_ms": {names[p]: round(1e3 * t_plan[p], 3) for p in range(P)},
                          "mixed_stmts_per_s": round(batch / t_mixed), "per_plan_stmts_per_s": round(batch / sum(t_plan)),
                          "mixed_over_per_plan": round(t_mixed / sum(t_plan), 3)}))
    mv.close()
    for k in keep:
        k.close()
    gens.close()
    ctx.close()


if __name__ == "__main__":
    main()
