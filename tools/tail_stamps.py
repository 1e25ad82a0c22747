"""Where the failed-group tail spends its time: a library built with -DZK_TAIL_STAMPS (tools/build_variant.sh tail_stamps
-DZK_TAIL_STAMPS; run with ZKGPU_LIB=build/ab/tail_stamps/libzkgpu.so) notes the cycle counter at the end of every section of
k_locate_fused, k_recheck_fused and k_group_combine (kernels.hpp, TAIL_STAMP): the first lane of wavefront 0 and of the last
two wavefronts, in the workgroups of the first 16 failed groups / queued rows of one 10 240-transaction device batch with one
damaged transaction in 64 (160 failed groups), as bench.py runs it.
usage: tail_stamps.py [serial=1]   (serial: every kernel alone on the chip, as `bench.py --solo` times them)"""
import os as _os; _os.environ.setdefault("ZKGPU_TEST_HOOKS", "1")
import os, sys, statistics, struct
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_util import benched_randomness, benched_step
from zkvm_amd import Context
from zkvm_amd.verifier import BlockVerifier, BulletproofGens
serial = int(sys.argv[1]) if len(sys.argv) > 1 else 1
batch = 10240
KERNELS, WGS, WHO, SLOTS = ("k_locate_fused", "k_recheck_fused", "k_group_combine"), 16, 3, 10
NAMES = {0: "start", 1: "own share summed", 2: "past the barrier", 3: "partial sums gathered", 4: "suffix scan (sum k d_k)",
         5: "row's sum is one point", 6: "prefix scan (k S1)", 7: "verdict / culprit named", 8: "digits / locating scalars written"}
ctx = Context(0)
gens = BulletproofGens(ctx, 256, table_bits=-1)
bv = BlockVerifier(ctx, gens, batches_in_flight=5)
bv.set_merge(batch)
for i in range(bv.lanes()):
    bv.lane(i).set_serial(serial)
txs, expected = benched_step(1024, 0, 64, 0)
k = batch // 1024
com, proofs = b"".join(t[2] for t in txs) * k, b"".join(t[3] for t in txs) * k
r = benched_randomness(0, 0, 1024) * k
d = [ctx.to_device(x) for x in (com, proofs, r)]
for rep in range(3):
    bv.wait(bv.submit_dev(2, 2, batch, d[0], d[1], len(txs[0][3]), d[2]))
n = len(KERNELS) * WGS * WHO * SLOTS
raw = ctx.debug_read("tail_stamps", n * 8)
assert len(raw) == n * 8, "this library was not built with -DZK_TAIL_STAMPS"
buf = struct.unpack("<%dQ" % n, raw)
for kern, kname in enumerate(KERNELS):
    for who in range(WHO):
        # the sections a thread passed, in the order it passed them: each is timed from the stamp before it
        rows = {}
        for wg in range(WGS):
            s = buf[((kern * WGS + wg) * WHO + who) * SLOTS:][:SLOTS]
            seen = sorted((v, i) for i, v in enumerate(s) if v)
            if len(seen) < 2 or seen[0][1] != 0:
                continue
            order = tuple(i for _, i in seen)
            rows.setdefault(order, []).append([seen[j + 1][0] - seen[j][0] for j in range(len(seen) - 1)] + [seen[-1][0] - seen[0][0]])
        for order, rr in rows.items():
            tot = statistics.median(x[-1] for x in rr)
            print("%s, %s: %d workgroups, cycle-counter ticks (median; share of the stamped life)" %
                  (kname, ("thread 0 (wavefront 0)", "first lane of the last wavefront but one", "first lane of the last wavefront")[who], len(rr)))
            for j, slot in enumerate(order[1:]):
                m = statistics.median(x[j] for x in rr)
                print("  -> %-40s %9.0f  %5.1f %%" % (NAMES.get(slot, "slot %d" % slot), m, 100.0 * m / tot))
            print("  %-43s %9.0f" % ("start to last stamp", tot))
bv.close(); gens.close(); ctx.close()
