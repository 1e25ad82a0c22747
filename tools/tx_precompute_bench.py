"""Whole transaction calls, precompute-only beside verifying, from ONE process: zkgpu_tx_verify_batch over the committed 1024
payments repeated to 1024 / 8192 / 32 768 per call, under 0x2401, 0x2501, 0x401 and 0x501 in turn.
usage: tx_precompute_bench.py [--host-threads N] [--calls N] [sizes ...]
Per format and size one line: the least and the median time of `calls` library calls (5) after a warm one, offsets and output
buffers made beforehand.  ZKGPU_TX_HASH_LEVELS=1 / 0 picks the kernel that hashes the tapes of 0x2501 (csrc/tx_device.hpp)."""
import os as _os; _os.environ.setdefault("ZKGPU_TEST_HOOKS", "1")   # the profile / mode hooks (include/zkgpu_hooks.h) are not exports
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
from gpu_util import load_tx_fixture
from zkvm_amd import Context
from zkvm_amd.verifier import BulletproofGens, BlockVerifier


def _option(name, default):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    v = int(sys.argv[i + 1])
    del sys.argv[i: i + 2]
    return v


HT = _option("--host-threads", 16)
CALLS = _option("--calls", 5)
sizes = [int(a) for a in sys.argv[1:]] or [1024, 8192, 32768]
fixture = load_tx_fixture()
ctx = Context(0)
gens = BulletproofGens(ctx, 256, table_bits=16)
bv = BlockVerifier(ctx, gens)
print("host threads %d, ZKGPU_TX_HASH_LEVELS=%s" % (HT, os.environ.get("ZKGPU_TX_HASH_LEVELS", "(unset)")))
for n in sizes:
    txs = (fixture * ((n + len(fixture) - 1) // len(fixture)))[:n]
    blob, lens = b"".join(txs), [len(t) for t in txs]
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.asarray(lens, dtype=np.uint64), out=offs[1:])
    bm, st = C.create_string_buffer((n + 7) // 8), C.create_string_buffer(33 * n)
    for fmt in (0x2401, 0x2501, 0x401, 0x501):
        bv.set_tx_format(fmt)
        times = []
        for k in range(CALLS + 1):
            t0 = time.perf_counter()
            rc = bv.lib.zkgpu_tx_verify_batch(bv.h, n, blob, offs.ctypes.data_as(C.POINTER(C.c_uint64)), HT, bm, st)
            times.append(time.perf_counter() - t0)
            assert rc == 0 and st.raw[:n] == bytes([3 if fmt & 0x2000 else 0]) * n
        times = sorted(times[1:])
        print("%#06x  %6d per call: least %8.3f ms, median %8.3f ms  (%.2f M tx/s at the least)" % (fmt, n, times[0] * 1e3, times[len(times) // 2] * 1e3, n / times[0] / 1e6))
        if fmt == 0x2501:                                    # the hashing launches of one more call, timed in place by the library's own events
            ctx.profile(True); ctx.profile_reset()
            bv.lib.zkgpu_tx_verify_batch(bv.h, n, blob, offs.ctypes.data_as(C.POINTER(C.c_uint64)), HT, bm, st)
            ctx.profile(False)
            for name, (launches, ms) in sorted(ctx.profile_read().items()):
                print("          %-18s %3d launches, %8.3f ms in all, %7.1f us each" % (name, launches, ms, 1e3 * ms / launches))
            ctx.profile_reset()
bv.close()
gens.close()
ctx.close()
