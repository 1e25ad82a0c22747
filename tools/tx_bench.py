"""zkgpu_tx_verify_batch on the committed 1024 transactions (per-stage times with ZKGPU_PROVER_TIMING=1).
usage: tx_bench.py [--device-hashing] [--device-signing] [--host-threads N] [--calls N] [--in-flight K] [copies of the fixture per call] [block chunk] [tx chunk]
(TX_BENCH_FORMAT=<word>: the base format and the layout flags, e.g. 2 for reason codes or 1042 = 2 | 0x400 | 16 for the IDs and the root; --device-hashing: or-ed with ZKGPU_TXFORMAT_HASH_ON_DEVICE; --device-signing: with
that flag and ZKGPU_TXFORMAT_SIGN_ON_DEVICE; --calls N: library calls timed alone (3); --host-threads N: the
host_threads of every call, 0 = the CPUs the process may use; --in-flight K: also K calls of that size through submit / wait)"""
import os as _os; _os.environ.setdefault("ZKGPU_TEST_HOOKS", "1")   # the profile / mode hooks (include/zkgpu_hooks.h) are not exports
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
from gpu_util import load_tx_fixture
from zkvm_amd import Context
from zkvm_amd.verifier import BulletproofGens, BlockVerifier
DEVICE_SIGNING = "--device-signing" in sys.argv
if DEVICE_SIGNING:
    sys.argv.remove("--device-signing")
DEVICE_HASHING = "--device-hashing" in sys.argv or DEVICE_SIGNING
if "--device-hashing" in sys.argv:
    sys.argv.remove("--device-hashing")
def _option(name, default):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    v = int(sys.argv[i + 1])
    del sys.argv[i: i + 2]
    return v
HOST_THREADS = _option("--host-threads", None)
IN_FLIGHT = _option("--in-flight", 0)
CALLS = _option("--calls", 3)
rep = int(sys.argv[1]) if len(sys.argv) > 1 else 1
txs = load_tx_fixture() * rep
ctx = Context(0)
gens = BulletproofGens(ctx, 256, table_bits=16)
chunk = int(sys.argv[2]) if len(sys.argv) > 2 else 0
bv = BlockVerifier(ctx, gens, chunk=chunk)
bv.set_tx_format(int(os.environ.get("TX_BENCH_FORMAT", bv.TXFORMAT_RECOLLECTED_V1)) | (bv.TXFORMAT_HASH_ON_DEVICE if DEVICE_HASHING else 0)
                 | (bv.TXFORMAT_SIGN_ON_DEVICE if DEVICE_SIGNING else 0))
if len(sys.argv) > 3:
    bv.set_tx_chunk(int(sys.argv[3]))
HT = HOST_THREADS if HOST_THREADS is not None else int(sys.argv[4]) if len(sys.argv) > 4 else 0
if os.environ.get("TX_BENCH_TRANSCRIPT_MODE"):        # experiment: the lanes' transcript replay (0 automatic, 1 lane, 2 cooperative)
    for i in range(bv.lanes()):
        bv.lane(i).set_transcript_mode(int(os.environ["TX_BENCH_TRANSCRIPT_MODE"]))
bv.verify_txs(txs[:64])
blob, lens = b"".join(txs), [len(t) for t in txs]
for _ in range(4):
    t0 = time.perf_counter()
    bm, st = bv.verify_txs_packed(blob, lens, HT)
    dt = time.perf_counter() - t0
    print("%.2f ms, %.0f tx/s (%d transactions per call)" % (dt * 1e3, len(txs) / dt, len(txs)), file=sys.stderr)
assert os.environ.get("ZKGPU_TEST_TX_FREE_HASHING") == "1" or not any(st)      # (a -DZK_MEASURE_FREE_HASHING build with that variable set makes every signature fail)
# the library call alone (offsets and output buffers made beforehand)
offs = np.zeros(len(lens) + 1, dtype=np.uint64)
np.cumsum(np.asarray(lens, dtype=np.uint64), out=offs[1:])
# (TX_BENCH_FORMAT may carry ZKGPU_TXFORMAT_RETURN_IDS / _RETURN_LOG | K << 16: the library then writes 33, or 33 + 1 + 33 K, bytes per transaction;
# with ZKGPU_TXFORMAT_RETURN_ROOT, 16, 32 more bytes behind them)
bmb, stb = C.create_string_buffer((len(lens) + 7) // 8), C.create_string_buffer(bv._tx_status_bytes(len(lens), *bv._tx_layout, bv._tx_root))
for _ in range(CALLS):
    t0 = time.perf_counter()
    rc = bv.lib.zkgpu_tx_verify_batch(bv.h, len(lens), blob, offs.ctypes.data_as(C.POINTER(C.c_uint64)), HT, bmb, stb)
    dt = time.perf_counter() - t0
    print("library call alone: %.2f ms, %.0f tx/s (rc %d)" % (dt * 1e3, len(txs) / dt, rc), file=sys.stderr)
if IN_FLIGHT:
    for _ in range(5):
        t0 = time.perf_counter()
        ids = [bv.submit_txs_packed(blob, lens, HT) for _ in range(IN_FLIGHT)]
        for i in ids:
            bv.wait_txs(i)
        dt = time.perf_counter() - t0
        print("%d calls in flight: %.2f ms, %.0f tx/s" % (IN_FLIGHT, dt * 1e3, IN_FLIGHT * len(txs) / dt), file=sys.stderr)
if DEVICE_HASHING:
    import struct
    print("transaction IDs from the device so far: %d" % struct.unpack("<Q", ctx.debug_read("tx_hashed_on_device", 8)), file=sys.stderr)
if DEVICE_SIGNING:
    print("signature challenges from the device so far: %d" % struct.unpack("<Q", ctx.debug_read("tx_signed_on_device", 8)), file=sys.stderr)
ctx.profile(True); ctx.profile_reset()
bm, st = bv.verify_txs(txs)
ctx.profile(False)
for name, (n, ms) in sorted(ctx.profile_read().items(), key=lambda kv: -kv[1][1])[:14]:
    print('%-24s %4d launches %9.3f ms' % (name, n, ms), file=sys.stderr)
