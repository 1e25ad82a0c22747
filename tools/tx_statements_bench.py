"""Whole calls over statements records beside the transactions they came from, every leg in FRESH processes, alternated.
usage: tx_statements_bench.py [--host-threads N] [--calls N] [--rounds N] [--parent-lib PATH] [sizes ...]
Legs: 4 (records, the host's transcripts), 0x204 (records, a_i and c formed on the device), 2 (format 2 on the transactions the
records were taken from) and, with --parent-lib, format 2 on another build of the library (the parent commit's, built beside).
The committed 1024 2-in/2-out payments repeated to 1024 / 8192 / 32 768 per call; per leg, size and process one line: the least
and the median of `calls` library calls (5) after a warm one, offsets and output buffers made beforehand.  The driver starts one
child per leg and round, one at a time: --rounds 2 gives leg A, B, C, D, A, B, C, D."""
import os as _os; _os.environ.setdefault("ZKGPU_TEST_HOOKS", "1")   # the profile / mode hooks (include/zkgpu_hooks.h) are not exports
import ctypes as C
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _option(name, default, kind=int):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    v = kind(sys.argv[i + 1])
    del sys.argv[i: i + 2]
    return v


HT = _option("--host-threads", 16)
CALLS = _option("--calls", 5)
ROUNDS = _option("--rounds", 2)
PARENT = _option("--parent-lib", "", str)
LEG = _option("--leg", "", str)
sizes = [int(a) for a in sys.argv[1:]] or [1024, 8192, 32768]


def child(leg):
    import numpy as np
    from gpu_util import load_tx_fixture
    from zkvm_amd import Context
    from zkvm_amd.verifier import BulletproofGens, BlockVerifier
    fmt = int(leg.split(":")[0], 0)
    fixture = load_tx_fixture()
    if fmt & 4:
        from oracle import binding as oracle
        from tx_statements_util import record_of_payment
        oracle.load()
        fixture = [record_of_payment(oracle, t) for t in fixture]
    ctx = Context(0)
    gens = BulletproofGens(ctx, 256, table_bits=16)
    bv = BlockVerifier(ctx, gens)
    bv._check(bv.lib.zkgpu_verifier_set_tx_format(bv.h, fmt))
    for n in sizes:
        items = (fixture * ((n + len(fixture) - 1) // len(fixture)))[:n]
        blob = b"".join(items)
        offs = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(np.asarray([len(t) for t in items], dtype=np.uint64), out=offs[1:])
        bm, st = C.create_string_buffer((n + 7) // 8), C.create_string_buffer(n)
        times = []
        for k in range(CALLS + 1):
            t0 = time.perf_counter()
            rc = bv.lib.zkgpu_tx_verify_batch(bv.h, n, blob, offs.ctypes.data_as(C.POINTER(C.c_uint64)), HT, bm, st)
            times.append(time.perf_counter() - t0)
            assert rc == 0 and st.raw[:n] == bytes(n), (rc, set(st.raw[:n]))
        times = sorted(times[1:])
        print("%-12s %6d per call: least %8.3f ms, median %8.3f ms  (%.2f M/s at the least)" % (leg, n, times[0] * 1e3, times[len(times) // 2] * 1e3, n / times[0] / 1e6), flush=True)
    bv.close()
    gens.close()
    ctx.close()


if LEG:
    child(LEG)
else:
    legs = [("4", None), ("0x204", None), ("2", None)] + ([("2:parent", PARENT)] if PARENT else [])
    print("host threads %d, %d calls after a warm one, %d processes per leg" % (HT, CALLS, ROUNDS), flush=True)
    for _ in range(ROUNDS):
        for leg, lib in legs:
            env = dict(os.environ, **({"ZKGPU_LIB": lib} if lib else {}))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--host-threads", str(HT), "--calls", str(CALLS)] + [str(s) for s in sizes],
                               env=env, timeout=600)
            if r.returncode != 0:                             # (nothing more is started on the device after a child that failed)
                sys.exit("leg %s failed with %d" % (leg, r.returncode))
