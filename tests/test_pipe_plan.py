"""The plan of one device batch of the verification pipeline (zkvm_amd/csrc/pipe_plan.hpp through libzkhost.so,
zkhost_pipe_plan): the geometry pipe_enqueue settles before its first launch and the bytes of every workspace buffer --
against a model of the sizing rules written here, on the CPU; then, directly, that every buffer a launch of the plan writes
is at least as large as that launch's grid needs, and that no size shrinks when the batch grows."""
import ctypes as C
import itertools
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT, NIELS, SMALL_TBL = 40 * 4, 32 * 4, 8          # bytes of an extended / a cached point; multiples per small table
TAIL_THREADS, LOCATE_MIN_BATCH = 512, 2048
OUT = ("nbytes P n_lanes group n_groups locate spec grp_rows Pg Pf Pl "
       "grp_sc grp_digits grp_partials grp_ok row_map grp_fail grp_fail_sum grp_ws grp_wf grp_dyn rechk_pts "
       "accept accept2 bitmap pinned status digits st_partials dynsum "
       "dyn_rows window_sums window_flags msm_fail small_tbl recoded").split()
SIZES = OUT[11:]
BATCHES = (1, 2, 15, 16, 17, 197, 2047, 2048, 2049, 10240, 15360)
WINDOWS = tuple(255 // w + 1 for w in (8, 9, 10, 14, 16))
NS, DYN_PER_ROW = 2 + 2 * 256, 27                  # a 2x2 cloak statement: generator terms, proof-specific points


@pytest.fixture(scope="module")
def plan():
    from zkvm_amd import build
    build.build()
    lib = C.CDLL(os.path.join(ROOT, "zkvm_amd", "lib", "libzkhost.so"))
    lib.zkhost_pipe_plan.restype = None
    lib.zkhost_pipe_plan.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * len(OUT))()

    def call(B, W, prep, gs, locate_mode, locate_parts, forced_parts, reasons, n_dyn=None, n_static=None):
        n_dyn = DYN_PER_ROW * B if n_dyn is None else n_dyn
        n_static = NS * B if n_static is None else n_static
        lib.zkhost_pipe_plan((C.c_int64 * 11)(B, n_dyn, n_static, W, prep, NS if prep else 0, gs, locate_mode, locate_parts, forced_parts, reasons), out)
        return dict(zip(OUT, out))
    return call


def _model(B, W, prep, gs, locate_mode, locate_parts, forced_parts, reasons, n_dyn=None, n_static=None):
    n_dyn = DYN_PER_ROW * B if n_dyn is None else n_dyn
    n_static = NS * B if n_static is None else n_static
    ns = NS if prep else 0
    m = {"nbytes": (B + 7) // 8}
    # enough lanes to fill the chip (131 072), at most 16 per (row, window); a forced number as it is
    m["P"] = forced_parts if forced_parts > 0 else max(1, min(16, -(-131072 // (B * W))))
    m["n_lanes"] = B * W * m["P"]
    m["group"] = min(gs, B) if (prep and gs > 1) else 1
    m["n_groups"] = -(-B // m["group"])
    grouped = m["group"] > 1
    m["locate"] = int(grouped and (locate_mode >= 2 or (locate_mode == 0 and B >= LOCATE_MIN_BATCH)))
    m["spec"] = int(m["locate"] and locate_mode == 3)
    m["grp_rows"] = m["n_groups"] * (2 if m["spec"] else 1)
    m["Pg"] = max(1, min(32, -(-65536 // (m["grp_rows"] * W)))) if grouped else 1
    m["Pf"] = 32
    m["Pl"] = locate_parts if locate_parts > 0 else 32
    rows, groups = m["grp_rows"], m["n_groups"]
    located_apart = m["locate"] and not m["spec"]
    per_row = max(W * max(m["Pg"], m["Pl"] if located_apart else 0), TAIL_THREADS)
    g = {"grp_sc": rows * ns * 32, "grp_digits": rows * ns * W * 2, "grp_partials": rows * per_row * EXT, "grp_ok": groups,
         "row_map": 4 * B, "grp_fail": 12 * groups, "grp_fail_sum": groups * EXT, "grp_ws": groups * 64 * EXT, "grp_wf": groups * 64 * 4,
         "grp_dyn": groups * EXT, "rechk_pts": B * EXT}
    m.update(g if grouped else dict.fromkeys(g, 0))
    # room for the rows' own lanes: B x W x P swings with the rounding of P (2047 x 32 x 3 > 2048 x 32 x 2), its bound
    # min(16 B W, 131 071 + B W) does not; a forced number of parts as it is
    own_room = m["n_lanes"] if forced_parts > 0 else min(16 * B * W, 131071 + B * W)
    m.update(accept=B, accept2=B, bitmap=m["nbytes"], pinned=m["nbytes"] + 64 + (B if reasons else 0), status=64,
             digits=max(n_static, 1) * W * 2, dynsum=B * EXT,
             st_partials=max(own_room, B * max(W * m["Pf"], TAIL_THREADS) if grouped else 0) * EXT,
             dyn_rows=max(n_dyn, 1) * NIELS, window_sums=B * 64 * EXT, window_flags=B * 64 * 4, msm_fail=4 * B,
             small_tbl=max(n_dyn, 1) * SMALL_TBL * EXT, recoded=max(n_dyn, 1) * 32)
    return m


def _grid():
    return itertools.product(BATCHES, WINDOWS, (1, 0), (1, 3, 16, 64), (0, 1, 2, 3), (0, 1, 5, 64), (0, 1, 16), (0, 1))


def test_the_plan_is_the_model_over_the_grid_and_seeded_shapes(plan):
    n = 0
    for args in _grid():
        assert plan(*args) == _model(*args), args
        n += 1
    assert n == 11 * 5 * 2 * 4 * 4 * 4 * 3 * 2
    rng = random.Random(2718)
    for _ in range(2000):
        B = rng.choice([rng.randrange(1, 40), rng.randrange(1, 5000), rng.randrange(1, 1 << 20)])
        args = (B, rng.choice(WINDOWS + (64, 128)), rng.randrange(2), rng.choice([1, 2, 7, 16, 64, 1000]), rng.randrange(4),
                rng.choice([0, 1, 3, 32, 64]), rng.choice([0, 1, 2, 16]), rng.randrange(2))
        kw = {"n_dyn": rng.randrange(0, 128 * B + 1), "n_static": rng.randrange(0, 600 * B)}
        assert plan(*args, **kw) == _model(*args, **kw), (args, kw)


def test_every_buffer_a_launch_writes_covers_that_launch(plan):
    """lanes of the launches that write grp_partials and st_partials (zkgpu.hip, pipe_enqueue): the group sums (grp_rows x W x
    Pg), the locating sums when they are a launch of their own (n_groups x W x Pl), k_locate_fused (TAIL_THREADS shares per
    group); the rows' own sums (B x W x P), the re-check of the queued rows unfused (B x W x Pf) and fused (TAIL_THREADS
    shares per row)"""
    for args in _grid():
        p = plan(*args)
        B, W = args[0], args[1]
        assert p["st_partials"] >= B * W * p["P"] * EXT, args
        if p["group"] > 1:
            located_apart = p["locate"] and not p["spec"]
            assert p["grp_partials"] >= p["grp_rows"] * W * max(p["Pg"], p["Pl"] if located_apart else 0) * EXT, args
            assert p["grp_partials"] >= p["grp_rows"] * TAIL_THREADS * EXT, args
            assert p["st_partials"] >= B * max(W * p["Pf"], TAIL_THREADS) * EXT, args
            assert p["grp_digits"] >= p["grp_rows"] * NS * W * 2 and p["grp_fail"] >= 3 * 4 * p["n_groups"], args
        else:
            assert all(p[k] == 0 for k in SIZES[:11]), args
        assert p["pinned"] >= p["bitmap"] + 48 and p["status"] >= 48, args       # the results tail copies 48 status bytes


@pytest.fixture(scope="module")
def shrinking(plan):
    """{buffer: [(smaller batch, larger batch, the other arguments, bytes, bytes)]} wherever a larger batch of the grid is
    planned FEWER bytes of a buffer than the batch before it"""
    found = {}
    for rest in itertools.product(WINDOWS, (1, 0), (1, 3, 16, 64), (0, 1, 2, 3), (0, 1, 5, 64), (0, 1, 16), (0, 1)):
        prev = None
        for B in BATCHES:
            p = plan(B, *rest)
            for k in SIZES if prev else ():
                if p[k] < prev[k]:
                    found.setdefault(k, []).append((prev_B, B, rest, prev[k], p[k]))
            prev, prev_B = p, B
    return found


@pytest.mark.parametrize("buffer", SIZES)
def test_sizes_are_monotone_in_the_batch(shrinking, buffer):
    """More rows never need less room, whatever the knobs, over the batches of the grid (the locate threshold, 2048, sits
    inside it): a workspace reserved for a batch fits every smaller one.  (st_partials is why the plan keeps
    static_lanes_room and not the lanes themselves: with P = ceil(131 072 / (B x W)) parts, 2047 rows of 32 windows are
    196 512 lanes and 2048 rows 131 072.)"""
    assert buffer not in shrinking, shrinking[buffer][:3]
