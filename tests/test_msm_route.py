"""Which form of the multiscalar multiplication a call takes (zkvm_amd/csrc/msm_route.hpp through libzkhost.so,
zkhost_msm_route): the function run_to_windows and the batch entry points of zkgpu.hip call before their first launch --
against a model of the rules written here, on the CPU, over a grid that holds every threshold and both its neighbours; then,
directly, that every workspace buffer is at least as large as the launches that write it need."""
import ctypes as C
import itertools
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT, NIELS, DEC = 40 * 4, 32 * 4, 64 * 4            # bytes of an extended point, a decoded row, a decoder scratch row
DIRECT, BATCH, TABLES = 0, 1, 2
UNKNOWN = -1                                        # longest row not known (offsets in device memory): ~0 as the library sees it
OUT = ("small parts w n_windows n_buckets chunk_size chunks n_terms n_wins n_bins n_tasks max_entries too_large "
       "part_sort quad_reduce window_partials split_decode scan_blocks fat_cap fat_blocks hi_bits n_part n_tiles "
       "dyn_rows bins block_sums entries buckets partials partial_flags window_sums window_flags msm_fail heavy class_count "
       "bin_order dec_scratch part_hist part_block_sums part_entries").split()
ROWS = (1, 2, 4, 5, 63, 64, 65, 256, 257, 877, 878, 1024, 1025, 1228, 1229, 2048, 2049, 3000)
WIDTHS = (0, 2, 3, 4, 8, 9, 10, 16)


def _terms(B):
    """the thresholds in the number of proof-specific terms, each with both neighbours"""
    at = [1, B, 64 * B, 128 * B, 32768, 131072, 1 << 23]
    return sorted({0} | {v + d for v in at for d in (-1, 0, 1) if v + d >= 0})


@pytest.fixture(scope="module")
def route():
    from zkvm_amd import build
    build.build()
    lib = C.CDLL(os.path.join(ROOT, "zkvm_amd", "lib", "libzkhost.so"))
    lib.zkhost_msm_route.restype = None
    lib.zkhost_msm_route.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * len(OUT))()

    def call(B, n_dyn, n_static, longest, forced_w, entry):
        lib.zkhost_msm_route((C.c_int64 * 6)(B, n_dyn, n_static, longest, forced_w, entry), out)
        return dict(zip(OUT, out))
    return call


def _choose_window(n_terms, B):
    """the width with the fewest point additions: windows x (terms per row + two per bucket, 1.3 times that once a window is
    reduced in chunks); the narrowest on a tie"""
    per = n_terms / max(B, 1)
    best, best_cost = 4, 1e300
    for w in range(4, 17):
        half = 1 << (w - 1)
        cost = float(255 // w + 1) * (per + 2.0 * half * (1.3 if half > 64 else 1.0))
        if cost < best_cost:
            best, best_cost = w, cost
    return best


def _model(B, n_dyn, n_static, longest, forced_w, entry):
    m = dict.fromkeys(OUT, 0)
    longest = longest if longest >= 0 else (1 << 64) - 1
    if entry == BATCH:
        m["small"] = int(not forced_w and n_static == 0 and 0 < n_dyn <= 64 * B and B >= 64 and longest <= 256)
    elif entry == TABLES:
        m["small"] = int(not forced_w and n_dyn <= 128 * B)
    if m["small"]:
        # wavefronts per row: 4 up to 877 rows, 3 up to 1228, 2 up to 2048, then 1
        m.update(parts=4 if B <= 877 else 3 if B <= 1228 else 2 if B <= 2048 else 1, w=4, n_windows=64)
        return m
    if entry == TABLES:
        n_static = 0                                 # summed out of the tables: no part of the pipeline
    n = n_dyn + n_static
    w = max(2, min(16, forced_w or _choose_window(n, B)))
    W, half = 255 // w + 1, 1 << (w - 1)
    chunk = half if half <= 64 else 16
    chunks = -(-half // chunk)
    m.update(w=w, n_windows=W, n_buckets=half, chunk_size=chunk, chunks=chunks, n_terms=n, n_wins=B * W, n_bins=B * W * half,
             n_tasks=B * W * chunks, max_entries=n * W)
    m["too_large"] = int(n * W >= 1 << 32 or B * W * half >= 1 << 32 or n_dyn >= 1 << 30 or n_static >= 1 << 32)
    if m["too_large"]:
        return m
    m["part_sort"] = int(B == 1 and n_static == 0 and w >= 9 and 32768 <= n <= 1 << 23)
    m["quad_reduce"] = int(m["n_tasks"] <= 65536)
    m["window_partials"] = int(chunks > 1)
    m["split_decode"] = int(n_dyn >= 131072)
    m["scan_blocks"] = -(-m["n_bins"] // 2048)
    m["fat_cap"] = n * W // 96 + 64
    m["fat_blocks"] = min(-(-m["fat_cap"] * 16 // 256), 320)
    m.update(dyn_rows=max(n_dyn, 1) * NIELS, bins=4 * (m["n_bins"] + 1), block_sums=4 * (m["scan_blocks"] + 1), entries=4 * max(n * W, 1),
             buckets=m["n_bins"] * EXT, partials=m["n_tasks"] * EXT, partial_flags=4 * m["n_tasks"], window_sums=B * W * EXT,
             window_flags=4 * B * W, msm_fail=4 * B, heavy=4 * (65536 + 1 + m["fat_cap"] + 1), class_count=4 * 2 * 256,
             bin_order=4 * m["n_bins"], dec_scratch=n_dyn * DEC if m["split_decode"] else 0)
    if m["part_sort"]:
        m.update(hi_bits=w - 9, n_part=W << (w - 9), n_tiles=-(-n // 2048))
        m.update(part_hist=4 * m["n_part"] * m["n_tiles"], part_block_sums=4 * (2 * m["n_part"] + 4), part_entries=m["entries"])
    return m


def _grid():
    for B in ROWS:
        for args in itertools.product(_terms(B), (0, 1, 1000), (0, 256, 257, UNKNOWN), WIDTHS, (DIRECT, BATCH, TABLES)):
            yield (B,) + args
    for n_dyn, w in (((1 << 25) - 1, 2), (1 << 25, 2), ((1 << 30) - 1, 16), (1 << 30, 16), (1 << 29, 0)):      # past 32-bit entry indices
        yield (1, n_dyn, 0, UNKNOWN, w, DIRECT)
    yield (1 << 17, 1 << 20, 0, UNKNOWN, 16, DIRECT)                                                          # ... bin indices


@pytest.fixture(scope="module")
def planned(route):
    return [(args, route(*args)) for args in _grid()]


def test_the_route_is_the_model_over_every_threshold(planned):
    seen = {k: set() for k in ("small", "parts", "part_sort", "quad_reduce", "window_partials", "split_decode", "too_large", "w")}
    for args, got in planned:
        assert got == _model(*args), args
        for k in seen:
            seen[k].add(got[k])
    assert seen["parts"] == {0, 1, 2, 3, 4} and seen["w"] >= {2, 3, 4, 8, 9, 10, 16}
    assert all(seen[k] == {0, 1} for k in seen if k not in ("parts", "w"))


def test_each_threshold_sits_where_the_table_says(route):
    """the pairs the GPU tests straddle, spelled out"""
    def r(B, n_dyn, longest=1, w=0, entry=BATCH, n_static=0):
        return route(B, n_dyn, n_static, longest, w, entry)
    assert [r(B, 2 * B)["small"] for B in (63, 64)] == [0, 1]
    assert [r(64, 640, longest=m)["small"] for m in (256, 257, UNKNOWN)] == [1, 0, 0]
    assert [r(64, n)["small"] for n in (0, 64 * 64, 64 * 64 + 1)] == [0, 1, 0]
    assert r(64, 128, w=4)["small"] == 0 and r(64, 128, n_static=1)["small"] == 0
    assert [r(4, n, entry=TABLES, n_static=99)["small"] for n in (512, 513)] == [1, 0]
    assert r(4, 512, entry=TABLES, w=7)["small"] == 0 and r(4, 513, entry=TABLES, n_static=99)["n_terms"] == 513
    assert [r(B, 64)["parts"] for B in (64, 877, 878, 1228, 1229, 2048, 2049, 3000)] == [4, 4, 3, 3, 2, 2, 1, 1]
    for w in (9, 10, 16):
        assert [r(1, n, w=w, entry=DIRECT)["part_sort"] for n in (32767, 32768, 32769, 1 << 23, (1 << 23) + 1)] == [0, 1, 1, 1, 0]
    assert r(1, 40000, w=8, entry=DIRECT)["part_sort"] == 0 and r(2, 40000, w=9, entry=DIRECT)["part_sort"] == 0
    assert [(p["n_tasks"], p["quad_reduce"]) for p in (r(B, 2 * B, w=4) for B in (1024, 1025))] == [(65536, 1), (65600, 0)]
    assert [(p["n_tasks"], p["quad_reduce"]) for p in (r(B, 2 * B, w=8) for B in (256, 257))] == [(65536, 1), (65792, 0)]
    assert [(r(1, 100, w=w, entry=DIRECT)["chunks"], r(1, 100, w=w, entry=DIRECT)["window_partials"]) for w in (7, 8, 16)] == [(1, 0), (8, 1), (2048, 1)]
    assert [r(1, n, entry=DIRECT)["split_decode"] for n in (131071, 131072)] == [0, 1]
    assert [r(1, 100, w=w, entry=DIRECT)["w"] for w in (1, 2, 3, 16, 17)] == [2, 2, 3, 16, 16]


def test_every_buffer_covers_the_launches_that_write_it(planned):
    """run_to_windows (zkgpu.hip): what each launch writes, from its grid and its guards, against the bytes planned"""
    n = 0
    for args, p in planned:
        if p["small"] or p["too_large"]:
            continue
        n += 1
        B, n_dyn = args[0], args[1]
        terms, W, half = p["n_terms"], p["n_windows"], p["n_buckets"]
        bins = B * W * half
        assert p["n_bins"] == bins and p["n_wins"] == B * W
        assert p["dyn_rows"] >= n_dyn * NIELS and p["msm_fail"] >= 4 * B                      # the decoder: a row per point, a word per row
        if p["split_decode"]:
            assert p["dec_scratch"] >= n_dyn * DEC
        # the bin counters are cleared one past the last bin; the scan writes a sum per tile of 2048 bins and a word per bin
        assert p["bins"] >= 4 * (bins + 1) and p["scan_blocks"] * 2048 >= bins and p["block_sums"] >= 4 * p["scan_blocks"]
        assert p["entries"] >= 4 * terms * W                                                  # an entry per non-zero digit at most
        assert p["buckets"] >= bins * EXT and p["bin_order"] >= 4 * bins and p["class_count"] >= 4 * 2 * 256
        # a bin enters the fat list above 96 entries (so at most entries // 97 bins do), the heavy list holds 65536
        assert p["fat_cap"] * 97 > terms * W and p["heavy"] >= 4 * (65536 + 1 + p["fat_cap"] + 1) and p["fat_blocks"] <= 320
        # the reduce launch writes a point and a flag per task: into the window sums when a window is one chunk
        assert p["chunk_size"] * p["chunks"] >= half and p["chunk_size"] * (p["chunks"] - 1) < half
        assert p["n_tasks"] == B * W * p["chunks"] and bool(p["window_partials"]) == (p["chunks"] > 1)
        into, flags = ("partials", "partial_flags") if p["chunks"] > 1 else ("window_sums", "window_flags")
        assert p[into] >= p["n_tasks"] * EXT and p[flags] >= 4 * p["n_tasks"]
        assert p["window_sums"] >= B * W * EXT and p["window_flags"] >= 4 * B * W             # k_window_partials: a workgroup per window
        if p["part_sort"]:
            # a cell per (partition, tile); totals, bases (one more) and the ticket in block_sums; the partitions' 256 low
            # bins each are exactly the bins; an entry's term index has 23 bits; the partition counters fit the LDS
            assert p["n_tiles"] * 2048 >= terms and p["part_hist"] >= 4 * p["n_part"] * p["n_tiles"]
            assert p["part_block_sums"] >= 4 * (2 * p["n_part"] + 2) and p["part_entries"] >= 4 * terms * W
            assert p["n_part"] * 256 == bins and terms <= 1 << 23 and 4 * p["n_part"] <= 65536
    assert n > 20000
