"""Every route of the multiscalar multiplication at its thresholds, with the edge scalars and points of tests/msm_corpus.py.
Results are 32-byte encodings (or accept bits on the tables path) compared for equality with the CPU oracle; which route a
call took is read from the library's record (zkgpu_debug_read "msm_routes") and held against numbers written out here,
never against the library's own route function (that one has its CPU test: tests/test_msm_route.py)."""
import pytest

import msm_corpus as mc
from gpu_util import L, bits, points, scalars

pytestmark = pytest.mark.gpu
COUNTERS = ("small", "bucket", "part_sort", "count_scatter", "quad_reduce", "lane_reduce", "window_partials", "tables_small", "tables_bucket")


@pytest.fixture(scope="module")
def ctx():
    from zkvm_amd import Context
    c = Context(0)
    yield c
    c.set_window_bits(0)
    c.close()


def routed(ctx, call, forced_w=0):
    """-> (what call() returned, by how much each counter of the route record moved, the record after)"""
    before = ctx.msm_routes()
    ctx.set_window_bits(forced_w)
    try:
        out = call()
    finally:
        ctx.set_window_bits(0)
    after = ctx.msm_routes()
    return out, {k: after[k] - before[k] for k in COUNTERS}, after


def moved(**kw):
    return {**dict.fromkeys(COUNTERS, 0), **kw}


_MEMO = {}


def want_row(oracle, sc: bytes, pt: bytes) -> bytes:
    """the oracle's value of one row (rows repeat across the cases: computed once each)"""
    if (sc, pt) not in _MEMO:
        rc, enc, _ = oracle.msm(sc, pt)
        assert rc == 0
        _MEMO[sc, pt] = enc
    return _MEMO[sc, pt]


def batch_of(rows):
    """rows [(scalars, points)] -> (scalars, points, offsets)"""
    offs = [0]
    for sc, _ in rows:
        offs.append(offs[-1] + len(sc) // 32)
    return b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), offs


def values(ctx, rows):
    sc, pt, offs = batch_of(rows)
    out, ok = ctx.msm_batch(sc, pt, offs)
    assert bits(ok, len(rows)) == [1] * len(rows)
    return [out[32 * i: 32 * i + 32] for i in range(len(rows))]


def cycled_rows(oracle, lengths):
    """rows of the given lengths whose scalars cycle through the 4-bit corpus (the wrap range s >= 0x77..78 included) and
    whose points cycle through the edge points"""
    e = mc.edge_points(oracle)
    sc = [v for _, v in mc.all_scalars(4)]
    pts = [e["p"], e["identity"], e["base"], e["neg_p"], e["p"]] + e["uniform"]
    rows, k = [], 0
    for n in lengths:
        rows.append((mc.sc_bytes(sc[(k + i) % len(sc)] for i in range(n)), b"".join(pts[(k + 2 * i) % len(pts)] for i in range(n))))
        k += n + 1
    return rows


# ---- a. every window width of the bucket pipeline ---------------------------------------------------------------------------
@pytest.mark.parametrize("w", mc.WIDTHS)
def test_width_sweep_single_and_batch(ctx, oracle, w):
    """w = 2 .. 16 (128 .. 16 windows): the corpus of that width as one multiplication, then a forced-width batch of six rows by
    value.  A window is reduced in chunks of 16 buckets from 2^(w-1) > 64 on: k_window_partials from w = 8.  The single call
    has 16 x 2048 = 32 768 reduce tasks at most (quad form); the batch 6 x 19 x 512 = 58 368 at w = 14 (quad) and
    6 x 18 x 1024 = 110 592 at w = 15 (one lane each)."""
    e = mc.edge_points(oracle)
    sc, pt = mc.corpus_row(oracle, w)
    got, d, after = routed(ctx, lambda: ctx.msm(sc, pt), w)
    assert got == want_row(oracle, sc, pt)
    assert d == moved(bucket=1, count_scatter=1, quad_reduce=1, window_partials=1 if w >= 8 else 0) and after["bucket_w"] == w
    k = mc.sc_bytes([dict(mc.width_scalars(w))["every window half+1"]])
    rows = [(b"", b""), (k, e["uniform"][1]), (k + k, e["p"] + e["neg_p"]), (bytes(32 * 5), e["p"] * 2 + e["base"] + e["uniform"][0] * 2),
            (sc, pt), (scalars("sweep70", 70), points(oracle, "sweep70", 70, distinct=9))]
    got, d, after = routed(ctx, lambda: values(ctx, rows), w)
    assert got == [want_row(oracle, *r) for r in rows]
    assert got[0] == got[2] == got[3] == bytes(32)
    lane = 1 if w >= 15 else 0
    assert d == moved(bucket=1, count_scatter=1, quad_reduce=1 - lane, lane_reduce=lane, window_partials=1 if w >= 8 else 0)
    assert after["bucket_w"] == w and ctx.last_window_bits() == w


# ---- b. the partition sort's lower threshold ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sort_inputs(oracle):
    """32 769 terms over 16 distinct points, shared by the cases: uniform scalars, tile 3 (terms 6144 .. 8191) all zero"""
    n = 32769
    sc = bytearray(scalars("partsort", n))
    sc[32 * 6144: 32 * 8192] = bytes(32 * 2048)
    return sc, bytearray(points(oracle, "partsort", n, distinct=16))


@pytest.mark.parametrize("w", (9, 10, 16))
@pytest.mark.parametrize("n", (32767, 32768, 32769))
def test_partition_sort_threshold(ctx, oracle, sort_inputs, n, w):
    """a single multiplication of 32 768 terms and more at w >= 9 is sorted by partitions (w = 9: no high bucket bits, 10: one,
    16: seven), one term fewer by count / scan / scatter.  The corpus sits in the first and in the last tile of 2048 terms."""
    csc, cpt = mc.corpus_row(oracle, w)
    m = len(csc) // 32
    sc, pt = bytearray(sort_inputs[0][: 32 * n]), bytearray(sort_inputs[1][: 32 * n])
    sc[: 32 * m], pt[: 32 * m] = csc, cpt
    sc[32 * (n - m):], pt[32 * (n - m):] = csc, cpt
    sc, pt = bytes(sc), bytes(pt)
    got, d, after = routed(ctx, lambda: ctx.msm(sc, pt), w)
    assert got == want_row(oracle, sc, pt)
    sort = 1 if n >= 32768 else 0
    assert d == moved(bucket=1, part_sort=sort, count_scatter=1 - sort, quad_reduce=1, window_partials=1) and after["bucket_w"] == w


# ---- c. the two reduce forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,B,lane", [(4, 1024, 0), (4, 1025, 1), (8, 256, 0), (8, 257, 1)])
def test_reduce_form_threshold_by_value(ctx, oracle, w, B, lane):
    """65 536 reduce tasks take a quad of lanes each, 65 537 and more one lane: rows of two terms at w = 4 (64 windows of one
    chunk: 64 tasks a row) and at w = 8 (32 windows of 8 chunks: 256 a row, chunks past the first add lo x the running sum)."""
    e = mc.edge_points(oracle)
    sc = [v for _, v in mc.all_scalars(w)]
    rnd, pts = scalars("reduce", 37), [e["p"], e["base"], e["identity"]] + e["uniform"]
    rows = [(mc.sc_bytes([sc[i % len(sc)]]) + rnd[32 * (i % 37): 32 * (i % 37) + 32], pts[i % 7] + pts[(i // 7 + 3) % 7]) for i in range(B)]
    got, d, after = routed(ctx, lambda: values(ctx, rows), w)
    assert got == [want_row(oracle, *r) for r in rows]
    assert d == moved(bucket=1, count_scatter=1, quad_reduce=1 - lane, lane_reduce=lane, window_partials=1 if w == 8 else 0)


# ---- d. the per-point tables ---------------------------------------------------------------------------------------------------
def small_lengths(B, longest=256):
    return [longest if i == 7 else (0, 1, 2, 3, 5)[i % 5] for i in range(B)]


@pytest.mark.parametrize("B,parts", [(64, 4), (877, 4), (878, 3), (1228, 3), (1229, 2), (2048, 2), (2049, 1), (3000, 1)])
def test_small_path_parts_and_wrap_scalars(ctx, oracle, B, parts):
    """64 rows and more of a few terms each: one workgroup of 4 / 3 / 2 / 1 wavefronts per row.  Rows of 0, 1, 2, 3 and 5 terms
    (shorter than the parts) and one of 256; scalars through the whole 4-bit corpus: zero, every digit zero, -8 or +7, and the
    range s >= 0x77..78 whose recoded form wraps and leaves +8 in the top window."""
    rows = cycled_rows(oracle, small_lengths(B))
    got, d, after = routed(ctx, lambda: values(ctx, rows))
    assert got == [want_row(oracle, *r) for r in rows]
    assert d == moved(small=1) and after["small_parts"] == parts and ctx.last_window_bits() == 4


def test_small_path_boundaries_rows_longest_row_and_terms(ctx, oracle):
    """each pair: one side per-point tables, the other the bucket pipeline (width 4 chosen for a few terms a row, 5 for 64 a row:
    one chunk per window either way), equal values"""
    bucket4 = moved(bucket=1, count_scatter=1, quad_reduce=1)
    # 63 rows | 64 rows
    rows = cycled_rows(oracle, small_lengths(64))
    want = [want_row(oracle, *r) for r in rows]
    got63, d63, after63 = routed(ctx, lambda: values(ctx, rows[:63]))
    got64, d64, _ = routed(ctx, lambda: values(ctx, rows))
    assert got63 == want[:63] and got64 == want
    assert d63 == bucket4 and after63["bucket_w"] == 4 and d64 == moved(small=1)
    # the longest row 256 | 257
    longer = cycled_rows(oracle, small_lengths(64, longest=257))
    got, d, after = routed(ctx, lambda: values(ctx, longer))
    assert got == [want_row(oracle, *r) for r in longer] and d == bucket4 and after["bucket_w"] == 4
    assert got[:7] == want[:7]
    # 64 terms a row | one term more
    full = cycled_rows(oracle, [64] * 64)
    over = full[:63] + cycled_rows(oracle, [64] * 63 + [65])[63:]
    got_full, d_full, _ = routed(ctx, lambda: values(ctx, full))
    got_over, d_over, after = routed(ctx, lambda: values(ctx, over))
    assert got_full == [want_row(oracle, *r) for r in full] and got_over == [want_row(oracle, *r) for r in over]
    assert got_full[:63] == got_over[:63]
    assert d_full == moved(small=1) and d_over == bucket4 and after["bucket_w"] == 5


# ---- e. the proof-specific half of a batch over a point set with tables ---------------------------------------------------------
@pytest.mark.parametrize("table_bits", (5, 16))
def test_tables_path_small_and_bucket_dyn(ctx, oracle, table_bits):
    """four rows over twelve generators with tables: 512 proof-specific terms take the per-point tables, 513 the bucket pipeline
    (width 6 for 128 terms a row), 512 with a forced width as well.  Every row sums to the identity by construction (its last
    term cancels the rest) but row 2, whose last scalar is off by one.  Corpus scalars on both sides: 2^255 - 1 and
    2^255 - 19 reach the generator digits (at 16 bits a top digit of exactly +32768)."""
    from zkvm_amd import PointSet
    n_gen = 12
    gens = points(oracle, "route gens", n_gen)
    corpus = [v for _, v in mc.all_scalars(table_bits)]

    def build(dyn_counts):
        dyn, st_sc, st_idx, st_off, flat = [], b"", [], [0], []
        for i, nd in enumerate(dyn_counts):
            ks = [corpus[(5 * i + j) % len(corpus)] for j in range(n_gen)]
            idx = [(j + i) % n_gen for j in range(n_gen)]
            sc, pt = cycled_rows(oracle, [3] * i + [nd - 1])[-1] if i else mc.corpus_row(oracle, table_bits, rounds=4)
            sc, pt = sc[: 32 * (nd - 1)], pt[: 32 * (nd - 1)]
            assert len(sc) == 32 * (nd - 1)
            g_sc, g_pt = mc.sc_bytes(ks), b"".join(gens[32 * j: 32 * j + 32] for j in idx)
            total = want_row(oracle, g_sc + sc, g_pt + pt)
            sc += ((L - 1) if i != 2 else (L - 2)).to_bytes(32, "little")
            pt += total
            dyn.append((sc, pt))
            st_sc += g_sc
            st_idx += idx
            st_off.append(st_off[-1] + n_gen)
            flat.append((g_sc + sc, g_pt + pt))
        return batch_of(dyn), (st_sc, st_off, st_idx), batch_of(flat)

    plain, tabled = PointSet(ctx, gens), PointSet(ctx, gens)
    try:
        tabled.build_tables(table_bits)
        for counts, forced, expect in (((128, 128, 128, 128), 0, moved(small=1, tables_small=1)),
                                       ((128, 128, 129, 128), 0, moved(bucket=1, count_scatter=1, quad_reduce=1, tables_bucket=1)),
                                       ((128, 128, 128, 128), 9, moved(bucket=1, count_scatter=1, quad_reduce=1, window_partials=1, tables_bucket=1))):
            (d_sc, d_pt, d_off), (st_sc, st_off, st_idx), (f_sc, f_pt, f_off) = build(counts)
            want = oracle.verify_batch(f_sc, f_pt, f_off)
            assert bits(want, 4) == [1, 1, 0, 1]
            got, d, after = routed(ctx, lambda: ctx.verify_batch_ps(tabled, d_sc, d_pt, d_off, st_sc, st_off, static_index=st_idx), forced)
            assert got == want and d == expect, (counts, forced)
            if expect["bucket"]:
                assert after["bucket_w"] == (forced or 6)
            assert ctx.verify_batch_ps(plain, d_sc, d_pt, d_off, st_sc, st_off, static_index=st_idx) == want
            assert ctx.verify_batch(f_sc, f_pt, f_off) == want
    finally:
        plain.close()
        tabled.close()


# ---- f. fat and heavy bins inside a batch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", (0, 8))
def test_fat_and_heavy_bins_with_a_row_offset(ctx, oracle, w):
    """five rows through the bucket pipeline; row 1 holds 97 terms of one scalar on ONE point (bins of 97 entries: sixteen lanes
    each, and every addition a doubling), row 3 holds 2049 terms of one scalar (bins of 2049: a workgroup each).  Their bin
    indices carry the rows' offsets.  Width 7 is the library's choice for 454 terms a row."""
    e = mc.edge_points(oracle)
    k = (0x1f3e5d7c9b0a1122334455667788990011223344556677889900aabbccddeeff % L).to_bytes(32, "little")
    rows = [(scalars("bins0", 10), points(oracle, "bins0", 10)), (k * 97, e["uniform"][2] * 97), mc.corpus_row(oracle, w or 7),
            (k * 2049, points(oracle, "bins3", 2049, distinct=16)), (scalars("bins4", 3), e["p"] + e["neg_p"] + e["identity"])]
    got, d, after = routed(ctx, lambda: values(ctx, rows), w)
    assert got == [want_row(oracle, *r) for r in rows]
    assert d == moved(bucket=1, count_scatter=1, quad_reduce=1, window_partials=1 if w == 8 else 0) and after["bucket_w"] == (w or 7)
    assert after["fat"] >= 1 and after["heavy"] >= 1
    # one entry fewer on either list's threshold: 2048 entries are still a fat bin, 96 still one lane's
    for n, fat in ((2048, True), (96, False)):
        below = [rows[0], (k * n, points(oracle, "bins3", n, distinct=16)), rows[4]]
        got, _, after = routed(ctx, lambda: values(ctx, below), w)
        assert got == [want_row(oracle, *r) for r in below], n
        assert (after["fat"] >= 1) == fat and after["heavy"] == 0, (n, after)
