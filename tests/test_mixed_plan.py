"""The host's plan of a zkgpu_r1cs_verify_mixed call (zkvm_amd/csrc/mixed_plan.hpp through libzkhost.so, zkhost_mixed_plan):
the distinct plans, the order the statements are worked in, the lane order of the one-lane transcript, the MixStmt offsets,
the checks, and the per-call table the k_mx_* kernels index blindly -- against a model written here, on the CPU.

Plans of the cases (`INFOS`): all three LDS classes (one plan at exactly MIX_LDS_SMALL, one past it, one `large`), three
generator keys (padded n 8 and 64 under one capacity, padded n 8 under another), one plan without the cooperative
transcript (n_seg = 0), one with n_ch > 0xffff, one with more proof points than the pipeline takes, and one handle at two
positions of the list."""
import ctypes as C
import os
import random
import struct
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX_LDS_SMALL = 80 * 1024
TWO_PHASE, ONE_PHASE, BAD_LENGTH = 0, 1, 2
PAD = 0xFFFFFFFF
REC = 256                          # stands for sizeof(PrepPlan)
ERR_INDEX = "mixed verification: plan index out of range"
ERR_OFFSETS = "mixed verification: proof offsets decrease"

Info = namedtuple("Info", "id proof_words m n_ch n_ch_ext n_seg n_dyn n_static pn h_base n_targets lds_bytes large lp_slots")
Case = namedtuple("Case", "plans idx offs coop_wanted gs may_group")
SUMMARY = ("n_uniq cs0 cs1 cs2 cs3 class_lds0 class_lds1 lp_targets lp_pn lp_slots coop max_nch n_com n_pw n_ch n_raw n_abs n_dyn n_st "
           "n_checks n_grouped n_rows max_ns n_pairs n_lanes t_plans t_stmts t_order t_lanes t_doff t_soff t_grp t_mem t_goff t_end").split()


def _info(ident, k, m, n_chal2, pn, h_base, n_seg, lds, large=False, n_dyn=None, n_ch=None):
    n_ch = 14 + n_chal2 + 2 * k if n_ch is None else n_ch
    return Info(0x7F0000001000 + 0x340 * ident, (16 + 2 * k) * 8, m, n_ch, n_ch + 3 * n_chal2 + 56, n_seg, 11 + m + 2 * k if n_dyn is None else n_dyn,
                2 + 2 * pn, pn, h_base, 10 + 37 * ident, lds, int(large), 400 + 211 * ident)


SMALL_A, SMALL_B, ALONE, LARGE, NO_COOP, WIDE_CH, MANY_POINTS = (
    _info(0, 3, 1, 0, 8, 514, 9, 40000), _info(1, 3, 2, 2, 8, 514, 11, MIX_LDS_SMALL), _info(2, 6, 4, 0, 64, 514, 14, MIX_LDS_SMALL + 1),
    _info(3, 6, 9, 1, 64, 514, 21, 300000, large=True), _info(4, 3, 1, 0, 8, 258, 0, 30000), _info(5, 3, 1, 0, 8, 514, 9, 40000, n_ch=0x10000),
    _info(6, 3, 1, 0, 8, 514, 9, 40000, n_dyn=300))
INFOS = [SMALL_A, LARGE, SMALL_B, ALONE, SMALL_A, NO_COOP]        # (SMALL_A's handle twice; the large plan before smaller ones)


@pytest.fixture(scope="module")
def host():
    from zkvm_amd import build
    build.build()
    lib = C.CDLL(os.path.join(ROOT, "zkvm_amd", "lib", "libzkhost.so"))
    lib.zkhost_mixed_plan.restype = C.c_longlong
    lib.zkhost_mixed_plan.argtypes = [C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_size_t, C.c_int,
                                      C.c_uint32, C.c_int, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                      C.c_char_p, C.c_size_t]
    return lib


def _full_len(info):
    return 1 + 4 * info.proof_words


def _offsets(plans, idx, lengths=None):
    offs = [0]
    for i, p in enumerate(idx):
        offs.append(offs[-1] + (_full_len(plans[p]) if lengths is None else lengths[i]))
    return offs


def _cases():
    """batches 1, 2, 63, 64, 65, 130 x group sizes 1, 2, 16 x may_group x three seeded plan-index vectors: over the five list
    positions with the cooperative transcript, over all six (NO_COOP among them), and in runs (plan by plan)"""
    out = []
    for batch in (1, 2, 63, 64, 65, 130):
        for gs in (1, 2, 16):
            for may_group in (True, False):
                for seed in range(3):
                    rng = random.Random(1000 * batch + 10 * gs + seed)
                    idx = [rng.randrange(5 if seed == 0 else 6) for _ in range(batch)]
                    if seed == 2:
                        idx.sort(key=lambda p: (p * 7) % 6)
                    lengths = [_full_len(INFOS[p]) - (96 if rng.randrange(4) == 0 else 0) for p in idx]
                    out.append(Case(INFOS, idx, _offsets(INFOS, idx, lengths), seed != 1 or batch != 64, gs, may_group))
    return out


CASES = _cases()
Plan = namedtuple("Plan", "s uniq stmts order lanes doff soff groups members goff table")


def _call(host, case):
    """-> Plan, or the error text"""
    n, batch = len(case.plans), len(case.idx)
    flat = (C.c_uint64 * (14 * n))(*[v for info in case.plans for v in info])
    idx = (C.c_uint32 * batch)(*case.idx)
    offs = (C.c_uint64 * (batch + 1))(*case.offs)
    summary, uniq, err = (C.c_uint64 * len(SUMMARY))(), (C.c_uint32 * n)(), C.create_string_buffer(128)
    args = (flat, n, idx, offs, batch, int(case.coop_wanted), case.gs, int(case.may_group), REC)
    size = host.zkhost_mixed_plan(*args, None, 0, summary, uniq, err, 128)
    if size < 0:
        return err.value.decode()
    table = C.create_string_buffer(size)
    assert host.zkhost_mixed_plan(*args, table, size, summary, uniq, err, 128) == size
    s = dict(zip(SUMMARY, summary))
    t = table.raw

    def words(fmt, at, count):
        return list(struct.unpack_from("<%d%s" % (count, fmt), t, at))
    stmts = [struct.unpack_from("<2I8Q", t, s["t_stmts"] + 72 * i) for i in range(batch)]
    groups = [struct.unpack_from("<4IQ", t, s["t_grp"] + 24 * g) for g in range(s["n_checks"])]
    return Plan(s, list(uniq)[: s["n_uniq"]], stmts, words("I", s["t_order"], batch), words("I", s["t_lanes"], s["n_lanes"]),
                words("Q", s["t_doff"], batch + 1), words("Q", s["t_soff"], batch + 1), groups,
                words("I", s["t_mem"], batch if groups else 0), words("Q", s["t_goff"], len(groups) + 1 if groups else 0), t)


@pytest.fixture(scope="module")
def planned(host):
    return [(case, _call(host, case)) for case in CASES]


# ---- the model -----------------------------------------------------------------------------------------------------------
def _cls(info):
    return 2 if info.large else 1 if info.lds_bytes > MIX_LDS_SMALL else 0


def _form(info, length):
    return TWO_PHASE if length == _full_len(info) else ONE_PHASE if length == _full_len(info) - 96 else BAD_LENGTH


def _distinct(case):
    """-> (distinct plans as list positions, by first use; per statement its distinct plan)"""
    uniq, pid = [], []
    for p in case.idx:
        ids = [case.plans[u].id for u in uniq]
        if case.plans[p].id not in ids:
            uniq.append(p)
            ids.append(case.plans[p].id)
        pid.append(ids.index(case.plans[p].id))
    return uniq, pid


def _rows_fit(batch, n_dyn, n_static):
    return n_static > 0 and 0 < n_dyn <= 128 * batch


def _model_checks(case):
    """-> [members] per check, in the table's order; [] when every statement is checked alone"""
    uniq, pid = _distinct(case)
    batch = len(case.idx)
    infos = [case.plans[u] for u in uniq]
    if not (case.may_group and case.gs > 1 and batch > 1 and
            _rows_fit(batch, sum(infos[p].n_dyn for p in pid), sum(infos[p].n_static for p in pid))):
        return []
    order = sorted(range(batch), key=lambda i: (_cls(infos[pid[i]]), pid[i], i))
    keys = []
    for i in order:
        if (infos[pid[i]].pn, infos[pid[i]].h_base) not in keys:
            keys.append((infos[pid[i]].pn, infos[pid[i]].h_base))
    checks = []
    for key in keys:
        run = [i for i in order if (infos[pid[i]].pn, infos[pid[i]].h_base) == key]
        checks += [run[k: k + case.gs] for k in range(0, len(run), case.gs)]
    return checks if any(len(c) >= 2 for c in checks) else []


def _model_table(case):
    uniq, pid = _distinct(case)
    batch = len(case.idx)
    infos = [case.plans[u] for u in uniq]
    coop = case.coop_wanted and all(i.n_seg != 0 and i.n_ch <= 0xFFFF for i in infos)
    order = sorted(range(batch), key=lambda i: (_cls(infos[pid[i]]), pid[i], i))
    lanes = []
    if not coop:
        for k, i in enumerate(order):
            lanes.append(i)
            if k + 1 == batch or pid[order[k + 1]] != pid[i]:
                lanes += [PAD] * (-len(lanes) % 64)
    stmts, doff, soff, tot = b"", [], [], dict(com=0, pw=0, ch=0, raw=0, absorb=0, dyn=0, st=0)
    for i in range(batch):
        p = infos[pid[i]]
        stmts += struct.pack("<2I8Q", pid[i], _form(p, case.offs[i + 1] - case.offs[i]), case.offs[i], tot["com"], tot["pw"], tot["ch"],
                             tot["raw"], tot["absorb"], tot["dyn"], tot["st"])
        doff.append(tot["dyn"])
        soff.append(tot["st"])
        for name, add in (("com", 8 * p.m), ("pw", p.proof_words), ("ch", 8 * p.n_ch_ext), ("raw", 16 * p.n_ch if coop else 0),
                          ("absorb", 25 * p.n_seg if coop else 0), ("dyn", p.n_dyn), ("st", p.n_static)):
            tot[name] += add
    checks = _model_checks(case)
    groups, goff, first, rows = b"", [], 0, 0
    for c in checks:
        ns = infos[pid[c[0]]].n_static
        groups += struct.pack("<4IQ", first, len(c), ns, 0, rows)
        goff.append(rows)
        first, rows = first + len(c), rows + ns

    def u32(v):
        return struct.pack("<%dI" % len(v), *v)

    def u64(v):
        return struct.pack("<%dQ" % len(v), *v)
    sections = [bytes(REC * len(uniq)), stmts, u32(order), u32(lanes), u64(doff + [tot["dyn"]]), u64(soff + [tot["st"]]), groups,
                u32([i for c in checks for i in c]), u64(goff + [rows]) if checks else b""]
    table = b""
    for sec in sections[:-1]:
        table += sec
        table += bytes(-len(table) % 256)
    return table + sections[-1]


# ---- the properties ------------------------------------------------------------------------------------------------------
def test_order(planned):
    for case, pl in planned:
        uniq, pid = _distinct(case)
        batch = len(case.idx)
        assert pl.uniq == uniq
        assert sorted(pl.order) == list(range(batch))                                            # a permutation
        key = [(_cls(case.plans[uniq[pid[i]]]), pid[i], i) for i in pl.order]
        assert key == sorted(key)                        # by (class, plan in order of first use), stable in the caller's numbering
        classes = [k[0] for k in key]
        assert [pl.s["cs0"], pl.s["cs1"], pl.s["cs2"], pl.s["cs3"]] == [0, classes.count(0), classes.count(0) + classes.count(1), batch]
        for k in (0, 1):
            assert pl.s["class_lds%d" % k] == max([case.plans[u].lds_bytes for u in uniq if _cls(case.plans[u]) == k], default=0)
        large = [case.plans[u] for u in uniq if _cls(case.plans[u]) == 2]
        assert (pl.s["lp_targets"], pl.s["lp_pn"], pl.s["lp_slots"]) == tuple(max([getattr(i, f) for i in large], default=0)
                                                                              for f in ("n_targets", "pn", "lp_slots"))


def test_lane_order(planned):
    seen = set()
    for case, pl in planned:
        _, pid = _distinct(case)
        assert bool(pl.lanes) == (not pl.s["coop"])                                              # only for the one-lane transcript
        seen.add(bool(pl.lanes))
        if not pl.lanes:
            continue
        assert [x for x in pl.lanes if x != PAD] == pl.order
        assert len(pl.lanes) % 64 == 0
        at = 0
        while at < len(pl.lanes):                        # run by run: one plan, no padding inside, padded to a multiple of 64
            plan = pid[pl.lanes[at]]
            n = 0
            while at + n < len(pl.lanes) and pl.lanes[at + n] != PAD and pid[pl.lanes[at + n]] == plan:
                n += 1
            padded = -(-n // 64) * 64
            assert n >= 1 and pl.lanes[at + n: at + padded] == [PAD] * (padded - n)
            assert at + padded == len(pl.lanes) or (pl.lanes[at + padded] != PAD and pid[pl.lanes[at + padded]] != plan)
            at += padded
    assert seen == {True, False}


def test_coop(host, planned):
    for case, pl in planned:
        present = {case.plans[p] for p in case.idx}
        assert pl.s["coop"] == int(case.coop_wanted and NO_COOP not in present)
        assert pl.s["max_nch"] == max(i.n_ch for i in present)
    idx = [0, 1, 0]
    assert _call(host, Case([SMALL_A, SMALL_B], idx, _offsets([SMALL_A, SMALL_B], idx), True, 16, True)).s["coop"] == 1
    assert _call(host, Case([SMALL_A, SMALL_B], idx, _offsets([SMALL_A, SMALL_B], idx), False, 16, True)).s["coop"] == 0
    assert _call(host, Case([SMALL_A, NO_COOP], idx, _offsets([SMALL_A, NO_COOP], idx), True, 16, True)).s["coop"] == 0
    assert _call(host, Case([SMALL_A, WIDE_CH], idx, _offsets([SMALL_A, WIDE_CH], idx), True, 16, True)).s["coop"] == 0
    assert _call(host, Case([SMALL_A, NO_COOP], [0, 0, 0], _offsets([SMALL_A], [0, 0, 0]), True, 16, True)).s["coop"] == 1      # (listed, not present)


def test_statement_offsets_are_prefix_sums(planned):
    for case, pl in planned:
        uniq, pid = _distinct(case)
        coop = pl.s["coop"]
        com = pw = ch = raw = absorb = dyn = st = 0
        for i, s in enumerate(pl.stmts):
            p = case.plans[uniq[pid[i]]]
            assert s[0] == pid[i] and s[2] == case.offs[i]
            assert s[3:] == (com, pw, ch, raw, absorb, dyn, st)
            assert (pl.doff[i], pl.soff[i]) == (dyn, st)
            com, pw, ch, dyn, st = com + 8 * p.m, pw + p.proof_words, ch + 8 * p.n_ch_ext, dyn + p.n_dyn, st + p.n_static
            if coop:
                raw, absorb = raw + 16 * p.n_ch, absorb + 25 * p.n_seg
        assert (pl.doff[-1], pl.soff[-1]) == (dyn, st)
        assert [pl.s[k] for k in ("n_com", "n_pw", "n_ch", "n_raw", "n_abs", "n_dyn", "n_st")] == [com, pw, ch, raw, absorb, dyn, st]


def test_proof_form(host, planned):
    full = _full_len(ALONE)
    lengths = [full, full - 96, full + 1, full - 1, full - 95, full - 97, 0]
    pl = _call(host, Case([ALONE], [0] * len(lengths), _offsets([ALONE], [0] * len(lengths), lengths), True, 16, True))
    assert [s[1] for s in pl.stmts] == [TWO_PHASE, ONE_PHASE, BAD_LENGTH, BAD_LENGTH, BAD_LENGTH, BAD_LENGTH, BAD_LENGTH]
    for case, pl in planned:
        assert [s[1] for s in pl.stmts] == [_form(case.plans[p], case.offs[i + 1] - case.offs[i]) for i, p in enumerate(case.idx)]


def test_checks(planned):
    n_grouped_cases = 0
    for case, pl in planned:
        uniq, pid = _distinct(case)
        batch = len(case.idx)
        if not pl.groups:
            continue
        n_grouped_cases += 1

        def key(i):
            return (case.plans[uniq[pid[i]]].pn, case.plans[uniq[pid[i]]].h_base)
        assert sorted(pl.members) == list(range(batch))                                         # the checks partition the statements
        at = 0
        for first, count, ns, pad, st in pl.groups:
            assert (first, pad) == (at, 0) and count >= 1
            at += count
        assert at == batch
        checks = [pl.members[g[0]: g[0] + g[1]] for g in pl.groups]
        for c, g in zip(checks, pl.groups):
            assert len({key(i) for i in c}) == 1                                                 # one key per check
            assert len(c) <= case.gs
            assert g[2] == 2 + 2 * key(c[0])[0]
        keys = [key(c[0]) for c in checks]
        for k in set(keys):                              # a key's checks are consecutive and only its last one is short
            where = [n for n, kk in enumerate(keys) if kk == k]
            assert where == list(range(where[0], where[-1] + 1))
            assert all(len(checks[n]) == case.gs for n in where[:-1])
        rank = {i: n for n, i in enumerate(pl.order)}
        first_of = {}
        for i in pl.order:
            first_of.setdefault(key(i), len(first_of))
        want = sorted(range(batch), key=lambda i: (first_of[key(i)], rank[i]))
        assert pl.members == want                                                                # the (class, plan) order, stably by key
        rows = 0
        for g, off in zip(pl.groups, pl.goff):
            assert g[4] == off == rows                                                           # row offsets: prefix sums of ns
            rows += g[2]
        assert pl.goff[-1] == rows == pl.s["n_rows"]
        assert pl.s["max_ns"] == max(g[2] for g in pl.groups)
        assert pl.s["n_checks"] == len(checks)
        assert (pl.s["n_pairs"], pl.s["n_grouped"]) == (sum(len(c) >= 2 for c in checks), sum(len(c) for c in checks if len(c) >= 2)) != (0, 0)
        assert checks == _model_checks(case)
    assert n_grouped_cases >= 20


def _ungrouped(pl):
    s = pl.s
    return (not pl.groups and not pl.members and not pl.goff and s["t_grp"] == s["t_mem"] == s["t_goff"] == s["t_end"] == len(pl.table) and
            (s["n_checks"], s["n_grouped"], s["n_rows"], s["max_ns"], s["n_pairs"]) == (0, 0, 0, 0, 0))


def test_no_checks(host, planned):
    for case, pl in planned:
        if case.gs == 1 or len(case.idx) == 1 or not case.may_group:
            assert _ungrouped(pl)
        else:
            assert bool(pl.groups) == bool(_model_checks(case))
    idx = [0, 0, 2, 3, 0]
    plans = [SMALL_A, LARGE, SMALL_B, ALONE]
    assert _call(host, Case(plans, idx, _offsets(plans, idx), True, 2, True)).s["n_pairs"] == 2      # (the grouped form of the five below)
    assert _ungrouped(_call(host, Case(plans, idx, _offsets(plans, idx), True, 1, True)))              # group_size 1
    assert _ungrouped(_call(host, Case(plans, idx[:1], _offsets(plans, idx[:1]), True, 2, True)))      # one statement
    assert _ungrouped(_call(host, Case(plans, idx, _offsets(plans, idx), True, 2, False)))             # may_group off
    apart = [SMALL_A, ALONE, NO_COOP]                                                                  # three keys, one statement each
    assert _ungrouped(_call(host, Case(apart, [2, 0, 1], _offsets(apart, [2, 0, 1]), True, 16, True)))
    many = [MANY_POINTS, SMALL_A]                        # 300 proof points per statement: more than 128 per row on average
    assert _ungrouped(_call(host, Case(many, [0] * 6, _offsets(many, [0] * 6), True, 16, True)))
    assert _call(host, Case(many, [0, 1, 1, 1], _offsets(many, [0, 1, 1, 1]), True, 16, True)).s["n_pairs"] == 1      # (354 points <= 128 x 4)


def test_errors(host):
    idx = [4, 0, 4, 0, 2]
    pl = _call(host, Case(INFOS, idx, _offsets(INFOS, idx), True, 16, True))
    assert pl.uniq == [4, 2] and pl.s["n_uniq"] == 2 and pl.s["t_stmts"] == 2 * REC              # a repeated handle: one plan record
    assert [s[0] for s in pl.stmts] == [0, 0, 0, 0, 1]
    assert _call(host, Case(INFOS, [0, len(INFOS), 1], _offsets(INFOS, [0, 0, 1]), True, 16, True)) == ERR_INDEX
    offs = _offsets(INFOS, [0, 1, 2])
    assert _call(host, Case(INFOS, [0, 1, 2], [offs[0], offs[1], offs[1] - 1, offs[3]], True, 16, True)) == ERR_OFFSETS
    assert _call(host, Case(INFOS, [0, 1, 9], [0, 5, 4, 9], True, 16, True)) == ERR_OFFSETS      # (found in the caller's order: statement 1 first)
    assert _call(host, Case(INFOS, [0, 9, 1], [0, 5, 9, 8], True, 16, True)) == ERR_INDEX


def test_table_bytes(planned):
    """sections in order at multiples of 256 bytes, zero between them, the plans' records left blank, MixGroup::pad zero,
    no checks sections without a check of two: byte for byte the model's table"""
    for case, pl in planned:
        s = pl.s
        assert s["t_plans"] == 0 and all(s[k] % 256 == 0 for k in SUMMARY[SUMMARY.index("t_plans"): SUMMARY.index("t_end")])
        assert pl.table == _model_table(case)
