"""The plan of one device prover call (zkvm_amd/csrc/prover_call_plan.hpp through libzkhost's zkhost_prover_call_plan and
zkvm_amd.native.prover_call_plan): the constant blob, the input area, the rows of the multiscalar multiplications and their
scaffolding, the bytes of every workspace buffer and the steps -- held against what prove_device did before it walked a plan,
restated here in Python from that code as read (never by calling the library): an 8-bit range statement (single phase), a
shuffle of two (multipliers only in phase 2), a system without commitments (m = 0) and the 2-in/2-out cloak, at batches of
1, 5 and 9 (the odd ones put the 16-byte alignment of the scaffolding to work).  No GPU."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_util import GADGET_LABEL, K_OUT, describe_range, describe_shuffle, gadget_witness  # noqa: E402

GIVEN = 0xFFFFFFFF
EXT = 40 * 4                                   # bytes of a point as the kernels store it
FILL_LANES = 131072
ALL_STEPS = [("phase0", 0, 0), ("msm", 0, 0),
             ("lanes", 1, 1), ("wg", 1, 2), ("lanes", 1, 4), ("wg", 1, 8), ("rng", 1, 0), ("msm", 1, 0),
             ("lanes", 2, 1), ("wg", 2, 2), ("lanes", 2, 4), ("wg", 2, 8), ("rng", 2, 0), ("msm", 2, 0),
             ("lanes", 3, 1), ("wg", 3, 2), ("lanes", 3, 4), ("msm", 3, 0),
             ("lanes", 4, 1), ("wg", 4, 2), ("ipa", 0, 0), ("finish", 0, 0)]
SINGLE_PHASE = [s for s in ALL_STEPS if s not in (("wg", 2, 2), ("lanes", 2, 4), ("wg", 2, 8), ("rng", 2, 0))]
# name -> (description or None for the cloak, mult_def, generators, the steps as a literal list)
SHAPES = {
    "range 8": (describe_range(8), None, 8, SINGLE_PHASE),
    "shuffle 2": (describe_shuffle(2), gadget_witness(2, 2, [0] * 4)[0], 2, ALL_STEPS),
    "no commitments": ((0, 1, 1, [], [[(K_OUT, 0, 1, -1, 0)]]), None, 1, [s for s in SINGLE_PHASE if s != ("msm", 0, 0)]),
    "cloak 2x2": (None, None, 256, ALL_STEPS),
}
BATCHES = (1, 5, 9)


@pytest.fixture(scope="module")
def plan_of():
    from zkvm_amd import build
    from zkvm_amd.native import R1csDescription, prover_call_plan
    build.build()
    descs = {name: R1csDescription(GADGET_LABEL, *s[0]) for name, s in SHAPES.items() if s[0] is not None}

    def plan(name, batch, W=8, seeded=False, blindings=True):
        _, mult_def, cap, _ = SHAPES[name]
        if name in descs:
            return prover_call_plan(batch, W, cap, desc=descs[name], mult_def=mult_def, seeded=seeded, blindings=blindings)
        return prover_call_plan(batch, W, cap, cloak=(2, 2), seeded=seeded, blindings=blindings)
    return plan


# ---- prove_device before the plan, restated ----------------------------------------------------------------------------------
def rows_pairs(rows):
    return [2 * i for i in range(rows + 1)], [0, 1] * rows


def rows_commit(batch, first, last, cap, empty_when_none):
    offsets, index, cnt = [0], [], last - first
    g, h = [2 + first + j for j in range(cnt)], [2 + cap + first + j for j in range(cnt)]
    for _ in range(batch):
        if cnt == 0 and empty_when_none:
            offsets += [offsets[-1]] * 3
            continue
        for row in ([1] + g + h, [1] + g, [1] + g + h):            # A_I, A_O, S
            index += row
            offsets.append(offsets[-1] + len(row))
    return offsets, index


def parts(rows, W):
    return max(1, min(64, (FILL_LANES + rows * W - 1) // (rows * W))) if rows else None


def expected(sh, batch, W):
    m, n1, n, pn, cap = sh["m"], sh["n1"], sh["n"], sh["pn"], sh["gens_capacity"]
    b_val, b_giv = batch * m * 32, batch * sh["n_given"] * 64
    e = {"in": {"values": 0, "blindings": b_val, "given": 2 * b_val, "seeds": 2 * b_val + b_giv, "bytes": 2 * b_val + b_giv + batch * 32 + 64}}
    row_len, n_ipa_rows = pn + 1, 2 * batch
    lays = [rows_pairs(batch * m), rows_commit(batch, 0, n1, cap, False), rows_commit(batch, n1, n, cap, True), rows_pairs(batch * 5)]
    rows = [batch * m, 3 * batch, 3 * batch, 5 * batch, n_ipa_rows]
    terms = [2 * batch * m, batch * sh["r1_terms"], batch * sh["r2_terms"], 10 * batch, n_ipa_rows * row_len]
    for i in range(4):
        assert (len(lays[i][0]), len(lays[i][1])) == (rows[i] + 1, terms[i])
    lay = bytearray()

    def place(data):
        at = len(lay)
        lay.extend(data)
        lay.extend(bytes(-len(lay) % 16))
        return at
    e["msm"] = []
    for i in range(5):
        offsets = lays[i][0] if i < 4 else [r * row_len for r in range(n_ipa_rows + 1)]
        o_off = place(b"".join(v.to_bytes(8, "little") for v in offsets))
        o_idx = place(b"".join(v.to_bytes(4, "little") for v in lays[i][1])) if i < 4 else 0
        e["msm"].append({"rows": rows[i], "terms": terms[i], "P": parts(rows[i], W), "kinds": 3 if i in (1, 2) else 1, "o_off": o_off, "o_idx": o_idx})
    e["lay"] = bytes(lay)
    vec = pn * 32
    e["ws"] = {"pv_state": batch * sh["state_words"] * 4, "pv_rows0": max(batch * m, 1) * 64, "pv_rows1": batch * sh["r1_terms"] * 32,
               "pv_rows2": max(batch * sh["r2_terms"], 1) * 32, "pv_rows3": batch * 5 * 64, "pv_pts": max(batch * 5, batch * m) * 32 + 64,
               "pv_com": max(batch * m, 1) * 32, "pv_ab": batch * 64, "pv_proofs": batch * sh["proof_stride"],
               "ipa_lv": batch * vec, "ipa_rv": batch * vec, "ipa_cg": batch * vec, "ipa_ch": batch * vec, "ipa_w": batch * 32, "ipa_u": batch * 64,
               "in_st_scalars": n_ipa_rows * row_len * 32, "in_st_index": n_ipa_rows * row_len * 4, "status": 64,
               # the buffers msm_ps_dev used to re-ensure at each of the call's 4 + k multiplications: the largest of them
               "digits": max(max(t, 1) * W * 2 for t in terms), "rechk_pts": max(rows) * EXT}
    # lanes each multiplication writes, and the room for them that never shrinks as the batch grows (rows * W * P swings, as
    # pipe_plan.hpp's static_lanes_room documents for the verifier: P is a rounded-up quotient)
    e["st_partials_need"] = max(r * W * parts(r, W) for r in rows if r) * EXT
    e["ws"]["st_partials"] = max(min(64 * r * W, FILL_LANES - 1 + r * W) for r in rows) * EXT
    return e


def test_described_shapes_are_the_ones_restated(plan_of):
    """the shape a plan is made for (pv_build, not part of the plan) where the description gives it away"""
    for name, (d, mult_def, cap, _) in SHAPES.items():
        sh = plan_of(name, 5)["shape"]
        if d is None:
            assert (sh["m"], sh["pn"], sh["k"], sh["gens_capacity"]) == (8, 256, 8, 256) and sh["n"] > sh["n1"] > 0
            continue
        m, n1, n = d[:3]
        pn = 1
        while pn < n:
            pn *= 2
        k = pn.bit_length() - 1
        n_given = n if mult_def is None else sum(1 for i in range(n) if GIVEN in mult_def[2 * i: 2 * i + 2])
        assert sh == dict(sh, m=m, n1=n1, n=n, pn=pn, k=k, n_given=n_given, r1_terms=3 + 5 * n1, r2_terms=3 + 5 * (n - n1) if n > n1 else 0,
                          proof_stride=(1 + 32 * (16 + 2 * k) + 15) & ~15, gens_capacity=cap), name


@pytest.mark.parametrize("name", list(SHAPES))
def test_inputs_rows_scaffolding_and_workspace(plan_of, name):
    for batch in BATCHES:
        for W in (8, 19):
            p = plan_of(name, batch, W)
            e = expected(p["shape"], batch, W)
            assert p["in"] == e["in"], (batch, W)
            assert p["ipa_row_len"] == p["shape"]["pn"] + 1
            for i in range(5):
                want = dict(e["msm"][i])
                if want["P"] is None:                                   # no rows: never launched (steps), any P will do
                    want["P"] = p["msm"][i]["P"]
                assert p["msm"][i] == want, (batch, W, i)
                assert p["msm"][i]["o_off"] % 16 == 0 and p["msm"][i]["o_idx"] % 16 == 0
            assert p["lay_bytes"] == len(e["lay"]) and p["lay"] == e["lay"], (batch, W)
            assert p["ws"] == e["ws"], (batch, W)
            assert p["ws"]["st_partials"] >= e["st_partials_need"]


@pytest.mark.parametrize("name", list(SHAPES))
def test_steps_are_the_literal_list(plan_of, name):
    for batch in BATCHES:
        assert plan_of(name, batch)["steps"] == SHAPES[name][3]
    stages = [s for s in ALL_STEPS if s[0] in ("lanes", "wg")]
    assert len(stages) == len(set(stages)) == 13                       # the instantiations of k_pv_lanes / k_pv_wg there are


def words(b):
    b += bytes(-len(b) % 4)
    return [int.from_bytes(b[i: i + 4], "little") for i in range(0, len(b), 4)]


def draw_table(entries):
    """prover_draw.hpp: tag || LE64(index) || 0x1F in five words, three words of zero"""
    out = []
    for tag, index in entries:
        out += words((tag + index.to_bytes(8, "little") + b"\x1f").ljust(20, b"\0")) + [0, 0, 0]
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_blob_tables_padding_key_and_draw_table(plan_of, name):
    from zkvm_amd.native import PV_PLAN_TABLES
    d, mult_def, cap, _ = SHAPES[name]
    plain, seeded = plan_of(name, 5), plan_of(name, 5, seeded=True, blindings=False)
    sh, at, blob = plain["shape"], plain["at"], plain["blob"]
    order = [at[t] for t in PV_PLAN_TABLES[:-1]]
    assert order[0] == 0 and order[1] == 52 and order == sorted(order) and all(o % 4 == 0 for o in order)      # init: 52 words
    key = [sh["m"], sh["n1"], sh["n"], sh["pn"], sh["gens_capacity"], 0, 0, 0]
    assert blob[-8:] == key and at["draw"] == 0
    labels = d[3] if d is not None else None
    if labels is not None:
        lab = b"".join(bytes([len(s)]) + s.ljust(31, b"\0") for s in labels) or bytes(32)
        assert blob[at["chal_labels"]:-8] == words(lab), "the label block, then the key"
        # the tables a description gives away: constraint offsets, kinds and indices of the terms, the multipliers' definitions
        cons = d[4]
        nt = sum(len(c) for c in cons)

        def table(t, count):
            nxt = order[order.index(at[t]) + 1]
            assert nxt - at[t] == (count + 3) & ~3 and blob[at[t] + count: nxt] == [0] * (nxt - at[t] - count), t
            return blob[at[t]: at[t] + count]
        assert table("con_off", len(cons) + 1) == [sum(len(c) for c in cons[:i]) for i in range(len(cons) + 1)]
        assert table("t_kind", nt) == [t[0] for c in cons for t in c] and table("t_idx", nt) == [t[1] for c in cons for t in c]
        table("t_mono", nt), table("t_coef", 8 * nt)
        md = mult_def if mult_def is not None else [GIVEN] * (2 * sh["n"])
        assert table("mult_def", 2 * sh["n"]) == md
        slots, given = [], 0
        for i in range(sh["n"]):
            is_given = GIVEN in md[2 * i: 2 * i + 2]
            slots.append(given if is_given else GIVEN)
            given += is_given
        assert table("given_slot", sh["n"]) == slots
    # a call that drew its seed: the same tables, the draw table of m + 1 entries between the labels and the key
    m = sh["m"]
    entries = [(b"blinding", j) for j in range(m)] if d is not None else [(t, j) for j in range(m // 2) for t in (b"q_blinding", b"f_blinding")]
    table_words = draw_table(entries + [(b"rng", 0)])
    assert len(table_words) == 8 * (m + 1)
    assert seeded["at"] == dict(at, draw=len(blob) - 8)
    assert seeded["blob"] == blob[:-8] + table_words + key
    assert plan_of(name, 9)["blob"] == blob, "the blob does not depend on the batch"


@pytest.mark.parametrize("name", list(SHAPES))
def test_blindings_brought_change_only_the_draw_flag(plan_of, name):
    for batch in BATCHES:
        brought, drawn = plan_of(name, batch, seeded=True, blindings=True), plan_of(name, batch, seeded=True, blindings=False)
        assert (brought["draw_blindings"], drawn["draw_blindings"]) == (False, True)
        assert dict(brought, draw_blindings=True) == drawn
        for blindings in (True, False):
            assert plan_of(name, batch, blindings=blindings)["draw_blindings"] is False      # no seed of the call's own: nothing is drawn


@pytest.mark.parametrize("name", list(SHAPES))
def test_a_plan_fits_inside_the_plan_of_every_larger_batch(plan_of, name):
    """every size is monotone in the batch, 1 .. 64, at 8 and 19 windows -- st_partials because the plan reserves room, not
    rows * W * P (at 19 windows that product shrinks from 22 to 23 statements: 110 rows x 19 x 63 lanes > 115 x 19 x 60)"""
    assert 110 * 19 * parts(110, 19) == 131670 > 115 * 19 * parts(115, 19) == 131100
    for W in (8, 19):
        last = None
        for batch in range(1, 65):
            p = plan_of(name, batch, W)
            sizes = dict(p["ws"], pv_in=p["in"]["bytes"], pv_lay=p["lay_bytes"], pv_plan=len(p["blob"]))
            if last is not None:
                assert all(sizes[k] >= last[k] for k in sizes), (W, batch, [k for k in sizes if sizes[k] < last[k]])
            last = sizes


def test_stand_alone_check_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tools/prover_call_plan_check.cpp: a program of its own (no Python in the process) plans the shapes and batches above,
    fills the scaffolding into a heap buffer of exactly lay_bytes and reads every table of the view over a blob of exactly its
    words"""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    r = subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtime: " + r.stderr.strip()[-300:])
    exe = tmp_path / "prover_call_plan_check"
    subprocess.run([cxx] + flags + [os.path.join(ROOT, "tools", "prover_call_plan_check.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok:") and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
