// prover_call_plan.hpp -- what ONE device prover call (prove_device, zkgpu.hip) settles before its first launch: the words
// of its constant blob, the layout of its input area, the rows of its multiscalar multiplications with their scaffolding,
// the bytes of every workspace buffer a launch of it writes, and its steps in the order they are queued.
// No HIP here: prove_device walks the plan on the device, pv_emulate (hostlib.cpp, staged) walks the same steps on the host,
// and the CPU tests read the plan through zkhost_prover_call_plan.
#pragma once
#include "pipe_plan.hpp"
#include "prover_draw.hpp"
#include "prover_plan.hpp"

#include <cstring>
#include <vector>

namespace zk {

// ---- the steps of a call, written once: X(kind, phase, stage mask) -------------------------------------------------------
// msm: `phase` is the multiplication (0 value commitments, 1 / 2 A_I A_O S of the phase, 3 T_1 T_3..T_6); lanes / wg: a stage
// of a phase with one lane / one workgroup per proof (k_pv_lanes<phase, mask> / k_pv_wg<phase, mask>: prove_device
// instantiates exactly the stages listed here); rng: the TranscriptRng's draws of phase 1 / 2; ipa: the inner-product rounds
enum class PvStepKind : uint32_t { phase0, msm, lanes, wg, rng, ipa, finish };
struct PvStep { PvStepKind kind; uint32_t phase, mask; };
#define PV_CALL_STEPS(X) \
  X(phase0, 0, 0) X(msm, 0, 0) \
  X(lanes, 1, 1) X(wg, 1, 2) X(lanes, 1, 4) X(wg, 1, 8) X(rng, 1, 0) X(msm, 1, 0) \
  X(lanes, 2, 1) X(wg, 2, 2) X(lanes, 2, 4) X(wg, 2, 8) X(rng, 2, 0) X(msm, 2, 0) \
  X(lanes, 3, 1) X(wg, 3, 2) X(lanes, 3, 4) X(msm, 3, 0) \
  X(lanes, 4, 1) X(wg, 4, 2) X(ipa, 0, 0) X(finish, 0, 0)

// the steps a statement shape takes: no value commitments without values; without second-phase multipliers phase 2 is its
// transcript stage alone, and multiplication 2 still runs (three empty rows per proof: the identity, no digits)
inline std::vector<PvStep> steps_for(const PvShape& sh) {
  static constexpr PvStep all[] = {
#define X(K, PH, ST) {PvStepKind::K, PH, ST},
      PV_CALL_STEPS(X)
#undef X
  };
  std::vector<PvStep> steps;
  for (const PvStep& s : all) {
    if (s.kind == PvStepKind::msm && s.phase == 0 && sh.m == 0) continue;
    if (sh.n == sh.n1 && s.phase == 2 && (s.kind == PvStepKind::rng || s.mask > 1)) continue;
    steps.push_back(s);
  }
  return steps;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------
// seeded: the call drew its own seed (the draw table is part of the blob, k_pv_draw fills the rng seeds); cloak_tags: that
// table is the cloak's (else the described system's); blindings: the caller brought them (else a seeded call draws them too)
struct PvCallFlags { bool seeded, cloak_tags, blindings; };

// one multiscalar multiplication: rows, terms, lanes per (row, window), kinds of rows per proof (msm_ps_dev), and where the
// scaffolding holds its offsets (rows + 1 x 8 bytes) and generator indices (terms x 4 bytes)
struct PvMsm { size_t rows, terms; int P; uint32_t kinds; size_t o_off, o_idx; };
constexpr int PV_MSM_IPA = 4;      // plan.msm[4]: L_j, R_j of every proof in one round; its indices are written by k_ipa_round

// the buffers of a context a call writes, as zkgpu_ctx names them
#define PV_WORKSPACE(X) \
  X(pv_state) X(pv_rows0) X(pv_rows1) X(pv_rows2) X(pv_rows3) X(pv_pts) X(pv_com) X(pv_ab) X(pv_proofs) X(ipa_lv) X(ipa_rv) \
  X(ipa_cg) X(ipa_ch) X(ipa_w) X(ipa_u) X(in_st_scalars) X(in_st_index) X(status) X(digits) X(st_partials) X(rechk_pts)

struct PvCallPlan {
  PvShape sh;
  size_t batch;
  bool draw_blindings;               // k_pv_draw writes the blindings as well as the rng seeds
  std::vector<uint32_t> blob;        // the constant tables, each padded to four words | the draw table of a seeded call | the key
  struct {                           // where each table starts, in words (draw: 0 without a seed)
#define X(f) size_t f;
    PV_PLAN_TABLES(X)
#undef X
    size_t chal_labels, draw;
  } at;
  struct { size_t values, blindings, given, seeds, bytes; } in;      // the input area: offsets, and its bytes
  PvMsm msm[5];
  size_t ipa_row_len, lay_bytes;     // terms of an inner-product row; bytes of the scaffolding
  struct {
#define X(b) size_t b;
    PV_WORKSPACE(X)
#undef X
  } ws;
  std::vector<PvStep> steps;

  PvPlan view(const uint32_t* base) const {      // the tables where the blob lies (PvHostPlan::view: where the vectors lie)
    PvPlan p;
#define X(f) p.f = base + at.f;
    PV_PLAN_TABLES(X)
#undef X
    p.chal_labels = (const uint8_t*)(base + at.chal_labels);
    return p;
  }
  PvRows rows_of(int which) const {
    const size_t cap = sh.gens_capacity;
    return which == 0 ? pv_rows_pairs(batch * sh.m) : which == 1 ? pv_rows_commit(batch, 0, sh.n1, cap, false)
         : which == 2 ? pv_rows_commit(batch, sh.n1, sh.n, cap, true) : pv_rows_pairs(batch * 5);
  }
  // lay: lay_bytes of them.  false: the rows are not the ones the plan laid out (nothing may be launched over them)
  bool fill_scaffolding(uint8_t* lay) const {
    std::memset(lay, 0, lay_bytes);
    for (int i = 0; i < PV_MSM_IPA; ++i) {
      const PvRows r = rows_of(i);
      if (r.offsets.size() != msm[i].rows + 1 || r.index.size() != msm[i].terms) return false;
      std::memcpy(lay + msm[i].o_off, r.offsets.data(), r.offsets.size() * 8);
      if (!r.index.empty()) std::memcpy(lay + msm[i].o_idx, r.index.data(), r.index.size() * 4);
    }
    for (size_t r = 0; r <= msm[PV_MSM_IPA].rows; ++r) { const uint64_t v = r * ipa_row_len; std::memcpy(lay + msm[PV_MSM_IPA].o_off + 8 * r, &v, 8); }
    return true;
  }
};

// W: windows of the point set's tables
inline PvCallPlan plan_prover_call(const PvHostPlan& hp, size_t batch, int W, PvCallFlags flags) {
  PvCallPlan p = {};
  const PvShape& sh = p.sh = hp.sh;
  p.batch = batch;
  p.draw_blindings = flags.seeded && !flags.blindings;
  auto put = [&p](const std::vector<uint32_t>& v) {
    const size_t at = p.blob.size();
    p.blob.insert(p.blob.end(), v.begin(), v.end());
    p.blob.resize((p.blob.size() + 3) & ~(size_t)3, 0);
    return at;
  };
#define X(f) p.at.f = put(hp.f);
  PV_PLAN_TABLES(X)
#undef X
  std::vector<uint32_t> labels((hp.chal_labels.size() + 3) / 4, 0);
  std::memcpy(labels.data(), hp.chal_labels.data(), hp.chal_labels.size());
  p.at.chal_labels = put(labels);
  p.at.draw = flags.seeded ? put(flags.cloak_tags ? pv_draw_table_cloak(sh.m / 2) : pv_draw_table_desc(sh.m)) : 0;
  (void)put({sh.m, sh.n1, sh.n, sh.pn, sh.gens_capacity});   // part of the key the cached scaffolding goes by
  // inputs: values | blindings | given | seeds
  const size_t b_val = batch * sh.m * 32, b_giv = batch * (size_t)sh.n_given * 64;
  p.in = {0, b_val, 2 * b_val, 2 * b_val + b_giv, 2 * b_val + b_giv + batch * 32 + 64};
  // rows and their scaffolding, every array at a multiple of 16 bytes
  p.ipa_row_len = (size_t)sh.pn + 1;
  const size_t rows[5] = {batch * sh.m, 3 * batch, 3 * batch, 5 * batch, 2 * batch};
  const size_t terms[5] = {2 * batch * sh.m, batch * (size_t)sh.r1_terms, batch * (size_t)sh.r2_terms, 10 * batch, 2 * batch * p.ipa_row_len};
  auto place = [&p](size_t bytes) { const size_t at = p.lay_bytes; p.lay_bytes = (p.lay_bytes + bytes + 15) & ~(size_t)15; return at; };
  size_t max_rows = 0, max_terms = 1;
  uint64_t room = 0;
  for (int i = 0; i < 5; ++i) {
    PvMsm& m = p.msm[i];
    m = {rows[i], terms[i], row_parts(rows[i], W), i == 1 || i == 2 ? 3u : 1u, place((rows[i] + 1) * 8), 0};
    if (i != PV_MSM_IPA) m.o_idx = place(terms[i] * 4);
    max_rows = std::max(max_rows, m.rows); max_terms = std::max(max_terms, m.terms);
    room = std::max(room, row_lanes_room(m.rows, W));     // >= rows * W * P, and never shrinks as the batch grows
  }
  // workspace
  const size_t vec = (size_t)sh.pn * 32, ext = (size_t)PLAN_EXT_WORDS * 4;
  p.ws.pv_state = batch * (size_t)sh.state_words * 4;
  p.ws.pv_rows0 = std::max<size_t>(batch * sh.m, 1) * 64;
  p.ws.pv_rows1 = batch * (size_t)sh.r1_terms * 32;
  p.ws.pv_rows2 = std::max<size_t>(batch * (size_t)sh.r2_terms, 1) * 32;
  p.ws.pv_rows3 = batch * 5 * 64;
  p.ws.pv_pts = std::max<size_t>(batch * 5, batch * sh.m) * 32 + 64;
  p.ws.pv_com = std::max<size_t>(batch * sh.m, 1) * 32;
  p.ws.pv_ab = p.ws.ipa_u = batch * 64;
  p.ws.pv_proofs = batch * (size_t)sh.proof_stride;
  p.ws.ipa_lv = p.ws.ipa_rv = p.ws.ipa_cg = p.ws.ipa_ch = batch * vec;
  p.ws.ipa_w = batch * 32;
  p.ws.in_st_scalars = terms[PV_MSM_IPA] * 32;
  p.ws.in_st_index = terms[PV_MSM_IPA] * 4;
  p.ws.status = 64;
  // shared by the call's 4 + k multiplications: the largest of them
  p.ws.digits = max_terms * W * 2;
  p.ws.st_partials = (size_t)room * ext;
  p.ws.rechk_pts = max_rows * ext;
  p.steps = steps_for(sh);
  return p;
}

}  // namespace zk
