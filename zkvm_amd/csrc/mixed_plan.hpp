// mixed_plan.hpp -- the host's plan of ONE zkgpu_r1cs_verify_mixed call: which plans it holds, the order its statements
// are worked in, the checks they are cut into, and the per-call table the k_mx_* kernels (mixed_kernels.hpp) index blindly.
//
//   table := plans | statements | order | lane order | row offsets (dynamic, static) | checks | their members | row offsets
//            of the checks                                                  (every section starts on a multiple of 256 bytes)
//   plans       one device plan record (PrepPlan, prep_kernels.hpp) per DISTINCT plan handle, by first use; left blank
//               here, the caller copies them in (they hold device pointers)
//   statements  one MixStmt per statement, in the caller's order
//   order       the statements sorted by (LDS class, plan), stably: workgroup b of a per-statement kernel takes order[b]
//   lane order  (one-lane transcript only) the same, each plan's run padded to a multiple of 64 with ~0u
//   checks      (only when some check has two or more members) MixGroup per check, members[], the checks' row offsets
//
// No HIP here: mixed_enqueue (zkgpu.hip) and the CPU tests (libzkhost, zkhost_mixed_plan) run the same function.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace zk {

// k_mx_prepare's LDS classes: a plan needing more than this takes a CU's 160 KiB LDS alone (one workgroup per CU)
constexpr size_t MIX_LDS_SMALL = 80 * 1024;

constexpr uint32_t MIX_FORM_TWO_PHASE = 0, MIX_FORM_ONE_PHASE = 1, MIX_FORM_BAD_LENGTH = 2;

struct MixStmt {
  uint32_t plan, form;         // form: MIX_FORM_*; a proof of the wrong length is never read
  uint64_t proof;              // first byte of the proof
  uint64_t com, pw, ch, raw;   // first word of its commitments, proof words, challenge slots, raw challenge bytes
  uint64_t absorb;             // first entry of its absorbed words (cooperative transcript)
  uint64_t dyn, st;            // first dynamic / static term of its row
};

// a check of a mixed call (mixed_kernels.hpp, "group checks")
struct MixGroup {
  uint32_t first, count;       // its members: members[first .. first + count), statements in the caller's numbering
  uint32_t ns, pad;            // static terms of its row: 2 + 2 pn of its key
  uint64_t st;                 // first static term of its row among the checks' rows
};

// proof bytes of a statement shape: the two-phase wire format, or the one-phase one (three points fewer)
inline uint32_t proof_form(uint32_t proof_words, uint64_t len) {
  const uint64_t two_phase = 1 + 4ull * proof_words;
  return len == two_phase ? MIX_FORM_TWO_PHASE : len + 96 == two_phase ? MIX_FORM_ONE_PHASE : MIX_FORM_BAD_LENGTH;
}

// rows the multiscalar-multiplication pipeline takes (pipe_eligible, zkgpu.hip): some of each kind, and no more
// proof-specific points than its small-table stage has room for
inline bool pipe_rows_fit(uint64_t n_msm, uint64_t n_dyn, uint64_t n_static) {
  return n_static && n_dyn && n_dyn <= 128ull * n_msm;
}

// what the planning reads of a zkgpu_cloak_plan
struct MixPlanInfo {
  uint64_t id;                 // the handle's address: one handle at two positions of `plans` is one plan
  uint32_t proof_words, m, n_ch, n_ch_ext, n_seg, n_dyn, n_static, pn, h_base, n_targets;
  size_t lds_bytes;
  bool large;                  // past a CU's LDS: prepared by large_prep.hpp
  uint32_t lp_slots;           // large_prep.hpp's workspace slots per statement (lp_layout)
};

struct MixPlanOptions {
  bool coop_wanted;            // the cooperative transcript, if every plan of the call has it
  uint32_t group_size;         // members per check at most
  bool may_group;              // the point set has generator tables at the width the pipeline uses
};

struct MixCallPlan {
  const char* error = nullptr;               // an argument error: nothing below is set
  std::vector<uint32_t> uniq;                // the distinct plans by first use: indices into the caller's infos
  uint32_t class_start[4] = {0, 0, 0, 0};    // order[class_start[k] .. class_start[k + 1]): the statements of LDS class k
  size_t class_lds[2] = {0, 0};              // the largest LDS of classes 0 and 1
  uint32_t lp_targets = 0, lp_pn = 0, lp_slots = 0;      // the large plans' widest grids and workspace per statement
  bool coop = false;
  size_t max_nch = 0, n_lanes = 0;           // largest n_ch of the call; entries of the lane order
  uint64_t n_com = 0, n_pw = 0, n_ch = 0, n_raw = 0, n_abs = 0, n_dyn = 0, n_st = 0;      // totals over the statements
  // the checks (all zero: every statement is checked alone, and the table has no checks sections)
  uint32_t n_checks = 0, n_grouped = 0, n_pairs = 0, max_ns = 0;      // n_grouped statements in n_pairs checks of two or more
  uint64_t n_rows = 0;                       // static terms over the checks' rows
  size_t t_plans = 0, t_stmts = 0, t_order = 0, t_lanes = 0, t_doff = 0, t_soff = 0, t_grp = 0, t_mem = 0, t_goff = 0, t_end = 0;
  std::vector<char> tab;                     // t_end bytes
};

// Statement i belongs to infos[plan_index[i]] and its proof is bytes [proof_offsets[i], proof_offsets[i + 1]).
// plan_record_bytes: sizeof(PrepPlan).  batch >= 1.
inline MixCallPlan plan_mixed_call(const MixPlanInfo* infos, size_t n_infos, const uint32_t* plan_index, const uint64_t* proof_offsets,
                                   size_t batch, const MixPlanOptions& opt, size_t plan_record_bytes) {
  MixCallPlan out;
  for (size_t i = 0; i < batch; ++i) {
    if (plan_index[i] >= n_infos) { out.error = "mixed verification: plan index out of range"; return out; }
    if (proof_offsets[i + 1] < proof_offsets[i]) { out.error = "mixed verification: proof offsets decrease"; return out; }
  }
  const uint32_t B = (uint32_t)batch;
  // distinct plans (by handle) and the statements sorted by plan
  std::vector<uint32_t>& uniq = out.uniq;
  std::vector<uint32_t> pid_of(n_infos, ~0u), pid(B);
  for (uint32_t i = 0; i < B; ++i) {
    uint32_t& slot = pid_of[plan_index[i]];
    if (slot == ~0u) {
      const uint64_t id = infos[plan_index[i]].id;
      for (uint32_t u = 0; u < uniq.size() && slot == ~0u; ++u) if (infos[uniq[u]].id == id) slot = u;
      if (slot == ~0u) { slot = (uint32_t)uniq.size(); uniq.push_back(plan_index[i]); }
    }
    pid[i] = slot;
  }
  const uint32_t U = (uint32_t)uniq.size();
  auto info = [&](uint32_t u) -> const MixPlanInfo& { return infos[uniq[u]]; };
  // LDS classes of k_mx_prepare: plans that leave room for two or more workgroups per CU, and those that take one alone.
  // Statements are ordered by (class, plan); k_mx_prepare runs once per class present, each launch with its own class's
  // largest LDS, so that one large program in a call does not cut every small statement to one workgroup per CU.
  // Class 2: plans past a CU's LDS, prepared by large_prep.hpp's four launches, however many such plans the call holds.
  std::vector<uint32_t> count(U, 0), order(B), cls(U), by_class(U);
  for (uint32_t u = 0; u < U; ++u) { cls[u] = info(u).large ? 2u : info(u).lds_bytes > MIX_LDS_SMALL ? 1u : 0u; by_class[u] = u; }
  std::stable_sort(by_class.begin(), by_class.end(), [&](uint32_t a, uint32_t b) { return cls[a] < cls[b]; });
  for (uint32_t i = 0; i < B; ++i) ++count[pid[i]];
  out.class_start[3] = B;
  {
    std::vector<uint32_t> at(U, 0);
    uint32_t run = 0;
    for (uint32_t u : by_class) {
      at[u] = run;
      run += count[u];
      for (uint32_t k = cls[u] + 1; k < 3; ++k) out.class_start[k] = run;
      if (cls[u] < 2) {
        out.class_lds[cls[u]] = std::max(out.class_lds[cls[u]], info(u).lds_bytes);
      } else {
        out.lp_targets = std::max(out.lp_targets, info(u).n_targets);
        out.lp_pn = std::max(out.lp_pn, info(u).pn);
        out.lp_slots = std::max(out.lp_slots, info(u).lp_slots);
      }
    }
    for (uint32_t i = 0; i < B; ++i) order[at[pid[i]]++] = i;
  }
  out.coop = opt.coop_wanted;
  for (uint32_t u = 0; u < U; ++u) out.coop &= info(u).n_seg != 0 && info(u).n_ch <= 0xffffu;
  std::vector<uint32_t> lane_order;
  if (!out.coop) {                       // each plan's run padded to whole wavefronts
    lane_order.reserve(B + 64 * U);
    for (uint32_t i = 0; i < B; ++i) {
      lane_order.push_back(order[i]);
      if (i + 1 == B || pid[order[i + 1]] != pid[order[i]])
        while (lane_order.size() % 64) lane_order.push_back(~0u);
    }
  }
  out.n_lanes = lane_order.size();
  // the checks: statements in (class, plan) order, stably by generator key, each key's run cut into checks of group_size
  uint64_t n_dyn_all = 0, n_st_all = 0;
  for (uint32_t u = 0; u < U; ++u) { n_dyn_all += (uint64_t)count[u] * info(u).n_dyn; n_st_all += (uint64_t)count[u] * info(u).n_static; }
  std::vector<MixGroup> checks;
  std::vector<uint32_t> members;
  if (opt.may_group && pipe_rows_fit(B, n_dyn_all, n_st_all) && opt.group_size > 1 && B > 1) {
    std::vector<std::pair<uint32_t, uint32_t>> keys;      // (padded n, index of H_0)
    std::vector<uint32_t> key_of(U);
    for (uint32_t u : by_class) {
      const std::pair<uint32_t, uint32_t> k(info(u).pn, info(u).h_base);
      size_t at = std::find(keys.begin(), keys.end(), k) - keys.begin();
      if (at == keys.size()) keys.push_back(k);
      key_of[u] = (uint32_t)at;
    }
    members = order;
    std::stable_sort(members.begin(), members.end(), [&](uint32_t a, uint32_t b) { return key_of[pid[a]] < key_of[pid[b]]; });
    const uint32_t gs = opt.group_size;
    for (uint32_t i = 0; i < B;) {
      const uint32_t key = key_of[pid[members[i]]];
      uint32_t n = 1;
      while (n < gs && i + n < B && key_of[pid[members[i + n]]] == key) ++n;
      const uint32_t ns = info(pid[members[i]]).n_static;
      checks.push_back(MixGroup{i, n, ns, 0, out.n_rows});
      out.n_rows += ns;
      out.max_ns = std::max(out.max_ns, ns);
      if (n >= 2) { out.n_grouped += n; ++out.n_pairs; }
      i += n;
    }
    if (out.n_grouped == 0) { checks.clear(); members.clear(); out.n_rows = 0; out.max_ns = 0; }
    out.n_checks = (uint32_t)checks.size();
  }
  const bool grouped = out.n_checks != 0;
  // the table, laid out as the device reads it
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  out.t_plans = 0;
  out.t_stmts = up(out.t_plans + U * plan_record_bytes);
  out.t_order = up(out.t_stmts + B * sizeof(MixStmt));
  out.t_lanes = up(out.t_order + 4 * (size_t)B);
  out.t_doff = up(out.t_lanes + 4 * lane_order.size());
  out.t_soff = up(out.t_doff + 8 * ((size_t)B + 1));
  out.t_grp = up(out.t_soff + 8 * ((size_t)B + 1));
  out.t_mem = up(out.t_grp + checks.size() * sizeof(MixGroup));
  out.t_goff = up(out.t_mem + 4 * members.size());
  out.t_end = out.t_goff + (grouped ? 8 * (checks.size() + 1) : 0);
  out.tab.assign(out.t_end, 0);
  char* tab = out.tab.data();
  if (grouped) {
    memcpy(tab + out.t_grp, checks.data(), checks.size() * sizeof(MixGroup));
    memcpy(tab + out.t_mem, members.data(), 4 * members.size());
    uint64_t* goff = (uint64_t*)(tab + out.t_goff);
    for (size_t g = 0; g < checks.size(); ++g) goff[g] = checks[g].st;
    goff[checks.size()] = out.n_rows;
  }
  for (uint32_t u = 0; u < U; ++u) out.max_nch = std::max<size_t>(out.max_nch, info(u).n_ch);
  MixStmt* ms = (MixStmt*)(tab + out.t_stmts);
  uint64_t *dyn_off = (uint64_t*)(tab + out.t_doff), *st_off = (uint64_t*)(tab + out.t_soff);
  for (uint32_t i = 0; i < B; ++i) {
    const MixPlanInfo& p = info(pid[i]);
    MixStmt& s = ms[i];
    s.plan = pid[i];
    s.form = proof_form(p.proof_words, proof_offsets[i + 1] - proof_offsets[i]);
    s.proof = proof_offsets[i];
    s.com = out.n_com; s.pw = out.n_pw; s.ch = out.n_ch; s.raw = out.n_raw; s.absorb = out.n_abs; s.dyn = out.n_dyn; s.st = out.n_st;
    dyn_off[i] = out.n_dyn; st_off[i] = out.n_st;
    out.n_com += 8ull * p.m; out.n_pw += p.proof_words; out.n_ch += 8ull * p.n_ch_ext;
    if (out.coop) { out.n_raw += 16ull * p.n_ch; out.n_abs += 25ull * p.n_seg; }
    out.n_dyn += p.n_dyn; out.n_st += p.n_static;
  }
  dyn_off[B] = out.n_dyn; st_off[B] = out.n_st;
  memcpy(tab + out.t_order, order.data(), 4 * (size_t)B);
  if (!lane_order.empty()) memcpy(tab + out.t_lanes, lane_order.data(), 4 * lane_order.size());
  return out;
}

}  // namespace zk
