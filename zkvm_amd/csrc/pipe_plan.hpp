// pipe_plan.hpp -- what the verification pipeline of ONE device batch (pipe_enqueue, zkgpu.hip) settles before its first
// launch: the geometry of its generator sums and group checks, and the bytes of every workspace buffer a launch of it writes.
// The synchronous tables path and the grouped mixed call size their sums and their small-window block by the same helpers.
// No HIP here: pipe_enqueue and the CPU tests (libzkhost, zkhost_pipe_plan) run the same function.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace zk {

// words of a point as the kernels store it and multiples per point of the small tables: zkgpu.hip holds them against
// kernels.hpp's EXT_WORDS, NIELS_WORDS and SMALL_TBL
constexpr int PLAN_EXT_WORDS = 40, PLAN_NIELS_WORDS = 32, PLAN_SMALL_TBL = 8;
constexpr int TAIL_THREADS = 512;              // threads per row in k_recheck_fused (shares of the row's generator sum)
constexpr size_t LOCATE_MIN_BATCH = 2048;      // transactions per batch from which failed groups are located instead of re-checked in full

// lanes per (row, window) of k_static_accumulate over B rows of their own: enough lanes to fill the chip, 16 at most
constexpr uint64_t FILL_LANES = 131072, MAX_PARTS = 16;
inline int static_parts(uint64_t B, int W, int forced) {
  return forced > 0 ? forced : (int)std::max<uint64_t>(1, std::min<uint64_t>(MAX_PARTS, (FILL_LANES + B * W - 1) / (B * W)));
}
// room for those lanes that never shrinks as B grows (a workspace reserved for a batch must fit every smaller one): the parts are a
// rounded-up quotient, and B * W * parts itself swings (2047 rows of 32 windows: 3 parts, 196 512 lanes; 2048 rows: 2 parts, 131 072)
inline uint64_t static_lanes_room(uint64_t B, int W, int forced) {
  return forced > 0 ? B * W * forced : std::min<uint64_t>(MAX_PARTS * B * W, FILL_LANES - 1 + B * W);
}
// ... over `rows` rows whose values are wanted one by one (zkgpu_msm_ps_batch, the device prover's multiplications): 64 at
// most, and the room for them that never shrinks as the rows grow
constexpr uint64_t MAX_ROW_PARTS = 64;
inline int row_parts(uint64_t rows, int W) {
  const uint64_t cells = std::max<uint64_t>(rows * W, 1);
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(MAX_ROW_PARTS, (FILL_LANES + cells - 1) / cells));
}
inline uint64_t row_lanes_room(uint64_t rows, int W) { return std::min<uint64_t>(MAX_ROW_PARTS * rows * W, FILL_LANES - 1 + rows * W); }
// ... over the rows of group checks (few checks each: short chains of additions per lane keep their latency down)
inline int group_parts(uint64_t rows, int W) { return (int)std::max<uint64_t>(1, std::min<uint64_t>(32, (65536 + rows * W - 1) / (rows * W))); }

// the small-window block: decoded proof points, window sums and flags of B rows of 64 four-bit windows, the rows' decode
// failures, the per-point tables and the recoded scalars
struct SmallWindowBytes { size_t dyn_rows, window_sums, window_flags, msm_fail, small_tbl, recoded; };
inline SmallWindowBytes small_window_bytes(uint64_t B, uint64_t n_dyn) {
  const uint64_t pts = std::max<uint64_t>(n_dyn, 1), ext = PLAN_EXT_WORDS * 4;
  return {(size_t)(pts * PLAN_NIELS_WORDS * 4), (size_t)(B * 64 * ext), (size_t)(B * 64 * 4), (size_t)(B * 4), (size_t)(pts * PLAN_SMALL_TBL * ext),
          (size_t)(pts * 32)};
}

// rows, proof-specific terms, generator terms | windows of the generator tables | the rows come from proofs prepared on the
// device (group checks: only then), with ns generator terms per statement
struct PipeShape { uint64_t n_msm, n_dyn, n_static; int W; bool whole_proof; uint32_t ns; };
struct PipeKnobs { int group_size, locate_mode, locate_parts, forced_parts; bool want_reasons; };

struct PipePlan {
  size_t nbytes;                     // of the accept bitmap
  int P; uint64_t n_lanes;           // lanes per (row, window) of the rows' own generator sums: n_lanes = B * W * P
  uint32_t group, n_groups;          // transactions per group check (1: none), group checks
  bool locate, spec;                 // a failed group's culprit is located | by sums formed beside the group sums
  uint32_t grp_rows;                 // rows of the group launch: the groups, twice when spec
  int Pg, Pf, Pl;                    // lanes per (row, window): group launch, individual re-check, locating multiplication
  // bytes per workspace buffer (the grp_* and rechk_pts: 0 without group checks)
  size_t grp_sc, grp_digits, grp_partials, grp_ok, row_map, grp_fail, grp_fail_sum, grp_ws, grp_wf, grp_dyn, rechk_pts;
  size_t accept, accept2, bitmap, pinned, status, digits, st_partials, dynsum;
  SmallWindowBytes small;
};

inline PipePlan plan_pipe(const PipeShape& sh, const PipeKnobs& k) {
  PipePlan p = {};
  const size_t B = (size_t)sh.n_msm, ext = (size_t)PLAN_EXT_WORDS * 4;
  const int W = sh.W;
  p.nbytes = (B + 7) / 8;
  p.P = static_parts(B, W, k.forced_parts);
  p.n_lanes = (uint64_t)B * W * p.P;
  // group checks (k_group_combine): only for whole proofs (the weights come from k_transcript)
  p.group = (sh.whole_proof && k.group_size > 1) ? (uint32_t)std::min<size_t>((size_t)k.group_size, B) : 1;
  p.n_groups = (uint32_t)((B + p.group - 1) / p.group);
  // locating the culprit of a failed group saves work (one multiscalar multiplication instead of `group`) at the
  // price of two more dependent stages: worth it once the batch is large enough for the work to matter.  Mode 3 forms the
  // locating sums of ALL groups beside the group sums (twice the rows in the same multiplication), so that a failed group's
  // culprit is named by k_group_combine itself: no extra stage, ~3 % more point arithmetic per batch.
  p.locate = p.group > 1 && (k.locate_mode >= 2 || (k.locate_mode == 0 && B >= LOCATE_MIN_BATCH));
  p.spec = p.locate && k.locate_mode == 3;
  p.grp_rows = p.spec ? 2 * p.n_groups : p.n_groups;
  p.Pg = 1; p.Pf = 32;
  // the locating multiplication runs for the failed groups only, on the tail of the batch: many short chains (its grid is
  // sized for every group failing; lanes beyond the device-side count leave at once)
  p.Pl = k.locate_parts > 0 ? k.locate_parts : 32;
  if (p.group > 1) {
    const size_t rows = p.grp_rows, ns = sh.ns, groups = p.n_groups;
    p.Pg = group_parts(rows, W);
    p.grp_sc = rows * ns * 32; p.grp_digits = rows * ns * W * 2;
    // written by the group launch (W * Pg lanes per row), by the unfused locating launch (W * Pl) and by k_locate_fused
    // (TAIL_THREADS shares per row)
    p.grp_partials = rows * std::max<size_t>((size_t)W * std::max(p.Pg, p.locate && !p.spec ? p.Pl : 0), TAIL_THREADS) * ext;
    p.grp_ok = groups; p.grp_fail = groups * 12; p.grp_fail_sum = p.grp_dyn = groups * ext;
    p.grp_ws = groups * 64 * ext; p.grp_wf = groups * 64 * 4;
    p.row_map = B * 4; p.rechk_pts = B * ext;
  }
  p.accept = p.accept2 = B; p.bitmap = p.nbytes; p.status = 64;
  p.pinned = p.nbytes + 64 + (k.want_reasons ? B : 0);
  p.digits = (size_t)(std::max<uint64_t>(sh.n_static, 1) * W * 2);
  // written by the rows' own sums (n_lanes, within static_lanes_room), and with group checks by the re-check of the queued
  // rows: W * Pf lanes per row unfused, TAIL_THREADS shares per row in k_recheck_fused
  p.st_partials = (size_t)(std::max<uint64_t>(static_lanes_room(B, W, k.forced_parts), p.group > 1 ? (uint64_t)B * std::max(W * p.Pf, TAIL_THREADS) : 0) * ext);
  p.dynsum = B * ext;
  p.small = small_window_bytes(B, sh.n_dyn);
  return p;
}

}  // namespace zk
