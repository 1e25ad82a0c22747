// mixed_kernels.hpp -- the device-side head of r1cs::Verifier::verify for a batch whose statements belong to
// DIFFERENT constraint systems (zkgpu_r1cs_verify_mixed): the per-statement stages of prep_kernels.hpp, run on a view
// (PrepStmt) made from a per-call table instead of from a by-value PrepShape, so that one launch per stage serves every plan.
//
//   PrepPlan  (prep_kernels.hpp) one per distinct plan of the call, copied from the plan as it stands
//   MixStmt   one per statement, in the CALLER's order: its plan, proof wire form, and where its inputs, its
//             challenge slots and its rows of the multiscalar multiplication live (rows have the statement's own
//             lengths: 11 + m + 2k dynamic and 2 + 2 pn static terms)
//   order     the statements sorted by plan: workgroup b of the per-statement kernels takes statement order[b]
//   lane_order  the same, each plan's run padded to a multiple of 64 with ~0u: the one-lane-per-statement
//             transcript sees one plan per wavefront (its tape loop stays uniform)
//
// Outputs are those of the homogeneous kernels at the statement's own offsets; the verdict bits, the accept
// flags and r_bytes stay indexed by the caller's position.  `grouped` (per call: some check of the call has two or more
// members, see "group checks" below) makes the transcript stages put rho = r^2 into every statement's scalars.
#pragma once
#include "prep_kernels.hpp"
#include "mixed_plan.hpp"     // MixStmt, MixGroup, MIX_FORM_*: the table as the host lays it out

namespace zk {

// a statement's view without its rows: its plan's shape and arrays
__device__ __forceinline__ PrepStmt mix_view(const PrepPlan& pln) {
  PrepStmt ps = {pln.sh, pln.mono_chal, pln.mono_pow, pln.tgt_off, pln.term_info, pln.prod_qm, pln.prod_coef};
  ps.h_base = pln.h_base;
  return ps;
}

// ---- k_mx_proof_unpack: one workgroup per statement; sets the statement's well-formedness flag (first writer)
__global__ void __launch_bounds__(256)
k_mx_proof_unpack(const PrepPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ order,
                  const uint8_t* __restrict__ proofs, uint32_t* __restrict__ pw, uint32_t* __restrict__ wellformed) {
  const uint32_t stmt = order[blockIdx.x];
  const MixStmt& stm = stmts[stmt];
  const uint32_t proof_words = plans[stm.plan].sh.proof_words;
  const uint32_t form = stm.form, compact = form == MIX_FORM_ONE_PHASE;
  const uint8_t* p = proofs + stm.proof;
  for (uint32_t j = threadIdx.x; j < proof_words; j += blockDim.x)
    pw[stm.pw + j] = form != MIX_FORM_BAD_LENGTH ? proof_word(p, j, compact) : 0;
  if (threadIdx.x == 0)     // version byte and length must agree
    wellformed[stmt] = (form != MIX_FORM_BAD_LENGTH && p[0] == (compact ? 0 : 1)) ? 1u : 0u;
}

// ---- k_mx_transcript: k_transcript with one plan per wavefront (lane_order)
__global__ void __launch_bounds__(64)
k_mx_transcript(const PrepPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ lane_order,
                const uint32_t* __restrict__ com, const uint32_t* __restrict__ pw, const uint32_t* __restrict__ rbytes,
                uint32_t* __restrict__ ch, uint32_t* __restrict__ wellformed, uint32_t grouped) {
  __shared__ uint32_t lds[50 * 64];
  const uint32_t lane = threadIdx.x;
  const uint32_t first = lane_order[blockIdx.x * 64];       // (a run never starts with padding)
  const uint32_t mine = lane_order[blockIdx.x * 64 + lane];
  const bool live = mine != ~0u;
  const uint32_t stmt = live ? mine : first;                // padding lanes replay their wavefront's first statement
  const MixStmt& stm = stmts[stmt];
  const PrepPlan& pln = plans[stmts[first].plan];           // the wavefront's plan, the lane's own rows
  PrepStmt ps = mix_view(pln);
  ps.com = com + stm.com;
  ps.pw = pw + stm.pw;
  ps.rbytes = rbytes + (uint64_t)stmt * 16;
  const bool ok = transcript_stmt(ps, ch + stm.ch, lds + lane, pln.init, pln.tape, pln.n_ops, grouped);
  if (live && !ok) atomicAnd(&wellformed[stmt], 0u);
}

// ---- the cooperative transcript: k_mx_tape_gather + k_mx_transcript_coop + k_mx_challenges --------------------------
// k_mx_tape_gather: one workgroup per statement, its n_seg x 25 absorbed words
__global__ void __launch_bounds__(256)
k_mx_tape_gather(const PrepPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ order,
                 const uint32_t* __restrict__ com, const uint32_t* __restrict__ pw, uint2* __restrict__ absorb) {
  const MixStmt& stm = stmts[order[blockIdx.x]];
  const PrepPlan& pln = plans[stm.plan];
  PrepStmt ps = mix_view(pln);
  ps.com = com + stm.com;
  ps.pw = pw + stm.pw;
  for (uint32_t r = threadIdx.x; r < pln.n_seg * 25; r += blockDim.x)
    absorb[stm.absorb + r] = tape_gather_word(ps, pln.seg_const, pln.seg_map, r / 25, r % 25);
}

// k_mx_transcript_coop: one wavefront per statement
__global__ void __launch_bounds__(64)
k_mx_transcript_coop(const PrepPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ order,
                     const uint2* __restrict__ absorb, uint32_t* __restrict__ raw) {
  const MixStmt& stm = stmts[order[blockIdx.x]];
  const PrepPlan& pln = plans[stm.plan];
  transcript_coop_stmt(pln.n_seg, pln.seg_info, pln.init, absorb + stm.absorb, raw + stm.raw);
}

// k_mx_challenges: k_challenges per statement (blockDim = 128; dynamic LDS: the largest n_ch of the call x 32 bytes)
__global__ void __launch_bounds__(128)
k_mx_challenges(const PrepPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ order,
                const uint32_t* __restrict__ raw, const uint32_t* __restrict__ pw, const uint32_t* __restrict__ rbytes,
                uint32_t* __restrict__ ch, uint32_t* __restrict__ wellformed, uint32_t grouped) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];     // n_ch slots of 8 words
  const uint32_t stmt = order[blockIdx.x];
  const MixStmt& stm = stmts[stmt];
  PrepStmt ps = mix_view(plans[stm.plan]);
  ps.pw = pw + stm.pw;
  ps.rbytes = rbytes + (uint64_t)stmt * 16;
  ps.raw = raw + stm.raw;
  challenges_stmt(ps, ch + stm.ch, lds, &wellformed[stmt], grouped);
}

// the scalar preparation of the statements of a mixed call, launch statement b = order[b]: k_mx_prepare's and, for the plans
// that exceed a CU's LDS, large_prep.hpp's.  They write the generator index too, and no recoded form (k_small_tables makes
// it in mixed calls)
struct LpMixed {
  const PrepPlan* plans;
  const MixStmt* stmts;
  const uint32_t* order;
  const uint32_t* ch;
  uint32_t* dyn_scalars;
  uint32_t* static_scalars;
  uint32_t* static_index;
  __device__ PrepStmt at(uint32_t b) const {
    const MixStmt& stm = stmts[order[b]];
    PrepStmt ps = mix_view(plans[stm.plan]);
    ps.ch = ch + stm.ch;
    ps.ds = dyn_scalars + stm.dyn * 8;
    ps.ss = static_scalars + stm.st * 8;
    ps.sx = static_index + stm.st;
    return ps;
  }
};

// ---- k_mx_prepare: k_prepare per statement (dynamic LDS: the largest plan of the call).  Also writes the generator index
// of the statement's static terms: B, B_blinding, G_0..G_{pn-1}, H_0..H_{pn-1}
__global__ void __launch_bounds__(256, 4)
k_mx_prepare(const PrepPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ order,
             const uint32_t* __restrict__ ch, uint32_t* __restrict__ dyn_scalars, uint32_t* __restrict__ static_scalars,
             uint32_t* __restrict__ static_index) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const LpMixed src = {plans, stmts, order, ch, dyn_scalars, static_scalars, static_index};
  prepare_stmt<true>(src.at(blockIdx.x), lds);
}

// ---- k_mx_gather_dyn_points: one workgroup per statement, its proof-specific points in the order of its dynamic terms
// (compressed; decoded by the MSM's k_decompress)
__global__ void __launch_bounds__(256)
k_mx_gather_dyn_points(const PrepPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ order,
                       const uint32_t* __restrict__ com, const uint32_t* __restrict__ pw, uint32_t* __restrict__ dyn_points) {
  const MixStmt& stm = stmts[order[blockIdx.x]];
  const PrepShape& sh = plans[stm.plan].sh;
  for (uint32_t g = threadIdx.x; g < sh.n_dyn * 8; g += blockDim.x)
    dyn_points[stm.dyn * 8 + g] = dyn_point(sh, com + stm.com, pw + stm.pw, g >> 3)[g & 7];
}

// ---- group checks of a mixed call ------------------------------------------------------------------------------------
// Generators depend on their index alone: statements whose plans have the same padded multiplier count and the same
// generator capacity have the same static index list [B, B_blinding, G_0.., H_0..], whatever their constraints.  The host
// cuts the statements of each such key into CHECKS of up to group_size members (MixGroup, mixed_plan.hpp; a statement checked alone is a
// check of one member).  The equations of a check's members are added under the weights rho = r^2 the transcript put into
// their scalars: the members' generator scalars collapse into ONE static row per check (k_mx_group_scalars ->
// k_static_accumulate over the checks' rows), the members' own dynamic sums are added to it (k_mx_group_combine).  A check
// of two or more members that fails queues its members for k_recheck_fused, each alone on its own static row.

// lane (check, j): sum over the members (those not known bad already: their rows are left out) of static scalar j, its
// digits as k_static_digits writes them, and the generator index of term j (the first member's: the key's)
__global__ void __launch_bounds__(256)
k_mx_group_scalars(const MixStmt* __restrict__ stmts, const MixGroup* __restrict__ groups, const uint32_t* __restrict__ members,
                   const uint32_t* __restrict__ st_scalars, const uint32_t* __restrict__ st_index,
                   const uint32_t* __restrict__ msm_fail, const uint32_t* __restrict__ wellformed, uint64_t n_rows,
                   int16_t* __restrict__ digits /*[W][n_rows]*/, uint32_t* __restrict__ grp_index /*[n_rows]*/, int w, int W) {
  const MixGroup grp = groups[blockIdx.x];
  const uint32_t j = blockIdx.y * blockDim.x + threadIdx.x;
  if (j >= grp.ns) return;
  const uint32_t* mem = members + grp.first;
  scm acc = scm_zero();
  for (uint32_t i = 0; i < grp.count; ++i) {
    const uint32_t stmt = mem[i];
    if (tx_excluded(msm_fail, wellformed, stmt)) continue;
    const uint4* src = reinterpret_cast<const uint4*>(st_scalars + (stmts[stmt].st + j) * 8);
    const uint4 a = src[0], b = src[1];
    scm v;
    v.v[0] = a.x; v.v[1] = a.y; v.v[2] = a.z; v.v[3] = a.w; v.v[4] = b.x; v.v[5] = b.y; v.v[6] = b.z; v.v[7] = b.w;
    acc = scm_add(acc, v);
  }
  const uint64_t at = grp.st + j;
  grp_index[at] = st_index[stmts[mem[0]].st + j];
  for (int t = 0; t < W; ++t) digits[(uint64_t)t * n_rows + at] = 0;
  __attribute__((aligned(16))) uint32_t sum[8];
  for (int i = 0; i < 8; ++i) sum[i] = acc.v[i];
  for_each_digit(sum, w, W, [&](int t, int d) { digits[(uint64_t)t * n_rows + at] = (int16_t)d; });   // (< l: no range flag to raise)
}

// one workgroup per check: wavefront 0 adds the partial sums of the check's static row and the dynamic sums of its members
// and tests for the identity -> accept[] of the members.  A failed check of two or more members counts in n_fail, queues its
// members in row_map (n_recheck) and all four wavefronts write the digits of those members' own static scalars
// ([W][n_static_total], at the statements' own terms) for k_recheck_fused.
__global__ void __launch_bounds__(256)
k_mx_group_combine(const uint32_t* __restrict__ partials, uint32_t n_partials, const uint32_t* __restrict__ dyn_sum,
                   const uint32_t* __restrict__ msm_fail, const uint32_t* __restrict__ wellformed,
                   const MixStmt* __restrict__ stmts, const MixGroup* __restrict__ groups, const uint32_t* __restrict__ members,
                   const uint32_t* __restrict__ st_scalars, uint64_t n_static_total, uint8_t* __restrict__ accept,
                   uint32_t* __restrict__ n_fail, uint32_t* __restrict__ row_map, uint32_t* __restrict__ n_recheck,
                   int16_t* __restrict__ rechk_digits, int w, int W) {
  __shared__ uint32_t sh_recheck;
  const MixGroup grp = groups[blockIdx.x];
  const uint32_t* mem = members + grp.first;
  const int t = threadIdx.x, lane = t & 63;
  if (t < 64) {
    ge acc;
    ge_identity(acc);
    for (uint32_t c = lane; c < n_partials; c += 64) {
      ge p;
      load_ext(p, partials + ((uint64_t)blockIdx.x * n_partials + c) * EXT_WORDS);
      ge_add(acc, acc, p);
    }
    for (uint32_t i = lane; i < grp.count; i += 64) {
      const uint32_t stmt = mem[i];
      if (!tx_excluded(msm_fail, wellformed, stmt)) {
        ge p;
        load_ext(p, dyn_sum + (uint64_t)stmt * EXT_WORDS);
        ge_add(acc, acc, p);
      }
    }
#pragma unroll 1
    for (int delta = 32; delta >= 1; delta >>= 1) {
      ge other;
      shfl_down_ge(other, acc, delta);
      if (lane < delta) ge_add(acc, acc, other);
    }
    const int ok = __shfl((lane == 0 && ge_is_identity(acc)) ? 1 : 0, 0);
    for (uint32_t i = lane; i < grp.count; i += 64)
      accept[mem[i]] = (ok && !tx_excluded(msm_fail, wellformed, mem[i])) ? 1 : 0;
    const bool recheck = !ok && grp.count >= 2;
    if (recheck) {
      for (uint32_t i0 = 0; i0 < grp.count; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool live = i < grp.count && !tx_excluded(msm_fail, wellformed, mem[i]);
        const unsigned long long lives = __ballot(live);
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(n_recheck, (uint32_t)__popcll(lives));
        base = __shfl(base, 0);
        if (live) row_map[base + (uint32_t)__popcll(lives & ((1ull << lane) - 1))] = mem[i];
      }
      if (lane == 0) atomicAdd(n_fail, 1u);
    }
    if (lane == 0) sh_recheck = recheck ? 1u : 0u;
  }
  __syncthreads();
  if (!sh_recheck) return;
  for (uint32_t i = 0; i < grp.count; ++i) {
    const uint32_t stmt = mem[i];
    if (tx_excluded(msm_fail, wellformed, stmt)) continue;
    const uint64_t k0 = stmts[stmt].st;
    for (uint32_t j = (uint32_t)t; j < grp.ns; j += blockDim.x) {
      const uint64_t g = k0 + j;
      for (int tt = 0; tt < W; ++tt) rechk_digits[(uint64_t)tt * n_static_total + g] = 0;
      for_each_digit(st_scalars + 8 * g, w, W, [&](int tt, int dd) { rechk_digits[(uint64_t)tt * n_static_total + g] = (int16_t)dd; });
    }
  }
}

}  // namespace zk
