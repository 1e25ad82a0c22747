// mixed_kernels.hpp -- the device-side head of r1cs::Verifier::verify for a batch whose statements belong to
// DIFFERENT constraint systems (zkgpu_r1cs_verify_mixed): the per-statement stages of prep_kernels.hpp with the
// shape read from a per-call table instead of a by-value PrepShape, so that one launch per stage serves every plan.
//
//   MixPlan   one per distinct plan of the call: its PrepShape and the device addresses of its replay arrays
//   MixStmt   one per statement, in the CALLER's order: its plan, proof wire form, and where its inputs, its
//             challenge slots and its rows of the multiscalar multiplication live (rows have the statement's own
//             lengths: 11 + m + 2k dynamic and 2 + 2 pn static terms)
//   order     the statements sorted by plan: workgroup b of the per-statement kernels takes statement order[b]
//   lane_order  the same, each plan's run padded to a multiple of 64 with ~0u: the one-lane-per-statement
//             transcript sees one plan per wavefront (its tape loop stays uniform)
//
// Outputs are those of the homogeneous kernels at the statement's own offsets; the verdict bits, the accept
// flags and r_bytes stay indexed by the caller's position.  Statements are always checked alone (rho = 1).
#pragma once
#include "prep_kernels.hpp"

namespace zk {

struct MixPlan {
  PrepShape sh;
  const uint32_t* init;        // STROBE state after Transcript::new(label) + the r1cs domain separator (50 words)
  const uint4* tape;
  const uint32_t* seg_info;    // cooperative transcript (n_seg = 0: not available for this plan)
  const uint32_t* seg_const;
  const uint16_t* seg_map;
  const uint32_t* mono_chal;
  const uint32_t* mono_pow;
  const uint32_t* tgt_off;
  const uint32_t* term_info;
  const uint2* prod_qm;
  const uint32_t* prod_coef;
  uint32_t n_ops, n_seg;
  uint32_t h_base;             // index of H_0 in the point set: 2 + the plan's generator capacity
  uint32_t pad;
};

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

// ---- k_mx_proof_unpack: one workgroup per statement; sets the statement's well-formedness flag (first writer)
__global__ void __launch_bounds__(256)
k_mx_proof_unpack(const MixPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ order,
                  const uint8_t* __restrict__ proofs, uint32_t* __restrict__ pw, uint32_t* __restrict__ wellformed) {
  const uint32_t stmt = order[blockIdx.x];
  const MixStmt& stm = stmts[stmt];
  const uint32_t proof_words = plans[stm.plan].sh.proof_words;
  const uint32_t form = stm.form, compact = form == MIX_FORM_ONE_PHASE;
  const uint8_t* p = proofs + stm.proof;
  for (uint32_t j = threadIdx.x; j < proof_words; j += blockDim.x) {
    uint32_t v = 0;
    if (form != MIX_FORM_BAD_LENGTH && (!compact || j < 24 || j >= 48)) {
      const uint8_t* b = p + 1 + 4 * (uint64_t)((compact && j >= 48) ? j - 24 : j);
      v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    }
    pw[stm.pw + j] = v;
  }
  if (threadIdx.x == 0)     // version byte and length must agree
    wellformed[stmt] = (form != MIX_FORM_BAD_LENGTH && p[0] == (compact ? 0 : 1)) ? 1u : 0u;
}

// ---- k_mx_transcript: k_transcript with one plan per wavefront (lane_order)
__global__ void __launch_bounds__(64)
k_mx_transcript(const MixPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ lane_order,
                const uint32_t* __restrict__ com, const uint32_t* __restrict__ pw, const uint32_t* __restrict__ rbytes,
                uint32_t* __restrict__ ch, uint32_t* __restrict__ wellformed) {
  __shared__ uint32_t lds[50 * 64];
  const uint32_t lane = threadIdx.x;
  const uint32_t first = lane_order[blockIdx.x * 64];       // (a run never starts with padding)
  const uint32_t mine = lane_order[blockIdx.x * 64 + lane];
  const bool live = mine != ~0u;
  const uint32_t stmt = live ? mine : first;                // padding lanes replay their wavefront's first statement
  const MixStmt& stm = stmts[stmt];
  const MixPlan& pln = plans[stmts[first].plan];
  const PrepShape& sh = pln.sh;
  const uint4* __restrict__ tape = pln.tape;
  const uint32_t n_ops = pln.n_ops;
  const uint32_t* __restrict__ mono_chal = pln.mono_chal;
  const uint32_t* __restrict__ mono_pow = pln.mono_pow;
  uint32_t* st = lds + lane;                    // word w of this lane: st[w * 64]
  for (int i = 0; i < 50; ++i) st[i * 64] = pln.init[i];
  const uint32_t* c = com + stm.com;
  const uint32_t* p = pw + stm.pw;
  uint32_t* out = ch + stm.ch;
#pragma unroll 1
  for (uint32_t o = 0; o < n_ops; ++o) {
    const uint4 op = tape[o];
    if (op.x == TAPE_XOR) {
      st[op.y * 64] ^= op.z;
    } else if (op.x == TAPE_DATA) {
      const uint32_t* src = op.y == TAPE_SRC_PROOF ? p : c;
      const int last_word = (int)(op.y == TAPE_SRC_PROOF ? sh.proof_words : sh.m * 8) - 1;
      const uint32_t spos = op.w & 0xffffu, n = op.w >> 16;
      const int delta = (int)op.z - (int)spos;            // source byte = state byte + delta
#pragma unroll 1
      for (uint32_t w = spos >> 2; w <= (spos + n - 1) >> 2; ++w) {
        const int sb = (int)(4 * w) + delta;              // source byte under state byte 4w
        const int wi = sb >> 2;
        const uint32_t sh8 = (uint32_t)(sb & 3) * 8;
        const uint32_t lo = src[min(max(wi, 0), last_word)], hi = src[min(max(wi + 1, 0), last_word)];
        const uint32_t v = sh8 ? (lo >> sh8) | (hi << (32 - sh8)) : lo;
        const uint32_t first = max(spos, 4 * w) - 4 * w, last = min(spos + n, 4 * w + 4) - 4 * w;
        const uint32_t mask = (last == 4 ? 0xffffffffu : ((1u << (8 * last)) - 1)) & ~((1u << (8 * first)) - 1);
        st[w * 64] ^= v & mask;
      }
    } else if (op.x == TAPE_PERM) {
      uint32_t klo[25], khi[25];
#pragma unroll
      for (int q = 0; q < 25; ++q) { klo[q] = st[(2 * q) * 64]; khi[q] = st[(2 * q + 1) * 64]; }
      keccak_f1600_halves(klo, khi);
#pragma unroll
      for (int q = 0; q < 25; ++q) { st[(2 * q) * 64] = klo[q]; st[(2 * q + 1) * 64] = khi[q]; }
    } else {                                               // TAPE_CHAL
      uint32_t wv[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) { wv[q] = st[q * 64]; st[q * 64] = 0; }
      st_scm(out + op.y * 8, scm_from_wide(wv));
    }
  }
  // well-formedness: no identity among the proof points, canonical scalars
  bool ok = true;
  // (A_I2, A_O2, S2 are the identity in single-phase proofs: not tested, as in the reference)
  for (int i = 0; i < 11; ++i) ok &= (i >= 3 && i < 6) | !words_are_zero(p + 8 * i);
  const uint32_t* sc3 = p + 88;               // t_x, t_x_blinding, e_blinding
  const uint32_t* lr = p + 112;               // L_0 R_0 L_1 R_1 ...
  const uint32_t* ab = lr + 16 * sh.k;        // a, b
  ok &= scm_is_canonical(sc3) & scm_is_canonical(sc3 + 8) & scm_is_canonical(sc3 + 16) & scm_is_canonical(ab) &
        scm_is_canonical(ab + 8);
  for (uint32_t j = 0; j < sh.k; ++j) ok &= !words_are_zero(lr + 16 * j) & !words_are_zero(lr + 16 * j + 8);
#pragma unroll 1
  for (int q = 0; q < 5; ++q) st_scm(out + (8 + q) * 8, scm_from_words(q < 3 ? sc3 + 8 * q : ab + 8 * (q - 3)));
  {
    // r combines the two halves of this proof's equation; rho = r^2 weighs the whole equation inside a
    // group of transactions checked by one multiscalar multiplication (coefficients r^2, r^3 of a
    // transaction's two halves: a polynomial identity in independent r's, Schwartz-Zippel as for r alone)
    const scm rr = scm_from_wide(rbytes + (uint64_t)stmt * 16);
    st_scm(out + 7 * 8, rr);
    st_scm(out + 13 * 8, scm_one());            // rho: every statement is checked alone
  }
  // the serial chains k_prepare needs, done here where every lane has one to do: second-phase
  // monomials, z^(2^L), y^(2^L), u_j^2, U = prod u_j^2, prod_{l != j} u_l^2.  (Measured the other way
  // round -- raw challenge bytes out of this kernel, reductions and chains on parallel lanes of
  // k_prepare: transcript 0.57 -> 0.38 ms, prepare 0.25 -> 0.27 ms, and the step 3-5 % SLOWER: the
  // chip-filling kernel's extra work costs more than the light kernel's latency.)
  uint32_t* sym = out + sh.n_ch * 8;
  uint32_t* strides = sym + sh.n_mono * 8;
  uint32_t* uj = out + (CH_FIXED + sh.n_chal2) * 8;
  uint32_t* uex = uj + 8 * sh.k;
#pragma unroll 1
  for (uint32_t j = 0; j < sh.n_mono; ++j) {
    scm v = scm_one();
    if (mono_chal[j] != 0xffffffffu) {
      scm cc;
      ld_scm(cc, out + (CH_FIXED + mono_chal[j]) * 8);
      v = scm_pow_u32(cc, mono_pow[j]);
    }
    st_scm(sym + 8 * j, v);
  }
  {
    scm cc;
    ld_scm(cc, out + 1 * 8);
    st_scm(strides, cc);
#pragma unroll 1
    for (uint32_t L = 1; (1u << L) < sh.n_cons; ++L) { cc = scm_sq(cc); st_scm(strides + 8 * L, cc); }
    ld_scm(cc, out + 0 * 8);                      // y
    ok &= !words_are_zero(cc.v);
    st_scm(strides + 16 * 8, cc);
#pragma unroll 1
    for (uint32_t L = 1; L < sh.k; ++L) { cc = scm_sq(cc); st_scm(strides + (16 + L) * 8, cc); }
    // prefix products of the u_j^2 go to the "excluded" slots, then the suffix pass completes them
    scm run = scm_one(), p1 = scm_one();
#pragma unroll 1
    for (uint32_t j = 0; j < sh.k; ++j) {
      ld_scm(cc, uj + 8 * j);
      ok &= !words_are_zero(cc.v);
      p1 = scm_mul(p1, cc);
      const scm sq = scm_sq(cc);
      st_scm(strides + (32 + j) * 8, sq);
      st_scm(uex + 8 * j, run);                   // prod_{l < j} u_l^2
      run = scm_mul(run, sq);
    }
    st_scm(out + 6 * 8, run);                     // U = prod u_j^2
    st_scm(out + 5 * 8, p1);                      // P1 = prod u_j
    run = scm_one();
#pragma unroll 1
    for (uint32_t j = sh.k; j-- > 0;) {
      scm pre, sq;
      ld_scm(pre, uex + 8 * j);
      st_scm(uex + 8 * j, scm_mul(pre, run));     // prod_{l != j} u_l^2
      ld_scm(sq, strides + (32 + j) * 8);
      run = scm_mul(run, sq);
    }
  }
  if (live && !ok) atomicAnd(&wellformed[stmt], 0u);
}

// ---- the cooperative transcript: k_mx_tape_gather + k_mx_transcript_coop + k_mx_challenges --------------------------
// k_mx_tape_gather: one workgroup per statement, its n_seg x 25 absorbed words
__global__ void __launch_bounds__(256)
k_mx_tape_gather(const MixPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ order,
                 const uint32_t* __restrict__ com, const uint32_t* __restrict__ pw, uint2* __restrict__ absorb) {
  const uint32_t stmt = order[blockIdx.x];
  const MixStmt& stm = stmts[stmt];
  const MixPlan& pln = plans[stm.plan];
  const uint32_t* c = com + stm.com;
  const uint32_t* p = pw + stm.pw;
  const uint32_t n_com_bytes = 32 * pln.sh.m, per_tx = pln.n_seg * 25;
  for (uint32_t r = threadIdx.x; r < per_tx; r += blockDim.x) {
    const uint32_t seg = r / 25, q = r % 25;
    const uint4 mp4 = *reinterpret_cast<const uint4*>(pln.seg_map + (uint64_t)seg * 200 + 8 * q);
    const uint32_t mp[4] = {mp4.x, mp4.y, mp4.z, mp4.w};
    uint32_t lo = pln.seg_const[seg * 50 + 2 * q], hi = pln.seg_const[seg * 50 + 2 * q + 1];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const uint32_t idx = (mp[b >> 1] >> (16 * (b & 1))) & 0xffffu;
      if (idx) {
        const uint32_t i = idx - 1;
        const uint32_t word = i < n_com_bytes ? c[i >> 2] : p[(i - n_com_bytes) >> 2];
        const uint32_t byte = (word >> (8 * (i & 3))) & 0xffu;
        if (b < 4) lo ^= byte << (8 * b); else hi ^= byte << (8 * (b - 4));
      }
    }
    absorb[stm.absorb + r] = make_uint2(lo, hi);
  }
}

// k_mx_transcript_coop: one wavefront per statement
__global__ void __launch_bounds__(64)
k_mx_transcript_coop(const MixPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ order,
                     const uint2* __restrict__ absorb, uint32_t* __restrict__ raw) {
  const uint32_t stmt = order[blockIdx.x], lane = threadIdx.x;
  const MixStmt& stm = stmts[stmt];
  const MixPlan& pln = plans[stm.plan];
  const uint32_t n_seg = pln.n_seg;
  const uint32_t* __restrict__ seg_info = pln.seg_info;
  const coop::KcLane k = coop::kc_lane(lane);
  const coop::KeccakCoop<DevKcTraits>::Consts c = {k.live, k.rot_swap, k.rot_t, k.src[0], k.src[1], k.src[2], k.iota};
  uint32_t lo = k.live ? pln.init[2 * k.q] : 0, hi = k.live ? pln.init[2 * k.q + 1] : 0;
  const uint2* ab = absorb + stm.absorb + k.q;
  const bool first8 = k.live && k.q < 8;           // state bytes 0..63: what a challenge squeezes
  uint2 nxt = k.live ? ab[0] : make_uint2(0, 0);
#pragma unroll 1
  for (uint32_t seg = 0; seg < n_seg; ++seg) {
    const uint32_t info = seg_info[seg];
    const uint2 cur = nxt;
    if (seg + 1 < n_seg && k.live) nxt = ab[(uint64_t)(seg + 1) * 25];      // in flight during the permutation
    const uint32_t slot = info & 0xffffu;
    if (slot) {
      if (k.primary && k.q < 8) {
        uint32_t* o = raw + stm.raw + (uint64_t)(slot - 1) * 16 + 2 * k.q;
        o[0] = lo; o[1] = hi;
      }
      if (first8) { lo = 0; hi = 0; }
    }
    lo ^= cur.x; hi ^= cur.y;
    if (info >> 31) coop::KeccakCoop<DevKcTraits>::permute(lo, hi, c);
  }
}

// k_mx_challenges: k_challenges per statement (blockDim = 128; dynamic LDS: the largest n_ch of the call x 32 bytes)
__global__ void __launch_bounds__(128)
k_mx_challenges(const MixPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ order,
                const uint32_t* __restrict__ raw, const uint32_t* __restrict__ pw, const uint32_t* __restrict__ rbytes,
                uint32_t* __restrict__ ch, uint32_t* __restrict__ wellformed) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];     // n_ch slots of 8 words
  const uint32_t stmt = order[blockIdx.x], t = threadIdx.x, nt = blockDim.x;
  const MixStmt& stm = stmts[stmt];
  const MixPlan& pln = plans[stm.plan];
  const PrepShape& sh = pln.sh;
  const uint32_t* __restrict__ mono_chal = pln.mono_chal;
  const uint32_t* __restrict__ mono_pow = pln.mono_pow;
  const uint32_t* p = pw + stm.pw;
  uint32_t* out = ch + stm.ch;
  const uint32_t n2 = sh.n_chal2, k = sh.k;
  // phase 1: every slot is the reduction of 64 little-endian bytes (8-word sources padded with zeros)
  for (uint32_t s = t; s < sh.n_ch; s += nt) {
    uint32_t w[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) w[q] = 0;
    const bool is_chal = s < 5 || (s >= (uint32_t)CH_FIXED && s < CH_FIXED + n2 + k);
    const uint32_t* src = nullptr;
    int words = 0;
    if (is_chal) { src = raw + stm.raw + (uint64_t)s * 16; words = 16; }
    else if (s == 7 || s == 13) { src = rbytes + (uint64_t)stmt * 16; words = 16; }
    else if (s >= 8 && s <= 12) { src = s <= 10 ? p + 88 + 8 * (s - 8) : p + 112 + 16 * k + 8 * (s - 11); words = 8; }
#pragma unroll
    for (int q = 0; q < 16; ++q) if (q < words) w[q] = src[q];
    scm v = scm_from_wide(w);
    if (s == 13) v = scm_one();  // rho: every statement is checked alone
    if (words) { st_scm(lds + 8 * s, v); st_scm(out + 8 * s, v); }
  }
  __syncthreads();
  uint32_t* sym = out + sh.n_ch * 8;
  uint32_t* strides = sym + sh.n_mono * 8;
  if (t < 64) {
    // chains, one per lane: 0 the squarings of z, 1 those of y, 2 + j the monomial j (challenge^power).
    // Uniform loop: acc = acc^2 [* base]; a chain stores what it needs as it goes.
    const uint32_t n_chains = 2 + sh.n_mono;
    uint32_t n_zs = 1;
    while ((1u << n_zs) < sh.n_cons) ++n_zs;           // strides z^(2^L), L < n_zs
    for (uint32_t base0 = 0; base0 < n_chains; base0 += 64) {
      const uint32_t cid = base0 + t;
      scm base = scm_one(), acc = scm_one();
      uint32_t steps = 0, e = 0;
      if (cid == 0) { ld_scm(base, lds + 8 * 1); acc = base; steps = n_zs - 1; st_scm(strides, acc); }
      else if (cid == 1) { ld_scm(base, lds + 8 * 0); acc = base; steps = k ? k - 1 : 0; st_scm(strides + 16 * 8, acc); }
      else if (cid < n_chains) {
        const uint32_t j = cid - 2, mc = mono_chal[j];
        e = mono_pow[j];
        if (mc != 0xffffffffu && e != 0) {
          ld_scm(base, lds + 8 * (CH_FIXED + mc));
          acc = base;
          steps = 31 - __clz(e);                        // bits below the top one
        } else {
          e = 0;
        }
      }
      uint32_t max_steps = steps;
#pragma unroll 1
      for (int d = 32; d >= 1; d >>= 1) max_steps = max(max_steps, (uint32_t)__shfl_xor((int)max_steps, d));
#pragma unroll 1
      for (uint32_t i = 1; i <= max_steps; ++i) {
        const bool on = i <= steps;
        const scm sq = scm_sq(acc);
        if (on) acc = sq;
        const bool mul = on && cid >= 2 && ((e >> (steps - i)) & 1);
        if (__any(mul)) { const scm m = scm_mul(acc, base); if (mul) acc = m; }
        if (on && cid == 0) st_scm(strides + 8 * i, acc);
        if (on && cid == 1) st_scm(strides + (16 + i) * 8, acc);
      }
      if (cid >= 2 && cid < n_chains) st_scm(sym + 8 * (cid - 2), acc);
    }
    return;
  }
  // wavefront 1
  const uint32_t lane = t - 64;
  bool ok = true;
  if (lane == 0) {
    // well-formedness: no identity among the proof points (A_I2, A_O2, S2 are the identity in single-phase
    // proofs: not tested, as in the reference), canonical scalars
    for (int i = 0; i < 11; ++i) ok &= (i >= 3 && i < 6) | !words_are_zero(p + 8 * i);
    const uint32_t* sc3 = p + 88;
    const uint32_t* lr = p + 112;
    const uint32_t* ab = lr + 16 * k;
    ok &= scm_is_canonical(sc3) & scm_is_canonical(sc3 + 8) & scm_is_canonical(sc3 + 16) & scm_is_canonical(ab) &
          scm_is_canonical(ab + 8);
    for (uint32_t j = 0; j < k; ++j) ok &= !words_are_zero(lr + 16 * j) & !words_are_zero(lr + 16 * j + 8);
    ok &= !words_are_zero(lds + 0);                    // y = 0: the reference's inversion has no answer either
  }
  // products of the inner-product challenges u_j (lane j < k <= 16): prefix and suffix products by
  // doubling steps, then P1 = prod u_j, U = P1^2, u_j^2 and prod_{l != j} u_l^2 = (prefix_{j-1} suffix_{j+1})^2
  uint32_t* uj = lds + (CH_FIXED + n2) * 8;
  uint32_t* uex = out + (CH_FIXED + n2 + k) * 8;
  scm u = scm_one();
  if (lane < k) { ld_scm(u, uj + 8 * lane); ok &= !words_are_zero(u.v); }
  scm pre = u, suf = u;
#pragma unroll 1
  for (uint32_t d = 1; d < k; d <<= 1) {
    scm a, b;
#pragma unroll
    for (int q = 0; q < 8; ++q) { a.v[q] = (uint32_t)__shfl_up((int)pre.v[q], d); b.v[q] = (uint32_t)__shfl_down((int)suf.v[q], d); }
    const scm pa = scm_mul(pre, a), sb = scm_mul(suf, b);
    if (lane >= d && lane < k) pre = pa;
    if (lane + d < k) suf = sb;
  }
  scm pm, sp;                                           // prefix_{j-1}, suffix_{j+1}
#pragma unroll
  for (int q = 0; q < 8; ++q) { pm.v[q] = (uint32_t)__shfl_up((int)pre.v[q], 1); sp.v[q] = (uint32_t)__shfl_down((int)suf.v[q], 1); }
  if (lane == 0) pm = scm_one();
  if (lane + 1 >= k) sp = scm_one();
  const scm ex = scm_mul(pm, sp), ex2 = scm_sq(ex), u2 = scm_sq(u);
  if (lane < k) { st_scm(strides + (32 + lane) * 8, u2); st_scm(uex + 8 * lane, ex2); }
  if (k == 0 ? lane == 0 : lane == k - 1) {
    const scm p1 = k ? pre : scm_one();
    st_scm(out + 5 * 8, p1);
    st_scm(out + 6 * 8, scm_sq(p1));
  }
  if (!__all(ok) && lane == 0) atomicAnd(&wellformed[stmt], 0u);
}

// ---- k_mx_prepare: k_prepare per statement (dynamic LDS: the largest plan of the call).  Also writes the generator index
// of the statement's static terms: B, B_blinding, G_0..G_{pn-1}, H_0..H_{pn-1}
__global__ void __launch_bounds__(256, 4)
k_mx_prepare(const MixPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ order,
             const uint32_t* __restrict__ ch, uint32_t* __restrict__ dyn_scalars, uint32_t* __restrict__ static_scalars,
             uint32_t* __restrict__ static_index) {
  const MixStmt& stm = stmts[order[blockIdx.x]];
  const MixPlan& pln = plans[stm.plan];
  const PrepShape& sh = pln.sh;
  const uint32_t* __restrict__ tgt_off = pln.tgt_off;
  const uint32_t* __restrict__ term_info = pln.term_info;
  const uint2* __restrict__ prod_qm = pln.prod_qm;
  const uint32_t* __restrict__ prod_coef = pln.prod_coef;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  constexpr uint32_t SW = SCL_WORDS;
  uint32_t* chs = lds;
  uint32_t* sym = chs + sh.n_ch * SW;
  uint32_t* zs = sym + sh.n_mono * SW;          // z^(2^L)
  uint32_t* ys = zs + 16 * SW;                   // y^-(2^L)
  uint32_t* us2 = ys + 16 * SW;                  // u_j^2
  uint32_t* wv = chs + sh.n_ch_ext * SW;
  const uint32_t LB = prep_lo_bits(sh), NLO = 1u << LB, PH = sh.pn >> LB, ZLO = sh.n_cons < 16 ? sh.n_cons : 16, ZH = prep_zhi(sh);
  uint32_t* ylo = wv + sh.n_targets * SW;       // plain y^l, l < 16            (rho y^i = ylo[i & 15] * yhi[i >> 4], plain)
  uint32_t* yhi = ylo + 16 * SW;                 // rho y^(16 h)
  uint32_t* slo = yhi + PH * SW;                 // s_i = slo[i & 15] * shi[i >> 4]
  uint32_t* shi = slo + 16 * SW;
  uint32_t* red = shi + PH * SW;
  uint32_t* shr = red + 8 * SW;                  // 0: x U  1: a P1  2: b P1  3: c' (plain)  4: a P1 rho Y (plain)  5: c' (Montgomery)  6: rho Y (plain)  7: plain 1
                                                 // 8 .. 12: (x U) u, (a P1 rho Y) u, (b P1) u, U u, c' u -- what slots 0, 4, 2, U, 3 are for i >= n1
  uint32_t* zpow = lds + (((uint32_t)(shr + 16 * SW - lds) + 3u) & ~3u);      // region A (16-byte aligned), first life
  uint32_t* tv = zpow + sh.n_cons * SW;
  uint32_t* zlo = tv;                            // z^(l+1), l < 16              (z^(q+1) = zlo[q & 15] * zhi[q >> 4])
  uint32_t* zhi = tv + 16 * SW;                  // z^(16 h)
  uint32_t* yip = zpow;                          // region A, second life: two packed tables (8 words per entry)
  uint32_t* sv = yip + sh.pn * 8;
  const uint32_t t = threadIdx.x, nt = blockDim.x;

  // the transaction's slots (canonical Montgomery words) -> limb form
  for (uint32_t i = t; i < sh.n_ch_ext; i += nt) {
    const uint4* src = reinterpret_cast<const uint4*>(ch + stm.ch + (uint64_t)i * 8);
    const uint4 a = src[0], b = src[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    st_scl(chs + i * SW, scl_from_words(w));
  }
  __syncthreads();
  uint32_t* xp = us2 + 16 * SW;                  // xp[0..4] = x^2..x^6, xp[5] = r x^2
  if (t == 0) {                                  // what the small tables start from
    scl z, rho;
    ld_scl(z, zs); ld_scl(rho, chs + 13 * SW);
    st_scl(zlo, z); st_scl(zhi, scl_one());
    st_scl(ylo, scl_plain_one()); st_scl(yhi, rho);
    st_scl(slo, scl_one()); st_scl(shi, scl_one());
    st_scl(shr + 7 * SW, scl_plain_one());
  }
  __syncthreads();
  // phase B: the six small tables by doubling, all in the same steps, one job = one product dst = a * b per lane.  Beside
  // them, on the lanes that follow: the powers of x the proof-point scalars need (step 0: x^2 | step 1: x^3, x^4, r x^2 |
  // step 2: x^5, x^6) and, in step 0, x U, a P1, b P1.  A payment's steps have 10, 15, 27, 48, 10 jobs: one wavefront.
#pragma unroll 1
  for (uint32_t L = 0, half = 1;; ++L, half <<= 1) {
    auto fresh = [half](uint32_t n) { return n > half ? (n - half < half ? n - half : half) : 0u; };   // entries [half, 2 half) of a table of n
    const uint32_t c0 = fresh(ZLO), c1 = fresh(ZH), c2 = fresh(NLO), c3 = fresh(PH);
    const uint32_t n_tab = c0 + c1 + 2 * (c2 + c3), n_side = L == 0 ? 4u : L == 1 ? 3u : L == 2 ? 2u : 0u;
    if (n_tab + n_side == 0) break;
    for (uint32_t j0 = t; j0 < n_tab + n_side; j0 += nt) {
      uint32_t j = j0;
      const uint32_t* pa;
      const uint32_t* pb;
      uint32_t* pd;
      if (j < c0) { pa = zlo + j * SW; pb = zs + L * SW; pd = zlo + (half + j) * SW; }
      else if ((j -= c0) < c1) { pa = zhi + j * SW; pb = zs + (L + 4) * SW; pd = zhi + (half + j) * SW; }
      else if ((j -= c1) < c2) { pa = ylo + j * SW; pb = ys + L * SW; pd = ylo + (half + j) * SW; }
      else if ((j -= c2) < c3) { pa = yhi + j * SW; pb = ys + (L + LB) * SW; pd = yhi + (half + j) * SW; }
      else if ((j -= c3) < c2) { pa = slo + j * SW; pb = us2 + (sh.k - 1 - L) * SW; pd = slo + (half + j) * SW; }
      else if ((j -= c2) < c3) { pa = shi + j * SW; pb = us2 + (sh.k - 1 - L - LB) * SW; pd = shi + (half + j) * SW; }
      else {
        j -= c3;
        const uint32_t* const px = chs + 3 * SW;
        if (L == 0) {
          if (j == 0) { pa = px; pb = px; pd = xp; }                                      // x^2
          else { pa = chs + (j == 1 ? 3 : j == 2 ? 11 : 12) * SW; pb = chs + (j == 1 ? 6 : 5) * SW; pd = shr + (j - 1) * SW; }   // x U | a P1 | b P1
        } else if (L == 1) {
          pa = j == 2 ? chs + 7 * SW : xp;                                               // x^2 x | x^2 x^2 | r x^2
          pb = j == 0 ? px : xp;
          pd = xp + (j == 0 ? 1 : j == 1 ? 2 : 5) * SW;
        } else {
          pa = xp + 2 * SW; pb = j == 0 ? px : xp; pd = xp + (j == 0 ? 3 : 4) * SW;       // x^4 x | x^4 x^2
        }
      }
      scl a, b;
      ld_scl(a, pa); ld_scl(b, pb);
      st_scl(pd, scl_mul(a, b));
    }
    __syncthreads();
  }
  // ... and z^(q+1) for every constraint q, one product each
  for (uint32_t q = t; q < sh.n_cons; q += nt) {
    scl a, b;
    ld_scl(a, zlo + SW * (q & 15)); ld_scl(b, zhi + SW * (q >> 4));
    st_scl(zpow + SW * q, scl_mul(a, b));
  }
  __syncthreads();
  // phase C: plan replay, a range of targets at a time: the products of the range (one multiplication per product, two
  // when a second-phase challenge is involved), then one sum per target.  Every stored value is a product (< 2^255) or
  // a weakly reduced sum (< 2 l).
#pragma unroll 1
  for (uint32_t ck = 0; ck < sh.n_chunks; ++ck) {
    const uint32_t g0 = sh.chunk_tgt[ck], g1 = sh.chunk_tgt[ck + 1];
    const uint32_t p0 = sh.chunk_prod[ck], p1 = sh.chunk_prod[ck + 1];
    for (uint32_t p = p0 + t; p < p1; p += nt) {
      scl c, zq;
      ld_scl(c, prod_coef + SW * (uint64_t)p);
      const uint2 qm = prod_qm[p];
      ld_scl(zq, zpow + SW * qm.x);
      if (qm.y != 0) { scl m; ld_scl(m, sym + SW * qm.y); c = scl_mul(c, m); }
      st_scl(tv + SW * (p - p0), scl_mul(c, zq));
    }
    __syncthreads();
    // <= HEAVY_TERMS terms, each < 2^255 or its negative (256 l - v, limbs < 2^27.6): limbs < 2^31.6, value < 2^264.1
    auto term_value = [&](uint32_t e) {
      const uint32_t info = term_info[e];
      scl v;
      if (info & TERM_UNIT) ld_scl(v, zpow + SW * (info & TERM_IDX));
      else ld_scl(v, tv + SW * ((info & TERM_IDX) - p0));
      return scl_cneg(v, (info & TERM_NEG) != 0);
    };
    for (uint32_t g = g0 + t; g < g1; g += nt) {
      bool heavy = false;
      for (uint32_t hI = 0; hI < sh.n_heavy; ++hI) heavy |= (sh.heavy[hI] == g);
      if (heavy) continue;
      scl acc = scl_zero();
      uint32_t cnt = 0;
      for (uint32_t e = tgt_off[g]; e < tgt_off[g + 1]; ++e) {
        acc = scl_add(acc, term_value(e));
        if (++cnt == HEAVY_TERMS) { acc = scl_weak(acc); cnt = 1; }
      }
      st_scl(wv + SW * g, scl_weak(acc));
    }
    // heavy targets: every lane sums a strided share, wavefront shuffles fold the lanes, lane 0 of
    // each wave parks its sum in the scratch slots after the products (4 per heavy target)
    for (uint32_t hI = 0; hI < sh.n_heavy; ++hI) {
      const uint32_t g = sh.heavy[hI];
      if (g < g0 || g >= g1) continue;
      scl acc = scl_zero();
      uint32_t cnt = 0;
      for (uint32_t e = tgt_off[g] + t; e < tgt_off[g + 1]; e += nt) {
        acc = scl_add(acc, term_value(e));
        if (++cnt == HEAVY_TERMS) { acc = scl_weak(acc); cnt = 1; }
      }
      acc = wave_sum_scl(scl_weak(acc));
      uint32_t* wave_sums = tv + (sh.tv_cap + 4 * hI) * SW;
      if ((t & 63) == 63) st_scl(wave_sums + SW * (t >> 6), acc);
      __syncthreads();
      if (t == 0) {
        scl tot = scl_zero();
        for (uint32_t wI = 0; wI < (nt >> 6); ++wI) { scl v; ld_scl(v, wave_sums + SW * wI); tot = scl_add(tot, v); }
        st_scl(wv + SW * g, scl_weak(tot));
      }
    }
    __syncthreads();
  }
  // phase E (region A is dead).  The whole equation is taken times c' = rho y^(pn-1) U, U = prod u_j^2
  // (rho: chs slot 13, 1 unless the batch is checked in groups), which needs no inverse:
  //     c' y^-i        = U * yp[pn-1-i]             yp[j] = rho y^j, kept in PLAIN form
  //     c' s_i         = yp[pn-1] * P1 * sU[i]      sU[i] = prod_j u_j^(2 bit_(k-1-j)(i)),  P1 = prod u_j
  //     c' y^-i s_r    = yp[pn-1-i] * P1 * sU[r]    (U s_i = prod u_j^(2 +- 1) = P1 sU[i])
  // Both tables grow by doubling (entry + 2^L = entry * stride_L).
  for (uint32_t idx = t; idx < 2 * sh.pn; idx += nt) {
    const bool second = idx >= sh.pn;
    const uint32_t i = second ? idx - sh.pn : idx;
    scl a, b;
    ld_scl(a, (second ? slo : ylo) + SW * (i & (NLO - 1)));
    ld_scl(b, (second ? shi : yhi) + SW * (i >> LB));
    st_scl8((second ? sv : yip) + 8 * i, scl_mul(a, b));
  }
  __syncthreads();
  const uint32_t* wL = wv;
  const uint32_t* wR = wv + sh.n * SW;
  const uint32_t* wO = wv + 2 * sh.n * SW;
  const uint32_t* wV = wv + 3 * sh.n * SW;
  const uint32_t* wc = wV + sh.m * SW;
  // dsum = rho sum_{i<n} y^(pn-1-i) wR_i wL_i  (= c' delta / U; plain partial sums, block reduction)
  {
    scl part = scl_zero();
    uint32_t cnt = 0;
    for (uint32_t i = t; i < sh.n; i += nt) {
      scl a, b, c;
      ld_scl8(a, yip + 8 * (sh.pn - 1 - i)); ld_scl(b, wR + SW * i); ld_scl(c, wL + SW * i);
      part = scl_add(part, scl_mul(scl_mul(b, c), a));
      if (++cnt == 32) { part = scl_weak(part); cnt = 1; }
    }
    part = wave_sum_scl(scl_weak(part));          // <= 32 products, limbs < 2^31
    if ((t & 63) == 63) st_scl(red + SW * (1 + (t >> 6)), part);
    if (t >= nt - 2) {                            // c' = U rho Y | a P1 rho Y, both plain (rho Y = yip[pn-1] is plain)
      const bool second = t == nt - 1;
      scl a, b;
      ld_scl8(a, yip + 8 * (sh.pn - 1));
      ld_scl(b, second ? shr + 1 * SW : chs + 6 * SW);
      st_scl(shr + (second ? 4 : 3) * SW, scl_mul(b, a));
      if (!second) st_scl(shr + 6 * SW, a);       // rho Y, unpacked
    }
    __syncthreads();
    if (t == 0) {                                 // the sum, converted plain -> Montgomery
      const uint32_t z = lane_zero();
      scl tot = scl_zero();
      for (uint32_t wI = 0; wI < (nt >> 6); ++wI) { scl v; ld_scl(v, red + SW * (1 + wI) + z); tot = scl_add(tot, v); }
      st_scl(red, scl_mul(scl_weak(tot), scl_r2()));
    } else if (t >= nt - 6) {                     // c' in Montgomery form | the generator loop's factors times u
      const uint32_t w = nt - 1 - t;              // 0: c' R^2 | 1: (x U) u | 2: (a P1 rho Y) u | 3: (b P1) u | 4: U u | 5: c' u
      scl a, b;
      ld_scl(a, w == 0 || w == 5 ? shr + 3 * SW : w == 1 ? shr + 0 * SW : w == 2 ? shr + 4 * SW : w == 3 ? shr + 2 * SW : chs + 6 * SW);
      ld_scl(b, chs + 2 * SW);
      const scl r2 = scl_r2();
#pragma unroll
      for (int q = 0; q < 10; ++q) b.v[q] = w == 0 ? r2.v[q] : b.v[q];
      st_scl(shr + (w == 0 ? 5 : 7 + w) * SW, scl_mul(a, b));
    }
    __syncthreads();
  }
  uint32_t* ds = dyn_scalars + stm.dyn * 8;
  uint32_t* ss = static_scalars + stm.st * 8;
  uint32_t* sx = static_index + stm.st;            // the generators of this statement's static terms
  if (t == 0) { sx[0] = 0; sx[1] = 1; }
  // ---- proof-point scalars, B and B_blinding: the last wavefront, BEFORE its share of the generator scalars, so that
  // this short serial tail runs beside the other wavefronts' generator loop instead of after it.  Every lane does the
  // same two rounds v = a * b with operands of its own, read from LDS where they are needed (a lane that needs fewer
  // rounds passes its value through), and the conversion; the scalar of B is spread over four lanes: with c' delta = U dsum,
  //     c' (w (t_x - a b) + r (x^2 (wc + delta) - t_x))  =  c' [w (t_x - [a b])]  +  [r x^2] ([c' wc] + [U dsum]) - r [c' t_x]
  // lane jB: a b, then w (t_x - .), converted TIMES the plain c';  jB+1: c' wc, then r x^2 (. + U dsum), minus jB+3's product,
  // converted;  jB+2: U dsum;  jB+3: c' t_x, then r (.);  the partial results travel by wavefront shuffles and the two halves
  // are added as plain values.  The factor c' of everything else rides on the final Montgomery -> plain conversion too (a
  // product with the plain c' instead of with 1).
  const uint32_t tail0 = nt - 64;
  if (t >= tail0) {
    const uint32_t lane = t - tail0, n_dyn = sh.n_dyn;
    const uint32_t* const p_u = chs + 2 * SW;
    const uint32_t* const p_x = chs + 3 * SW;
    const uint32_t* const p_U = chs + 6 * SW;
    const uint32_t* const p_r = chs + 7 * SW;
    const uint32_t* const p_cp = shr + 5 * SW;     // c', Montgomery
    // positions: 0 B (a b ..), 1 B's second half (c' wc ..), 2 U dsum, 3 c' t_x, 4 B_blinding, 5 + j the proof point j
#pragma unroll 1
    for (uint32_t pos0 = 0; pos0 < n_dyn + 5; pos0 += 64) {
      const uint32_t pos = pos0 + lane;
      const uint32_t j = pos - 5;                 // proof-point index when pos >= 5
      const uint32_t* pa = p_x;
      const uint32_t* pb = p_x;
      const uint32_t* pconv = shr + 3 * SW;       // c', plain
      bool m1 = true;                             // does round 1 multiply?  (otherwise v = a)
      if (pos == 0) { pa = chs + 11 * SW; pb = chs + 12 * SW; }                                              // a b
      else if (pos == 1) { pa = p_cp; pb = wc; }                                                             // c' wc
      else if (pos == 2) { pa = p_U; pb = red; }                                                             // U dsum
      else if (pos == 3) { pa = p_cp; pb = chs + 8 * SW; }                                                   // c' t_x
      else if (pos == 4) { pa = p_r; pb = chs + 9 * SW; }                                                    // r t_x_blinding
      else if (j < 3) { if (j) pa = xp + (j - 1) * SW; m1 = false; }                                         // x, x^2, x^3
      else if (j < 6) { if (j > 3) pa = xp + (j - 4) * SW; pb = p_u; }                                       // u x^(1..3)
      else if (j < 6 + sh.m) { pa = wV + SW * (j - 6); pb = xp + 5 * SW; }                                   // wV_j r x^2
      else if (j < 11 + sh.m) {                                                                              // r x, r x^3 .. r x^6
        const uint32_t q = j - 6 - sh.m;
        if (q) pa = xp + q * SW;
        pb = p_r;
      } else if (j < n_dyn) {
        const uint32_t q = j - 11 - sh.m;         // u_j^2 for L_j; for R_j  c' u_j^-2 = rho Y prod_{l != j} u_l^2
        if (q < sh.k) { pa = pb = chs + (CH_FIXED + sh.n_chal2 + q) * SW; }
        else { pa = chs + (CH_FIXED + sh.n_chal2 + sh.k + (q - sh.k)) * SW; pconv = shr + 6 * SW; m1 = false; }
      } else m1 = false;
      scl a, b, v;
      ld_scl(a, pa); ld_scl(b, pb);
      v = a;
      {
        const scl pr = scl_mul(a, b);
        if (m1) v = pr;
      }
      if (pos0 == 0) {                            // round 2: the scalars of B and B_blinding (first pass only, lanes 0..4)
        scl other = shfl_down_scl(v, 1);
        bool m2 = false;
        if (pos == 0) { scl tx_; ld_scl(tx_, chs + 8 * SW); ld_scl(a, chs + 4 * SW); b = scl_sub(tx_, v); m2 = true; }       // w (t_x - a b)
        else if (pos == 1) { ld_scl(a, xp + 5 * SW); b = scl_add(v, other); m2 = true; }                                      // r x^2 (c' wc + U dsum)
        else if (pos == 3) { ld_scl(a, p_r); b = v; m2 = true; }                                                             // r c' t_x
        else if (pos == 4) { scl e; ld_scl(e, chs + 10 * SW); scl sum = scl_add(e, v); scl_carry(sum); v = scl_neg(sum); }    // -(e_blinding + r t_x_blinding)
        const scl pr2 = scl_mul(a, b);
        if (m2) v = pr2;
        other = shfl_down_scl(v, 2);
        if (pos == 1) { v = scl_sub(v, other); pconv = shr + 7 * SW; }                // r (x^2 (..) - c' t_x), converted as it is
      }                                                                               // (lane 0: w (t_x - a b), converted times c')
      scl conv_by;
      ld_scl(conv_by, pconv);
      scl plain = scl_mul(v, conv_by);            // Montgomery -> plain, times the plain factor
      if (pos0 == 0) {                            // B's two halves meet as plain values
        const scl other = shfl_down_scl(plain, 1);
        if (pos == 0) plain = scl_add(plain, other);
      }
      uint32_t o[8];
      scl_canon_words(o, plain);
      if (pos >= 5 && j < n_dyn) {
        // the scalar (k_small_tables recodes it for k_small_accumulate)
#pragma unroll
        for (int q = 0; q < 8; ++q) ds[j * 8 + q] = o[q];
      } else if (pos == 0 || pos == 4) {
#pragma unroll
        for (int q = 0; q < 8; ++q) ss[(pos == 0 ? 0 : 1) * 8 + q] = o[q];
      }
    }
  }
  // generator scalars (times c'), reduced to canonical words at the very end:
  //   c' g_i = (x U) wR_i yp[pn-1-i] - (a P1 rho Y) sU_i
  //   c' h_i = yp[pn-1-i] ((x U) wL_i + U wO_i - (b P1) sU_(pn-1-i)) - c'        (times u for i >= n1)
  {
    // the factors the whole workgroup shares live in scalar registers.  For i >= n1 (second-phase multipliers and the padding)
    // both scalars carry the factor u: a wavefront whose lanes are all there reads the copies that already carry it (slots
    // 8 .. 12: two products less per i), a mixed one multiplies at the end.  (Read per lane from LDS, whichever copy the lane
    // needs, the factors take 50 vector registers more and the kernel spills.)
    for (uint32_t i = t; i < sh.pn; i += nt) {
      const bool hi = i >= sh.n1;
      const bool with_u = __builtin_amdgcn_readfirstlane((int)__all(hi)) != 0;
      const uint32_t* const f = shr + 8 * SW;
      scl xU, aY_plain, bP, U, cp_plain;
      ld_scl_shared(xU, with_u ? f + 0 * SW : shr + 0 * SW); ld_scl_shared(aY_plain, with_u ? f + 1 * SW : shr + 4 * SW);
      ld_scl_shared(bP, with_u ? f + 2 * SW : shr + 2 * SW); ld_scl_shared(U, with_u ? f + 3 * SW : chs + 6 * SW);
      ld_scl_shared(cp_plain, with_u ? f + 4 * SW : shr + 3 * SW);
      scl yp, si, sr;
      ld_scl8(yp, yip + 8 * (sh.pn - 1 - i)); ld_scl8(si, sv + 8 * i); ld_scl8(sr, sv + 8 * (sh.pn - 1 - i));
      scl g = scl_neg(scl_mul(aY_plain, si));                 // limbs < 2^27.6, value < 2^260.1
      scl inner = scl_neg(scl_mul(bP, sr));
      if (i < sh.n) {
        scl wl, wr, wo;
        ld_scl(wl, wL + SW * i); ld_scl(wr, wR + SW * i); ld_scl(wo, wO + SW * i);
        g = scl_add(g, scl_mul(scl_mul(xU, wr), yp));
        inner = scl_add(inner, scl_add(scl_mul(xU, wl), scl_mul(U, wo)));   // limbs < 2^28, value < 2^260.2
      }
      scl h = scl_sub(scl_mul(yp, inner), cp_plain);          // yp, c' tight and < 2^255
      if (!with_u && __any(hi)) {                             // (a wavefront that straddles n1)
        scl u;
        ld_scl_shared(u, chs + 2 * SW);
        const scl gu = scl_mul(g, u), hu = scl_mul(h, u);
        if (hi) { g = gu; h = hu; }
      }
      uint32_t gw[8], hw[8];
      scl_canon_words(gw, g);
      scl_canon_words(hw, h);
      uint4* og = reinterpret_cast<uint4*>(ss + (2 + i) * 8);
      uint4* oh = reinterpret_cast<uint4*>(ss + (2 + sh.pn + i) * 8);
      og[0] = make_uint4(gw[0], gw[1], gw[2], gw[3]); og[1] = make_uint4(gw[4], gw[5], gw[6], gw[7]);
      oh[0] = make_uint4(hw[0], hw[1], hw[2], hw[3]); oh[1] = make_uint4(hw[4], hw[5], hw[6], hw[7]);
      sx[2 + i] = 2 + i;
      sx[2 + sh.pn + i] = pln.h_base + i;
    }
  }
}

// ---- k_mx_gather_dyn_points: one workgroup per statement, its proof-specific points in the order of its dynamic terms
// [A_I1 A_O1 S1 A_I2 A_O2 S2 | V.. | T_1 T_3 T_4 T_5 T_6 | L.. | R..] (compressed; decoded by the MSM's k_decompress)
__global__ void __launch_bounds__(256)
k_mx_gather_dyn_points(const MixPlan* __restrict__ plans, const MixStmt* __restrict__ stmts, const uint32_t* __restrict__ order,
                       const uint32_t* __restrict__ com, const uint32_t* __restrict__ pw, uint32_t* __restrict__ dyn_points) {
  const MixStmt& stm = stmts[order[blockIdx.x]];
  const PrepShape& sh = plans[stm.plan].sh;
  const uint32_t* p = pw + stm.pw;
  const uint32_t* c = com + stm.com;
  for (uint32_t g = threadIdx.x; g < sh.n_dyn * 8; g += blockDim.x) {
    const uint32_t q = g & 7, j = g >> 3;
    const uint32_t* src;
    if (j < 6) src = p + 8 * j;
    else if (j < 6 + sh.m) src = c + 8 * (j - 6);
    else if (j < 11 + sh.m) src = p + 8 * (6 + (j - 6 - sh.m));
    else {
      const uint32_t r = j - 11 - sh.m;
      src = p + 112 + (r < sh.k ? 16 * r : 16 * (r - sh.k) + 8);
    }
    dyn_points[stm.dyn * 8 + g] = src[q];
  }
}

// large_prep.hpp's kernels over the statements of a mixed call whose plans exceed a CU's LDS: launch statement b is
// order[b]; they write the generator index too, and no recoded form (k_small_tables makes it in mixed calls)
struct LpMixed {
  const MixPlan* plans;
  const MixStmt* stmts;
  const uint32_t* order;
  const uint32_t* ch;
  uint32_t* dyn_scalars;
  uint32_t* static_scalars;
  uint32_t* static_index;
  __device__ LpStmt at(uint32_t b) const {
    const MixStmt& stm = stmts[order[b]];
    const MixPlan& pln = plans[stm.plan];
    return {pln.sh, pln.tgt_off, pln.term_info, pln.prod_qm, pln.prod_coef, ch + stm.ch, dyn_scalars + stm.dyn * 8, nullptr,
            static_scalars + stm.st * 8, static_index + stm.st, pln.h_base};
  }
};

}  // namespace zk
