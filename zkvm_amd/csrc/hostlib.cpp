// hostlib.cpp -- the host-only part of the product (scalar field, Merlin transcript,
// R1CS verifier scalar preparation) as a plain C++ shared library, so that the CPU test
// tier can exercise it without a GPU.  libzkgpu.so compiles the very same headers.
#include "r1cs_verifier.hpp"
#include "cloak_plan.hpp"
#include "curve.hpp"
#include "r1cs_prover.hpp"
#include "transcript_tape.hpp"
#include "keccak_coop.hpp"
#include "prover_plan.hpp"
#include "prover_call_plan.hpp"
#include "zkvm_tx.hpp"

#include <array>
#include <map>

#include <cstring>

using namespace zk;

extern "C" {

// op: 0 add, 1 sub, 2 mul, 3 neg(a), 4 invert(a), 5 reduce only; inputs are 64-byte wide values
int zkhost_scalar_op(int op, const uint8_t a64[64], const uint8_t b64[64], uint8_t out[32]) {
  const Scalar a = Scalar::from_wide(a64), b = Scalar::from_wide(b64);
  Scalar r;
  switch (op) {
    case 0: r = a + b; break;
    case 1: r = a - b; break;
    case 2: r = a * b; break;
    case 3: r = -a; break;
    case 4: r = a.invert(); break;
    case 5: r = a; break;
    default: return -1;
  }
  r.to_bytes(out);
  return 0;
}

int zkhost_scalar_is_canonical(const uint8_t b[32]) {
  Scalar s;
  return Scalar::from_canonical(b, s) ? 1 : 0;
}

// Transcript::new(label); n x append_message(labels[i], msgs[i]); challenge_bytes(ch_label, out)
int zkhost_merlin(const char* label, int n, const char* const* labels, const uint8_t* const* msgs, const size_t* lens,
                  const char* ch_label, uint8_t* out, size_t out_len) {
  Transcript t(label);
  for (int i = 0; i < n; ++i) t.append_message(labels[i], msgs[i], lens[i]);
  t.challenge_bytes(ch_label, out, out_len);
  return 0;
}

// cloak::prepare_tx; buffers sized by the caller: dyn 32 * 64 each, static 32 * (2 + 2 * cap), index 4 * (2 + 2 * cap)
int zkhost_cloak_prepare(const uint8_t* commitments, size_t n_in, size_t n_out, const uint8_t* proof, size_t proof_len,
                         const uint8_t r64[64], size_t gens_capacity, uint8_t* dyn_scalars, uint8_t* dyn_points,
                         size_t* n_dyn, uint8_t* static_scalars, uint32_t* static_index, size_t* n_static,
                         size_t* padded_n) {
  VerifierMsm m;
  if (!cloak::prepare_tx(commitments, n_in, n_out, proof, proof_len, Scalar::from_wide(r64), gens_capacity, m)) return 1;
  *n_dyn = m.dyn_scalars.size() / 32;
  *n_static = m.static_scalars.size() / 32;
  *padded_n = m.padded_n;
  std::memcpy(dyn_scalars, m.dyn_scalars.data(), m.dyn_scalars.size());
  std::memcpy(dyn_points, m.dyn_points.data(), m.dyn_points.size());
  std::memcpy(static_scalars, m.static_scalars.data(), m.static_scalars.size());
  std::memcpy(static_index, m.static_index.data(), m.static_index.size() * 4);
  return 0;
}

// A constraint system described as data (include/zkgpu.h, zkgpu_r1cs_desc) through the host verifier:
// same argument conventions as zkgpu_r1cs_plan_create; output as zkhost_cloak_prepare.
int zkhost_r1cs_prepare(const char* label, uint32_t m, uint32_t n1, uint32_t n, uint32_t n_chal, const char* const* chal_labels,
                        uint32_t n_cons, const uint64_t* term_offsets, const uint8_t* kinds, const uint32_t* idx,
                        const uint8_t* coeff, const int32_t* chal, const uint32_t* power, const uint8_t* commitments,
                        const uint8_t* proof, size_t proof_len, const uint8_t r64[64], size_t gens_capacity,
                        uint8_t* dyn_scalars, uint8_t* dyn_points, size_t* n_dyn, uint8_t* static_scalars,
                        uint32_t* static_index, size_t* n_static, size_t* padded_n) {
  R1csDesc d;
  d.label = label; d.m = m; d.n1 = n1; d.n = n;
  for (uint32_t i = 0; i < n_chal; ++i) d.chal_names.push_back(chal_labels[i]);
  for (uint32_t q = 0; q < n_cons; ++q) {
    std::vector<R1csDesc::Term> con;
    for (uint64_t t = term_offsets[q]; t < term_offsets[q + 1]; ++t) {
      Scalar c;
      if (kinds[t] > 4 || !Scalar::from_canonical(coeff + 32 * t, c)) return -1;
      con.push_back(R1csDesc::Term{(VarKind)kinds[t], idx[t], c, chal[t], power[t]});
    }
    d.cons.push_back(std::move(con));
  }
  try { (void)plan_from_desc(d); } catch (const std::exception&) { return -1; }
  VerifierMsm msm;
  if (!prepare_desc(d, commitments, proof, proof_len, Scalar::from_wide(r64), gens_capacity, msm)) return 1;
  *n_dyn = msm.dyn_scalars.size() / 32;
  *n_static = msm.static_scalars.size() / 32;
  *padded_n = msm.padded_n;
  std::memcpy(dyn_scalars, msm.dyn_scalars.data(), msm.dyn_scalars.size());
  std::memcpy(dyn_points, msm.dyn_points.data(), msm.dyn_points.size());
  std::memcpy(static_scalars, msm.static_scalars.data(), msm.static_scalars.size());
  std::memcpy(static_index, msm.static_index.data(), msm.static_index.size() * 4);
  return 0;
}

// Keccak-f[1600] through the emulated wavefront of keccak_coop.hpp (the algorithm k_transcript_coop runs)
// The lazy scalar form of sc_dev.hpp (scl) against the canonical one (scm) on pseudo-random chains of operations:
// returns the number of mismatches (tests/test_host_logic.py expects 0).
uint64_t zkhost_scl_selftest(uint64_t seed, uint32_t rounds) {
  uint64_t st = seed ? seed : 1, bad = 0;
  auto rnd = [&st]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (uint32_t)(st >> 16); };
  auto rnd_scm = [&]() {
    uint32_t w[16];
    for (auto& x : w) x = rnd();
    return scm_from_wide(w);
  };
  auto same = [](const scm& a, const scl& b) {
    uint32_t w[8];
    scl_canon_words(w, b);
    bool ok = true;
    for (int i = 0; i < 8; ++i) ok &= w[i] == a.v[i];
    return ok;
  };
  for (uint32_t r = 0; r < rounds; ++r) {
    scm a = rnd_scm(), b = rnd_scm(), c = rnd_scm();
    if (r == 0) { a = scm_zero(); }
    if (r == 1) { b = scm_neg(scm_one()); c = b; a = b; }
    const scl la = scl_from_scm(a), lb = scl_from_scm(b), lc = scl_from_scm(c);
    if (!same(scm_mul(a, b), scl_mul(la, lb))) ++bad;
    if (!same(scm_add(a, b), scl_add(la, lb))) ++bad;
    if (!same(scm_sub(a, b), scl_sub(la, lb))) ++bad;
    if (!same(scm_neg(a), scl_neg(la))) ++bad;
    // (a - b) (c - a) + sum of 16 products - b, everything lazy
    scm acc = scm_mul(scm_sub(a, b), scm_sub(c, a));
    scl lacc = scl_mul(scl_sub(la, lb), scl_sub(lc, la));
    scm x = a; scl lx = la;
    for (int i = 0; i < 16; ++i) {
      x = scm_mul(x, c); lx = scl_mul(lx, lc);
      const bool neg = rnd() & 1;
      acc = neg ? scm_sub(acc, x) : scm_add(acc, x);
      lacc = scl_add(lacc, scl_cneg(lx, neg));
    }
    acc = scm_sub(acc, b); lacc = scl_sub(lacc, lb);
    if (!same(acc, lacc)) ++bad;
    if (!same(acc, scl_weak(lacc))) ++bad;
    if (!same(scm_mul(acc, a), scl_mul(lacc, la))) ++bad;
    // the Euclidean inverse of the device prover against Fermat's
    {
      const scm inv_f = scm_invert(a), inv_e = pv_invert(a), inv_u = pv_invert_uniform(a);
      for (int i = 0; i < 8; ++i) if (inv_f.v[i] != inv_e.v[i]) { ++bad; break; }
      for (int i = 0; i < 8; ++i) if (inv_f.v[i] != inv_u.v[i]) { ++bad; break; }
    }
    // plain <-> Montgomery
    uint32_t plain[8];
    scm_to_words(plain, a);
    const scl lp = scl_mul(la, scl_plain_one());
    uint32_t w[8];
    scl_canon_words(w, lp);
    for (int i = 0; i < 8; ++i) if (w[i] != plain[i]) { ++bad; break; }
    if (!same(a, scl_mul(lp, scl_r2()))) ++bad;
    if (!same(scm_one(), scl_one())) ++bad;
    // wave-tree shape: 64 values added with a carry after each doubling
    scl tree = lx; scm stree = x;
    for (int i = 0; i < 6; ++i) { tree = scl_add_c(tree, tree); stree = scm_add(stree, stree); }
    if (!same(stree, tree)) ++bad;
  }
  return bad;
}

void zkhost_keccak_coop(uint64_t state[25]) { coop::keccak_f1600_emulated(state); }

// The cooperative form of the transcript on the host: the tape regrouped into segments
// (build_coop_segments), each word's absorbed bytes gathered as k_tape_gather does, the state spread over
// an emulated wavefront as in k_transcript_coop.  out: 32-byte challenge scalars in the order of
// zkhost_tape_challenges; returns their count or -1.
int zkhost_coop_challenges(uint32_t n_in, uint32_t n_out, const uint8_t* commitments, const uint8_t* proof,
                           size_t proof_len, uint8_t* out, size_t capacity) {
  const CloakPlan plan = PlanBuilder::build(n_in, n_out);
  const uint32_t m = plan.m, k = plan.k, n_chal2 = (uint32_t)plan.chal_names.size();
  if (proof_len != 1 + 32ull * (16 + 2 * k)) return -1;
  const uint32_t ch_fixed = 14;
  Transcript tr("ZkVM.r1cs");
  tr.append_message("dom-sep", (const uint8_t*)"r1cs v1", 7);
  uint32_t init[52];
  tr.export_state(init);
  const std::vector<uint32_t> tape = build_r1cs_verifier_tape(init[50], init[51], m, plan.chal_names, k, plan.pn, ch_fixed);
  const CoopSegments segs = build_coop_segments(tape, m);
  if (!segs.n_seg()) return -1;
  using KC = coop::KeccakCoop<coop::HostTraits>;
  const auto consts = coop::host_consts();
  coop::LaneVec lo, hi;
  for (uint32_t i = 0; i < 64; ++i) {
    const coop::KcLane kl = coop::kc_lane(i);
    lo.l[i] = kl.live ? init[2 * kl.q] : 0;
    hi.l[i] = kl.live ? init[2 * kl.q + 1] : 0;
  }
  std::map<uint32_t, std::vector<uint8_t>> got;
  for (uint32_t sgm = 0; sgm < segs.n_seg(); ++sgm) {
    const uint32_t info = segs.info[sgm], slot = info & 0xffffu;
    if (slot) {
      std::vector<uint8_t> bytes(64);
      for (uint32_t i = 0; i < 64; ++i) {
        const coop::KcLane kl = coop::kc_lane(i);
        if (kl.primary && kl.q < 8) { std::memcpy(&bytes[8 * kl.q], &lo.l[i], 4); std::memcpy(&bytes[8 * kl.q + 4], &hi.l[i], 4); }
        if (kl.live && kl.q < 8) { lo.l[i] = 0; hi.l[i] = 0; }
      }
      got[slot - 1] = bytes;
    }
    for (uint32_t i = 0; i < 64; ++i) {
      const coop::KcLane kl = coop::kc_lane(i);
      if (!kl.live) continue;
      uint64_t w = (uint64_t)segs.consts[sgm * 50 + 2 * kl.q] | ((uint64_t)segs.consts[sgm * 50 + 2 * kl.q + 1] << 32);
      for (int b = 0; b < 8; ++b) {
        const uint32_t idx = segs.map[sgm * 200 + 8 * kl.q + b];
        if (idx) { const uint32_t j = idx - 1; w ^= (uint64_t)(j < 32 * m ? commitments[j] : proof[1 + j - 32 * m]) << (8 * b); }
      }
      lo.l[i] ^= (uint32_t)w; hi.l[i] ^= (uint32_t)(w >> 32);
    }
    if (info >> 31) KC::permute(lo, hi, consts);
  }
  std::vector<uint32_t> order = {0, 1, 2, 3, 4};
  for (uint32_t j = 0; j < n_chal2; ++j) order.push_back(ch_fixed + j);
  for (uint32_t j = 0; j < k; ++j) order.push_back(ch_fixed + n_chal2 + j);
  if (order.size() > capacity) return -1;
  for (size_t i = 0; i < order.size(); ++i) {
    if (!got.count(order[i])) return -1;
    Scalar::from_wide(got[order[i]].data()).to_bytes(out + 32 * i);
  }
  return (int)order.size();
}

// The device-side transcript tape (transcript_tape.hpp) against the Transcript class on the same
// proof: out_tape / out_direct receive 32-byte challenge scalars in slot order y z u x w, the
// second-phase challenges, the k inner-product challenges.  Returns their count, or -1.
int zkhost_tape_challenges(uint32_t n_in, uint32_t n_out, const uint8_t* commitments, const uint8_t* proof,
                           size_t proof_len, uint8_t* out_tape, uint8_t* out_direct, size_t capacity) {
  const CloakPlan plan = PlanBuilder::build(n_in, n_out);
  const uint32_t m = plan.m, k = plan.k, n_chal2 = (uint32_t)plan.chal_names.size();
  if (proof_len != 1 + 32ull * (16 + 2 * k)) return -1;
  const uint32_t ch_fixed = 14;
  Transcript tr("ZkVM.r1cs");
  tr.append_message("dom-sep", (const uint8_t*)"r1cs v1", 7);
  uint32_t init[52];
  tr.export_state(init);
  const std::vector<uint32_t> tape = build_r1cs_verifier_tape(init[50], init[51], m, plan.chal_names, k, plan.pn, ch_fixed);
  uint8_t state[200];
  std::memcpy(state, init, 200);
  std::map<uint32_t, std::vector<uint8_t>> got;
  run_tape_host(tape, state, commitments, proof + 1, [](uint8_t* st) {
    uint64_t a[25];
    std::memcpy(a, st, 200);
    keccak_f1600(a);
    std::memcpy(st, a, 200);
  }, got);
  std::vector<uint32_t> order = {0, 1, 2, 3, 4};
  for (uint32_t j = 0; j < n_chal2; ++j) order.push_back(ch_fixed + j);
  for (uint32_t j = 0; j < k; ++j) order.push_back(ch_fixed + n_chal2 + j);
  if (order.size() > capacity) return -1;
  for (size_t i = 0; i < order.size(); ++i) {
    if (!got.count(order[i])) return -1;
    Scalar::from_wide(got[order[i]].data()).to_bytes(out_tape + 32 * i);
  }
  // the same sequence through the Transcript class
  const uint8_t* f = proof + 1;
  std::vector<Scalar> direct(order.size());
  for (uint32_t i = 0; i < m; ++i) tr.append_message("V", commitments + 32 * i, 32);
  {
    uint8_t b[8] = {0};
    for (int q = 0; q < 8; ++q) b[q] = (uint8_t)((uint64_t)m >> (8 * q));
    tr.append_message("m", b, 8);
  }
  tr.append_message("A_I1", f, 32); tr.append_message("A_O1", f + 32, 32); tr.append_message("S1", f + 64, 32);
  if (n_chal2 == 0) {
    tr.append_message("dom-sep", (const uint8_t*)"r1cs-1phase", 11);
  } else {
    tr.append_message("dom-sep", (const uint8_t*)"r1cs-2phase", 11);
    for (uint32_t j = 0; j < n_chal2; ++j) {
      direct[5 + j] = tr.challenge_scalar(plan.chal_names[j].c_str());
    }
  }
  tr.append_message("A_I2", f + 96, 32); tr.append_message("A_O2", f + 128, 32); tr.append_message("S2", f + 160, 32);
  direct[0] = tr.challenge_scalar("y");
  direct[1] = tr.challenge_scalar("z");
  const char* tl[5] = {"T_1", "T_3", "T_4", "T_5", "T_6"};
  for (int i = 0; i < 5; ++i) tr.append_message(tl[i], f + 32 * (6 + i), 32);
  direct[2] = tr.challenge_scalar("u");
  direct[3] = tr.challenge_scalar("x");
  tr.append_message("t_x", f + 32 * 11, 32);
  tr.append_message("t_x_blinding", f + 32 * 12, 32);
  tr.append_message("e_blinding", f + 32 * 13, 32);
  direct[4] = tr.challenge_scalar("w");
  tr.append_message("dom-sep", (const uint8_t*)"ipp v1", 6);
  {
    uint8_t b[8] = {0};
    for (int q = 0; q < 8; ++q) b[q] = (uint8_t)((uint64_t)plan.pn >> (8 * q));
    tr.append_message("n", b, 8);
  }
  for (uint32_t j = 0; j < k; ++j) {
    tr.append_message("L", f + 32 * (14 + 2 * j), 32);
    tr.append_message("R", f + 32 * (14 + 2 * j + 1), 32);
    direct[5 + n_chal2 + j] = tr.challenge_scalar("u");
  }
  for (size_t i = 0; i < order.size(); ++i) direct[i].to_bytes(out_direct + 32 * i);
  return (int)order.size();
}

}  // extern "C"

namespace {
// Reference evaluation of prover rows on the host (CPU tests only; the product evaluates them with
// zkgpu_msm_ps_batch): bucket method over decoded generator points, window 8 -- 4 for the rows of a few terms (value
// commitments, T_i), where walking 255 buckets per window was nearly all of the work.
void host_rows(const std::vector<ge>& gens, const std::vector<MsmRow>& rows, std::vector<uint8_t>& out) {
  out.assign(32 * rows.size(), 0);
  for (size_t r = 0; r < rows.size(); ++r) {
    const MsmRow& row = rows[r];
    ge acc;
    ge_identity(acc);
    std::vector<std::array<uint8_t, 32>> sb(row.scalars.size());
    for (size_t i = 0; i < sb.size(); ++i) row.scalars[i].to_bytes(sb[i].data());
    const int c = sb.size() <= 16 ? 4 : 8, n_buckets = 1 << c;
    for (int win = 256 / c - 1; win >= 0; --win) {
      for (int d = 0; d < c; ++d) ge_double(acc, acc);
      std::vector<ge> bucket(n_buckets);
      std::vector<char> used(n_buckets, 0);
      for (size_t i = 0; i < sb.size(); ++i) {
        const unsigned b = c == 8 ? sb[i][win] : (sb[i][win >> 1] >> (4 * (win & 1))) & 15u;
        if (!b) continue;
        if (used[b]) ge_add(bucket[b], bucket[b], gens[row.index[i]]);
        else { bucket[b] = gens[row.index[i]]; used[b] = 1; }
      }
      ge run, sum;
      ge_identity(run);
      ge_identity(sum);
      for (int b = n_buckets - 1; b >= 1; --b) {
        if (used[b]) ge_add(run, run, bucket[b]);
        ge_add(sum, sum, run);
      }
      ge_add(acc, acc, sum);
    }
    uint32_t enc[8];
    ristretto_encode(enc, acc);
    std::memcpy(&out[32 * r], enc, 32);
  }
}
}  // namespace

extern "C" {

// One cloak proof on the host: the product's prover (r1cs_prover.hpp) with its rows evaluated by the
// reference MSM above.  generators = [B, B_blinding, G_0..G_{cap-1}, H_0..H_{cap-1}] compressed.
// Returns 0; commitments = 64 (n_in + n_out) bytes, proof_len_out = bytes written to proof.
int zkhost_cloak_prove(uint32_t n_in, uint32_t n_out, const uint64_t* quantities, const uint8_t* flavors,
                       const uint8_t seed[32], const uint8_t* generators, size_t gens_capacity, uint8_t* commitments,
                       uint8_t* proof, size_t proof_cap, size_t* proof_len_out, size_t* multipliers) {
  std::vector<ge> gens(2 + 2 * gens_capacity);
  for (size_t i = 0; i < gens.size(); ++i) {
    uint32_t w[8];
    std::memcpy(w, generators + 32 * i, 32);
    if (!ristretto_decode(gens[i], w)) return -1;
  }
  std::unique_ptr<R1csProver> prp = cloak_prover(n_in, n_out, quantities, flavors, seed, gens_capacity);
  R1csProver& pr = *prp;
  std::vector<MsmRow> rows;
  std::vector<uint8_t> pts;
  pr.begin(rows);
  while (!pr.done()) {
    host_rows(gens, rows, pts);
    pr.step(pts.data(), rows);
  }
  if (pr.failed() || pr.proof().size() > proof_cap) return -2;
  std::memcpy(commitments, pr.commitments().data(), pr.commitments().size());
  std::memcpy(proof, pr.proof().data(), pr.proof().size());
  *proof_len_out = pr.proof().size();
  if (multipliers) *multipliers = pr.multipliers();
  return 0;
}

// The prover for a constraint system described as data (desc_prover) with the reference MSM of this library:
// description arrays as zkhost_r1cs_prepare; mult_def: 2 per multiplier; values: m x 32 bytes; given: n_given x 64
// bytes (left, right); blindings derived from the seed as oracle/gadgets.c does ("blinding", i).
int zkhost_r1cs_prove(const char* label, uint32_t m, uint32_t n1, uint32_t n, uint32_t n_chal, const char* const* chal_labels,
                      uint32_t n_cons, const uint64_t* term_offsets, const uint8_t* kinds, const uint32_t* idx,
                      const uint8_t* coeff, const int32_t* chal, const uint32_t* power, const uint32_t* mult_def,
                      const uint8_t* values, const uint8_t* given, size_t n_given, const uint8_t seed[32],
                      const uint8_t* generators, size_t gens_capacity, uint8_t* commitments, uint8_t* proof, size_t proof_cap,
                      size_t* proof_len_out) {
  R1csDesc d;
  d.label = label; d.m = m; d.n1 = n1; d.n = n;
  for (uint32_t i = 0; i < n_chal; ++i) d.chal_names.push_back(chal_labels[i]);
  for (uint32_t q = 0; q < n_cons; ++q) {
    std::vector<R1csDesc::Term> con;
    for (uint64_t t = term_offsets[q]; t < term_offsets[q + 1]; ++t) {
      Scalar c;
      if (kinds[t] > 4 || !Scalar::from_canonical(coeff + 32 * t, c)) return -1;
      con.push_back(R1csDesc::Term{(VarKind)kinds[t], idx[t], c, chal[t], power[t]});
    }
    d.cons.push_back(std::move(con));
  }
  std::vector<ge> gens(2 + 2 * gens_capacity);
  for (size_t i = 0; i < gens.size(); ++i) {
    uint32_t w[8];
    std::memcpy(w, generators + 32 * i, 32);
    if (!ristretto_decode(gens[i], w)) return -1;
  }
  std::vector<Scalar> vals, bl;
  for (uint32_t i = 0; i < m; ++i) {
    uint8_t wide[64] = {0};
    std::memcpy(wide, values + 32 * i, 32);
    vals.push_back(Scalar::from_wide(wide));
    bl.push_back(R1csProver::derive_scalar(seed, "blinding", i));
  }
  std::vector<std::pair<Scalar, Scalar>> gv;
  for (size_t i = 0; i < n_given; ++i) {
    uint8_t wl[64] = {0}, wr[64] = {0};
    std::memcpy(wl, given + 64 * i, 32); std::memcpy(wr, given + 64 * i + 32, 32);
    gv.emplace_back(Scalar::from_wide(wl), Scalar::from_wide(wr));
  }
  std::vector<uint32_t> md(mult_def, mult_def + 2 * (size_t)n);
  std::unique_ptr<R1csProver> prp = desc_prover(d, md, vals, bl, gv, seed, gens_capacity);
  R1csProver& pr = *prp;
  std::vector<MsmRow> rows;
  std::vector<uint8_t> pts;
  pr.begin(rows);
  while (!pr.done()) {
    host_rows(gens, rows, pts);
    pr.step(pts.data(), rows);
  }
  if (pr.failed() || pr.proof().size() > proof_cap) return -2;
  std::memcpy(commitments, pr.commitments().data(), pr.commitments().size());
  std::memcpy(proof, pr.proof().data(), pr.proof().size());
  *proof_len_out = pr.proof().size();
  return 0;
}

}  // extern "C"

// ---- the DEVICE prover (prover_dev.hpp) run on the host with one "thread" per proof: the same phase functions the
// kernels call, the reference multiscalar multiplication of this library between them.  CPU tests compare the bytes
// with the host prover's and the oracle's.
namespace {
// pv_emulate's way through a phase: 0 the whole phase in one call (PV_ALL), 1 stage by stage in the device's order, the
// one-thread stages on an environment that inverts as the lane kernels do (zkhost_set_pv_staged; the CPU tests run both)
int g_pv_staged = 0;
struct PvHostEnv {
  static constexpr bool kInvertInEveryLane = false;
  uint32_t st[52];
  uint32_t tid() const { return 0; }
  uint32_t nt() const { return 1; }
  void sync() {}
  void sum(scl*, int) {}
  uint32_t* strobe() { return st; }
};

struct PvHostLaneEnv {          // what k_pv_lanes / k_pv_ipa_lanes give a proof: one thread, the fixed-chain inverse
  static constexpr bool kInvertInEveryLane = true;
  uint32_t st[52];
  uint32_t tid() const { return 0; }
  uint32_t nt() const { return 1; }
  void sync() {}
  void sum(scl*, int) {}
  uint32_t* strobe() { return st; }
};

void words_of(const uint8_t* b, size_t n_words, std::vector<uint32_t>& out) {
  for (size_t i = 0; i < n_words; ++i) out.push_back((uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24));
}
Scalar scalar_of_words(const uint32_t* w) {
  uint8_t wide[64] = {0};
  for (int i = 0; i < 8; ++i) for (int b = 0; b < 4; ++b) wide[4 * i + b] = (uint8_t)(w[i] >> (8 * b));
  return Scalar::from_wide(wide);
}
void rows_points(const std::vector<ge>& gens, const uint32_t* scalars, const PvRows& lay, std::vector<uint32_t>& out_words) {
  std::vector<MsmRow> rows(lay.offsets.size() - 1);
  for (size_t r = 0; r + 1 < lay.offsets.size(); ++r)
    for (uint64_t k = lay.offsets[r]; k < lay.offsets[r + 1]; ++k) rows[r].add(scalar_of_words(scalars + 8 * k), lay.index[k]);
  std::vector<uint8_t> pts;
  host_rows(gens, rows, pts);
  out_words.clear();
  words_of(pts.data(), pts.size() / 4, out_words);
}

int pv_emulate(const R1csDesc& d, const std::vector<uint32_t>& mult_def, const std::vector<uint32_t>& values, const std::vector<uint32_t>& blindings,
               const std::vector<uint32_t>& given, const uint8_t seed[32], const uint8_t* generators, size_t cap, uint8_t* commitments,
               uint8_t* proof, size_t proof_cap, size_t* proof_len_out) {
  std::vector<ge> gens(2 + 2 * cap);
  for (size_t i = 0; i < gens.size(); ++i) {
    uint32_t w[8];
    std::memcpy(w, generators + 32 * i, 32);
    if (!ristretto_decode(gens[i], w)) return -1;
  }
  PvHostPlan hp;
  try { hp = pv_build(d, mult_def, cap); } catch (const std::exception&) { return -3; }
  const PvShape& sh = hp.sh;
  if (given.size() != 16 * (size_t)sh.n_given || values.size() != 8 * (size_t)sh.m || sh.proof_len > proof_cap) return -4;
  const PvPlan P = hp.view();
  std::vector<uint32_t> state(sh.state_words, 0), rows0(16 * std::max<uint32_t>(sh.m, 1)), rows1(8 * std::max<uint32_t>(sh.r1_terms, 1)), rows2(8 * std::max<uint32_t>(sh.r2_terms, 1)),
      rows3(5 * 16), lv(8 * sh.pn), rv(8 * sh.pn), cg(8 * sh.pn), ch(8 * sh.pn), w(8), uu(16), rng_seed;
  uint8_t rs[32];
  R1csProver::derive(seed, "rng", 0, rs, 32);
  words_of(rs, 8, rng_seed);
  std::vector<uint8_t> pbytes(sh.proof_stride, 0);
  PvBatch B{};
  B.state = state.data(); B.values = values.data(); B.blindings = blindings.data(); B.given = given.empty() ? values.data() : given.data();
  B.rng_seed = rng_seed.data(); B.proofs = pbytes.data(); B.rows0 = rows0.data(); B.rows1 = rows1.data(); B.rows2 = rows2.data(); B.rows3 = rows3.data();
  B.ipa_lv = lv.data(); B.ipa_rv = rv.data(); B.ipa_cg = cg.data(); B.ipa_ch = ch.data(); B.ipa_w = w.data(); B.ipa_u = uu.data();
  PvHostEnv env;
  PvHostLaneEnv lane;
  std::vector<uint32_t> pts;
  uint32_t* const rows[4] = {rows0.data(), rows1.data(), rows2.data(), rows3.data()};
  auto msm = [&](uint32_t which, const PvRows& lay) {
    rows_points(gens, rows[which], lay, pts);
    if (which == 0) for (size_t i = 0; i < 8 * (size_t)sh.m; ++i) for (int b = 0; b < 4; ++b) commitments[4 * i + b] = (uint8_t)(pts[i] >> (8 * b));
  };
  auto stage = [&](auto& e, uint32_t phase, uint32_t st) {
    if (phase == 1) pv_phase1(e, sh, P, B, 0, pts.data(), st);
    else if (phase == 2) pv_phase2(e, sh, P, B, 0, pts.data(), st);
    else if (phase == 3) pv_phase3(e, sh, P, B, 0, pts.data(), st);
    else pv_phase4(e, sh, P, B, 0, pts.data(), st);
  };
  auto draws = [&](uint32_t phase) {
    if (phase == 1) pv_rng_draw(sh, state.data(), rows1.data(), 0, sh.n1, PV_IBL1); else pv_rng_draw(sh, state.data(), rows2.data(), sh.n1, sh.n, PV_IBL2);
  };
  if (g_pv_staged) {
    // the device's order: the steps prove_device walks, the rows of the plan for a batch of one
    const PvCallPlan plan = plan_prover_call(hp, 1, 1, {});
    for (const PvStep& s : plan.steps) switch (s.kind) {
      case PvStepKind::phase0: pv_phase0(env, sh, B, 0); break;
      case PvStepKind::msm: msm(s.phase, plan.rows_of((int)s.phase)); break;
      case PvStepKind::lanes: stage(lane, s.phase, s.mask); break;
      case PvStepKind::wg: stage(env, s.phase, s.mask); break;
      case PvStepKind::rng: draws(s.phase); break;
      case PvStepKind::ipa: case PvStepKind::finish: break;      // below, for both readings
    }
  } else {
    // the independent reading: every phase whole, in the order the protocol gives
    pv_phase0(env, sh, B, 0);
    msm(0, pv_rows_pairs(sh.m));
    stage(env, 1, PV_ALL); draws(1);
    msm(1, pv_rows_commit(1, 0, sh.n1, cap, false));
    stage(env, 2, PV_ALL); if (sh.n > sh.n1) draws(2);
    msm(2, pv_rows_commit(1, sh.n1, sh.n, cap, true));
    stage(env, 3, PV_ALL);
    msm(3, pv_rows_pairs(5));
    stage(env, 4, PV_ALL);
  }
  const bool staged = g_pv_staged != 0;
  if (state[sh.o_flag]) return -2 - (int)state[sh.o_flag];
  // the inner-product rounds (on the device: k_ipa_round + the tables); here with the host's scalars
  std::vector<Scalar> L(sh.pn), R(sh.pn), G(sh.pn), H(sh.pn);
  for (uint32_t i = 0; i < sh.pn; ++i) {
    uint32_t t[8];
    scm a; for (int q = 0; q < 8; ++q) a.v[q] = lv[8 * i + q];
    scm_to_words(t, a); L[i] = scalar_of_words(t);
    for (int q = 0; q < 8; ++q) a.v[q] = rv[8 * i + q];
    scm_to_words(t, a); R[i] = scalar_of_words(t);
    G[i] = scalar_of_words(&cg[8 * i]); H[i] = scalar_of_words(&ch[8 * i]);
  }
  const Scalar wq = scalar_of_words(w.data());
  size_t len = sh.pn;
  for (uint32_t round = 0; round < sh.k; ++round) {
    const size_t half = len / 2;
    Scalar cL = Scalar::zero(), cR = Scalar::zero();
    for (size_t j = 0; j < half; ++j) { cL += L[j] * R[half + j]; cR += L[half + j] * R[j]; }
    std::vector<MsmRow> rows(2);
    for (size_t idx = 0; idx < sh.pn; ++idx) {
      const size_t j = idx % len;
      const bool hi = j >= half;
      const size_t jj = hi ? j - half : j;
      if (hi) { rows[0].add(L[jj] * G[idx], (uint32_t)(2 + idx)); rows[1].add(R[jj] * H[idx], (uint32_t)(2 + cap + idx)); }
      else { rows[0].add(R[half + jj] * H[idx], (uint32_t)(2 + cap + idx)); rows[1].add(L[half + jj] * G[idx], (uint32_t)(2 + idx)); }
    }
    rows[0].add(cL * wq, 0);
    rows[1].add(cR * wq, 0);
    std::vector<uint8_t> lr;
    host_rows(gens, rows, lr);
    std::vector<uint32_t> lrw;
    words_of(lr.data(), 16, lrw);
    if (staged) pv_ipa_round(lane, sh, B, 0, round, lrw.data()); else pv_ipa_round(env, sh, B, 0, round, lrw.data());
    const Scalar u = scalar_of_words(uu.data()), ui = scalar_of_words(uu.data() + 8);
    for (size_t j = 0; j < half; ++j) {
      L[j] = L[j] * u + L[half + j] * ui;
      R[j] = R[j] * ui + R[half + j] * u;
    }
    for (size_t idx = 0; idx < sh.pn; ++idx) {
      const bool hi = (idx % len) >= half;
      G[idx] *= hi ? u : ui;
      H[idx] *= hi ? ui : u;
    }
    len = half;
  }
  uint8_t ab[64];
  L[0].to_bytes(ab); R[0].to_bytes(ab + 32);
  std::vector<uint32_t> abw;
  words_of(ab, 16, abw);
  pv_finish(sh, B, 0, abw.data());
  std::memcpy(proof, pbytes.data(), sh.proof_len);
  *proof_len_out = sh.proof_len;
  return 0;
}

// a constraint system handed over as arrays (the fields of zkgpu_r1cs_desc); false: a kind or a coefficient out of range
bool pv_desc_of(R1csDesc& d, const char* label, uint32_t m, uint32_t n1, uint32_t n, uint32_t n_chal, const char* const* chal_labels, uint32_t n_cons,
                const uint64_t* term_offsets, const uint8_t* kinds, const uint32_t* idx, const uint8_t* coeff, const int32_t* chal, const uint32_t* power) {
  d.label = label; d.m = m; d.n1 = n1; d.n = n;
  for (uint32_t i = 0; i < n_chal; ++i) d.chal_names.push_back(chal_labels[i]);
  for (uint32_t q = 0; q < n_cons; ++q) {
    std::vector<R1csDesc::Term> con;
    for (uint64_t t = term_offsets[q]; t < term_offsets[q + 1]; ++t) {
      Scalar c;
      if (kinds[t] > 4 || !Scalar::from_canonical(coeff + 32 * t, c)) return false;
      con.push_back(R1csDesc::Term{(VarKind)kinds[t], idx[t], c, chal[t], power[t]});
    }
    d.cons.push_back(std::move(con));
  }
  return true;
}
}  // namespace

extern "C" {
void zkhost_set_pv_staged(int on) { g_pv_staged = on; }
int zkhost_prove_dev_cloak(uint32_t n_in, uint32_t n_out, const uint64_t* quantities, const uint8_t* flavors, const uint8_t seed[32],
                           const uint8_t* generators, size_t gens_capacity, uint8_t* commitments, uint8_t* proof, size_t proof_cap,
                           size_t* proof_len_out) {
  R1csDesc d;
  std::vector<uint32_t> md, values, blindings, given;
  PvCloakTrace::trace(n_in, n_out, d, md);
  for (size_t i = 0; i < (size_t)n_in + n_out; ++i) {
    uint8_t b[32];
    Scalar::from_u64(quantities[i]).to_bytes(b); words_of(b, 8, values);
    words_of(flavors + 32 * i, 8, values);
    R1csProver::derive_scalar(seed, "q_blinding", i).to_bytes(b); words_of(b, 8, blindings);
    R1csProver::derive_scalar(seed, "f_blinding", i).to_bytes(b); words_of(b, 8, blindings);
  }
  pv_cloak_given(n_in, n_out, quantities, flavors, given);
  return pv_emulate(d, md, values, blindings, given, seed, generators, gens_capacity, commitments, proof, proof_cap, proof_len_out);
}

// The witness queue of one cloak statement as the device prover receives it (pv_cloak_given): per first-phase allocation
// its (left, right) assignment, 2 x 32 canonical bytes, in the gadget's allocation order.  -> the number of pairs; `out`
// is written when `cap` pairs hold them all.
size_t zkhost_cloak_given(uint32_t n_in, uint32_t n_out, const uint64_t* quantities, const uint8_t* flavors, uint8_t* out, size_t cap) {
  std::vector<uint32_t> given;
  pv_cloak_given(n_in, n_out, quantities, flavors, given);
  const size_t pairs = given.size() / 16;
  if (out && pairs <= cap)
    for (size_t i = 0; i < given.size(); ++i)
      for (int b = 0; b < 4; ++b) out[4 * i + b] = (uint8_t)(given[i] >> (8 * b));
  return pairs;
}

int zkhost_prove_dev_r1cs(const char* label, uint32_t m, uint32_t n1, uint32_t n, uint32_t n_chal, const char* const* chal_labels,
                          uint32_t n_cons, const uint64_t* term_offsets, const uint8_t* kinds, const uint32_t* idx,
                          const uint8_t* coeff, const int32_t* chal, const uint32_t* power, const uint32_t* mult_def,
                          const uint8_t* values, const uint8_t* given, size_t n_given, const uint8_t seed[32],
                          const uint8_t* generators, size_t gens_capacity, uint8_t* commitments, uint8_t* proof, size_t proof_cap,
                          size_t* proof_len_out) {
  R1csDesc d;
  if (!pv_desc_of(d, label, m, n1, n, n_chal, chal_labels, n_cons, term_offsets, kinds, idx, coeff, chal, power)) return -1;
  std::vector<uint32_t> md(mult_def, mult_def + 2 * (size_t)n), vw, bw, gw;
  words_of(values, 8 * (size_t)m, vw);
  for (uint32_t i = 0; i < m; ++i) {
    uint8_t b[32];
    R1csProver::derive_scalar(seed, "blinding", i).to_bytes(b);
    words_of(b, 8, bw);
  }
  words_of(given, 16 * n_given, gw);
  return pv_emulate(d, md, vw, bw, gw, seed, generators, gens_capacity, commitments, proof, proof_cap, proof_len_out);
}

// The plan of one device prover call (prover_call_plan.hpp) -- of the cloak when n_in + n_out > 0, else of the system described
// by the arrays (mult_def NULL: every multiplier given).  flags: 1 the call drew its seed, 2 the cloak's tag table, 4 the caller
// brought blindings.  numbers[PV_CALL_PLAN_NUMBERS]: steps, blob words, scaffolding bytes, draw_blindings, terms of an
// inner-product row | the input area: values blindings given seeds bytes | the blob's tables in PV_PLAN_TABLES order, then
// chal_labels, draw | per multiplication 0..4: rows terms P kinds o_off o_idx | the workspace in PV_WORKSPACE order | the
// shape the plan was made for (pv_build): m n1 n pn k n_given r1_terms r2_terms state_words proof_stride gens_capacity.
// steps (3 words each: kind phase mask), blob, lay: written when not NULL, as many as numbers[0..2] say.
// -> 0; -1 a description out of range; -3 one the device prover cannot serve; -4 scaffolding out of step;
// -5 the numbers written are not PV_CALL_PLAN_NUMBERS (the lists above changed without it)
enum { PV_CALL_PLAN_NUMBERS = 5 + 5 + 16 + 5 * 6 + 21 + 11 };
int zkhost_prover_call_plan(const char* label, uint32_t m, uint32_t n1, uint32_t n, uint32_t n_chal, const char* const* chal_labels,
                            uint32_t n_cons, const uint64_t* term_offsets, const uint8_t* kinds, const uint32_t* idx,
                            const uint8_t* coeff, const int32_t* chal, const uint32_t* power, const uint32_t* mult_def,
                            uint32_t n_in, uint32_t n_out, size_t gens_capacity, size_t batch, int W, uint32_t flags,
                            uint64_t* numbers, uint32_t* steps, uint32_t* blob, uint8_t* lay) {
  R1csDesc d;
  std::vector<uint32_t> md;
  PvHostPlan hp;
  try {
    if (n_in + n_out) {
      PvCloakTrace::trace(n_in, n_out, d, md);
    } else {
      if (!pv_desc_of(d, label, m, n1, n, n_chal, chal_labels, n_cons, term_offsets, kinds, idx, coeff, chal, power)) return -1;
      md.assign(2 * (size_t)n, PV_GIVEN);
      if (mult_def) md.assign(mult_def, mult_def + 2 * (size_t)n);
    }
    hp = pv_build(d, md, gens_capacity);
  } catch (const std::exception&) { return -3; }
  const PvCallPlan p = plan_prover_call(hp, batch, W, {(flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0});
  uint64_t* o = numbers;
  *o++ = p.steps.size(); *o++ = p.blob.size(); *o++ = p.lay_bytes; *o++ = p.draw_blindings; *o++ = p.ipa_row_len;
  *o++ = p.in.values; *o++ = p.in.blindings; *o++ = p.in.given; *o++ = p.in.seeds; *o++ = p.in.bytes;
#define X(f) *o++ = p.at.f;
  PV_PLAN_TABLES(X) X(chal_labels) X(draw)
#undef X
  for (const PvMsm& mm : p.msm) { *o++ = mm.rows; *o++ = mm.terms; *o++ = (uint64_t)mm.P; *o++ = mm.kinds; *o++ = mm.o_off; *o++ = mm.o_idx; }
#define X(b) *o++ = p.ws.b;
  PV_WORKSPACE(X)
#undef X
  const PvShape& sh = p.sh;
  for (uint32_t v : {sh.m, sh.n1, sh.n, sh.pn, sh.k, sh.n_given, sh.r1_terms, sh.r2_terms, sh.state_words, sh.proof_stride, sh.gens_capacity}) *o++ = v;
  if (o - numbers != PV_CALL_PLAN_NUMBERS) return -5;
  if (steps) for (const PvStep& s : p.steps) { *steps++ = (uint32_t)s.kind; *steps++ = s.phase; *steps++ = s.mask; }
  if (blob) std::memcpy(blob, p.blob.data(), p.blob.size() * 4);
  if (lay && !p.fill_scaffolding(lay)) return -4;
  return 0;
}
}  // extern "C"

// ---- ZkVM transactions (zkvm_tx.hpp): the host half of Tx::verify, with this library's reference group arithmetic for
// the aggregated key.  Out: status (0 ok, 1 invalid, 2 outside the subset), txid, the cloak's shape and commitments,
// the terms of the signature equation (scalars | points, 32 bytes each; *n_sig of them).
extern "C" int zkhost_tx_prepare(const uint8_t* tx, size_t len, uint8_t txid[32], uint32_t* n_in, uint32_t* n_out, uint8_t* commitments,
                                 size_t com_cap, uint8_t* sig_scalars, uint8_t* sig_points, size_t sig_cap, size_t* n_sig,
                                 size_t* proof_offset, size_t* proof_len) {
  using namespace zk::zkvm;
  TxStatement st = tx_prepare(tx, len);
  *n_sig = 0;
  if (st.status != TX_OK) return (int)st.status;
  const size_t n_terms = st.sig_scalars.size() / 32, n_keys = n_terms - 2;
  if (st.commitments.size() > com_cap || n_terms > sig_cap) return -1;
  // aggregated key X = sum a_i X_i with the reference multiscalar multiplication
  std::vector<ge> pts(n_keys);
  MsmRow row;
  for (size_t i = 0; i < n_keys; ++i) {
    uint32_t w[8];
    std::memcpy(w, &st.sig_points[32 * (2 + i)], 32);
    if (!ristretto_decode(pts[i], w)) return (int)TX_INVALID;
    Scalar a;
    Scalar::from_canonical(&st.sig_scalars[32 * (2 + i)], a);
    row.add(a, (uint32_t)i);
  }
  std::vector<uint8_t> agg;
  host_rows(pts, {row}, agg);
  ge B;
  B.X = fe_BASE_X(); B.Y = fe_BASE_Y(); B.Z = fe_one(); B.T = fe_BASE_T();
  uint32_t benc[8];
  ristretto_encode(benc, B);
  tx_finish_signature(st, (const uint8_t*)benc, agg.data());
  std::memcpy(txid, st.txid, 32);
  *n_in = st.n_in; *n_out = st.n_out;
  std::memcpy(commitments, st.commitments.data(), st.commitments.size());
  std::memcpy(sig_scalars, st.sig_scalars.data(), st.sig_scalars.size());
  std::memcpy(sig_points, st.sig_points.data(), st.sig_points.size());
  *n_sig = n_terms;
  *proof_offset = (size_t)(st.proof - tx);
  *proof_len = st.proof_len;
  return 0;
}

// PvRngCoop (the TranscriptRng's draws on a state spread over an emulated wavefront) against PvRng (one lane, state in
// registers) and thereby against the byte-wise STROBE: n draws from a keyed generator; returns mismatches.
extern "C" uint64_t zkhost_rng_coop_selftest(uint64_t seed, uint32_t n_draws) {
  using namespace zk::coop;
  uint32_t w[52];
  {
    Transcript t("rng selftest");
    uint8_t sd[32];
    for (int i = 0; i < 32; ++i) sd[i] = (uint8_t)(seed >> (8 * (i & 7))) ^ (uint8_t)i;
    t.rekey_with_witness("v_blinding", sd, 32);
    t.finalize_rng(sd);
    t.export_state(w);
  }
  PvRng a;
  a.load(w);
  if (!a.fast()) return ~0ull;
  LaneVec lo, hi;
  PvRngCoop<HostTraits>::Masks m;
  for (uint32_t i = 0; i < 64; ++i) {
    const KcLane k = kc_lane(i);
    lo.l[i] = k.live ? w[2 * k.q] : 0;
    hi.l[i] = k.live ? w[2 * k.q + 1] : 0;
    auto holds = [&k](uint32_t q) { return (k.live && k.q == q) ? ~0u : 0u; };
    m.w4.l[i] = holds(4); m.w5.l[i] = holds(5); m.w8.l[i] = holds(8); m.w9.l[i] = holds(9); m.w20.l[i] = holds(20);
    m.keep.l[i] = (k.live && k.q < 8) ? 0u : ~0u;
  }
  const auto c = host_consts();
  uint64_t bad = 0;
  for (uint32_t d = 0; d < n_draws; ++d) {
    const scm want = a.draw();
    PvRngCoop<HostTraits>::draw(lo, hi, c, m, d == 0 && w[50] == 32);
    uint32_t wd[16];
    for (uint32_t i = 0; i < 64; ++i) {
      const KcLane k = kc_lane(i);
      if (k.primary && k.q < 8) { wd[2 * k.q] = lo.l[i]; wd[2 * k.q + 1] = hi.l[i]; }
    }
    PvRngCoop<HostTraits>::taken(lo, hi, m);
    const scm got = scm_from_wide(wd);
    for (int q = 0; q < 8; ++q) if (got.v[q] != want.v[q]) { ++bad; break; }
  }
  uint32_t wa[52];
  a.store(wa);
  for (uint32_t i = 0; i < 64; ++i) {
    const KcLane k = kc_lane(i);
    if (k.primary && (lo.l[i] != wa[2 * k.q] || hi.l[i] != wa[2 * k.q + 1])) ++bad;
  }
  return bad;
}

// HostPool (host_pool.hpp, the workers behind every host stage of the product): every index of every call visited exactly
// once for a range of sizes and thread counts, calls from `callers` threads at once (one at a time gets the pool, the
// others wait their turn), and repeated use of the sleeping workers.  Returns the number of violations.
#include "host_pool.hpp"
// what host_threads = 0 means: the CPUs this process may keep busy (affinity mask, control-group quota)
extern "C" int zkhost_usable_cpus() { return zk::usable_cpus(); }

extern "C" uint64_t zkhost_pool_selftest(uint32_t rounds, uint32_t callers) {
  std::atomic<uint64_t> bad{0}, took{0}, refused{0};
  auto one = [&](uint32_t salt) {
    static const size_t sizes[] = {0, 1, 2, 15, 16, 17, 255, 1000, 4097};
    static const int threads[] = {2, 3, 8, 32, 100};
    for (uint32_t r = 0; r < rounds; ++r)
      for (size_t n : sizes)
        for (int nt : threads) {
          std::vector<std::atomic<uint32_t>> hits(n);
          for (auto& h : hits) h.store(0);
          const std::function<void(size_t)> f = [&](size_t i) { (void)salt; hits[i].fetch_add(1); };
          if (zk::HostPool::get().run(n, std::min(nt, zk::HostPool::MAX_WORKERS + 1), f)) {
            ++took;
            for (auto& h : hits) if (h.load() != 1) ++bad;
          } else {
            ++refused;
            for (auto& h : hits) if (h.load() != 0) ++bad;   // a refused call must not have touched anything
          }
        }
  };
  std::vector<std::thread> th;
  for (uint32_t c = 1; c < callers; ++c) th.emplace_back(one, c);
  one(0);
  for (auto& t : th) t.join();
  if (took.load() == 0) ++bad;
  if (refused.load() != 0) ++bad;                     // only a forked process is refused
  return bad.load();
}

// ---- the framing of the sharded verification's one exchange (comm_frame.hpp), for the CPU tests: a world of any size is
// ---- the test concatenating the slots its "ranks" packed
#include "ticket_cut.hpp"
// the device batches a burst of tickets leaves in (tickets per batch) under the equal-parts policy; returns their number
extern "C" size_t zkhost_ticket_cut(const uint64_t* sizes, size_t n, uint64_t target, uint64_t* out_counts, size_t cap) {
  std::vector<size_t> v(sizes, sizes + n);
  const std::vector<size_t> cut = zk::ticket_cut(v, (size_t)target);
  for (size_t i = 0; i < cut.size() && i < cap; ++i) out_counts[i] = cut[i];
  return cut.size();
}

// the plan of one zkgpu_r1cs_verify_mixed call (mixed_plan.hpp).  infos: n_infos rows of MIXHOOK_INFO values in the order of
// MixPlanInfo's fields; plan_record_bytes stands for sizeof(PrepPlan) (the plans section stays zero).  -> the table's bytes
// (copied to `table` when they fit `cap`), or -1 with the argument error's text in `err`.  summary[MIXHOOK_SUMMARY]:
// distinct plans | class_start[4] | class_lds[2] | lp_targets lp_pn lp_slots | coop | max_nch | n_com n_pw n_ch n_raw n_abs
// n_dyn n_st | n_checks n_grouped n_rows max_ns, checks of two or more | lane-order entries | t_plans .. t_end (10);
// uniq[n_infos]: the distinct plans as indices into infos
#include "mixed_plan.hpp"
constexpr int MIXHOOK_INFO = 14, MIXHOOK_SUMMARY = 35;
extern "C" long long zkhost_mixed_plan(const uint64_t* infos, size_t n_infos, const uint32_t* plan_index, const uint64_t* proof_offsets,
                                       size_t batch, int coop_wanted, uint32_t group_size, int may_group, size_t plan_record_bytes,
                                       uint8_t* table, size_t cap, uint64_t* summary, uint32_t* uniq, char* err, size_t err_cap) {
  std::vector<MixPlanInfo> in(n_infos);
  for (size_t p = 0; p < n_infos; ++p) {
    const uint64_t* f = infos + MIXHOOK_INFO * p;
    in[p] = MixPlanInfo{f[0], (uint32_t)f[1], (uint32_t)f[2], (uint32_t)f[3], (uint32_t)f[4], (uint32_t)f[5], (uint32_t)f[6], (uint32_t)f[7],
                        (uint32_t)f[8], (uint32_t)f[9], (uint32_t)f[10], (size_t)f[11], f[12] != 0, (uint32_t)f[13]};
  }
  const MixCallPlan mp = plan_mixed_call(in.data(), n_infos, plan_index, proof_offsets, batch,
                                         MixPlanOptions{coop_wanted != 0, group_size, may_group != 0}, plan_record_bytes);
  if (mp.error) {
    if (err_cap) { std::strncpy(err, mp.error, err_cap - 1); err[err_cap - 1] = 0; }
    return -1;
  }
  const uint64_t sum[MIXHOOK_SUMMARY] = {
      mp.uniq.size(), mp.class_start[0], mp.class_start[1], mp.class_start[2], mp.class_start[3], mp.class_lds[0], mp.class_lds[1],
      mp.lp_targets, mp.lp_pn, mp.lp_slots, mp.coop, mp.max_nch, mp.n_com, mp.n_pw, mp.n_ch, mp.n_raw, mp.n_abs, mp.n_dyn, mp.n_st,
      mp.n_checks, mp.n_grouped, mp.n_rows, mp.max_ns, mp.n_pairs, mp.n_lanes,
      mp.t_plans, mp.t_stmts, mp.t_order, mp.t_lanes, mp.t_doff, mp.t_soff, mp.t_grp, mp.t_mem, mp.t_goff, mp.t_end};
  std::memcpy(summary, sum, sizeof sum);
  std::copy(mp.uniq.begin(), mp.uniq.end(), uniq);
  if (mp.t_end <= cap) std::memcpy(table, mp.tab.data(), mp.t_end);
  return (long long)mp.t_end;
}

// the plan of one device batch of the verification pipeline (pipe_plan.hpp).  in[11]: n_msm n_dyn n_static W whole_proof ns |
// group_size locate_mode locate_parts forced_parts want_reasons.  out[36]: PipePlan's fields in their order
#include "pipe_plan.hpp"
extern "C" void zkhost_pipe_plan(const int64_t* in, uint64_t* out) {
  const PipePlan p = plan_pipe(PipeShape{(uint64_t)in[0], (uint64_t)in[1], (uint64_t)in[2], (int)in[3], in[4] != 0, (uint32_t)in[5]},
                               PipeKnobs{(int)in[6], (int)in[7], (int)in[8], (int)in[9], in[10] != 0});
  const uint64_t flat[36] = {
      p.nbytes, (uint64_t)p.P, p.n_lanes, p.group, p.n_groups, p.locate, p.spec, p.grp_rows, (uint64_t)p.Pg, (uint64_t)p.Pf, (uint64_t)p.Pl,
      p.grp_sc, p.grp_digits, p.grp_partials, p.grp_ok, p.row_map, p.grp_fail, p.grp_fail_sum, p.grp_ws, p.grp_wf, p.grp_dyn, p.rechk_pts,
      p.accept, p.accept2, p.bitmap, p.pinned, p.status, p.digits, p.st_partials, p.dynsum,
      p.small.dyn_rows, p.small.window_sums, p.small.window_flags, p.small.msm_fail, p.small.small_tbl, p.small.recoded};
  std::memcpy(out, flat, sizeof flat);
}

// which form of the multiscalar multiplication a call takes, and its workspace (msm_route.hpp).  in[6]: n_msm n_dyn n_static
// max_dyn_row (< 0: not known) forced_w entry (0 straight to the bucket pipeline, 1 batch, 2 batch over a set with tables).
// out[40]: MsmRoute's fields in their order
#include "msm_route.hpp"
extern "C" void zkhost_msm_route(const int64_t* in, uint64_t* out) {
  const MsmRoute r = plan_msm(MsmShape{(uint64_t)in[0], (uint64_t)in[1], (uint64_t)in[2], (uint64_t)in[3], (int)in[4], (int)in[5]});
  const uint64_t flat[40] = {
      r.small, (uint64_t)r.parts, (uint64_t)r.w, (uint64_t)r.n_windows, r.n_buckets, r.chunk_size, r.chunks, r.n_terms, r.n_wins, r.n_bins, r.n_tasks,
      r.max_entries, r.too_large, r.part_sort, r.quad_reduce, r.window_partials, r.split_decode, r.scan_blocks, r.fat_cap, r.fat_blocks,
      r.hi_bits, r.n_part, r.n_tiles,
      r.dyn_rows, r.bins, r.block_sums, r.entries, r.buckets, r.partials, r.partial_flags, r.window_sums, r.window_flags, r.msm_fail, r.heavy,
      r.class_count, r.bin_order, r.dec_scratch, r.part_hist, r.part_block_sums, r.part_entries};
  std::memcpy(out, flat, sizeof flat);
}

// verifier randomness the library draws itself (draw_r.hpp): r(seed, first) .. r(seed, first + count - 1), 64 bytes each -- the
// host side of the function k_draw_r runs on the device
#include "draw_r.hpp"
extern "C" void zkhost_draw_r(const uint8_t seed[32], uint64_t first, size_t count, uint8_t* out) { draw_r_bytes(seed, first, count, out); }

// prover randomness the library draws itself (prover_draw.hpp): statements first .. first + count - 1 of a call -- the host
// side of the function k_pv_draw runs on the device.  table: m + 1 records of 24 bytes, the tag (NUL-padded to 16) and its
// index as LE64; the first m are blindings (64 bytes reduced mod l), the last is the 32-byte rng seed.  out: count x 32 (m + 1).
// -> 0, or -1 for a tag that is empty or longer than ten bytes
#include "prover_draw.hpp"
extern "C" int zkhost_prover_draw(const uint8_t call_seed[32], uint64_t first, size_t count, const uint8_t* table, size_t m, uint8_t* out) {
  std::vector<uint32_t> t((m + 1) * PV_DRAW_ENTRY_WORDS);
  for (size_t d = 0; d <= m; ++d) {
    const uint8_t* rec = table + 24 * d;
    uint64_t index = 0;
    for (int k = 0; k < 8; ++k) index |= (uint64_t)rec[16 + k] << (8 * k);
    if (!pv_draw_entry((const char*)rec, strnlen((const char*)rec, 16), index, &t[PV_DRAW_ENTRY_WORDS * d])) return -1;
  }
  pv_draw_bytes(call_seed, first, count, t.data(), m, out);
  return 0;
}

#include "comm_frame.hpp"
extern "C" size_t zkhost_comm_slot_bytes(const uint64_t* cuts, int world) { return commframe::slot_bytes(cuts, world); }
extern "C" void zkhost_comm_pack(uint8_t* out, size_t slot, const uint64_t* cuts, int rank, const uint8_t* local_bitmap, int local_status) {
  commframe::pack(out, slot, cuts, rank, local_bitmap, local_status);
}
extern "C" int zkhost_comm_unpack(const uint8_t* all, size_t slot, const uint64_t* cuts, int world, int rank, uint8_t* whole) {
  return commframe::unpack(all, slot, cuts, world, rank, whole);
}

// ---- the keys-first pass of zkgpu_tx_verify_batch (tx_prepare_many with only = P_MUSIG: the plan drops every other hash job)
// ---- against the full pass, for the CPU tests: per transaction status and a SHA3-512 digest over what BOTH must leave in
// ---- the statement before the signature challenge -- arity, proof length, commitments, s, -1, the MuSig coefficients
// ---- a_i, R and the keys X_i.
extern "C" void zkhost_tx_rows_group(const uint8_t* txs, const uint64_t* offs, size_t count, int lockstep, int keys_only,
                                     uint8_t* status, uint8_t* digest /*64 per tx*/) {
  using namespace zk::zkvm;
  for (size_t g = 0; g < count; g += 8) {
    const size_t n = std::min<size_t>(8, count - g);
    const uint8_t* p[8]; size_t l[8];
    TxStatement st[8];
    for (size_t i = 0; i < n; ++i) { p[i] = txs + offs[g + i]; l[i] = (size_t)(offs[g + i + 1] - offs[g + i]); }
    tx_prepare_many(p, l, st, n, lockstep != 0, keys_only ? (uint8_t)P_MUSIG : ALL_PROTOS);
    for (size_t i = 0; i < n; ++i) {
      status[g + i] = (uint8_t)st[i].status;
      Sponge sp = sha3_512_sponge();
      if (st[i].status == TX_OK) {
        const uint64_t head[3] = {st[i].n_in, st[i].n_out, (uint64_t)st[i].proof_len};
        sp.absorb((const uint8_t*)head, sizeof head);
        sp.absorb(st[i].commitments.data(), st[i].commitments.size());
        sp.absorb(st[i].sig_scalars.data(), st[i].sig_scalars.size());
        sp.absorb(st[i].sig_points.data() + 32, st[i].sig_points.size() - 32);     // ([0] is the basepoint's place, filled later)
      }
      sp.squeeze(digest + 64 * (g + i), 64);
    }
  }
}

// ---- the lockstep (AVX-512, eight transactions at a time) form of the payment VM's hashing against the one-at-a-time
// ---- form: for the CPU tests.  Per transaction out: status | txid (32) | then, for accepted ones, the statement's
// ---- commitments, signature scalars and points (after the challenge has been applied with the given aggregated keys)
// ---- folded into a SHA3-512 digest (64).  Returns 1 when AVX-512 is available (0: both modes ran one at a time).
extern "C" int zkhost_tx_prepare_group(const uint8_t* txs, const uint64_t* offs, size_t count, int lockstep, const uint8_t* agg_keys /*32 per tx*/,
                                       uint8_t* status, uint8_t* txid /*32 per tx*/, uint8_t* digest /*64 per tx*/) {
  using namespace zk::zkvm;
  uint8_t base[32];
  for (int i = 0; i < 32; ++i) base[i] = (uint8_t)(0xB0 + i);
  for (size_t g = 0; g < count; g += 8) {
    const size_t n = std::min<size_t>(8, count - g);
    const uint8_t* p[8]; size_t l[8];
    TxStatement st[8];
    for (size_t i = 0; i < n; ++i) { p[i] = txs + offs[g + i]; l[i] = (size_t)(offs[g + i + 1] - offs[g + i]); }
    tx_prepare_many(p, l, st, n, lockstep != 0);
    TxStatement* live[8]; const uint8_t* keys[8]; size_t nl = 0;
    for (size_t i = 0; i < n; ++i) if (st[i].status == TX_OK) { live[nl] = &st[i]; keys[nl] = agg_keys + 32 * (g + i); ++nl; }
    if (lockstep) tx_finish_signature_many(live, keys, base, nl);
    else for (size_t i = 0; i < nl; ++i) tx_finish_signature(*live[i], base, keys[i]);
    for (size_t i = 0; i < n; ++i) {
      status[g + i] = (uint8_t)st[i].status;
      std::memcpy(txid + 32 * (g + i), st[i].txid, 32);
      Sponge sp = sha3_512_sponge();
      if (st[i].status == TX_OK) {
        sp.absorb(st[i].commitments.data(), st[i].commitments.size());
        sp.absorb(st[i].sig_scalars.data(), st[i].sig_scalars.size());
        sp.absorb(st[i].sig_points.data(), st[i].sig_points.size());
      }
      sp.squeeze(digest + 64 * (g + i), 64);
    }
  }
  return x8_available() ? 1 : 0;
}

// ---- building transactions (zkvm_tx_build.hpp): what bench.py and the tests feed zkgpu_tx_verify_batch with -----------
#include "zkvm_tx_build.hpp"
#include <thread>

// one signed payment around an existing cloak proof -> its length (0: it does not fit `cap`, or the arities are outside 1..16)
extern "C" size_t zkhost_tx_wrap_payment(size_t n_in, size_t n_out, const uint8_t* com, const uint8_t* proof, size_t proof_len,
                                         const uint8_t seed[32], uint64_t mintime, uint64_t maxtime, uint8_t* out, size_t cap) {
  const std::vector<uint8_t> tx = zk::zkvm::tx_wrap_payment(n_in, n_out, com, proof, proof_len, seed, mintime, maxtime);
  if (tx.empty() || tx.size() > cap) return 0;
  std::memcpy(out, tx.data(), tx.size());
  return tx.size();
}

// `count` of them on `threads` threads: statement i = coms[i] (64 (n_in + n_out) bytes), proofs[i] (proof_len bytes), seeds[i]
// (32 bytes), mintime = mintime0 + i; the transactions back to back in `out`, offsets[count + 1].  -> 0, or -1 (one did not
// build or `cap` is too small)
extern "C" int zkhost_tx_wrap_many(size_t count, size_t n_in, size_t n_out, const uint8_t* coms, const uint8_t* proofs, size_t proof_len,
                                   const uint8_t* seeds, uint64_t mintime0, uint64_t maxtime, int threads, uint8_t* out, size_t cap,
                                   uint64_t* offsets) {
  std::vector<std::vector<uint8_t>> made(count);
  (void)zk::zkvm::base_table();                       // (built before the threads start)
  const int nt = std::max(1, std::min<int>(threads > 0 ? threads : zk::usable_cpus(), 64));
  std::vector<std::thread> th;
  const size_t wcom = 64 * (n_in + n_out);
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      for (size_t i = (size_t)t; i < count; i += (size_t)nt)
        made[i] = zk::zkvm::tx_wrap_payment(n_in, n_out, coms + i * wcom, proofs + i * proof_len, proof_len, seeds + 32 * i, mintime0 + i, maxtime);
    });
  for (auto& t : th) t.join();
  offsets[0] = 0;
  for (size_t i = 0; i < count; ++i) {
    if (made[i].empty()) return -1;
    offsets[i + 1] = offsets[i] + made[i].size();
  }
  if (offsets[count] > cap) return -1;
  for (size_t i = 0; i < count; ++i) std::memcpy(out + offsets[i], made[i].data(), made[i].size());
  return 0;
}

// ---- the scheduling of a transaction call on the CPU (tx_call.hpp) ----------------------------------------------------
// zkgpu_tx_verify_batch = TxCall + a device.  Here the device is a stand-in: every stage "runs" on a thread of its own that
// first sleeps a pseudo-random while (so that completions arrive in every order the real device could produce) and then
// computes the stage with this library's reference group arithmetic -- aggregated keys and signature equations for real,
// cloak proofs by a table the caller supplies (proof_ok[i]: this test is about the scheduling, and the reference R1CS
// verifier takes 30 ms per proof).  The sanitizer tier runs it under ThreadSanitizer and AddressSanitizer: flags, ring,
// stage cuts, hand-overs, the error paths (fail_at: the n-th device operation fails) -- no GPU involved.
#include "tx_call.hpp"
#include <atomic>
#include <random>

namespace {
using namespace zk::zkvm;

void ge_scalarmult_host(ge& out, const Scalar& s, const ge& p) {
  uint8_t b[32];
  s.to_bytes(b);
  ge_identity(out);
  for (int i = 255; i >= 0; --i) {
    ge_double(out, out);
    if ((b[i >> 3] >> (i & 7)) & 1) ge_add(out, out, p);
  }
}
bool decode_host(ge& p, const uint8_t enc[32]) {
  uint32_t w[8];
  std::memcpy(w, enc, 32);
  return ristretto_decode(p, w);
}
// acc += sum of sc[t] pt[t] over the terms [lo, hi); false: a point that does not decode or a scalar that is not canonical
bool add_terms(ge& acc, const uint8_t* sc, const uint8_t* pt, uint64_t lo, uint64_t hi) {
  for (uint64_t t = lo; t < hi; ++t) {
    ge X, aX;
    Scalar a;
    if (!decode_host(X, pt + 32 * t) || !Scalar::from_canonical(sc + 32 * t, a)) return false;
    ge_scalarmult_host(aX, a, X);
    ge_add(acc, acc, aX);
  }
  return true;
}

class HostTxDevice : public TxDevice {
 public:
  // format: the mode of the call the stand-in serves, handed to TxCall as it is (format()); a stand-in answers no question about
  // the mode itself.  Its CLASS must be the one the format calls for: this one neither hashes nor chains (stand_in_format)
  HostTxDevice(const uint8_t* txs, const uint64_t* offs, size_t batch, const uint8_t* proof_ok, uint32_t seed, int fail_at, const TxFormat& format)
      : txs_(txs), offs_(offs), batch_(batch), proof_ok_(proof_ok), rng_(seed), fail_at_(fail_at), format_(format) {
    ge B;
    B.X = fe_BASE_X(); B.Y = fe_BASE_Y(); B.Z = fe_one(); B.T = fe_BASE_T();
    encode_point(base_, B);
  }
  ~HostTxDevice() override {
    for (auto& s : keys_) if (s.th.joinable()) s.th.join();
    for (auto& s : sigs_) if (s.th.joinable()) s.th.join();
  }
  const uint8_t* basepoint() override { return base_; }
  int keys_enqueue(int slot, const uint8_t* sc, const uint8_t* pt, const uint64_t* off, size_t rows) override {
    if (failing()) return -3;
    Stage& s = keys_[slot];
    if (s.th.joinable()) { err_ = "key slot reused before it was collected"; return -1; }
    s.done = false;
    s.ok.assign((rows + 7) / 8 + 1, 0);
    s.values.assign(32 * rows, 0);
    const unsigned us = delay();
    s.th = std::thread([=, &s] {
      std::this_thread::sleep_for(std::chrono::microseconds(us));
      for (size_t r = 0; r < rows; ++r) {
        ge acc;
        ge_identity(acc);
        if (add_terms(acc, sc, pt, off[r], off[r + 1])) { s.ok[r / 8] |= (uint8_t)(1u << (r % 8)); encode_point(&s.values[32 * r], acc); }
      }
      s.done = true;
    });
    return 0;
  }
  bool keys_done(int slot) override { return keys_[slot].done; }
  int keys_collect(int slot, uint8_t* ok_bits, uint8_t* values, uint8_t*) override {     // (a device without reasons: `why` is ignored)
    Stage& s = keys_[slot];
    if (!s.th.joinable()) { err_ = "nothing to collect in this key slot"; return -1; }
    s.th.join();
    if (failing()) return -3;
    std::memcpy(ok_bits, s.ok.data(), s.ok.size() - 1);
    std::memcpy(values, s.values.data(), s.values.size());
    return 0;
  }
  int proofs_stage(size_t ring_slot, size_t n, const TxProofSource* src, int, void** handle, std::string* err) override {
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (ring_busy_[ring_slot]) { *err = "ring slot staged while its last chunk is still in flight"; return -1; }
      ring_busy_[ring_slot] = true;
      ++staged_total_;
    }
    Proofs* p = new Proofs();
    p->ring_slot = ring_slot;
    p->src.assign(src, src + n);
    *handle = p;
    return 0;
  }
  int proofs_start(size_t ring_slot, void* handle) override {
    Proofs* p = (Proofs*)handle;
    if (p->ring_slot != ring_slot) { err_ = "chunk started on another ring slot than it was staged in"; return -1; }
    if (failing()) return -3;
    p->bits.assign((p->src.size() + 7) / 8 + 1, 0);
    const unsigned us = delay();
    p->th = std::thread([this, p, us] {
      std::this_thread::sleep_for(std::chrono::microseconds(us));
      for (size_t q = 0; q < p->src.size(); ++q) {
        // which transaction of the call does this proof belong to?  (the proof lies inside its bytes)
        const uint64_t at = (uint64_t)(p->src[q].proof - txs_);
        size_t lo = 0, hi = batch_;
        while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if (offs_[mid] <= at) lo = mid; else hi = mid; }
        if (proof_ok_[lo]) p->bits[q / 8] |= (uint8_t)(1u << (q % 8));
      }
      p->done = true;
    });
    return 0;
  }
  bool proofs_done(void* handle) override { return ((Proofs*)handle)->done; }
  int proofs_finish(void* handle, uint8_t* accept_bits, uint8_t*) override {
    Proofs* p = (Proofs*)handle;
    if (p->th.joinable()) p->th.join();
    const bool fail = failing();
    if (!fail) std::memcpy(accept_bits, p->bits.data(), p->bits.size() - 1);
    proofs_release(handle);
    return fail ? -3 : 0;
  }
  void proofs_release(void* handle) override {
    Proofs* p = (Proofs*)handle;
    if (p->th.joinable()) p->th.join();
    { std::lock_guard<std::mutex> lk(mu_); ring_busy_[p->ring_slot] = false; ++released_total_; }
    delete p;
  }
  int sigs_enqueue(int slot, size_t rows, const uint8_t* dsc, const uint8_t* dpt, const uint64_t* doff, const uint8_t* bsc, const SigChain* chain) override {
    if (chain) { err_ = "a chained signature stage on a device that does not chain"; return -1; }
    if (failing()) return -3;
    Stage& s = sigs_[slot];
    if (s.th.joinable()) { err_ = "signature slot reused before it was collected"; return -1; }
    s.done = false;
    s.ok.assign((rows + 7) / 8 + 1, 0);
    const unsigned us = delay();
    s.th = std::thread([=, &s] {
      std::this_thread::sleep_for(std::chrono::microseconds(us));
      sig_rows_check(s, rows, dsc, dpt, doff, bsc);
      s.done = true;
    });
    return 0;
  }
  bool sigs_done(int slot) override { return sigs_[slot].done; }
  int sigs_collect(int slot, uint8_t* bits, uint8_t*) override {
    Stage& s = sigs_[slot];
    if (!s.th.joinable()) { err_ = "nothing to collect in this signature slot"; return -1; }
    s.th.join();
    if (failing()) return -3;
    std::memcpy(bits, s.ok.data(), s.ok.size() - 1);
    return 0;
  }
  std::string last_error() override { return err_.empty() ? "injected device fault" : err_; }
  const TxFormat& format() const override { return format_; }
  size_t leaked() { std::lock_guard<std::mutex> lk(mu_); return staged_total_ - released_total_; }

 protected:
  struct Stage;
  void sig_rows_check(Stage& s, size_t rows, const uint8_t* dsc, const uint8_t* dpt, const uint64_t* doff, const uint8_t* bsc) {
    for (size_t r = 0; r < rows; ++r) {
      Scalar sb;
      if (!Scalar::from_canonical(bsc + 32 * r, sb)) continue;
      ge acc;
      base_mul(acc, sb);
      if (add_terms(acc, dsc, dpt, doff[r], doff[r + 1]) && ge_is_identity(acc)) s.ok[r / 8] |= (uint8_t)(1u << (r % 8));
    }
  }
  struct Stage { std::thread th; std::atomic<bool> done{false}; std::vector<uint8_t> ok, values; };
  struct Proofs { size_t ring_slot = 0; std::vector<TxProofSource> src; std::vector<uint8_t> bits; std::thread th; std::atomic<bool> done{false}; };
  unsigned delay() { std::lock_guard<std::mutex> lk(mu_); return (unsigned)(rng_() % 400); }
  bool failing() { return fail_at_ >= 0 && ops_.fetch_add(1) == fail_at_; }
  const uint8_t* txs_;
  const uint64_t* offs_;
  size_t batch_;
  const uint8_t* proof_ok_;
  std::mutex mu_;
  std::mt19937 rng_;
  const int fail_at_;
  std::atomic<int> ops_{0};
  Stage keys_[2], sigs_[2];
  bool ring_busy_[TxCall::RING] = {false};
  size_t staged_total_ = 0, released_total_ = 0;
  uint8_t base_[32];
  std::string err_;
  const TxFormat format_;
};
// the format of a verifying call for the stand-in of `kind` -- 0 HostTxDevice, 1 hashing, 2 chaining: base 1 and the device
// switches that class serves; out: what the caller is handed
TxFormat stand_in_format(int kind, const TxOutLayout& out = TxOutLayout()) {
  TxFormat f;
  f.base = TXFORMAT_V1; f.hash_on_device = kind >= 1; f.sign_on_device = kind >= 2; f.out = out;
  return f;
}
}  // namespace

// One call over a stand-in device, fail-closed in both outputs.  -> the call's return code; *n_chunks, *n_sig_stages: what was
// planned; *leaked: staged chunks never released (must be 0)
namespace {
int txcall_selftest(HostTxDevice& dev, size_t batch, const uint8_t* txs, const uint64_t* offs, int host_threads, size_t chunk, int n_slots,
                    uint8_t* accept_bitmap, uint8_t* status, size_t* n_chunks, size_t* n_sig_stages, size_t* leaked) {
  TxOutLayout().begin(accept_bitmap, status, batch);
  std::vector<TxStatement> store;
  int rc;
  {
    TxCall call(dev, store, (size_t)1 << 17, batch, txs, offs, host_threads, chunk, accept_bitmap, status, n_slots);
    *n_chunks = call.n_chunks();
    *n_sig_stages = call.n_sig_stages_planned();
    rc = call.run();
  }
  *leaked = dev.leaked();
  if (rc != 0) TxOutLayout().fail_closed(accept_bitmap, status, batch);
  return rc;
}
}  // namespace

extern "C" int zkhost_txcall_selftest(size_t batch, const uint8_t* txs, const uint64_t* offs, const uint8_t* proof_ok, int host_threads,
                                      size_t chunk, uint32_t delay_seed, int fail_at, uint8_t* accept_bitmap, uint8_t* status,
                                      size_t* n_chunks, size_t* n_sig_stages, size_t* leaked) {
  HostTxDevice dev(txs, offs, batch, proof_ok, delay_seed, fail_at, stand_in_format(0));
  return txcall_selftest(dev, batch, txs, offs, host_threads, chunk, 2, accept_bitmap, status, n_chunks, n_sig_stages, leaked);
}

// TWO calls driven by ONE thread through start / step / done / finish, one stage slot each -- how the engine of
// zkgpu_tx_verify_submit keeps two rounds in flight: the transactions [0, split) and [split, batch) as two calls whose steps
// alternate; the caller naps on a condition variable the calls' staging threads signal (on_news).  -> 0, or the first error
extern "C" int zkhost_txcall_pair_selftest(size_t batch, size_t split, const uint8_t* txs, const uint64_t* offs, const uint8_t* proof_ok,
                                           int host_threads, size_t chunk, uint32_t delay_seed, uint8_t* accept_bitmap, uint8_t* status,
                                           size_t* leaked) {
  TxOutLayout().begin(accept_bitmap, status, batch);
  if (split == 0 || split >= batch || split % 8) return -1;
  std::vector<TxStatement> store[2];
  std::vector<uint8_t> bits[2] = {std::vector<uint8_t>((split + 7) / 8 + 1, 0), std::vector<uint8_t>((batch - split + 7) / 8 + 1, 0)};
  std::mutex news_mu;
  std::condition_variable news_cv;
  bool news = false;
  int rc_all = 0;
  size_t leaked_all = 0;
  {
    HostTxDevice dev0(txs, offs, batch, proof_ok, delay_seed, -1, stand_in_format(0)), dev1(txs, offs, batch, proof_ok, delay_seed + 1, -1, stand_in_format(0));
    std::vector<TxCall::Piece> p0{{txs, offs, split}}, p1{{txs, offs + split, batch - split}};
    // (the second call's offsets are still relative to `txs`: Piece = base pointer + its own offsets)
    TxCall c0(dev0, store[0], (size_t)1 << 17, p0, host_threads, chunk, bits[0].data(), status, 1);
    TxCall c1(dev1, store[1], (size_t)1 << 17, p1, host_threads, chunk, bits[1].data(), status + split, 1);
    TxCall* calls[2] = {&c0, &c1};
    for (TxCall* c : calls) {
      c->set_on_news([&] { { std::lock_guard<std::mutex> nl(news_mu); news = true; } news_cv.notify_one(); });
      const int rc = c->start();
      if (rc != 0 && rc_all == 0) rc_all = rc;
    }
    while (!c0.done() || !c1.done()) {
      bool progress = false;
      for (TxCall* c : calls) if (!c->done()) progress |= c->step();
      if (!progress) {
        std::unique_lock<std::mutex> nl(news_mu);
        if (!news) news_cv.wait_until(nl, std::chrono::system_clock::now() + std::chrono::microseconds(50));
        news = false;
      }
    }
    // (the engine's rule: finish() only once the device has settled, so that it never sleeps inside one call)
    for (int spins = 0; !(c0.settled() && c1.settled()) && spins < 2000000; ++spins) std::this_thread::sleep_for(std::chrono::microseconds(20));
    for (TxCall* c : calls) { const int rc = c->finish(); if (rc != 0 && rc_all == 0) rc_all = rc; }
    leaked_all = dev0.leaked() + dev1.leaked();
  }
  *leaked = leaked_all;
  if (rc_all != 0) { TxOutLayout().fail_closed(accept_bitmap, status, batch); return rc_all; }
  for (size_t i = 0; i < split; ++i) if ((bits[0][i / 8] >> (i % 8)) & 1) accept_bitmap[i / 8] |= (uint8_t)(1u << (i % 8));
  for (size_t i = split; i < batch; ++i) { const size_t q = i - split; if ((bits[1][q / 8] >> (q % 8)) & 1) accept_bitmap[i / 8] |= (uint8_t)(1u << (i % 8)); }
  return 0;
}

// ---- the hash tape of a flagged transaction call (tx_hash_tape.hpp) on the CPU: the VM's structure pass over `count`
// ---- transactions as ONE chunk, the flattener, the interpreter -- the function k_tx_hash runs per lane -- and, beside it,
// ---- run_plan over the same plans.  Out: status per transaction; the block's head (16 words; its last, unused word holds
// ---- the STROBE position at which a contract-ID transcript starts, for the test's model of the rate boundary), its piece
// ---- records (4 words each, pieces_cap of them at most) and lane table; per
// ---- transaction its shape on the tape (0xffffffff: not on it) and first slot; the tape's transaction IDs (32 bytes per
// ---- transaction, zero where not on it); every slot as the tape left it and as run_plan did, and which of them the tape's
// ---- three protocols write (the others are the host's MuSig slots, which the tape leaves zero).
// ---- -> transactions on the tape, or -1 a plan the tape cannot hold, -2 the block fails hash_tape_check, -3 an output too small
#include "tx_hash_tape.hpp"
namespace {
// the taped second pass over `count` transactions as ONE chunk, the tape not yet finished; false: a plan the tape cannot hold
bool tape_one_chunk(const uint8_t* txs, const uint64_t* offs, size_t count, int threads, zk::zkvm::TxHashTape& tape, zk::zkvm::TxStatement* st) {
  std::atomic<int> bad{0};
  tape.reset(count);
  zk::zkvm::tx_groups_of_eight(count, threads, [&](size_t i) { return std::make_pair(txs + offs[i], (size_t)(offs[i + 1] - offs[i])); },
                               [&](const uint8_t** p, const size_t* l, size_t first, size_t n) {
                                 if (!zk::zkvm::tx_prepare_many_taped(p, l, st + first, n, tape, first)) bad = 1;
                               });
  return !bad;
}
}  // namespace
extern "C" long long zkhost_tx_hash_tape(const uint8_t* txs, const uint64_t* offs, size_t count, int threads, uint8_t* status,
                                         uint32_t* head16, uint32_t* pieces, size_t pieces_cap, uint32_t* lanes, size_t lanes_cap, uint32_t* tx_shape, uint64_t* tx_slot0,
                                         uint8_t* txid, uint8_t* slots_tape, uint8_t* slots_plan, uint8_t* slot_kept, size_t slots_cap) {
  using namespace zk::zkvm;
  TxHashTape tape;
  std::vector<TxStatement> st(count);
  const bool bad = !tape_one_chunk(txs, offs, count, threads, tape, st.data());
  for (size_t i = 0; i < count; ++i) { status[i] = (uint8_t)st[i].status; tx_shape[i] = TAPE_IDLE; tx_slot0[i] = 0; }
  std::memset(txid, 0, 32 * count);
  if (bad) return -1;
  tape.finish(threads);
  const HashTapeHead& h = tape.head();
  if (!hash_tape_check(tape.block(), h.words)) return -2;
  std::memcpy(head16, &h, 64);
  if (h.n_lanes > lanes_cap || h.n_slots > slots_cap || h.n_pieces > pieces_cap) return -3;
  std::memcpy(pieces, tape.block() + h.pieces, 16 * (size_t)h.n_pieces);
  std::memcpy(lanes, tape.block() + h.lanes, 4 * (size_t)h.n_lanes);
  std::vector<uint32_t> protos, sl, ids;
  std::vector<uint8_t> labels;
  hash_tape_constants(protos, labels);
  head16[15] = protos[(size_t)P_CONTRACTID * TAPE_PROTO_WORDS + 50];
  hash_tape_run_host(tape.block(), protos, labels, sl, ids);
  std::memcpy(slots_tape, sl.data(), 32 * (size_t)h.n_slots);
  std::memset(slots_plan, 0, 32 * (size_t)h.n_slots);
  std::memset(slot_kept, 0, h.n_slots);
  TxPlan P; TxSlots out; TxStatement s2;
  for (size_t t = 0; t < tape.n_tx(); ++t) {
    const size_t i = tape.position(t);
    const uint32_t* rec = tape.block() + h.txs + 4 * t;
    tx_shape[i] = rec[0]; tx_slot0[i] = rec[2];
    std::memcpy(txid + 32 * i, &ids[8 * t], 32);
    P.only = 0xff;
    tx_structure(txs + offs[i], (size_t)(offs[i + 1] - offs[i]), s2, P, out);
    if (s2.status != TX_OK || (uint64_t)rec[2] + P.n_slots > h.n_slots) return -2;
    run_plan(P, slots_plan + 32 * (size_t)rec[2]);
    for (const HashJob& j : P.jobs) if (tape_keeps(j.proto)) slot_kept[rec[2] + j.out_slot] = 1;
  }
  return (long long)tape.n_tx();
}

// ---- the scheduling of a FLAGGED call (a format that hashes: TxFormat::hashes) on the CPU: the stand-in above, and the
// ---- tapes of the chunks interpreted by tx_hash_run on a thread of their own after a random delay.  hash_fail_at: the
// ---- n-th hash_enqueue / hash_collect reports an error (-1: none).  *hashed: transaction IDs the stand-in produced.
namespace {
class HostHashingTxDevice : public HostTxDevice {
 public:
  HostHashingTxDevice(const uint8_t* txs, const uint64_t* offs, size_t batch, const uint8_t* proof_ok, uint32_t seed, int hash_fail_at, int fail_at, const TxFormat& format)
      : HostTxDevice(txs, offs, batch, proof_ok, seed, fail_at, format), hrng_(seed ^ 0x9e3779b9u), hash_fail_at_(hash_fail_at) { hash_tape_constants(protos_, labels_); }
  ~HostHashingTxDevice() override { for (auto& s : h_) if (s.th.joinable()) s.th.join(); }
  TxHashTape* hash_tape(int slot) override { return &h_[slot].tape; }
  int hash_enqueue(int slot, const TxHashTape& tape) override {
    HashStage& s = h_[slot];
    if (s.th.joinable()) { herr_ = "hash slot reused before it was collected"; return -1; }
    if (&tape != &s.tape || !hash_tape_check(tape.block(), tape.head().words)) { herr_ = "not this slot's tape, or a block that fails its check"; return -1; }
    if (hash_failing()) { herr_ = "injected fault of the hashing stage"; return -3; }
    s.done = false;
    const unsigned us = (unsigned)(hrng_() % 400);
    s.th = std::thread([this, &s, us] {
      std::this_thread::sleep_for(std::chrono::microseconds(us));
      hash_tape_run_host(s.tape.block(), protos_, labels_, s.slots, s.ids);
      // (the caller is handed the log: what k_tx_log_gather does, lane by lane, with the table the device would be sent)
      const size_t K = format_.log_k();
      s.log_ok = true;
      if (K && s.tape.n_tx()) {
        std::vector<uint32_t> table;
        s.log_ok = tx_log_table(s.tape.block(), table) && tx_log_lanes_fit(s.tape.n_tx(), K);
        s.log.assign(8 * K * s.tape.n_tx(), 0xa5a5a5a5u);
        for (uint32_t idx = 0; s.log_ok && idx < (uint32_t)(K * s.tape.n_tx()); ++idx)
          tx_log_gather_lane(s.tape.block(), table.data(), s.slots.data(), s.log.data(), idx, (uint32_t)K);
        if (s.log_ok) logged_ += tx_log_handed_back(s.tape.block(), table, K);
      }
      s.done = true;
    });
    return 0;
  }
  bool hash_done(int slot) override { return h_[slot].done; }
  int hash_collect(int slot, uint8_t* txids) override {
    HashStage& s = h_[slot];
    if (!s.th.joinable()) { herr_ = "nothing to collect in this hash slot"; return -1; }
    s.th.join();
    if (hash_failing()) { herr_ = "injected fault of the hashing stage"; return -3; }
    if (txids) { std::memcpy(txids, s.ids.data(), 32 * s.tape.n_tx()); ++id_asks_; }
    hashed_ += s.tape.n_tx();
    return 0;
  }
  std::string last_error() override { return herr_.empty() ? HostTxDevice::last_error() : herr_; }
  uint64_t hashed() const { return hashed_; }
  uint64_t id_asks() const { return id_asks_; }           // collects that were given a host buffer for the IDs
  const uint8_t* hash_log(int slot) override { return format_.log_k() && h_[slot].log_ok ? (const uint8_t*)h_[slot].log.data() : nullptr; }
  uint64_t logged() const { return logged_; }             // log entries the stand-in's gather handed back

 protected:
  struct HashStage { TxHashTape tape; std::thread th; std::atomic<bool> done{true}; std::vector<uint32_t> slots, ids, log; bool log_ok = true; };
  bool hash_failing() { return hash_fail_at_ >= 0 && hops_++ == hash_fail_at_; }
  HashStage h_[2];
  std::vector<uint32_t> protos_;
  std::vector<uint8_t> labels_;
  std::mt19937 hrng_;
  const int hash_fail_at_;
  int hops_ = 0;
  uint64_t hashed_ = 0, id_asks_ = 0;
  std::atomic<uint64_t> logged_{0};
  std::string herr_;
};
}  // namespace

extern "C" int zkhost_txcall_hashing_selftest(size_t batch, const uint8_t* txs, const uint64_t* offs, const uint8_t* proof_ok, int host_threads,
                                              size_t chunk, uint32_t delay_seed, int hash_fail_at, int n_slots, uint8_t* accept_bitmap,
                                              uint8_t* status, size_t* n_chunks, size_t* leaked, uint64_t* hashed) {
  HostHashingTxDevice dev(txs, offs, batch, proof_ok, delay_seed, hash_fail_at, -1, stand_in_format(1));
  size_t n_sig_stages;
  const int rc = txcall_selftest(dev, batch, txs, offs, host_threads, chunk, n_slots, accept_bitmap, status, n_chunks, &n_sig_stages, leaked);
  *hashed = dev.hashed();
  return rc;
}


// ---- the signature challenge of a flagged call (tx_sig_rows.hpp: ZKGPU_TXFORMAT_SIGN_ON_DEVICE) on the CPU: `count`
// ---- transactions as ONE chunk the way a chaining call treats it -- the taped second pass, the tape interpreted (the IDs
// ---- in the tape's order), the aggregated keys with the reference arithmetic, the chunk's signature rows with a_i in place,
// ---- the row -> tape map -- and tx_sig_row, the function k_tx_sig_rows runs per lane, over every row.  Beside it,
// ---- tx_finish_signature over the same statements.  Out, per transaction (zero where the VM did not accept it): status, the
// ---- number of keys, the ID, the aggregated key, R, and `cap` scalars each of a_i, of what tx_sig_row wrote and of what
// ---- tx_finish_signature wrote.  -> rows run, or -1 a plan the tape cannot hold, -2 no script, -3 more than `cap` keys
#include "tx_sig_rows.hpp"
extern "C" long long zkhost_tx_sig_rows(const uint8_t* txs, const uint64_t* offs, size_t count, int threads, size_t cap, uint8_t* status, uint32_t* n_keys,
                                        uint8_t* txid, uint8_t* agg, uint8_t* R, uint8_t* a_in, uint8_t* from_rows, uint8_t* from_host) {
  using namespace zk::zkvm;
  TxHashTape tape;
  std::vector<TxStatement> st(count);
  const bool bad = !tape_one_chunk(txs, offs, count, threads, tape, st.data());
  std::memset(n_keys, 0, 4 * count); std::memset(txid, 0, 32 * count); std::memset(agg, 0, 32 * count); std::memset(R, 0, 32 * count);
  std::memset(a_in, 0, 32 * cap * count); std::memset(from_rows, 0, 32 * cap * count); std::memset(from_host, 0, 32 * cap * count);
  for (size_t i = 0; i < count; ++i) status[i] = (uint8_t)st[i].status;
  if (bad) return -1;
  tape.finish(threads);
  std::vector<uint32_t> protos, sl, ids;
  std::vector<uint8_t> labels;
  hash_tape_constants(protos, labels);
  hash_tape_run_host(tape.block(), protos, labels, sl, ids);
  SigScript script;
  if (!sig_script(script)) return -2;
  std::vector<size_t> live;
  for (size_t i = 0; i < count; ++i) if (st[i].status == TX_OK) live.push_back(i);
  std::vector<uint32_t> at(count, TAPE_IDLE), pos(live.size());
  for (size_t t = 0; t < tape.n_tx(); ++t) at[tape.position(t)] = (uint32_t)t;
  std::vector<uint64_t> soff(live.size() + 1, 0);
  for (size_t q = 0; q < live.size(); ++q) {
    const size_t k = st[live[q]].sig_scalars.size() / 32 - 2;
    if (k > cap || at[live[q]] == TAPE_IDLE) return -3;
    pos[q] = at[live[q]];
    soff[q + 1] = soff[q] + k + 1;
  }
  std::vector<uint32_t> ssc(8 * soff.back() + 8), spt(8 * soff.back() + 8), aggw(8 * live.size() + 8, 0);
  uint8_t base[32];
  { ge B; B.X = fe_BASE_X(); B.Y = fe_BASE_Y(); B.Z = fe_one(); B.T = fe_BASE_T(); encode_point(base, B); }
  for (size_t q = 0; q < live.size(); ++q) {
    TxStatement& t = st[live[q]];
    const size_t i = live[q], k = t.sig_scalars.size() / 32 - 2;
    std::memcpy(&ssc[8 * soff[q]], t.sig_scalars.data() + 32, 32 * (k + 1));
    std::memcpy(&spt[8 * soff[q]], t.sig_points.data() + 32, 32 * (k + 1));
    ge acc;
    ge_identity(acc);
    if (add_terms(acc, t.sig_scalars.data(), t.sig_points.data(), 2, 2 + k)) encode_point((uint8_t*)&aggw[8 * q], acc);             // (a key that does not decode: zeros, as the key stage leaves them)
    n_keys[i] = (uint32_t)k;
    std::memcpy(txid + 32 * i, &ids[8 * pos[q]], 32);
    std::memcpy(agg + 32 * i, &aggw[8 * q], 32);
    std::memcpy(R + 32 * i, &t.sig_points[32], 32);
    std::memcpy(a_in + 32 * cap * i, &t.sig_scalars[64], 32 * k);
    TxStatement h = t;
    std::memcpy(h.txid, &ids[8 * pos[q]], 32);
    tx_finish_signature(h, base, (const uint8_t*)&aggw[8 * q]);
    std::memcpy(from_host + 32 * cap * i, &h.sig_scalars[64], 32 * k);
  }
  SigRowsView v{&script, ids.data(), pos.data(), aggw.data(), soff.data(), spt.data(), ssc.data(), (uint32_t)live.size()};
  sig_rows_run_host(v);
  for (size_t q = 0; q < live.size(); ++q)
    std::memcpy(from_rows + 32 * cap * live[q], &ssc[8 * (soff[q] + 1)], 32 * (size_t)n_keys[live[q]]);
  return (long long)live.size();
}

// ---- the scheduling of a call that CHAINS (TxFormat::chains) on the CPU: the hashing stand-in above, plus a signature stage
// ---- that waits -- on its own thread, as the device waits on events -- for the key stage of key_slot and the tape of hash_slot,
// ---- forms the challenges with tx_sig_row and then checks the rows like the unchained stage.  sig_fail_at: the n-th
// ---- chained sigs_enqueue / sigs_collect reports an error (-1: none).  *signed_rows: rows whose challenge the stand-in produced.
namespace {
class HostChainingTxDevice : public HostHashingTxDevice {
 public:
  HostChainingTxDevice(const uint8_t* txs, const uint64_t* offs, size_t batch, const uint8_t* proof_ok, uint32_t seed, int sig_fail_at, int hash_fail_at, int fail_at,
                       const TxFormat& format)
      : HostHashingTxDevice(txs, offs, batch, proof_ok, seed, hash_fail_at, fail_at, format), crng_(seed ^ 0x51ed270bu), sig_fail_at_(sig_fail_at) { have_script_ = sig_script(script_); }
  int sigs_enqueue(int slot, size_t rows, const uint8_t* dsc, const uint8_t* dpt, const uint64_t* doff, const uint8_t* bsc, const SigChain* chain) override {
    if (!chain) { cerr_ = "an unchained signature stage on a device that chains"; return -1; }
    const uint32_t* tape_pos = chain->tape_pos;
    Stage& s = sigs_[slot];
    Stage& ks = keys_[chain->key_slot];
    HashStage& hs = h_[chain->hash_slot];
    if (!have_script_) { cerr_ = "no script of the signature transcript"; return -1; }
    if (s.th.joinable()) { cerr_ = "signature slot reused before it was collected"; return -1; }
    if (!ks.th.joinable() || !hs.th.joinable()) { cerr_ = "a chained signature stage without its key stage or its tape in flight"; return -1; }
    if (ks.values.size() != 32 * rows) { cerr_ = "the key stage of the slot has other rows than the signature stage"; return -1; }
    for (size_t r = 0; r < rows; ++r) if (tape_pos[r] >= hs.tape.n_tx()) { cerr_ = "a row names a transaction the tape does not hold"; return -1; }
    if (sig_failing()) { cerr_ = "injected fault of the chained signature stage"; return -3; }
    s.done = false;
    s.ok.assign((rows + 7) / 8 + 1, 0);
    s.values.assign(dsc, dsc + 32 * doff[rows]);          // (the stage's own copy of the scalars, as the device's buffer is: -c a_i go here)
    const unsigned us = (unsigned)(crng_() % 400);
    s.th = std::thread([=, &s, &ks, &hs] {
      std::this_thread::sleep_for(std::chrono::microseconds(us));
      while (!ks.done || !hs.done) std::this_thread::sleep_for(std::chrono::microseconds(20));
      std::vector<uint32_t> sc(s.values.size() / 4 + 8), pt(8 * doff[rows] + 8), agg(8 * rows + 8);
      std::memcpy(sc.data(), s.values.data(), s.values.size());
      std::memcpy(pt.data(), dpt, 32 * doff[rows]);
      std::memcpy(agg.data(), ks.values.data(), 32 * rows);
      SigRowsView v{&script_, hs.ids.data(), tape_pos, agg.data(), doff, pt.data(), sc.data(), (uint32_t)rows};
      sig_rows_run_host(v);
      std::memcpy(s.values.data(), sc.data(), s.values.size());
      sig_rows_check(s, rows, s.values.data(), dpt, doff, bsc);
      signed_ += rows;
      s.done = true;
    });
    return 0;
  }
  int sigs_collect(int slot, uint8_t* bits, uint8_t* why) override {
    const int rc = HostHashingTxDevice::sigs_collect(slot, bits, why);
    if (rc == 0 && sig_failing()) { cerr_ = "injected fault of the chained signature stage"; return -3; }
    return rc;
  }
  std::string last_error() override { return cerr_.empty() ? HostHashingTxDevice::last_error() : cerr_; }
  uint64_t signed_rows() const { return signed_; }

 private:
  bool sig_failing() { return sig_fail_at_ >= 0 && sops_++ == sig_fail_at_; }
  SigScript script_;
  bool have_script_ = false;
  std::mt19937 crng_;
  const int sig_fail_at_;
  int sops_ = 0;
  std::atomic<uint64_t> signed_{0};
  std::string cerr_;
};
}  // namespace

extern "C" int zkhost_txcall_chaining_selftest(size_t batch, const uint8_t* txs, const uint64_t* offs, const uint8_t* proof_ok, int host_threads,
                                               size_t chunk, uint32_t delay_seed, int sig_fail_at, int n_slots, uint8_t* accept_bitmap,
                                               uint8_t* status, size_t* n_chunks, size_t* n_sig_stages, size_t* leaked, uint64_t* hashed,
                                               uint64_t* signed_rows) {
  HostChainingTxDevice dev(txs, offs, batch, proof_ok, delay_seed, sig_fail_at, -1, -1, stand_in_format(2));
  const int rc = txcall_selftest(dev, batch, txs, offs, host_threads, chunk, n_slots, accept_bitmap, status, n_chunks, n_sig_stages, leaked);
  *hashed = dev.hashed();
  *signed_rows = dev.signed_rows();
  return rc;
}

// ---- a call whose caller is handed more than bits and status bytes -- the transaction IDs (TxFormat::ids: ZKGPU_TXFORMAT_RETURN_IDS),
// ---- the log's entries (TxFormat::log_k: ZKGPU_TXFORMAT_RETURN_LOG) -- on the CPU, over any of the three stand-ins above, with the
// ---- LIBRARY's own layout code (tx_out.hpp): begin, piece, the round's hand-out and the fail-closed clean-up are the functions
// ---- session.hpp calls.  kind 0: HostTxDevice, 1: hashing, 2: chaining.  fail_at: the n-th operation of stage fail_stage fails
// ---- (-1: none) -- 0 keys / proofs / unchained signatures, 1 the hashing stage, 2 the chained signature stage.
namespace {
std::unique_ptr<HostTxDevice> tx_stand_in(int kind, int fail_stage, int fail_at, const uint8_t* txs, const uint64_t* offs, size_t batch, const uint8_t* proof_ok,
                                          uint32_t delay_seed, const TxFormat& format) {
  const int f0 = fail_stage == 0 ? fail_at : -1, f1 = fail_stage == 1 ? fail_at : -1, f2 = fail_stage == 2 ? fail_at : -1;
  if (kind == 0) return std::unique_ptr<HostTxDevice>(new HostTxDevice(txs, offs, batch, proof_ok, delay_seed, f0, format));
  if (kind == 1) return std::unique_ptr<HostTxDevice>(new HostHashingTxDevice(txs, offs, batch, proof_ok, delay_seed, f1, f0, format));
  return std::unique_ptr<HostTxDevice>(new HostChainingTxDevice(txs, offs, batch, proof_ok, delay_seed, f2, f1, f0, format));
}
struct TxOutSelftest { size_t chunks = 0, leaked = 0, host_hashed = 0; uint64_t id_asks = 0, hashed = 0, logged = 0; bool dirty = false; };
// split = 0: a lone call, status_a its whole status argument under layout la.  split > 0 (a multiple of 8, < batch): [0, split)
// and [split, batch) as two callers' pieces of ONE merged call, as a round of zkgpu_tx_verify_submit holds them: one bitmap and
// one status array for the round, handed out to status_a (la) and status_b (lb), each caller's bits to its part of accept_bitmap.
// dirty: a failed call had left something behind a caller's status bytes before it was fail-closed (must not be).
int tx_out_selftest(int kind, TxOutLayout la, TxOutLayout lb, size_t batch, size_t split, const uint8_t* txs, const uint64_t* offs, const uint8_t* proof_ok,
                    int host_threads, size_t chunk, uint32_t delay_seed, int fail_at, int fail_stage, int n_slots, uint8_t* accept_bitmap,
                    uint8_t* status_a, uint8_t* status_b, TxOutSelftest& t) {
  if (kind < 0 || kind > 2 || fail_stage < 0 || fail_stage > kind || !status_a || (split && (split >= batch || split % 8 || !status_b))) return -1;
  const size_t na = split ? split : batch, nb = split ? batch - split : 0;
  TxFormat format = stand_in_format(kind);               // (the round's device brings back what the wider of its calls asks for)
  format.out.ids = la.ids || (nb && lb.ids);
  format.out.log_k = std::max(la.log_k, nb ? lb.log_k : 0);
  const std::unique_ptr<HostTxDevice> dev = tx_stand_in(kind, fail_stage, fail_at, txs, offs, batch, proof_ok, delay_seed, format);
  const TxHandOut to[2] = {{na, la, accept_bitmap, status_a}, {nb, lb, accept_bitmap + split / 8, status_b}};
  for (const TxHandOut& h : to) if (h.batch) h.layout.begin(h.bits, h.area, h.batch);
  std::vector<uint8_t> round_bits((batch + 7) / 8 + 1, 0), round_status(split ? batch : 0, (uint8_t)TX_INVALID);
  std::vector<TxStatement> store;
  int rc;
  {
    std::unique_ptr<TxCall> call;
    if (split == 0) {
      call.reset(new TxCall(*dev, store, (size_t)1 << 17, batch, txs, offs, host_threads, chunk, round_bits.data(), status_a, n_slots));
    } else {
      std::vector<TxCall::Piece> pieces{la.piece(txs, offs, na, status_a), lb.piece(txs, offs + split, nb, status_b)};
      call.reset(new TxCall(*dev, store, (size_t)1 << 17, pieces, host_threads, chunk, round_bits.data(), round_status.data(), n_slots));
    }
    t.chunks = call->n_chunks();
    rc = call->run();
    t.host_hashed = call->n_host_hashed();
  }
  t.leaked = dev->leaked();
  if (kind >= 1) {
    const HostHashingTxDevice& h = *static_cast<const HostHashingTxDevice*>(dev.get());
    t.id_asks = h.id_asks(); t.hashed = h.hashed(); t.logged = h.logged();
  }
  for (const TxHandOut& h : to)
    for (size_t i = h.batch; rc != 0 && i < h.layout.bytes(h.batch); ++i) if (h.area[i]) t.dirty = true;
  if (split) {
    tx_round_hand_out(round_bits.data(), round_status.data(), rc == 0, to, 2);
  } else if (rc != 0) {
    la.fail_closed(accept_bitmap, status_a, batch);
  } else {
    std::memcpy(accept_bitmap, round_bits.data(), (batch + 7) / 8);
  }
  return rc;
}
}  // namespace

// ---- the transaction IDs: status_a / status_b are 33 bytes per transaction (1 when return_ids = 0).  out[0] chunks, out[1] staged
// ---- chunks never released, out[2] hash_collect calls that were given a host buffer, out[3] transactions whose ID the HOST's second
// ---- pass hashed, out[4] IDs the stand-in's hashing stage produced, out[5] the body's `dirty` (must be 0)
extern "C" int zkhost_txcall_ids_selftest(int kind, int return_ids, size_t batch, size_t split, const uint8_t* txs, const uint64_t* offs,
                                          const uint8_t* proof_ok, int host_threads, size_t chunk, uint32_t delay_seed, int fail_at, int fail_stage,
                                          int n_slots, uint8_t* accept_bitmap, uint8_t* status_a, uint8_t* status_b, uint64_t* out) {
  for (int q = 0; q < 6; ++q) out[q] = 0;
  TxOutLayout lay;
  lay.ids = return_ids != 0;
  TxOutSelftest t;
  const int rc = tx_out_selftest(kind, lay, lay, batch, split, txs, offs, proof_ok, host_threads, chunk, delay_seed, fail_at, fail_stage, n_slots,
                                 accept_bitmap, status_a, status_b, t);
  out[0] = t.chunks; out[1] = t.leaked; out[2] = t.id_asks; out[3] = t.host_hashed; out[4] = t.hashed; out[5] = t.dirty;
  return rc;
}

// ---- ... and the log's entries with window K: kind 0, the host's second pass fills the records; 1, 2: the hashing stage gathers
// ---- the entries' contract IDs (tx_log_gather_lane, the kernel's code) and the call adds counts and kinds.  status_a is 33 + 1 +
// ---- 33 K bytes per transaction, status_b 33 + 1 + 33 k_b with a window of its own (0: K).  out[0] chunks, out[1] staged chunks
// ---- never released, out[2] transactions the HOST's second pass hashed, out[3] IDs the stand-in's hashing stage produced, out[4]
// ---- log entries its gather handed back, out[5] the body's `dirty` (must be 0)
extern "C" int zkhost_txcall_log_selftest(int kind, size_t K, size_t k_b, size_t batch, size_t split, const uint8_t* txs, const uint64_t* offs,
                                          const uint8_t* proof_ok, int host_threads, size_t chunk, uint32_t delay_seed, int fail_at, int fail_stage,
                                          int n_slots, uint8_t* accept_bitmap, uint8_t* status_a, uint8_t* status_b, uint64_t* out) {
  for (int q = 0; q < 6; ++q) out[q] = 0;
  if (K < 1 || K > 255 || k_b > 255) return -1;
  TxOutLayout la, lb;
  la.ids = lb.ids = true;
  la.log_k = K; lb.log_k = k_b ? k_b : K;
  TxOutSelftest t;
  const int rc = tx_out_selftest(kind, la, lb, batch, split, txs, offs, proof_ok, host_threads, chunk, delay_seed, fail_at, fail_stage, n_slots,
                                 accept_bitmap, status_a, status_b, t);
  out[0] = t.chunks; out[1] = t.leaked; out[2] = t.host_hashed; out[3] = t.hashed; out[4] = t.logged; out[5] = t.dirty;
  return rc;
}

// ---- the layout header itself (tx_out.hpp), for the CPU test.  op 0: the format word in[0] -> out: valid, base, hash, sign, ids,
// ---- K, precompute-only.  Ops 1 .. 4 take a layout in[0] = ids, in[1] = K and a batch in[2]: op 1 -> out: bytes(batch), the offsets of the status
// ---- byte / ID / record of transaction in[3] and of a piece's ID / record areas (-1: not there), the piece's window; op 2 begin,
// ---- 3 nothing-in-the-subset, 4 fail-closed over bitmap and area (either may be NULL).  op 5, a round's hand-out: in[0] calls,
// ---- in[1] ok, then (ids, K, batch) per call; bitmap / area hold the ROUND's bits / status bytes, out_bits / out_area the
// ---- calls' bitmaps ((batch + 7) / 8 bytes each) and areas one behind the other.  op 6, the round rule (tx_round_mates,
// ---- tx_round_format): in[0] the word the round's first call was submitted under, in[1] the word in force now, in[2] the word a
// ---- candidate was submitted under (all three valid) -> out: does the candidate share the round, then the round format's base,
// ---- hash, sign, precompute-only, reasons.  -> 0, -1 on bad arguments
extern "C" int zkhost_tx_out_layout(int op, const int64_t* in, uint8_t* bitmap, uint8_t* area, uint8_t* out_bits, uint8_t* out_area, int64_t* out) {
  if (!in || op < 0 || op > 6 || ((op <= 1 || op == 6) && !out)) return -1;
  const auto layout = [](const int64_t* q) { TxOutLayout l; l.ids = q[0] != 0; l.log_k = (size_t)q[1]; return l; };
  if (op == 0) {
    TxFormat f;
    const int64_t r[7] = {TxFormat::of((int)in[0], &f), f.base, f.hash_on_device, f.sign_on_device, f.out.ids, (int64_t)f.out.log_k, f.precompute_only};
    std::copy(r, r + 7, out);
    return 0;
  }
  if (op == 6) {
    TxFormat first, now, candidate;
    if (!TxFormat::of((int)in[0], &first) || !TxFormat::of((int)in[1], &now) || !TxFormat::of((int)in[2], &candidate)) return -1;
    const TxFormat f = tx_round_format(first, now);
    const int64_t r[6] = {tx_round_mates(candidate, first), f.base, f.hash_on_device, f.sign_on_device, f.precompute_only, f.reasons()};
    std::copy(r, r + 6, out);
    return 0;
  }
  if (op == 5) {
    std::vector<TxHandOut> to;
    for (int64_t c = 0; c < in[0]; ++c) {
      to.push_back({(size_t)in[4 + 3 * c], layout(in + 2 + 3 * c), out_bits, out_area});
      out_bits += (to.back().batch + 7) / 8; out_area += to.back().layout.bytes(to.back().batch);
    }
    tx_round_hand_out(bitmap, area, in[1] != 0, to.data(), to.size());
    return 0;
  }
  const TxOutLayout lay = layout(in);
  const size_t batch = (size_t)in[2];
  if (op == 2) lay.begin(bitmap, area, batch);
  if (op == 3) lay.nothing_in_subset(area, batch);
  if (op == 4) lay.fail_closed(bitmap, area, batch);
  if (op != 1) return 0;
  uint8_t* const base = (uint8_t*)(uintptr_t)4096;        // (offsets only: nothing is read or written)
  const auto at = [&](const uint8_t* p) { return p ? (int64_t)(p - base) : (int64_t)-1; };
  const TxPiece pc = lay.piece(nullptr, nullptr, batch, base);
  const int64_t r[7] = {(int64_t)lay.bytes(batch), at(lay.status_of(base, (size_t)in[3])), at(lay.id_of(base, batch, (size_t)in[3])),
                        at(lay.record_of(base, batch, (size_t)in[3])), at(pc.ids), at(pc.log), (int64_t)pc.log_k};
  std::copy(r, r + 7, out);
  return 0;
}

// ---- tx_prepare_many_logged (tx_log.hpp) and tx_prepare_many (zkvm_tx.hpp) are two sets of parameters of ONE second pass
// ---- (tx_run_group); what must not differ between them is guarded here: the two passes side by side over the same transactions in the same groups of eight, statement by statement -- status, reason text, header,
// ---- transaction ID, arity, commitments, where the proof lies, the signature's scalars and points.  -> statements that differ
// ---- (must be 0), -1 on bad arguments.  *lockstep_groups (may be NULL): groups of eight whose plans had one shape, i.e. that
// ---- AVX-512 hashes in lockstep where the CPU has it -- so that a test knows it compared both ways of running the plans.
extern "C" long long zkhost_tx_prepare_logged_compare(const uint8_t* txs, const uint64_t* offs, size_t batch, size_t K, uint64_t* lockstep_groups) {
  if (!txs || !offs || K < 1 || K > 255) return -1;
  long long differ = 0;
  uint64_t same_shape_groups = 0;
  std::vector<uint8_t> recs(8 * tx_log_record_bytes(K));
  for (size_t first = 0; first < batch; first += 8) {
    const size_t cnt = std::min<size_t>(8, batch - first);
    const uint8_t* p[8];
    size_t l[8];
    for (size_t q = 0; q < cnt; ++q) { p[q] = txs + offs[first + q]; l[q] = (size_t)(offs[first + q + 1] - offs[first + q]); }
    TxStatement a[8], b[8];
    std::fill(recs.begin(), recs.end(), (uint8_t)0);
    tx_prepare_many(p, l, a, cnt, true, ALL_PROTOS);
    tx_prepare_many_logged(p, l, b, cnt, recs.data(), K);
    bool one_shape = cnt >= 3;
    TxPlan P0, P;
    TxSlots out;
    TxStatement s2;
    for (size_t q = 0; q < cnt; ++q) {
      const TxStatement &x = a[q], &y = b[q];
      const bool same = x.status == y.status && std::strcmp(x.why, y.why) == 0 && x.version == y.version && x.mintime == y.mintime &&
                        x.maxtime == y.maxtime && std::memcmp(x.txid, y.txid, 32) == 0 && x.n_in == y.n_in && x.n_out == y.n_out &&
                        x.commitments.size() == y.commitments.size() && std::memcmp(x.commitments.data(), y.commitments.data(), x.commitments.size()) == 0 &&
                        x.proof == y.proof && x.proof_len == y.proof_len && x.sig_scalars.size() == y.sig_scalars.size() &&
                        std::memcmp(x.sig_scalars.data(), y.sig_scalars.data(), x.sig_scalars.size()) == 0 && x.sig_points.size() == y.sig_points.size() &&
                        std::memcmp(x.sig_points.data(), y.sig_points.data(), x.sig_points.size()) == 0;
      if (!same) ++differ;
      // (a statement the VM does not accept has no record)
      if (x.status != TX_OK) for (size_t i = 0; i < tx_log_record_bytes(K); ++i) if (recs[q * tx_log_record_bytes(K) + i]) { ++differ; break; }
      (q == 0 ? P0 : P).only = 0xff;
      tx_structure(p[q], l[q], s2, q == 0 ? P0 : P, out);
      if (s2.status != TX_OK || (q > 0 && !P.same_shape(P0))) one_shape = false;
    }
    if (one_shape) ++same_shape_groups;
  }
  if (lockstep_groups) *lockstep_groups = same_shape_groups;
  return differ;
}

// ---- the hash tape walked by dependency level (tx_hash_levels.hpp) on the CPU: `count` transactions as ONE chunk the way a
// ---- precompute-only call tapes it (no job run on the host), the side table, and the level interpreter -- the function
// ---- k_tx_hash_levels runs per lane -- level by level and lane by lane with `lanes` lanes per transaction, beside tx_hash_run
// ---- over the same block.  Out: status per transaction; the block and the table (words; sizes[0], sizes[1]: how many, sizes[2]:
// ---- slots); per transaction (zero where not on the tape) the ID the level walk left and the one tx_hash_run left;
// ---- sizes[3]: slot words on which the two differ (must be 0).
// ---- -> transactions on the tape, or -1 a plan the tape cannot hold, -2 the block fails hash_tape_check, -3 an output too small,
// ---- -4 no side table
#include "tx_hash_levels.hpp"
extern "C" long long zkhost_tx_hash_levels(const uint8_t* txs, const uint64_t* offs, size_t count, int threads, uint32_t lanes, uint8_t* status,
                                           uint32_t* block, size_t block_cap, uint32_t* table, size_t table_cap, uint64_t* sizes,
                                           uint8_t* txid_levels, uint8_t* txid_run) {
  using namespace zk::zkvm;
  TxHashTape tape;
  std::vector<TxStatement> st(count);
  std::atomic<int> bad{0};
  tape.reset(count);
  tx_groups_of_eight(count, threads, [&](size_t i) { return std::make_pair(txs + offs[i], (size_t)(offs[i + 1] - offs[i])); },
                     [&](const uint8_t** p, const size_t* l, size_t first, size_t n) {
                       if (!tx_prepare_many_taped(p, l, &st[first], n, tape, first, NO_PROTO)) bad = 1;
                     });
  for (size_t i = 0; i < count; ++i) status[i] = (uint8_t)st[i].status;
  std::memset(txid_levels, 0, 32 * count); std::memset(txid_run, 0, 32 * count);
  for (int q = 0; q < 4; ++q) sizes[q] = 0;
  if (bad) return -1;
  tape.finish(threads);
  const HashTapeHead& h = tape.head();
  if (!hash_tape_check(tape.block(), h.words)) return -2;
  std::vector<uint32_t> tab, protos, sl, ids, lsl, lids;
  std::vector<uint8_t> labels;
  if (!tx_hash_levels_table(tape.block(), tab)) return -4;
  sizes[0] = h.words; sizes[1] = tab.size(); sizes[2] = h.n_slots;
  if (h.words > block_cap || tab.size() > table_cap) return -3;
  std::memcpy(block, tape.block(), 4 * (size_t)h.words);
  std::memcpy(table, tab.data(), 4 * tab.size());
  hash_tape_constants(protos, labels);
  hash_tape_run_host(tape.block(), protos, labels, sl, ids);
  if (!hash_tape_run_levels_host(tape.block(), protos, labels, lanes, lsl, lids)) return -4;
  for (size_t w = 0; w < sl.size(); ++w) sizes[3] += sl[w] != lsl[w];
  for (size_t t = 0; t < tape.n_tx(); ++t) {
    std::memcpy(txid_levels + 32 * tape.position(t), &lids[8 * t], 32);
    std::memcpy(txid_run + 32 * tape.position(t), &ids[8 * t], 32);
  }
  return (long long)tape.n_tx();
}

// ---- a PRECOMPUTE-ONLY call (TxFormat::precompute: ZKGPU_TXFORMAT_PRECOMPUTE_ONLY) on the CPU: TxCall over a stand-in that
// ---- hashes (hashing = 1: the tapes interpreted as above, hash_fail_at as there) or not, with reasons (format 2) or without, the
// ---- caller handed IDs and, K > 0, the log -- and that COUNTS every key, proof and signature operation it is asked for: there
// ---- must be none.  status is laid out by tx_out.hpp (33 + (K ? 1 + 33 K : 0) bytes per transaction), begun and fail-closed as
// ---- session.hpp does it.  out[0] chunks, out[1] key / proof / signature operations asked for (must be 0), out[2] transactions
// ---- the host's pass hashed, out[3] IDs the stand-in's hashing stage produced, out[4] transactions that left with
// ---- PRECOMPUTED, out[5] something lay behind the status bytes of a failed call before it was fail-closed (must be 0)
namespace {
class HostPrecomputeTxDevice : public HostHashingTxDevice {
 public:
  HostPrecomputeTxDevice(const uint8_t* txs, const uint64_t* offs, size_t batch, uint32_t seed, int hash_fail_at, const TxFormat& format)
      : HostHashingTxDevice(txs, offs, batch, nullptr, seed, hash_fail_at, -1, format) {}
  int keys_enqueue(int, const uint8_t*, const uint8_t*, const uint64_t*, size_t) override { return asked(); }
  int keys_collect(int, uint8_t*, uint8_t*, uint8_t*) override { return asked(); }
  int proofs_stage(size_t, size_t, const TxProofSource*, int, void**, std::string*) override { return asked(); }
  int proofs_start(size_t, void*) override { return asked(); }
  int proofs_finish(void*, uint8_t*, uint8_t*) override { return asked(); }
  void proofs_release(void*) override { (void)asked(); }
  int sigs_enqueue(int, size_t, const uint8_t*, const uint8_t*, const uint64_t*, const uint8_t*, const SigChain*) override { return asked(); }
  int sigs_collect(int, uint8_t*, uint8_t*) override { return asked(); }
  uint64_t stage_ops() const { return stage_ops_; }

 private:
  int asked() { ++stage_ops_; return -1; }
  std::atomic<uint64_t> stage_ops_{0};
};
}  // namespace

extern "C" int zkhost_txcall_precompute_selftest(int hashing, int reasons, size_t K, size_t batch, const uint8_t* txs, const uint64_t* offs, int host_threads,
                                                 size_t chunk, uint32_t delay_seed, int hash_fail_at, int n_slots, uint8_t* accept_bitmap, uint8_t* status,
                                                 uint64_t* out) {
  for (int q = 0; q < 6; ++q) out[q] = 0;
  if (K > 255 || !status || !accept_bitmap) return -1;
  TxFormat format;
  format.base = reasons ? TXFORMAT_V1_REASONS : TXFORMAT_V1;
  format.hash_on_device = hashing != 0; format.precompute_only = true;
  format.out.ids = true; format.out.log_k = K;
  HostPrecomputeTxDevice dev(txs, offs, batch, delay_seed, hash_fail_at, format);
  format.out.begin(accept_bitmap, status, batch);
  std::vector<TxStatement> store;
  int rc;
  {
    TxCall call(dev, store, (size_t)1 << 17, batch, txs, offs, host_threads, chunk, accept_bitmap, status, n_slots);
    out[0] = call.n_chunks();
    rc = call.run();
    out[2] = call.n_host_hashed();
    out[4] = rc == 0 ? call.n_precomputed() : 0;
  }
  out[1] = dev.stage_ops(); out[3] = dev.hashed();
  for (size_t i = batch; rc != 0 && i < format.out.bytes(batch); ++i) if (status[i]) out[5] = 1;
  if (rc != 0) format.out.fail_closed(accept_bitmap, status, batch);
  return rc;
}

// ---- records of what the caller's own VM left (tx_statements.hpp; ZKGPU_TXFORMAT_STATEMENTS_V1) on the CPU ---------------------
#include "tx_musig_rows.hpp"
#include "tx_statements.hpp"

// ---- the parser alone.  -> the statement's status (0 ok, 1 invalid, 2 unsupported); out_u32: n_in, n_out, terms, proof offset in
// ---- the record, proof length; why: the reason text (up to 63 bytes, NUL-terminated); txid 32 bytes; commitments (cap_com bytes
// ---- of room), scalars / points (cap_terms * 32 bytes of room each): copied as far as they fit
extern "C" int zkhost_tx_statement_parse(const uint8_t* rec, size_t len, uint32_t* out_u32, char* why, uint8_t* txid, uint8_t* commitments, size_t cap_com,
                                         uint8_t* scalars, uint8_t* points, size_t cap_terms) {
  TxStatement st;
  tx_statement_parse(rec, len, st);
  out_u32[0] = st.n_in; out_u32[1] = st.n_out; out_u32[2] = (uint32_t)(st.sig_scalars.size() / 32);
  out_u32[3] = st.proof ? (uint32_t)(st.proof - rec) : 0; out_u32[4] = (uint32_t)st.proof_len;
  std::strncpy(why, st.why, 63); why[63] = 0;
  std::memcpy(txid, st.txid, 32);
  std::memcpy(commitments, st.commitments.data(), std::min(cap_com, st.commitments.size()));
  std::memcpy(scalars, st.sig_scalars.data(), std::min(32 * cap_terms, st.sig_scalars.size()));
  std::memcpy(points, st.sig_points.data(), std::min(32 * cap_terms, st.sig_points.size()));
  return (int)st.status;
}

// ---- the records of a group of up to eight with the host's MuSig jobs run (lockstep != 0: eight-wide where the CPU can): per
// ---- record its status and, at scalars + 32 * 66 * i, its terms' scalars (s, -1, a_0 ..)
extern "C" void zkhost_tx_statements_group(const uint8_t* recs, const uint64_t* offs, size_t count, int lockstep, uint8_t* status, uint8_t* scalars) {
  const uint8_t* p[8];
  size_t l[8];
  TxStatement st[8];
  count = std::min<size_t>(count, 8);
  for (size_t q = 0; q < count; ++q) { p[q] = recs + offs[q]; l[q] = (size_t)(offs[q + 1] - offs[q]); }
  tx_statements_many(p, l, st, count, true, lockstep != 0);
  for (size_t q = 0; q < count; ++q) {
    status[q] = (uint8_t)st[q].status;
    std::memcpy(scalars + 32 * 66 * q, st[q].sig_scalars.data(), st[q].sig_scalars.size());
  }
}

// ---- musig_row, the function k_musig_rows runs per lane, over every row: scalars (32 bytes per term, in and out -- the key
// ---- terms are written), points, offsets (rows + 1), skip.  trace[3]: where the sponge's rate boundary fell (tx_musig_rows.hpp).
// ---- -> 0, -1: no script / bad arguments
extern "C" int zkhost_musig_rows(uint8_t* scalars, const uint8_t* points, const uint64_t* offsets, size_t rows, uint32_t skip, uint32_t* trace) {
  MusigScript sc;
  if (!musig_script(sc) || !scalars || !points || !offsets || rows >= (1u << 31)) return -1;
  for (size_t r = 0; r < rows; ++r) if (offsets[r + 1] < offsets[r] + skip + 1) return -1;
  const size_t n = (size_t)offsets[rows];
  std::vector<uint32_t> sw(8 * n + 8), pw(8 * n + 8);
  std::memcpy(sw.data(), scalars, 32 * n);
  std::memcpy(pw.data(), points, 32 * n);
  uint32_t tr[3] = {0, 0, 0};
  const MusigRowsView v{&sc, offsets, pw.data(), sw.data(), (uint32_t)rows, skip, tr};
  musig_rows_run_host(v);
  std::memcpy(scalars, sw.data(), 32 * n);
  if (trace) std::memcpy(trace, tr, sizeof tr);
  return 0;
}

// ---- the recipe the device's script is recorded from (tx_musig_jobs) against what the VM's plan holds for one serialized
// ---- transaction: job for job and piece for piece -- protocol, labels, kinds, lengths, immediates, the bytes of the keys, the
// ---- challenge's label and length.  -> the number of MuSig jobs compared (= the keys), -1: they differ, -2: the VM rejects it
extern "C" long long zkhost_musig_recipe_compare(const uint8_t* tx, size_t len) {
  TxStatement st;
  TxPlan P;
  TxSlots out;
  P.only = 0xff;
  tx_structure(tx, len, st, P, out);
  if (st.status != TX_OK) return -2;
  const size_t k = st.sig_points.size() / 32 - 2;
  std::vector<const uint8_t*> keys(k);
  for (size_t j = 0; j < k; ++j) keys[j] = &st.sig_points[32 * (2 + j)];
  MusigRecorder rec;
  std::vector<uint32_t> slots;
  tx_musig_jobs(rec, keys.data(), k, slots);
  size_t at = 0;
  for (const HashJob& j : P.jobs) {
    if (j.proto != P_MUSIG) continue;
    if (at >= rec.jobs.size()) return -1;
    const MusigRecorder::Job& r = rec.jobs[at++];
    if (r.proto != j.proto || r.chal_label != j.chal_label || r.out_len != j.out_len || r.pieces.size() != j.count) return -1;
    for (uint32_t q = 0; q < j.count; ++q) {
      const HashPiece& h = P.pieces[j.first + q];
      const MusigRecorder::Piece& rp = r.pieces[q];
      if (h.label != rp.label || h.len != rp.len || h.msg_len != rp.len || (h.kind == HashPiece::Imm) != rp.imm || h.kind == HashPiece::Slot) return -1;
      uint8_t imm[8];
      for (int b = 0; b < 8; ++b) imm[b] = (uint8_t)(rp.value >> (8 * b));
      if (std::memcmp(piece_bytes(P, h, nullptr), rp.imm ? imm : rp.p, h.len) != 0) return -1;
    }
  }
  return at == rec.jobs.size() && at == k ? (long long)at : -1;
}

// ---- the scheduling of a statements call (TxCall::step_statements) on the CPU: the stand-in of zkhost_txcall_selftest under a
// ---- statements format, which refuses every hashing operation and -- forms_musig() -- forms the coefficients itself: a key stage that
// ---- arrives as points alone (musig_row with skip 0, then the stage), a signature stage that arrives as a chain with the host's
// ---- IDs (musig_row with skip 1, tx_sig_row over those IDs once the slot's key stage is through, then the equations).
namespace {
class HostStatementsTxDevice : public HostTxDevice {
 public:
  HostStatementsTxDevice(const uint8_t* recs, const uint64_t* offs, size_t batch, const uint8_t* proof_ok, uint32_t seed, int fail_at, const TxFormat& format)
      : HostTxDevice(recs, offs, batch, proof_ok, seed, fail_at, format), srng_(seed ^ 0x3c6ef372u) {
    have_scripts_ = musig_script(musig_) && sig_script(script_);
  }
  TxHashTape* hash_tape(int) override { ++hash_asks_; return nullptr; }
  int hash_enqueue(int, const TxHashTape&) override { ++hash_asks_; return -1; }
  int hash_collect(int, uint8_t*) override { ++hash_asks_; return -1; }
  int keys_enqueue(int slot, const uint8_t* sc, const uint8_t* pt, const uint64_t* off, size_t rows) override {
    if (format_.forms_musig()) { err_ = "a key stage with scalars on a device that forms them"; return -1; }
    return HostTxDevice::keys_enqueue(slot, sc, pt, off, rows);
  }
  int keys_enqueue_formed(int slot, const uint8_t* pt, const uint64_t* off, size_t rows) override {
    if (!format_.forms_musig() || !have_scripts_) { err_ = "a key stage without scalars on a device that does not form them"; return -1; }
    std::vector<uint8_t>& sc = formed_[slot];
    sc.assign(32 * off[rows], 0);
    if (zkhost_musig_rows(sc.data(), pt, off, rows, 0, nullptr) != 0) { err_ = "a key row without a key"; return -1; }
    return HostTxDevice::keys_enqueue(slot, sc.data(), pt, off, rows);
  }
  int keys_collect(int slot, uint8_t* ok_bits, uint8_t* values, uint8_t* why) override {
    const int rc = HostTxDevice::keys_collect(slot, ok_bits, values, why);
    if (rc == 0 && why) for (size_t r = 0; 32 * r < keys_[slot].values.size(); ++r) why[r] = ((ok_bits[r / 8] >> (r % 8)) & 1) ? 0 : TxCall::WHY_KEY;
    return rc;
  }
  int proofs_finish(void* handle, uint8_t* accept_bits, uint8_t* why) override {
    const size_t n = ((Proofs*)handle)->src.size();
    const int rc = HostTxDevice::proofs_finish(handle, accept_bits, why);
    if (rc == 0 && why) for (size_t r = 0; r < n; ++r) why[r] = ((accept_bits[r / 8] >> (r % 8)) & 1) ? 0 : (uint8_t)(TxCall::WHY_PROOF_FIRST + 2);
    return rc;
  }
  int sigs_enqueue(int slot, size_t rows, const uint8_t* dsc, const uint8_t* dpt, const uint64_t* doff, const uint8_t* bsc, const SigChain* chain) override {
    sig_rows_[slot] = rows;
    if (!format_.forms_musig()) return HostTxDevice::sigs_enqueue(slot, rows, dsc, dpt, doff, bsc, chain);
    if (!chain || !chain->txids || !have_scripts_) { err_ = "a signature stage of a device that forms the coefficients without the host's IDs"; return -1; }
    if (failing()) return -3;
    Stage& s = sigs_[slot];
    Stage& ks = keys_[chain->key_slot];
    if (s.th.joinable()) { err_ = "signature slot reused before it was collected"; return -1; }
    if (!ks.th.joinable() || ks.values.size() != 32 * rows) { err_ = "a chained signature stage without its key stage in flight"; return -1; }
    s.done = false;
    s.ok.assign((rows + 7) / 8 + 1, 0);
    s.values.assign(dsc, dsc + 32 * doff[rows]);
    const uint8_t* ids = chain->txids;
    const unsigned us = (unsigned)(srng_() % 400);
    s.th = std::thread([=, &s, &ks] {
      std::this_thread::sleep_for(std::chrono::microseconds(us));
      (void)zkhost_musig_rows(s.values.data(), dpt, doff, rows, 1, nullptr);
      while (!ks.done) std::this_thread::sleep_for(std::chrono::microseconds(20));
      std::vector<uint32_t> sc(s.values.size() / 4 + 8), pt(8 * doff[rows] + 8), agg(8 * rows + 8), idw(8 * rows + 8), pos(rows);
      std::memcpy(sc.data(), s.values.data(), s.values.size());
      std::memcpy(pt.data(), dpt, 32 * doff[rows]);
      std::memcpy(agg.data(), ks.values.data(), 32 * rows);
      std::memcpy(idw.data(), ids, 32 * rows);
      for (size_t r = 0; r < rows; ++r) pos[r] = (uint32_t)r;
      SigRowsView v{&script_, idw.data(), pos.data(), agg.data(), doff, pt.data(), sc.data(), (uint32_t)rows};
      sig_rows_run_host(v);
      std::memcpy(s.values.data(), sc.data(), s.values.size());
      sig_rows_check(s, rows, s.values.data(), dpt, doff, bsc);
      formed_rows_ += rows;
      s.done = true;
    });
    return 0;
  }
  int sigs_collect(int slot, uint8_t* bits, uint8_t* why) override {
    const int rc = HostTxDevice::sigs_collect(slot, bits, why);
    if (rc == 0 && why) for (size_t r = 0; r < sig_rows_[slot]; ++r) why[r] = ((bits[r / 8] >> (r % 8)) & 1) ? 0 : TxCall::WHY_SIGNATURE;
    return rc;
  }
  uint64_t hash_asks() const { return hash_asks_; }
  uint64_t formed_rows() const { return formed_rows_; }

 private:
  std::mt19937 srng_;
  MusigScript musig_;
  SigScript script_;
  bool have_scripts_ = false;
  std::vector<uint8_t> formed_[2];
  size_t sig_rows_[2] = {0, 0};
  std::atomic<uint64_t> hash_asks_{0}, formed_rows_{0};
};
}  // namespace

// One statements call over the stand-in, fail-closed in both outputs (status: one byte per record; may be NULL).  on_device: the
// stand-in forms a_i and c (0x204) or the host's transcripts do (4).  out[0] chunks, out[1] staged chunks never released, out[2]
// hashing operations asked for (must be 0), out[3] records whose second pass the host hashed (must be 0), out[4] signature rows
// whose coefficients the stand-in formed
extern "C" int zkhost_txcall_statements_selftest(int on_device, int reasons, size_t batch, const uint8_t* recs, const uint64_t* offs, const uint8_t* proof_ok,
                                                 int host_threads, size_t chunk, uint32_t delay_seed, int fail_at, int n_slots, uint8_t* accept_bitmap,
                                                 uint8_t* status, uint64_t* out) {
  for (int q = 0; q < 5; ++q) out[q] = 0;
  if (!accept_bitmap || !recs || !offs || !proof_ok) return -1;
  TxFormat format;
  format.base = TXFORMAT_STATEMENTS_V1; format.sign_on_device = on_device != 0; format.mute = reasons == 0;
  HostStatementsTxDevice dev(recs, offs, batch, proof_ok, delay_seed, fail_at, format);
  TxOutLayout().begin(accept_bitmap, status, batch);
  std::vector<TxStatement> store;
  int rc;
  {
    TxCall call(dev, store, (size_t)1 << 17, batch, recs, offs, host_threads, chunk, accept_bitmap, status, n_slots);
    out[0] = call.n_chunks();
    rc = call.run();
    out[3] = call.n_host_hashed();
  }
  out[1] = dev.leaked(); out[2] = dev.hash_asks(); out[4] = dev.formed_rows();
  if (rc != 0) TxOutLayout().fail_closed(accept_bitmap, status, batch);
  return rc;
}

// ---- WHAT THE DEVICE IS ASKED, recorded (tests/test_tx_call_sequences.py holds it against tests/golden/tx_call_sequences.json):
// ---- a wrapper that forwards every call of TxCall to a stand-in and notes, in the order they arrive, (operation, slot or ring
// ---- slot, rows, detail).  rows of a collect: those of the stage that was queued in the slot; detail: the terms of a key stage,
// ---- 0 / 1 / 2 for a signature stage with final scalars / chained to a tape / chained with the host's IDs, 1 for a hash_collect
// ---- that was given a host buffer.  (proofs_stage comes from the staging thread: the list has a lock of its own.)
#include <map>
namespace {
class TracingTxDevice : public TxDevice {
 public:
  enum Op : int64_t { KEYS_ENQUEUE, KEYS_ENQUEUE_FORMED, KEYS_COLLECT, PROOFS_STAGE, PROOFS_START, PROOFS_FINISH, SIGS_ENQUEUE, SIGS_COLLECT, HASH_ENQUEUE, HASH_COLLECT };
  explicit TracingTxDevice(TxDevice& in) : in_(in) {}
  const std::vector<int64_t>& trace() const { return trace_; }
  const uint8_t* basepoint() override { return in_.basepoint(); }
  int keys_enqueue(int slot, const uint8_t* sc, const uint8_t* pt, const uint64_t* off, size_t rows) override {
    key_rows_[slot] = rows;
    saw(KEYS_ENQUEUE, slot, rows, off[rows]);
    return in_.keys_enqueue(slot, sc, pt, off, rows);
  }
  int keys_enqueue_formed(int slot, const uint8_t* pt, const uint64_t* off, size_t rows) override {
    key_rows_[slot] = rows;
    saw(KEYS_ENQUEUE_FORMED, slot, rows, off[rows]);
    return in_.keys_enqueue_formed(slot, pt, off, rows);
  }
  bool keys_done(int slot) override { return in_.keys_done(slot); }
  int keys_collect(int slot, uint8_t* ok_bits, uint8_t* values, uint8_t* why) override {
    saw(KEYS_COLLECT, slot, key_rows_[slot], 0);
    return in_.keys_collect(slot, ok_bits, values, why);
  }
  int proofs_stage(size_t ring_slot, size_t n, const TxProofSource* src, int host_threads, void** handle, std::string* err) override {
    const int rc = in_.proofs_stage(ring_slot, n, src, host_threads, handle, err);
    std::lock_guard<std::mutex> lk(mu_);
    if (rc == 0) staged_[*handle] = {ring_slot, n};
    note(PROOFS_STAGE, ring_slot, n, 0);
    return rc;
  }
  int proofs_start(size_t ring_slot, void* handle) override { saw(PROOFS_START, ring_slot, staged(handle).second, 0); return in_.proofs_start(ring_slot, handle); }
  bool proofs_done(void* handle) override { return in_.proofs_done(handle); }
  int proofs_finish(void* handle, uint8_t* accept_bits, uint8_t* why) override {
    const auto at = staged(handle);
    saw(PROOFS_FINISH, at.first, at.second, 0);
    return in_.proofs_finish(handle, accept_bits, why);
  }
  void proofs_release(void* handle) override { in_.proofs_release(handle); }
  int sigs_enqueue(int slot, size_t rows, const uint8_t* dsc, const uint8_t* dpt, const uint64_t* doff, const uint8_t* bsc, const SigChain* chain) override {
    sig_rows_[slot] = rows;
    saw(SIGS_ENQUEUE, slot, rows, !chain ? 0 : chain->txids ? 2 : 1);
    return in_.sigs_enqueue(slot, rows, dsc, dpt, doff, bsc, chain);
  }
  bool sigs_done(int slot) override { return in_.sigs_done(slot); }
  int sigs_collect(int slot, uint8_t* bits, uint8_t* why) override { saw(SIGS_COLLECT, slot, sig_rows_[slot], 0); return in_.sigs_collect(slot, bits, why); }
  std::string last_error() override { return in_.last_error(); }
  TxHashTape* hash_tape(int slot) override { return in_.hash_tape(slot); }
  int hash_enqueue(int slot, const TxHashTape& tape) override {
    hash_rows_[slot] = tape.n_tx();
    saw(HASH_ENQUEUE, slot, tape.n_tx(), 0);
    return in_.hash_enqueue(slot, tape);
  }
  bool hash_done(int slot) override { return in_.hash_done(slot); }
  int hash_collect(int slot, uint8_t* txids) override { saw(HASH_COLLECT, slot, hash_rows_[slot], txids != nullptr); return in_.hash_collect(slot, txids); }
  const uint8_t* hash_log(int slot) override { return in_.hash_log(slot); }
  const TxFormat& format() const override { return in_.format(); }

 private:
  void note(int64_t op, size_t slot, size_t rows, uint64_t detail) { const int64_t e[4] = {op, (int64_t)slot, (int64_t)rows, (int64_t)detail}; trace_.insert(trace_.end(), e, e + 4); }     // (mu_ held)
  void saw(int64_t op, size_t slot, size_t rows, uint64_t detail) { std::lock_guard<std::mutex> lk(mu_); note(op, slot, rows, detail); }
  std::pair<size_t, size_t> staged(void* handle) { std::lock_guard<std::mutex> lk(mu_); return staged_[handle]; }
  TxDevice& in_;
  std::mutex mu_;
  std::vector<int64_t> trace_;
  std::map<void*, std::pair<size_t, size_t>> staged_;      // a staged chunk's ring slot and proofs
  size_t key_rows_[2] = {0, 0}, sig_rows_[2] = {0, 0}, hash_rows_[2] = {0, 0};
};
}  // namespace

// One CLEAN call (no injected fault) under the format word `word` over the stand-in the word calls for -- transactions, or for
// the statements words their records -- and what the device was asked.  out: the trace, four values per operation, `cap`
// operations of room; plan[0] chunks, plan[1] signature stages planned.  -> operations noted, or -1 bad arguments (a word that
// is refused or enables nothing among them), -2 the call failed, -3 more than `cap` operations
extern "C" long long zkhost_txcall_trace(int word, int n_slots, size_t chunk, size_t batch, const uint8_t* txs, const uint64_t* offs, const uint8_t* proof_ok,
                                         int host_threads, uint32_t delay_seed, int64_t* out, size_t cap, uint64_t* plan) {
  TxFormat format;
  if (!TxFormat::of(word, &format) || format.base == 0 || !txs || !offs || !proof_ok || !out || !plan) return -1;
  std::unique_ptr<HostTxDevice> dev;
  if (format.statements()) dev.reset(new HostStatementsTxDevice(txs, offs, batch, proof_ok, delay_seed, -1, format));
  else if (format.precompute()) dev.reset(new HostPrecomputeTxDevice(txs, offs, batch, delay_seed, -1, format));
  else dev = tx_stand_in(format.chains() ? 2 : format.hashes() ? 1 : 0, 0, -1, txs, offs, batch, proof_ok, delay_seed, format);
  TracingTxDevice traced(*dev);
  std::vector<uint8_t> bitmap((batch + 7) / 8 + 1), status(format.out.bytes(batch));
  format.out.begin(bitmap.data(), status.data(), batch);
  std::vector<TxStatement> store;
  {
    TxCall call(traced, store, (size_t)1 << 17, batch, txs, offs, host_threads, chunk, bitmap.data(), status.data(), n_slots);
    plan[0] = call.n_chunks(); plan[1] = call.n_sig_stages_planned();
    if (call.run() != 0) return -2;
  }
  const size_t n = traced.trace().size() / 4;
  if (n > cap) return -3;
  std::copy(traced.trace().begin(), traced.trace().end(), out);
  return (long long)n;
}

// ---- ZKGPU_TXFORMAT_RETURN_ROOT on the CPU (tx_out.hpp with the flag, tx_root.hpp), for tests/test_tx_root_host.py.  op 0: the
// ---- format word in[0] -> out: valid, base, hash, sign, ids, K, precompute-only, root.  Ops 1 .. 4 take a layout in[0] = ids,
// ---- in[1] = K, in[2] = root and a batch in[3]: op 1 -> out: bytes(batch), the offset of the root and of a piece's root (-1: not
// ---- there); op 2 begin, 3 nothing-in-the-subset, 4 fail-closed over bitmap and area (either may be NULL).  op 5, a round's
// ---- hand-out: in[0] calls, in[1] ok, then (ids, K, root, batch) per call; bitmap / area hold the ROUND's bits / status bytes,
// ---- data the round's roots (32 bytes per call), out_bits / out_area the calls' bitmaps and areas one behind the other.
// ---- op 6, the host fold: in[0] = n IDs at data, in[1] = the span (levels per pass; anything outside 1 .. 7: the default),
// ---- in[2] = host threads -> 32 bytes at out_area; out[0] = passes.  -> 0, -1 on bad arguments
#include "tx_root.hpp"
extern "C" int zkhost_tx_root(int op, const int64_t* in, const uint8_t* data, uint8_t* bitmap, uint8_t* area, uint8_t* out_bits, uint8_t* out_area, int64_t* out) {
  if (!in || op < 0 || op > 6 || ((op <= 1 || op == 6) && !out)) return -1;
  const auto layout = [](const int64_t* q) { TxOutLayout l; l.ids = q[0] != 0; l.log_k = (size_t)q[1]; l.root = q[2] != 0; return l; };
  if (op == 0) {
    TxFormat f;
    const int64_t r[8] = {TxFormat::of((int)in[0], &f), f.base, f.hash_on_device, f.sign_on_device, f.out.ids, (int64_t)f.out.log_k, f.precompute_only, f.out.root};
    std::copy(r, r + 8, out);
    return 0;
  }
  if (op == 6) {
    if (in[0] < 0 || (in[0] > 0 && !data) || !out_area) return -1;
    tx_root_fold_host(data, (size_t)in[0], (uint32_t)std::max<int64_t>(0, std::min<int64_t>(in[1], 64)), (int)in[2], out_area);
    out[0] = tx_root_passes((uint64_t)in[0], tx_root_span(in[1]));
    return 0;
  }
  if (op == 5) {
    if (!data) return -1;
    std::vector<TxHandOut> to;
    for (int64_t c = 0; c < in[0]; ++c) {
      to.push_back({(size_t)in[5 + 4 * c], layout(in + 2 + 4 * c), out_bits, out_area, data + 32 * c});
      out_bits += (to.back().batch + 7) / 8; out_area += to.back().layout.bytes(to.back().batch);
    }
    tx_round_hand_out(bitmap, area, in[1] != 0, to.data(), to.size());
    return 0;
  }
  const TxOutLayout lay = layout(in);
  const size_t batch = (size_t)in[3];
  if (op == 2) lay.begin(bitmap, area, batch);
  if (op == 3) lay.nothing_in_subset(area, batch);
  if (op == 4) lay.fail_closed(bitmap, area, batch);
  if (op != 1) return 0;
  uint8_t* const base = (uint8_t*)(uintptr_t)4096;        // (offsets only: nothing is read or written)
  const auto at = [&](const uint8_t* p) { return p ? (int64_t)(p - base) : (int64_t)-1; };
  const TxPiece pc = lay.piece(nullptr, nullptr, batch, base);
  const int64_t r[3] = {(int64_t)lay.bytes(batch), at(lay.root_of(base, batch)), at(pc.root)};
  std::copy(r, r + 3, out);
  return 0;
}
