// prover_call_plan_check.cpp -- the plan of a device prover call (zkvm_amd/csrc/prover_call_plan.hpp) in a program of its
// own, for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_prover_call_plan.py compiles and runs it): for an 8-bit
// range statement, a shuffle of two, a system without commitments and the 2-in/2-out cloak, batches of 1, 5 and 9, with and
// without a seed of the call's own: plan, fill the scaffolding into a heap buffer of EXACTLY lay_bytes, copy the blob into one
// of exactly its words and read every table of the view over it from its first to its last word.
#include "../zkvm_amd/csrc/prover_call_plan.hpp"

#include <cstdio>
#include <memory>

using namespace zk;

namespace {
using Term = R1csDesc::Term;
Term term(VarKind kind, uint32_t idx, int coeff, int chal = -1, uint32_t pow = 0) {
  return Term{kind, idx, coeff < 0 ? -Scalar::from_u64((uint64_t)-coeff) : Scalar::from_u64((uint64_t)coeff), chal, pow};
}

R1csDesc range_bits(uint32_t bits) {
  R1csDesc d;
  d.label = "zkvm_amd.gadget"; d.m = 1; d.n1 = d.n = bits;
  std::vector<Term> acc{term(VarKind::Committed, 0, 1)};
  for (uint32_t i = 0; i < bits; ++i) {
    d.cons.push_back({term(VarKind::MulOut, i, 1)});
    d.cons.push_back({term(VarKind::MulLeft, i, 1), term(VarKind::MulRight, i, 1), term(VarKind::One, 0, -1)});
    acc.push_back(term(VarKind::MulRight, i, -(1 << i)));
  }
  d.cons.push_back(acc);
  return d;
}

R1csDesc shuffle_two() {      // (x_1 - z)(x_0 - z) = (y_1 - z)(y_0 - z), z a second-phase challenge
  R1csDesc d;
  d.label = "zkvm_amd.gadget"; d.m = 4; d.n1 = 0; d.n = 2;
  d.chal_names = {"shuffle challenge"};
  for (uint32_t i = 0; i < 2; ++i) {
    d.cons.push_back({term(VarKind::Committed, 2 * i + 1, 1), term(VarKind::One, 0, -1, 0, 1), term(VarKind::MulLeft, i, -1)});
    d.cons.push_back({term(VarKind::Committed, 2 * i, 1), term(VarKind::One, 0, -1, 0, 1), term(VarKind::MulRight, i, -1)});
  }
  d.cons.push_back({term(VarKind::MulOut, 0, 1), term(VarKind::MulOut, 1, -1)});
  return d;
}

R1csDesc no_commitments() {   // one multiplier, handed in, whose product is zero
  R1csDesc d;
  d.label = "zkvm_amd.gadget"; d.m = 0; d.n1 = d.n = 1;
  d.cons.push_back({term(VarKind::MulOut, 0, 1)});
  return d;
}

uint64_t check(const char* name, const PvHostPlan& hp, bool cloak) {
  uint64_t sum = 0;
  for (size_t batch : {1, 5, 9})
    for (int W : {8, 19})
      for (int flags = 0; flags < 4; ++flags) {
        const PvCallPlan p = plan_prover_call(hp, batch, W, {(flags & 1) != 0, cloak, (flags & 2) != 0});
        std::unique_ptr<uint8_t[]> lay(new uint8_t[p.lay_bytes]);
        if (!p.fill_scaffolding(lay.get())) { std::printf("%s: scaffolding out of step\n", name); std::exit(1); }
        for (size_t i = 0; i < p.lay_bytes; ++i) sum += lay[i];
        std::unique_ptr<uint32_t[]> blob(new uint32_t[p.blob.size()]);
        std::memcpy(blob.get(), p.blob.data(), p.blob.size() * 4);
        const PvPlan v = p.view(blob.get());
#define X(f) for (size_t i = 0; i < hp.f.size(); ++i) { if (v.f[i] != hp.f[i]) { std::printf("%s: table " #f " differs\n", name); std::exit(1); } sum += v.f[i]; }
        PV_PLAN_TABLES(X)
#undef X
        for (size_t i = 0; i < hp.chal_labels.size(); ++i) { if (v.chal_labels[i] != hp.chal_labels[i]) std::exit(1); }
        if (p.at.draw) for (size_t i = 0; i < (size_t)PV_DRAW_ENTRY_WORDS * (hp.sh.m + 1); ++i) sum += blob[p.at.draw + i];
        for (size_t i = 0; i < 5; ++i) sum += blob[p.blob.size() - 8 + i];      // the key
        sum += p.steps.size() + p.in.bytes + p.ws.st_partials;
      }
  return sum;
}
}  // namespace

int main() {
  uint64_t sum = 0;
  const std::vector<uint32_t> given8(16, PV_GIVEN), given1(2, PV_GIVEN);
  sum += check("range 8", pv_build(range_bits(8), given8, 8), false);
  sum += check("shuffle 2", pv_build(shuffle_two(), {0, 1, 2, 3}, 2), false);
  sum += check("no commitments", pv_build(no_commitments(), given1, 1), false);
  R1csDesc d;
  std::vector<uint32_t> md;
  PvCloakTrace::trace(2, 2, d, md);
  sum += check("cloak 2x2", pv_build(d, md, 256), true);
  std::printf("ok: %llu\n", (unsigned long long)sum);
  return 0;
}
