// prover_seed.hpp -- the host side of a prover call without seeds (include/zkgpu.h: seeds == NULL; prover_draw.hpp): the call's
// one seed from the OS, its life in host memory, and the launch of k_pv_draw.  A piece of zkgpu.hip, included there inside
// its unnamed namespace ahead of the provers (like session.hpp it uses the context, HIP_TRY, Launch and os_random of that file).
#pragma once

bool test_hooks_enabled();   // (session.hpp)

// a secret leaves host memory (stores the compiler may not drop)
inline void wipe(void* p, size_t n) {
  volatile uint8_t* v = (volatile uint8_t*)p;
  while (n--) *v++ = 0;
}

// ONE seed for the whole call, from which statement i of the call -- whatever slice proves it -- gets seed_i.  The seed is a
// secret: it leaves host memory with this object, and the context keeps a copy only for a process that asked for the hooks
// before it loaded the library (zkgpu_debug_read "prover_seed"; zero after a call that brought its own seeds).  The lockstep
// provers (mode 1) take their seeds from host memory: seed_0 || seed_1 || ..., by the host side of the same derivation.
struct PvCallSeed {
  uint8_t b[32] = {0};
  bool drawn = false;
  std::vector<uint8_t> per_statement;
  ~PvCallSeed() {
    wipe(b, sizeof b);
    if (!per_statement.empty()) wipe(per_statement.data(), per_statement.size());
  }
  // *seeds NULL: draws (c->mu held).  false: the OS gave no randomness -- last_error says so, nothing has been launched
  bool begin(zkgpu_ctx* c, const uint8_t** seeds, size_t batch) {
    memset(c->prover_seed, 0, sizeof c->prover_seed);
    if (*seeds) return true;
    if (!os_random(b, sizeof b)) { wipe(b, sizeof b); c->last_error = "getrandom failed"; return false; }
    drawn = true;
    if (test_hooks_enabled()) memcpy(c->prover_seed, b, sizeof b);
    if (c->prover_mode == 1) {
      per_statement.resize(32 * batch);
      for (size_t i = 0; i < batch; ++i) pv_statement_seed(b, i, &per_statement[32 * i]);
      *seeds = per_statement.data();
    }
    return true;
  }
  // the seed the device prover derives from; NULL: the call brought its seeds, or the lockstep provers have theirs
  const uint8_t* for_device(const zkgpu_ctx* c) const { return drawn && c->prover_mode != 1 ? b : nullptr; }
  // a call that drew its seed and failed publishes nothing (a call with seeds of its own answers as it always did)
  int closed(int rc, uint8_t* commitments, size_t com_bytes, uint8_t* proofs, size_t proof_bytes, size_t* proof_len) const {
    if (drawn && rc != ZKGPU_OK) { memset(commitments, 0, com_bytes); memset(proofs, 0, proof_bytes); *proof_len = 0; }
    return rc;
  }
};

// Blinding factors (unless the caller brought them: draw_blindings false) and rng seeds of statements first .. first + batch - 1
// of the call, drawn into the regions of the input area that prove_device otherwise fills by upload; table: the m + 1 entries
// in the plan blob.  The launch is collected here: a draw that was not made must fail the call, not leave an earlier call's
// bytes in its place.
inline int pv_draw_launch(zkgpu_ctx* c, hipStream_t s, const uint8_t call_seed[32], uint64_t first, size_t batch, uint32_t m, bool draw_blindings,
                          const uint32_t* table, void* d_blindings, void* d_rng_seed) {
  const uint32_t d0 = draw_blindings ? 0u : m;
  const uint64_t lanes = (uint64_t)batch * (m + 1 - d0);
  DrawSeed ds = draw_seed(call_seed);
  {
    Launch l(c, "k_pv_draw");
    hipLaunchKernelGGL(k_pv_draw, dim3(blocks_for(lanes, 64)), dim3(64), 0, s, ds, first, lanes, m, d0, table, (uint32_t*)d_blindings, (uint32_t*)d_rng_seed);
  }
  wipe(&ds, sizeof ds);
  HIP_TRY(c, hipGetLastError());
  return ZKGPU_OK;
}
