// tx_sig_rows.hpp -- the challenge of a transaction's signature formed where its inputs already lie (zkgpu.h:
// ZKGPU_TXFORMAT_SIGN_ON_DEVICE): per signature row the transcript of zkvm_tx.hpp's tx_finish_signature, its challenge c
// reduced mod l, and the row's MuSig coefficients a_i overwritten with the canonical bytes of -c a_i -- tx_sig_row, one
// function for the host and the device (k_tx_sig_rows runs it one lane per row; the CPU tests and libzkhost run the same code).
//
// WHAT is hashed is not written down here.  sig_script() runs tx_finish_signature itself over a recording transcript and
// keeps what it saw: the messages in order, each with its label, its length and WHERE its bytes come from -- the transaction
// ID, the aggregated key, R (told apart by the address the function read them from) or bytes of its own (the domain
// separator: copied) -- and the label of the challenge.  The kernel interprets that script; no label and no domain separator
// is restated, and a change of tx_finish_signature changes both sides.
//
// A row is a row of the signature stage's dynamic terms (tx_call.hpp): term 0 = (-1, R), terms 1.. = (a_i, X_i).  Its
// transaction ID lies in the hashing stage's dense array at txid[8 * tape_pos[row]], its aggregated key in the key stage's
// values at agg[8 * row] (all zero when a key did not decode: defined bytes, and the row's equation fails on that key anyway).
#pragma once
#include <stdint.h>

#include "tx_hash_tape.hpp"   // TapeStrobe and its operations; ZK_TAPE_HD
#include "sc_dev.hpp"

namespace zk {
namespace zkvm {

constexpr uint32_t SIG_CONST = 0, SIG_TXID = 1, SIG_KEY = 2, SIG_R = 3;      // where a message's bytes come from
constexpr uint32_t SIG_MAX_MSG = 8, SIG_POOL_WORDS = 64;
struct SigScript {
  uint32_t init[TAPE_PROTO_WORDS];      // the initial transcript of P_SIGNTX (50 state words, position, begin marker)
  uint32_t n_msg, chal_label, chal_len, zero;
  uint32_t msg[SIG_MAX_MSG][4];         // label, source, length, offset of a SIG_CONST message's bytes in the pool
  uint32_t pool[SIG_POOL_WORDS];        // label texts and constant bytes.  A label is (byte offset | length << 16)
};
static_assert(sizeof(SigScript) % 16 == 0, "whole uint4s");

struct SigRowsView {
  const SigScript* script;
  const uint32_t* txid;                 // hashing stage: 8 words per transaction of the tape
  const uint32_t* tape_pos;             // per row: which of them
  const uint32_t* agg;                  // key stage: 8 words per row
  const uint64_t* offsets;              // rows + 1: the rows' extents in points / scalars
  const uint32_t* points;               // 8 words per term
  uint32_t* scalars;                    // 8 words per term; a_i -> -c a_i in place
  uint32_t rows;
};

// meta-AD of a label of the pool, then of a 32-bit length (continued): what opens append_message / challenge_bytes
ZK_TAPE_HD inline void sig_label_len(TapeStrobe& s, const uint32_t* pool, uint32_t label, uint32_t len) {
  tape_begin_op(s, 16u | 2u);
  tape_absorb(s, pool, label & 0xffffu, label >> 16);
  for (int i = 0; i < 4; ++i) tape_absorb_byte(s, (len >> (8 * i)) & 0xffu);
}

// st: 50 words of scratch, word i at st[i * stride]
ZK_TAPE_HD inline void tx_sig_row(const SigRowsView& v, uint32_t row, uint32_t* st, uint32_t stride) {
  const SigScript& sc = *v.script;
  const uint64_t t0 = v.offsets[row], t1 = v.offsets[row + 1];
  if (t1 <= t0) return;                                  // (no such row is made: R is the row's first term)
  for (uint32_t i = 0; i < 50; ++i) st[i * stride] = sc.init[i];
  TapeStrobe s{st, stride, sc.init[50], sc.init[51]};
  for (uint32_t m = 0; m < sc.n_msg; ++m) {
    const uint32_t kind = sc.msg[m][1], len = sc.msg[m][2];
    sig_label_len(s, sc.pool, sc.msg[m][0], len);
    tape_begin_op(s, 2u);
    if (kind == SIG_TXID) tape_absorb(s, v.txid + 8 * (size_t)v.tape_pos[row], 0, len);
    else if (kind == SIG_KEY) tape_absorb(s, v.agg + 8 * (size_t)row, 0, len);
    else if (kind == SIG_R) tape_absorb(s, v.points + 8 * t0, 0, len);
    else tape_absorb(s, sc.pool, sc.msg[m][3], len);
  }
  sig_label_len(s, sc.pool, sc.chal_label, sc.chal_len);
  tape_begin_op(s, 1u | 2u | 4u);                        // PRF: the position is 0 afterwards, the 64 bytes the first 16 words
  uint32_t wide[16];
  for (uint32_t i = 0; i < 16; ++i) wide[i] = st[i * stride];
  const scm c = scm_from_wide(wide);
  for (uint64_t t = t0 + 1; t < t1; ++t) {
    uint32_t* a = v.scalars + 8 * t;
    uint32_t w[8];
    for (int i = 0; i < 8; ++i) w[i] = a[i];
    scm_to_words(w, scm_neg(scm_mul(c, scm_from_words(w))));
    for (int i = 0; i < 8; ++i) a[i] = w[i];
  }
}

#if defined(__HIPCC__)
}  // namespace zkvm
// One lane per row, 64 per block, grid = rows / 64 rounded up.  A row's transcript is two or three permutations, so there
// is nothing to share between lanes; the state lies in LDS as k_tx_hash lays it out (word i of lane l at st[i * 64 + l]).
__global__ void __launch_bounds__(64)
k_tx_sig_rows(zkvm::SigRowsView v) {
  __shared__ uint32_t st[50 * 64];
  const uint32_t row = blockIdx.x * 64 + threadIdx.x;
  if (row >= v.rows) return;
  zkvm::tx_sig_row(v, row, st + threadIdx.x, 64);
}
namespace zkvm {
#endif

}  // namespace zkvm
}  // namespace zk

// ===================================================== host side =====================================================
#include "zkvm_tx.hpp"       // Transcript, TxStatement, proto_transcript, tx_finish_signature

#include <cstring>
#include <string>
#include <vector>

namespace zk {
namespace zkvm {

// the transcript tx_finish_signature is run over to write the script: it hashes nothing and notes what it is given
struct SigRecorder {
  struct Seen { std::string label; const uint8_t* p; size_t n; };
  std::vector<Seen>* seen = nullptr;
  std::string* challenge = nullptr;
  SigRecorder() {}
  explicit SigRecorder(const Transcript&) {}
  void append_message(const char* label, const uint8_t* msg, size_t n) { seen->push_back(Seen{label, msg, n}); }
  void append_point(const char* label, const uint8_t p[32]) { append_message(label, p, 32); }
  Scalar challenge_scalar(const char* label) { *challenge = label; return Scalar::from_u64(0); }
};

// -> false: tx_finish_signature has become something the script cannot hold (the caller fails the call)
inline bool sig_script(SigScript& sc) {
  std::memset(&sc, 0, sizeof sc);
  proto_transcript(P_SIGNTX).export_state(sc.init);
  TxStatement st;
  st.sig_scalars.resize(96); st.sig_points.resize(96);
  uint8_t base[32] = {0}, agg[32] = {0};
  std::vector<SigRecorder::Seen> seen;
  std::string chal;
  SigRecorder rec;
  rec.seen = &seen; rec.challenge = &chal;
  tx_finish_signature(st, base, agg, &rec);
  uint8_t* pool = (uint8_t*)sc.pool;
  size_t used = 0;
  auto put = [&](const void* p, size_t n, uint32_t& at) {
    if (used + n > 4 * SIG_POOL_WORDS) return false;
    at = (uint32_t)used;
    std::memcpy(pool + used, p, n);
    used += n;
    return true;
  };
  auto label = [&](const std::string& t, uint32_t& out) {
    uint32_t at = 0;
    if (t.size() >= 0x10000 || !put(t.data(), t.size(), at)) return false;
    out = at | ((uint32_t)t.size() << 16);
    return true;
  };
  if (seen.size() > SIG_MAX_MSG || chal.empty()) return false;
  bool have[4] = {false, false, false, false};
  for (size_t m = 0; m < seen.size(); ++m) {
    const SigRecorder::Seen& s = seen[m];
    const uint32_t kind = s.p == st.txid ? SIG_TXID : s.p == agg ? SIG_KEY : s.p == &st.sig_points[32] ? SIG_R : SIG_CONST;
    if (!label(s.label, sc.msg[m][0])) return false;
    if (kind != SIG_CONST && s.n != 32) return false;
    if (kind == SIG_CONST && !put(s.p, s.n, sc.msg[m][3])) return false;
    sc.msg[m][1] = kind; sc.msg[m][2] = (uint32_t)s.n;
    have[kind] = true;
  }
  if (!have[SIG_TXID] || !have[SIG_KEY] || !have[SIG_R]) return false;     // a challenge that ignored one of them signs nothing
  if (!label(chal, sc.chal_label)) return false;
  sc.n_msg = (uint32_t)seen.size(); sc.chal_len = 64;
  return true;
}

// every row of a stage on the CPU, as the kernel runs them
inline void sig_rows_run_host(const SigRowsView& v) {
  uint32_t st[50];
  for (uint32_t row = 0; row < v.rows; ++row) tx_sig_row(v, row, st, 1);
}

}  // namespace zkvm
}  // namespace zk
