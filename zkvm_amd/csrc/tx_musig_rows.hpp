// tx_musig_rows.hpp -- the MuSig coefficients a_i of a signature's keys formed where the keys already lie (zkgpu.h:
// ZKGPU_TXFORMAT_STATEMENTS_V1 | ZKGPU_TXFORMAT_SIGN_ON_DEVICE): per row the transcripts of zkvm_tx.hpp's key aggregation,
// a_i = H("Musig.aggregated-key": n, X_0 .. X_{n-1}, then i) reduced mod l, written as canonical bytes into the row's scalar
// terms -- musig_row, one function for the host and the device (k_musig_rows runs it one lane per row; the CPU tests and
// libzkhost run the same code), on the TapeStrobe operations of tx_hash_tape.hpp as tx_sig_row is.
//
// WHAT is hashed is not written down here.  tx_musig_jobs() below is the recipe the host's plans are written with (the one
// zkvm_tx.hpp's VM writes for a payment; the CPU tests compare the two job for job); musig_script() runs it over a recorder
// and keeps what it saw: the messages in order, each with its label, its length and what its bytes are -- the number of
// keys, the keys themselves, the index of the key the coefficient belongs to -- and the label and length of the challenge.
// The kernel interprets that script; no label is restated, and a change of the recipe changes both sides.
//
// A row is a row of a stage's dynamic terms (tx_call.hpp): `skip` leading terms that are not keys (0 in a key stage's rows,
// 1 in a signature stage's, whose term 0 is R), then one term (a_i, X_i) per key.  Everything the transcripts of one row share
// -- n and the keys -- is absorbed ONCE; the state behind it is kept in a second plane of 50 words, and per key it is
// restored, i is absorbed and 64 bytes are squeezed.  So a row of k keys costs the permutations of ONE pass over its keys
// plus one or two per key, where the host's plan re-absorbs the prefix for every key (k passes).
#pragma once
#include <stdint.h>

#include "tx_hash_tape.hpp"   // TapeStrobe and its operations; ZK_TAPE_HD
#include "sc_dev.hpp"

namespace zk {
namespace zkvm {

constexpr uint32_t MUSIG_COUNT = 0, MUSIG_KEYS = 1, MUSIG_INDEX = 2;          // what a message's bytes are
constexpr uint32_t MUSIG_MAX_MSG = 4, MUSIG_POOL_WORDS = 16;
struct MusigScript {
  uint32_t init[TAPE_PROTO_WORDS];      // the initial transcript of P_MUSIG (50 state words, position, begin marker)
  uint32_t n_msg, chal_label, chal_len, zero;
  uint32_t msg[MUSIG_MAX_MSG][4];       // label, kind, length of one message, 0.  MUSIG_KEYS stands for one message PER KEY;
                                        // MUSIG_INDEX is the last: what lies before it is the prefix the keys of a row share
  uint32_t pool[MUSIG_POOL_WORDS];      // label texts.  A label is (byte offset | length << 16)
};
static_assert(sizeof(MusigScript) % 16 == 0, "whole uint4s");

// where the rate boundary of the sponge fell while a row's messages were absorbed (trace, three counters; NULL: not asked,
// as on the device): strictly inside the two bytes that open an operation, inside a label and its length, inside a key
constexpr uint32_t MUSIG_IN_HEADER = 0, MUSIG_IN_LABEL = 1, MUSIG_IN_KEY = 2;
struct MusigRowsView {
  const MusigScript* script;
  const uint64_t* offsets;              // rows + 1: the rows' extents in points / scalars
  const uint32_t* points;               // 8 words per term
  uint32_t* scalars;                    // 8 words per term; the key terms' are written
  uint32_t rows, skip;                  // skip: leading terms of every row that are not keys
  uint32_t* trace;
};

ZK_TAPE_HD inline void musig_seen(uint32_t* trace, uint32_t which, uint32_t pos_before, uint32_t n) {
  if (trace && pos_before + n > TAPE_RATE) ++trace[which];
}
// what opens a message or a challenge of `len` bytes: meta-AD of a label of the pool and of the length, then (data: a message)
// the operation that takes the bytes
ZK_TAPE_HD inline void musig_open(TapeStrobe& s, const uint32_t* pool, uint32_t label, uint32_t len, bool data, uint32_t* trace) {
  musig_seen(trace, MUSIG_IN_HEADER, s.pos, 2);
  tape_begin_op(s, 16u | 2u);
  musig_seen(trace, MUSIG_IN_LABEL, s.pos, (label >> 16) + 4);
  tape_absorb(s, pool, label & 0xffffu, label >> 16);
  for (int i = 0; i < 4; ++i) tape_absorb_byte(s, (len >> (8 * i)) & 0xffu);
  if (!data) return;
  musig_seen(trace, MUSIG_IN_HEADER, s.pos, 2);
  tape_begin_op(s, 2u);
}
ZK_TAPE_HD inline void musig_u64(TapeStrobe& s, uint32_t x) {                 // (a count or an index: below 2^32)
  for (int i = 0; i < 4; ++i) tape_absorb_byte(s, (x >> (8 * i)) & 0xffu);
  for (int i = 0; i < 4; ++i) tape_absorb_byte(s, 0);
}

// st: 100 words of scratch, word i at st[i * stride] -- the state in words 0 .. 49, the saved prefix in words 50 .. 99
ZK_TAPE_HD inline void musig_row(const MusigRowsView& v, uint32_t row, uint32_t* st, uint32_t stride) {
  const MusigScript& sc = *v.script;
  const uint64_t t0 = v.offsets[row] + v.skip, t1 = v.offsets[row + 1];
  if (t1 <= t0 || sc.n_msg == 0) return;                 // (no such row is made: a signature has a key)
  const uint32_t k = (uint32_t)(t1 - t0);
  for (uint32_t i = 0; i < 50; ++i) st[i * stride] = sc.init[i];
  TapeStrobe s{st, stride, sc.init[50], sc.init[51]};
  for (uint32_t m = 0; m + 1 < sc.n_msg; ++m) {          // the prefix: everything before the index
    const uint32_t label = sc.msg[m][0], len = sc.msg[m][2];
    if (sc.msg[m][1] == MUSIG_COUNT) { musig_open(s, sc.pool, label, len, true, v.trace); musig_u64(s, k); continue; }
    for (uint32_t j = 0; j < k; ++j) {
      musig_open(s, sc.pool, label, len, true, v.trace);
      musig_seen(v.trace, MUSIG_IN_KEY, s.pos, len);
      tape_absorb(s, v.points + 8 * (t0 + j), 0, len);
    }
  }
  for (uint32_t i = 0; i < 50; ++i) st[(50 + i) * stride] = st[i * stride];
  const uint32_t pos = s.pos, pos_begin = s.pos_begin;
  const uint32_t last = sc.n_msg - 1;
  for (uint32_t i = 0; i < k; ++i) {
    if (i) {
      for (uint32_t q = 0; q < 50; ++q) st[q * stride] = st[(50 + q) * stride];
      s.pos = pos; s.pos_begin = pos_begin;
    }
    musig_open(s, sc.pool, sc.msg[last][0], sc.msg[last][2], true, v.trace);
    musig_u64(s, i);
    musig_open(s, sc.pool, sc.chal_label, sc.chal_len, false, v.trace);
    tape_begin_op(s, 1u | 2u | 4u);                      // PRF: the position is 0 afterwards, the 64 bytes the first 16 words
    uint32_t wide[16];
    for (uint32_t q = 0; q < 16; ++q) wide[q] = st[q * stride];
    uint32_t w[8];
    scm_to_words(w, scm_from_wide(wide));
    uint32_t* a = v.scalars + 8 * (t0 + i);
    for (int q = 0; q < 8; ++q) a[q] = w[q];
  }
}

#if defined(__HIPCC__)
}  // namespace zkvm
// One lane per row, 64 per block, grid = rows / 64 rounded up; the state and the saved prefix lie in LDS as k_tx_hash lays
// its state out (word i of lane l at st[i * 64 + l]): 100 words per lane, 25.6 KB per block.
__global__ void __launch_bounds__(64)
k_musig_rows(zkvm::MusigRowsView v) {
  __shared__ uint32_t st[100 * 64];
  const uint32_t row = blockIdx.x * 64 + threadIdx.x;
  if (row >= v.rows) return;
  zkvm::musig_row(v, row, st + threadIdx.x, 64);
}
namespace zkvm {
#endif

}  // namespace zkvm
}  // namespace zk

// ===================================================== host side =====================================================
#include "zkvm_tx.hpp"       // TxPlan, Proto, Label, label_text, proto_transcript

#include <cstring>
#include <string>
#include <vector>

namespace zk {
namespace zkvm {

// The recipe: the jobs of the coefficients of `k` keys, written to anything that takes a plan's calls -- a TxPlan (the host
// hashes them: tx_statements.hpp) or the recorder below (the device's script).  a: the slots of a_0 .. a_{k-1}.
template <class Plan, class Slots>
inline void tx_musig_jobs(Plan& P, const uint8_t* const* keys, size_t k, Slots& a) {
  for (size_t i = 0; i < k; ++i) {
    P.begin(P_MUSIG);
    P.u64(L_n, k);
    for (size_t j = 0; j < k; ++j) P.bytes(L_X, keys[j], 32, 32);
    P.u64(L_i, i);
    a.push_back(P.end(L_a_i, 64));
  }
}

// a plan that hashes nothing and notes what it is asked for
struct MusigRecorder {
  struct Piece { uint8_t label; bool imm; uint64_t value; const uint8_t* p; uint32_t len; };
  struct Job { uint8_t proto, chal_label, out_len; std::vector<Piece> pieces; };
  std::vector<Job> jobs;
  void begin(uint8_t proto) { jobs.push_back(Job{proto, 0, 0, {}}); }
  void u64(uint8_t label, uint64_t x) { jobs.back().pieces.push_back(Piece{label, true, x, nullptr, 8}); }
  void bytes(uint8_t label, const uint8_t* p, uint32_t len, uint32_t) { jobs.back().pieces.push_back(Piece{label, false, 0, p, len}); }
  uint32_t end(uint8_t chal_label, uint8_t out_len) { jobs.back().chal_label = chal_label; jobs.back().out_len = out_len; return (uint32_t)jobs.size() - 1; }
};

// -> false: the recipe has become something the script cannot hold (the caller fails the call)
inline bool musig_script(MusigScript& sc) {
  std::memset(&sc, 0, sizeof sc);
  proto_transcript(P_MUSIG).export_state(sc.init);
  constexpr size_t K = 3;
  uint8_t key[K][32] = {{0}};
  const uint8_t* keys[K] = {key[0], key[1], key[2]};
  MusigRecorder rec;
  std::vector<uint32_t> slots;
  tx_musig_jobs(rec, keys, K, slots);
  if (rec.jobs.size() != K) return false;
  uint8_t* pool = (uint8_t*)sc.pool;
  size_t used = 0;
  auto label = [&](uint8_t l, uint32_t& out) {
    if (l >= N_LABEL) return false;
    const char* t = label_text(l);
    const size_t n = std::strlen(t);
    if (used + n > 4 * MUSIG_POOL_WORDS) return false;
    std::memcpy(pool + used, t, n);
    out = (uint32_t)used | ((uint32_t)n << 16);
    used += n;
    return true;
  };
  const MusigRecorder::Job& j0 = rec.jobs[0];
  // every job is one transcript of P_MUSIG with a 64-byte challenge under one label, the same pieces but for the index
  for (size_t i = 0; i < K; ++i) {
    const MusigRecorder::Job& j = rec.jobs[i];
    if (j.proto != P_MUSIG || j.out_len != 64 || j.chal_label != j0.chal_label || j.pieces.size() != j0.pieces.size()) return false;
    for (size_t q = 0; q < j.pieces.size(); ++q)
      if (j.pieces[q].label != j0.pieces[q].label || j.pieces[q].imm != j0.pieces[q].imm || j.pieces[q].len != j0.pieces[q].len || j.pieces[q].p != j0.pieces[q].p) return false;
  }
  uint32_t n = 0;
  bool have[3] = {false, false, false};
  for (size_t q = 0; q < j0.pieces.size();) {
    const MusigRecorder::Piece& p = j0.pieces[q];
    if (n == MUSIG_MAX_MSG || have[MUSIG_INDEX]) return false;             // (nothing may follow the index: the prefix is saved before it)
    uint32_t kind;
    if (p.imm) {
      bool count = true, index = true;
      for (size_t i = 0; i < K; ++i) { count = count && rec.jobs[i].pieces[q].value == K; index = index && rec.jobs[i].pieces[q].value == i; }
      if (count == index) return false;
      kind = count ? MUSIG_COUNT : MUSIG_INDEX;
      ++q;
    } else {                                                               // the keys, in order, one message each
      for (size_t i = 0; i < K; ++i, ++q)
        if (q >= j0.pieces.size() || j0.pieces[q].imm || j0.pieces[q].p != keys[i] || j0.pieces[q].len != 32 || j0.pieces[q].label != p.label) return false;
      kind = MUSIG_KEYS;
    }
    if (have[kind] || !label(p.label, sc.msg[n][0])) return false;
    have[kind] = true;
    sc.msg[n][1] = kind; sc.msg[n][2] = p.len;
    ++n;
  }
  if (!have[MUSIG_COUNT] || !have[MUSIG_KEYS] || !have[MUSIG_INDEX]) return false;
  if (!label(j0.chal_label, sc.chal_label)) return false;
  sc.n_msg = n; sc.chal_len = 64;
  return true;
}

// every row of a stage on the CPU, as the kernel runs them
inline void musig_rows_run_host(const MusigRowsView& v) {
  uint32_t st[100];
  for (uint32_t row = 0; row < v.rows; ++row) musig_row(v, row, st, 1);
}

}  // namespace zkvm
}  // namespace zk
