// tx_statements.hpp -- the records of ZKGPU_TXFORMAT_STATEMENTS_V1: what a caller's OWN VM leaves behind per transaction
// (upstream: `Tx::precompute()` -> `PrecomputedTx`), parsed into the TxStatement the passes of zkvm_tx.hpp's VM would have
// left, so that everything behind the VM -- key aggregation, the Schnorr equation, the cloak proof: `PrecomputedTx::verify`
// -- runs as it does for a serialized transaction (tx_call.hpp: step_statements).
//
// THE FRAMING IS THIS LIBRARY'S OWN, not a recollection of anything upstream; little endian:
//
//   txid:32 | R:32 s:32 | k:u32 keys[k]:32 each | n_in:u32 n_out:u32 | commitments: 64*(n_in+n_out) | p:u32 R1CSProof[p]
//
// keys: in the order the program's signtx instructions met them; commitments: (quantity, flavor) per value, inputs first.
// THE LIBRARY CANNOT KNOW WHETHER txid BELONGS TO ANYTHING: it is the message the signature is checked over, no more.
//
// What the parser decides (the order the checks are made in):
//   fewer than 96 bytes                                     INVALID   "record malformed"                  (status 16)
//   s not canonical                                         INVALID   "signature scalar not canonical"    (status 21: the text
//                                                                     is zkvm_tx.hpp's, by which TxCall tells the two apart)
//   fields overrun the record or do not fill it; k = 0      INVALID   "record malformed"                  (status 16)
//   k > 64; n_in or n_out 0 or above 64                     UNSUPPORTED: the caller's own verifier must  (status 2)
// The MuSig coefficients are written as jobs of a TxPlan with the recipe of tx_musig_rows.hpp and run by run_plans_x8 /
// run_plan -- or left to the device (host_musig = false: the terms read zero).
#pragma once
#include "tx_musig_rows.hpp"
#include "zkvm_tx.hpp"

namespace zk {
namespace zkvm {

constexpr uint32_t STATEMENT_MAX_KEYS = 64, STATEMENT_MAX_VALUES = 64;

// -> the keys' offset in the record (0: the statement is not TX_OK)
inline size_t tx_statement_parse(const uint8_t* rec, size_t len, TxStatement& st) {
  st.status = TX_INVALID; st.why = "record malformed";
  st.version = st.mintime = st.maxtime = 0;
  std::memset(st.txid, 0, 32);
  st.n_in = st.n_out = 0;
  st.commitments.resize(0);
  st.proof = nullptr; st.proof_len = 0;
  st.sig_scalars.resize(0); st.sig_points.resize(0);
  if (len < 96) return 0;
  Scalar s;
  if (!Scalar::from_canonical(rec + 64, s)) { st.why = "signature scalar not canonical"; return 0; }
  size_t at = 96;
  if (len - at < 4) return 0;
  const uint32_t k = rd32(rec + at);
  at += 4;
  if (k == 0 || (len - at) / 32 < k) return 0;
  const size_t keys_at = at;
  at += 32 * (size_t)k;
  if (len - at < 8) return 0;
  const uint32_t n_in = rd32(rec + at), n_out = rd32(rec + at + 4);
  at += 8;
  const uint64_t values = (uint64_t)n_in + n_out;
  if ((len - at) / 64 < values) return 0;
  const size_t com_at = at;
  at += 64 * (size_t)values;
  if (len - at < 4) return 0;
  const uint32_t p = rd32(rec + at);
  at += 4;
  if (len - at != p) return 0;
  if (k > STATEMENT_MAX_KEYS || n_in == 0 || n_out == 0 || n_in > STATEMENT_MAX_VALUES || n_out > STATEMENT_MAX_VALUES) {
    st.status = TX_UNSUPPORTED; st.why = "more keys or values than the library serves";
    return 0;
  }
  std::memcpy(st.txid, rec, 32);
  st.n_in = n_in; st.n_out = n_out;
  st.commitments.assign(rec + com_at, 64 * (size_t)values);
  st.proof = rec + at; st.proof_len = p;
  // terms: [0] B (scalar s), [1] R (scalar -1), [2 + i] X_i (scalar a_i) -- as tx_structure leaves them
  st.sig_scalars.resize(32 * (2 + (size_t)k));
  st.sig_points.resize(32 * (2 + (size_t)k));
  s.to_bytes(&st.sig_scalars[0]);
  (-Scalar::one()).to_bytes(&st.sig_scalars[32]);
  std::memcpy(&st.sig_points[32], rec + 32, 32);
  std::memcpy(&st.sig_points[64], rec + keys_at, 32 * (size_t)k);
  st.status = TX_OK; st.why = "";
  return keys_at;
}

// Up to eight records: parsed, and (host_musig) the coefficients hashed on the host -- in lockstep when the records have the
// same number of keys, as payments of a block mostly do -- and moved into the statements' scalar terms.
inline void tx_statements_many(const uint8_t* const* rec, const size_t* len, TxStatement* st, size_t count, bool host_musig, bool allow_x8 = true) {
  TxGroupScratch& w = tx_group_scratch();
  int live[8], n_live = 0;
  for (size_t i = 0; i < count && i < 8; ++i) {
    const size_t keys_at = tx_statement_parse(rec[i], len[i], st[i]);
    if (st[i].status != TX_OK || !host_musig) continue;
    TxPlan& P = w.plans[i];
    P.only = 0xff;
    P.clear();
    w.outs[i].a.clear();
    const size_t k = st[i].sig_points.size() / 32 - 2;
    const uint8_t* keys[STATEMENT_MAX_KEYS];
    for (size_t j = 0; j < k; ++j) keys[j] = rec[i] + keys_at + 32 * j;
    tx_musig_jobs(P, keys, k, w.outs[i].a);
    w.slot_mem[i].resize(32 * (size_t)P.n_slots + 32);
    live[n_live++] = (int)i;
  }
  bool lockstep = false;
#if ZK_HAVE_X8
  lockstep = allow_x8 && n_live >= 3 && x8_available();
  for (int q = 1; lockstep && q < n_live; ++q) lockstep = w.plans[live[q]].same_shape(w.plans[live[0]]);
  if (lockstep) {
    const TxPlan* P[8];
    uint8_t* S[8];
    for (int l = 0; l < 8; ++l) {
      if (l < n_live) { P[l] = &w.plans[live[l]]; S[l] = w.slot_mem[live[l]].data(); }
      else { P[l] = &w.plans[live[0]]; w.spare[l].resize(w.slot_mem[live[0]].size()); S[l] = w.spare[l].data(); }     // padding: lane 0's work again
    }
    run_plans_x8(P, S, P_MUSIG);
  }
#endif
  for (int q = 0; q < n_live; ++q) {
    const int i = live[q];
    if (!lockstep) run_plan(w.plans[i], w.slot_mem[i].data(), P_MUSIG);
    for (size_t j = 0; j < w.outs[i].a.size(); ++j) std::memcpy(&st[i].sig_scalars[32 * (2 + j)], w.slot_mem[i].data() + 32 * (size_t)w.outs[i].a[j], 32);
  }
}

}  // namespace zkvm
}  // namespace zk
