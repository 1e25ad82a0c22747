// tx_log.hpp -- the Input / Output entries of a transaction's log, read off its hash plan (zkgpu.h: ZKGPU_TXFORMAT_RETURN_LOG).
//
// A node that has verified a block applies it: every consumed contract leaves its UTXO set, every created one enters it.  It
// needs the contract IDs of the transaction log's Input(id) / Output(id) entries, in the order the program logged them.
// Nothing is hashed for them: plan_merkle (zkvm_tx.hpp) writes one leaf job per log entry whose message is ONE piece, labelled
// L_input or L_output, of kind Slot, naming the slot that holds the entry's contract ID.  Walking a plan's pieces for those two
// labels therefore yields (kind, slot) in log order; the header's leaf has other labels and is not listed.
//
//   the host's second pass (no ZKGPU_TXFORMAT_HASH_ON_DEVICE): tx_prepare_many_logged runs the plans as tx_prepare_many does
//     and copies the entries' slots into the record of the transaction, in a side array of the call (tx_call.hpp);
//   the device (ZKGPU_TXFORMAT_HASH_ON_DEVICE): the tape's block keeps every plan SHAPE's pieces (tx_hash_tape.hpp), so the
//     entries of a shape are a small table -- tx_log_table -- uploaded beside the tape (it is not part of the block);
//     k_tx_log_gather (tx_hash_kernels.hpp) copies the slots the table names from the slot memory k_tx_hash filled into a dense
//     array, K x 32 bytes per transaction, and that array alone is copied down.  Counts and kinds come from the host's table.
//
// A record (what the caller is handed per transaction):  count:u8 | kind[K]:u8 | id[K][32]  -- K the window the format asked
// for.  count > K: the real count (saturated at 255) and nothing else; bytes past `count` are zero.  A record that lists its
// entries has no kind byte of 0 among them, so count >= 1 with kind[0] == 0 always reads "did not fit" -- which is how 255
// under K = 255 tells "255 entries, listed" from "255 or more, not listed" (tx_log_listed).
#pragma once
#include "tx_hash_tape.hpp"
#include "tx_out.hpp"     // tx_log_record_bytes: the size of a record is part of the layout

namespace zk {
namespace zkvm {

constexpr uint32_t TXLOG_INPUT = 1, TXLOG_OUTPUT = 2;     // (ZKGPU_TXLOG_INPUT / _OUTPUT: tx_device.hpp asserts them)

// ---- the table of a tape: words.  [0, n_shapes): where shape s's entries start; there: count, then count x (kind, slot)
#if defined(__HIPCC__)
typedef uint4 TxLogQuad;                                  // (the vector type: one 16-byte load or store, and a local copy stays in registers)
#else
struct alignas(16) TxLogQuad { uint32_t x, y, z, w; };
#endif

// lane idx = transaction * K + window position j of a chunk's tape: the 32 bytes of entry j of that transaction's log to
// out[idx] if its shape has more than j and at most K entries, zeros otherwise.  Two 16-byte loads and stores: slots and out
// are 16-byte aligned (32 bytes per slot / entry from an aligned base).  One function for the kernel and the CPU stand-in.
// (idx is 32 bits: a chunk holds fewer than 2^24 transactions and K is at most 255 -- tx_log_lanes_fit, asked before a launch)
ZK_TAPE_HD inline void tx_log_gather_lane(const uint32_t* tape, const uint32_t* table, const uint32_t* slots, uint32_t* out, uint32_t idx, uint32_t K) {
  const HashTapeHead& h = *(const HashTapeHead*)tape;
  const uint32_t tx = idx / K, j = idx - tx * K;
  const uint32_t* rec = tape + h.txs + 4 * (size_t)tx;
  const uint32_t* tab = table + table[rec[0]];
  TxLogQuad* to = (TxLogQuad*)(out + 8 * (size_t)idx);
  TxLogQuad lo{0, 0, 0, 0}, hi{0, 0, 0, 0};
  if (j < tab[0] && tab[0] <= K) {
    const TxLogQuad* from = (const TxLogQuad*)(slots + 8 * ((size_t)rec[2] + tab[2 + 2 * j]));
    lo = from[0]; hi = from[1];
  }
  to[0] = lo; to[1] = hi;
}
inline bool tx_log_lanes_fit(uint64_t n_tx, uint64_t K) { return n_tx * K < ((uint64_t)1 << 32); }

// The table of a finished block: per shape, its leaf pieces in job order.  -> false: an entry names a slot outside its shape's
// slot area (cannot happen with a block that passes hash_tape_check; the kernel indexes by it blindly, so it is asked anyway).
inline bool tx_log_table(const uint32_t* block, std::vector<uint32_t>& table) {
  const HashTapeHead& h = *(const HashTapeHead*)block;
  table.assign(h.n_shapes, 0);
  for (uint32_t s = 0; s < h.n_shapes; ++s) {
    const uint32_t* sh = block + h.shapes + 4 * s;
    table[s] = (uint32_t)table.size();
    const size_t at = table.size();
    table.push_back(0);
    for (uint32_t ji = sh[0]; ji < sh[0] + sh[1]; ++ji) {
      const uint32_t* job = block + h.jobs + 4 * ji;
      if ((job[0] & 0xffu) != P_TXID) continue;
      for (uint32_t q = job[2]; q < job[2] + job[3]; ++q) {
        const uint32_t* pc = block + h.pieces + 4 * q;
        const uint32_t label = pc[0] & 0xffu;
        if ((label != L_input && label != L_output) || (pc[0] >> 8) != TAPE_SLOT) continue;
        if (pc[3] >= sh[2]) return false;
        table.push_back(label == L_input ? TXLOG_INPUT : TXLOG_OUTPUT);
        table.push_back(pc[3]);
        ++table[at];
      }
    }
  }
  return true;
}
inline const uint32_t* tx_log_shape(const std::vector<uint32_t>& table, uint32_t shape) { return table.data() + table[shape]; }
// entries the gather hands back for the transactions of a block: those of shapes with at most K entries
inline uint64_t tx_log_handed_back(const uint32_t* block, const std::vector<uint32_t>& table, size_t K) {
  const HashTapeHead& h = *(const HashTapeHead*)block;
  uint64_t n = 0;
  for (uint32_t t = 0; t < h.n_tx; ++t) { const uint32_t c = tx_log_shape(table, (block + h.txs + 4 * t)[0])[0]; if (c <= K) n += c; }
  return n;
}

// One record from `count` entries (kind, where the 32 bytes lie): rec is 1 + 33 K bytes, ZERO on entry
template <class Entry> inline void tx_log_record(uint8_t* rec, size_t K, size_t count, Entry entry) {
  rec[0] = (uint8_t)std::min<size_t>(count, 255);
  if (count > K) return;
  for (size_t j = 0; j < count; ++j) {
    const std::pair<uint32_t, const uint8_t*> e = entry(j);
    rec[1 + j] = (uint8_t)e.first;
    std::memcpy(rec + 1 + K + 32 * j, e.second, 32);
  }
}
// does a record of window K list its entries (or has it none), rather than give their number alone?
inline bool tx_log_listed(const uint8_t* rec, size_t K) { return rec[0] <= K && (rec[0] == 0 || rec[1] != 0); }
// a record of window K_in (as the call keeps it) into a caller's record of window K_out (zero on entry)
inline void tx_log_record_copy(uint8_t* out, size_t K_out, const uint8_t* in, size_t K_in) {
  const size_t count = in[0];
  out[0] = in[0];
  if (count > K_out || !tx_log_listed(in, K_in)) return;
  std::memcpy(out + 1, in + 1, count);
  std::memcpy(out + 1 + K_out, in + 1 + K_in, 32 * count);
}

// the entries of a plan that has run, from its slot memory, into the transaction's record (zero on entry)
inline void tx_log_of_plan(const TxPlan& P, const uint8_t* slots, uint8_t* rec, size_t K) {
  static thread_local std::vector<std::pair<uint32_t, const uint8_t*>> found;
  found.clear();
  for (const HashJob& j : P.jobs) {
    if (j.proto != P_TXID) continue;
    for (uint32_t q = j.first; q < j.first + j.count; ++q) {
      const HashPiece& h = P.pieces[q];
      if ((h.label != L_input && h.label != L_output) || h.kind != HashPiece::Slot || h.slot >= P.n_slots) continue;
      found.push_back({h.label == L_input ? TXLOG_INPUT : TXLOG_OUTPUT, slots + 32 * (size_t)h.slot});
    }
  }
  tx_log_record(rec, K, found.size(), [&](size_t j) { return found[j]; });
}

// tx_prepare_many (zkvm_tx.hpp) with every protocol -- the host's second pass -- that also leaves every accepted transaction's
// record at recs + i * (1 + 33 K), read off the zeroed slot memory its plan wrote.  Same statements, same hashing.
inline void tx_prepare_many_logged(const uint8_t* const* tx, const size_t* len, TxStatement* st, size_t count, uint8_t* recs, size_t K) {
  tx_run_group(tx, len, st, count, ALL_PROTOS, ALL_PROTOS, true, true, [&](size_t i, const TxPlan& plan, const TxSlots&, const uint8_t* slots) {
    tx_log_of_plan(plan, slots, recs + i * tx_log_record_bytes(K), K);
  });
}

// The one pass of a precompute-only call (ZKGPU_TXFORMAT_PRECOMPUTE_ONLY) whose host hashes: the same structure pass, the plans
// run for what the transaction ID and the log need and nothing else (ID_PROTOS: no MuSig coefficient is hashed, the statement's
// signature scalars are not what a verifying call would find there), the records as above when recs is not NULL.
static_assert(P_CONTRACTID < P_MUSIG && P_RATCHET < P_MUSIG && P_TXID < P_MUSIG && P_SIGNTX > P_MUSIG,
              "ID_PROTOS (zkvm_tx.hpp: run_plan) takes every protocol below P_MUSIG: the three the ID and the log are hashed from, and no other");
inline void tx_precompute_many(const uint8_t* const* tx, const size_t* len, TxStatement* st, size_t count, uint8_t* recs, size_t K) {
  tx_run_group(tx, len, st, count, ALL_PROTOS, ID_PROTOS, true, true, [&](size_t i, const TxPlan& plan, const TxSlots&, const uint8_t* slots) {
    if (recs) tx_log_of_plan(plan, slots, recs + i * tx_log_record_bytes(K), K);
  });
}

}  // namespace zkvm
}  // namespace zk
