// tx_out.hpp -- what a transaction call hands its caller, laid out ONCE: the format word of zkgpu_verifier_set_tx_format decoded
// and validated (TxFormat) -- with it the MODE of a call, as predicates every layer asks --, the layout of a call's status
// argument as a value (TxOutLayout), which calls in flight share a round and under what format (tx_round_mates,
// tx_round_format), and the hand-out of a merged round to its calls (tx_round_hand_out).  Host-only, no HIP and no zkgpu.h (its constants are restated; session.hpp asserts them), so
// that libzkgpu and libzkhost -- the CPU self-tests of hostlib.cpp -- compile the SAME code, like pipe_plan.hpp or msm_route.hpp.
//
// The status argument of a call over `batch` transactions:   status[batch] | id[batch][32] | record[batch][1 + 33 K] | root[32]
//   status: one byte per transaction (0 beside a set accept bit and nowhere else);
//   id (ZKGPU_TXFORMAT_RETURN_IDS): the transaction ID of every ACCEPTED transaction, zeros elsewhere;
//   record (ZKGPU_TXFORMAT_RETURN_LOG with window K, only beside the IDs): count | kind[K] | id[K][32] (tx_log.hpp), likewise.
//   root (ZKGPU_TXFORMAT_RETURN_ROOT, only beside the IDs): the Merkle root over the call's IDs in call order (tx_root.hpp), behind
//     everything else so that nothing moves; written last, and only if EVERY transaction of the call reads 0 (3 under
//     precompute-only) -- zeros otherwise.  Of a call over no transaction it is the empty tree's hash.
// Three moments write the whole of it -- begin, nothing_in_subset, fail_closed; in between TxCall::verdicts writes beside the
// bits it sets, through a TxPiece.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace zk {
namespace zkvm {

// (ZKGPU_TXFORMAT_*, ZKGPU_TXSTATUS_REJECTED / _OUTSIDE_SUBSET / _PRECOMPUTED)
constexpr int TXFORMAT_V1 = 1, TXFORMAT_V1_REASONS = 2, TXFORMAT_STATEMENTS_V1 = 4, TXFORMAT_HASH_ON_DEVICE = 256, TXFORMAT_SIGN_ON_DEVICE = 512, TXFORMAT_RETURN_IDS = 1024,
              TXFORMAT_RETURN_ROOT = 16, TXFORMAT_RETURN_LOG = 2048, TXFORMAT_PRECOMPUTE_ONLY = 8192, TXFORMAT_LOG_SHIFT = 16;
constexpr uint8_t TXOUT_REJECTED = 1, TXOUT_OUTSIDE_SUBSET = 2, TXOUT_PRECOMPUTED = 3;
inline size_t tx_log_record_bytes(size_t K) { return 1 + 33 * K; }

// One caller's transactions inside a call (TxCall::Piece).  ids (may be NULL): 32 * batch bytes of that caller's, zeroed by it,
// for the IDs of what is accepted; log / log_k (may be NULL): batch records of 1 + 33 * log_k bytes, zeroed likewise; root (may
// be NULL): 32 bytes, zeroed likewise, for the root over that caller's IDs if every one of its transactions is handed its ID
struct TxPiece { const uint8_t* txs; const uint64_t* tx_offsets; size_t batch; uint8_t* ids = nullptr; uint8_t* log = nullptr; size_t log_k = 0; uint8_t* root = nullptr; };

struct TxOutLayout {
  bool ids = false;                                       // the ID area is there
  size_t log_k = 0;                                       // the window K of the records (0: no record area; only beside ids)
  bool root = false;                                      // the call's root is there, 32 bytes behind everything else (only beside ids)

  size_t bytes(size_t batch) const { return batch * (1 + (ids ? 32 : 0) + (log_k ? tx_log_record_bytes(log_k) : 0)) + (root ? 32 : 0); }
  // where transaction i's status byte, ID and record lie in a caller's area of bytes(batch) (NULL: that part is not there)
  uint8_t* status_of(uint8_t* area, size_t i) const { return area ? area + i : nullptr; }
  uint8_t* id_of(uint8_t* area, size_t batch, size_t i) const { return area && ids ? area + batch + 32 * i : nullptr; }
  uint8_t* record_of(uint8_t* area, size_t batch, size_t i) const { return area && log_k ? area + 33 * batch + i * tx_log_record_bytes(log_k) : nullptr; }
  uint8_t* root_of(uint8_t* area, size_t batch) const { return area && root ? area + bytes(batch) - 32 : nullptr; }
  TxPiece piece(const uint8_t* txs, const uint64_t* tx_offsets, size_t batch, uint8_t* area) const {
    return TxPiece{txs, tx_offsets, batch, id_of(area, batch, 0), record_of(area, batch, 0), log_k, root_of(area, batch)};
  }

  // a call begins: no bit set, every transaction "rejected", no ID, no record, no root (all three moments clear everything
  // behind the status bytes, the root with it -- also of a call over no transaction)
  void begin(uint8_t* bitmap, uint8_t* area, size_t batch) const { fill(bitmap, 0, (batch + 7) / 8); all(area, TXOUT_REJECTED, batch); }
  // no format is enabled: every transaction of a call that has begun is outside the subset
  void nothing_in_subset(uint8_t* area, size_t batch) const { all(area, TXOUT_OUTSIDE_SUBSET, batch); }
  // a call that failed: "nothing accepted" -- never a reason, never 0, never an ID or a log entry; "outside the subset" stays
  void fail_closed(uint8_t* bitmap, uint8_t* area, size_t batch) const {
    fill(bitmap, 0, (batch + 7) / 8);
    for (size_t i = 0; area && i < batch; ++i) if (area[i] != TXOUT_OUTSIDE_SUBSET) area[i] = TXOUT_REJECTED;
    clear_behind_status(area, batch);
  }

 private:
  static void fill(uint8_t* p, int byte, size_t n) { if (p && n) std::memset(p, byte, n); }
  void clear_behind_status(uint8_t* area, size_t batch) const { if (area) fill(area + batch, 0, bytes(batch) - batch); }
  void all(uint8_t* area, int status, size_t batch) const { fill(area, status, batch); clear_behind_status(area, batch); }
};

// The format word, decoded.  of(): false for a word zkgpu_verifier_set_tx_format refuses -- negative; the log flag without a
// window K in bits 16 .. 23 or a window without the flag; the log without the IDs; signing on the device without hashing
// there; flags (or any stray bit) without one of the two base formats; precompute-only without the IDs (it has nothing else
// to hand out) or beside signing on the device (it checks no signature); the root without the IDs it is the root of, or
// beside anything but the two base formats.  0 alone is valid: no format enabled.
// The statements format (base 4: tx_statements.hpp) takes ONE flag, signing on the device, and takes it without hashing there:
// the ID arrives in the record, and there is nothing to hash for it.  Beside any other flag or a window it is refused.
struct TxFormat {
  int base = 0;                                           // 0 none, 1, 2 (the same bytes and bits as 1; the status bytes carry a reason),
                                                          // 4 (records of what the caller's own VM left; status bytes as those of 2)
  bool mute = false;                                      // (base 4 of a caller without a status argument: no reason byte is brought back)
  bool hash_on_device = false, sign_on_device = false;
  bool precompute_only = false;                           // the VM, the ID and the log alone: nothing is verified, nothing accepted (status 3)
  TxOutLayout out;
  static bool of(int word, TxFormat* f) {
    const int log_k = (word >> TXFORMAT_LOG_SHIFT) & 255;
    const bool log = (word & TXFORMAT_RETURN_LOG) != 0, ids = (word & TXFORMAT_RETURN_IDS) != 0;
    const bool hash = (word & TXFORMAT_HASH_ON_DEVICE) != 0, sign = (word & TXFORMAT_SIGN_ON_DEVICE) != 0;
    const bool pre = (word & TXFORMAT_PRECOMPUTE_ONLY) != 0, root = (word & TXFORMAT_RETURN_ROOT) != 0;
    if (word < 0 || log != (log_k != 0) || (log && !ids) || (pre && (!ids || sign)) || (root && !ids)) return false;
    const int base = word & ~(TXFORMAT_HASH_ON_DEVICE | TXFORMAT_SIGN_ON_DEVICE | TXFORMAT_RETURN_IDS | TXFORMAT_RETURN_LOG | TXFORMAT_PRECOMPUTE_ONLY | TXFORMAT_RETURN_ROOT |
                            (255 << TXFORMAT_LOG_SHIFT));
    if (base == TXFORMAT_STATEMENTS_V1 ? (hash || ids || log || pre || root) : (sign && !hash)) return false;
    if (word != 0 && base != TXFORMAT_V1 && base != TXFORMAT_V1_REASONS && base != TXFORMAT_STATEMENTS_V1) return false;
    f->base = base; f->mute = false; f->hash_on_device = hash; f->sign_on_device = sign; f->precompute_only = pre;
    f->out.ids = ids; f->out.log_k = (size_t)log_k; f->out.root = root;
    return true;
  }
  static TxFormat of_valid(int word) { TxFormat f; if (!of(word, &f)) f = TxFormat(); return f; }     // (of a word validated when it was stored)
  // What a call under the format IS, said here once -- for a decoded word and for a format filled in by hand alike; the scheduler
  // (tx_call.hpp), the device (tx_device.hpp) and the CPU stand-ins (hostlib.cpp) ask these and narrow nothing themselves.
  bool statements() const { return base == TXFORMAT_STATEMENTS_V1; }                      // the pieces are records of the caller's own VM: nothing is hashed for an ID
  bool reasons() const { return base == TXFORMAT_V1_REASONS || (statements() && !mute); } // every stage brings back a reason byte per row
  bool hashes() const { return hash_on_device && !statements(); }                         // the transaction IDs come from the device: tapes, no host second pass
  bool chains() const { return hashes() && sign_on_device; }                              // ... and the signature's challenge: keys, tape and signatures are one chain
  bool precompute() const { return precompute_only && out.ids && !chains() && !statements(); }   // the VM, the IDs and the log alone: nothing is verified
  bool forms_musig() const { return statements() && sign_on_device; }                     // a statements call whose device forms a_i and c
  bool ids() const { return out.ids; }                                                    // the caller is handed the IDs of what it accepted
  size_t log_k() const { return out.ids ? out.log_k : 0; }                                // ... and at most so many log entries per transaction (only beside the IDs)
  bool root() const { return out.ids && out.root && !statements(); }                      // ... and the root over the IDs of a call that kept every transaction
  // the same for a caller that passed no status argument: nowhere to say a reason or to put an ID or a record -- the format-1 call
  // (`mute` is read by reasons() for base 4 alone, which has no reasonless twin to fall back to; formats 1 / 2 never read it)
  TxFormat without_status() const { TxFormat f = *this; f.base = base == TXFORMAT_V1_REASONS ? TXFORMAT_V1 : base; f.mute = true; f.out = TxOutLayout(); return f; }
};

// Which calls of zkgpu_tx_verify_submit share a round, and the format the round runs under -- from the format each call was
// SUBMITTED under.  A call's kind: PRECOMPUTE, keyed by (base, hash_on_device); STATEMENTS, keyed by (sign_on_device); anything
// else VERIFY, one key whatever word the calls were submitted under (base format and device switches are read when the round
// starts, as they always were).  A round holds calls of one kind and one key.
enum class TxRoundKind { VERIFY, PRECOMPUTE, STATEMENTS };
inline TxRoundKind tx_round_kind(const TxFormat& f) { return f.precompute_only ? TxRoundKind::PRECOMPUTE : f.statements() ? TxRoundKind::STATEMENTS : TxRoundKind::VERIFY; }
inline bool tx_round_mates(const TxFormat& a, const TxFormat& b) {
  const TxRoundKind kind = tx_round_kind(a);
  if (kind != tx_round_kind(b)) return false;
  if (kind == TxRoundKind::PRECOMPUTE) return a.base == b.base && a.hash_on_device == b.hash_on_device;
  return kind != TxRoundKind::STATEMENTS || a.sign_on_device == b.sign_on_device;
}
// first: what the round's first call was submitted under; now: the verifier's format as the round starts.  A precompute-only
// round runs under the base format and the hashing switch its calls were queued under, whatever the format says by now, and
// never chains; a statements round under base 4 and the signing switch of its calls; a verifying round under the format in
// force now -- unless that is the statements format: its bytes are transactions, and it runs under its first call's word.
// `out` comes back empty (the caller ORs in the calls' layouts) and `mute` false; base 0 still means "nothing inside the subset".
inline TxFormat tx_round_format(const TxFormat& first, const TxFormat& now) {
  const TxRoundKind kind = tx_round_kind(first);
  TxFormat f;
  if (kind == TxRoundKind::PRECOMPUTE) { f.base = first.base; f.hash_on_device = first.hash_on_device; f.precompute_only = true; return f; }
  if (kind == TxRoundKind::STATEMENTS) { f.base = TXFORMAT_STATEMENTS_V1; f.sign_on_device = first.sign_on_device; return f; }
  f = now.statements() ? first : now;
  f.precompute_only = false; f.mute = false; f.out = TxOutLayout();
  return f;
}

// One call of a merged round (zkgpu_tx_verify_submit): its own bitmap ((batch + 7) / 8 bytes) and its own area of
// layout.bytes(batch), whose ID and record parts the round's TxCall wrote through the call's TxPiece.  tx_round_hand_out gives
// every call of a finished round its bits, re-based to its bit 0, and its status bytes out of the round's (the calls'
// transactions in order); ok = false, a round that failed: every call is fail-closed.  root (may be NULL; read only for a
// layout with a root): the 32 bytes the round's TxCall wrote for THIS call's transactions -- they reach the call's area only
// if the round is ok and every status byte of the call reads 0 (or every one PRECOMPUTED); the area's root is zero otherwise.
struct TxHandOut { size_t batch; TxOutLayout layout; uint8_t* bits; uint8_t* area; const uint8_t* root = nullptr; };
// does a finished call hand out every one of its transactions: all 0, or all PRECOMPUTED (never of a call over none here:
// zkgpu_tx_verify_submit takes no empty call)
inline bool tx_call_whole(const uint8_t* status, size_t batch) {
  if (batch == 0 || (status[0] != 0 && status[0] != TXOUT_PRECOMPUTED)) return false;
  for (size_t i = 1; i < batch; ++i) if (status[i] != status[0]) return false;
  return true;
}
inline void tx_round_hand_out(const uint8_t* round_bits, const uint8_t* round_status, bool ok, const TxHandOut* calls, size_t n_calls) {
  size_t at = 0;
  for (size_t c = 0; c < n_calls; ++c) {
    const TxHandOut& to = calls[c];
    if (to.batch) { std::memset(to.bits, 0, (to.batch + 7) / 8); std::memcpy(to.area, round_status + at, to.batch); }
    if (!ok) to.layout.fail_closed(to.bits, to.area, to.batch);
    for (size_t i = 0; ok && i < to.batch; ++i) {
      const size_t g = at + i;
      if ((round_bits[g / 8] >> (g % 8)) & 1) to.bits[i / 8] |= (uint8_t)(1u << (i % 8));
    }
    if (uint8_t* root = to.layout.root_of(to.area, to.batch)) {
      if (ok && to.root && tx_call_whole(to.area, to.batch)) std::memcpy(root, to.root, 32);
      else std::memset(root, 0, 32);
    }
    at += to.batch;
  }
}

}  // namespace zkvm
}  // namespace zk
