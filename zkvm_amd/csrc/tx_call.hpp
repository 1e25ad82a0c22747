// tx_call.hpp -- the SCHEDULING of one zkgpu_tx_verify_batch call (upstream: zkvm
// `Verifier::verify_tx` over a block, as recalled -- no file:line exists under /root/reference): chunks, stages, the two
// host threads and everything they share, with the device behind an interface.
//
// Until round 3 this was one 480-line function of fifteen capturing lambdas inside session.hpp (the
// round-2 and round-3 advisors each found a hazard in it).  It is a class now, and it does not know HIP: the same code is
// driven (a) by the verifier in libzkgpu (tx_device.hpp: GpuTxDevice) and (b) in libzkhost by a CPU stand-in whose
// "device" finishes its work on threads of its own after random delays (hostlib.cpp: zkhost_txcall_selftest), which the
// sanitizer tier runs under ThreadSanitizer -- the flags, the ring, the stage cuts and the hand-overs between the two
// threads are exercised on the CPU with no GPU in sight.
//
// A call is cut into equal chunks of at most 8192 transactions (4096 when the call is longer than 16 384; an override for
// tests).  Two threads:
//   the STAGING thread (made for the call; its loops run on the worker pool): per chunk a first VM pass as far as the
//     signature's keys and their MuSig coefficients (or, for a call that is ONE chunk, the stack machine alone first: the
//     proofs go out before anything is hashed), the rows (a_i, X_i) of the aggregated keys, the chunk's cloak statements
//     gathered for the device (TxDevice::proofs_stage); then, per chunk, the second pass -- everything else the VM hashes --
//     and, whenever a run of chunks has its transaction IDs made AND its aggregated keys back, the signature transcripts and
//     the rows of the equations s B - R - sum (c a_i) X_i;
//   the CALLING thread: everything that talks to the device, never waiting for one thing while another could be queued:
//     key stages (two slots, alternating), proofs (a ring of RING staging areas), signature stages (two slots).
// accept = the VM accepted & the keys decode & the signature holds & the proof verifies; fail-closed in both outputs.
//
// THE MODE of a call is one value, the device's TxFormat (tx_out.hpp: dev.format(), the verifier's format word decoded or a
// stand-in's filled in by hand), and its predicates are the only place that says which flag counts beside which.  TxCall keeps
// the value (fmt_) and asks it; what also depends on the call's own arguments stays here: reasons_ needs a status array to
// write to, ids_ / log_k_ a piece with room.  None of the switches has a host fallback: an error of a stage is an error of the call.
//
// format().reasons() (format 2, or a statements call with a status argument): every stage hands its rows one byte each beside
// the bit; verdicts() then writes, beside every clear bit, the LOWEST code that applies to the transaction -- the order
// upstream would meet the faults in: decoding and the VM (16, host), r1cs::Verifier::verify (17 .. 19), the keys the signature
// covers (20), the deferred signature check (21).  The bits are formed exactly as without reasons.
//
// ONE scheduler; two predicates change what the device does:
//   format().hashes() (ZKGPU_TXFORMAT_HASH_ON_DEVICE, never in a statements call) takes the contract IDs, the anchor ratchets and
//     the transaction-ID tree of every chunk off the staging thread: the second pass writes the chunk's plans into a tape
//     (tx_hash_tape.hpp) instead of running them, the calling thread queues the tape (hash_enqueue: one copy up, one launch, one
//     copy of the IDs down) and hands the IDs to the statements when they are back; the signature transcripts of a chunk then
//     wait for its IDs as they wait for its keys.  Two tapes may be in flight (one when two calls share the stage contexts).
//   format().chains() (hashes() and ZKGPU_TXFORMAT_SIGN_ON_DEVICE) also leaves the signature's challenge to the device
//     (tx_sig_rows.hpp), formed from the IDs and the aggregated keys where the two stages left them: a chunk's key stage, its
//     tape and its signature stage are then ONE chain on the device, ordered by events, and nothing between keys_enqueue and
//     sigs_collect of a chunk waits for the host.  The staging thread makes a chunk's signature rows in the FIRST pass, beside
//     its key rows, with the MuSig coefficients a_i where -c a_i belong; there is one signature stage per chunk (the runs of
//     ~10 000 exist for the host's transcripts), queued as soon as the chunk's keys and tape are; the key stage's bits and the
//     signature bits of a chunk are collected together, when its signature stage is through, and that is when its slot is
//     free again (the IDs are not brought down: nothing on the host reads them).  A row whose key did not decode runs through
//     all the same: its bit is ANDed with the key's.
// What the caller is handed beside the bits changes nothing of the schedule, and its layout is tx_out.hpp's (TxOutLayout, TxPiece):
//   format().ids() (ZKGPU_TXFORMAT_RETURN_IDS): the transaction ID of every ACCEPTED transaction, written by verdicts() where it
//     writes TX_OK and nowhere else (Piece::ids), from the statement's txid: the one the VM's second pass hashed for the
//     signature, or the one the device's tape produced.  Nothing is hashed for it; all it adds is that a device that chains
//     copies its IDs down after all (hash_collect with a host buffer).
//   format().log_k() (ZKGPU_TXFORMAT_RETURN_LOG, only beside ids()): also the Input / Output entries of every accepted
//     transaction's log (tx_log.hpp), one record each (Piece::log), written by verdicts() where it writes the ID.  The records
//     of the whole call are kept in a side array of the call until then: the host's second pass fills them from the slots its
//     plans wrote (tx_prepare_many_logged); a device that hashes brings the entries' contract IDs down with the transaction IDs
//     (hash_log) and the host adds counts and kinds from the tape's shape table.  Nothing is hashed for it either.
//   format().root() (ZKGPU_TXFORMAT_RETURN_ROOT, only beside ids()): also the Merkle root over the IDs of a caller's transactions in
//     call order (tx_root.hpp; Piece::root), written by verdicts() LAST and only for a piece every transaction of which was
//     handed its ID -- zeros stay otherwise.  Without hashes() the IDs are the host VM's and verdicts() folds them on the host
//     threads; with it the device hashes a leaf per transaction behind every tape (hash_place says where in the call the tape
//     starts) and, behind the LAST tape, folds every asking piece's range and copies the roots down (root_enqueue) on that
//     tape's stream -- finish() collects them where it collects the tape, and no step waits for them.
// Two predicates pick another kind of call altogether:
//   format().precompute() (ZKGPU_TXFORMAT_PRECOMPUTE_ONLY, only beside ids(), never with chains() or statements()): the call
//     VERIFIES NOTHING.  The staging thread makes ONE pass per chunk -- the VM and the plans of what the ID and the log need, run
//     on the host or, with hashes(), written to the chunk's tape with no job run at all -- and the calling thread queues and
//     collects tapes (step_precompute: the first two sub-steps of step_host_signed) or, without hashes(), only waits for the
//     staging thread.  No key stage, no proofs, no signature stage is planned, staged or queued.  verdicts() sets no bit and
//     writes PRECOMPUTED (3), never 0, beside the ID and the record of every transaction the VM ran to the end.
//   format().statements() (ZKGPU_TXFORMAT_STATEMENTS_V1): the pieces hold RECORDS of what the caller's own VM left
//     (tx_statements.hpp), not transactions.  The staging thread makes ONE pass per chunk -- the records parsed, the MuSig jobs run
//     on the host -- and no tape is ever written; the ID arrived in the record, so a chunk's signature rows wait for its keys
//     alone.  With format().forms_musig() (ZKGPU_TXFORMAT_SIGN_ON_DEVICE beside it) no transcript runs on the host at all: a key
//     stage goes out as points and offsets (keys_enqueue_formed), a chunk's signature stage right behind it as a chain whose IDs
//     the host uploads (SigChain::txids), and both are collected together.  verdicts() is the verifying call's.
// The calling thread's sub-steps (snapshot, queue_keys, queue_tape, tape_turn, proofs_turn, keys_turn, sigs_turn, queue_chain,
// chain_turn, end_step) are the same whatever the mode; what differs is when a slot counts as free and the ORDER in which the
// sub-steps run: step_host_signed(), step_chained(), step_precompute() and step_statements(), which say why.
#pragma once
#include "host_pool.hpp"
#include "tx_hash_tape.hpp"
#include "tx_log.hpp"
#include "tx_out.hpp"
#include "tx_root.hpp"
#include "tx_statements.hpp"
#include "zkvm_tx.hpp"

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace zk {
namespace zkvm {

struct TxProofSource { uint32_t n_in, n_out; const uint8_t* com; const uint8_t* proof; uint64_t proof_len; };
// What a signature stage of a device that chains waits for ON THE DEVICE: the key stage queued last in key_slot (its row r holds
// the aggregated key of row r) and the tape queued last in hash_slot (tape_pos[r]: which of its transactions row r signs).
// txids (a statements call whose device forms the coefficients: TxFormat::forms_musig): THE IDS COME FROM THE HOST -- 32 bytes
// per row, uploaded with the rows; there is no hash slot (hash_slot and tape_pos are not read: a row's ID is its own)
struct SigChain { int key_slot, hash_slot; const uint32_t* tape_pos; const uint8_t* txids = nullptr; };

// f(p, l, first, cnt) for every group of eight of `count` transactions -- the groups the VM hashes in lockstep -- with p[q],
// l[q] = where(first + q): where transaction first + q lies and how long it is
template <class Where, class F>
inline void tx_groups_of_eight(size_t count, int threads, Where where, F f) {
  host_parallel((count + 7) / 8, threads, [&](size_t g) {
    const uint8_t* p[8];
    size_t l[8];
    const size_t first = 8 * g, cnt = std::min<size_t>(8, count - first);
    for (size_t q = 0; q < cnt; ++q) { const auto at = where(first + q); p[q] = at.first; l[q] = at.second; }
    f(p, l, first, cnt);
  });
}

// What a call needs of the device.  Status codes are the library's (0 = ok).  `slot` is 0 or 1: two stages of a kind may be
// in flight, and TxCall never reuses a slot before it has collected what the slot held.
class TxDevice {
 public:
  virtual ~TxDevice() {}
  virtual const uint8_t* basepoint() = 0;                                   // 32 bytes: the encoding of B
  // aggregated keys: rows of (a_i, X_i) -> per row the encoding of sum a_i X_i (values) and "every key decodes" (ok bits)
  virtual int keys_enqueue(int slot, const uint8_t* scalars, const uint8_t* points, const uint64_t* offsets, size_t rows) = 0;
  virtual bool keys_done(int slot) = 0;                                     // never blocks
  // why (here and below; may be NULL, and is ignored unless format().reasons()): one reason byte per row, 0 beside a set bit
  virtual int keys_collect(int slot, uint8_t* ok_bits, uint8_t* values, uint8_t* why) = 0;
  // cloak proofs of one chunk.  proofs_stage runs on the STAGING thread (host work: grouping by shape, gathering into the
  // ring slot's staging area); start / finish / release on the calling thread.  A handle that was staged is released
  // exactly once -- by proofs_finish, or by proofs_release if it was never started.
  virtual int proofs_stage(size_t ring_slot, size_t n, const TxProofSource* src, int host_threads, void** handle, std::string* err) = 0;
  virtual int proofs_start(size_t ring_slot, void* handle) = 0;
  virtual bool proofs_done(void* handle) = 0;                               // never blocks: would proofs_finish return at once?
  virtual int proofs_finish(void* handle, uint8_t* accept_bits, uint8_t* why) = 0;
  virtual void proofs_release(void* handle) = 0;
  // signature equations: per row dynamic terms (scalars, points) + one term on the basepoint's table -> "is the identity".
  // chain (NULL: the scalars are final; otherwise only under a format that chains() or forms_musig()): the rows of ONE chunk in
  // the order of its key stage's rows, with the coefficients a_i in place of -c a_i -- the device forms c behind what `chain` names
  virtual int sigs_enqueue(int slot, size_t rows, const uint8_t* dyn_scalars, const uint8_t* dyn_points, const uint64_t* dyn_offsets,
                           const uint8_t* base_scalars, const SigChain* chain) = 0;
  virtual bool sigs_done(int slot) = 0;                                     // never blocks
  virtual int sigs_collect(int slot, uint8_t* bits, uint8_t* why) = 0;
  virtual std::string last_error() = 0;
  // the mode of the call the device was made for (tx_out.hpp): one value; TxCall reads it once
  virtual const TxFormat& format() const = 0;
  // transaction IDs on the device (format().hashes(); a device whose format does not say so is never asked).  hash_tape(slot):
  // the flattener of that slot, kept by the device between calls (the staging thread fills it).  hash_enqueue queues the
  // finished tape; hash_collect waits and writes 32 bytes per transaction of the tape, in the tape's order -- nowhere when the
  // pointer is null: a device that chains is only waited for, its IDs stay where its signature stage read them (with
  // format().ids() it brings them down like one that only hashes: hash_collect is given a host buffer).
  virtual TxHashTape* hash_tape(int) { return nullptr; }
  virtual int hash_enqueue(int, const TxHashTape&) { return -1; }
  virtual bool hash_done(int) { return true; }                              // never blocks
  virtual int hash_collect(int, uint8_t*) { return -1; }
  // (format().log_k() > 0) the entries' contract IDs the device gathered behind a tape: hash_log(slot), valid from a
  // hash_collect that returned 0 until the slot's next hash_enqueue, is n_tx x log_k() x 32 bytes in the tape's order, entry j
  // of a transaction whose shape logs count <= log_k() entries at [t][j], zeros elsewhere.
  virtual const uint8_t* hash_log(int) { return nullptr; }
  // (format().forms_musig()) a key stage as points and offsets alone: the device writes the scalars; the signature stage then
  // arrives as a chain whose IDs come from the host (SigChain::txids), its key terms' scalars unset.
  virtual int keys_enqueue_formed(int, const uint8_t*, const uint64_t*, size_t) { return -1; }
  // (format().root() beside format().hashes()) the roots of a call on the device.  root_begin(total), before the call's first
  // tape: a call of `total` transactions starts -- its leaves read zero.  hash_place(slot, lo), before every hash_enqueue: the
  // slot's next tape holds transactions of the call from lo on, and transaction t of it lies at lo + tape.position(t).
  // root_enqueue(slot, ranges, n), once, after the call's last tape was queued (or found empty) in `slot`: behind every tape
  // queued so far, the root over the leaves [ranges[2 r], ranges[2 r] + ranges[2 r + 1]) for r < n, and their way down.
  // root_collect waits and writes 32 bytes per range; root_done never blocks.  No host fallback: an error is the call's.
  virtual int root_begin(size_t) { return -1; }
  virtual void hash_place(int, size_t) {}
  virtual int root_enqueue(int, const uint64_t*, size_t) { return -1; }
  virtual bool root_done(int) { return true; }
  virtual int root_collect(int, uint8_t*) { return -1; }
};

class TxCall {
 public:
  static constexpr size_t RING = 6;                      // staging areas for the proofs of chunks in flight
  enum : int { OK = 0, EINVAL_ = -1, ENOMEM_ = -4 };     // (ZKGPU_OK / _EINVAL / _ENOMEM: this header does not see zkgpu.h)
  // status bytes of a call with reasons (ZKGPU_TXSTATUS_*, restated for the same reason; session.hpp asserts them)
  enum : uint8_t { WHY_NONE = 1, WHY_TX_INVALID = 16, WHY_PROOF_FIRST = 17, WHY_KEY = 20, WHY_SIGNATURE = 21 };
  static constexpr uint8_t PRECOMPUTED = TXOUT_PRECOMPUTED;     // what a precompute-only call writes where a verifying one decides between 0 and a reason

  // several callers' transactions as ONE call (zkgpu_tx_verify_submit: calls in flight are merged as tickets are): the
  // pieces in order, transaction i of the merged call = the i-th transaction counted through them.  ids / log are written only
  // under a format with ids() / with log_k() >= the piece's log_k
  using Piece = TxPiece;
  static_assert(TX_INVALID == TXOUT_REJECTED && TX_UNSUPPORTED == TXOUT_OUTSIDE_SUBSET, "tx_out.hpp restates two status bytes");
  // store: what the VM leaves per transaction, kept by the caller between calls (fresh memory costs a page fault per 4 KB);
  // at most `kept` entries of it are used, the rest of a longer call lives in the call.
  // A lone call: `status` (may be NULL) is the caller's whole status argument, laid out as the format's ids() and log_k() say
  TxCall(TxDevice& dev, std::vector<TxStatement>& store, size_t kept, size_t batch, const uint8_t* txs, const uint64_t* tx_offsets,
         int host_threads, size_t chunk_override, uint8_t* accept_bitmap, uint8_t* status, int n_slots = 2)
      : TxCall(dev, store, kept, std::vector<Piece>{TxOutLayout{dev.format().ids(), dev.format().log_k(), dev.format().root()}.piece(txs, tx_offsets, batch, status)}, host_threads,
               chunk_override, accept_bitmap, status, n_slots) {}
  TxCall(TxDevice& dev, std::vector<TxStatement>& store, size_t kept, const std::vector<Piece>& pieces, int host_threads,
         size_t chunk_override, uint8_t* accept_bitmap, uint8_t* status, int n_slots = 2)
      : dev_(dev), store_(store), batch_(total_of(pieces)), threads_(host_threads), accept_(accept_bitmap), status_(status),
        fmt_(dev.format()), reasons_(fmt_.reasons() && status != nullptr), ids_(fmt_.ids() && any_ids(pieces)), log_k_(ids_ && any_log(pieces, fmt_.log_k()) ? fmt_.log_k() : 0),
        root_(ids_ && fmt_.root() && any_root(pieces)), timing_(getenv("ZKGPU_PROVER_TIMING") != nullptr), t00_(now()), n_slots_((size_t)std::max(1, std::min(2, n_slots))) {
    ptr_.reserve(batch_); len_.reserve(batch_);
    if (root_) {
      handed_.assign(batch_, 0);
      size_t at = 0;
      for (const Piece& pc : pieces) { if (pc.root && pc.ids) { root_out_.push_back(pc.root); root_ranges_.push_back(at); root_ranges_.push_back(pc.batch); } at += pc.batch; }
      root_dev_.assign(32 * root_out_.size(), 0);
    }
    if (ids_) id_out_.reserve(batch_);
    if (log_k_) { log_out_.reserve(batch_); log_rec_.assign(batch_ * tx_log_record_bytes(log_k_), 0); }
    for (const Piece& pc : pieces) {
      if (ids_) for (size_t i = 0; i < pc.batch; ++i) id_out_.push_back(pc.ids ? pc.ids + 32 * i : nullptr);
      if (log_k_) for (size_t i = 0; i < pc.batch; ++i) log_out_.push_back({log_fits(pc, log_k_) ? pc.log + i * tx_log_record_bytes(pc.log_k) : nullptr, pc.log_k});
      for (size_t i = 0; i < pc.batch; ++i) { ptr_.push_back(pc.txs + pc.tx_offsets[i]); len_.push_back((size_t)(pc.tx_offsets[i + 1] - pc.tx_offsets[i])); }
    }
    plan(chunk_override, kept);
  }
  ~TxCall() { stop_stager(); }
  TxCall(const TxCall&) = delete;
  TxCall& operator=(const TxCall&) = delete;

  // -> 0, or the first error (both outputs then still read "nothing accepted"); error_text(): what it was
  int run() {
    const int rc = start();
    if (rc != OK) return rc;
    while (!done()) {
      if (step()) continue;
      std::unique_lock<std::mutex> lk(hm_);
      const double t0 = now();
#if defined(__SANITIZE_THREAD__)
      // (gcc 11's ThreadSanitizer does not intercept pthread_cond_clockwait, which wait_for on the steady clock becomes with
      // glibc >= 2.30: it then misses the unlock inside the wait and reports a "double lock".  Same nap on the system clock.)
      hcv_.wait_until(lk, std::chrono::system_clock::now() + std::chrono::microseconds(50));
#else
      hcv_.wait_for(lk, std::chrono::microseconds(50));
#endif
      t_wait_host_ += now() - t0;
    }
    return finish();
  }
  // The same in pieces, for a caller that drives SEVERAL calls from one thread (the engine of zkgpu_tx_verify_submit): start()
  // makes the staging thread; step() does whatever can be done now without blocking and says whether anything was; done():
  // nothing is left to queue (or the call has failed); finish() collects what is in flight and writes the verdicts.
  // on_news: called by the staging thread whenever it has published something (to wake a caller that naps elsewhere).
  void set_on_news(std::function<void()> f) { on_news_ = std::move(f); }
  int start() {
    try {
      stager_ = std::thread([this] {
        try {
          staging_main();
        } catch (...) {                                  // std::bad_alloc in practice: an error for the call, not the end of the process
          std::lock_guard<std::mutex> lk(hm_);
          stager_failed_ = true;
          hcv_.notify_all();
        }
        if (on_news_) on_news_();
      });
    } catch (...) {                                      // no thread to be had: an error for the call as well
      error_ = "the staging thread of the call could not be started";
      rc_ = ENOMEM_;
      finished_ = true;
      return ENOMEM_;
    }
    return OK;
  }
  bool done() const { return finished_; }
  // after done(): has the device finished everything this call still has in flight, i.e. would finish() return without
  // waiting?  (A caller that drives several calls asks before it calls finish(), so that it never sleeps inside one call
  // while another has work to queue.)  Never blocks.
  bool settled() {
    for (size_t s = 0; s < seg_.size(); ++s) if (seg_[s].pending && !dev_.keys_done((int)(s % n_slots_))) return false;
    const size_t n_sig = n_sig_made_locked();
    for (size_t s = 0; s < n_sig; ++s) if (sig_stages_[s]->pending && !dev_.sigs_done((int)(s % n_slots_))) return false;
    for (const auto& k : chunks_) if (k->handle && k->started && !dev_.proofs_done(k->handle)) return false;
    for (size_t c = next_hcollect_; c < next_hash_; ++c) if (hash_pending_[c] && !dev_.hash_done((int)(c % n_slots_))) return false;
    if (root_pending_ && !dev_.root_done(root_slot_)) return false;
    return true;
  }
  int finish() {
    stop_stager();
    if (timing_ && rc_ == OK) {                          // (timing only: poll, so that the marks say which chain ends the call)
      std::vector<uint8_t> seen_s(sig_stages_.size(), 0);
      const double t_end = now() + 1.0;
      while (!settled() && now() < t_end) {
        device_marks();
        for (size_t q = 0; q < n_sig_made_locked(); ++q)
          if (!seen_s[q] && sig_stages_[q]->pending && dev_.sigs_done((int)(q % n_slots_))) { seen_s[q] = 1; mark("signatures done on the device, stage", q); }
      }
      device_marks();
    }
    // (after an error: nothing is left pending on the device)
    for (size_t s = 0; s < seg_.size(); ++s) keys_collect(s);
    while (next_hcollect_ < next_hash_) hash_collect(next_hcollect_++, !fmt_.chains() || ids_);
    if (root_pending_) {                                 // (queued behind the last tape on its stream: that tape's collect has waited for it)
      root_pending_ = false;
      const int rc = dev_.root_collect(root_slot_, root_dev_.data());
      if (rc != OK) note(rc, dev_.last_error());
    }
    for (size_t s = 0; s < n_sig_made_locked(); ++s) sigs_collect(s);
    for (size_t c = 0; c < chunks_.size(); ++c) proofs_collect(*chunks_[c]);
    report();
    if (rc_ != OK) return rc_;
    verdicts();
    return OK;
  }
  const std::string& error_text() const { return error_; }
  size_t n_chunks() const { return chunks_.size(); }
  size_t n_sig_stages_planned() const { return sig_plan_.size(); }
  // transactions whose second pass ran on the host with every protocol -- the transaction ID's among them (0 on a device that hashes)
  size_t n_host_hashed() { std::lock_guard<std::mutex> lk(hm_); return n_host_hashed_; }
  // (after finish() returned OK) transactions that left a precompute-only call with PRECOMPUTED
  size_t n_precomputed() const { return n_precomputed_; }

 private:
  struct Chunk {
    size_t lo = 0, n = 0, index = 0;                     // transactions [lo, lo + n) of the call; which chunk
    size_t g0 = 0;                                       // live transactions of the call before this chunk
    std::vector<size_t> live;                            // positions in the chunk the VM accepted
    void* handle = nullptr;                              // its staged proofs
    bool started = false;
    std::vector<uint8_t> pbits, pwhy;                    // the proofs' verdicts by position in `live`; with reasons, why
    int stage_rc = 0;
    std::string stage_err;
  };
  struct Segment {                                       // the key stage of one chunk
    size_t g_lo = 0, g_hi = 0;                           // live transactions of the call (positions in live_all_)
    std::vector<uint64_t> koff;                          // rows (a_i, X_i) per live transaction
    std::vector<uint8_t> ksc, kpt, kok, kwhy;
    bool pending = false;
  };
  struct SigStage {                                      // the signature equations of a run of chunks
    size_t first = 0, last = 0;                          // chunks [first, last)
    std::vector<size_t> keyed;                           // global live indices of the transactions whose keys all decode
    std::vector<uint64_t> soff;
    std::vector<uint8_t> ssc, spt, sst, bits, why;
    std::vector<uint32_t> pos;                           // (a device that chains) per row, its transaction on the chunk's tape
    std::vector<uint8_t> ids;                            // (a statements call whose device forms a_i and c) per row, its 32-byte ID
    bool pending = false;
  };
  struct Span { size_t first, last; };

  static size_t total_of(const std::vector<Piece>& pieces) { size_t n = 0; for (const Piece& p : pieces) n += p.batch; return n; }
  static bool any_ids(const std::vector<Piece>& pieces) { for (const Piece& p : pieces) if (p.ids && p.batch) return true; return false; }
  static bool any_root(const std::vector<Piece>& pieces) { for (const Piece& p : pieces) if (p.root && p.ids && p.batch) return true; return false; }
  // (a piece's window is at most the device's: the round's device is made for the widest of its calls)
  static bool log_fits(const Piece& p, size_t k) { return p.log && p.ids && p.log_k >= 1 && p.log_k <= k; }
  static bool any_log(const std::vector<Piece>& pieces, size_t k) { for (const Piece& p : pieces) if (log_fits(p, k) && p.batch) return true; return false; }
  static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  void mark(const char* what, size_t i) const { if (timing_) fprintf(stderr, "    %7.3f ms  %s %zu\n", (now() - t00_) * 1e3, what, i); }
  TxStatement& statement(size_t i) { return i < store_.size() ? store_[i] : beyond_[i - store_.size()]; }
  void note(int rc, const std::string& what) { if (rc != OK && rc_ == OK) { rc_ = rc; error_ = what; } }

  // ---- the plan: everything that depends on the SIZE of the call alone, so that the same call made again has stages of the
  // same sizes and the device side's buffers, grown once, are never grown again
  void plan(size_t chunk_override, size_t kept) {
    std::vector<size_t> cuts{0};
    const size_t chunk = chunk_override ? chunk_override : (batch_ <= 16384 ? 8192 : 4096);
    const size_t parts = (batch_ + chunk - 1) / chunk;
    for (size_t q = 1; q < parts; ++q) cuts.push_back(chunk_override ? std::min(batch_, q * chunk) : batch_ * q / parts);
    cuts.push_back(batch_);
    // (multiples of eight: the groups of eight the VM hashes in lockstep are then the same in both passes, and none
    // straddles the end of the statement store)
    for (size_t q = 1; q + 1 < cuts.size(); ++q) cuts[q] = std::max(cuts[q - 1], cuts[q] & ~(size_t)7);
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    if (cuts.size() < 2) cuts = {0, batch_};
    const size_t n = cuts.size() - 1;
    chunks_.resize(n);
    for (size_t c = 0; c < n; ++c) {
      chunks_[c].reset(new Chunk());
      chunks_[c]->lo = cuts[c]; chunks_[c]->n = cuts[c + 1] - cuts[c]; chunks_[c]->index = c;
    }
    seg_.resize(n);
    // signature stages: runs of chunks of ~10 000 transactions in all, the last run's last chunk on its own
    for (size_t c = 0; c < n;) {
      const size_t first = c;
      size_t count = 0;
      while (c < n && (count == 0 || count + chunks_[c]->n <= 10240 + 1536)) { count += chunks_[c]->n; ++c; }
      runs_.push_back({first, c});
      if (c == n && c - first > 1) { sig_plan_.push_back({first, c - 1}); sig_plan_.push_back({c - 1, c}); }
      else sig_plan_.push_back({first, c});
    }
    if (fmt_.precompute()) { sig_plan_.clear(); all_sigs_made_ = true; }     // (no signature is looked at)
    if (fmt_.chains() || fmt_.forms_musig()) {           // one stage per chunk, all of them there from the start: chain_rows_[c] publishes c's rows
      sig_plan_.clear();
      for (size_t c = 0; c < n; ++c) { sig_plan_.push_back({c, c + 1}); sig_stages_.emplace_back(new SigStage()); sig_stages_[c]->first = c; sig_stages_[c]->last = c + 1; }
      n_sig_stages_ = sig_next_ = n; all_sigs_made_ = true;
      chain_rows_.assign(n, 0);
    }
    sig_stages_.reserve(sig_plan_.size());               // the calling thread indexes it while the staging thread appends: it never moves
    staged_.assign(n, 0); arena_free_.assign(n, 0); key_rows_.assign(n, 0); keys_arrived_.assign(n, 0);
    tape_ready_.assign(n, 0); hash_pending_.assign(n, 0);
    const size_t k8 = kept & ~(size_t)7;                 // (a multiple of eight: see the chunk boundaries)
    if (store_.size() > k8) { store_.resize(k8); store_.shrink_to_fit(); }
    if (store_.size() < std::min(batch_, k8)) store_.resize(std::min(batch_, k8));
    beyond_.resize(batch_ > store_.size() ? batch_ - store_.size() : 0);
    live_all_.reserve(batch_);
    agg_.assign(32 * std::max<size_t>(batch_, 1), 0);
    key_ok_.assign(batch_, 0);
    // A call that is ONE chunk sends its proofs first: theirs is the longest chain, and what they need is known once the VM's
    // stack machine has run, before anything is hashed.  A longer call keeps "keys, then proofs" per chunk: with proofs of
    // earlier chunks on the device, key kernels queued behind a chunk's proofs wait too long.
    proofs_first_ = n == 1;
  }

  // ================================================ staging thread ================================================
  // f(p, l, first, cnt) over the chunk's groups of eight; `first` counts from the chunk's first transaction
  template <class F> void chunk_groups(const Chunk& k, F f) {
    tx_groups_of_eight(k.n, threads_, [&](size_t i) { return std::make_pair(ptr_[k.lo + i], len_[k.lo + i]); }, f);
  }
  void vm_pass(Chunk& k, uint8_t only) {                // the VM over the chunk, hashing the jobs of `only` alone
    const double t0 = now();
    // (consecutive statements: the store's, or the overflow's -- a group of eight never straddles the two)
    // (the second pass of a call whose caller is handed the log: the same, and the entries' slots into the call's records)
    chunk_groups(k, [&](const uint8_t** p, const size_t* l, size_t first, size_t cnt) {
      if (log_k_ && only == ALL_PROTOS) tx_prepare_many_logged(p, l, &statement(k.lo + first), cnt, &log_rec_[(k.lo + first) * tx_log_record_bytes(log_k_)], log_k_);
      else tx_prepare_many(p, l, &statement(k.lo + first), cnt, true, only);
    });
    std::lock_guard<std::mutex> lk(hm_);
    (only == ALL_PROTOS ? t_vm_ : t_keys_host_) += now() - t0;
    if (only == ALL_PROTOS) n_host_hashed_ += k.n;
  }
  // the second pass of a chunk on a device that hashes: the plans into the slot's tape, the MuSig jobs alone on the host
  void vm_pass_taped(Chunk& k, TxHashTape& tape, uint8_t host_only) {
    const double t0 = now();
    std::atomic<int> bad{0};
    tape.reset(k.n);
    chunk_groups(k, [&](const uint8_t** p, const size_t* l, size_t first, size_t cnt) {
      if (!tx_prepare_many_taped(p, l, &statement(k.lo + first), cnt, tape, first, host_only)) bad = 1;
    });
    tape.finish(threads_);
    std::lock_guard<std::mutex> lk(hm_);
    if (bad) tape_failed_ = true;
    t_vm_ += now() - t0;
  }
  // the one pass of a precompute-only call over a chunk whose plans the host runs: IDs into the statements, records into log_rec_
  void vm_pass_ids(Chunk& k) {
    const double t0 = now();
    chunk_groups(k, [&](const uint8_t** p, const size_t* l, size_t first, size_t cnt) {
      tx_precompute_many(p, l, &statement(k.lo + first), cnt, log_k_ ? &log_rec_[(k.lo + first) * tx_log_record_bytes(log_k_)] : nullptr, log_k_);
    });
    std::lock_guard<std::mutex> lk(hm_);
    t_vm_ += now() - t0;
    n_host_hashed_ += k.n;
  }
  void scan(Chunk& k, Segment& sg) {                    // which transactions the VM accepts
    sg.g_lo = k.g0 = live_all_.size();
    for (size_t i = 0; i < k.n; ++i) {
      const TxStatement& t = statement(k.lo + i);
      if (status_ && t.status == TX_UNSUPPORTED) status_[k.lo + i] = TX_UNSUPPORTED;     // (TX_OK is written at the very end only)
      if (t.status == TX_OK) { k.live.push_back(i); live_all_.push_back(k.lo + i); }
    }
    k.pbits.assign((k.live.size() + 7) / 8 + 1, 0);
    if (reasons_) k.pwhy.assign(k.live.size(), (uint8_t)WHY_NONE);
    sg.g_hi = live_all_.size();
  }
  void key_rows_out(size_t ci, Segment& sg) {           // rows (a_i, X_i) of the chunk's aggregated keys -> the calling thread
    const double t0 = now();
    const size_t nl = sg.g_hi - sg.g_lo;
    sg.kok.assign((nl + 7) / 8 + 1, 0);
    if (reasons_) sg.kwhy.assign(nl, (uint8_t)WHY_NONE);
    sg.koff.assign(nl + 1, 0);
    for (size_t j = 0; j < nl; ++j) sg.koff[j + 1] = sg.koff[j] + statement(live_all_[sg.g_lo + j]).sig_scalars.size() / 32 - 2;
    sg.ksc.resize(32 * sg.koff.back()); sg.kpt.resize(32 * sg.koff.back());
    host_parallel(nl, threads_, [&](size_t j) {
      const TxStatement& t = statement(live_all_[sg.g_lo + j]);
      memcpy(sg.ksc.data() + 32 * sg.koff[j], t.sig_scalars.data() + 64, t.sig_scalars.size() - 64);
      memcpy(sg.kpt.data() + 32 * sg.koff[j], t.sig_points.data() + 64, t.sig_points.size() - 64);
    });
    std::lock_guard<std::mutex> lk(hm_);
    t_keys_host_ += now() - t0;
    key_rows_[ci] = 1;
    news();
  }
  // The rows of a signature stage, one per entry of sg.keyed, row q from the statement row(q): (x_0, R), (x_i, X_i) ... in ssc /
  // spt from soff[q] on, s for the basepoint in sst -- as the statement holds them when its row is copied.  form(first, cnt):
  // what is still to be done to the statements of rows [first, first + cnt), a group of eight, before they are copied.
  template <class Row, class Form> void lay_rows(SigStage& sg, Row row, Form form) {
    const size_t ns = sg.keyed.size();
    sg.bits.assign((ns + 7) / 8 + 1, 0);
    if (reasons_) sg.why.assign(ns, (uint8_t)WHY_NONE);
    if (ns == 0) return;
    sg.soff.assign(ns + 1, 0);
    for (size_t q = 0; q < ns; ++q) sg.soff[q + 1] = sg.soff[q] + row(q).sig_scalars.size() / 32 - 1;
    sg.ssc.resize(32 * sg.soff.back()); sg.spt.resize(32 * sg.soff.back());
    sg.sst.resize(32 * ns);
    host_parallel((ns + 7) / 8, threads_, [&](size_t g) {
      const size_t first = 8 * g, cnt = std::min<size_t>(8, ns - first);
      form(first, cnt);
      for (size_t q = first; q < first + cnt; ++q) {
        const TxStatement& t = row(q);
        memcpy(&sg.sst[32 * q], t.sig_scalars.data(), 32);
        memcpy(sg.ssc.data() + 32 * sg.soff[q], t.sig_scalars.data() + 32, t.sig_scalars.size() - 32);
        memcpy(sg.spt.data() + 32 * sg.soff[q], t.sig_points.data() + 32, t.sig_points.size() - 32);
      }
    });
  }
  // (a device that chains) the rows of the chunk's signature equations, one per live transaction in the order of its key
  // rows: (-1, R), (a_i, X_i) ..., and s on the basepoint -- everything but c -> the calling thread
  void chain_rows_out(size_t ci) {
    const double t0 = now();
    const Chunk& k = *chunks_[ci];
    SigStage& sg = *sig_stages_[ci];
    sg.keyed.resize(k.live.size());
    for (size_t q = 0; q < k.live.size(); ++q) sg.keyed[q] = k.g0 + q;
    lay_rows(sg, [&](size_t q) -> TxStatement& { return statement(k.lo + k.live[q]); }, [](size_t, size_t) {});
    if (fmt_.forms_musig()) {                            // (the IDs the records brought go up with the rows)
      sg.ids.resize(32 * k.live.size());
      for (size_t q = 0; q < k.live.size(); ++q) memcpy(&sg.ids[32 * q], statement(k.lo + k.live[q]).txid, 32);
    }
    std::lock_guard<std::mutex> lk(hm_);
    t_sig_host_ += now() - t0;
    chain_rows_[ci] = 1;
    news();
  }
  bool gather(size_t ci, Chunk& k) {                    // the chunk's cloak statements into its staging area; false: the call is over
    {
      std::unique_lock<std::mutex> lk(hm_);
      if (ci >= RING) hcv_.wait(lk, [&] { return quit_ || arena_free_[ci - RING]; });
      if (quit_) return false;
    }
    const double t1 = now();
    const size_t nl = k.live.size();
    if (nl) {
      std::vector<TxProofSource> src(nl);
      for (size_t q = 0; q < nl; ++q) {
        const TxStatement& t = statement(k.lo + k.live[q]);
        src[q] = TxProofSource{t.n_in, t.n_out, t.commitments.data(), t.proof, t.proof_len};
      }
      k.stage_rc = dev_.proofs_stage(ci % RING, nl, src.data(), threads_, &k.handle, &k.stage_err);
    }
    const double t2 = now();
    if (timing_) fprintf(stderr, "    staging thread, chunk %zu: gather %.3f ms\n", ci, (t2 - t1) * 1e3);
    std::lock_guard<std::mutex> lk(hm_);
    t_stage_host_ += t2 - t1;
    staged_[ci] = 1;
    news();
    return true;
  }
  void sig_rows(SigStage& sg) {                         // transcripts + rows of the equations of chunks [first, last)
    const size_t g_lo = chunks_[sg.first]->g0, g_hi = chunks_[sg.last - 1]->g0 + chunks_[sg.last - 1]->live.size();
    sg.keyed.clear();
    for (size_t g = g_lo; g < g_hi; ++g) if (key_ok_[g]) sg.keyed.push_back(g);
    const uint8_t* B = dev_.basepoint();
    const auto row = [&](size_t q) -> TxStatement& { return statement(live_all_[sg.keyed[q]]); };
    lay_rows(sg, row, [&](size_t first, size_t cnt) {                  // eight challenges c = H(txid, X, R) at a time
      TxStatement* tp[8];
      const uint8_t* ap[8];
      for (size_t q = 0; q < cnt; ++q) { tp[q] = &row(first + q); ap[q] = &agg_[32 * sg.keyed[first + q]]; }
      tx_finish_signature_many(tp, ap, B, cnt);
    });
  }
  void news() { hcv_.notify_all(); if (on_news_) on_news_(); }     // (hm_ held)
  bool keys_back(const Span& sp) const { for (size_t c = sp.first; c < sp.last; ++c) if (!keys_arrived_[c]) return false; return true; }
  // the signature stages that are due: their chunks' transaction IDs made, their keys back (hm_ held on entry and on return)
  void make_sig_stages(std::unique_lock<std::mutex>& lk, size_t ids_upto) {
    while (!quit_ && sig_next_ < sig_plan_.size() && sig_plan_[sig_next_].last <= ids_upto && keys_back(sig_plan_[sig_next_])) {
      std::unique_ptr<SigStage> sg(new SigStage());
      sg->first = sig_plan_[sig_next_].first; sg->last = sig_plan_[sig_next_].last;
      ++sig_next_;
      lk.unlock();
      const double t0 = now();
      sig_rows(*sg);
      const double dt = now() - t0;
      lk.lock();
      t_sig_host_ += dt;
      sig_stages_.push_back(std::move(sg));              // (reserved: never reallocates)
      ++n_sig_stages_;
      if (sig_next_ == sig_plan_.size()) all_sigs_made_ = true;
      news();
    }
  }
  // the stages that are due, until all of them are made (or the call is over): how a staging loop that makes them ends
  void make_sig_stages_to_the_end() {
    std::unique_lock<std::mutex> lk(hm_);
    for (;;) {
      make_sig_stages(lk, ids_upto_);
      if (quit_ || all_sigs_made_) return;
      hcv_.wait(lk, [&] { return quit_ || (keys_back(sig_plan_[sig_next_]) && sig_plan_[sig_next_].last <= ids_upto_); });
    }
  }
  // (hashes()) chunk ci's tape: wait for its slot -- free once chunk ci - n_slots has been collected --, write it (the jobs of
  // host_only alone run on the host), publish it; false: the call is over.  scanned (a precompute-only call, whose ONE pass
  // this is): which transactions the VM accepted, found before the tape is published
  bool tape_out(size_t ci, uint8_t host_only, Segment* scanned = nullptr) {
    {
      std::unique_lock<std::mutex> lk(hm_);
      hcv_.wait(lk, [&] { return quit_ || ids_upto_ + n_slots_ > ci; });
      if (quit_) return false;
    }
    vm_pass_taped(*chunks_[ci], *dev_.hash_tape((int)(ci % n_slots_)), host_only);
    if (scanned) scan(*chunks_[ci], *scanned);
    std::lock_guard<std::mutex> lk(hm_);
    if (quit_) return false;
    tape_ready_[ci] = 1;
    news();
    return true;
  }
  // A precompute-only call: one pass per chunk and nothing else.  With hashes() the pass writes the chunk's tape and runs no
  // job; otherwise it runs what the IDs and the log need.
  void staging_precompute() {
    for (size_t ci = 0; ci < chunks_.size(); ++ci) {
      if (fmt_.hashes()) {
        if (!tape_out(ci, NO_PROTO, &seg_[ci])) return;
        continue;
      }
      vm_pass_ids(*chunks_[ci]);
      scan(*chunks_[ci], seg_[ci]);
      std::lock_guard<std::mutex> lk(hm_);
      if (quit_) return;
      hashed_upto_ = ids_upto_ = ci + 1;
      news();
    }
  }
  // A statements call: ONE pass per chunk -- the records parsed, the MuSig jobs run unless the device forms the coefficients --
  // and no tape.  Per chunk the proofs are staged first (theirs is the longest chain, and a record holds all they need), then
  // the key rows, then (a device that forms a_i and c) the signature rows; the IDs arrived with the records, so the signature
  // transcripts of a chunk wait for its aggregated keys alone.
  void parse_pass(Chunk& k) {
    const double t0 = now();
    chunk_groups(k, [&](const uint8_t** p, const size_t* l, size_t first, size_t cnt) { tx_statements_many(p, l, &statement(k.lo + first), cnt, !fmt_.forms_musig()); });
    std::lock_guard<std::mutex> lk(hm_);
    t_keys_host_ += now() - t0;
  }
  void staging_statements() {
    for (size_t ci = 0; ci < chunks_.size(); ++ci) {
      Chunk& k = *chunks_[ci];
      parse_pass(k);
      scan(k, seg_[ci]);
      if (!gather(ci, k)) return;
      key_rows_out(ci, seg_[ci]);
      if (fmt_.forms_musig()) chain_rows_out(ci);
      std::unique_lock<std::mutex> lk(hm_);
      hashed_upto_ = ids_upto_ = ci + 1;
      if (!fmt_.forms_musig()) make_sig_stages(lk, ids_upto_);
      if (quit_) return;
    }
    if (!fmt_.forms_musig()) make_sig_stages_to_the_end();  // (else every stage was made beside its key rows)
  }
  void staging_main() {
    if (fmt_.statements()) { staging_statements(); return; }
    if (fmt_.precompute()) { staging_precompute(); return; }
    for (const Span& run : runs_) {                     // a run of chunks: keys and proofs of each on their way, then their IDs
      for (size_t ci = run.first; ci < run.last; ++ci) {
        Chunk& k = *chunks_[ci];
        Segment& sg = seg_[ci];
        // what the proofs need -- arity, commitments, proof bytes -- is known once the VM's stack machine has run; the keys
        // X_i and their MuSig coefficients a_i after the plan's MuSig jobs have; everything else (contract ids, anchors, the
        // transaction ID) only the signature transcripts wait for: the second pass below
        if (proofs_first_) {
          vm_pass(k, NO_PROTO);
          scan(k, sg);
          if (!gather(ci, k)) return;
          vm_pass(k, P_MUSIG);
          key_rows_out(ci, sg);
          if (fmt_.chains()) chain_rows_out(ci);
        } else {
          vm_pass(k, P_MUSIG);
          scan(k, sg);
          key_rows_out(ci, sg);
          if (fmt_.chains()) chain_rows_out(ci);
          if (!gather(ci, k)) return;
        }
      }
      for (size_t ci = run.first; ci < run.last; ++ci) {   // second pass, chunk by chunk
        {
          std::unique_lock<std::mutex> lk(hm_);
          make_sig_stages(lk, std::min(ci, ids_upto_));
          if (quit_) return;
        }
        if (fmt_.hashes()) {                               // the chunk's plans go to its tape, the MuSig jobs alone run here
          if (!tape_out(ci, P_MUSIG)) return;
          continue;
        }
        vm_pass(*chunks_[ci], ALL_PROTOS);
        std::lock_guard<std::mutex> lk(hm_);
        hashed_upto_ = ids_upto_ = ci + 1;
      }
    }
    if (!fmt_.chains()) make_sig_stages_to_the_end();       // (else every stage was made in the first pass)
  }
  void stop_stager() {
    { std::lock_guard<std::mutex> lk(hm_); quit_ = true; }
    hcv_.notify_all();
    if (stager_.joinable()) stager_.join();
  }

  // ================================================ calling thread ================================================
  size_t n_sig_made_locked() { std::lock_guard<std::mutex> lk(hm_); return n_sig_stages_; }
  void keys_collect(size_t s) {
    Segment& sg = seg_[s];
    if (!sg.pending) return;
    sg.pending = false;
    const double t0 = now();
    const int rc = dev_.keys_collect((int)(s % n_slots_), sg.kok.data(), agg_.data() + 32 * sg.g_lo, reasons_ ? sg.kwhy.data() : nullptr);
    if (rc != OK) note(rc, dev_.last_error());
    t_wait_ += now() - t0;
    for (size_t j = 0; j < sg.g_hi - sg.g_lo; ++j) key_ok_[sg.g_lo + j] = (sg.kok[j / 8] >> (j % 8)) & 1;
    mark("keys collected, segment", s);
  }
  void sigs_collect(size_t s) {
    SigStage& sg = *sig_stages_[s];                      // (s < the count read under hm_: the element is published)
    if (!sg.pending) return;
    sg.pending = false;
    const double t0 = now();
    const int rc = dev_.sigs_collect((int)(s % n_slots_), sg.bits.data(), reasons_ ? sg.why.data() : nullptr);
    if (rc != OK) note(rc, dev_.last_error());
    t_wait_ += now() - t0;
    mark("signatures collected, stage", s);
  }
  // the IDs of chunk c, from the device to the statements; the staging thread is told (ids_upto_).  (to_host = false, a
  // device that chains and a caller that does not ask for IDs: nothing on the host reads them -- the slot's tape is
  // collected and nothing is copied)
  void hash_collect(size_t c, bool to_host = true) {
    Chunk& k = *chunks_[c];
    if (hash_pending_[c]) {
      hash_pending_[c] = 0;
      const double t0 = now();
      const TxHashTape& tape = *dev_.hash_tape((int)(c % n_slots_));
      hash_ids_.resize(32 * tape.n_tx() + 32);
      const int rc = dev_.hash_collect((int)(c % n_slots_), to_host ? hash_ids_.data() : nullptr);
      if (rc != OK) note(rc, dev_.last_error());
      else if (to_host) for (size_t t = 0; t < tape.n_tx(); ++t) memcpy(statement(k.lo + tape.position(t)).txid, &hash_ids_[32 * t], 32);
      if (rc == OK && log_k_ && tape.n_tx()) log_collect(k, tape, dev_.hash_log((int)(c % n_slots_)));
      t_wait_ += now() - t0;
      mark("transaction IDs collected, chunk", c);
    }
    { std::lock_guard<std::mutex> lk(hm_); ids_upto_ = c + 1; }
    hcv_.notify_all();
  }
  // the records of a chunk whose tape is back: the IDs the device gathered, counts and kinds from the tape's shape table
  void log_collect(const Chunk& k, const TxHashTape& tape, const uint8_t* gathered) {
    if (!gathered || !tx_log_table(tape.block(), log_table_)) { note(EINVAL_, "the hashing stage brought no log entries back"); return; }
    const HashTapeHead& h = tape.head();
    for (size_t t = 0; t < tape.n_tx(); ++t) {
      const uint32_t* sh = tx_log_shape(log_table_, (tape.block() + h.txs + 4 * t)[0]);
      uint8_t* rec = &log_rec_[(k.lo + tape.position(t)) * tx_log_record_bytes(log_k_)];
      memset(rec, 0, tx_log_record_bytes(log_k_));
      tx_log_record(rec, log_k_, sh[0], [&](size_t j) { return std::make_pair(sh[1 + 2 * j], gathered + 32 * (t * log_k_ + j)); });
    }
  }
  void proofs_collect(Chunk& k) {
    if (k.handle) {
      if (k.started) {
        const double t0 = now();
        const int rc = dev_.proofs_finish(k.handle, k.pbits.data(), reasons_ ? k.pwhy.data() : nullptr);
        if (rc != OK) note(rc, dev_.last_error());
        t_wait_ += now() - t0;
        mark("proofs collected, chunk at", k.lo);
      } else {
        dev_.proofs_release(k.handle);
      }
      k.handle = nullptr; k.started = false;
    }
    std::lock_guard<std::mutex> lk(hm_);
    arena_free_[k.index] = 1;
    hcv_.notify_all();
  }
  void enqueue_proofs(size_t ci) {
    Chunk& k = *chunks_[ci];
    mark("staged, chunk", ci);
    if (k.stage_rc != OK) { note(k.stage_rc, k.stage_err); return; }
    if (k.live.empty() || !k.handle) return;
    const double t0 = now();
    const int rc = dev_.proofs_start(ci % RING, k.handle);
    if (rc != OK) note(rc, dev_.last_error()); else k.started = true;
    t_stage_ += now() - t0;
    mark("proofs queued, chunk", ci);
  }
  // ---- the sub-steps of step(): each does, without blocking, the one thing its name says if it can be done now, and says
  // whether it did.  What the staging thread has published is read once per step, under hm_:
  struct Ready {
    bool rows = false, staged = false, ring_free = true, tape = false, sig_rows = false;     // of next_key_ / next_stage_ (and its ring slot) / next_hash_ / next_sig_ (chained)
    bool sigs_all = false;                                                                   // every signature stage of the call is made,
    size_t sig_avail = 0;                                                                    // so many of them so far
    size_t ids_upto = 0;                                                                     // chunks whose IDs are in the statements (read by step_precompute alone)
  };
  bool snapshot(Ready& r) {                              // false: the staging thread has failed, and the call is over
    const size_t n = chunks_.size();
    std::lock_guard<std::mutex> lk(hm_);
    if (stager_failed_) { note(ENOMEM_, "out of host memory while staging the transactions"); finished_ = true; return false; }
    r.sig_avail = n_sig_stages_; r.sigs_all = all_sigs_made_; r.ids_upto = ids_upto_;
    if (next_key_ < n) r.rows = key_rows_[next_key_] != 0;
    if (next_stage_ < n) r.staged = staged_[next_stage_] != 0;
    if (next_stage_ >= RING) r.ring_free = arena_free_[next_stage_ - RING] != 0;
    if (fmt_.hashes() && next_hash_ < n) r.tape = tape_ready_[next_hash_] != 0;
    if ((fmt_.chains() || fmt_.forms_musig()) && next_sig_ < n) r.sig_rows = chain_rows_[next_sig_] != 0;
    if (tape_failed_) note(EINVAL_, "a transaction's hash plan does not fit the device's tape");
    return true;
  }
  // the key stage of segment next_key_.  go: its slot is free -- what held it last has been collected -- and the mode queues it now
  // (rc_ is the caller's to ask: step_host_signed() does not, and a key stage may follow a tape that failed in the same step --
  // finish() collects it)
  bool queue_keys(const Ready& r, bool go) {
    if (!r.rows || !go) return false;
    Segment& sg = seg_[next_key_];
    mark("key rows ready, segment", next_key_);
    const double t0 = now();
    if (sg.g_hi > sg.g_lo) {
      // (a statements call whose device forms the coefficients: points and offsets alone -- the scalars are the device's to write)
      const int rc = fmt_.forms_musig() ? dev_.keys_enqueue_formed((int)(next_key_ % n_slots_), sg.kpt.data(), sg.koff.data(), sg.g_hi - sg.g_lo)
                                : dev_.keys_enqueue((int)(next_key_ % n_slots_), sg.ksc.data(), sg.kpt.data(), sg.koff.data(), sg.g_hi - sg.g_lo);
      if (rc != OK) note(rc, dev_.last_error()); else sg.pending = true;
    }
    t_keys_ += now() - t0;
    mark("keys queued, segment", next_key_);
    ++next_key_;
    return true;
  }
  // the tape of chunk next_hash_ (a device that hashes).  slot_free: as for the keys
  bool queue_tape(const Ready& r, bool slot_free) {
    if (rc_ != OK || !r.tape || !slot_free) return false;
    const int slot = (int)(next_hash_ % n_slots_);
    const TxHashTape& tape = *dev_.hash_tape(slot);
    const double t0 = now();
    // (a call whose pieces ask for their roots: the leaves are zeroed before the first tape, every tape is told where it starts)
    if (root_ && next_hash_ == 0) { const int rc = dev_.root_begin(batch_); if (rc != OK) note(rc, dev_.last_error()); }
    if (root_) dev_.hash_place(slot, chunks_[next_hash_]->lo);
    if (tape.n_tx() && rc_ == OK) {
      const int rc = dev_.hash_enqueue(slot, tape);
      if (rc != OK) note(rc, dev_.last_error()); else hash_pending_[next_hash_] = 1;
    }
    t_keys_ += now() - t0;
    mark("transaction-ID tape queued, chunk", next_hash_);
    ++next_hash_;
    // (... and behind the last tape the folds and the roots' way down, on its stream)
    if (root_ && next_hash_ == chunks_.size() && rc_ == OK) {
      const int rc = dev_.root_enqueue(slot, root_ranges_.data(), root_out_.size());
      if (rc != OK) note(rc, dev_.last_error()); else { root_pending_ = true; root_slot_ = slot; }
    }
    return true;
  }
  // the proofs of chunk next_stage_, if the mode lets them start now: the ring slot's last chunk is collected as soon as the
  // device is through with it, and the chunk's proofs go out when the staging thread has staged them
  bool proofs_turn(const Ready& r, bool may_start) {
    if (rc_ != OK || next_stage_ >= chunks_.size() || !may_start) return false;
    bool progress = false;
    if (!r.ring_free) {
      Chunk& old = *chunks_[next_stage_ - RING];
      if (!old.handle || !old.started || dev_.proofs_done(old.handle)) { proofs_collect(old); progress = true; }
    }
    if (r.staged) { enqueue_proofs(next_stage_++); progress = true; }
    return progress;
  }
  bool end_step(bool progress) {
    if (rc_ != OK) { finished_ = true; return true; }
    if (timing_) device_marks();
    return progress;
  }
  // The calling thread never waits for one thing while another could be queued: it looks, in turn, for the key rows of a
  // chunk (its key stage goes out, before any of its proofs: what follows the keys is a chain, keys -> host transcripts ->
  // equations, and queued behind the proofs' chip-filling kernels its short kernels would wait for CUs), for a chunk the
  // staging thread has finished (its proofs go out), for aggregated keys that have arrived (the staging thread is told), and
  // for signature stages that are ready (the equations go out); with nothing to do it sleeps until the staging thread has
  // news, 50 us at most (what the device has finished is found out by asking).  On a device that hashes, a chunk's tape and
  // the IDs that are back come first of all: the transcripts wait for them.
  bool step_host_signed(const Ready& r) {
    const size_t n = chunks_.size();
    if (next_kcollect_ == n && next_stage_ == n && r.sigs_all && next_sig_ == r.sig_avail && (!fmt_.hashes() || next_hcollect_ == n)) { finished_ = true; return true; }
    bool progress = queue_tape(r, next_hcollect_ + n_slots_ > next_hash_);     // (its slot is free once chunk next_hash - n_slots is collected)
    progress |= tape_turn();
    // (... once segment next_key - n_slots is collected.  Unlike its siblings, and unlike step_chained(), the keys are queued
    // without asking rc_: this order always has queued them in the step in which a tape failed; finish() collects the stage)
    progress |= queue_keys(r, next_kcollect_ + n_slots_ > next_key_);
    progress |= proofs_turn(r, proofs_first_ || next_stage_ < next_key_);      // (a chunk's proofs after its keys, unless the call is one chunk)
    progress |= keys_turn();
    progress |= sigs_turn(r);
    return end_step(progress);
  }
  // the oldest tape in flight, if the device is through with it: its IDs collected into the statements, and the staging thread is told
  bool tape_turn() {
    if (rc_ != OK || next_hcollect_ >= next_hash_ || (hash_pending_[next_hcollect_] && !dev_.hash_done((int)(next_hcollect_ % n_slots_)))) return false;
    hash_collect(next_hcollect_++);
    return true;
  }
  // the aggregated keys of segment next_kcollect_, if the device is through with them: collected, and the staging thread is told
  bool keys_turn() {
    if (rc_ != OK || next_kcollect_ >= next_key_ || (seg_[next_kcollect_].pending && !dev_.keys_done((int)(next_kcollect_ % n_slots_)))) return false;
    keys_collect(next_kcollect_);
    { std::lock_guard<std::mutex> lk(hm_); keys_arrived_[next_kcollect_] = 1; }
    hcv_.notify_all();
    ++next_kcollect_;
    return true;
  }
  // the signature stages the staging thread has made (host transcripts), as far as their slots are free
  bool sigs_turn(const Ready& r) {
    bool progress = false;
    while (rc_ == OK && next_sig_ < r.sig_avail) {
      const double t0 = now();
      if (next_sig_ >= n_slots_) {                                            // the stage that used this slot last: collected once it is done
        if (sig_stages_[next_sig_ - n_slots_]->pending && !dev_.sigs_done((int)(next_sig_ % n_slots_))) break;
        sigs_collect(next_sig_ - n_slots_);
      }
      SigStage& sg = *sig_stages_[next_sig_];
      const size_t ns = sg.keyed.size();
      if (ns) {
        const int rc = dev_.sigs_enqueue((int)(next_sig_ % n_slots_), ns, sg.ssc.data(), sg.spt.data(), sg.soff.data(), sg.sst.data(), nullptr);
        if (rc != OK) note(rc, dev_.last_error()); else sg.pending = true;
      }
      t_sigs_ += now() - t0;
      mark("signatures queued, stage", next_sig_);
      ++next_sig_;
      progress = true;
    }
    return progress;
  }
  // (chains() or forms_musig()) the signature stage of chunk next_sig_, a chain behind what the chunk queued before it.
  // stages_queued: those are queued -- its key stage, and its tape where the mode has one (the device orders them)
  bool queue_chain(const Ready& r, bool stages_queued) {
    if (rc_ != OK || !r.sig_rows || !stages_queued) return false;
    const double t0 = now();
    chain_enqueue(next_sig_);
    t_sigs_ += now() - t0;
    mark("signatures queued, stage", next_sig_);
    ++next_sig_;
    return true;
  }
  // ... and what the oldest chain in flight brought back, once its signature stage is through: signature bits, key bits and --
  // where the mode has one -- its tape (the IDs themselves only for a caller that is handed them).  That frees the chunk's slot.
  bool chain_turn() {
    if (rc_ != OK || next_chain_ >= next_sig_ || (sig_stages_[next_chain_]->pending && !dev_.sigs_done((int)(next_chain_ % n_slots_)))) return false;
    sigs_collect(next_chain_);
    keys_collect(next_chain_);
    if (fmt_.chains()) { hash_collect(next_chain_, ids_); next_hcollect_ = next_chain_ + 1; }
    next_kcollect_ = ++next_chain_;
    return true;
  }
  // A statements call (tx_statements.hpp): the same sub-steps in a fourth order.  A chunk's proofs go out first, as soon as the
  // staging thread has staged them -- a record holds all they need, and nothing is hashed before them --; then its key stage;
  // then its signature stage.  No tape is ever asked for, and nothing waits for an ID.  With the host's transcripts the
  // signature stages are the staging thread's runs, made when their keys are back (step_host_signed's last two sub-steps);
  // on a device that forms a_i and c a chunk's signature stage is queued right behind its key stage (the device orders the
  // two), and both are collected together, oldest chunk first, which frees their slot (step_chained's, without the tape).
  bool step_statements(const Ready& r) {
    const size_t n = chunks_.size();
    if (fmt_.forms_musig() ? (next_chain_ == n && next_stage_ == n) : (next_kcollect_ == n && next_stage_ == n && r.sigs_all && next_sig_ == r.sig_avail)) { finished_ = true; return true; }
    bool progress = proofs_turn(r, true);
    progress |= queue_keys(r, rc_ == OK && (fmt_.forms_musig() ? next_chain_ : next_kcollect_) + n_slots_ > next_key_);
    if (fmt_.forms_musig()) { progress |= queue_chain(r, next_sig_ < next_key_); progress |= chain_turn(); }
    else { progress |= keys_turn(); progress |= sigs_turn(r); }
    return end_step(progress);
  }
  // The same for a device that chains.  Per chunk, in order: its key stage and its tape go out when the staging thread has
  // made them and the chunk that used their slot last has been collected; its signature stage as soon as both are queued
  // (the device orders the three); its proofs as before.  What a chunk brought back -- signature bits, key bits -- is
  // collected when its signature stage is through, oldest chunk first (its tape's slot is released then too: the IDs
  // themselves stay on the device); nothing else is waited for.
  bool step_chained(const Ready& r) {
    const size_t n = chunks_.size();
    if (next_chain_ == n && next_stage_ == n) { finished_ = true; return true; }
    bool progress = queue_keys(r, rc_ == OK && next_chain_ + n_slots_ > next_key_);
    progress |= queue_tape(r, next_chain_ + n_slots_ > next_hash_);
    progress |= queue_chain(r, next_sig_ < next_key_ && next_sig_ < next_hash_);
    // (a chunk's proofs after its keys -- unless its keys wait for a slot: a slot is free again only when a whole chain has been
    // collected, the first chain needs the first tape, and the staging thread writes tapes after it has gathered every chunk of
    // the run, for which the ring's areas must come free -- the proofs must not wait for keys that wait for them)
    progress |= proofs_turn(r, proofs_first_ || next_stage_ < next_key_ || next_key_ >= next_chain_ + n_slots_);
    progress |= chain_turn();
    return end_step(progress);
  }
  // A precompute-only call: the tapes and nothing else, in the order of step_host_signed() -- a chunk's tape goes out when the
  // staging thread has written it and its slot is free, the IDs that are back are collected.  Without a device that hashes there
  // is nothing to queue: the call is through when the staging thread has passed the last chunk.
  bool step_precompute(const Ready& r) {
    const size_t n = chunks_.size();
    if (fmt_.hashes() ? next_hcollect_ == n : r.ids_upto == n) { finished_ = true; return true; }
    if (!fmt_.hashes()) return end_step(false);
    bool progress = queue_tape(r, next_hcollect_ + n_slots_ > next_hash_);
    progress |= tape_turn();
    return end_step(progress);
  }
 public:
  bool step() {
    if (finished_) return false;
    if (rc_ != OK) { finished_ = true; return true; }
    Ready r;
    if (!snapshot(r)) return true;
    return fmt_.statements() ? step_statements(r) : fmt_.precompute() ? step_precompute(r) : fmt_.chains() ? step_chained(r) : step_host_signed(r);
  }
 private:
  // chunk c's signature stage as a chain behind its key stage and -- chains() -- its tape (both queued, or empty like the stage
  // itself); forms_musig(): there is no tape, the rows' IDs go up with them
  void chain_enqueue(size_t c) {
    const Chunk& k = *chunks_[c];
    SigStage& sg = *sig_stages_[c];
    const size_t ns = sg.keyed.size();
    if (ns == 0) return;
    const int slot = (int)(c % n_slots_);
    SigChain chain{slot, -1, nullptr};
    if (fmt_.forms_musig()) {
      if (!seg_[c].pending || sg.ids.size() != 32 * ns) { note(EINVAL_, "a signature stage without its key stage or its IDs"); return; }
      chain.txids = sg.ids.data();
    } else {
      const TxHashTape& tape = *dev_.hash_tape(slot);
      std::vector<uint32_t> at(k.n, TAPE_IDLE);
      for (size_t t = 0; t < tape.n_tx(); ++t) if (tape.position(t) < k.n) at[tape.position(t)] = (uint32_t)t;
      sg.pos.resize(ns);
      for (size_t q = 0; q < ns; ++q) {
        sg.pos[q] = at[k.live[q]];
        if (sg.pos[q] == TAPE_IDLE) { note(EINVAL_, "a transaction the VM accepted has no ID on its chunk's tape"); return; }
      }
      if (!seg_[c].pending || !hash_pending_[c]) { note(EINVAL_, "a signature stage without its key stage or its tape"); return; }
      chain.hash_slot = slot; chain.tape_pos = sg.pos.data();
    }
    const int rc = dev_.sigs_enqueue(slot, ns, sg.ssc.data(), sg.spt.data(), sg.soff.data(), sg.sst.data(), &chain);
    if (rc != OK) note(rc, dev_.last_error()); else sg.pending = true;
  }
  // (timing only) when the device is through with a chunk's proofs / a signature stage, as seen by the polling thread
  void device_marks() {
    if (seen_pdone_.size() != chunks_.size()) seen_pdone_.assign(chunks_.size(), 0);
    for (size_t c = 0; c < chunks_.size(); ++c) {
      Chunk& k = *chunks_[c];
      if (!seen_pdone_[c] && k.handle && k.started && dev_.proofs_done(k.handle)) { seen_pdone_[c] = 1; mark("proofs done on the device, chunk", c); }
    }
  }
  // what a precompute-only call writes: no bit; PRECOMPUTED, the ID and the record of every transaction the VM ran to the end;
  // beside the others what the host VM alone finds, as a verifying call of the same base format says it
  void precomputed_out() {
    for (const auto& kp : chunks_) {
      const Chunk& k = *kp;
      for (size_t j = 0; j < k.live.size(); ++j) {
        const size_t i = k.lo + k.live[j];
        if (status_) status_[i] = PRECOMPUTED;
        hand_out(i);
        ++n_precomputed_;
      }
    }
    if (reasons_) host_reasons_out();
  }
  // transaction i's ID and record to its caller, where that caller has room for them
  void hand_out(size_t i) {
    if (root_) handed_[i] = 1;
    if (ids_ && id_out_[i]) memcpy(id_out_[i], statement(i).txid, 32);
    if (log_k_ && log_out_[i].first) tx_log_record_copy(log_out_[i].first, log_out_[i].second, &log_rec_[i * tx_log_record_bytes(log_k_)], log_k_);
  }
  void verdicts() {
    if (fmt_.precompute()) { precomputed_out(); roots_out(); return; }
    std::vector<uint8_t> sig_ok(live_all_.size(), 0);
    // (key_ok_ matters for a chained stage alone, whose rows include those with an undecodable key; an unchained stage's
    // `keyed` holds only rows whose keys decoded, and the test is always true there)
    for (const auto& sg : sig_stages_)
      for (size_t q = 0; q < sg->keyed.size(); ++q) if (((sg->bits[q / 8] >> (q % 8)) & 1) && key_ok_[sg->keyed[q]]) sig_ok[sg->keyed[q]] = 1;
    for (const auto& kp : chunks_) {
      const Chunk& k = *kp;
      for (size_t j = 0; j < k.live.size(); ++j) {
        if (!sig_ok[k.g0 + j] || !((k.pbits[j / 8] >> (j % 8)) & 1)) continue;
        const size_t i = k.lo + k.live[j];
        accept_[i / 8] |= (uint8_t)(1u << (i % 8));
        if (status_) status_[i] = TX_OK;
        hand_out(i);                                         // (here alone: an ID or a record leaves only beside a set bit)
      }
    }
    if (reasons_) reasons_out();
    roots_out();
  }
  // The root of every piece that asked for one and whose transactions were ALL handed their IDs (a piece's root area is zero
  // until here, and stays zero otherwise): the device's where it hashed the IDs, else the fold of the statements' IDs on the
  // host threads (tx_root_fold_host).  Last of all: after the last ID.
  void roots_out() {
    if (!root_) return;
    std::vector<uint8_t> ids;
    for (size_t r = 0; r < root_out_.size(); ++r) {
      const size_t lo = (size_t)root_ranges_[2 * r], n = (size_t)root_ranges_[2 * r + 1];
      bool whole = true;
      for (size_t i = lo; i < lo + n && whole; ++i) whole = handed_[i] != 0;
      if (!whole) continue;
      if (fmt_.hashes() && n) { memcpy(root_out_[r], &root_dev_[32 * r], 32); continue; }
      ids.resize(32 * n);
      for (size_t i = 0; i < n; ++i) memcpy(&ids[32 * i], statement(lo + i).txid, 32);
      tx_root_fold_host(ids.data(), n, TX_ROOT_SPAN, threads_, root_out_[r]);
    }
  }
  // what the host itself rejected: the transaction (16) -- except the one check of the SIGNATURE the VM makes on the host, a
  // scalar s that is not canonical, which is the signature's reason (the text is zkvm_tx.hpp's, which keeps one status for both)
  static uint8_t host_reason(const TxStatement& t) {
    return strcmp(t.why, "signature scalar not canonical") == 0 ? (uint8_t)WHY_SIGNATURE : (uint8_t)WHY_TX_INVALID;
  }
  // Beside every clear bit of a transaction inside the subset, the lowest code that applies; 0 stays where verdicts() wrote it,
  // beside a set bit, and nowhere else.  A transaction no stage gave a reason for (cannot happen) reads "rejected" alone.
  void host_reasons_out() { for (size_t i = 0; i < batch_; ++i) if (statement(i).status == TX_INVALID) status_[i] = host_reason(statement(i)); }
  void reasons_out() {
    host_reasons_out();
    std::vector<uint8_t> sig_why(live_all_.size(), 0);
    for (const auto& sg : sig_stages_)
      for (size_t q = 0; q < sg->keyed.size(); ++q) sig_why[sg->keyed[q]] = sg->why[q];
    for (size_t s = 0; s < seg_.size(); ++s) {
      const Chunk& k = *chunks_[s];
      const Segment& sg = seg_[s];
      for (size_t j = 0; j < k.live.size(); ++j) {
        const size_t i = k.lo + k.live[j];
        if ((accept_[i / 8] >> (i % 8)) & 1) continue;
        const uint8_t p = k.pwhy[j], ky = j < sg.kwhy.size() ? sg.kwhy[j] : (uint8_t)WHY_NONE, sv = sig_why[k.g0 + j];
        status_[i] = p >= WHY_PROOF_FIRST && p < WHY_KEY ? p : ky == WHY_KEY ? ky : sv == WHY_SIGNATURE ? sv : (uint8_t)WHY_NONE;
      }
    }
  }
  void report() const {
    if (!timing_) return;
    fprintf(stderr, "tx verify: %zu transactions in %zu chunks: staging thread: keys pass %.2f ms, VM + ids %.2f ms, gather %.2f ms, signature "
                    "transcripts %.2f ms (%zu stages); calling thread: idle %.2f ms, queueing keys %.2f, proofs %.2f, signatures %.2f ms, "
                    "waiting for the device %.2f ms; %.2f ms in all\n",
            batch_, chunks_.size(), t_keys_host_ * 1e3, t_vm_ * 1e3, t_stage_host_ * 1e3, t_sig_host_ * 1e3, sig_stages_.size(), t_wait_host_ * 1e3,
            t_keys_ * 1e3, t_stage_ * 1e3, t_sigs_ * 1e3, t_wait_ * 1e3, (now() - t00_) * 1e3);
  }

  std::vector<uint8_t> seen_pdone_;
  TxDevice& dev_;
  std::vector<TxStatement>& store_;
  std::vector<TxStatement> beyond_;
  const size_t batch_;
  std::vector<const uint8_t*> ptr_;                      // where every transaction of the call lies, and how long it is
  std::vector<size_t> len_;
  const int threads_;
  uint8_t* const accept_;
  uint8_t* const status_;
  const TxFormat fmt_;                                   // the mode of the call: the device's format, read once (tx_out.hpp says what each predicate means)
  const bool reasons_;                                   // the format brings back reason bytes, and there is a status array to write them to
  const bool ids_;                                       // the IDs of accepted transactions go out (the device says so, and a piece has room for them)
  std::vector<uint8_t*> id_out_;                         // ... per transaction of the call, where its 32 bytes go (NULL: its caller has no room)
  const size_t log_k_;                                   // the log's entries go out too, at most so many per transaction (0: no)
  std::vector<std::pair<uint8_t*, size_t>> log_out_;     // ... per transaction, where its record goes (NULL: no room) and its caller's window
  std::vector<uint8_t> log_rec_;                         // ... the records of the whole call, window log_k_, until verdicts() hands them out
  std::vector<uint32_t> log_table_;                      // (calling thread: the shape table of the tape being collected)
  const bool root_;                                      // the roots of pieces that kept every transaction go out too (only beside ids_)
  std::vector<uint8_t*> root_out_;                       // ... per asking piece, where its 32 bytes go,
  std::vector<uint64_t> root_ranges_;                    // ... and (first transaction of the call, transactions) of it
  std::vector<uint8_t> root_dev_;                        // ... what a device that hashes brought down, 32 bytes per asking piece
  std::vector<char> handed_;                             // ... per transaction: verdicts() handed its ID out
  bool root_pending_ = false;                            // (calling thread) the folds are queued and not yet collected, in
  int root_slot_ = 0;                                    // ... this slot
  const bool timing_;
  const double t00_;
  const size_t n_slots_;                                 // key / signature stages in flight at once (2; 1 when two calls share the stage contexts)
  std::function<void()> on_news_;
  // the plan
  std::vector<std::unique_ptr<Chunk>> chunks_;
  std::vector<Segment> seg_;                             // one key stage per chunk
  std::vector<Span> runs_, sig_plan_;                    // runs of chunks (the staging thread's unit of work); the signature stages
  bool proofs_first_ = false;
  // ---- what the two threads share (under hm_).  key_rows_[c]: the rows of chunk c are made; keys_arrived_[c]: the calling
  // thread has its encodings back; staged_[c]: chunk c has been through the VM and its statements are staged in ring slot
  // c % RING; arena_free_[c]: its proofs have been collected (the slot may be reused); sig_stages_[0 .. n_sig_stages_): the
  // signature stages made so far; all_sigs_made_; quit_; stager_failed_
  std::mutex hm_;
  std::condition_variable hcv_;
  std::vector<char> staged_, arena_free_, key_rows_, keys_arrived_;
  // (a device that hashes) tape_ready_[c]: the staging thread has finished chunk c's tape; ids_upto_: chunks whose transaction
  // IDs are in the statements (without such a device: = hashed_upto_); tape_failed_: a plan the tape cannot hold
  std::vector<char> tape_ready_, chain_rows_;            // | (a device that chains) chunk c's signature rows are made
  size_t ids_upto_ = 0;
  bool tape_failed_ = false;
  std::vector<std::unique_ptr<SigStage>> sig_stages_;
  size_t n_sig_stages_ = 0, sig_next_ = 0, hashed_upto_ = 0, n_host_hashed_ = 0, n_precomputed_ = 0;
  bool all_sigs_made_ = false, quit_ = false, stager_failed_ = false;
  double t_keys_host_ = 0, t_sig_host_ = 0, t_stage_host_ = 0, t_vm_ = 0;
  // written by the staging thread BEFORE the flag that publishes them (key_rows_ / staged_ / n_sig_stages_), read by the
  // calling thread after it: live_all_, agg_ (the calling thread writes a segment's part before keys_arrived_), key_ok_
  std::vector<size_t> live_all_;
  std::vector<uint8_t> agg_, key_ok_;
  std::thread stager_;
  // calling thread only
  size_t next_key_ = 0, next_kcollect_ = 0, next_stage_ = 0, next_sig_ = 0, next_hash_ = 0, next_hcollect_ = 0;
  size_t next_chain_ = 0;                                // (a device that chains) chunks whose chain has been collected
  std::vector<char> hash_pending_;
  std::vector<uint8_t> hash_ids_;
  bool finished_ = false;
  int rc_ = OK;
  std::string error_;
  double t_keys_ = 0, t_stage_ = 0, t_sigs_ = 0, t_wait_ = 0, t_wait_host_ = 0;
};

}  // namespace zkvm
}  // namespace zk
