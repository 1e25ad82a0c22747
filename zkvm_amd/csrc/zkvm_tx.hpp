// zkvm_tx.hpp -- the caller's side of the hot path (second half): a serialized ZkVM
// transaction -> what `Tx::verify` / `Verifier::verify_tx` hands to the proof system: the transaction ID, the keys the
// transaction signature must cover, and the statement + proof of its `cloak`.  Host code, as upstream's VM is.
//
// UNPINNED RECOLLECTION.  /root/reference holds no source and no specification: the wire format, the
// opcodes, the labels and the hashing below restate what the survey's appendix and the public ZkVM design notes
// describe, as far as they could be recalled; they are self-consistent across this file and the oracle
// (oracle/zkvm_tx.c, written separately) and NOT checkable against upstream here.  DESIGN.md sec 4.5 is the normative
// description of what this subset is; everything outside it is reported as "unsupported", never as "invalid".
//
//   Tx       := version:u64 | mintime_ms:u64 | maxtime_ms:u64 | n:u32 program[n] | R:32 s:32 | n:u32 proof[n]
//   program  := instruction*          (subset: a payment)
//       0x00 push:n:x   0x02 drop   0x03 dup:k   0x04 roll:k   0x06 var   0x18 cloak:m:n
//       0x1b input      0x1c output:k            0x20 signtx           (immediates: u32 little-endian)
//   Contract := anchor:32 | predicate:32 | k:u32 | item*      item := 0x00 n:u32 bytes[n]  |  0x02 qty:32 flavor:32
#pragma once
#include "merlin.hpp"
#include "merlin_x8.hpp"
#include "scalar.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace zk {
namespace zkvm {

enum TxStatus : uint8_t { TX_OK = 0, TX_INVALID = 1, TX_UNSUPPORTED = 2 };

// Bytes with inline room for the common case (a payment's four values, its few keys) and a heap fallback beyond: the
// statements of a chunk are then ONE allocation of the calling thread, instead of three small ones per transaction made
// on the worker threads and freed on the caller's (cross-thread frees: 2.5 ms of an 8192-transaction call).
template <size_t N>
class SmallBytes {
 public:
  SmallBytes() = default;
  SmallBytes(const SmallBytes& o) { assign(o.data(), o.size()); }
  SmallBytes& operator=(const SmallBytes& o) { if (this != &o) assign(o.data(), o.size()); return *this; }
  SmallBytes(SmallBytes&& o) noexcept : n_(o.n_), heap_(std::move(o.heap_)) { if (heap_.empty() && n_) std::memcpy(inl_, o.inl_, n_); o.n_ = 0; }
  SmallBytes& operator=(SmallBytes&& o) noexcept {
    if (this != &o) { n_ = o.n_; heap_ = std::move(o.heap_); if (heap_.empty() && n_) std::memcpy(inl_, o.inl_, n_); o.n_ = 0; }
    return *this;
  }
  void resize(size_t n) {                       // contents beyond the old size are zero
    if (n <= N && heap_.empty()) { if (n > n_) std::memset(inl_ + n_, 0, n - n_); n_ = n; return; }
    if (heap_.empty()) { heap_.assign(inl_, inl_ + n_); }
    heap_.resize(n, 0);
    n_ = n;
  }
  void assign(const uint8_t* p, size_t n) { heap_.clear(); n_ = 0; resize(n); if (n) std::memcpy(data(), p, n); }
  size_t size() const { return n_; }
  bool empty() const { return n_ == 0; }
  uint8_t* data() { return heap_.empty() ? inl_ : heap_.data(); }
  const uint8_t* data() const { return heap_.empty() ? inl_ : heap_.data(); }
  uint8_t& operator[](size_t i) { return data()[i]; }
  const uint8_t& operator[](size_t i) const { return data()[i]; }

 private:
  size_t n_ = 0;
  uint8_t inl_[N];
  std::vector<uint8_t> heap_;
};

struct TxStatement {
  TxStatus status = TX_INVALID;
  const char* why = "";
  uint64_t version = 0, mintime = 0, maxtime = 0;
  uint8_t txid[32] = {0};
  // the one cloak of the transaction: m inputs, n outputs, 64 bytes (qty, flavor commitments) per value, inputs first
  uint32_t n_in = 0, n_out = 0;
  SmallBytes<256> commitments;
  const uint8_t* proof = nullptr;
  size_t proof_len = 0;
  // the signature check  s B - R - sum_i (c a_i) X_i == identity  as terms of a multiscalar multiplication
  SmallBytes<160> sig_scalars, sig_points;        // 32 bytes each, same count
};

// A stack item REFERS to its bytes -- inside the transaction (pushed strings, and the contracts and payloads parsed out of
// them) or inside the statement's commitment buffer (the values a cloak leaves) -- and owns nothing: the VM of a payment
// moves a few dozen items around, and with owning items it spent a third of its time in the allocator.
struct Item {
  enum Kind : uint8_t { Data, Variable, Value, Contract } kind = Data;
  const uint8_t* p = nullptr;          // Data: the string; Variable: 32-byte commitment; Value: qty | flavor; Contract: its serialization
  size_t n = 0;
};

inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint64_t rd64(const uint8_t* p) { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }

// ---- hashing as a PLAN ------------------------------------------------------------------------------------------------
// The VM below does not hash while it runs: it writes down WHAT is to be hashed -- a list of Merlin transcripts ("jobs":
// contract ids, anchors, the leaves and nodes of the transaction-ID Merkle tree, the MuSig coefficients), each a list of
// messages given as pieces (bytes of the transaction, bytes of the statement's commitment buffer, small immediates, or
// the 32-byte result of an earlier job: a "slot") -- and the plan is executed afterwards: one transaction at a time
// (run_plan), or EIGHT transactions of the same plan shape in lockstep on AVX-512 (run_plans_x8, merlin_x8.hpp).  Every
// hash starts from a copy of its label's freshly initialised transcript (two Keccak-f saved per hash).
enum Proto : uint8_t { P_CONTRACTID = 0, P_RATCHET, P_TXID, P_MUSIG, P_SIGNTX, N_PROTO };
enum Label : uint8_t { L_CONT = 0 /* more bytes of the message in progress */, L_contract, L_id, L_old, L_new, L_tx_version, L_tx_mintime,
                       L_tx_maxtime, L_merkle_leaf, L_input, L_output, L_L, L_R, L_merkle_node, L_merkle_empty, L_n, L_X, L_i, L_a_i,
                       L_txid, L_dom_sep, L_c, N_LABEL };
inline const char* label_text(uint8_t l) {
  static const char* const t[N_LABEL] = {"", "contract", "id", "old", "new", "tx.version", "tx.mintime", "tx.maxtime", "merkle.leaf", "input",
                                         "output", "L", "R", "merkle.node", "merkle.empty", "n", "X", "i", "a_i", "txid", "dom-sep", "c"};
  return t[l];
}
inline const Transcript& proto_transcript(uint8_t p) {
  static const Transcript t[N_PROTO] = {Transcript("ZkVM.contractid"), Transcript("ZkVM.ratchet-anchor"), Transcript("ZkVM.txid"),
                                        Transcript("Musig.aggregated-key"), Transcript("ZkVM.signtx")};
  return t[p];
}

struct HashPiece {
  enum Kind : uint8_t { Bytes = 0, Slot = 1, Imm = 2 };
  uint8_t label = L_CONT;        // != L_CONT: this piece opens a message of msg_len bytes in all
  uint8_t kind = Bytes;
  uint32_t slot = 0;             // Slot: which (32 bits: the number of hash jobs of a transaction is bounded by its length alone)
  uint32_t len = 0, msg_len = 0;
  uint32_t off = 0;              // Imm: offset into the plan's immediate pool
  const uint8_t* p = nullptr;    // Bytes: where
};
struct HashJob { uint8_t proto, chal_label, out_len; uint32_t out_slot; uint32_t first, count; };
struct TxPlan {
  std::vector<HashJob> jobs;
  std::vector<HashPiece> pieces;
  std::vector<uint8_t> imm;
  std::vector<uint32_t> shape;   // everything that must agree for two plans to run in lockstep (no pointers, no contents)
  uint32_t n_slots = 0;
  // only != 0xff: the plan keeps the jobs of that protocol alone -- whatever else the VM asks to be hashed is dropped as it
  // is written down (its slot numbers read 0 and are used by dropped jobs only): the keys-first pass of a call
  uint8_t only = 0xff;
  bool dropping = false;
  void clear() { jobs.clear(); pieces.clear(); imm.clear(); shape.clear(); n_slots = 0; dropping = false; }
  void begin(uint8_t proto) {
    dropping = only != 0xff && proto != only;
    if (dropping) return;
    jobs.push_back(HashJob{proto, 0, 0, 0, (uint32_t)pieces.size(), 0}); shape.push_back(0x4a000000u | proto);
  }
  void piece(uint8_t label, uint8_t kind, const uint8_t* p, uint32_t len, uint32_t msg_len, uint32_t slot = 0, uint32_t off = 0) {
    if (dropping) return;
    HashPiece h; h.label = label; h.kind = kind; h.p = p; h.len = len; h.msg_len = msg_len; h.slot = slot; h.off = off;
    pieces.push_back(h);
    shape.push_back(((uint32_t)label << 24) | ((uint32_t)kind << 16));
    shape.push_back(slot);
    shape.push_back(len);
    shape.push_back(msg_len);
  }
  void bytes(uint8_t label, const uint8_t* p, uint32_t len, uint32_t msg_len) { piece(label, HashPiece::Bytes, p, len, msg_len); }
  void slot(uint8_t label, uint32_t s, uint32_t msg_len = 32) { piece(label, HashPiece::Slot, nullptr, 32, msg_len, s); }
  void immediate(uint8_t label, const uint8_t* b, uint32_t len, uint32_t msg_len) {
    if (dropping) return;
    const uint32_t off = (uint32_t)imm.size();
    imm.insert(imm.end(), b, b + len);
    piece(label, HashPiece::Imm, nullptr, len, msg_len, 0, off);
  }
  void u64(uint8_t label, uint64_t x) {
    uint8_t b[8];
    for (int i = 0; i < 8; ++i) b[i] = (uint8_t)(x >> (8 * i));
    immediate(label, b, 8, 8);
  }
  // closes the job: its challenge (32 bytes, or 64 bytes reduced to a canonical scalar) goes to a new slot
  uint32_t end(uint8_t chal_label, uint8_t out_len) {
    if (dropping) { dropping = false; return 0; }
    HashJob& j = jobs.back();
    j.chal_label = chal_label; j.out_len = out_len; j.out_slot = n_slots++;
    j.count = (uint32_t)pieces.size() - j.first;
    shape.push_back(0x4b000000u | ((uint32_t)chal_label << 8) | out_len);
    return j.out_slot;
  }
  bool same_shape(const TxPlan& o) const { return shape.size() == o.shape.size() && (shape.empty() || std::memcmp(shape.data(), o.shape.data(), 4 * shape.size()) == 0); }
};

inline const uint8_t* piece_bytes(const TxPlan& P, const HashPiece& h, const uint8_t* slots) {
  return h.kind == HashPiece::Bytes ? h.p : h.kind == HashPiece::Slot ? slots + 32 * (size_t)h.slot : P.imm.data() + h.off;
}

// slots: 32 bytes per slot.  One transaction.  only != ALL_PROTOS: just the jobs of that protocol (they must not read slots
// of the others: true of P_MUSIG, whose inputs are keys and counters).
constexpr uint8_t ALL_PROTOS = 0xff;
constexpr uint8_t NO_PROTO = 0xfe, ID_PROTOS = 0xfd;     // (as `only`: no job at all -- the VM's stack machine alone | run_plan alone: every job but P_MUSIG's, what the transaction ID and the log need)
inline void run_plan(const TxPlan& P, uint8_t* slots, uint8_t only = ALL_PROTOS) {
  static thread_local std::vector<uint8_t> msg;
  for (const HashJob& j : P.jobs) {
    if (only != ALL_PROTOS && j.proto != only && !(only == ID_PROTOS && j.proto < P_MUSIG)) continue;
    Transcript t = proto_transcript(j.proto);
    for (uint32_t q = j.first; q < j.first + j.count;) {
      const HashPiece& h = P.pieces[q];
      if (h.len == h.msg_len) { t.append_message(label_text(h.label), piece_bytes(P, h, slots), h.len); ++q; continue; }
      msg.clear();                                        // a message in several pieces: assembled first
      uint32_t q2 = q;
      do { const HashPiece& g = P.pieces[q2]; const uint8_t* b = piece_bytes(P, g, slots); msg.insert(msg.end(), b, b + g.len); ++q2; }
      while (q2 < j.first + j.count && P.pieces[q2].label == L_CONT);
      t.append_message(label_text(h.label), msg.data(), msg.size());
      q = q2;
    }
    uint8_t out[64];
    t.challenge_bytes(label_text(j.chal_label), out, j.out_len);
    if (j.out_len == 64) Scalar::from_wide(out).to_bytes(slots + 32 * (size_t)j.out_slot);
    else std::memcpy(slots + 32 * (size_t)j.out_slot, out, 32);
  }
}

#if ZK_HAVE_X8
// Eight plans of one shape in lockstep (lanes may repeat a plan: padding).  slots[l]: lane l's slot memory.
ZK_X8 inline void run_plans_x8(const TxPlan* const P[8], uint8_t* const slots[8], uint8_t only = ALL_PROTOS) {
  const TxPlan& P0 = *P[0];
  for (size_t ji = 0; ji < P0.jobs.size(); ++ji) {
    const HashJob& j = P0.jobs[ji];
    if (only != ALL_PROTOS && j.proto != only && !(only == ID_PROTOS && j.proto < P_MUSIG)) continue;
    TranscriptX8 t(proto_transcript(j.proto));
    for (uint32_t q = j.first; q < j.first + j.count; ++q) {
      const HashPiece& h = P0.pieces[q];
      if (h.label != L_CONT) t.begin_message(label_text(h.label), h.msg_len);
      const uint8_t* d[8];
      for (int l = 0; l < 8; ++l) d[l] = piece_bytes(*P[l], P[l]->pieces[q], slots[l]);
      t.data(d, h.len);
    }
    uint8_t wide[8][64];
    uint8_t* out[8];
    for (int l = 0; l < 8; ++l) out[l] = j.out_len == 64 ? wide[l] : slots[l] + 32 * (size_t)j.out_slot;
    t.challenge(label_text(j.chal_label), out, j.out_len);
    if (j.out_len == 64)
      for (int l = 0; l < 8; ++l) Scalar::from_wide(wide[l]).to_bytes(slots[l] + 32 * (size_t)j.out_slot);
  }
}
#endif

// Merkle root over the log entries (RFC 6962 split: the largest power of two below the count goes left), every hash a
// Merlin transcript: leaf = entry's own messages then "merkle.leaf"; node = "L", "R" then "merkle.node".  -> slot of the root
struct LogEntry {
  enum Kind : uint8_t { Header, Input, Output } kind;
  uint64_t a = 0, b = 0, c = 0;
  uint32_t id_slot = 0;
};
inline uint32_t plan_merkle(TxPlan& P, const LogEntry* e, size_t n) {
  if (n == 0) { P.begin(P_TXID); return P.end(L_merkle_empty, 32); }
  if (n == 1) {
    P.begin(P_TXID);
    switch (e->kind) {
      case LogEntry::Header: P.u64(L_tx_version, e->a); P.u64(L_tx_mintime, e->b); P.u64(L_tx_maxtime, e->c); break;
      case LogEntry::Input: P.slot(L_input, e->id_slot); break;
      case LogEntry::Output: P.slot(L_output, e->id_slot); break;
    }
    return P.end(L_merkle_leaf, 32);
  }
  size_t k = 1;
  while (2 * k < n) k *= 2;
  const uint32_t l = plan_merkle(P, e, k), r = plan_merkle(P, e + k, n - k);
  P.begin(P_TXID);
  P.slot(L_L, l);
  P.slot(L_R, r);
  return P.end(L_merkle_node, 32);
}

// parses a serialized contract; false: malformed.  items (Data or Value) refer into `p`
inline bool parse_contract(const uint8_t* p, size_t n, const uint8_t*& predicate, std::vector<Item>* items, bool& unsupported) {
  if (n < 68) return false;
  predicate = p + 32;
  const uint32_t k = rd32(p + 64);
  size_t pos = 68;
  for (uint32_t i = 0; i < k; ++i) {
    if (pos >= n) return false;
    const uint8_t type = p[pos++];
    Item it;
    if (type == 0x00) {
      if (n - pos < 4) return false;
      const uint32_t len = rd32(p + pos);
      pos += 4;
      if (n - pos < len) return false;
      it.kind = Item::Data;
      it.p = p + pos; it.n = len;
      pos += len;
    } else if (type == 0x02) {
      if (n - pos < 64) return false;
      it.kind = Item::Value;
      it.p = p + pos; it.n = 64;
      pos += 64;
    } else if (type == 0x01) {
      unsupported = true;      // a program item: outside the subset
      return false;
    } else {
      return false;
    }
    if (items) items->push_back(it);
  }
  return pos == n;
}

// First half: parse, VM, and the PLAN of everything there is to hash (nothing is hashed yet).  The statement refers into
// `tx` (proof bytes), the plan into `tx` and into st.commitments: neither may move until the plan has run.
// txid_slot / a_slots: where the transaction ID and the MuSig coefficients will be found.
struct TxSlots { uint32_t txid = 0; std::vector<uint32_t> a; std::vector<const uint8_t*> keys; const uint8_t* sig = nullptr; };
inline void tx_structure(const uint8_t* tx, size_t len, TxStatement& st, TxPlan& P, TxSlots& out) {
  st.status = TX_INVALID; st.why = ""; st.n_in = st.n_out = 0; st.proof = nullptr; st.proof_len = 0;      // (field by field: the
  st.commitments.resize(0); st.sig_scalars.resize(0); st.sig_points.resize(0);                             //  inline buffers stay as they are)
  P.clear();
  out.a.clear(); out.keys.clear();
  auto fail = [&st](TxStatus s, const char* why) { st.status = s; st.why = why; };
  if (len < 24 + 4) { fail(TX_INVALID, "truncated header"); return; }
  st.version = rd64(tx); st.mintime = rd64(tx + 8); st.maxtime = rd64(tx + 16);
  size_t pos = 24;
  const uint32_t prog_len = rd32(tx + pos);
  pos += 4;
  if (len - pos < prog_len) { fail(TX_INVALID, "truncated program"); return; }
  const uint8_t* prog = tx + pos;
  pos += prog_len;
  if (len - pos < 64 + 4) { fail(TX_INVALID, "truncated signature"); return; }
  const uint8_t* sig = tx + pos;
  pos += 64;
  const uint32_t proof_len = rd32(tx + pos);
  pos += 4;
  if (len - pos != proof_len) { fail(TX_INVALID, "proof length does not match the transaction's"); return; }
  st.proof = tx + pos;
  st.proof_len = proof_len;
  if (st.version != 1) { fail(TX_UNSUPPORTED, "transaction version"); return; }
  if (st.mintime > st.maxtime) { fail(TX_INVALID, "mintime after maxtime"); return; }

  // scratch of the calling thread, reused from transaction to transaction
  static thread_local std::vector<Item> stack, payload;
  static thread_local std::vector<LogEntry> log;
  std::vector<const uint8_t*>& keys = out.keys;
  stack.clear(); log.clear();
  LogEntry hdr; hdr.kind = LogEntry::Header; hdr.a = st.version; hdr.b = st.mintime; hdr.c = st.maxtime;
  log.push_back(hdr);
  bool have_anchor = false, cloaked = false;
  uint32_t last_anchor = 0;              // slot
  size_t pc = 0;
  auto imm32 = [&](uint32_t& v) { if (prog_len - pc < 4) return false; v = rd32(prog + pc); pc += 4; return true; };
  while (pc < prog_len) {
    const uint8_t op = prog[pc++];
    switch (op) {
      case 0x00: {   // push:n:x
        uint32_t n;
        if (!imm32(n) || prog_len - pc < n) { fail(TX_INVALID, "push runs past the program"); return; }
        Item it; it.kind = Item::Data; it.p = prog + pc; it.n = n;
        pc += n;
        stack.push_back(it);
        break;
      }
      case 0x02:     // drop
        if (stack.empty()) { fail(TX_INVALID, "stack underflow"); return; }
        if (stack.back().kind == Item::Value || stack.back().kind == Item::Contract) { fail(TX_INVALID, "drop of a value or a contract"); return; }
        stack.pop_back();
        break;
      case 0x03: {   // dup:k
        uint32_t k;
        if (!imm32(k) || k >= stack.size()) { fail(TX_INVALID, "dup out of range"); return; }
        const Item src = stack[stack.size() - 1 - k];
        if (src.kind == Item::Value || src.kind == Item::Contract) { fail(TX_INVALID, "dup of a value or a contract"); return; }
        stack.push_back(src);
        break;
      }
      case 0x04: {   // roll:k
        uint32_t k;
        if (!imm32(k) || k >= stack.size()) { fail(TX_INVALID, "roll out of range"); return; }
        const Item it = stack[stack.size() - 1 - k];
        stack.erase(stack.end() - 1 - k);
        stack.push_back(it);
        break;
      }
      case 0x06: {   // var
        if (stack.empty() || stack.back().kind != Item::Data || stack.back().n != 32) { fail(TX_INVALID, "var needs a 32-byte commitment"); return; }
        stack.back().kind = Item::Variable;
        break;
      }
      case 0x18: {   // cloak:m:n
        uint32_t m, n;
        if (!imm32(m) || !imm32(n)) { fail(TX_INVALID, "cloak immediates"); return; }
        if (cloaked) { fail(TX_UNSUPPORTED, "more than one cloak per transaction"); return; }
        if (m == 0 || n == 0 || m > 64 || n > 64) { fail(TX_UNSUPPORTED, "cloak arity"); return; }
        if (stack.size() < (size_t)m + 2 * (size_t)n) { fail(TX_INVALID, "stack underflow"); return; }
        st.commitments.resize(64 * ((size_t)m + n));      // inputs, then outputs (the values pushed below refer into it)
        uint8_t* ins = st.commitments.data();
        uint8_t* outs = ins + 64 * (size_t)m;
        for (uint32_t j = n; j-- > 0;) {     // .. q_j f_j on top
          for (int half = 1; half >= 0; --half) {
            if (stack.back().kind != Item::Variable) { fail(TX_INVALID, "cloak outputs must be variables"); return; }
            std::memcpy(&outs[64 * j + 32 * half], stack.back().p, 32);
            stack.pop_back();
          }
        }
        for (uint32_t i = m; i-- > 0;) {
          if (stack.back().kind != Item::Value) { fail(TX_INVALID, "cloak inputs must be values"); return; }
          std::memcpy(&ins[64 * i], stack.back().p, 64);
          stack.pop_back();
        }
        st.n_in = m; st.n_out = n;
        for (uint32_t j = 0; j < n; ++j) { Item v; v.kind = Item::Value; v.p = &outs[64 * j]; v.n = 64; stack.push_back(v); }
        cloaked = true;
        break;
      }
      case 0x1b: {   // input
        if (stack.empty() || stack.back().kind != Item::Data) { fail(TX_INVALID, "input needs a serialized contract"); return; }
        const uint8_t* pred;
        bool unsupported = false;
        const Item c_ser = stack.back();
        stack.pop_back();
        if (!parse_contract(c_ser.p, c_ser.n, pred, nullptr, unsupported))
          { fail(unsupported ? TX_UNSUPPORTED : TX_INVALID, "malformed contract"); return; }
        LogEntry e; e.kind = LogEntry::Input;
        P.begin(P_CONTRACTID);
        P.bytes(L_contract, c_ser.p, (uint32_t)c_ser.n, (uint32_t)c_ser.n);
        e.id_slot = P.end(L_id, 32);
        log.push_back(e);
        last_anchor = e.id_slot;
        have_anchor = true;
        Item c = c_ser; c.kind = Item::Contract;
        stack.push_back(c);
        break;
      }
      case 0x1c: {   // output:k
        uint32_t k;
        if (!imm32(k)) { fail(TX_INVALID, "output immediate"); return; }
        if (stack.size() < (size_t)k + 1) { fail(TX_INVALID, "stack underflow"); return; }
        if (stack.back().kind != Item::Data || stack.back().n != 32) { fail(TX_INVALID, "output needs a 32-byte predicate"); return; }
        if (!have_anchor) { fail(TX_INVALID, "output before any input: no anchor"); return; }
        const uint8_t* pred = stack.back().p;
        stack.pop_back();
        const Item* items = stack.data() + (stack.size() - k);
        for (uint32_t q = 0; q < k; ++q) if (items[q].kind != Item::Data && items[q].kind != Item::Value) { fail(TX_INVALID, "output payload must be data or values"); return; }
        P.begin(P_RATCHET);
        P.slot(L_old, last_anchor);
        last_anchor = P.end(L_new, 32);
        // the new contract, serialized as the message "contract": anchor | predicate | k | items
        uint32_t ser_len = 68;
        for (uint32_t q = 0; q < k; ++q) ser_len += items[q].kind == Item::Value ? 1 + 64 : 1 + 4 + (uint32_t)items[q].n;
        P.begin(P_CONTRACTID);
        P.slot(L_contract, last_anchor, ser_len);
        P.bytes(L_CONT, pred, 32, ser_len);
        { const uint8_t kb[4] = {(uint8_t)k, (uint8_t)(k >> 8), (uint8_t)(k >> 16), (uint8_t)(k >> 24)}; P.immediate(L_CONT, kb, 4, ser_len); }
        for (uint32_t q = 0; q < k; ++q) {
          const Item& it = items[q];
          if (it.kind == Item::Value) {
            const uint8_t ty = 0x02;
            P.immediate(L_CONT, &ty, 1, ser_len);
          } else {
            const uint32_t n = (uint32_t)it.n;
            const uint8_t hd[5] = {0x00, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24)};
            P.immediate(L_CONT, hd, 5, ser_len);
          }
          if (it.n) P.bytes(L_CONT, it.p, (uint32_t)it.n, ser_len);
        }
        stack.resize(stack.size() - k);
        LogEntry e; e.kind = LogEntry::Output;
        e.id_slot = P.end(L_id, 32);
        log.push_back(e);
        break;
      }
      case 0x20: {   // signtx
        if (stack.empty() || stack.back().kind != Item::Contract) { fail(TX_INVALID, "signtx needs a contract"); return; }
        const uint8_t* pred;
        bool unsupported = false;
        const Item c_ser = stack.back();
        stack.pop_back();
        payload.clear();
        if (!parse_contract(c_ser.p, c_ser.n, pred, &payload, unsupported)) { fail(TX_INVALID, "malformed contract"); return; }
        keys.push_back(pred);
        for (const Item& it : payload) stack.push_back(it);
        break;
      }
      default:
        { fail(TX_UNSUPPORTED, "instruction outside the payment subset"); return; }
    }
  }
  if (!stack.empty()) { fail(TX_INVALID, "stack not empty at the end"); return; }
  if (!cloaked) { fail(TX_UNSUPPORTED, "no cloak: nothing for the proof system"); return; }
  if (keys.empty()) { fail(TX_INVALID, "no key signs the transaction"); return; }
  out.txid = plan_merkle(P, log.data(), log.size());

  // signature: X = sum a_i X_i (MuSig key aggregation), c = H(txid, X, R);  s B == R + c X
  Scalar s;
  if (!Scalar::from_canonical(sig + 32, s)) { fail(TX_INVALID, "signature scalar not canonical"); return; }
  // a_i = H("Musig.aggregated-key": n, X_0 .. X_{n-1}, then i): one transcript per key (the common prefix is absorbed again:
  // a permutation at most for a handful of keys)
  for (size_t i = 0; i < keys.size(); ++i) {
    P.begin(P_MUSIG);
    P.u64(L_n, keys.size());
    for (const uint8_t* k : keys) P.bytes(L_X, k, 32, 32);
    P.u64(L_i, i);
    out.a.push_back(P.end(L_a_i, 64));
  }
  out.sig = sig;
  st.sig_scalars.resize(32 * (2 + keys.size()));
  st.sig_points.resize(32 * (2 + keys.size()));
  st.status = TX_OK;
  // terms: [0] B (filled by the caller: scalar s), [1] R (scalar -1), [2 + i] X_i (scalar a_i for now -- tx_finish_hashes --,
  // -c a_i once tx_finish_signature knows the aggregated key)
  s.to_bytes(&st.sig_scalars[0]);
  (-Scalar::one()).to_bytes(&st.sig_scalars[32]);
  std::memcpy(&st.sig_points[32], sig, 32);
  for (size_t i = 0; i < keys.size(); ++i) std::memcpy(&st.sig_points[32 * (2 + i)], keys[i], 32);
}

// after the plan has run: the transaction ID and the MuSig coefficients move from the slots into the statement
// MEASUREMENT BUILDS ONLY (-DZK_MEASURE_FREE_HASHING, tools/build_variant.sh; like ZK_PREP_STAMPS): every Merlin hash of the
// host side -- contract ids, anchors, the transaction-ID tree, the MuSig factors, the signature challenge -- is SKIPPED (slots
// read zero, c = 1) when ZKGPU_TEST_TX_FREE_HASHING=1.  Verdicts are then wrong; the device does the same work.  It bounds from
// above what replaying the hash plans on the device could give.  The shipped library has no such branch: nothing in the
// environment can make it skip a hash (a verification bypass must not be one variable away).
#ifdef ZK_MEASURE_FREE_HASHING
inline bool tx_free_hashing_hook() {
  static const bool on = [] {
    const char* f = std::getenv("ZKGPU_TEST_TX_FREE_HASHING");
    return f && f[0] == '1';
  }();
  return on;
}
#else
constexpr bool tx_free_hashing_hook() { return false; }
#endif

inline void tx_finish_hashes(TxStatement& st, const TxSlots& out, const uint8_t* slots) {
  std::memcpy(st.txid, slots + 32 * (size_t)out.txid, 32);
  for (size_t i = 0; i < out.a.size(); ++i) std::memcpy(&st.sig_scalars[32 * (2 + i)], slots + 32 * (size_t)out.a[i], 32);
}

// The second pass over a group of up to eight transactions, written down ONCE (the plain pass below, the taped one in
// tx_hash_tape.hpp and the logged one in tx_log.hpp are its parameters): the structure pass -- parse, VM, the plan with the
// jobs of plan_only kept (ALL_PROTOS: every job) --, the statements the VM accepted, their plans run on the host for the jobs of
// host_only, tx_finish_hashes, then after(i, plan, its TxSlots, its slot memory) per accepted statement i in order.  Plans of one
// shape (payments of the same arity and payload sizes, as a block mostly holds) are hashed in lockstep, eight Keccak states per
// AVX-512 register, idle lanes repeating the first; anything else -- other shapes side by side, fewer than three, a CPU without
// AVX-512, allow_x8 = false -- one at a time.  Same results.  zero_slots: the slot memory reads zero before the plans run (a
// caller that sees slots the host does not write); false: it holds whatever the thread's last group left there.
// In a -DZK_MEASURE_FREE_HASHING build with the hook on, whatever the host would have run here is skipped and every slot reads
// zero -- uniformly, whichever of the three passes asks.
struct TxGroupScratch { TxPlan plans[8]; TxSlots outs[8]; std::vector<uint8_t> slot_mem[8], spare[8]; };
inline TxGroupScratch& tx_group_scratch() { static thread_local TxGroupScratch w; return w; }
template <class After>
inline void tx_run_group(const uint8_t* const* tx, const size_t* len, TxStatement* st, size_t count, uint8_t plan_only, uint8_t host_only,
                         bool allow_x8, bool zero_slots, After after) {
  TxGroupScratch& w = tx_group_scratch();
  const bool skip = tx_free_hashing_hook();
  int live[8], n_live = 0;
  for (size_t i = 0; i < count && i < 8; ++i) {
    w.plans[i].only = plan_only;
    tx_structure(tx[i], len[i], st[i], w.plans[i], w.outs[i]);
    if (st[i].status != TX_OK) continue;
    const size_t bytes = 32 * (size_t)w.plans[i].n_slots + 32;
    if (zero_slots || skip) w.slot_mem[i].assign(bytes, 0); else w.slot_mem[i].resize(bytes);
    live[n_live++] = (int)i;
  }
  bool lockstep = false;
#if ZK_HAVE_X8
  lockstep = !skip && allow_x8 && n_live >= 3 && x8_available();
  for (int q = 1; lockstep && q < n_live; ++q) lockstep = w.plans[live[q]].same_shape(w.plans[live[0]]);
  if (lockstep) {
    const TxPlan* P[8];
    uint8_t* S[8];
    for (int l = 0; l < 8; ++l) {
      if (l < n_live) { P[l] = &w.plans[live[l]]; S[l] = w.slot_mem[live[l]].data(); }
      else { P[l] = &w.plans[live[0]]; w.spare[l].resize(w.slot_mem[live[0]].size()); S[l] = w.spare[l].data(); }     // padding: lane 0's work again
    }
    run_plans_x8(P, S, host_only);
  }
#endif
  for (int q = 0; q < n_live; ++q) {
    const int i = live[q];
    if (!lockstep && !skip) run_plan(w.plans[i], w.slot_mem[i].data(), host_only);
    tx_finish_hashes(st[i], w.outs[i], w.slot_mem[i].data());
    after((size_t)i, w.plans[i], w.outs[i], w.slot_mem[i].data());
  }
}

// Runs up to eight transactions: parse, VM, transaction ID, signature terms.
// only = P_MUSIG: the signature's key rows alone -- status, s, R, the keys X_i and their MuSig coefficients a_i are what the
// statement holds afterwards (no transaction ID yet: what tx_finish_hashes copied is not one): the first pass of
// zkgpu_tx_verify_batch, which wants the aggregated keys of a whole call on their way to the device before the rest of the
// hashing starts.
inline void tx_prepare_many(const uint8_t* const* tx, const size_t* len, TxStatement* st, size_t count, bool allow_x8 = true,
                            uint8_t only = ALL_PROTOS) {
  tx_run_group(tx, len, st, count, only, only, allow_x8, false, [](size_t, const TxPlan&, const TxSlots&, const uint8_t*) {});
}

inline TxStatement tx_prepare(const uint8_t* tx, size_t len) {
  TxStatement st;
  tx_prepare_many(&tx, &len, &st, 1);
  return st;
}

// second half of the signature preparation, once the aggregated key X = sum a_i X_i is known as an encoding
// (one small multiscalar multiplication per transaction: zkgpu_msm_batch on the device, host_rows in the CPU tests)
inline void tx_apply_challenge(TxStatement& st, const uint8_t basepoint[32], const Scalar& c) {
  std::memcpy(&st.sig_points[0], basepoint, 32);
  const size_t n_keys = st.sig_scalars.size() / 32 - 2;
  for (size_t i = 0; i < n_keys; ++i) {
    Scalar ai;
    Scalar::from_canonical(&st.sig_scalars[32 * (2 + i)], ai);
    (-(c * ai)).to_bytes(&st.sig_scalars[32 * (2 + i)]);
  }
}
template <class T = Transcript> inline void tx_finish_signature(TxStatement& st, const uint8_t basepoint[32], const uint8_t agg_key[32], T* tap = nullptr) {
  T t = tap ? *tap : T(proto_transcript(P_SIGNTX));      // (tap: tx_sig_rows.hpp writes down what is hashed here, for the device)
  t.append_message("txid", st.txid, 32);
  t.append_message("dom-sep", (const uint8_t*)"schnorr-signature v1", 20);
  t.append_point("X", agg_key);
  t.append_point("R", &st.sig_points[32]);
  tx_apply_challenge(st, basepoint, t.challenge_scalar("c"));
}
// the same for up to eight transactions (the transcript has one shape whatever the transaction: always in lockstep)
inline void tx_finish_signature_many(TxStatement* const* st, const uint8_t* const* agg_key, const uint8_t basepoint[32], size_t count) {
  if (tx_free_hashing_hook()) {                 // (measurement hook: c = 1)
    for (size_t l = 0; l < count; ++l) tx_apply_challenge(*st[l], basepoint, Scalar::from_u64(1));
    return;
  }
#if ZK_HAVE_X8
  if (count >= 3 && count <= 8 && x8_available()) {
    [&]() ZK_X8 {
      TranscriptX8 t(proto_transcript(P_SIGNTX));
      const uint8_t* d[8];
      auto lane = [&](int l) { return (size_t)l < count ? (size_t)l : 0; };
      t.begin_message("txid", 32);
      for (int l = 0; l < 8; ++l) d[l] = st[lane(l)]->txid;
      t.data(d, 32);
      t.begin_message("dom-sep", 20);
      t.data_same((const uint8_t*)"schnorr-signature v1", 20);
      t.begin_message("X", 32);
      for (int l = 0; l < 8; ++l) d[l] = agg_key[lane(l)];
      t.data(d, 32);
      t.begin_message("R", 32);
      for (int l = 0; l < 8; ++l) d[l] = &st[lane(l)]->sig_points[32];
      t.data(d, 32);
      uint8_t wide[8][64];
      uint8_t* out[8];
      for (int l = 0; l < 8; ++l) out[l] = wide[l];
      t.challenge("c", out, 64);
      for (size_t l = 0; l < count; ++l) tx_apply_challenge(*st[l], basepoint, Scalar::from_wide(wide[l]));
    }();
    return;
  }
#endif
  for (size_t l = 0; l < count; ++l) tx_finish_signature(*st[l], basepoint, agg_key[l]);
}

}  // namespace zkvm
}  // namespace zk
