// tx_hash_tape.hpp -- the hash plans of a chunk of transactions (zkvm_tx.hpp: TxPlan) flattened into ONE block of words a
// kernel can index blindly, and the interpreter that runs it: tx_hash_run, one function for the host and the device
// (tx_hash_kernels.hpp: k_tx_hash runs it one lane per transaction; the CPU tests and libzkhost run the same code).  The block
// read another way -- its jobs by dependency level, several lanes per transaction -- is tx_hash_levels.hpp's.
//
// With ZKGPU_TXFORMAT_HASH_ON_DEVICE the second pass of a transaction call (tx_call.hpp) writes the plans of its chunk but
// runs none of the jobs of P_CONTRACTID, P_RATCHET and P_TXID on the host: they come here.  P_MUSIG and P_SIGNTX stay on the
// host.  Every job kept draws a 32-byte challenge (checked when a plan is added: no 64-byte challenge is hashed here).
//
// The block (32-bit words; every section starts at a multiple of 16 bytes; offsets below are in WORDS from the start):
//   head      16 words  HashTapeHead
//   shapes    4 words per DISTINCT plan shape: first job, jobs, slots of a transaction, the root's slot
//   jobs      4 words: proto | challenge label << 8 | out_len << 16, out slot, first piece, pieces
//   pieces    4 words: label | kind << 8, len, msg_len, slot      (Bytes and Imm pieces are both "the next len bytes of the
//                                                                  transaction's run": kind TAPE_RUN; Slot pieces keep their slot)
//   lanes     1 word per lane: the transaction it runs, or TAPE_IDLE.  Transactions are ordered by shape and each shape's run
//             is padded to a multiple of 64 lanes with TAPE_IDLE, so that a wavefront runs ONE shape and its control flow is
//             uniform (the rule of mixed_plan.hpp's lane order)
//   txs       4 words per transaction: shape, byte offset of its run in `data`, first slot of its slot area, 0
//   data      the contents of every transaction's Bytes and Imm pieces back to back in piece order (a few hundred bytes per
//             payment): copied, so that the kernel knows neither the transaction blob nor the statements' commitment buffers
// Slot numbers are the plan's own (the slots of the jobs that stay on the host are simply never written), 32 bytes each.
// Beside the block, ONCE per verifier (hash_tape_constants): the freshly initialised transcripts of the protocols -- 50 state
// words, position, begin marker -- and the label table -- length byte + text, 16 bytes per label -- both computed from
// zkvm_tx.hpp's proto_transcript() / label_text(): no label is restated here.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include "merlin_dev.hpp"
#define ZK_TAPE_HD __host__ __device__
#else
#define ZK_TAPE_HD
#endif
#include "keccak.hpp"

namespace zk {
namespace zkvm {

constexpr uint32_t TAPE_MAGIC = 0x54485854u, TAPE_IDLE = 0xffffffffu;
constexpr uint32_t TAPE_RUN = 0, TAPE_SLOT = 1;                       // piece kinds on the tape
constexpr uint32_t TAPE_PROTO_WORDS = 52, TAPE_LABEL_BYTES = 16, TAPE_RATE = 166;
struct HashTapeHead {
  uint32_t magic, n_lanes, n_tx, n_shapes, shapes, jobs, pieces, lanes, txs, data, n_jobs, n_pieces, data_bytes, n_slots, words, zero;
};
static_assert(sizeof(HashTapeHead) == 64, "16 words");

// what the interpreter reads and writes: the block, the constants, the slot memory (32 bytes per slot), the dense IDs
struct HashTapeView {
  const uint32_t* tape;       // the block
  const uint32_t* protos;     // N_PROTO x TAPE_PROTO_WORDS
  const uint8_t* labels;      // N_LABEL x TAPE_LABEL_BYTES
  uint32_t* slots;            // head.n_slots x 8 words
  uint32_t* txid;             // head.n_tx x 8 words
};

// ---- STROBE-128 on a state of 50 words st[i * stride] (merlin.hpp: Strobe128, the AD / meta-AD / PRF subset) -------------
struct TapeStrobe { uint32_t* st; uint32_t stride, pos, pos_begin; };

ZK_TAPE_HD inline void tape_permute(TapeStrobe& s) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t lo[25], hi[25];
#pragma unroll
  for (int q = 0; q < 25; ++q) { lo[q] = s.st[(2 * q) * s.stride]; hi[q] = s.st[(2 * q + 1) * s.stride]; }
  keccak_f1600_halves(lo, hi);
#pragma unroll
  for (int q = 0; q < 25; ++q) { s.st[(2 * q) * s.stride] = lo[q]; s.st[(2 * q + 1) * s.stride] = hi[q]; }
#else
  uint64_t a[25];
  for (int q = 0; q < 25; ++q) a[q] = (uint64_t)s.st[(2 * q) * s.stride] | ((uint64_t)s.st[(2 * q + 1) * s.stride] << 32);
  keccak_f1600(a);
  for (int q = 0; q < 25; ++q) { s.st[(2 * q) * s.stride] = (uint32_t)a[q]; s.st[(2 * q + 1) * s.stride] = (uint32_t)(a[q] >> 32); }
#endif
}

ZK_TAPE_HD inline void tape_xor(TapeStrobe& s, uint32_t at, uint32_t byte) { s.st[(at >> 2) * s.stride] ^= byte << (8 * (at & 3)); }
ZK_TAPE_HD inline void tape_run_f(TapeStrobe& s) {
  tape_xor(s, s.pos, s.pos_begin);
  tape_xor(s, s.pos + 1, 0x04);
  tape_xor(s, TAPE_RATE + 1, 0x80);
  tape_permute(s);
  s.pos = 0; s.pos_begin = 0;
}
ZK_TAPE_HD inline void tape_absorb_byte(TapeStrobe& s, uint32_t b) {
  tape_xor(s, s.pos, b);
  if (++s.pos == TAPE_RATE) tape_run_f(s);
}
// `n` bytes that lie at p[0 .. n) in memory of 32-bit little-endian words starting at byte `at` of `base`
ZK_TAPE_HD inline void tape_absorb(TapeStrobe& s, const uint32_t* base, uint32_t at, uint32_t n) {
  for (uint32_t i = at; i < at + n; ++i) tape_absorb_byte(s, (base[i >> 2] >> (8 * (i & 3))) & 0xffu);
}
ZK_TAPE_HD inline void tape_begin_op(TapeStrobe& s, uint32_t flags) {        // (flags: merlin.hpp kI 1, kA 2, kC 4, kM 16)
  const uint32_t old = s.pos_begin;
  s.pos_begin = s.pos + 1;
  tape_absorb_byte(s, old);
  tape_absorb_byte(s, flags);
  if ((flags & 4u) && s.pos != 0) tape_run_f(s);
}
// meta-AD of a label of the table, then of a 32-bit length (continued): what opens Merlin's append_message / challenge_bytes
ZK_TAPE_HD inline void tape_label_len(TapeStrobe& s, const uint8_t* labels, uint32_t label, uint32_t len) {
  const uint8_t* t = labels + TAPE_LABEL_BYTES * label;
  tape_begin_op(s, 16u | 2u);
  for (uint32_t i = 0; i < t[0]; ++i) tape_absorb_byte(s, t[1 + i]);
  for (int i = 0; i < 4; ++i) tape_absorb_byte(s, (len >> (8 * i)) & 0xffu);
}

// The jobs of the transaction on `lane` (nothing for an idle lane), in order: every message streamed piece by piece with its
// length framed once from msg_len, the challenge written to the job's slot; the last job's is the root: also to txid.
// st: 50 words of scratch, word i at st[i * stride].  -> false: the lane is idle.
ZK_TAPE_HD inline bool tx_hash_run(const HashTapeView& v, uint32_t lane, uint32_t* st, uint32_t stride) {
  const HashTapeHead& h = *(const HashTapeHead*)v.tape;
  const uint32_t tx = v.tape[h.lanes + lane];
  if (tx == TAPE_IDLE) return false;
  const uint32_t* rec = v.tape + h.txs + 4 * tx;
  const uint32_t* shape = v.tape + h.shapes + 4 * rec[0];
  const uint32_t* data = v.tape + h.data;
  uint32_t cursor = rec[1];
  uint32_t* slots = v.slots + 8 * (size_t)rec[2];
  TapeStrobe s{st, stride, 0, 0};
  for (uint32_t ji = shape[0]; ji < shape[0] + shape[1]; ++ji) {
    const uint32_t* job = v.tape + h.jobs + 4 * ji;
    const uint32_t* init = v.protos + TAPE_PROTO_WORDS * (job[0] & 0xffu);
    for (uint32_t i = 0; i < 50; ++i) st[i * stride] = init[i];
    s.pos = init[50]; s.pos_begin = init[51];
    for (uint32_t q = job[2]; q < job[2] + job[3]; ++q) {
      const uint32_t* pc = v.tape + h.pieces + 4 * q;
      const uint32_t label = pc[0] & 0xffu;
      if (label != 0) { tape_label_len(s, v.labels, label, pc[2]); tape_begin_op(s, 2u); }      // (0 = L_CONT: the message goes on)
      if ((pc[0] >> 8) == TAPE_SLOT) tape_absorb(s, slots + 8 * (size_t)pc[3], 0, 32);
      else { tape_absorb(s, data, cursor, pc[1]); cursor += pc[1]; }
    }
    tape_label_len(s, v.labels, (job[0] >> 8) & 0xffu, 32);
    tape_begin_op(s, 1u | 2u | 4u);                      // PRF: the position is 0 afterwards, the challenge the first 8 words
    uint32_t* out = slots + 8 * (size_t)job[1];
    for (uint32_t i = 0; i < 8; ++i) out[i] = st[i * stride];
  }
  const uint32_t* root = slots + 8 * (size_t)shape[3];
  for (uint32_t i = 0; i < 8; ++i) v.txid[8 * (size_t)tx + i] = root[i];
  return true;
}

}  // namespace zkvm
}  // namespace zk

// ===================================================== host side =====================================================
#include "host_pool.hpp"
#include "zkvm_tx.hpp"

#include <cassert>
#include <cstring>
#include <mutex>
#include <vector>

namespace zk {
namespace zkvm {

inline bool tape_keeps(uint8_t proto) { return proto == P_CONTRACTID || proto == P_RATCHET || proto == P_TXID; }

// protos: N_PROTO x 52 words; labels: N_LABEL x 16 bytes
inline void hash_tape_constants(std::vector<uint32_t>& protos, std::vector<uint8_t>& labels) {
  protos.assign((size_t)N_PROTO * TAPE_PROTO_WORDS, 0);
  for (uint8_t p = 0; p < N_PROTO; ++p) proto_transcript(p).export_state(&protos[(size_t)p * TAPE_PROTO_WORDS]);
  labels.assign((size_t)N_LABEL * TAPE_LABEL_BYTES, 0);
  for (uint8_t l = 0; l < N_LABEL; ++l) {
    const char* t = label_text(l);
    const size_t n = std::strlen(t);
    assert(n < TAPE_LABEL_BYTES);
    labels[(size_t)l * TAPE_LABEL_BYTES] = (uint8_t)n;
    std::memcpy(&labels[(size_t)l * TAPE_LABEL_BYTES + 1], t, n);
  }
}

// The flattener of one chunk.  reset(n); add(j, plan, root slot) for the transactions j < n the VM accepted -- from any
// thread, as long as the transactions of one group of eight (j / 8) come from one thread --; finish().  Nothing shrinks
// between chunks: the same call made again allocates nothing.
class TxHashTape {
 public:
  void reset(size_t n) {
    n_ = n;
    rec_.assign(n, Rec{});
    if (group_.size() < (n + 7) / 8) group_.resize((n + 7) / 8);
    for (size_t g = 0; g < (n + 7) / 8; ++g) group_[g].clear();
    shapes_.clear(); keys_.clear(); jobs_.clear(); pieces_.clear();
    order_.clear(); n_tx_ = 0;
  }
  // false: the plan holds a job this tape cannot run (a 64-byte challenge among the three protocols; a label or a piece
  // beyond the formats above) -- the caller fails the chunk
  bool add(size_t j, const TxPlan& P, uint32_t root_slot) {
    static thread_local std::vector<uint32_t> key;
    key.clear();
    key.push_back(P.n_slots); key.push_back(root_slot);
    std::vector<uint8_t>& run = group_[j / 8];
    const size_t run0 = run.size();
    for (const HashJob& jb : P.jobs) {
      if (!tape_keeps(jb.proto)) continue;
      if (jb.out_len != 32 || jb.out_slot >= P.n_slots || jb.chal_label >= N_LABEL) { run.resize(run0); return false; }
      key.push_back(0x4a000000u | jb.proto | ((uint32_t)jb.chal_label << 8)); key.push_back(jb.out_slot); key.push_back(jb.count);
      for (uint32_t q = jb.first; q < jb.first + jb.count; ++q) {
        const HashPiece& h = P.pieces[q];
        if (h.label >= N_LABEL || (h.kind == HashPiece::Slot && (h.len != 32 || h.slot >= P.n_slots))) { run.resize(run0); return false; }
        key.push_back((uint32_t)h.label | ((h.kind == HashPiece::Slot ? TAPE_SLOT : TAPE_RUN) << 8));
        key.push_back(h.len); key.push_back(h.msg_len); key.push_back(h.kind == HashPiece::Slot ? h.slot : 0);
        if (h.kind == HashPiece::Bytes) run.insert(run.end(), h.p, h.p + h.len);
        else if (h.kind == HashPiece::Imm) run.insert(run.end(), P.imm.begin() + h.off, P.imm.begin() + h.off + h.len);
      }
    }
    if (root_slot >= P.n_slots) { run.resize(run0); return false; }
    Rec& r = rec_[j];
    r.off = run0; r.len = run.size() - run0; r.n_slots = P.n_slots;
    r.shape = intern(key);
    return true;
  }
  // -> the block is built.  threads: for the copy of the runs
  void finish(int threads) {
    const size_t ns = keys_.size();
    std::vector<size_t> count(ns, 0), lane0(ns + 1, 0);
    for (size_t j = 0; j < n_; ++j) if (rec_[j].shape != TAPE_IDLE) { ++count[rec_[j].shape]; }
    for (size_t s = 0; s < ns; ++s) lane0[s + 1] = lane0[s] + ((count[s] + 63) & ~(size_t)63);
    const size_t n_lanes = lane0[ns];
    // transactions are numbered in the order of the chunk (the t-th one added, by position): txid[t]
    order_.clear();
    size_t data_bytes = 0, n_slots = 0;
    for (size_t j = 0; j < n_; ++j) {
      Rec& r = rec_[j];
      if (r.shape == TAPE_IDLE) continue;
      r.t = (uint32_t)order_.size(); order_.push_back((uint32_t)j);
      r.data_off = data_bytes; data_bytes += r.len;
      r.slot0 = n_slots; n_slots += r.n_slots;
    }
    n_tx_ = order_.size();
    HashTapeHead h{};
    h.magic = TAPE_MAGIC; h.n_lanes = (uint32_t)n_lanes; h.n_tx = (uint32_t)n_tx_; h.n_shapes = (uint32_t)ns;
    h.n_jobs = (uint32_t)(jobs_.size() / 4); h.n_pieces = (uint32_t)(pieces_.size() / 4);
    h.data_bytes = (uint32_t)data_bytes; h.n_slots = (uint32_t)n_slots;
    size_t at = 16;
    auto section = [&at](size_t words) { const size_t o = at; at = (at + words + 3) & ~(size_t)3; return (uint32_t)o; };
    h.shapes = section(4 * ns); h.jobs = section(jobs_.size()); h.pieces = section(pieces_.size());
    h.lanes = section(n_lanes); h.txs = section(4 * n_tx_); h.data = section((data_bytes + 3) / 4);
    h.words = (uint32_t)at;
    if (block_.size() < at) block_.resize(at + at / 8);
    uint32_t* b = block_.data();
    std::memcpy(b, &h, sizeof h);
    if (ns) std::memcpy(b + h.shapes, shapes_.data(), 16 * ns);
    if (!jobs_.empty()) std::memcpy(b + h.jobs, jobs_.data(), 4 * jobs_.size());
    if (!pieces_.empty()) std::memcpy(b + h.pieces, pieces_.data(), 4 * pieces_.size());
    for (size_t l = 0; l < n_lanes; ++l) b[h.lanes + l] = TAPE_IDLE;
    std::vector<size_t> next(lane0.begin(), lane0.end() - 1);
    for (size_t t = 0; t < n_tx_; ++t) {
      const Rec& r = rec_[order_[t]];
      b[h.lanes + next[r.shape]++] = (uint32_t)t;
      uint32_t* rec = b + h.txs + 4 * t;
      rec[0] = r.shape; rec[1] = (uint32_t)r.data_off; rec[2] = (uint32_t)r.slot0; rec[3] = 0;
    }
    if (data_bytes & 3) b[h.data + data_bytes / 4] = 0;              // (the last word's tail: defined bytes)
    uint8_t* data = (uint8_t*)(b + h.data);
    host_parallel((n_ + 7) / 8, threads, [&](size_t g) {
      for (size_t j = 8 * g; j < std::min(n_, 8 * g + 8); ++j) {
        const Rec& r = rec_[j];
        if (r.shape != TAPE_IDLE && r.len) std::memcpy(data + r.data_off, group_[g].data() + r.off, r.len);
      }
    });
  }
  const uint32_t* block() const { return block_.data(); }
  const HashTapeHead& head() const { return *(const HashTapeHead*)block_.data(); }
  size_t bytes() const { return 4 * (size_t)head().words; }
  size_t n_tx() const { return n_tx_; }
  size_t position(size_t t) const { return order_[t]; }            // where in the chunk transaction t of the tape lies

 private:
  struct Rec { uint32_t shape = TAPE_IDLE, t = 0, n_slots = 0; size_t off = 0, len = 0, data_off = 0, slot0 = 0; };
  // the shape whose key this is (a new one: its jobs and pieces are appended)
  uint32_t intern(const std::vector<uint32_t>& key) {
    std::lock_guard<std::mutex> lk(mu_);
    for (size_t s = 0; s < keys_.size(); ++s) if (keys_[s] == key) return (uint32_t)s;
    keys_.push_back(key);
    const uint32_t job0 = (uint32_t)(jobs_.size() / 4);
    uint32_t n_jobs = 0;
    for (size_t i = 2; i < key.size();) {
      const uint32_t head = key[i], out_slot = key[i + 1], count = key[i + 2];
      i += 3;
      jobs_.push_back((head & 0xffu) | (((head >> 8) & 0xffu) << 8) | (32u << 16));
      jobs_.push_back(out_slot); jobs_.push_back((uint32_t)(pieces_.size() / 4)); jobs_.push_back(count);
      for (uint32_t q = 0; q < count; ++q, i += 4) pieces_.insert(pieces_.end(), key.begin() + i, key.begin() + i + 4);
      ++n_jobs;
    }
    const uint32_t rec[4] = {job0, n_jobs, key[0], key[1]};
    shapes_.insert(shapes_.end(), rec, rec + 4);
    return (uint32_t)(keys_.size() - 1);
  }
  size_t n_ = 0, n_tx_ = 0;
  std::vector<Rec> rec_;
  std::vector<std::vector<uint8_t>> group_;
  std::mutex mu_;
  std::vector<std::vector<uint32_t>> keys_;
  std::vector<uint32_t> shapes_, jobs_, pieces_, order_, block_;
};

// Is the block what the interpreter may index blindly?  Every offset inside the block, every slot inside the transaction's
// slot area, every run inside `data`, every lane a transaction of its wavefront's shape or idle, every transaction once.
// (What the builder makes passes by construction; the CPU tests and the sanitizer program ask anyway.)
inline bool hash_tape_check(const uint32_t* b, size_t words) {
  if (words < 16) return false;
  const HashTapeHead& h = *(const HashTapeHead*)b;
  auto inside = [&](uint32_t off, uint64_t n) { return off >= 16 && (off & 3) == 0 && (uint64_t)off + n <= h.words; };
  if (h.magic != TAPE_MAGIC || h.words > words || (h.n_lanes & 63)) return false;
  if (!inside(h.shapes, 4ull * h.n_shapes) || !inside(h.jobs, 4ull * h.n_jobs) || !inside(h.pieces, 4ull * h.n_pieces) ||
      !inside(h.lanes, h.n_lanes) || !inside(h.txs, 4ull * h.n_tx) || !inside(h.data, ((uint64_t)h.data_bytes + 3) / 4)) return false;
  std::vector<uint64_t> run_len(h.n_shapes, 0);
  for (uint32_t s = 0; s < h.n_shapes; ++s) {
    const uint32_t* sh = b + h.shapes + 4 * s;
    if ((uint64_t)sh[0] + sh[1] > h.n_jobs || sh[3] >= sh[2]) return false;
    for (uint32_t ji = sh[0]; ji < sh[0] + sh[1]; ++ji) {
      const uint32_t* job = b + h.jobs + 4 * ji;
      if ((job[0] & 0xffu) >= N_PROTO || ((job[0] >> 8) & 0xffu) >= N_LABEL || (job[0] >> 16) != 32 || job[1] >= sh[2]) return false;
      if ((uint64_t)job[2] + job[3] > h.n_pieces) return false;
      for (uint32_t q = job[2]; q < job[2] + job[3]; ++q) {
        const uint32_t* pc = b + h.pieces + 4 * q;
        if ((pc[0] & 0xffu) >= N_LABEL || (pc[0] >> 8) > TAPE_SLOT) return false;
        if ((pc[0] >> 8) == TAPE_SLOT) { if (pc[3] >= sh[2] || pc[1] != 32) return false; }
        else run_len[s] += pc[1];
      }
    }
  }
  uint64_t slots = 0;
  for (uint32_t t = 0; t < h.n_tx; ++t) {
    const uint32_t* rec = b + h.txs + 4 * t;
    if (rec[0] >= h.n_shapes || (uint64_t)rec[1] + run_len[rec[0]] > h.data_bytes) return false;
    if (rec[2] != slots) return false;
    slots += (b + h.shapes + 4 * rec[0])[2];
  }
  if (slots != h.n_slots) return false;
  std::vector<uint8_t> seen(h.n_tx, 0);
  for (uint32_t w = 0; w < h.n_lanes; w += 64) {
    uint32_t shape = TAPE_IDLE;
    for (uint32_t l = w; l < w + 64; ++l) {
      const uint32_t t = b[h.lanes + l];
      if (t == TAPE_IDLE) continue;
      if (t >= h.n_tx || seen[t]) return false;
      seen[t] = 1;
      const uint32_t s = (b + h.txs + 4 * t)[0];
      if (shape != TAPE_IDLE && s != shape) return false;
      shape = s;
    }
  }
  for (uint32_t t = 0; t < h.n_tx; ++t) if (!seen[t]) return false;
  return true;
}

// The second pass of a flagged call over up to eight transactions (tx_run_group, zkvm_tx.hpp): parse, VM and the WHOLE plan;
// the MuSig jobs alone run here, everything else of the plan goes to the tape as transaction j0 + i of its chunk.  The slot
// memory is zeroed: the statement's transaction ID reads zero until the device's has been collected.
// -> false: a plan the tape cannot hold (the call fails closed)
// host_only = NO_PROTO (a precompute-only call): not even the MuSig jobs run -- nothing of the signature is looked at
inline bool tx_prepare_many_taped(const uint8_t* const* tx, const size_t* len, TxStatement* st, size_t count, TxHashTape& tape, size_t j0,
                                  uint8_t host_only = P_MUSIG) {
  bool ok = true;
  tx_run_group(tx, len, st, count, ALL_PROTOS, host_only, true, true,
               [&](size_t i, const TxPlan& plan, const TxSlots& out, const uint8_t*) { ok &= tape.add(j0 + i, plan, out.txid); });
  return ok;
}

// the whole tape on the CPU: slots (32 bytes per slot of the block) and IDs (32 bytes per transaction)
inline void hash_tape_run_host(const uint32_t* block, const std::vector<uint32_t>& protos, const std::vector<uint8_t>& labels,
                               std::vector<uint32_t>& slots, std::vector<uint32_t>& txid) {
  const HashTapeHead& h = *(const HashTapeHead*)block;
  slots.assign(8 * (size_t)h.n_slots + 8, 0);
  txid.assign(8 * (size_t)h.n_tx + 8, 0);
  HashTapeView v{block, protos.data(), labels.data(), slots.data(), txid.data()};
  uint32_t st[50];
  for (uint32_t lane = 0; lane < h.n_lanes; ++lane) tx_hash_run(v, lane, st, 1);
}

}  // namespace zkvm
}  // namespace zk
