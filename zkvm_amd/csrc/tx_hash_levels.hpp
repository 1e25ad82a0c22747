// tx_hash_levels.hpp -- the hash tape of a chunk (tx_hash_tape.hpp) walked by DEPENDENCY LEVEL instead of job by job: the side
// table that says which jobs of a shape may run together, the interpreter that runs one (transaction, lane, level) -- ONE
// function for the host and the device -- and k_tx_hash_levels, which gives every transaction T lanes.
//
// tx_hash_run walks a transaction's jobs in the order the VM wrote them, about 15 dependent hashes for a 2-in / 2-out payment,
// one lane per transaction.  But a transaction's jobs depend on each other only through the slots named by their TAPE_SLOT
// pieces, and several groups of them are independent: the contract IDs of the inputs, the header's leaf, the leaves of entries
// whose IDs are known, the nodes of one tree level.  A job's LEVEL is 0 if it reads no slot a job of the tape writes, else one
// more than the highest level among the producers of its slot pieces; the jobs of one level need nothing of each other.  A
// 2-in / 2-out payment has 15 jobs on 7 levels of 3, 3, 3, 2, 2, 1 and 1 jobs; an 8-in / 8-out one 57 jobs on 15 levels.
//
// The side table (32-bit words; built once per tape from the tape's own jobs and pieces -- no label, no protocol is known here;
// uploaded in a buffer of its own beside the tape, as the log's table is; the block's format is untouched):
//   [0] TAPE_LEVELS_MAGIC  [1] shapes  [2] words in all  [3] the most levels any shape has
//   [4 + s]  where shape s's part starts; there:
//     levels L | jobs J | first[0 .. L]: where in the order level l's jobs start (first[L] = J) | J x (job, run offset)
//   `job` counts from the shape's first job, in (level, job) order; `run offset` is where the job's TAPE_RUN pieces start in the
//   transaction's byte run -- the cursor tx_hash_run advances job by job, which piece lengths make a property of the shape.
//
// k_tx_hash_levels: T = TAPE_LEVEL_LANES = 4 lanes per transaction, 64 lanes per block, so a block (one wavefront) holds 16
// consecutive entries of the tape's lane table.  The tape pads every shape's run to 64 entries, so those 16 are ONE shape or
// idle: the lane ordering rule of the tape, in units of transactions x T.  (At a cost: the table is padded for 64 transactions
// per wavefront and is not re-padded here -- the block's format stays as it is -- so of the four blocks at the end of a
// shape's run up to three are wholly idle; they read 16 words and leave after the level count's two barriers.  Nothing at a
// call's chunk of one shape, most of the grid for a call of many shapes with a few transactions each.)  T = 4 because no level of a payment with up to
// three inputs and three outputs is wider (wider levels -- the nine level-0 jobs of eight inputs -- are walked in rounds of T), and because a
// quarter of the transactions per wavefront still fills the chip at the chunk sizes of a call (8192 transactions = 512 blocks).
// Each lane keeps its 50 state words in LDS as k_tx_hash does (word i of lane l at st[i * 64 + l]); the permutation is
// merlin_dev.hpp's, in registers.  Results cross lanes through the slot memory in global memory: between two levels stand a
// workgroup-scope fence and a block barrier (the block is the only reader of its transactions' slots before the kernel ends),
// nothing relies on lockstep execution, a lane without a job at a level waits at the barrier, and no lane returns before the
// last level of its block -- the level count is the block's, agreed through LDS.  Lanes of idle entries read their word of the
// lane table and nothing else.  Every index the interpreter reads from the tape or the table is bounded by the head's counts
// (and the table's size) before it is used: a block that fails hash_tape_check makes it skip the job, never read outside.
#pragma once
#include "tx_hash_tape.hpp"

namespace zk {
namespace zkvm {

constexpr uint32_t TAPE_LEVELS_MAGIC = 0x4c56454cu, TAPE_LEVEL_LANES = 4;

struct HashLevelsView { const uint32_t* table; uint32_t words; };     // the side table and its size

// The levels of the transaction an entry of the lane table names -- 0: not a transaction of this tape, or its shape's part of
// the table is not whole (then nothing of it is read).  At most the shape's jobs, which the head's count bounds.
ZK_TAPE_HD inline uint32_t tx_hash_levels_of(const HashTapeView& v, const HashLevelsView& lv, uint32_t tx) {
  const HashTapeHead& h = *(const HashTapeHead*)v.tape;
  if (tx >= h.n_tx || lv.words < 4 || lv.table[0] != TAPE_LEVELS_MAGIC) return 0;
  const uint32_t shape = (v.tape + h.txs + 4 * (size_t)tx)[0];
  if (shape >= h.n_shapes || shape >= lv.table[1] || 4 + (uint64_t)shape >= lv.words) return 0;
  const uint32_t at = lv.table[4 + shape];
  if ((uint64_t)at + 2 > lv.words) return 0;
  const uint32_t L = lv.table[at], J = lv.table[at + 1];
  if (J != (v.tape + h.shapes + 4 * (size_t)shape)[1] || J > h.n_jobs || L > J || (uint64_t)at + 2 + ((uint64_t)L + 1) + 2 * (uint64_t)J > lv.words) return 0;
  return L;
}

// The jobs of `level` that fall to lane `sub` of the `lanes` lanes of transaction `tx`: the sub-th, (sub + lanes)-th ... of the
// level in the table's order, each run exactly as tx_hash_run runs it -- every message streamed piece by piece with its length
// framed once from msg_len, the challenge written to the job's slot; the root's also to txid.  The caller orders the levels
// (every job of level l - 1 is finished and visible before any of level l starts).  st: 50 words of scratch, word i at
// st[i * stride].
ZK_TAPE_HD inline void tx_hash_level_run(const HashTapeView& v, const HashLevelsView& lv, uint32_t tx, uint32_t sub, uint32_t lanes, uint32_t level,
                                         uint32_t* st, uint32_t stride) {
  const HashTapeHead& h = *(const HashTapeHead*)v.tape;
  if (level >= tx_hash_levels_of(v, lv, tx)) return;       // (bounds tx, its shape and the shape's part of the table: L levels, J = the shape's jobs)
  const uint32_t* rec = v.tape + h.txs + 4 * (size_t)tx;
  const uint32_t* shape = v.tape + h.shapes + 4 * (size_t)rec[0];
  const uint32_t* tab = lv.table + lv.table[4 + rec[0]];
  const uint32_t L = tab[0], J = tab[1];
  if ((uint64_t)shape[0] + shape[1] > h.n_jobs || (uint64_t)rec[2] + shape[2] > h.n_slots) return;
  const uint32_t* first = tab + 2;
  const uint32_t* order = tab + 2 + (L + 1);
  const uint32_t* data = v.tape + h.data;
  uint32_t* slots = v.slots + 8 * (size_t)rec[2];
  TapeStrobe s{st, stride, 0, 0};
  for (uint32_t q = first[level] + sub; q < first[level + 1] && q < J; q += lanes) {
    if (order[2 * q] >= J) continue;
    const uint32_t* job = v.tape + h.jobs + 4 * (size_t)(shape[0] + order[2 * q]);
    uint32_t cursor = rec[1] + order[2 * q + 1];
    if ((uint64_t)job[2] + job[3] > h.n_pieces || job[1] >= shape[2] || (job[0] & 0xffu) >= N_PROTO || ((job[0] >> 8) & 0xffu) >= N_LABEL) continue;
    const uint32_t* init = v.protos + TAPE_PROTO_WORDS * (job[0] & 0xffu);
    for (uint32_t i = 0; i < 50; ++i) st[i * stride] = init[i];
    s.pos = init[50]; s.pos_begin = init[51];
    bool inside = true;
    for (uint32_t p = job[2]; p < job[2] + job[3]; ++p) {
      const uint32_t* pc = v.tape + h.pieces + 4 * (size_t)p;
      const uint32_t label = pc[0] & 0xffu;
      const bool slot = (pc[0] >> 8) == TAPE_SLOT;
      if (label >= N_LABEL || (slot ? pc[3] >= shape[2] : (uint64_t)cursor + pc[1] > h.data_bytes)) { inside = false; break; }
      if (label != 0) { tape_label_len(s, v.labels, label, pc[2]); tape_begin_op(s, 2u); }
      if (slot) tape_absorb(s, slots + 8 * (size_t)pc[3], 0, 32);
      else { tape_absorb(s, data, cursor, pc[1]); cursor += pc[1]; }
    }
    if (!inside) continue;
    tape_label_len(s, v.labels, (job[0] >> 8) & 0xffu, 32);
    tape_begin_op(s, 1u | 2u | 4u);
    uint32_t* out = slots + 8 * (size_t)job[1];
    for (uint32_t i = 0; i < 8; ++i) out[i] = st[i * stride];
    if (job[1] == shape[3]) for (uint32_t i = 0; i < 8; ++i) v.txid[8 * (size_t)tx + i] = st[i * stride];
  }
}

}  // namespace zkvm

#if defined(__HIPCC__)
__global__ void __launch_bounds__(64)
k_tx_hash_levels(zkvm::HashTapeView v, zkvm::HashLevelsView lv, uint32_t n_lanes) {
  constexpr uint32_t T = zkvm::TAPE_LEVEL_LANES;
  __shared__ uint32_t st[50 * 64];
  __shared__ uint32_t block_levels;
  const uint32_t entry = blockIdx.x * (64 / T) + threadIdx.x / T;      // of the tape's lane table
  const uint32_t tx = entry < n_lanes ? v.tape[((const zkvm::HashTapeHead*)v.tape)->lanes + entry] : zkvm::TAPE_IDLE;
  const uint32_t mine = tx == zkvm::TAPE_IDLE ? 0 : zkvm::tx_hash_levels_of(v, lv, tx);
  if (threadIdx.x == 0) block_levels = 0;
  __syncthreads();
  if (mine) atomicMax(&block_levels, mine);
  __syncthreads();
  const uint32_t levels = block_levels;
  for (uint32_t level = 0; level < levels; ++level) {
    if (level < mine) zkvm::tx_hash_level_run(v, lv, tx, threadIdx.x % T, T, level, st + threadIdx.x, 64);
    __threadfence_block();                                 // this level's slots before the next level's reads, for the whole block
    __syncthreads();
  }
}
#endif

}  // namespace zk

// ===================================================== host side =====================================================
#include <vector>

namespace zk {
namespace zkvm {

// The side table of a finished block.  -> false: a job reads a slot that a LATER job of its shape writes (tx_hash_run would read
// it before it is written: no order by levels computes the same), two jobs write one slot, or an index outside the shape --
// none of which a block that passes hash_tape_check and came from TxHashTape has
inline bool tx_hash_levels_table(const uint32_t* block, std::vector<uint32_t>& table) {
  const HashTapeHead& h = *(const HashTapeHead*)block;
  table.assign(4 + (size_t)h.n_shapes, 0);
  table[0] = TAPE_LEVELS_MAGIC; table[1] = h.n_shapes;
  std::vector<uint32_t> level, offset, producer;
  for (uint32_t s = 0; s < h.n_shapes; ++s) {
    const uint32_t* sh = block + h.shapes + 4 * (size_t)s;
    const uint32_t J = sh[1];
    if ((uint64_t)sh[0] + J > h.n_jobs) return false;
    level.assign(J, 0); offset.assign(J, 0); producer.assign(sh[2], TAPE_IDLE);
    uint32_t cursor = 0, L = 0;
    for (uint32_t j = 0; j < J; ++j) {
      const uint32_t* job = block + h.jobs + 4 * (size_t)(sh[0] + j);
      if ((uint64_t)job[2] + job[3] > h.n_pieces || job[1] >= sh[2] || producer[job[1]] != TAPE_IDLE) return false;
      offset[j] = cursor;
      for (uint32_t p = job[2]; p < job[2] + job[3]; ++p) {
        const uint32_t* pc = block + h.pieces + 4 * (size_t)p;
        if ((pc[0] >> 8) != TAPE_SLOT) { cursor += pc[1]; continue; }
        if (pc[3] >= sh[2]) return false;
        if (producer[pc[3]] != TAPE_IDLE) level[j] = std::max(level[j], level[producer[pc[3]]] + 1);     // (no producer on the tape: a slot of the host's)
      }
      producer[job[1]] = j;
      L = std::max(L, level[j] + 1);
    }
    // (a slot read before the job that writes it: found by a second look, now that every producer is known)
    for (uint32_t j = 0; j < J; ++j) {
      const uint32_t* job = block + h.jobs + 4 * (size_t)(sh[0] + j);
      for (uint32_t p = job[2]; p < job[2] + job[3]; ++p) {
        const uint32_t* pc = block + h.pieces + 4 * (size_t)p;
        if ((pc[0] >> 8) == TAPE_SLOT && producer[pc[3]] != TAPE_IDLE && producer[pc[3]] >= j) return false;
      }
    }
    table[4 + s] = (uint32_t)table.size();
    table.push_back(L); table.push_back(J);
    const size_t first = table.size();
    table.resize(first + L + 1, 0);
    for (uint32_t l = 0; l < L; ++l) {
      table[first + l] = (uint32_t)((table.size() - (first + L + 1)) / 2);
      for (uint32_t j = 0; j < J; ++j) if (level[j] == l) { table.push_back(j); table.push_back(offset[j]); }
    }
    table[first + L] = J;
    table[3] = std::max(table[3], L);
  }
  table[2] = (uint32_t)table.size();
  return true;
}

// the whole tape on the CPU the way k_tx_hash_levels walks it with `lanes` lanes per transaction: level by level, and within a
// level lane by lane -- every (transaction, lane) of a level before any of the next
inline bool hash_tape_run_levels_host(const uint32_t* block, const std::vector<uint32_t>& protos, const std::vector<uint8_t>& labels, uint32_t lanes,
                                      std::vector<uint32_t>& slots, std::vector<uint32_t>& txid) {
  const HashTapeHead& h = *(const HashTapeHead*)block;
  std::vector<uint32_t> table;
  slots.assign(8 * (size_t)h.n_slots + 8, 0);
  txid.assign(8 * (size_t)h.n_tx + 8, 0);
  if (lanes == 0 || !tx_hash_levels_table(block, table)) return false;
  HashTapeView v{block, protos.data(), labels.data(), slots.data(), txid.data()};
  const HashLevelsView lv{table.data(), (uint32_t)table.size()};
  uint32_t st[50];
  for (uint32_t level = 0; level < table[3]; ++level)
    for (uint32_t entry = 0; entry < h.n_lanes; ++entry) {
      const uint32_t tx = block[h.lanes + entry];
      if (tx == TAPE_IDLE) continue;
      for (uint32_t sub = 0; sub < lanes; ++sub) tx_hash_level_run(v, lv, tx, sub, lanes, level, st, 1);
    }
  return true;
}

}  // namespace zkvm
}  // namespace zk
