// tx_hash_kernels.hpp -- the hash tape of a chunk of transactions on the device (tx_hash_tape.hpp; zkgpu.h:
// ZKGPU_TXFORMAT_HASH_ON_DEVICE): contract IDs, anchor ratchets and the Merkle tree of the transaction ID.
//
// k_tx_hash: one lane per transaction, 64 lanes per block, grid = padded lanes / 64.  A transaction's jobs are a dependent
// chain through its slots, so lanes are the only parallelism inside a shape; a wavefront holds ONE shape (the tape pads every
// shape's run to 64), so its lanes walk the same jobs and pieces and differ in the bytes alone.  Each lane keeps its 50 state
// words in LDS (word i of lane l at st[i * 64 + l]: no bank conflicts, and byte positions index memory, not registers), as
// k_transcript does (prep_kernels.hpp); the permutation is merlin_dev.hpp's, in registers.  Idle lanes return before they
// touch memory other than their word of the lane table.  Slots live in global memory, 32 bytes each; the root's 32 bytes are
// also written to the dense txid[] array, which is all that is copied back.  (The same tape walked by dependency level, four
// lanes per transaction: k_tx_hash_levels, tx_hash_levels.hpp -- the hashing stage of a precompute-only call.)
//
// k_tx_log_gather (ZKGPU_TXFORMAT_RETURN_LOG; tx_log.hpp): behind k_tx_hash on the same stream, one lane per (transaction of
// the tape, window position j < K), 64 lanes per block.  A lane reads its transaction's shape and slot base from the tape's
// txs records and the shape's entry table from a buffer of its own; if the shape logs more than j and at most K entries it
// copies the 32 bytes of entry j's slot to log[tx][j] (two 16-byte loads and stores), otherwise it writes zeros -- every byte
// of the dense array is written, so the copy down never reads stale memory.  No LDS, no atomics; lanes past n_tx * K return
// before they touch memory.
#pragma once
#include "tx_hash_tape.hpp"
#include "tx_log.hpp"

namespace zk {

__global__ void __launch_bounds__(64)
k_tx_hash(zkvm::HashTapeView v, uint32_t n_lanes) {
  __shared__ uint32_t st[50 * 64];
  const uint32_t lane = blockIdx.x * 64 + threadIdx.x;
  if (lane >= n_lanes) return;
  zkvm::tx_hash_run(v, lane, st + threadIdx.x, 64);
}

__global__ void __launch_bounds__(64)
k_tx_log_gather(const uint32_t* tape, const uint32_t* table, const uint32_t* slots, uint32_t* log, uint32_t n_tx, uint32_t K) {
  const uint32_t idx = blockIdx.x * 64 + threadIdx.x;     // (n_tx * K < 2^32: asked by the host before the launch)
  if (idx >= n_tx * K) return;
  zkvm::tx_log_gather_lane(tape, table, slots, log, idx, K);
}

}  // namespace zk
