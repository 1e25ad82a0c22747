// tx_root_kernels.hpp -- the transaction root of a call on the device (tx_root.hpp; zkgpu.h: ZKGPU_TXFORMAT_RETURN_ROOT beside
// ZKGPU_TXFORMAT_HASH_ON_DEVICE): the IDs of a call are in HBM when its tapes have run; the tree over them is folded there and
// 32 bytes come down.
//
// k_tx_root_leaves: behind a chunk's k_tx_hash / k_tx_hash_levels on the same stream, one lane per transaction of the tape, 64
// lanes per block.  Lane t hashes the leaf of txid[t] and writes it to leaf[pos[t]], pos[t] = where in the CALL the transaction
// lies (the chunk's start + the position the ID copy-down uses; uploaded beside the tape).  The tape orders transactions by
// shape, the tree wants call order: the scatter is this kernel's.  A position outside the call-wide array writes nothing.  The
// array is zeroed when the call starts, so transactions that never reach a tape leave defined bytes (the root is discarded then).
//
// k_tx_root_fold: one block of TX_ROOT_LANES = 64 lanes (one wavefront) folds the aligned span of 2^s nodes that starts at node
// blockIdx.x << s of in[0 .. n_in) through s levels and writes node blockIdx.x of out.  The span's nodes lie in LDS in two
// arrays the levels alternate between (2^s and 2^(s - 1) nodes of 8 words); each lane keeps its 50 state words in LDS as
// k_tx_hash does (word i of lane l at st[i * 64 + l]); the permutation is merlin_dev.hpp's, in registers.  Between two levels
// stand a workgroup-scope fence and a block barrier; nothing relies on lockstep execution, the level count is the launch's (every
// lane passes every barrier), and a lane without a pair at a level only waits.  No cooperative launch, no grid-wide wait, no
// atomics: the host launches it once per pass (tx_root_passes), alternating two node arrays, until one node is left.  Every
// index is bounded by n_in and s: a block past the last span returns before it touches memory.
//
// s = TX_ROOT_SPAN = 7 and 64 lanes: the first level of a full span has 64 pairs, one per lane of ONE wavefront, so no lane of
// the block idles at the level that holds half the block's hashes, and the block needs no barrier across wavefronts.  LDS per
// block: 50 words x 64 lanes = 12.5 KB of state + 6 KB of nodes = 18.5 KB, eight blocks per CU of 160 KB -- more than a call
// supplies (8192 leaves are 64 blocks, 32 768 are 256: one per CU), so occupancy is the grid's, not the LDS's.  A larger s would
// save passes only beyond 2^14 leaves (two passes up to there) and idle more lanes per block; a smaller s adds launches.
#pragma once
#include "tx_root.hpp"

namespace zk {

__global__ void __launch_bounds__(64)
k_tx_root_leaves(zkvm::TxRootView c, const uint32_t* txid, const uint32_t* pos, uint32_t n_tx, uint32_t* leaf, uint32_t n_leaf) {
  __shared__ uint32_t st[50 * 64];
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n_tx) return;
  const uint32_t at = pos[t];
  if (at >= n_leaf) return;
  zkvm::tx_root_leaf(c, txid + zkvm::TX_ROOT_NODE_WORDS * (size_t)t, leaf + zkvm::TX_ROOT_NODE_WORDS * (size_t)at, st + threadIdx.x, 64);
}

__global__ void __launch_bounds__(zkvm::TX_ROOT_LANES)
k_tx_root_fold(zkvm::TxRootView c, const uint32_t* in, uint32_t n_in, uint32_t* out, uint32_t s) {
  constexpr uint32_t W = zkvm::TX_ROOT_NODE_WORDS, LANES = zkvm::TX_ROOT_LANES, FULL = 1u << zkvm::TX_ROOT_SPAN;
  __shared__ uint32_t st[50 * LANES];
  __shared__ uint32_t a[W * FULL], b[W * (FULL / 2)];
  if (s < 1 || s > zkvm::TX_ROOT_SPAN) return;              // (the whole grid alike: no barrier has been reached)
  const uint64_t first = (uint64_t)blockIdx.x << s;
  if (first >= n_in) return;                                // (the whole block alike)
  uint32_t m = (uint32_t)(n_in - first < (1ull << s) ? n_in - first : (1ull << s));
  for (uint32_t w = threadIdx.x; w < W * m; w += LANES) a[w] = in[W * first + w];
  __syncthreads();
  uint32_t* src = a;
  uint32_t* dst = b;
  for (uint32_t level = 0; level < s; ++level) {
    zkvm::tx_root_fold_level(c, src, m, dst, threadIdx.x, LANES, st + threadIdx.x, LANES);
    m = (m + 1) / 2;
    __threadfence_block();                                  // this level's nodes before the next level's reads, for the whole block
    __syncthreads();
    uint32_t* t = src; src = dst; dst = t;
  }
  if (threadIdx.x < W) out[W * (size_t)blockIdx.x + threadIdx.x] = src[threadIdx.x];
}

}  // namespace zk
