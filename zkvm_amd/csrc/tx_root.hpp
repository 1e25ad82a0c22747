// tx_root.hpp -- the transaction root of a call (ZKGPU_TXFORMAT_RETURN_ROOT; upstream: zkvm `MerkleTree::root` over a block's
// transaction IDs, as recalled): the Merkle tree over the IDs of a call in call order, as ONE function for the host and the
// device, in the style of tx_hash_levels.hpp.  tx_root_kernels.hpp runs it on the device; the CPU tests, libzkhost and a call
// whose IDs are the host VM's run the same code through tx_root_fold_host.
//
// The tree is the transaction ID's own (zkvm_tx.hpp: plan_merkle; RFC 6962 split, Merlin transcripts) under another domain label:
//   node  = Transcript(label) . "L" left . "R" right -> challenge "merkle.node"
//   leaf  = Transcript(label) . "txid" id            -> challenge "merkle.leaf"
//   empty = Transcript(label)                        -> challenge "merkle.empty"
// UNPINNED: the domain label (TX_ROOT_LABEL) and the leaf's message label are a recollection, like the rest of the transaction
// format -- nothing held here pins them.  They are not in the manifest of tools/unpinned_manifest.py: the manifest and its
// stored copies are rebuilt together, which the change that brought this header could not do.  An integrator who has the real
// sources checks these two lines beside the manifest: TX_ROOT_LABEL below and L_txid in tx_root_leaf.
// The message and challenge labels are the label table's (zkvm_tx.hpp, by index); the 52 words of the freshly initialised
// transcript are made once on the host (tx_root_init, as hash_tape_constants makes the protocols') and handed in as data.
//
// The fold is bottom-up, level by level: nodes 2q and 2q + 1 of a level make node q of the next, and an unpaired last node
// moves up unchanged.  That is the RFC 6962 tree: the split "largest power of two below n" puts every aligned pair of a level
// under one parent and leaves exactly the unpaired tails to be joined higher up.  A PASS folds every aligned span of 2^s nodes
// through s levels into one node (the last span may hold fewer), so n nodes become ceil(n / 2^s); passes repeat until one is
// left.  Aligned spans hold whole pairs at each of their levels, so passes of any s give the same root.
#pragma once
#include "tx_hash_tape.hpp"

namespace zk {
namespace zkvm {

constexpr uint32_t TX_ROOT_SPAN = 7;                      // levels per pass: a span of 128 nodes, 64 pairs at its first level
constexpr uint32_t TX_ROOT_LANES = 64;                    // lanes of the block that folds a span (tx_root_kernels.hpp)
constexpr uint32_t TX_ROOT_NODE_WORDS = 8;

// what the functions below read: the initial transcript (TAPE_PROTO_WORDS words) and the label table (hash_tape_constants)
struct TxRootView { const uint32_t* init; const uint8_t* labels; };

ZK_TAPE_HD inline void tx_root_begin(const TxRootView& c, TapeStrobe& s) {
  for (uint32_t i = 0; i < 50; ++i) s.st[i * s.stride] = c.init[i];
  s.pos = c.init[50]; s.pos_begin = c.init[51];
}
ZK_TAPE_HD inline void tx_root_message(const TxRootView& c, TapeStrobe& s, uint32_t label, const uint32_t* words) {
  tape_label_len(s, c.labels, label, 32);
  tape_begin_op(s, 2u);
  tape_absorb(s, words, 0, 32);
}
ZK_TAPE_HD inline void tx_root_challenge(const TxRootView& c, TapeStrobe& s, uint32_t label, uint32_t* out) {
  tape_label_len(s, c.labels, label, 32);
  tape_begin_op(s, 1u | 2u | 4u);
  for (uint32_t i = 0; i < TX_ROOT_NODE_WORDS; ++i) out[i] = s.st[i * s.stride];
}
// st: 50 words of scratch, word i at st[i * stride] (here and below); id, left, right, out: 8 words each
ZK_TAPE_HD inline void tx_root_leaf(const TxRootView& c, const uint32_t* id, uint32_t* out, uint32_t* st, uint32_t stride) {
  TapeStrobe s{st, stride, 0, 0};
  tx_root_begin(c, s);
  tx_root_message(c, s, L_txid, id);
  tx_root_challenge(c, s, L_merkle_leaf, out);
}
ZK_TAPE_HD inline void tx_root_node(const TxRootView& c, const uint32_t* left, const uint32_t* right, uint32_t* out, uint32_t* st, uint32_t stride) {
  TapeStrobe s{st, stride, 0, 0};
  tx_root_begin(c, s);
  tx_root_message(c, s, L_L, left);
  tx_root_message(c, s, L_R, right);
  tx_root_challenge(c, s, L_merkle_node, out);
}
ZK_TAPE_HD inline void tx_root_empty(const TxRootView& c, uint32_t* out, uint32_t* st, uint32_t stride) {
  TapeStrobe s{st, stride, 0, 0};
  tx_root_begin(c, s);
  tx_root_challenge(c, s, L_merkle_empty, out);
}

// One level of one span, the part of lane `lane` of `lanes`: the m nodes at src (8 words each) become (m + 1) / 2 nodes at dst --
// node q from src[2q] and src[2q + 1], the unpaired last one copied.  src and dst do not overlap; the caller orders the levels
// (every node of a level is written and visible before the next level reads it).  Nothing outside src[0 .. m) is read, nothing
// outside dst[0 .. (m + 1) / 2) written.
ZK_TAPE_HD inline void tx_root_fold_level(const TxRootView& c, const uint32_t* src, uint32_t m, uint32_t* dst, uint32_t lane, uint32_t lanes,
                                          uint32_t* st, uint32_t stride) {
  for (uint32_t q = lane; q < (m + 1) / 2; q += lanes) {
    const uint32_t* left = src + TX_ROOT_NODE_WORDS * (size_t)(2 * q);
    uint32_t* out = dst + TX_ROOT_NODE_WORDS * (size_t)q;
    if (2 * q + 1 < m) tx_root_node(c, left, left + TX_ROOT_NODE_WORDS, out, st, stride);
    else for (uint32_t i = 0; i < TX_ROOT_NODE_WORDS; ++i) out[i] = left[i];
  }
}
// how many nodes a pass of span s leaves of n, and how many passes bring n nodes down to one
ZK_TAPE_HD inline uint64_t tx_root_after_pass(uint64_t n, uint32_t s) { return (n + (1ull << s) - 1) >> s; }
ZK_TAPE_HD inline uint32_t tx_root_passes(uint64_t n, uint32_t s) { uint32_t p = 0; for (; n > 1; n = tx_root_after_pass(n, s)) ++p; return p; }
// the span an environment or a test may ask for: 1 .. TX_ROOT_SPAN, anything else is the default
ZK_TAPE_HD inline uint32_t tx_root_span(long long asked) { return asked >= 1 && asked <= (long long)TX_ROOT_SPAN ? (uint32_t)asked : TX_ROOT_SPAN; }

}  // namespace zkvm
}  // namespace zk

// ===================================================== host side =====================================================
#include <vector>

namespace zk {
namespace zkvm {

constexpr const char* TX_ROOT_LABEL = "ZkVM.txroot";      // (UNPINNED: see the head of the file)

// the freshly initialised transcript of the tree, TAPE_PROTO_WORDS words
inline void tx_root_init(uint32_t out[TAPE_PROTO_WORDS]) { Transcript(TX_ROOT_LABEL).export_state(out); }

// The constants a host fold needs, made once per process (the label table is hash_tape_constants').
struct TxRootHost {
  uint32_t init[TAPE_PROTO_WORDS];
  std::vector<uint8_t> labels;
  TxRootHost() { std::vector<uint32_t> protos; hash_tape_constants(protos, labels); tx_root_init(init); }
  TxRootView view() const { return TxRootView{init, labels.data()}; }
  static const TxRootHost& get() { static const TxRootHost h; return h; }
};

// The root over n IDs (32 bytes each, call order) on the CPU, the way the device walks it: the leaves, then passes of `span`
// levels over aligned spans -- the leaves and the spans of a pass spread over `threads` -- until one node is left.
// n = 0: the empty tree's hash.
inline void tx_root_fold_host(const uint8_t* ids, size_t n, uint32_t span, int threads, uint8_t out[32]) {
  const TxRootView c = TxRootHost::get().view();
  const uint32_t s = tx_root_span(span);
  uint32_t root[TX_ROOT_NODE_WORDS];
  if (n == 0) {
    uint32_t st[50];
    tx_root_empty(c, root, st, 1);
    std::memcpy(out, root, 32);
    return;
  }
  std::vector<uint32_t> a(TX_ROOT_NODE_WORDS * n), b;
  host_parallel((n + 63) / 64, threads, [&](size_t g) {
    uint32_t st[50], id[TX_ROOT_NODE_WORDS];
    for (size_t i = 64 * g; i < std::min(n, 64 * g + 64); ++i) { std::memcpy(id, ids + 32 * i, 32); tx_root_leaf(c, id, &a[TX_ROOT_NODE_WORDS * i], st, 1); }
  });
  size_t m = n;
  while (m > 1) {
    const size_t next = (size_t)tx_root_after_pass(m, s);
    b.assign(TX_ROOT_NODE_WORDS * next, 0);
    host_parallel(next, threads, [&](size_t sp) {
      const size_t first = sp << s;
      uint32_t cnt = (uint32_t)std::min<size_t>((size_t)1 << s, m - first);
      std::vector<uint32_t> x(a.begin() + TX_ROOT_NODE_WORDS * first, a.begin() + TX_ROOT_NODE_WORDS * (first + cnt)), y(TX_ROOT_NODE_WORDS * ((cnt + 1) / 2));
      uint32_t st[50];
      for (uint32_t level = 0; level < s; ++level) {
        tx_root_fold_level(c, x.data(), cnt, y.data(), 0, 1, st, 1);
        cnt = (cnt + 1) / 2;
        x.swap(y);
      }
      std::memcpy(&b[TX_ROOT_NODE_WORDS * sp], x.data(), 32);
    });
    a.swap(b);
    m = next;
  }
  std::memcpy(out, a.data(), 32);
}

}  // namespace zkvm
}  // namespace zk
