// The flattener and the interpreter of csrc/tx_hash_tape.hpp on their own, for a sanitizer build:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -Izkvm_amd/csrc \
//       tools/tx_hash_tape_selftest.cpp -o tx_hash_tape_selftest && ./tx_hash_tape_selftest [transactions] [seed]
// Seeded random payments (arities 1 .. 6 on either side, built and signed by zkvm_tx_build.hpp around arbitrary statement
// bytes), some truncated, in chunks of random size and scrambled order: every chunk is flattened on 1 .. 4 threads, the
// block must pass hash_tape_check, and every slot the tape's three protocols write -- the transaction ID among them -- must
// equal what run_plan writes for the same plan.  Exit status 0 and "ok" on success.
#include "tx_hash_tape.hpp"
#include "zkvm_tx_build.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace zk::zkvm;

int main(int argc, char** argv) {
  const size_t total = argc > 1 ? (size_t)atoll(argv[1]) : 3000;
  std::mt19937_64 rng(argc > 2 ? (uint64_t)atoll(argv[2]) : 1);
  std::vector<uint32_t> protos, slots, ids;
  std::vector<uint8_t> labels;
  hash_tape_constants(protos, labels);
  (void)base_table();
  TxHashTape tape;
  size_t done = 0, chunks = 0, shapes_seen = 0;
  while (done < total) {
    const size_t n = std::min<size_t>(total - done, 1 + rng() % 300);
    std::vector<std::vector<uint8_t>> txs(n);
    for (size_t i = 0; i < n; ++i) {
      const size_t a = 1 + rng() % 6, b = 1 + rng() % 6;
      std::vector<uint8_t> com(64 * (a + b)), proof(1 + rng() % 200);
      uint8_t seed[32];
      for (auto& c : com) c = (uint8_t)rng();
      for (auto& c : proof) c = (uint8_t)rng();
      for (auto& c : seed) c = (uint8_t)rng();
      txs[i] = tx_wrap_payment(a, b, com.data(), proof.data(), proof.size(), seed, rng() % 1000, 1000 + rng() % 1000);
      if (txs[i].empty()) { fprintf(stderr, "builder failed\n"); return 1; }
      if (rng() % 37 == 0) txs[i].resize(txs[i].size() - 1 - rng() % 40);        // rejected by the host: not on the tape
    }
    std::vector<TxStatement> st(n);
    tape.reset(n);
    const int threads = 1 + (int)(rng() % 4);
    std::atomic<int> bad{0};
    zk::host_parallel((n + 7) / 8, threads, [&](size_t g) {
      const uint8_t* p[8]; size_t l[8];
      const size_t first = 8 * g, cnt = std::min<size_t>(8, n - first);
      for (size_t q = 0; q < cnt; ++q) { p[q] = txs[first + q].data(); l[q] = txs[first + q].size(); }
      if (!tx_prepare_many_taped(p, l, &st[first], cnt, tape, first)) bad = 1;
    });
    if (bad) { fprintf(stderr, "a plan the tape cannot hold\n"); return 1; }
    tape.finish(threads);
    const HashTapeHead& h = tape.head();
    if (!hash_tape_check(tape.block(), h.words)) { fprintf(stderr, "chunk %zu: the block fails hash_tape_check\n", chunks); return 1; }
    hash_tape_run_host(tape.block(), protos, labels, slots, ids);
    size_t live = 0;
    for (size_t i = 0; i < n; ++i) live += st[i].status == TX_OK;
    if (live != tape.n_tx()) { fprintf(stderr, "chunk %zu: %zu live, %zu on the tape\n", chunks, live, tape.n_tx()); return 1; }
    TxPlan P; TxSlots out; TxStatement s2;
    std::vector<uint8_t> want;
    for (size_t t = 0; t < tape.n_tx(); ++t) {
      const size_t i = tape.position(t);
      const uint32_t* rec = tape.block() + h.txs + 4 * t;
      P.only = 0xff;
      tx_structure(txs[i].data(), txs[i].size(), s2, P, out);
      want.assign(32 * (size_t)P.n_slots + 32, 0);
      run_plan(P, want.data());
      for (const HashJob& j : P.jobs)
        if (tape_keeps(j.proto) && memcmp(&slots[8 * ((size_t)rec[2] + j.out_slot)], &want[32 * (size_t)j.out_slot], 32) != 0) {
          fprintf(stderr, "chunk %zu transaction %zu slot %u differs\n", chunks, i, j.out_slot);
          return 1;
        }
      if (memcmp(&ids[8 * t], &want[32 * (size_t)out.txid], 32) != 0) { fprintf(stderr, "chunk %zu transaction %zu: ID differs\n", chunks, i); return 1; }
    }
    shapes_seen += h.n_shapes;
    done += n; ++chunks;
  }
  printf("ok: %zu transactions in %zu chunks, %zu shape runs\n", done, chunks, shapes_seen);
  return 0;
}
