// The side table and the level interpreter of csrc/tx_hash_levels.hpp on their own, for a sanitizer build:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -Izkvm_amd/csrc \
//       tools/tx_precompute_check.cpp -o tx_precompute_check && ./tx_precompute_check [copies per shape] [seed]
// Payments of the shapes 1x1, 2x2, 3x1, 1x3, 4x4, 8x8 and 1x16 (built and signed by zkvm_tx_build.hpp around arbitrary statement
// bytes), shuffled into ONE chunk with a few truncated ones among them, flattened by the taped pass of a precompute-only call
// (no job run on the host).  The table must order every shape's jobs topologically and give each its place in the byte run;
// the tape walked level by level with T and with T / 2 lanes per transaction must leave every slot word and every ID word as
// tx_hash_run does.  Then the interpreter is handed what it must not trust: a tape cut short (the head's counts lowered under
// its transactions), a table cut short, and a tape whose records name shapes, slots, jobs and runs beyond its sections -- in
// exact-size heap copies, so that a read outside them is the sanitizer's to report.  Exit status 0 and "ok" on success.
#include "tx_hash_levels.hpp"
#include "zkvm_tx_build.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>

using namespace zk::zkvm;

static int fail(const char* what) { fprintf(stderr, "%s\n", what); return 1; }

// every slot piece's producer has a lower level, every job is listed once at its level, and its run offset is the sum of the
// TAPE_RUN lengths of the jobs before it
static bool table_is_topological(const uint32_t* b, const std::vector<uint32_t>& table, bool* wide) {
  const HashTapeHead& h = *(const HashTapeHead*)b;
  if (table.size() < 4 + (size_t)h.n_shapes || table[0] != TAPE_LEVELS_MAGIC || table[1] != h.n_shapes || table[2] != table.size()) return false;
  for (uint32_t s = 0; s < h.n_shapes; ++s) {
    const uint32_t* sh = b + h.shapes + 4 * s;
    const uint32_t* tab = table.data() + table[4 + s];
    const uint32_t L = tab[0], J = tab[1];
    if (J != sh[1] || L == 0 || L > J || tab[2] != 0 || tab[2 + L] != J) return false;
    const uint32_t* order = tab + 2 + L + 1;
    std::vector<uint32_t> level(J, TAPE_IDLE), offset(J, 0), producer(sh[2], TAPE_IDLE);
    for (uint32_t l = 0; l < L; ++l) {
      if (tab[2 + l] >= tab[2 + l + 1]) return false;                          // (no empty level)
      if (tab[2 + l + 1] - tab[2 + l] > TAPE_LEVEL_LANES) *wide = true;
      for (uint32_t q = tab[2 + l]; q < tab[2 + l + 1]; ++q) {
        if (order[2 * q] >= J || level[order[2 * q]] != TAPE_IDLE) return false;
        level[order[2 * q]] = l; offset[order[2 * q]] = order[2 * q + 1];
      }
    }
    uint32_t cursor = 0;
    for (uint32_t j = 0; j < J; ++j) {
      const uint32_t* job = b + h.jobs + 4 * (sh[0] + j);
      if (level[j] == TAPE_IDLE || offset[j] != cursor) return false;
      uint32_t need = 0;
      for (uint32_t p = job[2]; p < job[2] + job[3]; ++p) {
        const uint32_t* pc = b + h.pieces + 4 * p;
        if ((pc[0] >> 8) != TAPE_SLOT) { cursor += pc[1]; continue; }
        if (producer[pc[3]] == TAPE_IDLE) continue;
        if (level[producer[pc[3]]] >= level[j]) return false;
        need = std::max(need, level[producer[pc[3]]] + 1);
      }
      if (level[j] != need) return false;                                      // (the lowest level its producers allow)
      producer[job[1]] = j;
    }
  }
  return true;
}

int main(int argc, char** argv) {
  const size_t copies = argc > 1 ? (size_t)atoll(argv[1]) : 9;
  std::mt19937_64 rng(argc > 2 ? (uint64_t)atoll(argv[2]) : 1);
  static const size_t shapes[7][2] = {{1, 1}, {2, 2}, {3, 1}, {1, 3}, {4, 4}, {8, 8}, {1, 16}};
  std::vector<uint32_t> protos;
  std::vector<uint8_t> labels;
  hash_tape_constants(protos, labels);
  (void)base_table();
  std::vector<std::vector<uint8_t>> txs;
  for (const auto& ab : shapes)
    for (size_t c = 0; c < copies; ++c) {
      std::vector<uint8_t> com(64 * (ab[0] + ab[1])), proof(1 + rng() % 200);
      uint8_t seed[32];
      for (auto& x : com) x = (uint8_t)rng();
      for (auto& x : proof) x = (uint8_t)rng();
      for (auto& x : seed) x = (uint8_t)rng();
      txs.push_back(tx_wrap_payment(ab[0], ab[1], com.data(), proof.data(), proof.size(), seed, rng() % 1000, 1000 + rng() % 1000));
      if (txs.back().empty()) return fail("builder failed");
      if (rng() % 11 == 0) txs.back().resize(txs.back().size() - 1 - rng() % 40);       // rejected by the host: not on the tape
    }
  std::shuffle(txs.begin(), txs.end(), rng);
  const size_t n = txs.size();
  std::vector<TxStatement> st(n);
  TxHashTape tape;
  tape.reset(n);
  std::atomic<int> bad{0};
  zk::host_parallel((n + 7) / 8, 3, [&](size_t g) {
    const uint8_t* p[8]; size_t l[8];
    const size_t first = 8 * g, cnt = std::min<size_t>(8, n - first);
    for (size_t q = 0; q < cnt; ++q) { p[q] = txs[first + q].data(); l[q] = txs[first + q].size(); }
    if (!tx_prepare_many_taped(p, l, &st[first], cnt, tape, first, NO_PROTO)) bad = 1;
  });
  if (bad) return fail("a plan the tape cannot hold");
  tape.finish(3);
  const HashTapeHead& h = tape.head();
  if (!hash_tape_check(tape.block(), h.words)) return fail("the block fails hash_tape_check");
  std::vector<uint32_t> table, slots, ids, lslots, lids;
  if (!tx_hash_levels_table(tape.block(), table)) return fail("no side table");
  bool wide = false;
  if (!table_is_topological(tape.block(), table, &wide)) return fail("the side table is no topological order");
  if (!wide) return fail("no level wider than T among the shapes");
  hash_tape_run_host(tape.block(), protos, labels, slots, ids);
  for (uint32_t lanes : {TAPE_LEVEL_LANES, TAPE_LEVEL_LANES / 2}) {
    if (!hash_tape_run_levels_host(tape.block(), protos, labels, lanes, lslots, lids)) return fail("the level walk refused the tape");
    if (lslots != slots || lids != ids) return fail("the level walk and tx_hash_run differ");
  }

  // ---- what the interpreter must not trust, in exact-size copies
  const auto walk = [&](const std::vector<uint32_t>& blk, const std::vector<uint32_t>& tab, uint32_t n_tx_asked) {
    const HashTapeHead& hh = *(const HashTapeHead*)blk.data();
    std::vector<uint32_t> sl(8 * (size_t)hh.n_slots + 8, 0), id(8 * (size_t)hh.n_tx + 8, 0);
    std::vector<uint32_t> exact_tab(tab);
    exact_tab.shrink_to_fit();
    HashTapeView v{blk.data(), protos.data(), labels.data(), sl.data(), id.data()};
    const HashLevelsView lv{exact_tab.data(), (uint32_t)exact_tab.size()};
    uint32_t stt[50];
    for (uint32_t level = 0; level < table[3] + 1; ++level)
      for (uint32_t tx = 0; tx < n_tx_asked; ++tx)
        for (uint32_t sub = 0; sub < TAPE_LEVEL_LANES; ++sub) tx_hash_level_run(v, lv, tx, sub, TAPE_LEVEL_LANES, level, stt, 1);
  };
  const std::vector<uint32_t> block(tape.block(), tape.block() + h.words);
  {                                                        // a truncated tape: fewer transactions, slots, jobs, pieces and bytes than its records name
    std::vector<uint32_t> cut(block);
    HashTapeHead& ch = *(HashTapeHead*)cut.data();
    ch.n_tx /= 2; ch.n_slots /= 3; ch.n_jobs /= 2; ch.n_pieces /= 2; ch.data_bytes /= 2;
    walk(cut, table, h.n_tx + 5);
  }
  {                                                        // a truncated table
    for (size_t keep : {(size_t)0, (size_t)3, (size_t)4, 4 + (size_t)h.n_shapes, table.size() / 2, table.size() - 1})
      walk(block, std::vector<uint32_t>(table.begin(), table.begin() + std::min(keep, table.size())), h.n_tx);
  }
  {                                                        // an oversized tape: records that point beyond every section
    std::vector<uint32_t> big(block);
    HashTapeHead& bh = *(HashTapeHead*)big.data();
    for (uint32_t t = 0; t < bh.n_tx; ++t) {
      uint32_t* rec = big.data() + bh.txs + 4 * t;
      if (t % 4 == 0) rec[0] = bh.n_shapes + t;            // a shape that is not there
      if (t % 4 == 1) rec[1] = bh.data_bytes - 1;           // a run that ends past the data
      if (t % 4 == 2) rec[2] = bh.n_slots - 1;              // a slot area that ends past the slots
    }
    for (uint32_t j = 0; j < bh.n_jobs; j += 3) (big.data() + bh.jobs + 4 * j)[1] = 0x7fffffffu;       // an out slot far outside
    for (uint32_t p = 0; p < bh.n_pieces; p += 5) (big.data() + bh.pieces + 4 * p)[3] = 0x7fffffffu;   // a slot piece far outside
    for (uint32_t p = 1; p < bh.n_pieces; p += 5) (big.data() + bh.pieces + 4 * p)[1] = 0x7fffffffu;   // a run piece far too long
    walk(big, table, bh.n_tx);
    std::vector<uint32_t> tab(table);
    for (size_t i = 4; i < tab.size(); i += 7) tab[i] = 0xfffffff0u;                                    // ... and a table that does the same
    walk(block, tab, h.n_tx);
  }
  printf("ok: %zu transactions, %u on the tape in %u shapes, %u levels at most\n", n, h.n_tx, h.n_shapes, table[3]);
  return 0;
}
