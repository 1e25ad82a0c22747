// k_tx_hash and k_tx_hash_levels ALONE on one tape: the hashing stage of a transaction call with nothing around it.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -Izkvm_amd/csrc tools/tx_hash_bench.hip -o tx_hash_bench
//   ./tx_hash_bench run|levels [transactions ...]          (default: 1024 8192)
// Per size: that many DISTINCT 2-in / 2-out payments (built and signed by zkvm_tx_build.hpp around seeded statement bytes),
// flattened as a precompute-only call flattens them (no job run on the host), the tape and, for `levels`, its side table copied
// up once; then 3 warm launches and 25 timed ones, each between two HIP events of its own on an otherwise idle stream.  One
// kernel per process: a comparison alternates fresh processes.  The IDs the last launch left are held
// against tx_hash_run on the host.  One line per size:  kernel n min_us median_us max_us
#include "tx_hash_kernels.hpp"
#include "tx_hash_levels.hpp"
#include "zkvm_tx_build.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace zk::zkvm;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
  if (argc < 2 || (strcmp(argv[1], "run") && strcmp(argv[1], "levels"))) { fprintf(stderr, "usage: tx_hash_bench run|levels [transactions ...]\n"); return 2; }
  const bool levels = strcmp(argv[1], "levels") == 0;
  std::vector<size_t> sizes;
  for (int a = 2; a < argc; ++a) sizes.push_back((size_t)atoll(argv[a]));
  if (sizes.empty()) sizes = {1024, 8192};
  std::vector<uint32_t> protos;
  std::vector<uint8_t> labels;
  hash_tape_constants(protos, labels);
  (void)base_table();
  void* d_const = nullptr;
  CHECK(hipMalloc(&d_const, 4 * protos.size() + labels.size()));
  CHECK(hipMemcpy(d_const, protos.data(), 4 * protos.size(), hipMemcpyHostToDevice));
  CHECK(hipMemcpy((char*)d_const + 4 * protos.size(), labels.data(), labels.size(), hipMemcpyHostToDevice));
  hipStream_t stream;
  CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  for (const size_t n : sizes) {
    std::mt19937_64 rng(n);
    std::vector<std::vector<uint8_t>> txs(n);
    for (size_t i = 0; i < n; ++i) {
      std::vector<uint8_t> com(64 * 4), proof(641);
      uint8_t seed[32];
      for (auto& c : com) c = (uint8_t)rng();
      for (auto& c : proof) c = (uint8_t)rng();
      for (auto& c : seed) c = (uint8_t)rng();
      txs[i] = tx_wrap_payment(2, 2, com.data(), proof.data(), proof.size(), seed, rng() % 1000, 1000 + rng() % 1000);
      if (txs[i].empty()) { fprintf(stderr, "builder failed\n"); return 1; }
    }
    std::vector<TxStatement> st(n);
    TxHashTape tape;
    tape.reset(n);
    bool ok = true;
    for (size_t first = 0; first < n; first += 8) {
      const uint8_t* p[8]; size_t l[8];
      const size_t cnt = std::min<size_t>(8, n - first);
      for (size_t q = 0; q < cnt; ++q) { p[q] = txs[first + q].data(); l[q] = txs[first + q].size(); }
      ok &= tx_prepare_many_taped(p, l, &st[first], cnt, tape, first, NO_PROTO);
    }
    tape.finish(4);
    const HashTapeHead& h = tape.head();
    std::vector<uint32_t> table, want_slots, want_ids;
    if (!ok || h.n_tx != n || !hash_tape_check(tape.block(), h.words) || !tx_hash_levels_table(tape.block(), table)) { fprintf(stderr, "no tape\n"); return 1; }
    hash_tape_run_host(tape.block(), protos, labels, want_slots, want_ids);
    void *d_tape = nullptr, *d_slots = nullptr, *d_txid = nullptr, *d_table = nullptr;
    CHECK(hipMalloc(&d_tape, tape.bytes()));
    CHECK(hipMalloc(&d_slots, 32 * (size_t)h.n_slots + 32));
    CHECK(hipMalloc(&d_txid, 32 * n));
    CHECK(hipMalloc(&d_table, 4 * table.size()));
    CHECK(hipMemcpy(d_tape, tape.block(), tape.bytes(), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_table, table.data(), 4 * table.size(), hipMemcpyHostToDevice));
    const HashTapeView view{(const uint32_t*)d_tape, (const uint32_t*)d_const, (const uint8_t*)d_const + 4 * protos.size(), (uint32_t*)d_slots, (uint32_t*)d_txid};
    const HashLevelsView lv{(const uint32_t*)d_table, (uint32_t)table.size()};
    std::vector<float> us;
    for (int rep = 0; rep < 3 + 25; ++rep) {
      CHECK(hipMemsetAsync(d_slots, 0, 32 * (size_t)h.n_slots + 32, stream));
      CHECK(hipMemsetAsync(d_txid, 0, 32 * n, stream));
      CHECK(hipEventRecord(e0, stream));
      if (levels) hipLaunchKernelGGL(zk::k_tx_hash_levels, dim3(h.n_lanes / (64 / TAPE_LEVEL_LANES)), dim3(64), 0, stream, view, lv, h.n_lanes);
      else hipLaunchKernelGGL(zk::k_tx_hash, dim3(h.n_lanes / 64), dim3(64), 0, stream, view, h.n_lanes);
      CHECK(hipGetLastError());
      CHECK(hipEventRecord(e1, stream));
      CHECK(hipStreamSynchronize(stream));
      float ms = 0;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      if (rep >= 3) us.push_back(1e3f * ms);
    }
    std::vector<uint32_t> got(8 * n);
    CHECK(hipMemcpy(got.data(), d_txid, 32 * n, hipMemcpyDeviceToHost));
    if (memcmp(got.data(), want_ids.data(), 32 * n) != 0) { fprintf(stderr, "%s: the IDs differ from tx_hash_run's at %zu transactions\n", argv[1], n); return 1; }
    std::sort(us.begin(), us.end());
    printf("%s %zu min_us %.1f median_us %.1f max_us %.1f\n", levels ? "k_tx_hash_levels" : "k_tx_hash", n, us.front(), us[us.size() / 2], us.back());
    CHECK(hipFree(d_tape)); CHECK(hipFree(d_slots)); CHECK(hipFree(d_txid)); CHECK(hipFree(d_table));
  }
  return 0;
}
