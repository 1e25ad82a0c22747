// Does a transaction call write past its caller's status array?  With ZKGPU_TXFORMAT_RETURN_LOG and a window K the array is
// 33 + 1 + 33 K bytes per transaction: this program gives csrc/tx_call.hpp (over the stand-in devices of hostlib.cpp, laid out
// and fail-closed as session.hpp does it: zkhost_txcall_log_selftest) heap arrays of EXACTLY that size, for a sanitizer build:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer
//       tools/tx_log_overrun_check.cpp zkvm_amd/csrc/hostlib.cpp -o tx_log_overrun_check
//   ./tx_log_overrun_check [transactions]
// Every stand-in (0 host-hashed, 1 hashing, 2 chaining) x K in {1, 4, 5, 255} x a lone call (one chunk, chunks of 16, of 8) and two
// callers' pieces merged into one call (each caller an array and a window of its own); a fault at every operation of every
// stage.  Beside the sanitizer's verdict it checks what the arrays hold: status bytes and IDs are those of the call without the
// flag (zkhost_txcall_ids_selftest); a record stands beside status 0, counts the four entries of a 2-in/2-out payment, lists
// them when they fit -- the same bytes from all three stand-ins, whatever the window -- and is zero past them; everything else
// -- and everything after an error -- is zero.  Exit status 0 and "ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

extern "C" {
int zkhost_tx_wrap_many(size_t count, size_t n_in, size_t n_out, const uint8_t* coms, const uint8_t* proofs, size_t proof_len, const uint8_t* seeds,
                        uint64_t mintime0, uint64_t maxtime, int threads, uint8_t* out, size_t cap, uint64_t* offsets);
int zkhost_txcall_ids_selftest(int kind, int return_ids, size_t batch, size_t split, const uint8_t* txs, const uint64_t* offs, const uint8_t* proof_ok,
                               int host_threads, size_t chunk, uint32_t delay_seed, int fail_at, int fail_stage, int n_slots, uint8_t* accept_bitmap,
                               uint8_t* status_a, uint8_t* status_b, uint64_t* out);
int zkhost_txcall_log_selftest(int kind, size_t K, size_t k_b, size_t batch, size_t split, const uint8_t* txs, const uint64_t* offs, const uint8_t* proof_ok,
                               int host_threads, size_t chunk, uint32_t delay_seed, int fail_at, int fail_stage, int n_slots, uint8_t* accept_bitmap,
                               uint8_t* status_a, uint8_t* status_b, uint64_t* out);
}

namespace {

constexpr size_t ENTRIES = 4;                            // a 2-in/2-out payment logs two inputs and two outputs

struct Block {
  size_t n = 0;
  std::vector<uint8_t> blob, proof_ok;
  std::vector<uint64_t> offs;
};

// n signed 2-in/2-out payments around arbitrary statement bytes; one truncated, one of a later version, one with another
// mintime than it was signed with, one whose proof the stand-in's table rejects
bool make_block(size_t n, Block& b) {
  const size_t proof_len = 97;
  std::vector<uint8_t> coms(256 * n), proofs(proof_len * n), seeds(32 * n);
  uint32_t x = 54321;
  auto next = [&] { x = x * 1664525u + 1013904223u; return (uint8_t)(x >> 24); };
  for (auto& c : coms) c = next();
  for (auto& c : proofs) c = next();
  for (auto& c : seeds) c = next();
  std::vector<uint8_t> blob(4096 * n);
  std::vector<uint64_t> offs(n + 1);
  if (zkhost_tx_wrap_many(n, 2, 2, coms.data(), proofs.data(), proof_len, seeds.data(), 5, 1000000000ull, 2, blob.data(), blob.size(), offs.data()) != 0) return false;
  b.n = n;
  b.offs.assign(1, 0);
  b.proof_ok.assign(n, 1);
  for (size_t i = 0; i < n; ++i) {
    std::vector<uint8_t> tx(blob.begin() + (long)offs[i], blob.begin() + (long)offs[i + 1]);
    if (i == 3) tx.pop_back();                           // rejected by the host
    if (i == 5) tx[0] = 2;                               // a later version: outside the subset
    if (i == 9) tx[8] ^= 1;                              // another mintime: the ID changes, the signature fails
    if (i == 12) b.proof_ok[i] = 0;                      // the proof fails
    b.blob.insert(b.blob.end(), tx.begin(), tx.end());
    b.offs.push_back(b.blob.size());
  }
  return true;
}

// per transaction: status, ID, count and the entries (kind + ID, 33 bytes each) its record holds
struct Result { int rc = 0; std::vector<uint8_t> bits, status, ids, count; std::vector<std::vector<uint8_t>> entries; uint64_t out[6] = {0}; bool tail_zero = true; };

void take(Result& r, const uint8_t* s, size_t n, size_t K) {
  r.status.insert(r.status.end(), s, s + n);
  r.ids.insert(r.ids.end(), s + n, s + 33 * n);
  for (size_t i = 0; i < n; ++i) {
    const uint8_t* rec = s + 33 * n + i * (1 + 33 * K);
    const size_t held = rec[0] <= K ? rec[0] : 0;
    r.count.push_back(rec[0]);
    std::vector<uint8_t> e;
    for (size_t j = 0; j < held; ++j) { e.push_back(rec[1 + j]); e.insert(e.end(), rec + 1 + K + 32 * j, rec + 1 + K + 32 * j + 32); }
    r.entries.push_back(e);
    for (size_t j = held; j < K; ++j) {
      if (rec[1 + j]) r.tail_zero = false;
      for (size_t q = 0; q < 32; ++q) if (rec[1 + K + 32 * j + q]) r.tail_zero = false;
    }
  }
}

// one call with arrays of exactly the size the layout asks for (new[]: the sanitizer guards both ends)
Result run(const Block& b, int kind, size_t K, size_t k_b, size_t split, size_t chunk, int fail_at, int fail_stage, uint32_t seed) {
  const size_t na = split ? split : b.n, nb = split ? b.n - split : 0, kb = k_b ? k_b : K;
  std::unique_ptr<uint8_t[]> sa(new uint8_t[na * (34 + 33 * K)]), sb(nb ? new uint8_t[nb * (34 + 33 * kb)] : nullptr), bm(new uint8_t[(b.n + 7) / 8]);
  Result r;
  r.rc = zkhost_txcall_log_selftest(kind, K, k_b, b.n, split, b.blob.data(), b.offs.data(), b.proof_ok.data(), 2, chunk, seed, fail_at, fail_stage, 2, bm.get(),
                                    sa.get(), sb.get(), r.out);
  r.bits.assign(bm.get(), bm.get() + (b.n + 7) / 8);
  take(r, sa.get(), na, K);
  if (nb) take(r, sb.get(), nb, kb);
  return r;
}

#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "  (%s)\n", #cond); return false; } } while (0)

// want: the call without the flag (status bytes, IDs); full: the records of a window every transaction fits (empty: none yet)
bool check(const Block& b, const Result& want, const Result* full, const Result& r, int kind, size_t K, size_t k_b, size_t split, const char* what) {
  EXPECT(r.tail_zero, "%s kind %d K %zu: bytes past a record's entries\n", what, kind, K);
  EXPECT(r.out[1] == 0, "%s kind %d: a staged chunk leaked\n", what, kind);
  if (r.rc != 0) {                                       // fail-closed: nothing accepted, no reason, no ID, no record
    for (uint8_t c : r.bits) EXPECT(c == 0, "%s kind %d: a bit after an error\n", what, kind);
    for (size_t i = 0; i < b.n; ++i) EXPECT(r.status[i] == 1 || (r.status[i] == 2 && want.status[i] == 2), "%s kind %d: status %d at %zu after an error\n", what, kind, r.status[i], i);
    for (uint8_t c : r.ids) EXPECT(c == 0, "%s kind %d: an ID byte after an error\n", what, kind);
    for (size_t i = 0; i < b.n; ++i) EXPECT(r.count[i] == 0 && r.entries[i].empty(), "%s kind %d: a record at %zu after an error\n", what, kind, i);
    EXPECT(r.out[5] == 0, "%s kind %d: the failed call had written into an ID or record area\n", what, kind);
    return true;
  }
  EXPECT(r.bits == want.bits && r.status == want.status && r.ids == want.ids, "%s kind %d K %zu: verdicts or IDs differ from the unflagged call's\n", what, kind, K);
  for (size_t i = 0; i < b.n; ++i) {
    const size_t k = split && i >= split && k_b ? k_b : K;
    if (r.status[i] != 0) { EXPECT(r.count[i] == 0 && r.entries[i].empty(), "%s kind %d: a record beside status %d at %zu\n", what, kind, r.status[i], i); continue; }
    EXPECT(r.count[i] == ENTRIES, "%s kind %d K %zu: %d entries at %zu\n", what, kind, k, r.count[i], i);
    EXPECT(r.entries[i].size() == (k >= ENTRIES ? 33 * ENTRIES : 0), "%s kind %d K %zu: %zu entry bytes at %zu\n", what, kind, k, r.entries[i].size(), i);
    if (k < ENTRIES) continue;
    const uint8_t kinds[ENTRIES] = {1, 1, 2, 2};
    for (size_t j = 0; j < ENTRIES; ++j) {
      EXPECT(r.entries[i][33 * j] == kinds[j], "%s kind %d: kind %d of entry %zu at %zu\n", what, kind, r.entries[i][33 * j], j, i);
      bool zero = true;
      for (size_t q = 1; q <= 32; ++q) zero &= r.entries[i][33 * j + q] == 0;
      EXPECT(!zero, "%s kind %d: a zero contract ID, entry %zu at %zu\n", what, kind, j, i);
    }
    if (full) EXPECT(r.entries[i] == full->entries[i], "%s kind %d K %zu: the entries at %zu differ from the host-hashed ones\n", what, kind, k, i);
  }
  if (kind == 0) EXPECT(r.out[2] == b.n && r.out[4] == 0, "%s kind 0: %llu hashed on the host\n", what, (unsigned long long)r.out[2]);
  if (kind >= 1) EXPECT(r.out[2] == 0 && r.out[3] > 0, "%s kind %d: %llu transactions hashed on the host\n", what, kind, (unsigned long long)r.out[2]);
  if (kind >= 1) EXPECT((r.out[4] > 0) == (K >= ENTRIES || (split && k_b >= ENTRIES)), "%s kind %d K %zu: %llu entries gathered\n", what, kind, K, (unsigned long long)r.out[4]);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? (size_t)atoll(argv[1]) : 24;
  if (n < 24) { fprintf(stderr, "at least 24 transactions\n"); return 2; }
  Block b;
  if (!make_block(n, b)) { fprintf(stderr, "the builder failed\n"); return 1; }
  // the call without the new flag: status bytes and IDs
  Result want;
  {
    std::unique_ptr<uint8_t[]> st(new uint8_t[33 * n]), bm(new uint8_t[(n + 7) / 8]);
    want.rc = zkhost_txcall_ids_selftest(0, 1, n, 0, b.blob.data(), b.offs.data(), b.proof_ok.data(), 2, 0, 1, -1, 0, 2, bm.get(), st.get(), nullptr, want.out);
    want.bits.assign(bm.get(), bm.get() + (n + 7) / 8);
    want.status.assign(st.get(), st.get() + n);
    want.ids.assign(st.get() + n, st.get() + 33 * n);
  }
  if (want.rc != 0) { fprintf(stderr, "the plain call failed: %d\n", want.rc); return 1; }
  size_t accepted = 0;
  for (uint8_t s : want.status) accepted += s == 0;
  if (accepted + 4 != n || want.status[3] != 1 || want.status[5] != 2 || want.status[9] != 1 || want.status[12] != 1) { fprintf(stderr, "the block is not what it was built to be\n"); return 1; }
  const Result full = run(b, 0, 5, 0, 0, 0, -1, 0, 2);
  if (!check(b, want, nullptr, full, 0, 5, 0, 0, "first")) return 1;
  size_t calls = 1;
  for (int kind = 0; kind < 3; ++kind) {
    for (size_t K : {(size_t)1, (size_t)4, (size_t)5, (size_t)255}) {
      const size_t shapes[6][3] = {{0, 0, 0}, {0, 16, 0}, {0, 8, 0}, {16, 0, 0}, {16, 16, 3}, {8, 8, 9}};     // (split, chunk, the second caller's window)
      for (const auto& sh : shapes) {
        if (!check(b, want, &full, run(b, kind, K, sh[2], sh[0], sh[1], -1, 0, (uint32_t)(7 + calls)), kind, K, sh[2], sh[0], sh[0] ? "merged" : "lone")) return 1;
        ++calls;
      }
    }
    // a fault at every operation of every stage the stand-in has, lone and merged (windows 5 and 3), in chunks of 16
    for (int stage = 0; stage <= kind; ++stage)
      for (size_t split : {(size_t)0, (size_t)16})
        for (int k = 0;; ++k) {
          const Result r = run(b, kind, 5, 3, split, 16, k, stage, (uint32_t)(100 + k));
          if (!check(b, want, &full, r, kind, 5, 3, split, "faulted")) return 1;
          ++calls;
          if (r.rc == 0) break;                          // (the k-th operation does not exist: the call ran clean)
          if (k > 400) { fprintf(stderr, "a call that never runs clean\n"); return 1; }
        }
  }
  printf("ok: %zu calls over %zu transactions\n", calls, n);
  return 0;
}
