// Does a transaction call write past its caller's status array?  With ZKGPU_TXFORMAT_RETURN_IDS the array is 33 bytes per
// transaction, without it one: this program gives csrc/tx_call.hpp (over the stand-in devices of hostlib.cpp, laid out and
// fail-closed as session.hpp does it: zkhost_txcall_ids_selftest) heap arrays of EXACTLY that size, for a sanitizer build:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer
//       tools/tx_ids_overrun_check.cpp zkvm_amd/csrc/hostlib.cpp -o tx_ids_overrun_check
//   ./tx_ids_overrun_check [transactions]
// Every stand-in (0 host-hashed, 1 hashing, 2 chaining) x without / with the flag x a lone call (one chunk, chunks of 16, of 1) and
// two callers' pieces merged into one call (each caller an array of its own); with the flag, also a fault at every operation
// of every stage.  Beside the sanitizer's verdict it checks what the arrays hold: the status bytes do not depend on the flag,
// an ID stands beside status 0 and is the one zkhost_tx_prepare computes, everything else -- and everything after an error --
// is zero.  Exit status 0 and "ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

extern "C" {
int zkhost_tx_wrap_many(size_t count, size_t n_in, size_t n_out, const uint8_t* coms, const uint8_t* proofs, size_t proof_len, const uint8_t* seeds,
                        uint64_t mintime0, uint64_t maxtime, int threads, uint8_t* out, size_t cap, uint64_t* offsets);
int zkhost_tx_prepare(const uint8_t* tx, size_t len, uint8_t txid[32], uint32_t* n_in, uint32_t* n_out, uint8_t* commitments, size_t com_cap,
                      uint8_t* sig_scalars, uint8_t* sig_points, size_t sig_cap, size_t* n_sig, size_t* proof_offset, size_t* proof_len);
int zkhost_txcall_ids_selftest(int kind, int return_ids, size_t batch, size_t split, const uint8_t* txs, const uint64_t* offs, const uint8_t* proof_ok,
                               int host_threads, size_t chunk, uint32_t delay_seed, int fail_at, int fail_stage, int n_slots, uint8_t* accept_bitmap,
                               uint8_t* status_a, uint8_t* status_b, uint64_t* out);
}

namespace {

struct Block {
  size_t n = 0;
  std::vector<uint8_t> blob, proof_ok, txid;             // txid: 32 bytes per transaction, zero where the host VM does not accept it
  std::vector<uint64_t> offs;
};

// n signed 2-in/2-out payments around arbitrary statement bytes; one truncated, one of a later version, one with another
// mintime than it was signed with, one whose proof the stand-in's table rejects
bool make_block(size_t n, Block& b) {
  const size_t proof_len = 97;
  std::vector<uint8_t> coms(256 * n), proofs(proof_len * n), seeds(32 * n);
  uint32_t x = 12345;
  auto next = [&] { x = x * 1664525u + 1013904223u; return (uint8_t)(x >> 24); };
  for (auto& c : coms) c = next();
  for (auto& c : proofs) c = next();
  for (auto& c : seeds) c = next();
  std::vector<uint8_t> blob(4096 * n);
  std::vector<uint64_t> offs(n + 1);
  if (zkhost_tx_wrap_many(n, 2, 2, coms.data(), proofs.data(), proof_len, seeds.data(), 5, 1000000000ull, 2, blob.data(), blob.size(), offs.data()) != 0) return false;
  // the damages change lengths: the block is laid out again
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
  b.txid.assign(32 * n, 0);
  for (size_t i = 0; i < n; ++i) {
    uint8_t com[64 * 32], sc[32 * 40], pt[32 * 40];
    uint32_t a = 0, c = 0;
    size_t n_sig = 0, po = 0, pl = 0;
    uint8_t id[32];
    if (zkhost_tx_prepare(b.blob.data() + b.offs[i], (size_t)(b.offs[i + 1] - b.offs[i]), id, &a, &c, com, sizeof com, sc, pt, 40, &n_sig, &po, &pl) == 0)
      std::memcpy(&b.txid[32 * i], id, 32);
  }
  return true;
}

struct Result { int rc = 0; std::vector<uint8_t> bits, status, ids; uint64_t out[6] = {0}; };

// one call with arrays of exactly the size the layout asks for (new[]: the sanitizer guards both ends)
Result run(const Block& b, int kind, bool flag, size_t split, size_t chunk, int fail_at, int fail_stage, uint32_t seed) {
  const size_t na = split ? split : b.n, nb = split ? b.n - split : 0, per = flag ? 33 : 1;
  std::unique_ptr<uint8_t[]> sa(new uint8_t[per * na]), sb(nb ? new uint8_t[per * nb] : nullptr), bm(new uint8_t[(b.n + 7) / 8]);
  Result r;
  r.rc = zkhost_txcall_ids_selftest(kind, flag, b.n, split, b.blob.data(), b.offs.data(), b.proof_ok.data(), 2, chunk, seed, fail_at, fail_stage, 2, bm.get(),
                                    sa.get(), sb.get(), r.out);
  r.bits.assign(bm.get(), bm.get() + (b.n + 7) / 8);
  r.status.assign(sa.get(), sa.get() + na);
  if (nb) r.status.insert(r.status.end(), sb.get(), sb.get() + nb);
  if (flag) {
    r.ids.assign(sa.get() + na, sa.get() + 33 * na);
    if (nb) r.ids.insert(r.ids.end(), sb.get() + nb, sb.get() + 33 * nb);
  }
  return r;
}

#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "  (%s)\n", #cond); return false; } } while (0)

bool check(const Block& b, const Result& want, const Result& r, int kind, bool flag, const char* what) {
  if (r.rc != 0) {                                       // fail-closed: nothing accepted, no reason, no ID
    for (uint8_t c : r.bits) EXPECT(c == 0, "%s kind %d: a bit after an error\n", what, kind);
    for (size_t i = 0; i < b.n; ++i) EXPECT(r.status[i] == 1 || (r.status[i] == 2 && want.status[i] == 2), "%s kind %d: status %d at %zu after an error\n", what, kind, r.status[i], i);
    for (uint8_t c : r.ids) EXPECT(c == 0, "%s kind %d: an ID byte after an error\n", what, kind);
    EXPECT(r.out[5] == 0, "%s kind %d: the failed call had written into an ID area\n", what, kind);
    EXPECT(r.out[1] == 0, "%s kind %d: a staged chunk leaked\n", what, kind);
    return true;
  }
  EXPECT(r.bits == want.bits && r.status == want.status, "%s kind %d flag %d: verdicts differ from the plain call's\n", what, kind, (int)flag);
  EXPECT(r.out[1] == 0, "%s kind %d: a staged chunk leaked\n", what, kind);
  if (flag) {
    for (size_t i = 0; i < b.n; ++i) {
      const bool ok = r.status[i] == 0;
      EXPECT(ok == (((r.bits[i / 8] >> (i % 8)) & 1) != 0), "%s kind %d: status and bit disagree at %zu\n", what, kind, i);
      const uint8_t zero[32] = {0};
      EXPECT(std::memcmp(&r.ids[32 * i], ok ? &b.txid[32 * i] : zero, 32) == 0, "%s kind %d: the ID area at %zu\n", what, kind, i);
      if (ok) EXPECT(std::memcmp(&r.ids[32 * i], zero, 32) != 0, "%s kind %d: a zero ID at %zu\n", what, kind, i);
    }
  }
  // the device was asked for IDs with a host buffer exactly when something on the host reads them, and a device that hashes
  // left the host no ID to hash
  if (kind == 0) EXPECT(r.out[2] == 0 && r.out[3] == b.n, "%s kind 0: %llu asks, %llu hashed on the host\n", what, (unsigned long long)r.out[2], (unsigned long long)r.out[3]);
  if (kind >= 1) EXPECT(r.out[3] == 0 && r.out[4] > 0, "%s kind %d: %llu transactions hashed on the host\n", what, kind, (unsigned long long)r.out[3]);
  if (kind == 1) EXPECT(r.out[2] > 0, "%s kind 1: never asked for IDs\n", what);
  if (kind == 2) EXPECT((r.out[2] > 0) == flag, "%s kind 2 flag %d: asked for IDs %llu times\n", what, (int)flag, (unsigned long long)r.out[2]);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? (size_t)atoll(argv[1]) : 24;
  if (n < 24) { fprintf(stderr, "at least 24 transactions\n"); return 2; }
  Block b;
  if (!make_block(n, b)) { fprintf(stderr, "the builder failed\n"); return 1; }
  const Result want = run(b, 0, false, 0, 0, -1, 0, 1);
  if (want.rc != 0) { fprintf(stderr, "the plain call failed: %d\n", want.rc); return 1; }
  size_t accepted = 0;
  for (uint8_t s : want.status) accepted += s == 0;
  if (accepted + 4 != n || want.status[3] != 1 || want.status[5] != 2 || want.status[9] != 1 || want.status[12] != 1) { fprintf(stderr, "the block is not what it was built to be\n"); return 1; }
  size_t calls = 0;
  for (int kind = 0; kind < 3; ++kind)
    for (int flag = 0; flag < 2; ++flag) {
      const size_t shapes[6][2] = {{0, 0}, {0, 16}, {0, 1}, {16, 0}, {16, 16}, {8, 1}};     // (split, chunk)
      for (const auto& sh : shapes) {
        if (!check(b, want, run(b, kind, flag != 0, sh[0], sh[1], -1, 0, (uint32_t)(7 + calls)), kind, flag != 0, sh[0] ? "merged" : "lone")) return 1;
        ++calls;
      }
      // with the flag, a fault at every operation of every stage the stand-in has, lone and merged, in chunks of 16
      for (int stage = 0; flag && stage <= kind; ++stage)
        for (size_t split : {(size_t)0, (size_t)16})
          for (int k = 0;; ++k) {
            const Result r = run(b, kind, true, split, 16, k, stage, (uint32_t)(100 + k));
            if (!check(b, want, r, kind, true, "faulted")) return 1;
            ++calls;
            if (r.rc == 0) break;                        // (the k-th operation does not exist: the call ran clean)
            if (k > 400) { fprintf(stderr, "a call that never runs clean\n"); return 1; }
          }
    }
  printf("ok: %zu calls over %zu transactions\n", calls, n);
  return 0;
}
