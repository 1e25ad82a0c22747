// Do the host fold of a call's transaction root (csrc/tx_root.hpp) and the layout's clears with ZKGPU_TXFORMAT_RETURN_ROOT
// (csrc/tx_out.hpp) stay inside arrays of EXACTLY the size they are given?  A program of its own for a sanitizer build:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer
//       tools/tx_root_check.cpp -o tx_root_check
//   ./tx_root_check
// n = 0, 1 and 65 IDs on the heap (new[]: the sanitizer guards both ends), every span 1 .. 7, one and three host threads; the
// root is held against a top-down recursive tree written here over merlin.hpp's Transcript -- the RFC 6962 split, not the
// bottom-up fold.  Then begin, nothing-in-the-subset, fail-closed and a round's hand-out over status areas of exactly
// bytes(batch), for batches 0, 1 and 65 and the layouts with a root.  Exit status 0 and "ok" on success.
#include "../zkvm_amd/csrc/tx_out.hpp"
#include "../zkvm_amd/csrc/tx_root.hpp"

#include <cstdio>
#include <memory>

using namespace zk;
using namespace zk::zkvm;

namespace {

void reference(const uint8_t* ids, size_t lo, size_t hi, uint8_t out[32]) {
  Transcript t(TX_ROOT_LABEL);
  const size_t n = hi - lo;
  if (n == 0) { t.challenge_bytes(label_text(L_merkle_empty), out, 32); return; }
  if (n == 1) { t.append_message(label_text(L_txid), ids + 32 * lo, 32); t.challenge_bytes(label_text(L_merkle_leaf), out, 32); return; }
  size_t k = 1;
  while ((k << 1) < n) k <<= 1;
  uint8_t l[32], r[32];
  reference(ids, lo, lo + k, l);
  reference(ids, lo + k, hi, r);
  t.append_message(label_text(L_L), l, 32);
  t.append_message(label_text(L_R), r, 32);
  t.challenge_bytes(label_text(L_merkle_node), out, 32);
}

#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "  (%s)\n", #cond); return false; } } while (0)

bool folds() {
  for (size_t n : {(size_t)0, (size_t)1, (size_t)65}) {
    std::unique_ptr<uint8_t[]> ids(new uint8_t[32 * n]), want(new uint8_t[32]), got(new uint8_t[32]);
    uint32_t x = 2463534242u + (uint32_t)n;
    for (size_t i = 0; i < 32 * n; ++i) { x ^= x << 13; x ^= x >> 17; x ^= x << 5; ids[i] = (uint8_t)x; }
    reference(ids.get(), 0, n, want.get());
    for (uint32_t span = 1; span <= TX_ROOT_SPAN; ++span)
      for (int threads : {1, 3}) {
        memset(got.get(), 0xA5, 32);
        tx_root_fold_host(ids.get(), n, span, threads, got.get());
        EXPECT(memcmp(got.get(), want.get(), 32) == 0, "n %zu span %u threads %d: the fold is not the recursive tree\n", n, span, threads);
      }
  }
  return true;
}

bool clears() {
  for (size_t K : {(size_t)0, (size_t)1, (size_t)255})
    for (size_t batch : {(size_t)0, (size_t)1, (size_t)65}) {
      TxOutLayout lay; lay.ids = true; lay.log_k = K; lay.root = true;
      TxOutLayout old = lay; old.root = false;
      const size_t bytes = lay.bytes(batch), nb = (batch + 7) / 8;
      EXPECT(bytes == old.bytes(batch) + 32, "K %zu batch %zu: %zu bytes\n", K, batch, bytes);
      std::unique_ptr<uint8_t[]> area(new uint8_t[bytes]), bm(new uint8_t[nb]);
      EXPECT(lay.root_of(area.get(), batch) == area.get() + old.bytes(batch), "K %zu batch %zu: the root is not behind everything else\n", K, batch);
      memset(area.get(), 0xA5, bytes); memset(bm.get(), 0xFF, nb);
      lay.begin(bm.get(), area.get(), batch);
      for (size_t i = 0; i < bytes; ++i) EXPECT(area[i] == (i < batch ? TXOUT_REJECTED : 0), "begin: byte %zu of %zu\n", i, bytes);
      memset(area.get() + batch, 0xA5, bytes - batch);
      lay.nothing_in_subset(area.get(), batch);
      for (size_t i = 0; i < bytes; ++i) EXPECT(area[i] == (i < batch ? TXOUT_OUTSIDE_SUBSET : 0), "nothing in the subset: byte %zu of %zu\n", i, bytes);
      memset(area.get(), 0, batch); memset(area.get() + batch, 0xA5, bytes - batch); memset(bm.get(), 0xFF, nb);
      lay.fail_closed(bm.get(), area.get(), batch);
      for (size_t i = 0; i < bytes; ++i) EXPECT(area[i] == (i < batch ? TXOUT_REJECTED : 0), "fail-closed: byte %zu of %zu\n", i, bytes);
      for (size_t i = 0; i < nb; ++i) EXPECT(bm[i] == 0, "fail-closed: a bit\n");
      if (batch == 0) continue;
      // a round of this one call: whole -> its root arrives; one transaction short, or a failed round -> zeros
      std::unique_ptr<uint8_t[]> rbits(new uint8_t[nb + 1]), rstatus(new uint8_t[batch]), root(new uint8_t[32]);
      memset(root.get(), 0x77, 32);
      for (int kind = 0; kind < 3; ++kind) {
        memset(rbits.get(), 0xFF, nb + 1); memset(rstatus.get(), 0, batch);
        if (kind == 1) { rstatus[batch - 1] = 17; rbits[(batch - 1) / 8] &= (uint8_t)~(1u << ((batch - 1) % 8)); }
        memset(area.get(), 0xA5, bytes);
        const TxHandOut to{batch, lay, bm.get(), area.get(), root.get()};
        tx_round_hand_out(rbits.get(), rstatus.get(), kind != 2, &to, 1);
        const uint8_t* r = lay.root_of(area.get(), batch);
        for (size_t i = 0; i < 32; ++i) EXPECT(r[i] == (kind == 0 ? 0x77 : 0), "hand-out kind %d: root byte %zu\n", kind, i);
      }
    }
  return true;
}

}  // namespace

int main() {
  if (!folds() || !clears()) return 1;
  printf("ok\n");
  return 0;
}
