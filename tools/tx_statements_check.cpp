// The statements format (csrc/tx_statements.hpp, csrc/tx_musig_rows.hpp) on its own, for a sanitizer build:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -Izkvm_amd/csrc \
//       tools/tx_statements_check.cpp -o tx_statements_check && ./tx_statements_check [records] [seed]
// and once more with -fsanitize=thread.  Payments of 1 .. 16 keys (built and signed by zkvm_tx_build.hpp around arbitrary
// statement bytes) are run through the VM, and what it leaves is framed as records.  Then:
//   the parser over every record and over EVERY truncation of some, in exact-size heap copies (a read outside one is the
//     sanitizer's to report), must give back the VM's statement or refuse;
//   musig_row, with skip 0 and skip 1, must write the coefficients the VM's plan hashed;
//   tx_sig_row over the records' IDs must write what tx_finish_signature writes;
//   the stand-in scheduler of hostlib.cpp (the whole library source is compiled into this program: nothing is loaded), over
//     the first ten records, must accept every record in both modes, with the same bytes, and fail closed when the stand-in reports an error.
// Exit status 0 and "ok" on success.
#include "hostlib.cpp"

#include <array>
#include <cstdio>
#include <cstdlib>

static int fail(const char* what) { fprintf(stderr, "%s\n", what); return 1; }

static std::vector<uint8_t> record_of(const TxStatement& t) {
  const size_t k = t.sig_points.size() / 32 - 2;
  std::vector<uint8_t> r;
  auto put = [&](const void* p, size_t n) { r.insert(r.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
  auto put32 = [&](uint32_t x) { uint8_t b[4] = {(uint8_t)x, (uint8_t)(x >> 8), (uint8_t)(x >> 16), (uint8_t)(x >> 24)}; put(b, 4); };
  put(t.txid, 32);
  put(&t.sig_points[32], 32);
  put(&t.sig_scalars[0], 32);
  put32((uint32_t)k);
  put(&t.sig_points[64], 32 * k);
  put32(t.n_in); put32(t.n_out);
  put(t.commitments.data(), t.commitments.size());
  put32((uint32_t)t.proof_len);
  put(t.proof, t.proof_len);
  return r;
}

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? (size_t)atoll(argv[1]) : 40;
  std::mt19937_64 rng(argc > 2 ? (uint64_t)atoll(argv[2]) : 1);
  (void)base_table();
  std::vector<std::vector<uint8_t>> txs, recs;
  std::vector<TxStatement> vm(n);
  for (size_t i = 0; i < n; ++i) {
    const size_t n_in = 1 + i % 16, n_out = 1 + (i / 3) % 3;
    std::vector<uint8_t> com(64 * (n_in + n_out)), proof(1 + rng() % 200);
    uint8_t seed[32];
    for (auto& x : com) x = (uint8_t)rng();
    for (auto& x : proof) x = (uint8_t)rng();
    for (auto& x : seed) x = (uint8_t)rng();
    txs.push_back(tx_wrap_payment(n_in, n_out, com.data(), proof.data(), proof.size(), seed, 0, 1000));
    if (txs.back().empty()) return fail("builder failed");
    vm[i] = tx_prepare(txs.back().data(), txs.back().size());      // (the statement's proof points into txs[i], which stays)
    if (vm[i].status != TX_OK) return fail("the VM rejects a built payment");
    recs.push_back(record_of(vm[i]));
  }
  // ---- the parser: whole records, then every truncation and one byte too many, in exact-size copies
  for (size_t i = 0; i < n; ++i) {
    for (size_t len = i < 3 ? 0 : recs[i].size(); len <= recs[i].size() + 1; ++len) {
      std::vector<uint8_t> exact(recs[i].begin(), recs[i].begin() + std::min(len, recs[i].size()));
      if (len > recs[i].size()) exact.push_back(0);
      exact.shrink_to_fit();
      TxStatement st;
      tx_statements_many(std::array<const uint8_t*, 1>{exact.data()}.data(), std::array<size_t, 1>{exact.size()}.data(), &st, 1, true);
      if (len != recs[i].size()) { if (st.status != TX_INVALID) return fail("a truncated or overlong record was not refused"); continue; }
      const TxStatement& w = vm[i];
      if (st.status != TX_OK || memcmp(st.txid, w.txid, 32) || st.n_in != w.n_in || st.n_out != w.n_out || st.proof_len != w.proof_len ||
          memcmp(st.proof, w.proof, w.proof_len) || st.commitments.size() != w.commitments.size() ||
          memcmp(st.commitments.data(), w.commitments.data(), w.commitments.size()) || st.sig_scalars.size() != w.sig_scalars.size() ||
          memcmp(st.sig_scalars.data(), w.sig_scalars.data(), w.sig_scalars.size()) || memcmp(&st.sig_points[32], &w.sig_points[32], w.sig_points.size() - 32))
        return fail("the parser and the VM leave different statements");
    }
  }
  // ---- musig_row: the rows of all records as one stage, with skip 0 (key rows) and skip 1 (signature rows)
  for (uint32_t skip = 0; skip < 2; ++skip) {
    std::vector<uint64_t> off{0};
    std::vector<uint8_t> sc, pt, want;
    for (size_t i = 0; i < n; ++i) {
      const size_t from = skip ? 32 : 64;
      pt.insert(pt.end(), &vm[i].sig_points[from], &vm[i].sig_points[0] + vm[i].sig_points.size());
      want.insert(want.end(), &vm[i].sig_scalars[from], &vm[i].sig_scalars[0] + vm[i].sig_scalars.size());
      off.push_back(pt.size() / 32);
    }
    sc = want;
    for (size_t i = 0; i < n; ++i) for (uint64_t t = off[i] + skip; t < off[i + 1]; ++t) memset(&sc[32 * t], 0xee, 32);
    pt.shrink_to_fit(); sc.shrink_to_fit(); off.shrink_to_fit();
    if (zkhost_musig_rows(sc.data(), pt.data(), off.data(), n, skip, nullptr) != 0) return fail("musig rows refused");
    if (sc != want) return fail("musig_row and the VM's plan give different coefficients");
  }
  // ---- tx_sig_row over the records' IDs against tx_finish_signature
  {
    SigScript script;
    if (!sig_script(script)) return fail("no signature script");
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> sc, pt, ids(8 * n), agg(8 * n), pos(n);
    std::vector<TxStatement> fin(vm);
    uint8_t B[32];
    ge Bp; Bp.X = fe_BASE_X(); Bp.Y = fe_BASE_Y(); Bp.Z = fe_one(); Bp.T = fe_BASE_T();
    encode_point(B, Bp);
    for (size_t i = 0; i < n; ++i) {
      uint8_t key[32];
      for (auto& x : key) x = (uint8_t)rng();
      const size_t words = vm[i].sig_points.size() / 4 - 8;
      const size_t at = sc.size();
      sc.resize(at + words); pt.resize(at + words);
      memcpy(&sc[at], &vm[i].sig_scalars[32], 4 * words);
      memcpy(&pt[at], &vm[i].sig_points[32], 4 * words);
      memcpy(&ids[8 * i], vm[i].txid, 32);
      memcpy(&agg[8 * i], key, 32);
      pos[i] = (uint32_t)i;
      off.push_back(sc.size() / 8);
      tx_finish_signature(fin[i], B, key);
    }
    SigRowsView v{&script, ids.data(), pos.data(), agg.data(), off.data(), pt.data(), sc.data(), (uint32_t)n};
    sig_rows_run_host(v);
    for (size_t i = 0; i < n; ++i)
      if (memcmp(&sc[8 * (off[i] + 1)], &fin[i].sig_scalars[64], fin[i].sig_scalars.size() - 64)) return fail("tx_sig_row and tx_finish_signature differ");
  }
  // ---- the scheduler on the stand-in: both modes, several chunk sizes, then an error at every operation of one call
  {
    const size_t m = std::min<size_t>(n, 10);               // (the stand-in's group arithmetic is slow under a sanitizer: ten records, 55 keys)
    if (m < 10) return fail("the scheduler part wants ten records");
    std::vector<uint8_t> blob, ok(m, 1);
    std::vector<uint64_t> off{0};
    for (size_t i = 0; i < m; ++i) { blob.insert(blob.end(), recs[i].begin(), recs[i].end()); off.push_back(blob.size()); }
    blob[off[5] + 40] ^= 1;                                 // a byte of R: the signature of record 5 fails
    ok[9] = 0;
    std::vector<uint8_t> first_bm, first_st;
    for (int on_device = 0; on_device < 2; ++on_device)
      for (size_t chunk : {(size_t)0, (size_t)8}) {
        std::vector<uint8_t> bm((m + 7) / 8 + 1, 0xff), st(m, 0xff);
        uint64_t out[5];
        const int rc = zkhost_txcall_statements_selftest(on_device, 1, m, blob.data(), off.data(), ok.data(), 3, chunk, (uint32_t)(7 + chunk), -1, chunk == 8 ? 1 : 2,
                                                         bm.data(), st.data(), out);
        bm.resize((m + 7) / 8);
        if (rc != 0 || out[1] != 0 || out[2] != 0 || out[3] != 0 || out[4] != (on_device ? m : 0)) return fail("a statements call on the stand-in failed");
        for (size_t i = 0; i < m; ++i) {
          const uint8_t want = i == 5 ? 21 : i == 9 ? 19 : 0;
          if (st[i] != want || (((bm[i / 8] >> (i % 8)) & 1) != (want == 0))) return fail("a verdict of the stand-in call is wrong");
        }
        if (first_bm.empty()) { first_bm = bm; first_st = st; }
        if (bm != first_bm || st != first_st) return fail("the two modes give different bytes");
      }
    for (int on_device = 0; on_device < 2; ++on_device)
      for (int k = 0;; ++k) {
        std::vector<uint8_t> bm((m + 7) / 8 + 1, 0xff), st(m, 0xff);
        uint64_t out[5];
        const int rc = zkhost_txcall_statements_selftest(on_device, 1, m, blob.data(), off.data(), ok.data(), 2, 8, (uint32_t)(100 + k), k, 2, bm.data(), st.data(), out);
        if (rc == 0) break;
        if (k > 200) return fail("the injected error never stops");
        for (size_t i = 0; i < m; ++i) if (st[i] != 1 || ((bm[i / 8] >> (i % 8)) & 1)) return fail("a failed call is not closed");
        if (out[1] != 0) return fail("a failed call leaked a staged chunk");
      }
  }
  printf("ok: %zu records\n", n);
  return 0;
}
