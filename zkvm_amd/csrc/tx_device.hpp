// tx_device.hpp -- the device side of a transaction call (tx_call.hpp: TxDevice) on a verifier: GpuTxDevice, and the stage
// helpers only it uses.  Included by session.hpp (it uses the verifier and the pipeline internals of zkgpu.hip); the scheduling
// of the call -- which stage is queued when -- is tx_call.hpp's and knows nothing of this file.
#pragma once

namespace {

// rows of dynamic terms that lie in the context's input buffers, into a Job
void resident_rows(zkgpu_ctx* c, Job& job, size_t batch, uint64_t n_dyn, uint64_t max_dyn_row) {
  job.d_dyn_scalars = (const uint32_t*)c->in_scalars.p;
  job.d_dyn_points = (const uint32_t*)c->in_points.p;
  job.d_dyn_offsets = (const uint64_t*)c->in_offsets.p;
  job.n_dyn = n_dyn;
  job.n_msm = (uint32_t)batch;
  job.max_dyn_row = max_dyn_row;
}
// what queueing a stage ends in: after an error nothing of it counts as in flight, otherwise the context is busy until its collect
int stage_queued(zkgpu_ctx* c, int rc, size_t batch) {
  if (rc != ZKGPU_OK) { c->split = zkgpu_ctx::SplitOp{}; return rc; }
  c->pending = true; c->pending_batch = batch;
  return ZKGPU_OK;
}

// host arrays -> the context's input buffers -> kernels and result copy queued (batch_device_enqueue, value mode);
// split_collect finishes.  The arrays must stay alive until then; the context is marked busy meanwhile.
int msm_values_enqueue(zkgpu_ctx* c, const uint8_t* scalars, const uint8_t* points, const uint64_t* offsets, size_t batch) {
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  TRY(refuse_if_pending(c));
  DeviceGuard g(c->device);
  const uint64_t n = offsets[batch];
  TRY(upload(c, c->in_scalars, scalars, n * 32));
  TRY(upload(c, c->in_points, points, n * 32));
  TRY(upload(c, c->in_offsets, offsets, (batch + 1) * 8));
  Job job;
  resident_rows(c, job, batch, n, longest_row(offsets, batch));
  return stage_queued(c, batch_device_enqueue(c, job, true), batch);
}

int split_collect(zkgpu_ctx* c, uint8_t* bitmap, uint8_t* values) {
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  DeviceGuard g(c->device);
  c->pending = false;
  return batch_collect(c, bitmap, values);
}

// Reason bytes of a key or signature stage (tx_reason_kernels.hpp: k_tx_reason_stage), in two halves like the stage itself.
// They lie behind everything else the stage copies to the context's pinned result buffer -- bitmap | 64 status bytes | the
// values of a key stage -- so the buffer is brought to size BEFORE the stage is queued (it never shrinks, and the context is
// idle then); the kernel and its copy are queued behind the stage's own on the same stream, and the one wait of
// batch_collect covers them.
size_t stage_reasons_offset(size_t batch, bool values) { return (batch + 7) / 8 + 64 + (values ? 32 * batch : 0); }
int stage_reasons_reserve(zkgpu_ctx* c, size_t batch, bool values) {
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  TRY(refuse_if_pending(c));
  DeviceGuard g(c->device);
  return ensure_pinned(c, stage_reasons_offset(batch, values) + batch);
}
int stage_reasons_enqueue(zkgpu_ctx* c, uint8_t code_when_clear) {
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const size_t B = c->split.batch;
  if (c->split.kind == 0 || B == 0) return ZKGPU_OK;
  auto queue = [&]() -> int {
    TRY(ensure(c, c->tx_reason, B));
    {
      Launch l(c, "k_tx_reason_stage", c->split.stream);
      hipLaunchKernelGGL(k_tx_reason_stage, dim3(blocks_for(B, 256)), dim3(256), 0, c->split.stream, (const uint8_t*)c->bitmap.p, (uint32_t)B,
                         (uint32_t)code_when_clear, (uint8_t*)c->tx_reason.p);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync((char*)c->pinned + stage_reasons_offset(B, c->split.values), c->tx_reason.p, B, hipMemcpyDeviceToHost, c->split.stream));
    return ZKGPU_OK;
  };
  const int rc = queue();
  if (rc != ZKGPU_OK) { c->split = zkgpu_ctx::SplitOp{}; c->pending = false; }     // (the failed call has drained the device: the stage is not in flight any more)
  return rc;
}
// split_collect, and the stage's reason bytes with it (why may be NULL)
int split_collect_why(zkgpu_ctx* c, uint8_t* bitmap, uint8_t* values, uint8_t* why) {
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  const size_t B = c->split.batch;
  const bool vals = c->split.values;
  const int rc = split_collect(c, bitmap, values);
  if (!why) return rc;
  if (rc != ZKGPU_OK) { memset(why, ZKGPU_TXSTATUS_REJECTED, B); return rc; }
  if (B) memcpy(why, (const char*)c->pinned + stage_reasons_offset(B, vals), B);
  return rc;
}

// has everything queued by the last *_enqueue on this context run?  (never blocks)
bool split_done(zkgpu_ctx* c) {
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (c->split.kind == 0 || c->split.batch == 0) return true;
  DeviceGuard g(c->device);
  return hipStreamQuery(c->split.stream) != hipErrorNotReady;
}

// rows that already lie in the context's input buffers (c->mu held, the device set): kernels and result copy queued
int verify_ps_enqueue_resident(zkgpu_ctx* c, const zkgpu_pointset* ps, size_t batch, uint64_t nd, uint64_t ns, uint64_t max_dyn_row) {
  Job job;
  resident_rows(c, job, batch, nd, max_dyn_row);
  job.d_st_scalars = (const uint32_t*)c->in_st_scalars.p;
  job.d_st_index = (const uint32_t*)c->in_st_index.p;
  job.d_st_offsets = (const uint64_t*)c->in_st_offsets.p;
  job.n_static = ns;
  job.d_static_rows = ps->rows;
  return stage_queued(c, (ps->table && ns) ? batch_device_tables_enqueue(c, job, ps) : batch_device_enqueue(c, job, false), batch);
}

// rows of dynamic terms + terms on the resident set's tables (the signature equations) into the context's input buffers
// (c->mu held, the device set)
int verify_ps_upload(zkgpu_ctx* c, size_t batch, const uint8_t* dyn_scalars, const uint8_t* dyn_points, const uint64_t* dyn_offsets,
                     const uint8_t* static_scalars, const uint32_t* static_index, const uint64_t* static_offsets) {
  const uint64_t nd = dyn_offsets[batch], ns = static_offsets[batch];
  TRY(upload(c, c->in_scalars, dyn_scalars, nd * 32));
  TRY(upload(c, c->in_points, dyn_points, nd * 32));
  TRY(upload(c, c->in_offsets, dyn_offsets, (batch + 1) * 8));
  TRY(upload(c, c->in_st_scalars, static_scalars, ns * 32));
  TRY(upload(c, c->in_st_index, static_index, ns * 4));
  return upload(c, c->in_st_offsets, static_offsets, (batch + 1) * 8);
}

// the two together: host arrays -> kernels and result copy queued
int verify_ps_enqueue(zkgpu_ctx* c, const zkgpu_pointset* ps, size_t batch, const uint8_t* dyn_scalars, const uint8_t* dyn_points,
                      const uint64_t* dyn_offsets, const uint8_t* static_scalars, const uint32_t* static_index, const uint64_t* static_offsets) {
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  TRY(refuse_if_pending(c));
  DeviceGuard g(c->device);
  TRY(verify_ps_upload(c, batch, dyn_scalars, dyn_points, dyn_offsets, static_scalars, static_index, static_offsets));
  return verify_ps_enqueue_resident(c, ps, batch, dyn_offsets[batch], static_offsets[batch], longest_row(dyn_offsets, batch));
}

// a constant the verifier keeps on the device, in one or two parts, uploaded once: after a failure it is freed and reported,
// and `kept` stays empty for the next call to try again
int const_upload(zkgpu_ctx* c, Buffer& kept, const void* a, size_t na, const void* b = nullptr, size_t nb = 0) {
  Buffer made;
  TRY(ensure(c, made, na + nb));
  hipError_t e = hipMemcpy(made.p, a, na, hipMemcpyHostToDevice);
  if (e == hipSuccess && nb) e = hipMemcpy((char*)made.p + na, b, nb, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(made.p); HIP_TRY(c, e); }
  kept = made;
  return ZKGPU_OK;
}

// The device side of a transaction call (tx_call.hpp: TxDevice) on a verifier: key stages on aux_keys[slot], signature
// stages on aux_sigs[slot] (contexts of their own, each a pair of streams beside the lanes'), cloak proofs as blocks of
// mixed shapes on the lanes, staged through the verifier's ring of pinned / device areas.  v->mu is held by the call.
static_assert(zk::zkvm::TxCall::OK == ZKGPU_OK && zk::zkvm::TxCall::ENOMEM_ == ZKGPU_ENOMEM && zk::zkvm::TxCall::EINVAL_ == ZKGPU_EINVAL, "tx_call.hpp restates three status codes");
static_assert(zk::zkvm::TXLOG_INPUT == ZKGPU_TXLOG_INPUT && zk::zkvm::TXLOG_OUTPUT == ZKGPU_TXLOG_OUTPUT, "tx_log.hpp restates the two entry kinds");
uint32_t tx_root_span_from_env() { const char* e = getenv("ZKGPU_TX_ROOT_SPAN"); return zk::zkvm::tx_root_span(e ? atoll(e) : 0); }
const uint32_t g_tx_root_span = tx_root_span_from_env();   // (once, at load: no call reads the environment)
class GpuTxDevice : public zk::zkvm::TxDevice {
 public:
  // slot_base / arena_base: which of the verifier's stage contexts and staging areas this call uses (a call alone: slots 0
  // and 1, areas 0 .. RING - 1; two rounds in flight: one slot and one set of areas each)
  // format (tx_out.hpp: TxFormat, the verifier's format word decoded; of it the base format 0 never gets here) is kept as it
  // is, and its predicates are asked where they matter:
  //   reasons(): a format-2 call -- every stage also brings back one reason byte per row (tx_reason_kernels.hpp)
  //   hashes(): ZKGPU_TXFORMAT_HASH_ON_DEVICE -- the transaction IDs of every chunk come from k_tx_hash
  //   chains(): ZKGPU_TXFORMAT_SIGN_ON_DEVICE beside it -- the signature's challenge comes from k_tx_sig_rows
  //   ids(): ZKGPU_TXFORMAT_RETURN_IDS -- the caller is handed the IDs of what it accepted; all it changes HERE is that a chained
  //     stage copies its IDs down as an unchained one does (one copy on the hashing stream, no launch)
  //   log_k(): ZKGPU_TXFORMAT_RETURN_LOG beside it -- K, the log entries kept per transaction (0: no).  Here: behind k_tx_hash, on
  //     its stream, k_tx_log_gather and one more copy down (hash_queue); a call without it queues exactly what it queued before
  //   precompute(): ZKGPU_TXFORMAT_PRECOMPUTE_ONLY -- the call asks for the hashing stage alone (tx_call.hpp), and that stage
  //     walks the tape by dependency level (tx_hash_levels.hpp: k_tx_hash_levels) because that kernel, timed alone on the tapes of
  //     1024 and of 8192 payments, was faster in every process than k_tx_hash in any (median 250 / 255 us against a minimum of
  //     359 / 360 us: DESIGN.md sec 4.5, profiles/r14a_tx_precompute.txt); ZKGPU_TX_HASH_LEVELS=0 / 1 picks the kernel for the
  //     tests and for measuring (levels_).  A verifying call's stage never does: its launches are as they were
  //   statements(): ZKGPU_TXFORMAT_STATEMENTS_V1 -- the call's pieces are records (tx_statements.hpp); nothing is hashed for an ID
  //   root(): ZKGPU_TXFORMAT_RETURN_ROOT beside ids() -- asked only beside hashes() (tx_call.hpp folds the host VM's IDs itself).  Behind
  //     every tape, on its stream, one more copy up (the transactions' places in the call) and k_tx_root_leaves; behind the call's
  //     LAST tape k_tx_root_fold once per pass and asking piece, and 32 bytes per piece down (tx_root_kernels.hpp).  The folds wait
  //     ON THE DEVICE for the leaves the other slot's stream wrote (an event per slot); the host waits where it waited for the tape.
  //     ZKGPU_TX_ROOT_SPAN=1 .. 7 sets the levels per pass for the tests (root_span_).  A call without the flag queues what it queued before
  //   forms_musig(): ZKGPU_TXFORMAT_SIGN_ON_DEVICE beside it -- the MuSig coefficients come from k_musig_rows (tx_musig_rows.hpp) in
  //     both stages' rows, the challenge from k_tx_sig_rows over the IDs the host uploads; no host fallback: an error of a launch is the call's
  static constexpr bool TX_HASH_LEVELS_SERVE = true;
  explicit GpuTxDevice(zkgpu_verifier* v, int slot_base = 0, size_t arena_base = 0, const zk::zkvm::TxFormat& format = zk::zkvm::TxFormat())
      : v_(v), sb_(slot_base), ab_(arena_base), format_(format), levels_(format.precompute() && levels_asked()) {}
  const zk::zkvm::TxFormat& format() const override { return format_; }
  // points and offsets up, the coefficients written where the rows lie (skip 0), then the stage as msm_values_enqueue queues it
  int keys_enqueue_formed(int slot, const uint8_t* points, const uint64_t* offsets, size_t rows) override {
    zkgpu_ctx* c = keys(slot);
    if (!format_.forms_musig()) { err_ = "a key stage without scalars on a device that does not form them"; return ZKGPU_EINVAL; }
    TRY(reasons_room(c, rows, true));
    return reasons_behind(c, seen(formed_keys_queue(c, points, offsets, rows), c, "key coefficient stage: "), ZKGPU_TXSTATUS_KEY);
  }
  const uint8_t* hash_log(int slot) override { return format_.hashes() && format_.log_k() ? (const uint8_t*)hash(slot).h_log : nullptr; }
  zk::zkvm::TxHashTape* hash_tape(int slot) override { return &hash(slot).tape; }
  // one copy up, one launch, one copy of the IDs down, on the stage's own high-priority stream
  int hash_enqueue(int slot, const zk::zkvm::TxHashTape& tape) override {
    return seen(hash_queue(slot, tape), keys(slot), "transaction-ID hashing stage: ");
  }
  bool hash_done(int slot) override {
    zkgpu_verifier::TxHashStage& hs = hash(slot);
    if (!hs.stream || hs.n_tx == 0) return true;
    DeviceGuard g(v_->root->device);
    return hipStreamQuery(hs.stream) != hipErrorNotReady;
  }
  int hash_collect(int slot, uint8_t* txids) override {
    return seen(hash_wait(slot, txids), keys(slot), "transaction-ID hashing stage: ");
  }
  const uint8_t* basepoint() override { return v_->basepoint; }
  int keys_enqueue(int slot, const uint8_t* scalars, const uint8_t* points, const uint64_t* offsets, size_t rows) override {
    zkgpu_ctx* c = keys(slot);
    TRY(reasons_room(c, rows, true));
    return reasons_behind(c, seen(msm_values_enqueue(c, scalars, points, offsets, rows), c), ZKGPU_TXSTATUS_KEY);
  }
  bool keys_done(int slot) override { return split_done(keys(slot)); }
  int keys_collect(int slot, uint8_t* ok_bits, uint8_t* values, uint8_t* why) override {
    return seen(split_collect_why(keys(slot), ok_bits, values, format_.reasons() ? why : nullptr), keys(slot));
  }
  // (staging thread: touches the plans -- plans_mu -- the given arena and nothing else of the verifier)
  int proofs_stage(size_t ring_slot, size_t n, const zk::zkvm::TxProofSource* src, int host_threads, void** handle, std::string* err) override {
    zkgpu_txblock* blk = nullptr;
    const int rc = txblock_stage_host(v_, n, src, nullptr, host_threads, &blk, &v_->tx_arenas[ab_ + ring_slot], err);
    if (rc != ZKGPU_OK) return rc;
    Staged* st = new Staged();
    st->blk = blk;
    *handle = st;
    return ZKGPU_OK;
  }
  int proofs_start(size_t ring_slot, void* handle) override {
    Staged* st = (Staged*)handle;
    // one copy to HBM, and the chunk's batches queued on the lanes
    int rc = txblock_upload(v_, st->blk, &v_->tx_arenas[ab_ + ring_slot]);
    if (rc != ZKGPU_OK) { err_ = v_->last_error; return rc; }
    // a chunk of one shape goes to the device as few, large batches (measured: the last chunk in batches short enough for
    // the one-wavefront-per-transaction transcript, or cut in two, does not shorten the tail of the call)
    const size_t saved_chunk = v_->chunk;
    v_->chunk = std::max<size_t>(saved_chunk, 4096);
    st->run = block_start(v_, st->blk, true, format_.reasons());
    v_->chunk = saved_chunk;
    if (!st->run) { err_ = v_->last_error; return ZKGPU_ENOMEM; }
    if (st->run->rc != ZKGPU_OK) {
      // One device batch of the block could not be queued.  The call releases a chunk that was not started WITHOUT finishing
      // it, and the block goes with it -- but batches of the block's other shapes may already be on lanes, and their requests
      // refer to the block through the run: they are collected here, before the error leaves (found by injecting a fault at
      // every runtime call of a call of four shapes: the next call collected such a request and read the freed block).
      const int rc = st->run->rc;
      err_ = v_->last_error;
      std::vector<uint8_t> none((zkgpu_txblock_size(st->blk) + 7) / 8 + 1, 0);
      (void)block_finish(v_, st->run, none.data(), nullptr);
      st->run = nullptr;
      return rc;
    }
    return ZKGPU_OK;
  }
  bool proofs_done(void* handle) override {                // have the lanes finished every batch of this block?  (never blocks)
    Staged* st = (Staged*)handle;
    if (!st->run) return true;
    return block_done(v_, st->run);
  }
  int proofs_finish(void* handle, uint8_t* accept_bits, uint8_t* why) override {
    Staged* st = (Staged*)handle;
    int rc = ZKGPU_OK;
    if (st->run) { rc = block_finish(v_, st->run, accept_bits, format_.reasons() ? why : nullptr); if (rc != ZKGPU_OK) err_ = v_->last_error; }
    proofs_release(handle);
    return rc;
  }
  void proofs_release(void* handle) override {
    Staged* st = (Staged*)handle;
    if (st->blk) zkgpu_txblock_destroy(st->blk);
    delete st;
  }
  // chain: the rows up, the challenge kernel behind the slot's key stage and tape (events), the equations behind it -- all on
  // the signature context's stream, nothing waited for
  int sigs_enqueue(int slot, size_t rows, const uint8_t* dyn_scalars, const uint8_t* dyn_points, const uint64_t* dyn_offsets,
                   const uint8_t* base_scalars, const zk::zkvm::SigChain* chain) override {
    zkgpu_ctx* c = sigs(slot);
    // one term per row on the resident set's tables: index 0 = the basepoint B
    sidx_[slot].assign(rows, 0);
    soff_[slot].resize(rows + 1);
    for (size_t q = 0; q <= rows; ++q) soff_[slot][q] = q;
    TRY(reasons_room(c, rows, false));
    if (!chain)
      return reasons_behind(c, seen(verify_ps_enqueue(c, v_->ps, rows, dyn_scalars, dyn_points, dyn_offsets, base_scalars, sidx_[slot].data(), soff_[slot].data()), c),
                            ZKGPU_TXSTATUS_SIGNATURE);
    // (a profiled call: the stage's context takes the root's switch for this stage alone -- profile_to_root clears it when
    // the stage is collected, and here on every error, after which sigs_collect is not asked)
    bool profiled = false;
    { std::lock_guard<std::recursive_mutex> rl(v_->root->mu); profiled = v_->root->profiling; }
    int rc = seen(chain->txids ? host_ids_chain_queue(slot, *chain, rows, dyn_scalars, dyn_points, dyn_offsets, base_scalars, profiled)
                               : chain_queue(slot, *chain, rows, dyn_scalars, dyn_points, dyn_offsets, base_scalars, profiled), c, "signature challenge stage: ");
    if (rc == ZKGPU_OK) {
      std::lock_guard<std::recursive_mutex> lk(c->mu);
      DeviceGuard g(c->device);
      rc = seen(verify_ps_enqueue_resident(c, v_->ps, rows, dyn_offsets[rows], rows, longest_row(dyn_offsets, rows)), c);
    }
    if (rc == ZKGPU_OK) sig(slot).rows = rows;
    rc = reasons_behind(c, rc, ZKGPU_TXSTATUS_SIGNATURE);
    if (rc != ZKGPU_OK && profiled) profile_to_root(c);
    return rc;
  }
  bool sigs_done(int slot) override { return split_done(sigs(slot)); }
  int sigs_collect(int slot, uint8_t* bits, uint8_t* why) override {
    const int rc = seen(split_collect_why(sigs(slot), bits, nullptr, format_.reasons() ? why : nullptr), sigs(slot));
    if (format_.chains() || format_.forms_musig()) {
      zkgpu_ctx* c = sigs(slot);
      const size_t rows = sig(slot).rows;
      sig(slot).rows = 0;
      if (rc == ZKGPU_OK) { std::lock_guard<std::recursive_mutex> rl(v_->root->mu); v_->root->tx_signed_on_device += rows; if (format_.forms_musig()) v_->root->tx_musig_on_device += rows; }
      bool profiled = false;
      { std::lock_guard<std::recursive_mutex> lk(c->mu); profiled = c->profiling; }
      if (profiled) profile_to_root(c);                  // (only a call made with zkgpu_profile_enable on: nothing of it otherwise)
    }
    return rc;
  }
  std::string last_error() override { return err_; }
  int root_begin(size_t total) override { return seen(root_zero(total), keys(0), "transaction root stage: "); }
  void hash_place(int slot, size_t lo) override { hash(slot).place = lo; }
  int root_enqueue(int slot, const uint64_t* ranges, size_t n) override { return seen(root_queue(slot, ranges, n), keys(slot), "transaction root stage: "); }
  bool root_done(int slot) override {
    zkgpu_verifier::TxHashStage& hs = hash(slot);
    if (!hs.stream) return true;
    DeviceGuard g(v_->root->device);
    return hipStreamQuery(hs.stream) != hipErrorNotReady;
  }
  int root_collect(int slot, uint8_t* roots) override { return seen(root_wait(slot, roots), keys(slot), "transaction root stage: "); }

 private:
  struct Staged { zkgpu_txblock* blk = nullptr; zkgpu_verifier::BlockRun* run = nullptr; };
  zkgpu_verifier::TxHashStage& hash(int slot) const { return v_->tx_hash[(sb_ + slot) & 1]; }
  zkgpu_verifier::TxSigStage& sig(int slot) const { return v_->tx_sig[(sb_ + slot) & 1]; }
  // a profiled stage's launches go to the root's profile, where zkgpu_profile_get is asked for them (the stage's context is
  // not the caller's to ask), and the context's switch is off again: it is on for one stage of a profiled call and never else
  void profile_to_root(zkgpu_ctx* c) {
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    std::lock_guard<std::recursive_mutex> rl(v_->root->mu);
    for (const ProfEntry& e : c->prof) { ProfEntry& to = v_->root->prof[(size_t)prof_index(v_->root, e.name)]; to.launches += e.launches; to.ms += e.ms; }
    c->prof.clear();
    c->profiling = false;
  }
  // what a device with reasons adds around a key or signature stage of `rows` on c (stage_reasons_*): room for the reason bytes
  // before the stage is queued; behind it -- rc: what queueing it gave -- their kernel and copy
  int reasons_room(zkgpu_ctx* c, size_t rows, bool values) { return format_.reasons() ? seen(stage_reasons_reserve(c, rows, values), c) : ZKGPU_OK; }
  int reasons_behind(zkgpu_ctx* c, int rc, uint8_t code_when_clear) {
    return (rc == ZKGPU_OK && format_.reasons()) ? seen(stage_reasons_enqueue(c, code_when_clear), c) : rc;
  }
  // the rows of a chained stage up and the challenge kernel queued behind what `chain` names
  int chain_queue(int slot, const zk::zkvm::SigChain& chain, size_t rows, const uint8_t* dyn_scalars, const uint8_t* dyn_points,
                  const uint64_t* dyn_offsets, const uint8_t* base_scalars, bool profiled) {
    using namespace zk::zkvm;
    const uint32_t* tape_pos = chain.tape_pos;
    zkgpu_ctx* c = sigs(slot);
    zkgpu_ctx* kc = keys(chain.key_slot);
    zkgpu_verifier::TxHashStage& hs = hash(chain.hash_slot);
    zkgpu_verifier::TxSigStage& ss = sig(slot);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    TRY(refuse_if_pending(c));
    DeviceGuard g(c->device);
    // what the kernel indexes blindly: the key stage in flight in that slot has exactly these rows (its values: 32 bytes per
    // row), the tape in flight holds every transaction named, every row has R and at least one key
    hipStream_t key_stream = nullptr;
    {
      std::lock_guard<std::recursive_mutex> kl(kc->mu);
      if (!kc->pending || kc->split.kind != 1 || !kc->split.values || kc->split.batch != rows) { c->last_error = "no key stage of these rows in flight in the slot"; return ZKGPU_EINVAL; }
      key_stream = kc->split.stream;
    }
    if (rows == 0 || rows >= (1ull << 31) || hs.n_tx == 0 || !hs.stream) { c->last_error = "no tape in flight in the slot"; return ZKGPU_EINVAL; }
    for (size_t r = 0; r < rows; ++r)
      if (tape_pos[r] >= hs.n_tx || dyn_offsets[r + 1] < dyn_offsets[r] + 2) { c->last_error = "a signature row without its ID, its R or a key"; return ZKGPU_EINVAL; }
    if (!v_->tx_sig_const.p) {                           // once per verifier: what tx_finish_signature hashes, written down
      SigScript sc;
      if (!sig_script(sc)) { c->last_error = "the signature transcript does not fit the device's script"; return ZKGPU_EINVAL; }
      TRY(const_upload(c, v_->tx_sig_const, &sc, sizeof sc));
    }
    if (!ss.ev_keys) HIP_TRY(c, hipEventCreateWithFlags(&ss.ev_keys, hipEventDisableTiming));
    if (!ss.ev_ids) HIP_TRY(c, hipEventCreateWithFlags(&ss.ev_ids, hipEventDisableTiming));
    TRY(verify_ps_upload(c, rows, dyn_scalars, dyn_points, dyn_offsets, base_scalars, sidx_[slot].data(), soff_[slot].data()));
    TRY(upload(c, ss.d_pos, tape_pos, rows * 4));
    HIP_TRY(c, hipEventRecord(ss.ev_keys, key_stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, ss.ev_keys, 0));
    if (hs.ids_marked) {                                 // (beside ZKGPU_TXFORMAT_RETURN_LOG: recorded behind k_tx_hash, before the gather -- hash_queue)
      HIP_TRY(c, hipStreamWaitEvent(c->stream, hs.ev_ids, 0));
    } else {
      HIP_TRY(c, hipEventRecord(ss.ev_ids, hs.stream));
      HIP_TRY(c, hipStreamWaitEvent(c->stream, ss.ev_ids, 0));
    }
    c->profiling = profiled;
    SigRowsView view{(const SigScript*)v_->tx_sig_const.p, (const uint32_t*)hs.d_txid.p, (const uint32_t*)ss.d_pos.p, (const uint32_t*)kc->values.p,
                     (const uint64_t*)c->in_offsets.p, (const uint32_t*)c->in_points.p, (uint32_t*)c->in_scalars.p, (uint32_t)rows};
    {
      Launch l(c, "k_tx_sig_rows", c->stream);
      hipLaunchKernelGGL(zk::k_tx_sig_rows, dim3(blocks_for(rows, 64)), dim3(64), 0, c->stream, view);
    }
    HIP_TRY(c, hipGetLastError());
    return ZKGPU_OK;
  }
  // ---- a statements call whose device forms the MuSig coefficients (tx_musig_rows.hpp)
  // once per verifier: what the key aggregation hashes, written down by running the host's own recipe over a recorder
  int musig_const(zkgpu_ctx* c) {
    if (v_->tx_musig_const.p) return ZKGPU_OK;
    zk::zkvm::MusigScript sc;
    if (!zk::zkvm::musig_script(sc)) { c->last_error = "the key-aggregation transcripts do not fit the device's script"; return ZKGPU_EINVAL; }
    return const_upload(c, v_->tx_musig_const, &sc, sizeof sc);
  }
  // what k_musig_rows indexes blindly: the offsets rise, every row has its `skip` leading terms and at least one key
  static bool musig_rows_fit(const uint64_t* offsets, size_t rows, uint32_t skip) {
    if (rows == 0 || rows >= (1ull << 31)) return false;
    for (size_t r = 0; r < rows; ++r) if (offsets[r + 1] < offsets[r] + skip + 1) return false;
    return true;
  }
  // the coefficients of the rows that lie in c's input buffers (points, offsets; in_scalars has room for every term), on c's
  // stream (c->mu held, the device set)
  int musig_launch(zkgpu_ctx* c, size_t rows, uint32_t skip) {
    const zk::zkvm::MusigRowsView view{(const zk::zkvm::MusigScript*)v_->tx_musig_const.p, (const uint64_t*)c->in_offsets.p, (const uint32_t*)c->in_points.p,
                                       (uint32_t*)c->in_scalars.p, (uint32_t)rows, skip, nullptr};
    {
      Launch l(c, "k_musig_rows", c->stream);
      hipLaunchKernelGGL(zk::k_musig_rows, dim3(blocks_for(rows, 64)), dim3(64), 0, c->stream, view);
    }
    HIP_TRY(c, hipGetLastError());
    return ZKGPU_OK;
  }
  int formed_keys_queue(zkgpu_ctx* c, const uint8_t* points, const uint64_t* offsets, size_t rows) {
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    TRY(refuse_if_pending(c));
    DeviceGuard g(c->device);
    if (!musig_rows_fit(offsets, rows, 0) || offsets[0] != 0) { c->last_error = "a key row without a key"; return ZKGPU_EINVAL; }
    const uint64_t n = offsets[rows];
    TRY(musig_const(c));
    TRY(ensure(c, c->in_scalars, std::max<size_t>(n * 32, 16)));
    TRY(upload(c, c->in_points, points, n * 32));
    TRY(upload(c, c->in_offsets, offsets, (rows + 1) * 8));
    TRY(musig_launch(c, rows, 0));
    Job job;
    resident_rows(c, job, rows, n, longest_row(offsets, rows));
    return stage_queued(c, batch_device_enqueue(c, job, true), rows);
  }
  // the rows of a signature stage up with their IDs; k_musig_rows (skip 1: term 0 is R) at once, k_tx_sig_rows behind the
  // slot's key stage (the event chain_queue uses); nothing is waited for, and there is no hashing stage to order behind
  int host_ids_chain_queue(int slot, const zk::zkvm::SigChain& chain, size_t rows, const uint8_t* dyn_scalars, const uint8_t* dyn_points,
                           const uint64_t* dyn_offsets, const uint8_t* base_scalars, bool profiled) {
    using namespace zk::zkvm;
    zkgpu_ctx* c = sigs(slot);
    zkgpu_ctx* kc = keys(chain.key_slot);
    zkgpu_verifier::TxSigStage& ss = sig(slot);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    TRY(refuse_if_pending(c));
    DeviceGuard g(c->device);
    if (!format_.forms_musig()) { c->last_error = "a signature stage with the host's IDs on a device that does not form the coefficients"; return ZKGPU_EINVAL; }
    hipStream_t key_stream = nullptr;
    {
      std::lock_guard<std::recursive_mutex> kl(kc->mu);
      if (!kc->pending || kc->split.kind != 1 || !kc->split.values || kc->split.batch != rows) { c->last_error = "no key stage of these rows in flight in the slot"; return ZKGPU_EINVAL; }
      key_stream = kc->split.stream;
    }
    if (!musig_rows_fit(dyn_offsets, rows, 1) || dyn_offsets[0] != 0) { c->last_error = "a signature row without its R or a key"; return ZKGPU_EINVAL; }
    TRY(musig_const(c));
    if (!v_->tx_sig_const.p) {                           // once per verifier: what tx_finish_signature hashes, written down
      SigScript sc;
      if (!sig_script(sc)) { c->last_error = "the signature transcript does not fit the device's script"; return ZKGPU_EINVAL; }
      TRY(const_upload(c, v_->tx_sig_const, &sc, sizeof sc));
    }
    if (!ss.ev_keys) HIP_TRY(c, hipEventCreateWithFlags(&ss.ev_keys, hipEventDisableTiming));
    TRY(verify_ps_upload(c, rows, dyn_scalars, dyn_points, dyn_offsets, base_scalars, sidx_[slot].data(), soff_[slot].data()));
    TRY(upload(c, ss.d_ids, chain.txids, rows * 32));
    if (ss.h_pos.size() < rows) { const size_t old = ss.h_pos.size(); ss.h_pos.resize(rows); for (size_t r = old; r < rows; ++r) ss.h_pos[r] = (uint32_t)r; }
    TRY(upload(c, ss.d_pos, ss.h_pos.data(), rows * 4));  // (a row's ID is its own: the identity)
    c->profiling = profiled;
    TRY(musig_launch(c, rows, 1));
    HIP_TRY(c, hipEventRecord(ss.ev_keys, key_stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, ss.ev_keys, 0));
    SigRowsView view{(const SigScript*)v_->tx_sig_const.p, (const uint32_t*)ss.d_ids.p, (const uint32_t*)ss.d_pos.p, (const uint32_t*)kc->values.p,
                     (const uint64_t*)c->in_offsets.p, (const uint32_t*)c->in_points.p, (uint32_t*)c->in_scalars.p, (uint32_t)rows};
    {
      Launch l(c, "k_tx_sig_rows", c->stream);
      hipLaunchKernelGGL(zk::k_tx_sig_rows, dim3(blocks_for(rows, 64)), dim3(64), 0, c->stream, view);
    }
    HIP_TRY(c, hipGetLastError());
    return ZKGPU_OK;
  }
  // (errors are kept by the slot's key context, whose runtime-call macros these are)
  static int pinned_grow(zkgpu_ctx* c, void*& p, size_t& cap, size_t bytes) {
    if (bytes <= cap) return ZKGPU_OK;
    if (p) HIP_TRY(c, hipHostFree(p));
    p = nullptr; cap = 0;
    HIP_TRY(c, hipHostMalloc(&p, bytes + bytes / 8 + 4096, hipHostMallocDefault));
    cap = bytes + bytes / 8 + 4096;
    return ZKGPU_OK;
  }
  int hash_queue(int slot, const zk::zkvm::TxHashTape& tape) {
    using namespace zk::zkvm;
    zkgpu_ctx* c = keys(slot);
    zkgpu_verifier::TxHashStage& hs = hash(slot);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hs.n_tx = 0;
    TRY(hash_stream_and_const(c, hs));
    const HashTapeHead& h = tape.head();
    const size_t bytes = tape.bytes(), id_bytes = 32 * (size_t)h.n_tx;
    TRY(pinned_grow(c, hs.h_in, hs.h_in_cap, bytes));
    TRY(pinned_grow(c, hs.h_out, hs.h_out_cap, id_bytes));
    TRY(ensure(c, hs.d_tape, bytes));
    TRY(ensure(c, hs.d_slots, 32 * (size_t)h.n_slots + 32));
    TRY(ensure(c, hs.d_txid, id_bytes));
    memcpy(hs.h_in, tape.block(), bytes);
    HIP_TRY(c, hipMemcpyAsync(hs.d_tape.p, hs.h_in, bytes, hipMemcpyHostToDevice, hs.stream));
    HashTapeView view{(const uint32_t*)hs.d_tape.p, (const uint32_t*)v_->tx_hash_const.p,
                      (const uint8_t*)v_->tx_hash_const.p + 4 * (size_t)N_PROTO * TAPE_PROTO_WORDS, (uint32_t*)hs.d_slots.p, (uint32_t*)hs.d_txid.p};
    // (a profiled call: the stage's context takes the root's switch for the stage's launches alone, as a chained signature
    // stage's does -- hash_wait hands what they recorded to the root's profile; nothing else ever runs profiled on this context)
    bool profiled = false;
    { std::lock_guard<std::recursive_mutex> rl(v_->root->mu); profiled = v_->root->profiling; }
    c->profiling = profiled;
    if (levels_) {
      TRY(levels_queue(c, hs, tape, view));
    } else {
      Launch l(c, "k_tx_hash", hs.stream);
      hipLaunchKernelGGL(zk::k_tx_hash, dim3(h.n_lanes / 64), dim3(64), 0, hs.stream, view, h.n_lanes);
    }
    c->profiling = false;
    HIP_TRY(c, hipGetLastError());
    // (a chain beside ZKGPU_TXFORMAT_RETURN_LOG: its challenge kernel waits for the IDs, not for the gather and the copies queued
    // below -- the event it waits for is recorded here; without the flag chain_queue records its own, as it always has)
    hs.ids_marked = false;
    if (format_.chains() && (format_.log_k() || format_.root()) && h.n_tx) {     // (... nor for the leaves and the folds of a call that returns its root)
      if (!hs.ev_ids) HIP_TRY(c, hipEventCreateWithFlags(&hs.ev_ids, hipEventDisableTiming));
      HIP_TRY(c, hipEventRecord(hs.ev_ids, hs.stream));
      hs.ids_marked = true;
    }
    // (a chain reads them on the device: they come down only for a caller that is handed them)
    if (!format_.chains() || format_.ids()) HIP_TRY(c, hipMemcpyAsync(hs.h_out, hs.d_txid.p, id_bytes, hipMemcpyDeviceToHost, hs.stream));
    // (the caller is handed the log: the contract IDs its entries name, gathered from the slots into n_tx x K x 32 dense bytes)
    hs.logged = false;
    if (format_.log_k() && h.n_tx) {
      if (!tx_log_table(tape.block(), hs.log_table) || !tx_log_lanes_fit(h.n_tx, format_.log_k())) { c->last_error = "a log entry outside its transaction's slots"; return ZKGPU_EINVAL; }
      const size_t tab_bytes = 4 * hs.log_table.size(), log_bytes = 32 * format_.log_k() * (size_t)h.n_tx;
      TRY(pinned_grow(c, hs.h_tab, hs.h_tab_cap, tab_bytes));
      TRY(pinned_grow(c, hs.h_log, hs.h_log_cap, log_bytes));
      TRY(ensure(c, hs.d_tab, tab_bytes));
      TRY(ensure(c, hs.d_log, log_bytes));
      memcpy(hs.h_tab, hs.log_table.data(), tab_bytes);
      HIP_TRY(c, hipMemcpyAsync(hs.d_tab.p, hs.h_tab, tab_bytes, hipMemcpyHostToDevice, hs.stream));
      c->profiling = profiled;
      {
        Launch l(c, "k_tx_log_gather", hs.stream);
        hipLaunchKernelGGL(zk::k_tx_log_gather, dim3(blocks_for((uint64_t)h.n_tx * format_.log_k(), 64)), dim3(64), 0, hs.stream, (const uint32_t*)hs.d_tape.p,
                           (const uint32_t*)hs.d_tab.p, (const uint32_t*)hs.d_slots.p, (uint32_t*)hs.d_log.p, h.n_tx, (uint32_t)format_.log_k());
      }
      c->profiling = false;
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(hs.h_log, hs.d_log.p, log_bytes, hipMemcpyDeviceToHost, hs.stream));
      hs.n_logged = tx_log_handed_back(tape.block(), hs.log_table, format_.log_k());
      hs.logged = true;
    }
    if (format_.root() && h.n_tx) TRY(root_leaves_queue(c, hs, tape, profiled));
    hs.n_tx = h.n_tx;
    return ZKGPU_OK;
  }
  // the slot's stream, and once per verifier the protocols' initial transcripts and the label table (c->mu held, the device set)
  int hash_stream_and_const(zkgpu_ctx* c, zkgpu_verifier::TxHashStage& hs) {
    if (!hs.stream) {
      int least = 0, greatest = 0;
      HIP_TRY(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
      HIP_TRY(c, hipStreamCreateWithPriority(&hs.stream, hipStreamNonBlocking, greatest));
    }
    if (!v_->tx_hash_const.p) {
      std::vector<uint32_t> protos;
      std::vector<uint8_t> labels;
      zk::zkvm::hash_tape_constants(protos, labels);
      TRY(const_upload(c, v_->tx_hash_const, protos.data(), 4 * protos.size(), labels.data(), labels.size()));
    }
    return ZKGPU_OK;
  }
  // ---- the roots of a call (tx_root_kernels.hpp).  The call's stage: a lone call's is [0], a round's its set's
  zkgpu_verifier::TxRootStage& root_stage() const { return v_->tx_root[sb_ & 1]; }
  int slot_index(int slot) const { return (sb_ + slot) & 1; }
  zk::zkvm::TxRootView root_view() const {
    return zk::zkvm::TxRootView{(const uint32_t*)v_->tx_root_const.p, (const uint8_t*)v_->tx_hash_const.p + 4 * (size_t)zk::zkvm::N_PROTO * zk::zkvm::TAPE_PROTO_WORDS};
  }
  // a call of `total` transactions starts: its leaves read zero, on slot 0's stream; the event says when
  int root_zero(size_t total) {
    zkgpu_ctx* c = keys(0);
    zkgpu_verifier::TxHashStage& hs = hash(0);
    zkgpu_verifier::TxRootStage& rs = root_stage();
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    rs.total = 0; rs.n_ranges = 0; rs.marked[0] = rs.marked[1] = false;
    if (total == 0 || total >= (1ull << 31)) { c->last_error = "a call without transactions has no leaves"; return ZKGPU_EINVAL; }
    TRY(hash_stream_and_const(c, hs));
    if (!v_->tx_root_const.p) {                          // once per verifier: the tree's freshly initialised transcript
      uint32_t init[zk::zkvm::TAPE_PROTO_WORDS];
      zk::zkvm::tx_root_init(init);
      TRY(const_upload(c, v_->tx_root_const, init, sizeof init));
    }
    if (!rs.ev_zeroed) HIP_TRY(c, hipEventCreateWithFlags(&rs.ev_zeroed, hipEventDisableTiming));
    TRY(ensure(c, rs.d_leaves, 32 * total));
    for (Buffer& b : rs.d_nodes) TRY(ensure(c, b, 32 * ((total + 1) / 2)));
    HIP_TRY(c, hipMemsetAsync(rs.d_leaves.p, 0, 32 * total, hs.stream));
    HIP_TRY(c, hipEventRecord(rs.ev_zeroed, hs.stream));
    rs.zero_stream = hs.stream;
    rs.total = total;
    return ZKGPU_OK;
  }
  // the stream behind the zeroing of the call's leaves (its own stream already is)
  int root_behind_zeroing(zkgpu_ctx* c, zkgpu_verifier::TxHashStage& hs, zkgpu_verifier::TxRootStage& rs) {
    if (hs.stream != rs.zero_stream) HIP_TRY(c, hipStreamWaitEvent(hs.stream, rs.ev_zeroed, 0));
    return ZKGPU_OK;
  }
  // behind the tape just queued on hs.stream: its transactions' places in the call up, a leaf per transaction, the slot's event
  // (c->mu held, the device set)
  int root_leaves_queue(zkgpu_ctx* c, zkgpu_verifier::TxHashStage& hs, const zk::zkvm::TxHashTape& tape, bool profiled) {
    zkgpu_verifier::TxRootStage& rs = root_stage();
    const size_t n = tape.n_tx();
    if (rs.total == 0 || !v_->tx_root_const.p) { c->last_error = "a tape of a call whose leaves were never zeroed"; return ZKGPU_EINVAL; }
    TRY(pinned_grow(c, hs.h_root_pos, hs.h_root_pos_cap, 4 * n));
    TRY(ensure(c, hs.d_root_pos, 4 * n));
    uint32_t* pos = (uint32_t*)hs.h_root_pos;
    for (size_t t = 0; t < n; ++t) {
      const size_t at = hs.place + tape.position(t);
      if (at >= rs.total) { c->last_error = "a transaction of the tape lies outside its call"; return ZKGPU_EINVAL; }
      pos[t] = (uint32_t)at;
    }
    if (!hs.ev_leaves) HIP_TRY(c, hipEventCreateWithFlags(&hs.ev_leaves, hipEventDisableTiming));
    HIP_TRY(c, hipMemcpyAsync(hs.d_root_pos.p, hs.h_root_pos, 4 * n, hipMemcpyHostToDevice, hs.stream));
    TRY(root_behind_zeroing(c, hs, rs));
    c->profiling = profiled;
    {
      Launch l(c, "k_tx_root_leaves", hs.stream);
      hipLaunchKernelGGL(zk::k_tx_root_leaves, dim3(blocks_for(n, 64)), dim3(64), 0, hs.stream, root_view(), (const uint32_t*)hs.d_txid.p,
                         (const uint32_t*)hs.d_root_pos.p, (uint32_t)n, (uint32_t*)rs.d_leaves.p, (uint32_t)rs.total);
    }
    c->profiling = false;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(hs.ev_leaves, hs.stream));
    rs.marked[&hs == &v_->tx_hash[0] ? 0 : 1] = true;
    return ZKGPU_OK;
  }
  // behind the call's last tape, on its slot's stream: the other slot's leaves waited for (on the device), every range folded
  // pass by pass between the two node arrays, its root copied beside the others, all of them down in one copy
  int root_queue(int slot, const uint64_t* ranges, size_t n_ranges) {
    using namespace zk::zkvm;
    zkgpu_ctx* c = keys(slot);
    zkgpu_verifier::TxHashStage& hs = hash(slot);
    zkgpu_verifier::TxHashStage& other = hash(slot ^ 1);
    zkgpu_verifier::TxRootStage& rs = root_stage();
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    rs.n_ranges = 0;
    if (rs.total == 0 || n_ranges == 0) { c->last_error = "no call whose roots could be folded"; return ZKGPU_EINVAL; }
    for (size_t r = 0; r < n_ranges; ++r)
      if (ranges[2 * r] > rs.total || ranges[2 * r + 1] > rs.total - ranges[2 * r]) { c->last_error = "a root over transactions outside the call"; return ZKGPU_EINVAL; }
    TRY(hash_stream_and_const(c, hs));
    TRY(pinned_grow(c, rs.h_roots, rs.h_roots_cap, 32 * n_ranges));
    TRY(ensure(c, rs.d_roots, 32 * n_ranges));
    TRY(root_behind_zeroing(c, hs, rs));
    if (rs.marked[slot_index(slot ^ 1)] && other.ev_leaves && other.stream != hs.stream) HIP_TRY(c, hipStreamWaitEvent(hs.stream, other.ev_leaves, 0));
    bool profiled = false;
    { std::lock_guard<std::recursive_mutex> rl(v_->root->mu); profiled = v_->root->profiling; }
    const uint32_t s = root_span_;
    const TxRootView view = root_view();
    HIP_TRY(c, hipMemsetAsync(rs.d_roots.p, 0, 32 * n_ranges, hs.stream));     // (a range of no transaction keeps zeros: the empty tree's hash is the host's)
    for (size_t r = 0; r < n_ranges; ++r) {
      const uint32_t* in = (const uint32_t*)rs.d_leaves.p + TX_ROOT_NODE_WORDS * (size_t)ranges[2 * r];
      uint64_t count = ranges[2 * r + 1];
      if (count == 0) continue;
      for (uint32_t pass = 0; count > 1; ++pass) {
        const uint64_t next = tx_root_after_pass(count, s);
        uint32_t* out = (uint32_t*)rs.d_nodes[pass & 1].p;
        c->profiling = profiled;
        {
          Launch l(c, "k_tx_root_fold", hs.stream);
          hipLaunchKernelGGL(zk::k_tx_root_fold, dim3((uint32_t)next), dim3(TX_ROOT_LANES), 0, hs.stream, view, in, (uint32_t)count, out, s);
        }
        c->profiling = false;
        HIP_TRY(c, hipGetLastError());
        in = out; count = next;
      }
      HIP_TRY(c, hipMemcpyAsync((char*)rs.d_roots.p + 32 * r, in, 32, hipMemcpyDeviceToDevice, hs.stream));
    }
    HIP_TRY(c, hipMemcpyAsync(rs.h_roots, rs.d_roots.p, 32 * n_ranges, hipMemcpyDeviceToHost, hs.stream));
    rs.n_ranges = n_ranges;
    return ZKGPU_OK;
  }
  int root_wait(int slot, uint8_t* roots) {
    zkgpu_ctx* c = keys(slot);
    zkgpu_verifier::TxHashStage& hs = hash(slot);
    zkgpu_verifier::TxRootStage& rs = root_stage();
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    const size_t n = rs.n_ranges;
    rs.n_ranges = 0;
    if (n == 0 || !hs.stream) { c->last_error = "no roots in flight in the slot"; return ZKGPU_EINVAL; }
    HIP_TRY(c, hipStreamSynchronize(hs.stream));
    memcpy(roots, rs.h_roots, 32 * n);
    if (!c->ev_used.empty()) { prof_collect(c); profile_to_root(c); }     // (a profiled call: the folds have run)
    return ZKGPU_OK;
  }
  static bool levels_asked() {
    const char* e = getenv("ZKGPU_TX_HASH_LEVELS");
    return e && (e[0] == '0' || e[0] == '1') ? e[0] == '1' : TX_HASH_LEVELS_SERVE;
  }
  // the tape by dependency level: its side table up beside it, then k_tx_hash_levels -- 4 lanes per entry of the lane table, 16
  // entries per block (c->mu held, the device set, c->profiling as the launch wants it; after an error the switch is off again)
  int levels_queue(zkgpu_ctx* c, zkgpu_verifier::TxHashStage& hs, const zk::zkvm::TxHashTape& tape, const zk::zkvm::HashTapeView& view) {
    using namespace zk::zkvm;
    const HashTapeHead& h = tape.head();
    auto queue = [&]() -> int {
      if (!tx_hash_levels_table(tape.block(), hs.levels_table)) { c->last_error = "the tape's jobs have no order by levels"; return ZKGPU_EINVAL; }
      const size_t tab_bytes = 4 * hs.levels_table.size();
      TRY(pinned_grow(c, hs.h_levels, hs.h_levels_cap, tab_bytes));
      TRY(ensure(c, hs.d_levels, tab_bytes));
      memcpy(hs.h_levels, hs.levels_table.data(), tab_bytes);
      HIP_TRY(c, hipMemcpyAsync(hs.d_levels.p, hs.h_levels, tab_bytes, hipMemcpyHostToDevice, hs.stream));
      const HashLevelsView lv{(const uint32_t*)hs.d_levels.p, (uint32_t)hs.levels_table.size()};
      if (h.n_lanes == 0) return ZKGPU_OK;
      Launch l(c, "k_tx_hash_levels", hs.stream);
      hipLaunchKernelGGL(zk::k_tx_hash_levels, dim3(h.n_lanes / (64 / TAPE_LEVEL_LANES)), dim3(64), 0, hs.stream, view, lv, h.n_lanes);
      return ZKGPU_OK;
    };
    const int rc = queue();
    if (rc != ZKGPU_OK) c->profiling = false;
    return rc;
  }
  int hash_wait(int slot, uint8_t* txids) {
    zkgpu_ctx* c = keys(slot);
    zkgpu_verifier::TxHashStage& hs = hash(slot);
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    const size_t n = hs.n_tx;
    hs.n_tx = 0;
    if (n == 0) return ZKGPU_OK;
    HIP_TRY(c, hipStreamSynchronize(hs.stream));
    if (txids && (!format_.chains() || format_.ids())) memcpy(txids, hs.h_out, 32 * n);
    if (!c->ev_used.empty()) { prof_collect(c); profile_to_root(c); }     // (a profiled stage: its launches have run)
    { std::lock_guard<std::recursive_mutex> rl(v_->root->mu); v_->root->tx_hashed_on_device += n; if (hs.logged) v_->root->tx_logged_on_device += hs.n_logged; }
    return ZKGPU_OK;
  }
  // (an error's text: the context's, behind the name of the stage where a test or a caller tells stages by it)
  int seen(int rc, zkgpu_ctx* where, const char* stage = "") { if (rc != ZKGPU_OK) err_ = std::string(stage) + zkgpu_last_error(where); return rc; }
  zkgpu_ctx* keys(int slot) const { return v_->aux_keys[(sb_ + slot) & 1]; }
  zkgpu_ctx* sigs(int slot) const { return v_->aux_sigs[(sb_ + slot) & 1]; }
  zkgpu_verifier* v_;
  const int sb_;
  const size_t ab_;
  const zk::zkvm::TxFormat format_;                      // the mode of the call (tx_out.hpp): its predicates are asked where they matter
  const bool levels_;                                    // (a precompute-only call) its tapes are walked by level: the environment may say otherwise
  const uint32_t root_span_ = g_tx_root_span;            // levels per pass of the root's folds (ZKGPU_TX_ROOT_SPAN, read when the library was loaded)
  std::vector<uint32_t> sidx_[2];
  std::vector<uint64_t> soff_[2];
  std::string err_;
};

}  // namespace
