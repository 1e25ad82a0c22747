// tx_reason_kernels.hpp -- WHY a statement was rejected, as one byte per statement (include/zkgpu.h: ZKGPU_TXSTATUS_*).
//
// Upstream's Tx::verify returns Result<VerifiedTx, VMError>: the caller learns which check failed.  The device already
// tells the three ways a proof is bad apart -- the well-formedness flag of the unpack / transcript kernels, the "a point did
// not decode" flag of the point decoding, the identity test behind the accept bit -- and folds them into the accept bitmap.
// The kernels here read those flags once the batch's bitmap is FINAL (after the fold; where a group failed, after the
// locate / re-check tail) and write the lowest code that applies.  They are queued only for a device batch that a
// format-2 transaction call asked for (zkgpu_ctx::want_reasons); nothing else launches them.
//
// The codes are restated here because kernels.hpp does not see zkgpu.h; session.hpp asserts that they agree.
#pragma once
#include <stdint.h>

namespace zk {

enum : uint8_t {
  TXR_ACCEPTED = 0, TXR_REJECTED = 1,
  TXR_TX_INVALID = 16, TXR_PROOF_FORMAT = 17, TXR_PROOF_POINT = 18, TXR_PROOF_EQUATION = 19, TXR_KEY = 20, TXR_SIGNATURE = 21,
};

// Whole proofs, one thread per statement.  wellformed / msm_fail: the batch's flags as the pipeline left them (one word per
// statement); bitmap: the final accept bitmap.  Precedence is by code, lowest first: a malformed proof with an undecodable
// point reads "format", as upstream's R1CSProof::from_bytes fails before any point is decompressed.
__global__ void __launch_bounds__(256)
k_tx_reason_proofs(const uint32_t* __restrict__ wellformed, const uint32_t* __restrict__ msm_fail, const uint8_t* __restrict__ bitmap,
                   uint32_t n, uint8_t* __restrict__ reason) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t code = TXR_ACCEPTED;
  if (wellformed && !wellformed[i]) code = TXR_PROOF_FORMAT;
  else if (msm_fail[i]) code = TXR_PROOF_POINT;
  else if (!((bitmap[i >> 3] >> (i & 7)) & 1)) code = TXR_PROOF_EQUATION;
  reason[i] = code;
}

// The key stage and the signature stage of a transaction call, one thread per row: a stage has ONE way to fail a row that
// got this far (key stage: a key does not decode; signature stage: R, s or the equation -- the rows are the transactions
// whose keys all decode), so the code is the stage's, written beside a clear bit.
__global__ void __launch_bounds__(256)
k_tx_reason_stage(const uint8_t* __restrict__ bitmap, uint32_t n, uint32_t code_when_clear, uint8_t* __restrict__ reason) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  reason[i] = ((bitmap[i >> 3] >> (i & 7)) & 1) ? (uint8_t)TXR_ACCEPTED : (uint8_t)code_when_clear;
}

}  // namespace zk
