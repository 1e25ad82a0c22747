"""Host-side mirror of the reference's verification API for the path this repo accelerates.

Upstream (slingshot/zkvm, Rust; not mounted under /root/reference -- SURVEY.md sec 8(b)):

    Tx::verify(&self, bp_gens: &BulletproofGens) -> Result<VerifiedTx, VMError>
    Verifier::verify_tx(tx: &Tx, bp_gens: &BulletproofGens) -> Result<VerifiedTx, VMError>

Both run the VM over the program (out of scope here: SURVEY.md sec 2) and then spend their
time in `r1cs::Verifier::verify(proof, pc_gens, bp_gens)`.  `Verifier.verify_cloak_txs` below
is that second half for a batch: same inputs a `cloak` instruction leaves behind (value
commitments + R1CSProof bytes), same per-transaction Ok / Err outcome, one GPU call.

`BulletproofGens(gens_capacity)` mirrors `BulletproofGens::new(gens_capacity, 1)`: it owns the
device-resident generator set (and its fixed-base tables) instead of a Vec<RistrettoPoint>.
"""
from __future__ import annotations

import ctypes as C
import numpy as np
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence

from .native import Context, PointSet, ZkGpuError


class VMError(Exception):
    """Mirror of zkvm::VMError for the variants this path can produce."""


class InvalidR1CSProof(VMError):
    """VMError::InvalidR1CSProof.  `reason`: the status byte of a transaction call with reasons (TXSTATUS_PROOF_FORMAT,
    _PROOF_POINT or _PROOF_EQUATION: upstream has the one variant for the three), None where no reason is known."""
    reason: Optional[int] = None


class TxFormatError(VMError):
    """The transaction itself was rejected before any proof or signature was looked at (TXSTATUS_TX_INVALID): wire format,
    time bounds, a program or VM error -- upstream's VMError::FormatError and the VM's own variants, which this path keeps
    as one code."""
    reason: Optional[int] = None


class InvalidSignature(VMError):
    """The deferred signature check failed (TXSTATUS_KEY: a key the signature must cover does not decode; TXSTATUS_SIGNATURE:
    R, s or the equation) -- upstream's VMError::InvalidPoint / the musig error of Signature::verify, as recalled."""
    reason: Optional[int] = None


def tx_errors(status) -> List[Optional[VMError]]:
    """status bytes of verify_txs / wait_txs -> per transaction None (accepted) or the VMError upstream's Tx::verify would
    return, as recalled: TxFormatError (16), InvalidR1CSProof (17, 18, 19), InvalidSignature (20, 21), each
    with the code as `.reason`; a plain VMError for "rejected, no reason known" (1), for a transaction outside the subset
    (2: not an error of the transaction -- the caller's own VM decides) and for a byte this version does not know."""
    texts = {1: "rejected (no reason available)", 2: "outside the subset this library verifies: ask your own VM",
             16: "the transaction is malformed or its program failed in the VM", 17: "R1CS proof is malformed",
             18: "a commitment or proof point is not a ristretto255 encoding", 19: "R1CS proof did not verify",
             20: "a verification key does not decode", 21: "the transaction signature did not verify"}
    kinds = {16: TxFormatError, 17: InvalidR1CSProof, 18: InvalidR1CSProof, 19: InvalidR1CSProof, 20: InvalidSignature, 21: InvalidSignature}
    out: List[Optional[VMError]] = []
    for b in bytes(status):
        if b == 0:
            out.append(None)
            continue
        e = kinds.get(b, VMError)(texts.get(b, "unknown status byte %d" % b))
        e.reason = b
        out.append(e)
    return out


@dataclass
class CloakTx:
    """What a ZkVM `cloak` leaves for the proof system: (quantity, flavor) commitments of the
    inputs then the outputs (64 bytes per value) and the R1CSProof encoding."""
    n_in: int
    n_out: int
    commitments: bytes
    proof: bytes


class BulletproofGens:
    def __init__(self, ctx: Context, gens_capacity: int, table_bits: int = 0):
        self.ctx = ctx
        self.gens_capacity = gens_capacity
        b, bb = ctx.pedersen_gens()
        g, h = ctx.bulletproof_gens(gens_capacity)
        self.points = PointSet(ctx, b + bb + g + h)
        if table_bits:                 # -1: the library chooses the width (zkgpu_pointset_build_tables(.., 0)); 0: no tables
            self.points.build_tables(0 if table_bits < 0 else table_bits)

    def close(self) -> None:
        self.points.close()


class Prover:
    """Batch prover for cloak statements (zkgpu_cloak_prove_batch): the whole proof on the device (Context.set_prover_mode(1):
    host threads drive the provers in lockstep), every multiscalar multiplication on the generator tables."""

    def __init__(self, ctx: Context, bp_gens: BulletproofGens, host_threads: int = 0):
        self.ctx = ctx
        self.bp_gens = bp_gens
        self.host_threads = host_threads

    def prove_packed(self, n_in: int, n_out: int, batch: int, quantities, flavors: bytes, seeds: Optional[bytes] = None):
        """zkgpu_cloak_prove_batch on contiguous inputs (quantities: ctypes array of batch x (n_in + n_out) u64; flavors 32 B
        per value; seeds: None -- the library draws the call's randomness itself, the recommended form -- or 32 B per
        statement, never used for two statements) -> (commitments, proofs with stride 1569, proof_len); no per-proof Python work"""
        nv = n_in + n_out
        if len(flavors) != 32 * nv * batch or (seeds is not None and len(seeds) != 32 * batch) or len(quantities) != nv * batch:
            raise ValueError("quantities: one per value; flavors: 32 bytes per value; seeds: 32 bytes per statement, or None")
        import time
        com = C.create_string_buffer(max(64 * nv * batch, 1))
        stride = 1 + 32 * (16 + 2 * 16)
        proofs = C.create_string_buffer(max(stride * batch, 1))
        plen = C.c_size_t(0)
        t0 = time.perf_counter()
        rc = self.ctx.lib.zkgpu_cloak_prove_batch(self.ctx.h, self.bp_gens.points.h, self.bp_gens.gens_capacity, batch, n_in, n_out,
                                                  quantities, flavors, seeds, self.host_threads, com, proofs, stride, C.byref(plen))
        self.last_call_s = time.perf_counter() - t0
        self.ctx._check(rc)
        return com, proofs, plen.value

    def prove(self, n_in: int, n_out: int, quantities: Sequence[Sequence[int]], flavors: Sequence[Sequence[bytes]],
              seeds: Optional[Sequence[bytes]] = None) -> List[CloakTx]:
        """seeds: None -- the library draws the call's randomness itself (the batch is then len(quantities)) -- or one 32-byte
        seed per statement, never used for two statements"""
        batch, nv = len(quantities) if seeds is None else len(seeds), n_in + n_out
        assert len(quantities) == batch and len(flavors) == batch
        qa = (C.c_uint64 * max(batch * nv, 1))(*[q for row in quantities for q in row])
        fl = b"".join(f for row in flavors for f in row)
        com = C.create_string_buffer(max(64 * nv * batch, 1))
        stride = 1 + 32 * (16 + 2 * 16)
        proofs = C.create_string_buffer(max(stride * batch, 1))
        plen = C.c_size_t(0)
        import time
        sd = None if seeds is None else b"".join(seeds)
        t0 = time.perf_counter()
        rc = self.ctx.lib.zkgpu_cloak_prove_batch(
            self.ctx.h, self.bp_gens.points.h, self.bp_gens.gens_capacity, batch, n_in, n_out, qa, fl, sd,
            self.host_threads, com, proofs, stride, C.byref(plen))
        self.last_call_s = time.perf_counter() - t0          # the library call alone (bench.py)
        self.ctx._check(rc)
        return [CloakTx(n_in, n_out, com.raw[64 * nv * i: 64 * nv * (i + 1)], proofs.raw[stride * i: stride * i + plen.value])
                for i in range(batch)]


def _check_packed(n_in: int, n_out: int, batch: int, commitments: bytes, proofs: bytes, proof_len: int,
                  r_bytes: Optional[bytes]) -> None:
    """The C ABI sees pointers only: a short buffer would be a host heap over-read."""
    if len(commitments) != batch * 64 * (n_in + n_out):
        raise ValueError("commitments must hold 64 bytes per value and transaction")
    if len(proofs) != batch * proof_len:
        raise ValueError("proofs must hold proof_len bytes per transaction")
    if r_bytes is not None and len(r_bytes) != 64 * batch:
        raise ValueError("r_bytes must hold 64 bytes per transaction")


def _marshal_block(txs: Sequence[CloakTx], r_bytes: Optional[bytes]):
    batch = len(txs)
    offs = [0]
    for t in txs:
        if len(t.commitments) != 64 * (t.n_in + t.n_out):
            raise ValueError("commitments must hold 64 bytes per value")
        offs.append(offs[-1] + len(t.proof))
    if r_bytes is not None and len(r_bytes) != 64 * batch:
        raise ValueError("r_bytes must hold 64 bytes per transaction")
    return ((C.c_uint32 * max(batch, 1))(*[t.n_in for t in txs]), (C.c_uint32 * max(batch, 1))(*[t.n_out for t in txs]),
            b"".join(t.commitments for t in txs), b"".join(t.proof for t in txs), (C.c_uint64 * (batch + 1))(*offs))


class TxBlock:
    """zkgpu_txblock: a block of transactions of mixed shapes, grouped by shape and resident in HBM."""

    def __init__(self, bv: "BlockVerifier", txs: Sequence[CloakTx], r_bytes: Optional[bytes] = None):
        self.bv = bv
        self.n = len(txs)
        self.h = C.c_void_p()
        n_in, n_out, com, proofs, po = _marshal_block(txs, r_bytes)
        bv._check(bv.lib.zkgpu_txblock_create(bv.h, self.n, n_in, n_out, com, proofs, po, r_bytes, C.byref(self.h)))

    def shapes(self) -> int:
        return int(self.bv.lib.zkgpu_txblock_shapes(self.h))

    def close(self) -> None:
        if self.h:
            self.bv.lib.zkgpu_txblock_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BlockVerifier:
    """zkgpu_verifier: whole blocks of transactions of any mix of shapes (BASELINE configs[3]); the shape
    grouping, the plans and the batches in flight are the library's."""

    def __init__(self, ctx: Context, bp_gens: BulletproofGens, batches_in_flight: int = 0, chunk: int = 0):
        self.ctx, self.lib, self.bp_gens = ctx, ctx.lib, bp_gens
        self.h = C.c_void_p()
        rc = self.lib.zkgpu_verifier_create(ctx.h, bp_gens.points.h, bp_gens.gens_capacity, batches_in_flight, C.byref(self.h))
        # ZKGPU_WSECOND_VERIFIER (1): created, with a warning -- another verifier is alive on this device
        self.warning = self.lib.zkgpu_verifier_last_error(self.h).decode() if rc == 1 else ""
        if rc != 1:
            ctx._check(rc)
        self._runs = {}
        if chunk:
            self._check(self.lib.zkgpu_verifier_set_chunk(self.h, chunk))

    def _check(self, rc: int) -> None:
        if rc != 0:
            detail = self.lib.zkgpu_verifier_last_error(self.h).decode() if self.h else ""
            raise ZkGpuError(rc, self.lib.zkgpu_strerror(rc).decode() + (": " + detail if detail else ""))

    def lanes(self) -> int:
        return int(self.lib.zkgpu_verifier_lanes(self.h))

    def queue_info(self):
        """zkgpu_verifier_queue_info -> (lanes in use, lanes asked for, lanes dropped because they would not run beside the
        others, 1 when the HIP runtime had started before GPU_MAX_HW_QUEUES was set)"""
        out = (C.c_int * 4)()
        self._check(self.lib.zkgpu_verifier_queue_info(self.h, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def lane(self, i: int) -> Context:
        """zkgpu_verifier_lane: lane i's context (owned by the verifier) for set_group_size / the profile hooks."""
        return Context(_borrowed=int(self.lib.zkgpu_verifier_lane(self.h, i)))

    def verify(self, txs: Sequence[CloakTx], r_bytes: Optional[bytes] = None) -> bytes:
        batch = len(txs)
        n_in, n_out, com, proofs, po = _marshal_block(txs, r_bytes)
        bm = C.create_string_buffer(max((batch + 7) // 8, 1))
        self._check(self.lib.zkgpu_verifier_verify(self.h, batch, n_in, n_out, com, proofs, po, r_bytes, bm))
        return bm.raw[: (batch + 7) // 8]

    def set_merge(self, transactions: int) -> None:
        self._check(self.lib.zkgpu_verifier_set_merge(self.h, transactions))

    def reserve(self, n_in: int, n_out: int, transactions: int) -> None:
        """zkgpu_verifier_reserve: every lane's workspace sized for device batches of that many statements of the shape"""
        self._check(self.lib.zkgpu_verifier_reserve(self.h, n_in, n_out, transactions))

    def submit_dev(self, n_in: int, n_out: int, batch: int, d_commitments, d_proofs, proof_len: int, d_r=None) -> int:
        """zkgpu_verifier_submit_dev: queue one uniform batch (device buffers); -> ticket.  d_r None (recommended): the
        library draws the verifier randomness itself, per device batch."""
        from .native import _ptr
        t = C.c_uint64(0)
        self._check(self.lib.zkgpu_verifier_submit_dev(self.h, n_in, n_out, batch, _ptr(d_commitments), _ptr(d_proofs), proof_len,
                                                       _ptr(d_r), C.byref(t)))
        self.__dict__.setdefault("_ticket_batch", {})[t.value] = batch
        return int(t.value)

    def submit_many_dev(self, n_in: int, n_out: int, batch_each: int, d_commitments: Sequence, d_proofs: Sequence, proof_len: int,
                        d_r: Optional[Sequence] = None) -> List[int]:
        """zkgpu_verifier_submit_many_dev: queue len(d_commitments) uniform batches in one call; -> tickets.  d_r None, or
        None entries in it: those batches' verifier randomness is drawn by the library, per device batch."""
        from .native import _ptr
        count = len(d_commitments)
        assert len(d_proofs) == count and (d_r is None or len(d_r) == count)
        arr = lambda xs: None if xs is None else (C.c_void_p * max(count, 1))(*[_ptr(x) for x in xs])
        t = (C.c_uint64 * max(count, 1))()
        self._check(self.lib.zkgpu_verifier_submit_many_dev(self.h, n_in, n_out, count, batch_each, arr(d_commitments), arr(d_proofs),
                                                            proof_len, arr(d_r), t))
        for i in range(count):
            self.__dict__.setdefault("_ticket_batch", {})[t[i]] = batch_each
        return [int(t[i]) for i in range(count)]

    def submit(self, n_in: int, n_out: int, batch: int, commitments: bytes, proofs: bytes, proof_len: int, r_bytes: Optional[bytes]) -> int:
        """zkgpu_verifier_submit: queue one uniform batch from HOST memory (copied into pinned staging memory during the
        call: the buffers are free again when it returns); -> ticket"""
        assert len(commitments) >= batch * 64 * (n_in + n_out) and len(proofs) >= batch * proof_len and (r_bytes is None or len(r_bytes) >= 64 * batch)
        t = C.c_uint64(0)
        self._check(self.lib.zkgpu_verifier_submit(self.h, n_in, n_out, batch, commitments, proofs, proof_len, r_bytes, C.byref(t)))
        self.__dict__.setdefault("_ticket_batch", {})[t.value] = batch
        return int(t.value)

    def submit_many(self, n_in: int, n_out: int, batch_each: int, commitments: Sequence[bytes], proofs: Sequence[bytes], proof_len: int,
                    r_bytes: Optional[Sequence[Optional[bytes]]]) -> List[int]:
        """zkgpu_verifier_submit_many: queue len(commitments) uniform batches from host memory in one call; -> tickets"""
        count = len(commitments)
        assert len(proofs) == count and (r_bytes is None or len(r_bytes) == count)
        for i in range(count):
            assert len(commitments[i]) >= batch_each * 64 * (n_in + n_out) and len(proofs[i]) >= batch_each * proof_len
            assert r_bytes is None or r_bytes[i] is None or len(r_bytes[i]) >= 64 * batch_each
        arr = lambda xs: (C.c_char_p * max(count, 1))(*xs)                # noqa: E731
        t = (C.c_uint64 * max(count, 1))()
        self._check(self.lib.zkgpu_verifier_submit_many(self.h, n_in, n_out, count, batch_each, arr(commitments), arr(proofs), proof_len,
                                                        arr(r_bytes) if r_bytes is not None else None, t))
        for i in range(count):
            self.__dict__.setdefault("_ticket_batch", {})[t[i]] = batch_each
        return [int(t[i]) for i in range(count)]

    def wait(self, ticket: int) -> bytes:
        """zkgpu_verifier_wait: the accept bitmap of that ticket's batch"""
        batch = self.__dict__["_ticket_batch"].pop(ticket)
        bm = C.create_string_buffer(max((batch + 7) // 8, 1))
        self._check(self.lib.zkgpu_verifier_wait(self.h, ticket, bm))
        return bm.raw[: (batch + 7) // 8]

    def block(self, txs: Sequence[CloakTx], r_bytes: Optional[bytes] = None) -> TxBlock:
        return TxBlock(self, txs, r_bytes)

    def verify_block(self, block: TxBlock) -> bytes:
        bm = C.create_string_buffer(max((block.n + 7) // 8, 1))
        self._check(self.lib.zkgpu_verifier_verify_block(self.h, block.h, bm))
        return bm.raw[: (block.n + 7) // 8]

    def block_start(self, block: TxBlock) -> int:
        """zkgpu_verifier_block_start: the block's batches queued, a run id back at once"""
        run = C.c_uint64()
        self._check(self.lib.zkgpu_verifier_block_start(self.h, block.h, C.byref(run)))
        self._runs[int(run.value)] = block.n
        return int(run.value)

    def block_finish(self, run: int) -> bytes:
        """zkgpu_verifier_block_finish: the accept bitmap of the run's block"""
        n = self._runs.pop(run, None)
        if n is None:
            raise ZkGpuError(-1, "no such run in flight")
        bm = C.create_string_buffer(max((n + 7) // 8, 1))
        self._check(self.lib.zkgpu_verifier_block_finish(self.h, run, bm))
        return bm.raw[: (n + 7) // 8]

    TXFORMAT_RECOLLECTED_V1 = 1
    TXFORMAT_RECOLLECTED_V1_REASONS = 2    # the same bytes and the same bitmap; the status bytes say WHY (tx_errors)
    TXFORMAT_HASH_ON_DEVICE = 0x100        # a flag or-ed to either: contract IDs, anchors and the transaction ID hashed on the device
    TXFORMAT_SIGN_ON_DEVICE = 0x200        # a flag or-ed to a format WITH the one above: the signature's challenge formed on the device
    TXFORMAT_RETURN_IDS = 0x400            # a flag or-ed to any of those: the transaction ID of every accepted transaction comes back
    TXFORMAT_RETURN_LOG = 0x800            # a flag only beside the one above, with a window K << TXFORMAT_LOG_SHIFT: the log's entries too
    TXFORMAT_LOG_SHIFT = 16                # bits 16 .. 23 of the format: K, the log entries kept per transaction, 1 .. 255
    TXFORMAT_PRECOMPUTE_ONLY = 0x2000      # a flag only beside TXFORMAT_RETURN_IDS, never beside TXFORMAT_SIGN_ON_DEVICE: NOTHING is verified (precompute_txs)
    TXFORMAT_RETURN_ROOT = 0x10            # a flag only beside TXFORMAT_RETURN_IDS: the Merkle root over the call's transaction IDs comes back too (root=True)
    TXFORMAT_STATEMENTS_V1 = 4             # a third base format: records of what the caller's own VM left (verify_statements); alone or beside TXFORMAT_SIGN_ON_DEVICE
    TXLOG_INPUT, TXLOG_OUTPUT = 1, 2       # kind bytes of a log record (include/zkgpu.h: ZKGPU_TXLOG_*)
    # status bytes (include/zkgpu.h: ZKGPU_TXSTATUS_*); 16 .. 21 only with TXFORMAT_RECOLLECTED_V1_REASONS, lowest code first
    TXSTATUS_ACCEPTED = 0
    TXSTATUS_REJECTED = 1                  # rejected, no reason known (format 1, or any error)
    TXSTATUS_OUTSIDE_SUBSET = 2
    TXSTATUS_PRECOMPUTED = 3               # only under TXFORMAT_PRECOMPUTE_ONLY: the VM ran to the end, ID and log computed -- NOT a verdict
    TXSTATUS_TX_INVALID = 16
    TXSTATUS_PROOF_FORMAT = 17
    TXSTATUS_PROOF_POINT = 18
    TXSTATUS_PROOF_EQUATION = 19
    TXSTATUS_KEY = 20
    TXSTATUS_SIGNATURE = 21

    tx_errors = staticmethod(lambda status: tx_errors(status))    # (the module's helper, where the constants are)

    def set_tx_format(self, fmt: int, log_k: int = 0) -> None:
        """zkgpu_verifier_set_tx_format: the serialized-transaction format zkgpu_tx_verify_batch reads.  0 (the default):
        none -- every transaction is reported as outside the subset; TXFORMAT_RECOLLECTED_V1: the payment subset of
        DESIGN.md sec 4.5, an UNPINNED recollection of the ZkVM wire format (opt-in for exactly that reason);
        TXFORMAT_RECOLLECTED_V1_REASONS: the same, with a reason code in the status byte of every rejected transaction.
        Either may be or-ed with TXFORMAT_HASH_ON_DEVICE (same verdicts; most of the VM's hashing moves to the device), and
        then also with TXFORMAT_SIGN_ON_DEVICE (same verdicts; the signature's challenge is formed on the device as well).
        Any of those may be or-ed with TXFORMAT_RETURN_IDS: same verdicts, and verify_txs / wait_txs called with ids=True also
        return the 32-byte transaction ID of every accepted transaction.  (The library then writes 33 bytes per transaction
        into a call's status array; the arrays here are sized by what THIS method was given last, so set the format through it.)
        A format with TXFORMAT_RETURN_IDS may also carry TXFORMAT_RETURN_LOG and a window K of 1 .. 255 in bits 16 .. 23 -- given
        in `fmt` itself or as log_k=K, which sets both: verify_txs / wait_txs called with log=True then also return the Input /
        Output entries of every accepted transaction's log (the library writes 33 + 1 + 33 K bytes per transaction).
        A format with TXFORMAT_RETURN_IDS and without TXFORMAT_SIGN_ON_DEVICE may carry TXFORMAT_PRECOMPUTE_ONLY: the calls
        then VERIFY NOTHING -- upstream's Tx::precompute alone -- and are made through precompute_txs / submit_txs and
        wait_precomputed; verify_txs and wait_txs refuse, so that a status of 3 is never read as a verdict.
        A format with TXFORMAT_RETURN_IDS may carry TXFORMAT_RETURN_ROOT: the library then writes 32 more bytes behind everything
        else, and verify_txs / wait_txs / precompute_txs / wait_precomputed called with root=True return them as a last element --
        the Merkle root over the call's transaction IDs in call order if EVERY transaction of the call reads 0 (3 under
        precompute-only), 32 zero bytes otherwise."""
        if log_k:
            if not 1 <= log_k <= 255:
                raise ValueError("log_k is 1 .. 255")
            if fmt & (self.TXFORMAT_RETURN_LOG | (255 << self.TXFORMAT_LOG_SHIFT)):
                raise ValueError("log_k beside a format that already carries TXFORMAT_RETURN_LOG or a window")
            fmt |= self.TXFORMAT_RETURN_LOG | (log_k << self.TXFORMAT_LOG_SHIFT)
        self._check(self.lib.zkgpu_verifier_set_tx_format(self.h, fmt))
        self._tx_return_ids = bool(fmt & self.TXFORMAT_RETURN_IDS)
        self._tx_log_k = (fmt >> self.TXFORMAT_LOG_SHIFT) & 255 if fmt & self.TXFORMAT_RETURN_LOG else 0
        self._tx_precompute = bool(fmt & self.TXFORMAT_PRECOMPUTE_ONLY)
        self._tx_root = bool(fmt & self.TXFORMAT_RETURN_ROOT) and self._tx_return_ids
        self._tx_word = fmt

    _tx_root = False                       # the format carries TXFORMAT_RETURN_ROOT: 32 more bytes behind a call's status array
    _tx_return_ids = False
    _tx_log_k = 0
    _tx_precompute = False
    _tx_word = 0                           # the word set_tx_format was given last (verify_statements puts it back)

    class _TxLayout(NamedTuple):
        """the layout of a call's status array -- status[batch] | id[batch][32] | record[batch][1 + 33 K] -- as a value: what a
        call reads when it is made or submitted.  _tx_status_bytes and _tx_result below are the one statement of it here
        (the library's is csrc/tx_out.hpp)"""
        has_ids: bool = False
        log_k: int = 0

    @property
    def _tx_layout(self) -> "_TxLayout":
        return self._TxLayout(self._tx_return_ids, self._tx_log_k)

    @staticmethod
    def _tx_status_bytes(batch: int, has_ids: bool, log_k: int, has_root: bool = False) -> int:
        """bytes the library writes into a call's status array under that layout (has_root: and the 32 bytes of the root behind)"""
        return ((33 if has_ids else 1) + (1 + 33 * log_k if has_ids and log_k else 0)) * batch + (32 if has_ids and has_root else 0)

    def _tx_root_of(self, st, batch: int, log_k: int, has_root: bool) -> bytes:
        """the last 32 bytes of a call's status array under a layout with the root"""
        if not has_root:
            raise ValueError("root=True needs a format with TXFORMAT_RETURN_ROOT (set_tx_format)")
        at = self._tx_status_bytes(batch, True, log_k)
        return st.raw[at: at + 32]

    def _tx_result(self, bm, st, batch: int, has_ids: bool, ids: bool, log_k: int = 0, log: bool = False, beside: int = 0):
        """(bitmap, status bytes) of a transaction call, and with ids=True the call's ID area: 32 bytes per transaction, the ID
        beside status 0 and zeros everywhere else; with log=True both, and the call's log records as a fourth element: per
        transaction None (not accepted), a list of ("input" | "output", id) in log order, or -- accepted with more entries
        than the window holds -- their number as an int.  beside: the status byte a record stands beside (TXSTATUS_ACCEPTED; a
        precompute-only call: TXSTATUS_PRECOMPUTED)"""
        raw = st.raw
        out = (bm.raw[: (batch + 7) // 8], raw[:batch])
        if not (ids or log):
            return out
        if not has_ids:
            raise ValueError("ids=True needs a format with TXFORMAT_RETURN_IDS (set_tx_format)")
        area = raw[batch: 33 * batch]
        out += ([area[32 * i: 32 * i + 32] for i in range(batch)],)
        if not log:
            return out
        if not log_k:
            raise ValueError("log=True needs a format with TXFORMAT_RETURN_LOG (set_tx_format)")
        per, names, logs = 1 + 33 * log_k, {self.TXLOG_INPUT: "input", self.TXLOG_OUTPUT: "output"}, []
        for i in range(batch):
            rec = raw[33 * batch + per * i: 33 * batch + per * (i + 1)]
            if out[1][i] != beside:
                logs.append(None)
            elif rec[0] > log_k or (rec[0] and rec[1] == 0):      # (more than the window holds; 255 saturates: no listed entry has kind 0)
                logs.append(int(rec[0]))
            else:
                logs.append([(names.get(rec[1 + j], rec[1 + j]), rec[1 + log_k + 32 * j: 1 + log_k + 32 * j + 32]) for j in range(rec[0])])
        return out + (logs,)

    def set_tx_chunk(self, transactions: int) -> None:
        """zkgpu_verifier_set_tx_chunk: transactions per chunk of the staged pipeline inside verify_txs (0 = automatic)"""
        self._check(self.lib.zkgpu_verifier_set_tx_chunk(self.h, transactions))

    def set_tx_statements_kept(self, transactions: int) -> None:
        """zkgpu_verifier_set_tx_statements_kept: how many transactions' VM results (700 B each) the verifier keeps between calls"""
        self._check(self.lib.zkgpu_verifier_set_tx_statements_kept(self.h, transactions))

    def verify_txs(self, txs: Sequence[bytes], host_threads: int = 0, ids: bool = False, log: bool = False, root: bool = False):
        """zkgpu_tx_verify_batch: serialized ZkVM transactions (payment subset) -> (accept bitmap, status bytes:
        0 accepted, 1 rejected, 2 outside the subset).  Inert until set_tx_format names a format.  With
        TXFORMAT_RECOLLECTED_V1_REASONS the bitmap is the same and a rejected transaction reads one of TXSTATUS_TX_INVALID ..
        TXSTATUS_SIGNATURE instead of 1 (the lowest code that applies; 1 for every transaction after an error): tx_errors(status)
        turns the bytes into upstream's error variants.  ids=True (only under a format with TXFORMAT_RETURN_IDS): -> (bitmap,
        status bytes, ids) with ids[i] the transaction ID beside status 0 and 32 zero bytes beside everything else.  log=True
        (only under a format with TXFORMAT_RETURN_LOG): -> (bitmap, status bytes, ids, log) with log[i] None beside everything
        but status 0, else the transaction's Input / Output log entries as a list of ("input" | "output", contract ID) in
        the order the program logged them -- or, when there are more than the window K holds, their number as an int.
        root=True (only under a format with TXFORMAT_RETURN_ROOT): one more element at the end, the 32-byte Merkle root over the
        call's transaction IDs -- zeros unless every transaction of the call was accepted."""
        return self.verify_txs_packed(b"".join(txs), [len(t) for t in txs], host_threads, ids=ids, log=log, root=root)

    def verify_txs_packed(self, blob: bytes, lengths, host_threads: int = 0, ids: bool = False, log: bool = False, root: bool = False):
        """the same over one buffer of concatenated transactions and their lengths (same status bytes, reasons included)"""
        batch = len(lengths)
        has_ids, log_k = self._tx_layout
        if self._tx_precompute:
            raise ValueError("the format carries TXFORMAT_PRECOMPUTE_ONLY: nothing would be verified (precompute_txs)")
        if ids and not has_ids:
            raise ValueError("ids=True needs a format with TXFORMAT_RETURN_IDS (set_tx_format)")
        if log and not (has_ids and log_k):
            raise ValueError("log=True needs a format with TXFORMAT_RETURN_LOG (set_tx_format)")
        if root and not self._tx_root:
            raise ValueError("root=True needs a format with TXFORMAT_RETURN_ROOT (set_tx_format)")
        bm, st = self._tx_call(blob, lengths, host_threads)
        out = self._tx_result(bm, st, batch, has_ids, ids, log_k, log)
        return out + (self._tx_root_of(st, batch, log_k, self._tx_root),) if root else out

    def _tx_call(self, blob: bytes, lengths, host_threads: int):
        """zkgpu_tx_verify_batch under the layout in force -> (bitmap buffer, status buffer)"""
        batch = len(lengths)
        has_ids, log_k = self._tx_layout
        offs = np.zeros(batch + 1, dtype=np.uint64)
        np.cumsum(lengths if isinstance(lengths, np.ndarray) and lengths.dtype == np.uint64 else np.asarray(lengths, dtype=np.uint64), out=offs[1:])
        if int(offs[-1]) != len(blob):
            raise ValueError("the lengths add up to %d bytes, the buffer holds %d" % (int(offs[-1]), len(blob)))
        bm = C.create_string_buffer(max((batch + 7) // 8, 1))
        st = C.create_string_buffer(max(self._tx_status_bytes(batch, has_ids, log_k, self._tx_root), 1))      # (with the flags the library writes more than a byte per transaction)
        self._check(self.lib.zkgpu_tx_verify_batch(self.h, batch, blob, offs.ctypes.data_as(C.POINTER(C.c_uint64)), host_threads, bm, st))
        return bm, st

    def _precomputed(self, bm, st, batch: int, log_k: int):
        if any(bm.raw[: (batch + 7) // 8]):
            raise ZkGpuError("a precompute-only call set an accept bit")
        out = self._tx_result(bm, st, batch, True, True, log_k, bool(log_k), beside=self.TXSTATUS_PRECOMPUTED)
        return out[1], out[2], (out[3] if log_k else None)

    def precompute_txs(self, txs: Sequence[bytes], host_threads: int = 0, root: bool = False):
        """upstream's Tx::precompute over serialized transactions, under a format with TXFORMAT_PRECOMPUTE_ONLY: the VM runs, NOTHING
        is verified.  -> (status bytes, ids, logs).  status[i] is TXSTATUS_PRECOMPUTED (3) where the VM ran to the end -- beside
        it ids[i] is the transaction ID and, under TXFORMAT_RETURN_LOG, logs[i] the Input / Output entries as verify_txs lists
        them (or their number, when the window is too small) --, 2 outside the subset, otherwise what the host VM alone finds
        (1, or 16 / 21 with reasons), with ids[i] 32 zero bytes and logs[i] None.  logs is None without TXFORMAT_RETURN_LOG.
        A 3 is NOT a verdict: signature, keys, proof and commitments were not looked at -- never treat it as accepted.
        root=True (only under a format with TXFORMAT_RETURN_ROOT): -> (status bytes, ids, logs, root), the root over the IDs if
        every transaction reads 3, else 32 zero bytes."""
        if not (self._tx_precompute and self._tx_return_ids):
            raise ValueError("precompute_txs needs a format with TXFORMAT_PRECOMPUTE_ONLY (set_tx_format)")
        if root and not self._tx_root:
            raise ValueError("root=True needs a format with TXFORMAT_RETURN_ROOT (set_tx_format)")
        bm, st = self._tx_call(b"".join(txs), [len(t) for t in txs], host_threads)
        out = self._precomputed(bm, st, len(txs), self._tx_log_k)
        return out + (self._tx_root_of(st, len(txs), self._tx_log_k, self._tx_root),) if root else out

    def wait_precomputed(self, call_id: int, root: bool = False):
        """zkgpu_tx_verify_wait for a call submitted under a format with TXFORMAT_PRECOMPUTE_ONLY -> (status bytes, ids, logs) as
        precompute_txs (root=True: and the root, if the call was submitted under a format with TXFORMAT_RETURN_ROOT)"""
        queued = self.__dict__["_tx_calls"][call_id]
        if not (len(queued) > 5 and queued[5]):
            raise ValueError("the call was not submitted under a format with TXFORMAT_PRECOMPUTE_ONLY")
        batch, log_k, has_root = queued[2], queued[4], len(queued) > 6 and queued[6]
        if root and not has_root:
            raise ValueError("root=True: the call was not submitted under a format with TXFORMAT_RETURN_ROOT")
        bm = C.create_string_buffer(max((batch + 7) // 8, 1))
        st = C.create_string_buffer(max(self._tx_status_bytes(batch, True, log_k, has_root), 1))
        try:
            self._check(self.lib.zkgpu_tx_verify_wait(self.h, call_id, bm, st))
        finally:
            del self.__dict__["_tx_calls"][call_id]
        out = self._precomputed(bm, st, batch, log_k)
        return out + (self._tx_root_of(st, batch, log_k, has_root),) if root else out

    def submit_txs_packed(self, blob: bytes, lengths, host_threads: int = 0) -> int:
        """zkgpu_tx_verify_submit: the call is queued (calls in flight are merged into rounds); -> call id for wait_txs.  The
        buffers are kept alive here until the call has been waited for."""
        batch = len(lengths)
        offs = np.zeros(batch + 1, dtype=np.uint64)
        np.cumsum(lengths if isinstance(lengths, np.ndarray) and lengths.dtype == np.uint64 else np.asarray(lengths, dtype=np.uint64), out=offs[1:])
        if int(offs[-1]) != len(blob):
            raise ValueError("the lengths add up to %d bytes, the buffer holds %d" % (int(offs[-1]), len(blob)))
        cid = C.c_uint64(0)
        self._check(self.lib.zkgpu_tx_verify_submit(self.h, batch, blob, offs.ctypes.data_as(C.POINTER(C.c_uint64)), host_threads, C.byref(cid)))
        # (the layout of the call's status array is the one in force when it was queued: remembered with the call)
        self.__dict__.setdefault("_tx_calls", {})[int(cid.value)] = (blob, offs, batch) + self._tx_layout + (self._tx_precompute, self._tx_root)
        return int(cid.value)

    def submit_txs(self, txs: Sequence[bytes], host_threads: int = 0) -> int:
        return self.submit_txs_packed(b"".join(txs), [len(t) for t in txs], host_threads)

    def wait_txs(self, call_id: int, ids: bool = False, log: bool = False, root: bool = False):
        """zkgpu_tx_verify_wait -> (accept bitmap, status bytes) of that call; the status bytes are those verify_txs gives for
        the same transactions -- with TXFORMAT_RECOLLECTED_V1_REASONS the same reason codes, whatever round the call was merged into.
        ids=True (the call was submitted under a format with TXFORMAT_RETURN_IDS): -> (bitmap, status bytes, ids) as verify_txs;
        log=True (... with TXFORMAT_RETURN_LOG): -> (bitmap, status bytes, ids, log) as verify_txs; root=True (... with
        TXFORMAT_RETURN_ROOT): one more element at the end, the root over THIS call's IDs, as verify_txs"""
        queued = self.__dict__["_tx_calls"][call_id]
        batch, (has_ids, log_k) = queued[2], self._TxLayout(*queued[3:5])
        has_root = len(queued) > 6 and queued[6]
        if root and not has_root:
            raise ValueError("root=True: the call was not submitted under a format with TXFORMAT_RETURN_ROOT")
        if len(queued) > 5 and queued[5]:
            raise ValueError("the call was submitted under TXFORMAT_PRECOMPUTE_ONLY: nothing was verified (wait_precomputed)")
        if ids and not has_ids:
            raise ValueError("ids=True: the call was not submitted under a format with TXFORMAT_RETURN_IDS")
        if log and not (has_ids and log_k):
            raise ValueError("log=True: the call was not submitted under a format with TXFORMAT_RETURN_LOG")
        bm = C.create_string_buffer(max((batch + 7) // 8, 1))
        st = C.create_string_buffer(max(self._tx_status_bytes(batch, has_ids, log_k, has_root), 1))
        try:
            self._check(self.lib.zkgpu_tx_verify_wait(self.h, call_id, bm, st))
        finally:
            del self.__dict__["_tx_calls"][call_id]
        out = self._tx_result(bm, st, batch, has_ids, ids, log_k, log)
        return out + (self._tx_root_of(st, batch, log_k, has_root),) if root else out

    @staticmethod
    def _statement_records(records) -> list:
        """the record list of a statements call, refused here when it cannot be one: the library would read a str's or an int's
        bytes as a record and answer 16, which hides a caller's mistake"""
        if isinstance(records, (bytes, bytearray, memoryview, str)) or not hasattr(records, "__iter__"):
            raise TypeError("records: a sequence of bytes objects (zkvm_amd.pack_statement), one per transaction")
        out = []
        for i, r in enumerate(records):
            if not isinstance(r, (bytes, bytearray, memoryview)):
                raise TypeError("records[%d] is %s, not bytes (zkvm_amd.pack_statement)" % (i, type(r).__name__))
            out.append(bytes(r))
        if len(out) >= 1 << 31:
            raise ValueError("too many records for one call")
        return out

    def _statements_format(self, on_device: bool) -> None:
        self.set_tx_format(self.TXFORMAT_STATEMENTS_V1 | (self.TXFORMAT_SIGN_ON_DEVICE if on_device else 0))

    def verify_statements(self, records: Sequence[bytes], host_threads: int = 0, on_device: bool = False):
        """upstream's PrecomputedTx::verify behind the CALLER'S OWN VM: records of what that VM left (zkvm_amd.pack_statement) ->
        (accept bitmap, status bytes).  Sets the format to TXFORMAT_STATEMENTS_V1 -- with on_device=True beside
        TXFORMAT_SIGN_ON_DEVICE: the MuSig coefficients and the challenge are then formed on the device, same verdicts --, makes
        one zkgpu_tx_verify_batch call and PUTS BACK the format set_tx_format was given last, whichever way the call ends: a
        verify_txs afterwards reads transactions under the format it was set up with, never as records.  (The format is the
        verifier's: not to be raced with another thread's calls on the same BlockVerifier.)  bit = every key decodes and s B = R + c X and the cloak proof verifies; the status bytes
        are always reason codes (tx_errors): 0, 16 (record malformed), 17 .. 19 (proof), 20 (key), 21 (signature), 2 (more keys
        or values than the library serves: the caller's own verifier must).  The library cannot know whether a record's txid
        belongs to anything: it is the message the signature is checked over."""
        recs = self._statement_records(records)
        before = self._tx_word
        self._statements_format(on_device)
        try:
            bm, st = self._tx_call(b"".join(recs), [len(r) for r in recs], host_threads)
            return self._tx_result(bm, st, len(recs), False, False)
        finally:
            self.set_tx_format(before)

    def submit_statements(self, records: Sequence[bytes], host_threads: int = 0, on_device: bool = False) -> int:
        """the same through zkgpu_tx_verify_submit -> call id for wait_statements.  The call keeps the format it was queued under,
        whatever is set afterwards, and its round holds no transaction call and no statements call of the other mode.  The format
        set_tx_format was given last is put back before this returns."""
        recs = self._statement_records(records)
        before = self._tx_word
        self._statements_format(on_device)
        try:
            return self.submit_txs_packed(b"".join(recs), [len(r) for r in recs], host_threads)
        finally:
            self.set_tx_format(before)

    def wait_statements(self, call_id: int):
        """zkgpu_tx_verify_wait for a call made by submit_statements -> (accept bitmap, status bytes) as verify_statements"""
        return self.wait_txs(call_id)

    def tx_stats(self):
        """zkgpu_tx_verify_stats -> (rounds the engine has run, calls they held in all)"""
        out = (C.c_uint64 * 2)()
        self._check(self.lib.zkgpu_tx_verify_stats(self.h, out))
        return int(out[0]), int(out[1])

    def verify_sharded(self, comm, txs: Sequence[CloakTx], r_bytes: Optional[bytes] = None) -> bytes:
        """zkgpu_verifier_verify_sharded: every rank passes the whole block and receives the whole bitmap."""
        batch = len(txs)
        n_in, n_out, com, proofs, po = _marshal_block(txs, r_bytes)
        bm = C.create_string_buffer(max((batch + 7) // 8, 1))
        self._check(self.lib.zkgpu_verifier_verify_sharded(self.h, comm.h, batch, n_in, n_out, com, proofs, po, r_bytes, bm))
        return bm.raw[: (batch + 7) // 8]

    def close(self) -> None:
        if self.h:
            self.lib.zkgpu_verifier_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class R1csProver:
    """zkgpu_r1cs_prove_batch: proofs of a described constraint system (BASELINE.json configs[4])."""

    def __init__(self, ctx: Context, bp_gens: BulletproofGens, desc, mult_def: Optional[Sequence[int]] = None, host_threads: int = 0):
        self.ctx, self.bp_gens, self.desc, self.host_threads = ctx, bp_gens, desc, host_threads
        self.mult_def = (C.c_uint32 * max(len(mult_def), 1))(*mult_def) if mult_def is not None else None

    def prove(self, values: Sequence[Sequence[int]], given: Sequence[Sequence[tuple]], seeds: Optional[Sequence[bytes]] = None,
              blindings: Optional[Sequence[Sequence[int]]] = None):
        """values: per statement the m committed scalars; given: per statement the (left, right) assignments of the
        multipliers not defined by constraints; seeds: None -- the library draws the call's randomness itself (the batch is
        then len(values)) -- or one 32-byte seed per statement, never used for two statements; blindings: per statement the
        m blinding factors, or None to derive them.  -> (commitments per statement, proofs per statement)"""
        batch, m = len(values) if seeds is None else len(seeds), self.desc.m
        assert blindings is None or len(blindings) == batch
        n_given = len(given[0]) if batch else 0
        L = self.desc.L
        vb = b"".join(int(x % L).to_bytes(32, "little") for row in values for x in row)
        gb = b"".join(int(a % L).to_bytes(32, "little") + int(b % L).to_bytes(32, "little") for row in given for a, b in row)
        bb = None if blindings is None else b"".join(int(x % L).to_bytes(32, "little") for row in blindings for x in row)
        com = C.create_string_buffer(max(32 * m * batch, 1))
        stride = 1 + 32 * (16 + 2 * 16)
        proofs = C.create_string_buffer(max(stride * batch, 1))
        plen = C.c_size_t(0)
        import time
        sd = None if seeds is None else b"".join(seeds)
        t0 = time.perf_counter()
        rc = self.ctx.lib.zkgpu_r1cs_prove_batch(
            self.ctx.h, self.bp_gens.points.h, C.byref(self.desc.struct), self.mult_def, self.bp_gens.gens_capacity, batch, vb, bb,
            gb, n_given, sd, self.host_threads, com, proofs, stride, C.byref(plen))
        self.last_call_s = time.perf_counter() - t0          # the library call alone (bench.py)
        self.ctx._check(rc)
        return ([com.raw[32 * m * i: 32 * m * (i + 1)] for i in range(batch)],
                [proofs.raw[stride * i: stride * i + plen.value] for i in range(batch)])


class R1csVerifier:
    """Any constraint system, described as data (zkgpu_r1cs_plan_create): the device-side verifier for statements that
    are not a pure cloak -- `r1cs::Verifier::verify` for a uniform batch of proofs of ONE described statement shape."""

    def __init__(self, ctx: Context, bp_gens: BulletproofGens, desc):
        self.ctx, self.bp_gens, self.desc = ctx, bp_gens, desc
        self.h = C.c_void_p()
        ctx._check(ctx.lib.zkgpu_r1cs_plan_create(ctx.h, C.byref(desc.struct), bp_gens.gens_capacity, C.byref(self.h)))

    def info(self) -> dict:
        vals = [C.c_uint32() for _ in range(5)]
        self.ctx._check(self.ctx.lib.zkgpu_cloak_plan_info(self.h, *[C.byref(v) for v in vals]))
        out = dict(zip(("multipliers", "padded_n", "constraints", "terms", "proof_len"), [v.value for v in vals]))
        lay = (C.c_uint32 * 8)()
        self.ctx._check(self.ctx.lib.zkgpu_cloak_plan_layout(self.h, lay))
        out.update(zip(("slots", "n_ch", "n_chal2", "n_dyn", "n_static", "k", "m", "n_mono"), list(lay)))
        return out

    def verify_gpu(self, batch: int, commitments: bytes, proofs: bytes, proof_len: int, r_bytes: Optional[bytes] = None) -> bytes:
        """zkgpu_r1cs_verify_batch_gpu: transcript replay, scalars and the multiscalar multiplications on the device."""
        if len(commitments) != batch * 32 * self.desc.m or len(proofs) != batch * proof_len or (r_bytes is not None and len(r_bytes) != 64 * batch):
            raise ValueError("commitments: 32 bytes per commitment and statement; proofs: proof_len bytes per statement; r: 64 per statement")
        bm = C.create_string_buffer(max((batch + 7) // 8, 1))
        self.ctx._check(self.ctx.lib.zkgpu_r1cs_verify_batch_gpu(self.ctx.h, self.bp_gens.points.h, self.h, batch, commitments, proofs,
                                                                 proof_len, r_bytes, bm))
        return bm.raw[: (batch + 7) // 8]

    def verify_host_prepared(self, batch: int, commitments: bytes, proofs: bytes, proof_len: int, r_bytes: Optional[bytes] = None,
                             host_threads: int = 0) -> bytes:
        """zkgpu_r1cs_verify_batch: the verifier head on host threads, the multiscalar multiplications on the device."""
        if len(commitments) != batch * 32 * self.desc.m or len(proofs) != batch * proof_len or (r_bytes is not None and len(r_bytes) != 64 * batch):
            raise ValueError("commitments: 32 bytes per commitment and statement; proofs: proof_len bytes per statement; r: 64 per statement")
        bm = C.create_string_buffer(max((batch + 7) // 8, 1))
        self.ctx._check(self.ctx.lib.zkgpu_r1cs_verify_batch(self.ctx.h, self.bp_gens.points.h, C.byref(self.desc.struct),
                                                             self.bp_gens.gens_capacity, batch, commitments, proofs, proof_len, r_bytes, bm,
                                                             host_threads))
        return bm.raw[: (batch + 7) // 8]

    def close(self) -> None:
        if self.h:
            self.ctx.lib.zkgpu_r1cs_plan_destroy(self.h)
            self.h = C.c_void_p()


class MixedR1csVerifier:
    """zkgpu_r1cs_verify_mixed: statements of DIFFERENT constraint systems in one device call -- upstream's batch
    verification over a list of verifiers, each with its own constraint system.  `plans`: per plan an R1csVerifier (kept
    referenced here, so that its plan outlives this object's calls) or an (n_in, n_out) cloak shape (the plan is made here
    and owned by this object); statement i is checked against plans[plan_index[i]].  Every statement's commitments are
    checked against its plan's m x 32 bytes (the library reads exactly that much)."""

    def __init__(self, ctx: Context, bp_gens: BulletproofGens, plans):
        self.ctx, self.bp_gens = ctx, bp_gens
        self._owned, self._verifiers = [], []
        handles, self.m = [], []
        for p in plans:
            if isinstance(p, R1csVerifier):
                if not p.h:
                    raise ValueError("R1csVerifier already closed")
                self._verifiers.append(p)
                handles.append(p.h.value)
                self.m.append(p.desc.m)
            elif isinstance(p, tuple) and len(p) == 2:
                h = C.c_void_p()
                ctx._check(ctx.lib.zkgpu_cloak_plan_create(ctx.h, p[0], p[1], bp_gens.gens_capacity, C.byref(h)))
                self._owned.append(h)
                handles.append(h.value)
                self.m.append(2 * (p[0] + p[1]))                  # (quantity, flavor) per value
            else:
                raise TypeError("a plan is an R1csVerifier or an (n_in, n_out) cloak shape")
        self.n_plans = len(handles)
        self.handles = handles                                    # (what zkgpu_r1cs_verify_batch_gpu would take per plan)
        self._plans = (C.c_void_p * max(self.n_plans, 1))(*handles)

    def _args(self, plan_index: Sequence[int], commitments: Sequence[bytes], proofs: Sequence[bytes], r_bytes: Optional[bytes]):
        if any(v.h.value is None for v in self._verifiers) or self._plans is None:
            raise ValueError("a plan of this verifier has been closed")
        batch = len(plan_index)
        if len(commitments) != batch or len(proofs) != batch or (r_bytes is not None and len(r_bytes) != 64 * batch):
            raise ValueError("one commitment string and one proof per statement; r: 64 bytes per statement")
        for i, (p, c) in enumerate(zip(plan_index, commitments)):
            if not 0 <= p < self.n_plans:
                raise ValueError("statement %d: plan index %d out of range (%d plans)" % (i, p, self.n_plans))
            if len(c) != 32 * self.m[p]:
                raise ValueError("statement %d: %d bytes of commitments, its plan takes %d (32 per commitment)" % (i, len(c), 32 * self.m[p]))
        offs = [0]
        for p in proofs:
            offs.append(offs[-1] + len(p))
        return (batch, (C.c_uint32 * max(batch, 1))(*plan_index), b"".join(commitments), b"".join(proofs),
                (C.c_uint64 * (batch + 1))(*offs), r_bytes)

    def verify(self, plan_index: Sequence[int], commitments: Sequence[bytes], proofs: Sequence[bytes],
               r_bytes: Optional[bytes] = None) -> bytes:
        """-> the accept bitmap, in the order of the statements given"""
        batch, idx, com, pr, offs, r = self._args(plan_index, commitments, proofs, r_bytes)
        bm = C.create_string_buffer(max((batch + 7) // 8, 1))
        self.ctx._check(self.ctx.lib.zkgpu_r1cs_verify_mixed(self.ctx.h, self.bp_gens.points.h, self._plans, self.n_plans, batch,
                                                             idx, com, pr, offs, r, bm))
        return bm.raw[: (batch + 7) // 8]

    def submit(self, plan_index: Sequence[int], commitments: Sequence[bytes], proofs: Sequence[bytes],
               r_bytes: Optional[bytes] = None) -> None:
        """zkgpu_r1cs_verify_mixed_submit: queued, the inputs free again on return; `wait` collects the bitmap"""
        batch, idx, com, pr, offs, r = self._args(plan_index, commitments, proofs, r_bytes)
        self.ctx._check(self.ctx.lib.zkgpu_r1cs_verify_mixed_submit(self.ctx.h, self.bp_gens.points.h, self._plans, self.n_plans,
                                                                    batch, idx, com, pr, offs, r))
        self.ctx._pending_batch = batch

    def wait(self) -> bytes:
        return self.ctx.verify_wait()

    def close(self) -> None:
        for h in self._owned:
            self.ctx.lib.zkgpu_cloak_plan_destroy(h)
        self._owned, self._verifiers, self._plans = [], [], None


class Verifier:
    """Batch verifier; `verify_cloak_txs` returns one Optional[VMError] per transaction
    (None = Ok), the shape of `txs.iter().map(|tx| tx.verify(bp_gens))`."""

    def __init__(self, ctx: Context, bp_gens: BulletproofGens, host_threads: int = 0):
        self.ctx = ctx
        self.bp_gens = bp_gens
        self.host_threads = host_threads

    def verify_bitmap(self, txs: Sequence[CloakTx], r_bytes: Optional[bytes] = None) -> bytes:
        batch = len(txs)
        n_in = (C.c_uint32 * max(batch, 1))(*[t.n_in for t in txs])
        n_out = (C.c_uint32 * max(batch, 1))(*[t.n_out for t in txs])
        offs = [0]
        for t in txs:
            if len(t.commitments) != 64 * (t.n_in + t.n_out):
                raise ValueError("commitments must hold 64 bytes per value")
            offs.append(offs[-1] + len(t.proof))
        po = (C.c_uint64 * (batch + 1))(*offs)
        bm = C.create_string_buffer(max((batch + 7) // 8, 1))
        if r_bytes is not None and len(r_bytes) != 64 * batch:
            raise ValueError("r_bytes must hold 64 bytes per transaction")
        rc = self.ctx.lib.zkgpu_cloak_verify_batch(
            self.ctx.h, self.bp_gens.points.h, self.bp_gens.gens_capacity, batch, n_in, n_out,
            b"".join(t.commitments for t in txs), b"".join(t.proof for t in txs), po, r_bytes, bm, self.host_threads)
        self.ctx._check(rc)
        return bm.raw[: (batch + 7) // 8]

    # ---- host half on the device (plan replay) ---------------------------------------------
    def _plan(self, n_in: int, n_out: int):
        plans = self.__dict__.setdefault("_plans", {})
        key = (n_in, n_out)
        if key not in plans:
            h = C.c_void_p()
            self.ctx._check(self.ctx.lib.zkgpu_cloak_plan_create(self.ctx.h, n_in, n_out, self.bp_gens.gens_capacity,
                                                                 C.byref(h)))
            plans[key] = h
        return plans[key]

    def plan_info(self, n_in: int, n_out: int) -> dict:
        vals = [C.c_uint32() for _ in range(5)]
        self.ctx._check(self.ctx.lib.zkgpu_cloak_plan_info(self._plan(n_in, n_out), *[C.byref(v) for v in vals]))
        return dict(zip(("multipliers", "padded_n", "constraints", "terms", "proof_len"), [v.value for v in vals]))

    def _block_verifier(self) -> "BlockVerifier":
        bv = self.__dict__.get("_bv")
        if bv is None:
            bv = self.__dict__["_bv"] = BlockVerifier(self.ctx, self.bp_gens)
        return bv

    def verify_bitmap_gpu(self, txs: Sequence[CloakTx], r_bytes: Optional[bytes] = None) -> bytes:
        """As verify_bitmap, with the transcript replay and the scalar preparation on the GPU
        (zkgpu_verifier_verify: shape grouping, one device plan per shape and the batches in flight all live
        behind the C ABI).  A transaction whose shape cannot be verified over these generators, or whose
        proof length does not fit its shape, is rejected on its own, as in the reference."""
        return self._block_verifier().verify(txs, r_bytes)

    def plan_layout(self, n_in: int, n_out: int) -> dict:
        """zkgpu_cloak_plan_layout: sizes of the buffers zkgpu_debug_read returns for this shape."""
        out = (C.c_uint32 * 8)()
        self.ctx._check(self.ctx.lib.zkgpu_cloak_plan_layout(self._plan(n_in, n_out), out))
        return dict(zip(("slots", "n_ch", "n_chal2", "n_dyn", "n_static", "k", "m", "n_mono"), list(out)))

    def verify_packed_gpu(self, n_in: int, n_out: int, batch: int, commitments: bytes, proofs: bytes, proof_len: int,
                          r_bytes: Optional[bytes] = None) -> bytes:
        """zkgpu_cloak_verify_batch_gpu on already-contiguous buffers (what a Rust caller would hand over)."""
        _check_packed(n_in, n_out, batch, commitments, proofs, proof_len, r_bytes)
        bm = C.create_string_buffer(max((batch + 7) // 8, 1))
        rc = self.ctx.lib.zkgpu_cloak_verify_batch_gpu(self.ctx.h, self.bp_gens.points.h, self._plan(n_in, n_out), batch,
                                                       commitments, proofs, proof_len, r_bytes, bm)
        self.ctx._check(rc)
        return bm.raw[: (batch + 7) // 8]

    def verify_packed_gpu_dev(self, n_in: int, n_out: int, batch: int, d_commitments, d_proofs, proof_len: int,
                              d_r=None) -> bytes:
        """zkgpu_cloak_verify_batch_gpu_dev: inputs are device buffers (torch tensors or raw pointers).  d_r None
        (recommended): the library draws the verifier randomness itself, on the device."""
        from .native import _ptr
        bm = C.create_string_buffer(max((batch + 7) // 8, 1))
        rc = self.ctx.lib.zkgpu_cloak_verify_batch_gpu_dev(self.ctx.h, self.bp_gens.points.h, self._plan(n_in, n_out),
                                                           batch, _ptr(d_commitments), _ptr(d_proofs), proof_len,
                                                           _ptr(d_r), bm)
        self.ctx._check(rc)
        return bm.raw[: (batch + 7) // 8]

    def submit_packed_gpu_dev(self, n_in: int, n_out: int, batch: int, d_commitments, d_proofs, proof_len: int, d_r=None,
                              ctx: Optional[Context] = None) -> Context:
        """zkgpu_cloak_verify_submit_dev on `ctx` (this verifier's context or one of its forks): returns once the
        batch is queued; `ctx.verify_wait()` yields the accept bitmap.  d_r None: drawn by the library."""
        from .native import _ptr
        c = ctx or self.ctx
        c._check(c.lib.zkgpu_cloak_verify_submit_dev(c.h, self.bp_gens.points.h, self._plan(n_in, n_out), batch,
                                                     _ptr(d_commitments), _ptr(d_proofs), proof_len, _ptr(d_r)))
        c._pending_batch = batch
        return c

    def submit_packed_gpu(self, n_in: int, n_out: int, batch: int, commitments: bytes, proofs: bytes, proof_len: int,
                          r_bytes: Optional[bytes] = None, ctx: Optional[Context] = None) -> Context:
        """zkgpu_cloak_verify_submit: as submit_packed_gpu_dev with the inputs in host memory."""
        _check_packed(n_in, n_out, batch, commitments, proofs, proof_len, r_bytes)
        c = ctx or self.ctx
        c._check(c.lib.zkgpu_cloak_verify_submit(c.h, self.bp_gens.points.h, self._plan(n_in, n_out), batch,
                                                 commitments, proofs, proof_len, r_bytes))
        c._pending_batch = batch
        return c

    def close(self) -> None:
        bv = self.__dict__.pop("_bv", None)
        if bv is not None:
            bv.close()
        for h in self.__dict__.get("_plans", {}).values():
            self.ctx.lib.zkgpu_cloak_plan_destroy(h)
        self.__dict__["_plans"] = {}

    def prepare(self, txs: Sequence[CloakTx], r_bytes: Optional[bytes] = None):
        """Host half only: proof bytes -> MSM terms (CSR) for Context.verify_batch_ps*.
        -> dict(dyn_sc, dyn_pt, dyn_off, st_sc, st_idx, st_off, wellformed)"""
        batch = len(txs)
        n_in = (C.c_uint32 * max(batch, 1))(*[t.n_in for t in txs])
        n_out = (C.c_uint32 * max(batch, 1))(*[t.n_out for t in txs])
        offs = [0]
        dyn_cap = st_cap = 0
        for t in txs:
            offs.append(offs[-1] + len(t.proof))
            k = max(0, ((len(t.proof) - 1) // 32 - 16) // 2)
            dyn_cap += 11 + 2 * (t.n_in + t.n_out) + 2 * k
            st_cap += 2 + 2 * (1 << min(k, 20))
        po = (C.c_uint64 * (batch + 1))(*offs)
        ds, dp = C.create_string_buffer(max(32 * dyn_cap, 1)), C.create_string_buffer(max(32 * dyn_cap, 1))
        ss, si = C.create_string_buffer(max(32 * st_cap, 1)), (C.c_uint32 * max(st_cap, 1))()
        do, so = (C.c_uint64 * (batch + 1))(), (C.c_uint64 * (batch + 1))()
        wf = C.create_string_buffer(max(batch, 1))
        rc = self.ctx.lib.zkgpu_cloak_prepare_batch(
            self.bp_gens.gens_capacity, batch, n_in, n_out, b"".join(t.commitments for t in txs),
            b"".join(t.proof for t in txs), po, r_bytes, self.host_threads, ds, dp, do, dyn_cap, ss, si, so, st_cap, wf)
        self.ctx._check(rc)
        nd, ns = do[batch], so[batch]
        return {"dyn_sc": ds.raw[: 32 * nd], "dyn_pt": dp.raw[: 32 * nd], "dyn_off": list(do),
                "st_sc": ss.raw[: 32 * ns], "st_idx": list(si[:ns]), "st_off": list(so), "wellformed": wf.raw[:batch]}

    def verify_cloak_txs(self, txs: Sequence[CloakTx], r_bytes: Optional[bytes] = None) -> List[Optional[VMError]]:
        try:
            bm = self.verify_bitmap(txs, r_bytes)
        except ZkGpuError as e:   # fail closed: a device error is never an accept
            return [VMError(str(e)) for _ in txs]
        return [None if (bm[i // 8] >> (i % 8)) & 1 else InvalidR1CSProof("R1CS proof did not verify")
                for i in range(len(txs))]
