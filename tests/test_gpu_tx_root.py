"""ZKGPU_TXFORMAT_RETURN_ROOT (16) on the device: the Merkle root over a call's transaction IDs behind everything else in the
status array.  With ZKGPU_TXFORMAT_HASH_ON_DEVICE the leaves and the folds run there (csrc/tx_root_kernels.hpp: k_tx_root_leaves,
k_tx_root_fold); without it the host threads fold the host VM's IDs through the same function.

The reference is tests/test_tx_root_host.py's: the recursive RFC 6962 tree over the oracle's Merlin transcript, over the IDs the
call itself returned -- which the ID tests hold against the oracle's VM.

  1. sizes 1, 2, 3, 64, 65, 129 of mixed shapes under 0x502 | 16: the root is the reference's, every other byte the flagless word's;
  2. the same 65 payments under every legal mode: ONE root, the host path and the device path agree;
  3. chunks of 48 (no power of two) with 129 payments;
  4. a fresh process with ZKGPU_TX_ROOT_SPAN=2: four fold launches instead of one, the same root;
  5. one bad transaction (signature; proof): 32 zero bytes, everything else as without the flag; under 0x2000 it HAS a root;
  6. submitted calls of 40, 65 and 1 merged behind a long one: each its own root and its queued layout, whatever the format says
     at the wait.  (The format is the verifier's and setting it waits for a round in flight, so calls that merge on the device
     were all queued under one word; a round that mixes calls with and without the flag is the CPU test's hand-out.);
  7. batch == 0: the empty tree's hash;
  8. fail-closed at every runtime call of one flagged call (the software gate zkgpu_debug_fail_after: nothing faults).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from gpu_util import bits
from test_gpu_tx_reasons import _parts, _put
from test_tx_root_host import reference_root
from tx_root_child import RETURN_ROOT, old_bytes, payments as make_payments, raw_call

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASH, SIGN, IDS, LOG, PRE = 0x100, 0x200, 0x400, 0x800, 0x2000
WINDOW = LOG | (4 << 16)
ZERO = bytes(32)


@pytest.fixture(scope="module")
def ctx():
    from zkvm_amd import Context
    c = Context(0)
    yield c
    c.lib.zkgpu_debug_fail_after(c.h, 0, None)
    c.close()


@pytest.fixture(scope="module")
def gens(ctx):
    from zkvm_amd.verifier import BulletproofGens
    g = BulletproofGens(ctx, 256, table_bits=8)
    yield g
    g.close()


@pytest.fixture(scope="module")
def bv(ctx, gens):
    from zkvm_amd.verifier import BlockVerifier
    v = BlockVerifier(ctx, gens, batches_in_flight=3)
    yield v
    v.close()


@pytest.fixture(scope="module")
def payments(oracle):
    return make_payments(oracle, 129)


@pytest.fixture(scope="module")
def roots(ctx, bv, payments):
    """per size, the reference over the IDs a flagless call returned (computed once, shared)"""
    out = {}
    for n in (1, 2, 3, 40, 64, 65, 129):
        rc, bm, area, _ = raw_call(ctx, bv, 0x502, payments[:n])
        assert rc == 0 and bits(bm, n) == [1] * n and area[:n] == bytes(n)
        out[n] = reference_root([area[n + 32 * i: n + 32 * i + 32] for i in range(n)])
    return out


def sig_byte_flipped(tx):
    at = _parts(tx)[0] + 32
    return _put(tx, at, bytes([tx[at] ^ 1]))


def proof_byte_flipped(tx):
    at = _parts(tx)[1] + 1 + 32 * 11                       # t_x
    return _put(tx, at, bytes([tx[at] ^ 1]))


def test_the_flag_is_accepted_exactly_beside_the_ids(ctx, bv):
    for w in (1, 2, 0x101, 0x302):
        for rest in (0, WINDOW):
            assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, w | IDS | rest | RETURN_ROOT) == 0, hex(w)
            if not w & SIGN:
                assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, w | IDS | rest | PRE | RETURN_ROOT) == 0, hex(w)
        assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, w | RETURN_ROOT) == -1, hex(w)
    for bad in (RETURN_ROOT, RETURN_ROOT | IDS, 4 | RETURN_ROOT, 0x204 | RETURN_ROOT, 4 | IDS | RETURN_ROOT, 0x302 | IDS | PRE | RETURN_ROOT, 3 | IDS | RETURN_ROOT):
        assert ctx.lib.zkgpu_verifier_set_tx_format(bv.h, bad) == -1, hex(bad)
    bv.set_tx_format(0)


@pytest.mark.parametrize("n", (1, 2, 3, 64, 65, 129))
def test_sizes_of_mixed_shapes(ctx, bv, payments, roots, n):
    plain = raw_call(ctx, bv, 0x502, payments[:n])
    got = raw_call(ctx, bv, 0x502 | RETURN_ROOT, payments[:n])
    assert got[:3] == plain[:3] and got[0] == 0
    assert got[3] == roots[n], n
    # through the binding: the root is the last element
    bv.set_tx_format(0x502 | RETURN_ROOT)
    out = bv.verify_txs(payments[:n], host_threads=2, ids=True, root=True)
    assert out[3] == roots[n] and b"".join(out[2]) == plain[2][n:]


def test_one_root_under_every_mode(ctx, bv, payments, roots):
    txs = payments[:65]
    seen = set()
    for base in (1, 2):
        for dev in (0, HASH, HASH | SIGN):
            for rest in (0, WINDOW):
                word = base | dev | IDS | rest
                plain = raw_call(ctx, bv, word, txs)
                got = raw_call(ctx, bv, word | RETURN_ROOT, txs)
                assert got[0] == 0 and got[:3] == plain[:3] and got[3] == roots[65], hex(word)
                seen.add(got[3])
                if dev & SIGN:
                    continue
                plain = raw_call(ctx, bv, word | PRE, txs)
                got = raw_call(ctx, bv, word | PRE | RETURN_ROOT, txs)
                assert got[0] == 0 and got[:3] == plain[:3] and got[2][:65] == bytes([3]) * 65 and got[3] == roots[65], hex(word | PRE)
    assert seen == {roots[65]}


def test_a_chunk_edge_that_is_no_power_of_two(ctx, bv, payments, roots):
    bv.set_tx_chunk(48)
    try:
        for word in (0x502, 0x702, 0x2501):
            plain = raw_call(ctx, bv, word, payments)
            got = raw_call(ctx, bv, word | RETURN_ROOT, payments)
            assert got[0] == 0 and got[:3] == plain[:3] and got[3] == roots[129], hex(word)
    finally:
        bv.set_tx_chunk(0)


def test_several_passes_in_a_fresh_process(roots, tmp_path):
    """tests/tx_root_child.py with ZKGPU_TX_ROOT_SPAN=2: 65 leaves take four passes (65 -> 17 -> 5 -> 2 -> 1); the root is unchanged"""
    out = tmp_path / "span2.json"
    env = dict(os.environ, ZKGPU_TX_ROOT_SPAN="2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tx_root_child.py"), str(out)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    got = json.load(open(out))
    assert got["rc"] == 0 and got["same"] and got["bitmap"] == (bytes([255] * 8) + b"\x01").hex()
    assert bytes.fromhex(got["root"]) == roots[65]
    assert got["launches"] == {"k_tx_root_leaves": 1, "k_tx_root_fold": 4}, got["launches"]


@pytest.mark.parametrize("damage", (sig_byte_flipped, proof_byte_flipped))
def test_one_bad_transaction_leaves_no_root(ctx, bv, payments, roots, damage):
    txs = list(payments[:65])
    txs[37] = damage(txs[37])
    for word in (0x402, 0x502, 0x702):
        plain = raw_call(ctx, bv, word, txs)
        got = raw_call(ctx, bv, word | RETURN_ROOT, txs)
        assert got[0] == 0 and got[:3] == plain[:3], hex(word)
        assert bits(got[1], 65) == [int(i != 37) for i in range(65)] and got[2][37] in (19, 21)
        assert got[3] == ZERO, hex(word)
    # nothing is verified under 0x2000: the same call reads 3 everywhere and HAS a root -- the one of the undamaged IDs, which
    # neither a signature byte nor a proof byte enters
    for word in (0x2402, 0x2502):
        got = raw_call(ctx, bv, word | RETURN_ROOT, txs)
        assert got[0] == 0 and got[2][:65] == bytes([3]) * 65 and got[3] == roots[65], hex(word)


def test_submitted_calls_keep_their_own_root_and_their_queued_layout(ctx, bv, payments, roots):
    word = 0x502 | RETURN_ROOT
    parts = [(0, 40), (0, 65), (0, 1)]
    packed = lambda call: (b"".join(call), [len(t) for t in call], 2)      # noqa: E731
    merged = False
    for attempt in range(3):
        bv.set_tx_format(word)
        rounds0, calls0 = bv.tx_stats()
        blocker = bv.submit_txs_packed(*packed(payments * 8))
        cids = [bv.submit_txs_packed(*packed(payments[lo:hi])) for lo, hi in parts]
        bv.set_tx_format(0x402)                              # (waits for the rounds; the calls keep what they were queued under)
        out = bv.wait_txs(blocker, ids=True, root=True)
        assert out[1] == bytes(129 * 8) and out[3] != ZERO
        for cid, (lo, hi) in zip(cids, parts):
            bm, st, ids, root = bv.wait_txs(cid, ids=True, root=True)
            n = hi - lo
            assert bits(bm, n) == [1] * n and st == bytes(n) and root == roots[n] == reference_root(ids), n
        rounds, calls = bv.tx_stats()
        assert calls - calls0 == 4
        if rounds - rounds0 == 2:                            # (the three short calls left in one round behind the long one)
            merged = True
            break
    assert merged
    # a call queued without the flag has no root area, whatever the format says at the wait
    bv.set_tx_format(0x502)
    cid = bv.submit_txs_packed(*packed(payments[:5]))
    bv.set_tx_format(word)
    with pytest.raises(ValueError):
        bv.wait_txs(cid, ids=True, root=True)
    bv.set_tx_format(0x502)
    cid = C.c_uint64(0)
    blob, lengths, _ = packed(payments[:5])
    offs = (C.c_uint64 * 6)(*([0] + [sum(lengths[:i + 1]) for i in range(5)]))
    assert ctx.lib.zkgpu_tx_verify_submit(bv.h, 5, blob, offs, 2, C.byref(cid)) == 0
    bv.set_tx_format(word)
    bm, st = C.create_string_buffer(1), C.create_string_buffer(b"\xa5" * (33 * 5 + 64), 33 * 5 + 64)
    assert ctx.lib.zkgpu_tx_verify_wait(bv.h, cid.value, bm, st) == 0
    assert st.raw[:5] == bytes(5) and st.raw[33 * 5:] == b"\xa5" * 64


def test_a_call_over_no_transaction_returns_the_empty_root(ctx, bv):
    for word in (0x402, 0x502, 0x702, 0x2502, 0x502 | WINDOW):
        rc, bm, area, root = raw_call(ctx, bv, word | RETURN_ROOT, [])
        assert rc == 0 and area == b"" and root == reference_root([]), hex(word)
    bv.set_tx_format(0x502 | RETURN_ROOT)
    bm = C.create_string_buffer(1)
    assert ctx.lib.zkgpu_tx_verify_batch(bv.h, 0, None, None, 2, bm, None) == 0      # status == NULL stays legal


def test_a_failure_of_any_runtime_call_fails_the_call_closed(ctx, bv, payments, roots):
    """zkgpu_debug_fail_after makes the n-th runtime call of the library answer "failed" on the host (nothing faults on the
    device).  n walks through every runtime call of a warm flagged call of 65: every one of them, failed, ends the call with an
    error, a zero bitmap, status 1 everywhere, no ID and no root; the clean call after it is right"""
    txs, word, n = payments[:65], 0x702 | RETURN_ROOT, 65
    good = raw_call(ctx, bv, word, txs)
    assert good[0] == 0 and good[3] == roots[65] and good == raw_call(ctx, bv, word, txs)      # (warm)
    try:
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 10 ** 9, None)
        assert raw_call(ctx, bv, word, txs) == good
        calls = int(ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None))
        assert 10 <= calls <= 400, calls
        for q in range(1, calls + 1):
            ctx.lib.zkgpu_debug_fail_after(ctx.h, q, None)
            out = raw_call(ctx, bv, word, txs)
            fired = C.c_longlong(-1)
            ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, C.byref(fired))
            assert fired.value == 1, (q, fired.value)
            assert out[0] != 0 and out[1] == bytes((n + 7) // 8) and out[2] == bytes([1]) * n + bytes(32 * n) and out[3] == ZERO, q
            assert raw_call(ctx, bv, word, txs) == good, q                                       # the verifier is usable afterwards
        print("runtime calls of a clean flagged call of 65 payments:", calls)
    finally:
        ctx.lib.zkgpu_debug_fail_after(ctx.h, 0, None)
