"""The reason codes of the transaction calls (ZKGPU_TXSTATUS_*, ZKGPU_TXFORMAT_RECOLLECTED_V1_REASONS) on the CPU tier: they
are constants of the header, mirrored in the Rust declarations and the Python binding; they came through entry points that
exist (no new export, hook or struct); the Python helper maps every code to upstream's error variant; the manifest of
recollected constants still describes the sources as they are."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = {"ZKGPU_TXFORMAT_RECOLLECTED_V1_REASONS": 2, "ZKGPU_TXSTATUS_ACCEPTED": 0, "ZKGPU_TXSTATUS_REJECTED": 1,
         "ZKGPU_TXSTATUS_OUTSIDE_SUBSET": 2, "ZKGPU_TXSTATUS_TX_INVALID": 16, "ZKGPU_TXSTATUS_PROOF_FORMAT": 17,
         "ZKGPU_TXSTATUS_PROOF_POINT": 18, "ZKGPU_TXSTATUS_PROOF_EQUATION": 19, "ZKGPU_TXSTATUS_KEY": 20, "ZKGPU_TXSTATUS_SIGNATURE": 21}


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_constants_of_the_header_are_mirrored_in_rust_and_python():
    header = dict((n, int(v)) for n, v in re.findall(r"#define\s+(ZKGPU_[A-Z0-9_]+)\s+(-?\d+)\b", _read("include", "zkgpu.h")))
    rust = dict((n, int(v)) for n, v in re.findall(r"pub const (ZKGPU_[A-Z0-9_]+): c_int = (-?\d+);", _read("rust", "zkgpu-sys", "src", "lib.rs")))
    from zkvm_amd import native
    from zkvm_amd.verifier import BlockVerifier
    for name, value in CODES.items():
        assert header.get(name) == value, name
        assert rust.get(name) == value, name
        short = name[len("ZKGPU_"):]
        assert getattr(native, short) == value, short
        assert getattr(BlockVerifier, short) == value, short
    assert header["ZKGPU_TXFORMAT_RECOLLECTED_V1"] == 1 == BlockVerifier.TXFORMAT_RECOLLECTED_V1
    # the safe Rust wrapper names every code it is handed
    wrapper = _read("rust", "zkgpu", "src", "lib.rs")
    for name in CODES:
        assert "sys::" + name in wrapper, name


def test_no_new_export_hook_or_struct():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_capi_symbols import _declared, _hooks_declared
    assert len(_declared()) == 90
    assert len(_hooks_declared()) == 25
    header = re.sub(r"/\*.*?\*/", "", _read("include", "zkgpu.h"), flags=re.S)
    assert re.findall(r"typedef struct (\w+) \{", header) == ["zkgpu_r1cs_desc"]
    assert "return 3;" in re.search(r"int zkgpu_abi_version\(void\)\s*\{[^}]*\}", _read("zkvm_amd", "csrc", "zkgpu.hip")).group(0)


def test_tx_errors_maps_every_code_to_its_error_variant():
    from zkvm_amd.verifier import BlockVerifier as B, InvalidR1CSProof, InvalidSignature, TxFormatError, VMError, tx_errors
    errs = tx_errors(bytes([0, 1, 2, 16, 17, 18, 19, 20, 21, 77]))
    assert errs[0] is None
    kinds = [VMError, VMError, TxFormatError, InvalidR1CSProof, InvalidR1CSProof, InvalidR1CSProof, InvalidSignature, InvalidSignature, VMError]
    assert [type(e) for e in errs[1:]] == kinds
    assert [e.reason for e in errs[1:]] == [1, 2, 16, 17, 18, 19, 20, 21, 77]
    assert all(isinstance(e, VMError) and str(e) for e in errs[1:])
    assert errs[5].reason == B.TXSTATUS_PROOF_POINT and errs[8].reason == B.TXSTATUS_SIGNATURE
    assert InvalidR1CSProof("as before").reason is None          # (the error verify_cloak_txs has always returned)
    assert B.tx_errors(b"\x00\x13")[1].reason == B.TXSTATUS_PROOF_EQUATION and tx_errors(b"") == []


def test_the_manifest_of_recollected_constants_is_not_stale():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "unpinned_manifest.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
