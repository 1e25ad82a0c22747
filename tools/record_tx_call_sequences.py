#!/usr/bin/env python3
"""Records tests/golden/tx_call_sequences.json: what the scenarios of tests/test_tx_call_sequences.py ask of the stand-in device
on the host library that is built in this tree -- per kind of operation its ordered (slot, rows, detail), the planned chunks and
signature stages -- with the commit they were recorded from.  Run it on the commit whose behaviour is to be kept, BEFORE the
scheduler is changed; the test then holds every later commit against the file, which is never regenerated from the code under
test.  Every scenario is run under two delay seeds: a kind whose sequence differs between them is not deterministic, is left
out of that scenario and is named on the way out.

    python tools/record_tx_call_sequences.py [--commit ID] [--out FILE]        (no GPU)"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "tx_call_sequences.json"))
    ap.add_argument("--seeds", default="1,2", help="the two delay seeds")
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    from zkvm_amd.build import HOST_OUT, build
    build()
    host = C.CDLL(HOST_OUT)
    from oracle import binding as oracle
    oracle.build()
    oracle.load()
    from test_tx_call_sequences import KINDS, _inputs, _tx_call_sequences, scenario_name
    inputs = _inputs(oracle)
    first, second = (_tx_call_sequences(host, inputs, int(s)) for s in args.seeds.split(","))
    rec, left_out = {"recorded_from": commit, "scenarios": {}}, []
    for key, a in first.items():
        b, name = second[key], scenario_name(*key)
        assert (a["chunks"], a["sig_stages"]) == (b["chunks"], b["sig_stages"]), name
        same = [k for k in KINDS if a["kinds"][k] == b["kinds"][k]]
        left_out += [(name, k) for k in KINDS if k not in same]
        rec["scenarios"][name] = {"chunks": a["chunks"], "sig_stages": a["sig_stages"], "kinds": {k: a["kinds"][k] for k in same}}
        print("%-34s %2d chunks, %2d signature stages, operations %s" % (name, a["chunks"], a["sig_stages"], [len(a["kinds"][k]) for k in KINDS]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print("left out as not deterministic:", left_out or "nothing")


if __name__ == "__main__":
    main()
