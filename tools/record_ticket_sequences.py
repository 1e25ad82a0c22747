#!/usr/bin/env python3
"""Records tests/golden/ticket_sequences.json: what the scenarios of tests/test_gpu_ticket_sequences.py give on the library
that is built in this tree -- verdict bits, every lane's launch sequence, gated runtime calls -- with the commit they were
recorded from.  Run it on the commit whose behaviour is to be kept, BEFORE the ticket engine is changed; the test then holds
every later commit against the file, which is never regenerated from the code under test.

    python tools/record_ticket_sequences.py [--commit ID] [--out FILE]        (needs the GPU)"""
import os as _os; _os.environ.setdefault("ZKGPU_TEST_HOOKS", "1")   # the profile / fault-gate hooks (include/zkgpu_hooks.h) are not exports
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ticket_sequences.json"))
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    from zkvm_amd import Context, runtime_hint
    runtime_hint()                                          # (as tests/conftest.py: before the first HIP call)
    from oracle import binding as oracle
    oracle.load()
    from test_gpu_ticket_sequences import _ticket_sequences
    ctx = Context(0)
    try:
        rec = _ticket_sequences(ctx, oracle)
    finally:
        ctx.close()
    rec = {"recorded_from": commit, "lanes": rec["lanes"], "scenarios": rec["scenarios"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for name, s in rec["scenarios"].items():
        print("%-34s %4d runtime calls, launches per lane %s" % (name, s["runtime_calls"], [sum(n for _, n in lane) for lane in s["lanes"]]))


if __name__ == "__main__":
    main()
