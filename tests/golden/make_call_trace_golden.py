#!/usr/bin/env python3
"""The libtrx call trace of every stack of tests/test_call_trace.py, recorded on the kernel-logic emulator (deterministic: two runs give the
same trace).

    python tests/golden/make_call_trace_golden.py            # -> tests/golden/call_trace.json

The fixture pins what the host layer asked of the library at the commit before BatchedRCWA was split into its modes (9d6f213); run it at a
commit whose sequence of library calls is meant to become the new record, never to make a failing test pass.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.test_call_trace import FIXTURE, STACKS, record  # noqa: E402


def main():
    traces = {name: record("emu", name)[0] for name in sorted(STACKS)}
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(f' "{name}": [\n' + ",\n".join("  " + json.dumps(c) for c in calls) + "\n ]" for name, calls in traces.items())
                + "\n}\n")
    print({name: len(calls) for name, calls in traces.items()}, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
