#!/usr/bin/env python3
"""Writes tests/golden/launch_trace.json: the launch traces of tests/launch_trace.py's cases as the host code of THIS checkout
makes them.  No GPU: the library is loaded for its size queries only, every launch is recorded instead of made.

The fixture is the record of the host layer's kernel choices; it is rewritten only where a choice is meant to change.  A change
that must leave them alone (a refactoring of sparse.py, spconv/conv.py or the fused engine) reproduces the file byte for byte
when this script is run before and after it."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import launch_trace as LT  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else LT.GOLDEN
    LT.dump(out)
    fixture = LT.load(out)
    print(out, os.path.getsize(out), "bytes;", len(fixture["calls"]), "distinct calls;",
          {k: v["cases"] for k, v in fixture["sections"].items()})
