#!/usr/bin/env python3
"""Writes tests/golden/mixer_streams.json: per fixed input and mixer model [stream length, ACStats bits, sha256 of the model's p stream
(u16 little endian), sha256 of the coded stream], from tests/mixer_ref.py.  The reference has no such node, so these vectors come from
this build's own CPU restatement — they pin the DEFINITION (a change of the step shows up as a diff), not reference parity."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyoracle as oracle  # noqa: E402
from tests.test_mixer_cpu import GOLDEN, GOLDEN_MODELS, golden_entry, golden_inputs  # noqa: E402

out = {iname: {m: golden_entry(oracle, m, data) for m in GOLDEN_MODELS} for iname, data in golden_inputs().items()}
json.dump(out, open(GOLDEN, "w"), indent=1, sort_keys=True)
print("wrote", GOLDEN)
