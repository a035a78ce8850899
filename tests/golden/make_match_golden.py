"""Regenerates tests/golden/match_streams.json from tests/match_ref.py (run from the repository root: python tests/golden/make_match_golden.py).
Per input and model: [stream bytes, ACStats bits, sha256 of the u16 probabilities, sha256 of the stream]."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import pyoracle as orc  # noqa: E402
from tests import test_match_cpu as t  # noqa: E402

out = {iname: {model: t.golden_entry(orc, model, data) for model in t.GOLDEN_MODELS} for iname, data in t.golden_inputs().items()}
json.dump(out, open(t.GOLDEN, "w"), indent=1, sort_keys=True)
print("wrote", t.GOLDEN)
