"""Decode rates of the match-model mixer models on both kernel families: the sixteen-lane decoder with the match leaf (k_decode_spec with
its MATCH parameter, csrc/w3_decode_spec.h; W3_OPT_VARIANT decode_match_spec) against the lane-per-block kernels (k_cm / k_cm_staged with
the MATCH flag: the default for these models) on the same build and the same device, in one run.  enwik-shaped text synthesised as
bench.py does (tools/synth.c seed 1), 64 KiB blocks; order012_match_mix() and full_cm_match_mix().  Per model and size,
w3_decode_blocks_device on the context's own stream, timed with events on the legacy default stream (the context's stream is a blocking
one: ordered against it both ways), after a warm-up call, medians of --runs runs with min - max:
  spec          decode_match_spec: the sixteen-lane decoder (the eight-leaf form with MATCH), table formats by the batch's size
  spec_nm_on    ... with W3_OPT_TUNE bit 18: the nibble-major table formats whatever the size
  spec_nm_off   ... with W3_OPT_TUNE bit 17: the row-major formats whatever the size
  lane          default options: the lane-per-block kernels (--lane-runs runs: a run takes seconds whatever the size)
  spec_beats_lane / lane_beats_spec   one median below the other by more than both forms' min - max spreads together
Every timed decode is compared with the input, and w3_last_decode_path must name the family asked for.
    python tools/match_decode_rate.py [--sizes 99942400,4194304,65536] [--models order012,fullcm] [--runs 3] [--lane-runs 3] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import weath3rb0i_amd as w3  # noqa: E402
from tools import synth  # noqa: E402
from weath3rb0i_amd import _lib as L  # noqa: E402

BS = 65536
BIT = ("decode_match_spec",)
FORMS = (("spec", BIT, 0, L.W3_PATH_SPEC), ("spec_nm_on", BIT, 1 << 18, L.W3_PATH_SPEC), ("spec_nm_off", BIT, 1 << 17, L.W3_PATH_SPEC),
         ("lane", (), 0, L.W3_PATH_GENERIC))


def stats(ts, n):
    ts = sorted(ts)
    med = float(np.median(ts))
    return {"median_ms": round(med, 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3), "runs": len(ts),
            "mib_per_s": round(n / 1048576 / (med / 1e3), 1)}


def beats(new, old):
    return bool(old["median_ms"] - new["median_ms"] > (new["max_ms"] - new["min_ms"]) + (old["max_ms"] - old["min_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="99942400,4194304,65536")
    ap.add_argument("--models", default="order012,fullcm")
    ap.add_argument("--forms", default=",".join(f[0] for f in FORMS))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--lane-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    models = {}
    if "order012" in a.models:
        models["order012_match_mix()"] = w3.order012_match_mix()
    if "fullcm" in a.models:
        models["full_cm_match_mix()"] = w3.full_cm_match_mix()
    forms = [f for f in FORMS if f[0] in a.forms.split(",")]
    ctx = w3.Context(0)
    res = {"tool": "tools/match_decode_rate.py", "data": "enwik9-shaped text (tools/synth.c seed 1)", "device": torch.cuda.get_device_name(0),
           "block_size": BS, "runs": a.runs, "lane_runs": a.lane_runs, "rows": {}}

    def save():   # after every row: what is measured is in the file even if the run ends early
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    sizes = [int(float(s)) for s in a.sizes.split(",")]
    host = synth.text(max(sizes), seed=1, nthreads=min(16, os.cpu_count() or 1))
    stream = torch.cuda.default_stream()
    for n in sizes:
        d_in = torch.from_numpy(host[:n]).cuda()
        nb = (n + BS - 1) // BS
        d_out = torch.empty(max(n, 1 << 20), dtype=torch.uint8, device="cuda")
        d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
        d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_back = torch.empty(n, dtype=torch.uint8, device="cuda")
        for name, model in models.items():
            assert w3.Context.decode_spec_covers(model, variant=BIT) and not w3.Context.decode_spec_covers(model)
            ctx.encode_blocks_device(model, d_in, BS, d_out, d_lens, d_total)
            total = int(d_total.item())
            row = {"n": n, "blocks": nb, "compressed_bytes": total}
            for form, variant, tune, path in forms:
                ctx.set_variant(*variant)
                ctx.set_tune(tune)
                ms = []
                for k in range((a.lane_runs if form == "lane" else a.runs) + 1):
                    d_back.zero_()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    ctx.decode_blocks_device(model, d_out[:total], d_lens, BS, n, d_back)
                    e1.record(stream)
                    e1.synchronize()
                    assert ctx.last_decode_path() == path, (form, ctx.last_decode_path())
                    assert torch.equal(d_back, d_in), "decode differs from the input: " + form
                    if k:   # (the first call warms)
                        ms.append(e0.elapsed_time(e1))
                row[form] = stats(ms, n)
                print(json.dumps({"%s@%d" % (name, n): {form: row[form]}}), flush=True)
                res["rows"]["%s@%d" % (name, n)] = row
                save()
            ctx.set_variant()
            ctx.set_tune(0)
            if "spec" in row and "lane" in row:
                row["spec_beats_lane"] = beats(row["spec"], row["lane"])
                row["lane_beats_spec"] = beats(row["lane"], row["spec"])
            res["rows"]["%s@%d" % (name, n)] = row
            save()
        del d_in, d_out, d_lens, d_total, d_back
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))
    save()


if __name__ == "__main__":
    main()
