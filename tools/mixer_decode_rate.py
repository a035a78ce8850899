"""Decode rates of the logistic-mixer models on both kernel families: the sixteen-lane decoder (k_decode_spec with its mixer parameter,
csrc/w3_decode_spec.h), which takes a W3_MIX_ORDER0 spec by default, against the lane-per-block kernels (k_cm / k_cm_staged with the mixer
flag; W3_OPT_VARIANT decode_lane) on the same build and the same device.  enwik-shaped text synthesised as bench.py does (tools/synth.c
seed 1), 64 KiB blocks; order012_mix() and full_cm_mix().  Per model and size, w3_decode_blocks_device on the context's own stream, timed
with events on the legacy default stream (the context's stream is a blocking one: ordered against it both ways), after a warm-up call,
medians of --runs runs with min - max:
  spec          default options: the sixteen-lane decoder (for these two models the compile-time-specialised instances of their shapes),
                table formats by the batch's size
  spec_eight    W3_OPT_TUNE bit 19: the eight-leaf form, which serves every covered mixer spec
  spec_nm_on    W3_OPT_TUNE bit 18: the nibble-major table formats whatever the size
  spec_nm_off   W3_OPT_TUNE bit 17: the row-major formats whatever the size
  lane          the lane-per-block kernels (--lane-runs runs: a run takes seconds whatever the size, one lane walks a whole block)
  spec_beats_lane / lane_beats_spec / spec_beats_eight   one median below the other by more than both forms' min - max spreads together
Every timed decode is compared with the input, and w3_last_decode_path must name the family asked for.
    python tools/mixer_decode_rate.py [--sizes 99942400,4194304,65536] [--models order012,fullcm] [--runs 3] [--lane-runs 3] [--out FILE]"""
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
FORMS = (("spec", (), 0, L.W3_PATH_SPEC), ("spec_eight", (), 1 << 19, L.W3_PATH_SPEC), ("spec_nm_on", (), 1 << 18, L.W3_PATH_SPEC), ("spec_nm_off", (), 1 << 17, L.W3_PATH_SPEC),
         ("lane", ("decode_lane",), 0, L.W3_PATH_GENERIC))


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
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--lane-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    models = {}
    if "order012" in a.models:
        models["order012_mix()"] = w3.order012_mix()
    if "fullcm" in a.models:
        models["full_cm_mix()"] = w3.full_cm_mix()
    ctx = w3.Context(0)
    res = {"tool": "tools/mixer_decode_rate.py", "data": "enwik9-shaped text (tools/synth.c seed 1)", "device": torch.cuda.get_device_name(0),
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
            assert w3.Context.decode_spec_covers(model)
            ctx.encode_blocks_device(model, d_in, BS, d_out, d_lens, d_total)
            total = int(d_total.item())
            row = {"n": n, "blocks": nb, "compressed_bytes": total}
            for form, variant, tune, path in FORMS:
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
            ctx.set_variant()
            ctx.set_tune(0)
            row["spec_beats_lane"] = beats(row["spec"], row["lane"])
            row["lane_beats_spec"] = beats(row["lane"], row["spec"])
            row["spec_beats_eight"] = beats(row["spec"], row["spec_eight"])
            res["rows"]["%s@%d" % (name, n)] = row
            save()
        del d_in, d_out, d_lens, d_total, d_back
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))
    save()


if __name__ == "__main__":
    main()
