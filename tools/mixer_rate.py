"""What the logistic mixer node costs and gains (csrc/w3_lmix.h: k_lmix; csrc/w3_cm.h: the lane kernels with the mixer flag), on
enwik-shaped text synthesised as bench.py does (tools/synth.c seed 1), 64 KiB blocks: order012_mix() beside order012 (the BestOfTwo tree
over the same three leaves) and full_cm_mix() beside full_cm().  Medians of --runs runs with min - max, W3_OPT_TIMING on.  Per model and
size:
  twophase   W3_PATH_TWOPHASE: predict, mix (k_lmix), APM, coder and total ms from HIP events, compressed bytes
  generic    W3_PATH_GENERIC: the lane kernel's ms (mixer models only)
  decode     w3_decode_blocks_device wall time and MiB/s
  twophase_beats_generic   DESIGN.md 7's rule for W3_PATH_AUTO: the two-phase total's median below the lane kernel's by more than both
                           paths' min - max spreads together
Writes the JSON and a table of it as profiles/mixer/README.md.
    python tools/mixer_rate.py [--sizes 1e8,1e9] [--models order012,fullcm] [--runs 5] [--out profiles/mixer/mixer_rate.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import weath3rb0i_amd as w3  # noqa: E402
from tools import synth  # noqa: E402

BS = 65536
KEYS = ("predict_ms", "mix_ms", "apm_ms", "coder_ms", "generic_ms", "total_ms")


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "runs": len(ts)}


def beats(new, old):
    return bool(old["median_ms"] - new["median_ms"] > (new["max_ms"] - new["min_ms"]) + (old["max_ms"] - old["min_ms"]))


def models(which):
    tree = lambda: w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.OrderN(27, 3))
    out = {}
    if "order012" in which:
        out["order012"] = tree()
        out["order012_mix()"] = w3.order012_mix()
    if "fullcm" in which:
        out["full_cm()"] = w3.full_cm()
        out["full_cm_mix()"] = w3.full_cm_mix()
    return out


def readme(res, path):
    lines = ["# Logistic mixer node: rates (`python tools/mixer_rate.py`)", "",
             "%s, %s, blocks of %d bytes, medians of %d runs (min - max), milliseconds from HIP events." % (res["device"], res["data"], res["block_size"], res["runs"]), "",
             "| model @ bytes | path | predict | mix (`k_lmix`) | APM | coder | total | compressed bytes | decode MiB/s |", "|---|---|---|---|---|---|---|---|---|"]
    fmt = lambda s: "%.2f (%.2f - %.2f)" % (s["median_ms"], s["min_ms"], s["max_ms"]) if s else ""
    for key, row in res["rows"].items():
        for path_name in ("twophase", "generic"):
            r = row.get(path_name)
            if not r:
                continue
            lines.append("| %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (
                key, path_name, fmt(r.get("predict")), fmt(r.get("mix")), fmt(r.get("apm")), fmt(r.get("coder")),
                fmt(r.get("total")), "{:,}".format(row["compressed_bytes"]), row.get("decode", {}).get("mib_per_s", "")))
        if "twophase_beats_generic" in row:
            lines.append("| %s | W3_PATH_AUTO rule: two-phase beats the lane kernel by more than both spreads: **%s** | | | | | | | |" % (key, row["twophase_beats_generic"]))
    lines += ["", "`mix` beside `APM` on one input is `k_lmix` beside `k_apm0` (+ `k_apm1` for the full CM): the parent commit has no mixer to compare with.",
              "`W3_PATH_AUTO` takes the two-phase stage for a mixer spec only where the rule above holds (`lmix_auto_twophase`, `csrc/w3_lmix.h`)."]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1e8,1e9")
    ap.add_argument("--models", default="order012,fullcm")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="profiles/mixer/mixer_rate.json")
    a = ap.parse_args()
    ctx = w3.Context(0)
    ctx.set_timing(True)
    res = {"tool": "tools/mixer_rate.py", "data": "enwik9-shaped text (tools/synth.c seed 1)", "device": torch.cuda.get_device_name(0),
           "block_size": BS, "runs": a.runs, "rows": {}}

    def save():   # after every row: what is measured is in the file even if the run ends early
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        readme(res, os.path.join(os.path.dirname(os.path.abspath(a.out)), "README.md"))

    sizes = [int(float(s)) // BS * BS for s in a.sizes.split(",")]
    host = synth.text(max(sizes), seed=1, nthreads=min(16, os.cpu_count() or 1))
    for n in sizes:
        d_in = torch.from_numpy(host[:n]).cuda()
        nb = (n + BS - 1) // BS
        d_out = torch.empty(max(n, 1 << 20), dtype=torch.uint8, device="cuda")
        d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
        d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_back = torch.empty(n, dtype=torch.uint8, device="cuda")
        for name, model in models(a.models).items():
            row = {"n": n}
            for path in (("twophase", "generic") if "mix" in name else ("twophase",)):
                ctx.set_path(path)
                tms = []
                for k in range(a.runs + 1):
                    ctx.encode_blocks_device(model, d_in, BS, d_out, d_lens, d_total)
                    if k:   # (the first run warms)
                        tms.append(ctx.timing())
                row[path] = {key[:-3]: stats([t[key] for t in tms]) for key in KEYS if any(t[key] for t in tms)}
                total = int(d_total.item())
                assert row.setdefault("compressed_bytes", total) == total, "the two paths' outputs differ in size"
            ctx.set_path("auto")
            if "generic" in row:
                row["twophase_beats_generic"] = beats(row["twophase"]["total"], row["generic"]["total"])
            wall = []
            for k in range(min(a.runs, 3) + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.decode_blocks_device(model, d_out[:total], d_lens, BS, n, d_back)
                torch.cuda.synchronize()
                if k:
                    wall.append(1e3 * (time.perf_counter() - t0))
            assert torch.equal(d_back, d_in), "decode differs from the input"
            row["decode"] = stats(wall)
            row["decode"]["mib_per_s"] = round(n / 1048576 / (row["decode"]["median_ms"] / 1e3), 1)
            res["rows"]["%s@%d" % (name, n)] = row
            print(json.dumps({"%s@%d" % (name, n): row}), flush=True)
            save()
        del d_in, d_out, d_lens, d_total, d_back
        torch.cuda.empty_cache()
    ctx.close()
    save()


if __name__ == "__main__":
    main()
