"""What the match-model leaf costs and gains (csrc/w3_match.h: k_match_keys; the lane kernels with the MATCH flag), on enwik-shaped text
synthesised as bench.py does (tools/synth.c seed 1), 64 KiB blocks: order012_match_mix() beside order012_mix() and full_cm_match_mix()
beside full_cm_mix(), and order012_match_mix() with log_slots 12, 14, 16 and 18 (what decides the factories' default).  Medians of --runs
runs with min - max, W3_OPT_TIMING on, W3_PATH_TWOPHASE.  Per model and size: predict, match (k_match_keys), small, mix, APM, coder and
total ms from HIP events, compressed bytes, and for the match models the lane kernels' decode wall time and MiB/s (the sixteen-lane
decoder does not take the leaf).  Writes the JSON and a table of it as README.md beside it.
    python tools/match_rate.py [--sizes 99942400] [--models order012,fullcm,slots] [--runs 3] [--out profiles/match/match_rate.json]"""
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
KEYS = ("predict_ms", "match_ms", "small_ms", "mix_ms", "apm_ms", "coder_ms", "total_ms")
LOG_SLOTS = (12, 14, 18)   # beside the default 16


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "runs": len(ts)}


def models(which):
    out = {}
    if "order012" in which:
        out["order012_mix()"] = (w3.order012_mix(), False)
        out["order012_match_mix()"] = (w3.order012_match_mix(), True)
    if "slots" in which:
        for ls in LOG_SLOTS:
            out["order012 + MatchModel(4, %d)" % ls] = (w3.LogisticMixer([w3.Order0(), w3.Order1(), w3.OrderN(27, 3), w3.MatchModel(4, ls)]), False)
    if "fullcm" in which:
        out["full_cm_mix()"] = (w3.full_cm_mix(), False)
        out["full_cm_match_mix()"] = (w3.full_cm_match_mix(), True)
    return out


def readme(res, path):
    lines = ["# Match-model leaf: rates (`python tools/match_rate.py`)", "",
             "%s, %s, blocks of %d bytes, medians of %d runs (min - max), milliseconds from HIP events, `W3_PATH_TWOPHASE`." % (res["device"], res["data"], res["block_size"], res["runs"]), "",
             "| model @ bytes | predict | match (`k_match_keys`) | small | mix | APM | coder | total | compressed bytes | lane-kernel decode MiB/s |", "|---|---|---|---|---|---|---|---|---|---|"]
    fmt = lambda s: "%.2f (%.2f - %.2f)" % (s["median_ms"], s["min_ms"], s["max_ms"]) if s else ""
    for key, row in res["rows"].items():
        r = row["twophase"]
        lines.append("| %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (
            key, fmt(r.get("predict")), fmt(r.get("match")), fmt(r.get("small")), fmt(r.get("mix")), fmt(r.get("apm")), fmt(r.get("coder")), fmt(r.get("total")),
            "{:,}".format(row["compressed_bytes"]), row.get("decode", {}).get("mib_per_s", "")))
    lines += ["", "`match` is inside `predict`.  The parent commit has no match leaf: the rows without one are this build's, on the same input in the same run."]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="99942400")
    ap.add_argument("--models", default="order012,slots,fullcm")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="profiles/match/match_rate.json")
    a = ap.parse_args()
    ctx = w3.Context(0)
    ctx.set_timing(True)
    ctx.set_path("twophase")
    res = {"tool": "tools/match_rate.py", "data": "enwik9-shaped text (tools/synth.c seed 1)", "device": torch.cuda.get_device_name(0),
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
        for name, (model, decode) in models(a.models).items():
            row = {"n": n}
            tms = []
            for k in range(a.runs + 1):
                ctx.encode_blocks_device(model, d_in, BS, d_out, d_lens, d_total)
                if k:   # (the first run warms)
                    tms.append(ctx.timing())
            row["twophase"] = {key[:-3]: stats([t[key] for t in tms]) for key in KEYS if any(t[key] for t in tms)}
            total = row["compressed_bytes"] = int(d_total.item())
            if decode:
                wall = []
                for k in range(a.runs + 1):
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
