"""What the per-step statistics export costs (csrc/w3_steps.h: w3_export_steps_device), on enwik-shaped text synthesised as bench.py does
(tools/synth.c seed 1), for the bench model (Order0+1+2 + one APM stage: 6 columns with the bit) and init_model() (3 columns), at 1e8
bytes and at the largest size whose rows fit (at most 1e9).  Medians of --runs runs with min - max, W3_OPT_TIMING on.  Per model and size:
  staged / direct   the row kernel's two store forms (W3_OPT_TUNE bit 20): predict, APM and row-kernel ms from HIP events, the row kernel's
                    bytes read and written and its GB/s
  dtod              in the same process, a device-to-device copy of the row kernel's byte volume (read + written, halved: a copy
                    moves each of its bytes twice): the yardstick; `ratio` = row kernel median / copy median
  staged_beats_direct   DESIGN.md 7's rule: faster by more than both forms' min - max spreads together
  encode            w3_encode_probs_device over the model's own final column beside w3_encode_blocks_device on the same input
The store form to keep is the staged one only if staged_beats_direct holds at BOTH sizes.
    python tools/steps_rate.py [--sizes 1e8,max] [--runs 5] [--out profiles/steps/steps_rate.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import weath3rb0i_amd as w3  # noqa: E402
from weath3rb0i_amd import _lib as L  # noqa: E402
from tools import synth  # noqa: E402

BS = 65536


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "runs": len(ts)}


def beats(new, old):
    return bool(old["median_ms"] - new["median_ms"] > (new["max_ms"] - new["min_ms"]) + (old["max_ms"] - old["min_ms"]))


def models():
    return {"bench model (Order0+1+2 + APM)": w3.APM(w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.OrderN(27, 3))),
            "init_model()": w3.init_model()}


def largest_n(cols):
    """bytes of input whose rows (16 x cols per byte) fit beside the workspace of the predict phase (~90 bytes per input byte)"""
    free, _ = torch.cuda.mem_get_info()
    return int(min(1e9, free * 0.6 / (16 * cols + 90))) // BS * BS


def device_events(fn, runs):
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1e8,max")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="profiles/steps/steps_rate.json")
    a = ap.parse_args()
    ctx = w3.Context(0)
    ctx.set_timing(True)
    res = {"tool": "tools/steps_rate.py", "data": "enwik9-shaped text (tools/synth.c seed 1)", "device": torch.cuda.get_device_name(0),
           "block_size": BS, "format": "stretch_f16 with the bit column", "runs": a.runs, "rows": {}}

    def save():   # after every row: what is measured is in the file even if the run ends early
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    host = None
    for name, model in models().items():
        cols = ctx.steps_layout(model, "stretch_f16", True)["n_cols"]
        for size in a.sizes.split(","):
            n = largest_n(cols) if size == "max" else int(float(size))
            if host is None or len(host) < n:
                host = synth.text(max(n, int(1e9) if "max" in a.sizes else n), seed=1, nthreads=min(16, os.cpu_count() or 1))
            d_in = torch.from_numpy(host[:n]).cuda()
            rows = torch.empty((8 * n, cols), dtype=torch.float16, device="cuda")
            row = {"n": n, "cols": cols}
            for form, tune in (("staged", 0), ("direct", L.W3_TUNE_STEPS_DIRECT)):
                ctx.set_tune(tune)
                ctx.export_steps_device(model, d_in, BS, "stretch_f16", True, out=rows)      # warm
                profs = []
                for _ in range(a.runs):
                    ctx.export_steps_device(model, d_in, BS, "stretch_f16", True, out=rows)
                    profs.append(ctx.steps_profile())
                assert profs[0]["direct_stores"] == (1 if tune else 0)
                r = {k[:-3]: stats([p[k] for p in profs]) for k in ("predict_ms", "apm_ms", "rows_ms", "total_ms")}
                r["bytes_read"], r["bytes_written"] = profs[0]["bytes_read"], profs[0]["bytes_written"]
                r["rows_gb_per_s"] = round((r["bytes_read"] + r["bytes_written"]) / (r["rows"]["median_ms"] * 1e6), 1)
                row[form] = r
            ctx.set_tune(0)
            volume = (row["staged"]["bytes_read"] + row["staged"]["bytes_written"]) // 2 // 16 * 16
            src = torch.empty(volume, dtype=torch.uint8, device="cuda")
            dst = rows.view(torch.uint8).view(-1)
            if dst.numel() < volume:
                dst = torch.empty(volume, dtype=torch.uint8, device="cuda")
            dst[:volume].copy_(src)
            row["dtod"] = device_events(lambda: dst[:volume].copy_(src), a.runs)
            row["dtod"]["bytes_each_way"] = volume
            del src
            for form in ("staged", "direct"):
                row[form]["ratio_to_dtod"] = round(row[form]["rows"]["median_ms"] / max(row["dtod"]["median_ms"], 1e-6), 3)
            row["staged_beats_direct"] = beats(row["staged"]["rows"], row["direct"]["rows"])
            # the coder over the model's own final stream, beside the model's encode
            del rows, dst
            torch.cuda.empty_cache()
            lay = ctx.steps_layout(model, "p_u16", False)
            piece = ctx.export_steps_device(model, d_in, BS, "p_u16", False)
            d_p = piece[:, lay["col_final"]].contiguous()
            del piece
            torch.cuda.empty_cache()
            cap = max(n, 1 << 20)   # (text: the streams take about a quarter of the input)
            d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            d_lens = torch.zeros((n + BS - 1) // BS, dtype=torch.int32, device="cuda")
            d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
            wall = {"encode_probs_device": [], "encode_blocks_device": []}
            for k in range(a.runs + 1):
                for which in wall:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if which == "encode_probs_device":
                        out, _ = ctx.encode_probs_device(d_in, BS, d_p, out_cap=cap)
                        total = out.numel()
                        del out
                    else:
                        ctx.encode_blocks_device(model, d_in, BS, d_out, d_lens, d_total)
                        total = int(d_total.item())
                    if k:   # (the first round warms)
                        wall[which].append(1e3 * (time.perf_counter() - t0))
                    row.setdefault("compressed_bytes", {})[which] = total
            row["encode"] = {k: stats(v) for k, v in wall.items()}
            assert row["compressed_bytes"]["encode_probs_device"] == row["compressed_bytes"]["encode_blocks_device"]
            del d_p, d_out, d_in
            torch.cuda.empty_cache()
            res["rows"]["%s@%d" % (name, n)] = row
            print(json.dumps({"%s@%d" % (name, n): row}), flush=True)
            save()
    ctx.close()
    save()


if __name__ == "__main__":
    main()
