"""What the parallel context statistics export costs (csrc/w3_export.h: w3_export_counters_device / _staged), on enwik-shaped text
synthesised as bench.py does (tools/synth.c seed 1).  Medians of --runs runs with min - max, W3_OPT_TIMING on.  Parts (--parts):
  shapes    OrderN (11,3), (19,3), (24,3), (28,3) at --sizes from device memory, and (19,3) staged from pageable host memory: the call on
            the host clock, total and per-kernel ms from HIP events, epochs, replays, halvings
  sweep     the epoch size E over 1, 4, 16, 64 MiB at the largest size for (11,3) and (19,3): per-epoch passes over the delta table (8 x
            2^bits bytes each way) against replay scans of E bytes per listed context.  The default is the smallest median for (19,3).
  old       the claim: at 2^24 bytes, (11,3) and (19,3), the new device call (E = --old-epoch-mib, 16 MiB: one epoch) against the unchanged
            one-lane w3_export_counters (three runs of it), `beats` = faster by more than both sides' min - max spreads together; the
            two tables compared
With --history ac | huff the same parts measure w3_export_entropy_device (csrc/w3_export_entropy.h) for OrderNEntropy leaves; --out
defaults to profiles/export/export_entropy_rate.json then:
  shapes    ac:   init_model() = (11,3) over ACHistory(8, for_book1) and (19,3) over ACHistory(16, StationaryModel.new_on(input))
            huff: (11,3) and (19,3) over HuffHistory.new_on(input, 12, 12); with the key stage's ms and the epochs redone
  sweep     E over 1, 4, 16 MiB at the largest size for the (11,3) shape
  old       the (11,3) shape at 2^22 bytes (the one-lane call takes some 17 s a run there) at the default epoch
Results are merged into --out under --label (default "default"), so that other builds of the library (W3HIP_SO=..., built with
-DW3_EXP_LDS_BITS=.. or -DW3_EXP_LDS_REP=..: where the LDS form ends, copies per LDS counter) land in the same file.
    python tools/export_rate.py [--parts shapes,sweep,old] [--sizes 1e8,1e9] [--runs 5] [--label default] [--out profiles/export/export_rate.json]"""
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

MIB = 1 << 20


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "runs": len(ts)}


def beats(new, old):
    return bool(old["median_ms"] - new["median_ms"] > (new["max_ms"] - new["min_ms"]) + (old["max_ms"] - old["min_ms"]))


def measure(ctx, fn, runs, warm=True, entropy=False):
    """fn() runs one export call.  -> the call on the host clock, the profile's times, its counts"""
    if warm:
        fn()
    wall, profs = [], []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        wall.append(1e3 * (time.perf_counter() - t0))
        profs.append(ctx.export_entropy_profile() if entropy else ctx.export_profile())
    row = {"call": stats(wall)}
    for k in ("total_ms", "count_ms", "apply_ms", "replay_ms") + (("key_ms",) if entropy else ()):
        row[k[:-3]] = stats([p[k] for p in profs])
    row.update({k: profs[0][k] for k in ("epochs", "replays", "halvings") + (("huff_fixed_epochs",) if entropy else ())})
    return row


def entropy_parts(a, ctx, res, save, parts, sizes, host, d_all):
    """--history: the parts for w3_export_entropy_device"""
    def models(n):   # name -> model, the tables taken on the input of n bytes
        if a.history == "ac":
            return {"init_model 11,3 ACHistory(8,for_book1)": w3.init_model(),
                    "19,3 ACHistory(16,new_on(input))": w3.OrderNEntropy(19, 3, w3.ACHistory(16, w3.StationaryModel.new_on(ctx, d_all[:n])))}
        huff = w3.HuffHistory.new_on(ctx, d_all[:n], 12, 12)
        return {"11,3 HuffHistory(input,12,12)": w3.OrderNEntropy(11, 3, huff), "19,3 HuffHistory(input,12,12)": w3.OrderNEntropy(19, 3, huff)}

    if "shapes" in parts:
        res["shapes"] = {}
        for n in sizes:
            for name, model in models(n).items():
                out = torch.empty(1 << model.spec().nodes[0].bits, dtype=torch.int32, device="cuda")
                row = measure(ctx, lambda: ctx.export_entropy_device(model, d_all[:n], out), a.runs, entropy=True)
                res["shapes"]["%s@%d" % (name, n)] = row
                print(json.dumps({"%s@%d" % (name, n): row}), flush=True)
                save()
    if "sweep" in parts:
        res["epoch_sweep"] = {}
        n = max(sizes)
        name, model = list(models(n).items())[0]
        out = torch.empty(1 << 11, dtype=torch.int32, device="cuda")
        for e in (1, 4, 16):
            ctx.set_export_epoch(e * MIB)
            row = measure(ctx, lambda: ctx.export_entropy_device(model, d_all[:n], out), a.runs, entropy=True)
            res["epoch_sweep"]["%s@%d E=%dMiB" % (name, n, e)] = row
            print(json.dumps({"%s E=%dMiB" % (name, e): row}), flush=True)
            save()
        ctx.set_export_epoch(0)
    if "old" in parts:
        res["against_one_lane"] = {}
        n = 1 << 22
        name, model = list(models(n).items())[0]
        kept = {}
        new = measure(ctx, lambda: kept.__setitem__("new", ctx.export_entropy_device(model, d_all[:n])), a.runs, entropy=True)
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            n0, n1 = ctx.export_counters(model, host[:n])
            wall.append(1e3 * (time.perf_counter() - t0))
        got = kept["new"].cpu().numpy().view(np.uint32)
        same = bool(np.array_equal(got & 0xFFFF, n0) and np.array_equal(got >> 16, n1))
        row = {"new_device_call": new, "one_lane_call": stats(wall), "beats": beats(new["call"], stats(wall)), "tables_equal": same,
               "times_faster": round(stats(wall)["median_ms"] / max(new["call"]["median_ms"], 1e-6), 1)}
        res["against_one_lane"]["%s@%d" % (name, n)] = row
        print(json.dumps({"%s against one lane" % name: row}), flush=True)
        save()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="shapes,sweep,old")
    ap.add_argument("--sizes", default="1e8,1e9")
    ap.add_argument("--shapes", default="11:3,19:3,24:3,28:3")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--old-shapes", default="11:3,19:3", help="the shapes of `old`")
    ap.add_argument("--sweep-shapes", default="19:3,11:3", help="the shapes of `sweep`")
    ap.add_argument("--old-epoch-mib", type=int, default=16, help="the new call's epoch in `old`")
    ap.add_argument("--staged", type=int, default=1, help="0: leave the staged call out of `shapes`")
    ap.add_argument("--label", default="default")
    ap.add_argument("--history", default="", choices=("", "ac", "huff"), help="measure w3_export_entropy_device for these leaves")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = "profiles/export/export_entropy_rate.json" if a.history else "profiles/export/export_rate.json"
    parts = a.parts.split(",")
    sizes = [int(float(x)) for x in a.sizes.split(",")]
    shapes = [tuple(int(v) for v in x.split(":")) for x in a.shapes.split(",")]
    ctx = w3.Context(0)
    ctx.set_timing(True)
    res = {"library": os.path.basename(L.SO), "device": torch.cuda.get_device_name(0), "runs": a.runs}

    def save():   # after every row: what is measured is in the file even if the run ends early
        if not a.out:
            return
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        merged = {"tool": "tools/export_rate.py", "data": "enwik9-shaped text (tools/synth.c seed 1)", "builds": {}}
        if os.path.exists(a.out):
            merged = json.load(open(a.out))
        build = merged["builds"].setdefault(a.label, {})
        for k, v in res.items():
            if isinstance(v, dict):
                build.setdefault(k, {}).update(v)
            else:
                build[k] = v
        with open(a.out, "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")

    host = synth.text(max(sizes + [1 << 24]), seed=1)
    d_all = torch.from_numpy(host).cuda()
    tables = {}
    if a.history:
        if a.label == "default":
            a.label = a.history
        entropy_parts(a, ctx, res, save, parts, sizes, host, d_all)
        ctx.close()
        save()
        return
    if "shapes" in parts:
        res["shapes"] = {}
        for n in sizes:
            d_in = d_all[:n]
            for bits, align in shapes:
                out = torch.empty(1 << bits, dtype=torch.int32, device="cuda")
                row = measure(ctx, lambda: ctx.export_counters_device(w3.OrderN(bits, align), d_in, out), a.runs)
                res["shapes"]["%d,%d@%d" % (bits, align, n)] = row
                print(json.dumps({"%d,%d@%d" % (bits, align, n): row}), flush=True)
                save()
                del out
                torch.cuda.empty_cache()
            if not a.staged:
                continue
            row = measure(ctx, lambda: ctx.export_counters_staged(w3.OrderN(19, 3), host[:n]), a.runs)
            res["shapes"]["19,3@%d staged from pageable host memory" % n] = row
            print(json.dumps({"19,3 staged@%d" % n: row}), flush=True)
            save()
    if "sweep" in parts:
        res["epoch_sweep"] = {}
        n = max(sizes)
        for bits, align in [tuple(int(v) for v in x.split(":")) for x in a.sweep_shapes.split(",")]:
            out = torch.empty(1 << bits, dtype=torch.int32, device="cuda")
            for e in (1, 4, 16, 64):
                ctx.set_export_epoch(e * MIB)
                row = measure(ctx, lambda: ctx.export_counters_device(w3.OrderN(bits, align), d_all[:n], out), a.runs)
                res["epoch_sweep"]["%d,%d@%d E=%dMiB" % (bits, align, n, e)] = row
                print(json.dumps({"%d,%d E=%dMiB" % (bits, align, e): row}), flush=True)
                save()
            ctx.set_export_epoch(0)
    if "old" in parts:
        res["against_one_lane"] = {}
        n = 1 << 24
        ctx.set_export_epoch(a.old_epoch_mib * MIB)
        for bits, align in [tuple(int(v) for v in x.split(":")) for x in a.old_shapes.split(",")]:
            model = w3.OrderN(bits, align)
            new = measure(ctx, lambda: tables.__setitem__("new", ctx.export_counters_device(model, d_all[:n])), a.runs)
            wall = []
            for _ in range(3):
                t0 = time.perf_counter()
                n0, n1 = ctx.export_counters(model, host[:n])
                wall.append(1e3 * (time.perf_counter() - t0))
            got = tables["new"].cpu().numpy().view(np.uint32)
            same = bool(np.array_equal(got & 0xFFFF, n0) and np.array_equal(got >> 16, n1))
            row = {"new_device_call": new, "one_lane_call": stats(wall), "beats": beats(new["call"], stats(wall)), "tables_equal": same,
                   "times_faster": round(stats(wall)["median_ms"] / max(new["call"]["median_ms"], 1e-6), 1)}
            res["against_one_lane"]["%d,%d@%d" % (bits, align, n)] = row
            print(json.dumps({"%d,%d against one lane" % (bits, align): row}), flush=True)
            save()
        ctx.set_export_epoch(0)
    ctx.close()
    save()


if __name__ == "__main__":
    main()
