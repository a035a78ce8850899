"""What table preparation costs on the device (csrc/w3_prep.h) against the host loops it replaces, on enwik-shaped text synthesised as
bench.py does (tools/synth.c seed 1).  Per size:
  kernels              k_hist256, k_hist256_sum, k_stat_count, k_stat_walk from HIP events (w3_table_prep_profile): median and min / max of
                       --runs runs, the halvings per bit position, and what one halving costs if the walk is charged to them alone
  hist_rep             k_hist256 with 1, 2, 4, 8 and 16 copies of a wave's counters, on the text and on a buffer of equal bytes (the worst
                       case for same-address LDS adds): the measurement behind W3_HIST_REP
  *_device, *_staged   the four context calls end to end (host clock; the staged forms include the copy from pageable host memory)
  host_*               w3_stationary_table and the histogram loop of w3_huff_code_table on this machine's CPU, one thread: --host-runs
                       runs up to 1e8 bytes, once at 1e9
  crc_table            w3_crc32_blocks_device in the same run: a kernel that only streams the same bytes
  init_model_encode    w3_encode_blocks_device with init_model() (the model whose table StationaryModel::new prepares)
  beats_host           device median < host median by more than the two sides' min-max spreads together
    python tools/table_prep_rate.py [--sizes 1e6,1e8,1e9] [--runs 5] [--out profiles/table_prep/table_prep_rate.json]"""
import argparse
import ctypes as C
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


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "runs": len(ts)}


def timed(fn, runs, warm=True):
    if warm:
        fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return stats(ts)


def beats(dev, host):
    return bool(host["median_ms"] - dev["median_ms"] > (dev["max_ms"] - dev["min_ms"]) + (host["max_ms"] - host["min_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1e6,1e8,1e9")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default="profiles/table_prep/table_prep_rate.json")
    a = ap.parse_args()
    ctx = w3.Context(0)
    lib = L.load()
    res = {"tool": "tools/table_prep_rate.py", "data": "enwik9-shaped text (tools/synth.c seed 1)", "runs": a.runs, "device": torch.cuda.get_device_name(0),
           "stat_tile": L.W3_STAT_TILE, "stat_batch": L.W3_STAT_BATCH, "hist_rep": L.W3_HIST_REP, "sizes": {}}
    for n in [int(float(x)) for x in a.sizes.split(",")]:
        host = synth.text(n, seed=1)
        d_in = torch.from_numpy(host).cuda()
        d_eq = torch.full((n,), 0x20, dtype=torch.uint8, device="cuda")
        row = {"bytes": n}
        ctx.table_prep_profile(d_in)
        profs = [ctx.table_prep_profile(d_in) for _ in range(a.runs)]
        row["kernels"] = {k: stats([p[k + "_ms"] for p in profs]) for k in ("hist", "hist_sum", "stat_count", "stat_walk")}
        row["halvings"] = profs[0]["halvings"]
        want_counts = np.bincount(host, minlength=256)
        assert profs[0]["counts"].tolist() == want_counts.tolist()
        if max(row["halvings"]):
            row["walk_us_per_halving_of_the_busiest_position"] = round(1e3 * row["kernels"]["stat_walk"]["median_ms"] / max(row["halvings"]), 3)
        row["hist_rep"] = {}
        for rep in (1, 2, 4, 8, 16):
            ctx.table_prep_profile(d_in, rep), ctx.table_prep_profile(d_eq, rep)
            row["hist_rep"][str(rep)] = {"text": stats([ctx.table_prep_profile(d_in, rep)["hist_ms"] for _ in range(a.runs)]),
                                         "equal_bytes": stats([ctx.table_prep_profile(d_eq, rep)["hist_ms"] for _ in range(a.runs)])}
        row["hist_equal_bytes"] = row["hist_rep"][str(L.W3_HIST_REP)]["equal_bytes"]
        row["histogram_device"] = timed(lambda: ctx.histogram_device(d_in), a.runs)
        row["stationary_device"] = timed(lambda: ctx.stationary_table(d_in), a.runs)
        row["histogram_staged"] = timed(lambda: ctx.histogram(host), a.runs)
        row["stationary_staged"] = timed(lambda: ctx.stationary_table(host), a.runs)
        table = ctx.stationary_table(d_in)
        # the host loops, straight through the library (no copy in front)
        hp, t8, code = host.ctypes.data_as(C.c_void_p), (C.c_uint16 * 8)(), L.HuffCode()
        hruns = 1 if n > 10**8 else a.host_runs
        row["host_stationary"] = timed(lambda: lib.w3_stationary_table(hp, n, t8), hruns, warm=False)
        assert list(t8) == table == profs[0]["table"]
        row["host_histogram"] = timed(lambda: lib.w3_huff_code_table(hp, n, 16, C.byref(code)), hruns, warm=False)
        assert bytes(code) == bytes(w3.HuffCode.from_counts(profs[0]["counts"], 16).table)
        row["beats_host"] = {"histogram_device": beats(row["histogram_device"], row["host_histogram"]),
                             "histogram_staged": beats(row["histogram_staged"], row["host_histogram"]),
                             "stationary_device": beats(row["stationary_device"], row["host_stationary"]),
                             "stationary_staged": beats(row["stationary_staged"], row["host_stationary"])}
        bs = 65536
        nb = (n + bs - 1) // bs
        d_crc = torch.zeros(nb, dtype=torch.int32, device="cuda")
        row["crc_table"] = timed(lambda: ctx.crc32_blocks_device(d_in, bs, d_crc), a.runs)
        d_comp = torch.empty(n + 64 * nb + 4096, dtype=torch.uint8, device="cuda")
        d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
        d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
        model = w3.OrderNEntropy.new(11, 3, w3.ACHistory.new(8, w3.StationaryModel.from_table(table)))   # init_model() with this input's table
        row["init_model_encode"] = timed(lambda: ctx.encode_blocks_device(model, d_in, bs, d_comp, d_lens, d_total), a.runs)
        res["sizes"][str(n)] = row
        print(json.dumps({str(n): row}), flush=True)
        del d_in, d_eq, d_comp
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
