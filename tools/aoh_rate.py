"""AC-over-Huffman rates (w3_aoh_*; bin/ac-over-huffman/main.rs) on a device-resident enwik-shaped corpus synthesised as bench.py does
(tools/synth.c seed 1), 64 KiB blocks, at the reference's two best published configurations (hsize 13 / ctx 24 and hsize 12 / ctx 19):
encode and decode MiB/s on every path that is built and under W3_PATH_AUTO (the decode also on the sixteen-lane decoder, W3_OPT_VARIANT
aoh_decode_spec) (with timing.path, the form it took, and the phases'
milliseconds of one more call with W3_OPT_TIMING), the counting sink, the compressed size beside order012's and OrderN(32, 1)'s on the
same input; the wall time of the driver's full sweep (huffman_size 7..15 x ctx_bits 8..30, one call) on 20 MB; and the rate of the tests'
CPU truth (tests/host/aoh_ref.c, a C restatement of the driver's loop — not the reference) on 16 threads.  Every shape is warmed up
first; each figure is the median (and min / max) of --runs timed calls, host clock after a synchronise.
    python tools/aoh_rate.py [--sizes 1e9,1e8] [--runs 5] [--sweep-bytes 2e7] [--cpu-bytes 1e8] [--out profiles/aoh/aoh_rate.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import weath3rb0i_amd as w3  # noqa: E402
from weath3rb0i_amd import _lib as L  # noqa: E402
from tools import synth  # noqa: E402

CONFIGS = [(13, 24), (12, 19)]
BS = 65536


def timed(fn, runs):
    fn()   # (warm-up of this shape: workspace, Counter tables)
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median_ms": round(1e3 * float(np.median(ts)), 3), "min_ms": round(1e3 * ts[0], 3), "max_ms": round(1e3 * ts[-1], 3), "runs": runs}


def rate(row, n):
    row["mib_s"] = round(n / 2**20 / (row["median_ms"] / 1e3), 1)
    return row


def paths(ctx, code):
    out = ["generic"]
    ctx.set_path("twophase")
    try:
        ctx.aoh_encode_stats(code, 8, b"abracadabra", 64)
        out.append("twophase")
    except w3.W3Error as e:
        if e.code != L.W3_E_UNSUPPORTED:
            raise
    finally:
        ctx.set_path("auto")
    return out


def model_size(ctx, model, d_in, n):
    nb = (n + BS - 1) // BS
    d_bits = torch.zeros(nb, dtype=torch.int32, device="cuda")
    spec = model.spec()
    import ctypes as C
    ctx._chk(ctx.lib.w3_encode_stats_device(ctx.h, C.byref(spec), C.c_void_p(d_in.data_ptr()), n, BS, C.c_void_p(d_bits.data_ptr()), None))
    return int(d_bits.cpu().numpy().view(np.uint32).astype(np.uint64).sum()) // 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1e9,1e8")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sweep-bytes", type=float, default=2e7)
    ap.add_argument("--cpu-bytes", type=float, default=1e8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = w3.Context(0)
    res = {"tool": "tools/aoh_rate.py", "data": "enwik9-shaped text (tools/synth.c seed 1)", "block_size": BS, "runs": a.runs,
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in [int(float(x)) for x in a.sizes.split(",")]:
        host = synth.text(n, seed=1)
        d_in = torch.from_numpy(host).cuda()
        nb = (n + BS - 1) // BS
        row = {"blocks": nb,
               "csize_order012": model_size(ctx, w3.BestOfTwoModel(w3.BestOfTwoModel(w3.Order0(), w3.Order1()), w3.OrderN(27, 3)), d_in, n),
               "csize_ordern_32_1": model_size(ctx, w3.OrderN(32, 1), d_in, n)}
        print(json.dumps({str(n): row}), flush=True)
        for hs, cb in CONFIGS:
            code = w3.HuffCode.new(host, hs)
            key = "hsize%d_ctx%d" % (hs, cb)
            r = {"huffman_bits_per_byte": round(float(np.asarray(code.lens, dtype=np.float64)[host].mean()), 4) if n <= 2e8 else None}
            d_comp = torch.empty(n + 64 * nb + 4096, dtype=torch.uint8, device="cuda")
            d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
            d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
            d_bits = torch.zeros(nb, dtype=torch.int32, device="cuda")
            d_back = torch.empty(n, dtype=torch.uint8, device="cuda")
            ref = None
            for path in paths(ctx, code) + ["auto"]:
                ctx.set_path(path)
                r["encode_" + path] = rate(timed(lambda: ctx.aoh_encode_blocks_device(code, cb, d_in, BS, d_comp, d_lens, d_total), a.runs), n)
                total = int(d_total.item())
                r["stats_" + path] = rate(timed(lambda: ctx.aoh_encode_stats_device(code, cb, d_in, BS, d_bits), a.runs), n)
                # one more call of each with W3_OPT_TIMING: the form taken (timing.path) and the phases' milliseconds
                ctx.set_timing(True)
                for what, fn in (("encode_", lambda: ctx.aoh_encode_blocks_device(code, cb, d_in, BS, d_comp, d_lens, d_total)),
                                 ("stats_", lambda: ctx.aoh_encode_stats_device(code, cb, d_in, BS, d_bits))):
                    fn()
                    tm = ctx.timing()
                    r[what + path]["timing"] = {k: (round(tm[k], 3) if isinstance(tm[k], float) else tm[k])
                                                for k in ("path", "predict_ms", "coder_ms", "pack_ms", "generic_ms", "total_ms", "predict_bytes", "coder_bytes")}
                ctx.set_timing(False)
                if path != "auto":   # (decode ignores the option)
                    r["decode_" + path] = rate(timed(lambda: ctx.aoh_decode_blocks_device(code, cb, d_comp[:total], d_lens, BS, n, d_back), a.runs), n)
                    assert bool((d_back == d_in).all())
                    if path == "generic":   # the same decode on the sixteen-lane decoder (W3_OPT_VARIANT aoh_decode_spec; timing.path tells what ran)
                        ctx.set_variant("aoh_decode_spec")
                        d_back.zero_()
                        r["decode_aoh_decode_spec"] = rate(timed(lambda: ctx.aoh_decode_blocks_device(code, cb, d_comp[:total], d_lens, BS, n, d_back), a.runs), n)
                        r["decode_aoh_decode_spec"]["path"] = ctx.timing()["path"]
                        ctx.set_variant()
                        assert bool((d_back == d_in).all())
                # every path writes the same streams
                sig = (total, int(d_lens.to(torch.int64).sum().item()), int(d_bits.to(torch.int64).sum().item()), int(d_comp[:total].to(torch.int64).sum().item()))
                ref = ref or sig
                assert sig == ref, (path, sig, ref)
                ctx.set_path("auto")
            r["compressed_bytes"] = total
            r["csize"] = int(d_bits.cpu().numpy().view(np.uint32).astype(np.uint64).sum()) // 8
            row[key] = r
            print(json.dumps({str(n): {key: r}}), flush=True)
            del d_comp, d_lens, d_total, d_bits, d_back
            torch.cuda.empty_cache()
        res["sizes"][str(n)] = row
        del d_in
        torch.cuda.empty_cache()
    if a.sweep_bytes:
        from weath3rb0i_amd import sweep
        n = int(a.sweep_bytes)
        host = synth.text(n, seed=1).tobytes()
        lines = []
        t0 = time.perf_counter()
        best, params, _ = sweep.sweep_ac_over_huffman(ctx, host, BS, out=lines.append)
        res["sweep"] = {"bytes": n, "configurations": 9 * 23, "wall_s": round(time.perf_counter() - t0, 3), "best_csize": best, "best_hsize_ctx": list(params)}
        print(json.dumps({"sweep": res["sweep"]}), flush=True)
    if a.cpu_bytes:   # the tests' CPU truth, 16 threads: a C restatement of the driver's loop
        from oracle import pyoracle
        from tests import aoh_ref
        n = int(a.cpu_bytes)
        host = synth.text(n, seed=1).tobytes()
        with tempfile.TemporaryDirectory() as d:
            if aoh_ref.c_lib(d) is not None:
                res["cpu_truth_c_restatement_16_threads"] = {}
                for hs, cb in CONFIGS:
                    codes, lens = aoh_ref.code_table(pyoracle, host, hs)
                    t0 = time.perf_counter()
                    _, bl = aoh_ref.encode_blocks(pyoracle, d, codes, lens, cb, host, BS)
                    dt = time.perf_counter() - t0
                    res["cpu_truth_c_restatement_16_threads"]["hsize%d_ctx%d" % (hs, cb)] = {"bytes": n, "encode_s": round(dt, 3), "mib_s": round(n / 2**20 / dt, 1),
                                                                                             "compressed_bytes": int(bl.astype(np.uint64).sum())}
                print(json.dumps({"cpu": res["cpu_truth_c_restatement_16_threads"]}), flush=True)
    ctx.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
