"""What the per-block CRC-32 costs (w3_crc32_blocks_device, w3_crc32_verify_device and the checked ranges calls) on a device-resident
enwik-shaped corpus synthesised as bench.py does (tools/synth.c seed 1), in 64 KiB blocks, the bench model:
  crc_alone            w3_crc32_blocks_device over the corpus (checked against zlib on the first and the last block), with the rate it
                       amounts to and the time reading the corpus once at --hbm-tbs (the achievable HBM rate) would take
  full_decode          w3_decode_blocks_device, as the parent commit runs it
  full_decode_verify   the same followed by w3_crc32_verify_device on its output
  ranges_*             w3_decode_ranges_device for one 4 KiB range and for 64 of them, unchecked and checked (whole blocks + verify)
Every shape is warmed up first; each figure is the median (and min / max) of --runs timed calls, host clock after a synchronise (the
calls return when their output is complete).  verify_exceeds_spread: whether the verify's added median time is larger than the unverified
decode's own max - min.
    python tools/crc_rate.py [--sizes 1e9] [--runs 5] [--out profiles/crc/crc_rate.json]"""
import argparse
import json
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import weath3rb0i_amd as w3  # noqa: E402
from tools import synth  # noqa: E402


def timed(fn, runs):
    fn()   # (warm-up of this shape: workspace, model tables)
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median_ms": round(1e3 * float(np.median(ts)), 3), "min_ms": round(1e3 * ts[0], 3), "max_ms": round(1e3 * ts[-1], 3), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1e9")
    ap.add_argument("--block-size", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--model", default="order012apm")
    ap.add_argument("--hbm-tbs", type=float, default=6.0, help="achievable HBM read rate, TB/s, for the comparison line")
    ap.add_argument("--out", default="profiles/crc/crc_rate.json")
    a = ap.parse_args()
    bs = a.block_size
    model, mname = bench.make_model(w3, a.model)
    ctx = w3.Context(0)
    rng = np.random.default_rng(12345)
    res = {"tool": "tools/crc_rate.py", "model": mname, "block_size": bs, "data": "enwik9-shaped text (tools/synth.c seed 1)", "runs": a.runs,
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in [int(float(x)) for x in a.sizes.split(",")]:
        host = synth.text(n, seed=1)
        d_in = torch.from_numpy(host).cuda()
        nb = (n + bs - 1) // bs
        d_crc = torch.zeros(nb, dtype=torch.int32, device="cuda")
        row = {"bytes": n, "blocks": nb}
        row["crc_alone"] = timed(lambda: ctx.crc32_blocks_device(d_in, bs, d_crc), a.runs)
        crc = d_crc.cpu().numpy().view(np.uint32).copy()
        assert int(crc[0]) == zlib.crc32(host[:bs].tobytes()) and int(crc[-1]) == zlib.crc32(host[(nb - 1) * bs:].tobytes())
        row["crc_alone"]["tb_s"] = round(n / 1e12 / (row["crc_alone"]["median_ms"] / 1e3), 3)
        row["read_once_at_hbm_rate_ms"] = round(n / (a.hbm_tbs * 1e12) * 1e3, 3)
        d_comp = torch.empty(n // 2 + 64 * nb + 4096, dtype=torch.uint8, device="cuda")
        d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
        d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx.encode_blocks_device(model, d_in, bs, d_comp, d_lens, d_total)
        comp = d_comp[:int(d_total.item())]
        d_back = torch.empty(n, dtype=torch.uint8, device="cuda")

        def decode_verify():
            ctx.decode_blocks_device(model, comp, d_lens, bs, n, d_back)
            ctx.crc32_verify_device(d_back, bs, d_crc)

        row["full_decode"] = timed(lambda: ctx.decode_blocks_device(model, comp, d_lens, bs, n, d_back), a.runs)
        row["full_decode_verify"] = timed(decode_verify, a.runs)
        added = row["full_decode_verify"]["median_ms"] - row["full_decode"]["median_ms"]
        spread = row["full_decode"]["max_ms"] - row["full_decode"]["min_ms"]
        row["verify_added_ms"], row["full_decode_spread_ms"], row["verify_exceeds_spread"] = round(added, 3), round(spread, 3), bool(added > spread)
        d_out = torch.empty(64 * 4096, dtype=torch.uint8, device="cuda")

        def rand_ranges(k, length=4096):
            return np.stack([rng.integers(0, n - length, k), np.full(k, length)], axis=1)

        r0 = rand_ranges(64)
        ctx.decode_ranges_device(model, comp, d_lens, bs, n, r0, d_out, crc=crc)
        assert d_out.cpu().numpy().tobytes() == b"".join(host[o:o + k].tobytes() for o, k in r0.tolist())
        for k in (1, 64):
            row["ranges_%d_x_4k" % k] = timed(lambda: ctx.decode_ranges_device(model, comp, d_lens, bs, n, rand_ranges(k), d_out), a.runs)
            row["ranges_%d_x_4k_checked" % k] = timed(lambda: ctx.decode_ranges_device(model, comp, d_lens, bs, n, rand_ranges(k), d_out, crc=crc), a.runs)
        res["sizes"][str(n)] = row
        print(json.dumps({str(n): row}), flush=True)
        del d_in, d_comp, d_back, d_out
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
