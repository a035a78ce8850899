"""Random-access decode rates (w3_decode_ranges_device / w3_decode_ranges) of the bench model on a device-resident enwik-shaped corpus
synthesised as bench.py does (tools/synth.c seed 1): one 4 KiB range at a random offset, batches of 64 / 1,024 / 4,096 random 4 KiB
ranges, one contiguous 64 MiB range, and the full decode (w3_decode_blocks_device) of the same corpus — then the range cases through the
host variant from pinned memory.  Every shape is warmed up first; each figure is the median (and min / max) of --runs timed calls, host
clock after a synchronise (the calls return when their output is complete).
    python tools/range_rate.py [--size 1e9] [--block-sizes 65536,16384] [--runs 20] [--out profiles/ranges/range_rate.json]
--aoh HSIZE,CTX: the same shapes on AC-over-Huffman streams (w3_aoh_decode_ranges[_device]), each with the sixteen-lane decoder
k_aoh_decode_spec and with the lane kernel (W3_OPT_VARIANT decode_lane), device and host variants, with timing.path of every shape; the
full decode with and without W3_OPT_VARIANT aoh_decode_spec.
    python tools/range_rate.py --aoh 12,19 [--runs 5] [--out profiles/aoh_ranges/range_rate_aoh_12_19.json]"""
import argparse
import json
import os
import sys
import time

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


def main_aoh(a):
    hs, cb = [int(x) for x in a.aoh.split(",")]
    n = int(a.size)
    host = synth.text(n, seed=1)
    d_in = torch.from_numpy(host).cuda()
    code = w3.HuffCode.new(host, hs)
    ctx = w3.Context(0)
    rng = np.random.default_rng(12345)
    res = {"tool": "tools/range_rate.py --aoh", "huffman_size": hs, "ctx_bits": cb, "spec_covers": ctx.aoh_decode_spec_covers(cb), "bytes": n,
           "data": "enwik9-shaped text (tools/synth.c seed 1)", "runs": a.runs, "device": torch.cuda.get_device_name(0), "block_sizes": {}}
    for bs in [int(x) for x in a.block_sizes.split(",")]:
        nb = (n + bs - 1) // bs
        d_comp = torch.empty(n + 64 * nb + 4096, dtype=torch.uint8, device="cuda")
        d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
        d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx.aoh_encode_blocks_device(code, cb, d_in, bs, d_comp, d_lens, d_total)
        total = int(d_total.item())
        comp = d_comp[:total]
        d_out = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
        h_comp = torch.empty(total, dtype=torch.uint8).pin_memory()
        h_comp.copy_(comp.cpu())
        hc = h_comp.numpy()
        lens = d_lens.cpu().numpy().view(np.uint32).copy()

        def rand_ranges(k, length=4096):
            return np.stack([rng.integers(0, n - length, k), np.full(k, length)], axis=1)

        big = np.array([[int(rng.integers(0, n - (64 << 20))), 64 << 20]])
        row = {"compressed_bytes": total, "blocks": nb}

        def shape(key, fn):
            r = timed(fn, a.runs)
            r["path"] = ctx.timing()["path"]
            row[key] = r
            print(json.dumps({str(bs): {key: r}}), flush=True)

        for form, variant in (("spec", ()), ("lane", ("decode_lane",))):
            ctx.set_variant(*variant)
            r0 = rand_ranges(64)
            w0 = b"".join(host[o:o + k].tobytes() for o, k in r0.tolist())
            ctx.aoh_decode_ranges_device(code, cb, comp, d_lens, bs, n, r0, d_out)
            assert d_out[:64 * 4096].cpu().numpy().tobytes() == w0
            shape(form + "_one_4k", lambda: ctx.aoh_decode_ranges_device(code, cb, comp, d_lens, bs, n, rand_ranges(1), d_out))
            for k in (64, 1024, 4096):
                shape(form + "_batch_%d_x_4k" % k, lambda: ctx.aoh_decode_ranges_device(code, cb, comp, d_lens, bs, n, rand_ranges(k), d_out))
            shape(form + "_one_64m", lambda: ctx.aoh_decode_ranges_device(code, cb, comp, d_lens, bs, n, big, d_out))
            assert d_out.cpu().numpy().tobytes() == host[big[0, 0]:big[0, 0] + (64 << 20)].tobytes()
            if not a.no_host:   # the host variant from pinned memory: only the selected streams cross PCIe
                assert ctx.aoh_decode_ranges(code, cb, hc, lens, bs, n, r0).tobytes() == w0
                shape(form + "_host_one_4k", lambda: ctx.aoh_decode_ranges(code, cb, hc, lens, bs, n, rand_ranges(1)))
                for k in (64, 1024, 4096):
                    shape(form + "_host_batch_%d_x_4k" % k, lambda: ctx.aoh_decode_ranges(code, cb, hc, lens, bs, n, rand_ranges(k)))
                shape(form + "_host_one_64m", lambda: ctx.aoh_decode_ranges(code, cb, hc, lens, bs, n, big))
        d_back = torch.empty(n, dtype=torch.uint8, device="cuda")
        for key, variant in (("full_decode", ()), ("full_decode_aoh_decode_spec", ("aoh_decode_spec",))):
            ctx.set_variant(*variant)
            d_back.zero_()
            shape(key, lambda: ctx.aoh_decode_blocks_device(code, cb, comp, d_lens, bs, n, d_back))
            row[key]["mib_s"] = round(n / 2**20 / (row[key]["median_ms"] / 1e3), 1)
            assert bool((d_back == d_in).all())
        ctx.set_variant()
        res["block_sizes"][str(bs)] = row
        del d_comp, d_lens, d_out, d_back, h_comp
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=float, default=1e9)
    ap.add_argument("--block-sizes", default="65536,16384")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--model", default="order012apm")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--aoh", default=None, metavar="HSIZE,CTX", help="AC-over-Huffman streams: w3_aoh_decode_ranges[_device], both decoders")
    a = ap.parse_args()
    if a.aoh:
        return main_aoh(a)
    n = int(a.size)
    model, mname = bench.make_model(w3, a.model)
    host = synth.text(n, seed=1)
    d_in = torch.from_numpy(host).cuda()
    ctx = w3.Context(0)
    rng = np.random.default_rng(12345)
    res = {"tool": "tools/range_rate.py", "model": mname, "bytes": n, "data": "enwik9-shaped text (tools/synth.c seed 1)", "runs": a.runs,
           "device": torch.cuda.get_device_name(0), "block_sizes": {}}
    for bs in [int(x) for x in a.block_sizes.split(",")]:
        nb = (n + bs - 1) // bs
        d_comp = torch.empty(n // 2 + 64 * nb + 4096, dtype=torch.uint8, device="cuda")
        d_lens = torch.zeros(nb, dtype=torch.int32, device="cuda")
        d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx.encode_blocks_device(model, d_in, bs, d_comp, d_lens, d_total)
        total = int(d_total.item())
        comp = d_comp[:total]
        d_out = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")

        def rand_ranges(k, length=4096):
            return np.stack([rng.integers(0, n - length, k), np.full(k, length)], axis=1)

        # the ranges of every timed call are drawn anew (a random offset each time); they are checked once per shape
        def dev(k):
            def f():
                r = rand_ranges(k)
                ctx.decode_ranges_device(model, comp, d_lens, bs, n, r, d_out)
            return f

        r0 = rand_ranges(64)
        ctx.decode_ranges_device(model, comp, d_lens, bs, n, r0, d_out)
        assert d_out[:64 * 4096].cpu().numpy().tobytes() == b"".join(host[o:o + k].tobytes() for o, k in r0.tolist())
        big = np.array([[int(rng.integers(0, n - (64 << 20))), 64 << 20]])
        row = {"compressed_bytes": total, "blocks": nb}
        row["one_4k"] = timed(dev(1), a.runs)
        for k in (64, 1024, 4096):
            row["batch_%d_x_4k" % k] = timed(dev(k), a.runs)
        row["one_64m"] = timed(lambda: ctx.decode_ranges_device(model, comp, d_lens, bs, n, big, d_out), a.runs)
        assert d_out.cpu().numpy().tobytes() == host[big[0, 0]:big[0, 0] + (64 << 20)].tobytes()
        d_back = torch.empty(n, dtype=torch.uint8, device="cuda")
        row["full_decode"] = timed(lambda: ctx.decode_blocks_device(model, comp, d_lens, bs, n, d_back), a.runs)
        row["full_decode"]["mib_s"] = round(n / 2**20 / (row["full_decode"]["median_ms"] / 1e3), 1)
        del d_back
        if not a.no_host:   # the host variant from pinned memory: only the selected streams cross PCIe
            h_comp = torch.empty(total, dtype=torch.uint8).pin_memory()
            h_comp.copy_(comp.cpu())
            hc = h_comp.numpy()
            lens = d_lens.cpu().numpy().view(np.uint32).copy()

            def hst(k):
                return lambda: ctx.decode_ranges(model, hc, lens, bs, n, rand_ranges(k))

            got = ctx.decode_ranges(model, hc, lens, bs, n, r0)
            assert got.tobytes() == b"".join(host[o:o + k].tobytes() for o, k in r0.tolist())
            row["host_one_4k"] = timed(hst(1), a.runs)
            for k in (64, 1024, 4096):
                row["host_batch_%d_x_4k" % k] = timed(hst(k), a.runs)
            row["host_one_64m"] = timed(lambda: ctx.decode_ranges(model, hc, lens, bs, n, big), a.runs)
            del h_comp
        res["block_sizes"][str(bs)] = row
        print(json.dumps({str(bs): row}), flush=True)
        del d_comp, d_lens, d_out
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
