#!/usr/bin/env python3
"""Raster resampling throughput (mvp_gan/src/resample.py, csrc/resample.hip) on tools/raster_bench.py's synthetic 8192^2
terrain with its disc holes.  Times, with device events after warm-up: the area kernel at 2, 4 and 10/3, the interpolation
kernel at 1/2 and 3/10, the return trips from 2, 10/3, 1/2 and 3/10 with the native raster passed through, and the masked
average pooling one would otherwise write with torch on the same GPU at the factors 2 and 4 (avg_pool2d(z k), avg_pool2d(k),
a divide and a threshold), which is the yardstick of the area kernel.  GB/s are against algorithmic bytes: source values
and mask read once, outputs (value and mask) written once, the passed-through raster and its mask read once.  With --inpaint
also an inpaint_raster(model_cellsize=2 x cellsize) call with a random-weight generator and the share of it that the
resampling takes.  One process, one JSON line; a failing step raises and nothing runs after it.

    python tools/resample_bench.py [--size 8192] [--holes 0.3] [--reps 5] [--warmup 2] [--inpaint]
    rocprofv3 --kernel-trace --stats -d prof -o p --output-format csv -- python tools/resample_bench.py --no-torch
    python tools/resample_bench.py --kstats prof/.../p_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import sys
from fractions import Fraction

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "terra-gan_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

AREA = ("2/1", "4/1", "10/3")
INTERP = ("1/2", "3/10")
POOL = (2, 4)


def out_shape(H, W, s):
    return -(-H * s.denominator // s.numerator), -(-W * s.denominator // s.numerator)


def forward_bytes(H, W, s):
    Ho, Wo = out_shape(H, W, s)
    return H * W * 8 + Ho * Wo * 8                 # dem + mask in, value + mask out


def back_bytes(H, W, s):
    Ho, Wo = out_shape(H, W, s)
    return Ho * Wo * 4 + H * W * (8 + 8)           # the working raster in; native dem + mask in, value + mask out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--holes", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch pooling baseline (for a profiled run)")
    ap.add_argument("--inpaint", action="store_true", help="also time inpaint_raster(model_cellsize=...) and the resampling's share")
    ap.add_argument("--kstats", help="rocprofv3 kernel_stats.csv of a run of this tool: per-kernel us")
    a = ap.parse_args()
    H = W = a.size
    if a.kstats:
        rows = list(csv.DictReader(open(a.kstats)))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        ks = {}
        for r in rows:
            name = r["Name"].split("(")[0].replace("void ", "")
            ns = float(r["TotalDurationNs"])
            ks[name] = {"us_total": round(ns / 1e3, 1), "launches": int(r["Calls"]),
                        "us_per_launch": round(ns / 1e3 / int(r["Calls"]), 1), "share": round(ns / tot, 4)}
        print(json.dumps({"what": "resample kernels", "H": H, "W": W, "kernel_ms": round(tot / 1e6, 3), "kernels": ks}))
        return
    if not torch.cuda.is_available():
        sys.exit("resample_bench: needs an MI355X (no CPU timing)")
    from mvp_gan.src.resample import resample_back, resample_to
    from raster_bench import synth
    dev = torch.device("cuda:0")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, reps):
        for _ in range(a.warmup):
            out = fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, out

    def entry(ms, nbytes, extra=None):
        d = {"ms": round(ms, 4), "GB_per_s": round(nbytes / ms / 1e6, 1), "MB": round(nbytes / 1e6, 1)}
        d.update(extra or {})
        return d

    z, keep = synth(H, W, a.holes, 0)
    zd, kd = torch.from_numpy(z).to(dev), torch.from_numpy(keep).to(dev)
    res = {"what": "resample", "H": H, "W": W, "holes": a.holes, "reps": a.reps, "warmup": a.warmup, "forward": {}, "back": {}}
    for name in AREA + INTERP:
        s = Fraction(name)
        ms, (work, _, n_nan) = timed(lambda: resample_to(zd, kd, None, s, 0.5), a.reps)
        res["forward"][name] = entry(ms, forward_bytes(H, W, s), {"shape": list(work.shape), "unknown": int(n_nan.item())})
        if name != "4/1":
            ms, (_, n_nan) = timed(lambda: resample_back(work, zd, kd, scale=s), a.reps)
            res["back"][name] = entry(ms, back_bytes(H, W, s), {"unfilled": int(n_nan.item())})
        del work
    if not a.no_torch:
        import torch.nn.functional as F
        nan = torch.tensor(float("nan"), device=dev)

        def pooled(f):
            s = F.avg_pool2d((zd * kd)[None, None], f, ceil_mode=True)
            c = F.avg_pool2d(kd[None, None], f, ceil_mode=True)
            kn = c >= 0.5
            return torch.where(kn, s / c, nan)[0, 0], kn.to(torch.float32)[0, 0]

        res["torch_pool"] = {}
        for f in POOL:
            ms, _ = timed(lambda: pooled(f), a.reps)
            ours = res["forward"][f"{f}/1"]["ms"]
            res["torch_pool"][f"{f}/1"] = entry(ms, forward_bytes(H, W, Fraction(f)), {"area_kernel_ms": ours,
                                                                                         "speedup": round(ms / ours, 2)})
    if a.inpaint:
        from mvp_gan.src.inpaint_raster import inpaint_raster
        from mvp_gan.src.models import PConvUNet
        from tg_hip import ops as O
        torch.manual_seed(0)
        G = PConvUNet().to(dev)
        ms_t, (_, info) = timed(lambda: inpaint_raster(G, zd, kd, cellsize=0.5, model_cellsize=1.0), 1)
        ms_c, _ = timed(lambda: O.raster_count_unknown(zd, kd, None), a.reps)          # the native hole count
        ms_r = res["forward"]["2/1"]["ms"] + res["back"]["2/1"]["ms"] + ms_c
        res["inpaint"] = {"ms": round(ms_t, 2), "resample_ms": round(ms_r, 3), "resample_share": round(ms_r / ms_t, 5),
                          "windows": info["windows"], "run": info["run"], "unfilled": info["unfilled"],
                          "resample": info["resample"]}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
