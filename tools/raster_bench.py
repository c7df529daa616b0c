#!/usr/bin/env python3
"""Whole-raster inpainting throughput (mvp_gan/src/inpaint_raster.py) on a synthetic DSM: 8192^2 by default, about 30 %
holes in discs, window 512, overlap 64, batch 16.  Times complete inpaint_raster calls with device events after warm-up
and prints one JSON line: Mpx/s, windows/s, and the algorithmic bytes each raster kernel moves (divide them by the
kernel times of a separate `rocprofv3 --kernel-trace --stats` run for achieved GB/s).

    python tools/raster_bench.py [--size 8192] [--reps 3] [--warmup 1]
    rocprofv3 --kernel-trace --stats -d prof -o p --output-format csv -- python tools/raster_bench.py
    python tools/raster_bench.py --kstats prof/.../p_kernel_stats.csv     # host only: per-kernel us, share, GB/s
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "terra-gan_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def synth(H, W, hole_frac, seed):
    """Smooth terrain (separable sines, metres) and a keep-mask with random disc holes."""
    rng = np.random.default_rng(seed)
    y, x = np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64)
    z = np.zeros((H, W), np.float32)
    for _ in range(6):
        fy, fx, ph = rng.uniform(0.0005, 0.01), rng.uniform(0.0005, 0.01), rng.uniform(0, 6.3)
        z += (rng.uniform(30, 120) * np.sin(fy * y + ph))[:, None].astype(np.float32) * np.cos(fx * x - ph)[None, :].astype(np.float32)
    z += np.float32(900)
    hole = np.zeros((H, W), bool)
    while hole.mean() < hole_frac:
        for _ in range(64):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(24, 160)
            y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
            yy, xx = np.ogrid[y0:y1, x0:x1]
            hole[y0:y1, x0:x1] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return z, (~hole).astype(np.float32)


def kernel_bytes(plan, n_run, holes, cover_reads):
    """Bytes each kernel must move at least (fp32 dem + mask reads, fp32 writes)."""
    npx = plan.wh * plan.ww
    nwin = len(plan.ys) * len(plan.xs)
    return {
        "raster_stats_kernel": nwin * npx * 8,                        # dem + mask of every window
        "raster_gather_kernel": n_run * npx * (8 + 8),                # dem + mask in, x + m out
        "raster_blend_kernel": plan.H * plan.W * (8 + 4) + holes * 8 + cover_reads * 4,   # dem + mask in, raster out,
    }                                                                 # lo/hi per hole, window outputs per covering window


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--holes", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kstats", help="rocprofv3 kernel_stats.csv of a run of this tool: adds per-kernel GB/s and shares")
    a = ap.parse_args()
    from mvp_gan.src.inpaint_raster import inpaint_raster, plan_windows
    H = W = a.size
    z, mask = synth(H, W, a.holes, 0)
    plan = plan_windows(H, W, a.window, a.overlap)
    hole = mask == 0
    res = {"what": "inpaint_raster", "H": H, "W": W, "window": a.window, "overlap": a.overlap, "batch": a.batch,
           "hole_frac": round(float(hole.mean()), 4)}
    if a.kstats:
        # host only: the bytes of each kernel (holes and, per hole, the covering windows that ran) over its profiled time
        from tests import raster_oracle as RO
        _, _, cnt = RO.stats(z, plan, mask)
        ran = (cnt[:, 0] > 0) & (cnt[:, 1] > 0)
        cover = np.zeros((H, W), np.int8)
        for j, (y0, x0) in enumerate(RO.windows(plan)):
            if ran[j]:
                cover[y0:y0 + plan.wh, x0:x0 + plan.ww] += 1
        kb = kernel_bytes(plan, int(ran.sum()), int(hole.sum()), int(cover[hole].sum()))
        rows = list(csv.DictReader(open(a.kstats)))
        calls = a.reps + a.warmup                 # inpaint_raster calls of the profiled run
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        ks = {}
        for name, nbytes in kb.items():
            rs = [r for r in rows if r["Name"].startswith(name)]
            if rs:
                ns = sum(float(r["TotalDurationNs"]) for r in rs)
                ks[name] = {"us_per_raster": round(ns / calls / 1e3, 1), "share": round(ns / tot, 4),
                            "GB_per_s": round(nbytes * calls / ns, 1), "bytes_per_raster": nbytes}
        res.update(windows=len(ran), run=int(ran.sum()), kernel_ms_per_raster=round(tot / calls / 1e6, 3), kernels=ks,
                   raster_kernels_share=round(sum(v["share"] for v in ks.values()), 4))
        print(json.dumps(res))
        return
    if not torch.cuda.is_available():
        sys.exit("raster_bench: needs an MI355X (no CPU timing)")
    from mvp_gan.src.models import PConvUNet
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    G = PConvUNet().to(dev)
    zd, md = torch.from_numpy(z).to(dev), torch.from_numpy(mask).to(dev)
    for _ in range(a.warmup):
        out, info = inpaint_raster(G, zd, md, window=a.window, overlap=a.overlap, batch=a.batch)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        out, info = inpaint_raster(G, zd, md, window=a.window, overlap=a.overlap, batch=a.batch)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    res.update(windows=info["windows"], run=info["run"], unfilled=info["unfilled"], ms_per_raster=round(ms, 3),
               mpx_per_s=round(H * W / ms / 1e3, 2), windows_per_s=round(info["run"] / ms * 1e3, 2), reps=a.reps,
               warmup=a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
