#!/usr/bin/env python3
"""Whole-raster inpainting throughput (mvp_gan/src/inpaint_raster.py) on a synthetic DSM: 8192^2 by default, about 30 %
holes in discs, window 512, overlap 64, batch 16.  Times complete inpaint_raster calls with device events after warm-up
and prints one JSON line: Mpx/s, windows/s, and the algorithmic bytes each raster kernel moves (divide them by the
kernel times of a separate `rocprofv3 --kernel-trace --stats` run for achieved GB/s).

    python tools/raster_bench.py [--size 8192] [--reps 3] [--warmup 1] [--tta 2|4|8]
    python tools/raster_bench.py --tta 8 --kernels    # the three augmentation kernels alone: ms and GB/s, plain and transposing
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


def time_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def tta_kernels(zd, md, plan, tta, reps):
    """ms and algorithmic GB/s of tg_raster_gather_ops, tg_raster_tta_reduce and tg_raster_blend_tta on the bench raster: every
    window runs; the gather and the reduce once with plain members only (ops 0..3) and once with transposing ones (4..7)."""
    from tg_hip import ops as O
    dev = zd.device
    cp = O.raster_plan(plan.H, plan.W, plan.wh, plan.ww, plan.overlap, len(plan.ys), len(plan.xs))
    nwin, npx = len(plan.ys) * len(plan.xs), plan.wh * plan.ww
    lo, hi, _ = O.raster_window_stats(zd, md, cp)
    n = min(nwin, 256)
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    x, m = torch.empty(n, plan.wh, plan.ww, device=dev), torch.empty(n, plan.wh, plan.ww, device=dev)
    res = {}
    kinds = (("plain", (0, 1, 2, 3)), ("transposing", (4, 5, 6, 7))) if plan.wh == plan.ww else (("plain", (0, 1, 2, 3)),)
    for kind, ops in kinds:
        op_idx = np.resize(np.array(ops, np.int32), n)
        ms = time_ms(lambda: O.raster_gather_ops(zd, md, cp, lo, hi, idx, op_idx, x=x, m=m), reps)
        res[f"gather_ops_{kind}"] = {"ms": round(ms, 4), "GB_per_s": round(n * npx * 16 / ms / 1e6, 1), "items": n}
    T = min(tta, 4)
    nr = max(1, n // T)
    gout = x[:nr * T].view(nr, T, plan.wh, plan.ww)
    mean, var = torch.empty(nr, plan.wh, plan.ww, device=dev), torch.empty(nr, plan.wh, plan.ww, device=dev)
    for kind, ops in kinds:
        ms = time_ms(lambda: O.raster_tta_reduce(gout, np.array(ops[:T], np.int32), mean=mean, var=var), reps)
        res[f"tta_reduce_{kind}"] = {"ms": round(ms, 4), "GB_per_s": round(nr * npx * (T + 2) * 4 / ms / 1e6, 1), "windows": nr, "T": T}
    if tta == 8 and plan.wh == plan.ww:
        nr8 = max(1, n // 8)
        g8 = x[:nr8 * 8].view(nr8, 8, plan.wh, plan.ww)
        ms = time_ms(lambda: O.raster_tta_reduce(g8, np.arange(8, dtype=np.int32), mean=mean[:nr8], var=var[:nr8]), reps)
        res["tta_reduce_all8"] = {"ms": round(ms, 4), "GB_per_s": round(nr8 * npx * 10 * 4 / ms / 1e6, 1), "windows": nr8, "T": 8}
    run_of = torch.arange(nwin, dtype=torch.int32, device=dev)
    wmean = torch.rand(nwin, plan.wh, plan.ww, device=dev)
    wvar = torch.rand(nwin, plan.wh, plan.ww, device=dev) * 0.01
    hole = (md == 0)
    cover = torch.zeros(plan.H, plan.W, dtype=torch.int32, device=dev)
    for y0 in plan.ys:
        for x0 in plan.xs:
            cover[y0:y0 + plan.wh, x0:x0 + plan.ww] += 1
    holes, cover_reads = int(hole.sum().item()), int(cover[hole].sum().item())
    for name, fn, nbytes in (("blend_tta", lambda: O.raster_blend_tta(zd, md, cp, lo, hi, run_of, wmean, wvar),
                              plan.H * plan.W * (8 + 8) + holes * 8 + cover_reads * 8),
                             ("blend", lambda: O.raster_blend(zd, md, cp, lo, hi, run_of, wmean),
                              plan.H * plan.W * (8 + 4) + holes * 8 + cover_reads * 4)):
        ms = time_ms(fn, reps)
        res[name] = {"ms": round(ms, 4), "GB_per_s": round(nbytes / ms / 1e6, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--holes", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tta", type=int, choices=(1, 2, 4, 8), default=1, help="test-time augmentation members of every call")
    ap.add_argument("--kernels", action="store_true",
                    help="with --tta above 1: time the three augmentation kernels alone (device events) instead of whole calls")
    ap.add_argument("--kstats", help="rocprofv3 kernel_stats.csv of a run of this tool: adds per-kernel GB/s and shares")
    a = ap.parse_args()
    from mvp_gan.src.inpaint_raster import inpaint_raster, plan_windows
    H = W = a.size
    z, mask = synth(H, W, a.holes, 0)
    plan = plan_windows(H, W, a.window, a.overlap)
    hole = mask == 0
    res = {"what": "inpaint_raster", "H": H, "W": W, "window": a.window, "overlap": a.overlap, "batch": a.batch,
           "hole_frac": round(float(hole.mean()), 4)}
    if a.tta != 1:
        res["tta"] = a.tta
    if a.kernels and a.tta == 1:
        ap.error("--kernels needs --tta above 1")
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
    if a.kernels:
        res.update(what="inpaint_raster tta kernels", kernels=tta_kernels(zd, md, plan, a.tta, max(a.reps, 5)))
        print(json.dumps(res))
        return
    kw = {} if a.tta == 1 else {"tta": a.tta}
    for _ in range(a.warmup):
        out, info = inpaint_raster(G, zd, md, window=a.window, overlap=a.overlap, batch=a.batch, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        out, info = inpaint_raster(G, zd, md, window=a.window, overlap=a.overlap, batch=a.batch, **kw)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    res.update(windows=info["windows"], run=info["run"], unfilled=info["unfilled"], ms_per_raster=round(ms, 3),
               mpx_per_s=round(H * W / ms / 1e3, 2), windows_per_s=round(info["run"] / ms * 1e3, 2), reps=a.reps,
               warmup=a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
