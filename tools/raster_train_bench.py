#!/usr/bin/env python3
"""Cost of feeding train_step from a whole raster (mvp_gan/src/utils/raster_dataset.py).  On an 8192^2 synthetic DSM (metres)
it times train_step at 256^2 / B = 16 fed by RasterWindowLoader against the same loop fed from four fixed device batches
(the loader's own first four, so both see the same kind of data), alternating the two, with device events after warm-up.
It also times the loader alone and its host draws, and prints one JSON line.  The kernels' share of kernel time comes from a
separate profiler run:

    python tools/raster_train_bench.py [--size 8192] [--steps 40] [--reps 3]
    rocprofv3 --kernel-trace --stats -d prof -o p --output-format csv -- python tools/raster_train_bench.py --steps 20 --reps 1
    python tools/raster_train_bench.py --kstats prof/.../p_kernel_stats.csv      # host only: per-batch us, share, GB/s
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "terra-gan_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

KERNELS = ("hole_mask_kernel", "sample_init_kernel", "sample_minmax_kernel", "sample_norm_kernel")


def batch_bytes(B, w):
    """Algorithmic bytes per batch: the mask written, the window and mask read for min / max, the window read and x
    written for the normalising pass (draws and lo / hi are negligible)."""
    px = B * w * w * 4
    return {"hole_mask_kernel": px, "sample_minmax_kernel": 2 * px, "sample_norm_kernel": 2 * px}


def kstats(path, B, w):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {}
    nb = None
    for r in rows:
        name = r["Name"].split("(")[0].split("<")[0].strip()
        name = name.split(" ")[-1]
        if name in KERNELS:
            calls, ns = int(r["Calls"]), float(r["TotalDurationNs"])
            nb = calls if name == "hole_mask_kernel" else nb
            out[name] = {"calls": calls, "us_per_call": ns / calls / 1e3, "share_pct": 100 * ns / total}
    for name, by in batch_bytes(B, w).items():
        if name in out:
            out[name]["GB_per_s"] = by / (out[name]["us_per_call"] * 1e3)
    us = sum(v["us_per_call"] for v in out.values())
    return {"kernels": out, "us_per_batch": us, "share_pct": sum(v["share_pct"] for v in out.values()),
            "GB_per_s_per_batch": sum(batch_bytes(B, w).values()) / (us * 1e3) if us else None, "batches": nb}


def terrain(H, W, seed):
    """Smooth separable terrain in metres, built row block by row block (an 8192^2 float64 grid would be 512 MB)."""
    rng = np.random.default_rng(seed)
    y, x = np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32)
    z = np.full((H, W), 900, np.float32)
    for _ in range(6):
        fy, fx, ph = rng.uniform(0.0005, 0.01), rng.uniform(0.0005, 0.01), rng.uniform(0, 6.3)
        z += (np.float32(rng.uniform(30, 120)) * np.sin(fy * y + ph))[:, None] * np.cos(fx * x - ph)[None, :]
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kstats", help="rocprofv3 kernel_stats.csv to summarise (no GPU needed)")
    a = ap.parse_args()
    if a.kstats:
        print(json.dumps(kstats(a.kstats, a.batch, a.window)))
        return
    import torch
    os.environ.setdefault("TERRAGAN_ALLOW_STANDIN_VGG", "1")
    if not torch.cuda.is_available():
        raise SystemExit("raster_train_bench: needs a GPU")
    from mvp_gan.src.models import Discriminator, PConvUNet
    from mvp_gan.src.train import train_step
    from mvp_gan.src.utils.losses import InpaintingLoss
    from mvp_gan.src.utils.raster_dataset import RasterWindowLoader
    dev = torch.device("cuda:0")
    z = terrain(a.size, a.size, 0)
    t0 = time.perf_counter()
    L = RasterWindowLoader(z, window=a.window, batch_size=a.batch, steps_per_epoch=a.steps, split="train", seed=0, device=dev)
    t_init = time.perf_counter() - t0
    torch.manual_seed(0)
    G, D = PConvUNet().to(dev), Discriminator().to(dev)
    crit = InpaintingLoss(0.1, 0.1, device=torch.device("cpu")).to(dev)
    oG, oD = torch.optim.Adam(G.parameters(), lr=2e-4), torch.optim.Adam(D.parameters(), lr=2e-4)
    G.train(), D.train()
    fixed = []
    for b in L:
        fixed.append((b["image"].clone(), b["mask"].clone()))
        if len(fixed) == 4:
            break

    def run_fixed(k):
        for i in range(k):
            train_step(G, D, crit, oG, oD, *fixed[i % 4])

    def run_raster(k, epoch):
        L.steps_per_epoch = k
        L.set_epoch(epoch)
        for b in L:
            train_step(G, D, crit, oG, oD, b["image"], b["mask"])

    def run_loader(k, epoch):
        L.steps_per_epoch = k
        L.set_epoch(epoch)
        for b in L:
            pass

    def timed(fn, *args):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(*args)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    run_fixed(a.warmup)
    run_raster(a.warmup, 1000)
    run_loader(a.warmup, 1001)
    fx, rs, ld = [], [], []
    for r in range(a.reps):
        fx.append(timed(run_fixed, a.steps))
        rs.append(timed(run_raster, a.steps, r + 1))
        ld.append(timed(run_loader, a.steps, 100 + r))
    t0 = time.perf_counter()
    for b in range(50):
        L.draw(b)
    t_draw = (time.perf_counter() - t0) / 50 * 1e3
    mf, mr = float(np.median(fx)), float(np.median(rs))
    print(json.dumps({"size": a.size, "window": a.window, "batch": a.batch, "steps": a.steps, "reps": a.reps,
                      "ms_per_step_fixed": mf, "ms_per_step_raster": mr, "overhead_pct": 100 * (mr - mf) / mf,
                      "ms_per_step_fixed_all": fx, "ms_per_step_raster_all": rs, "ms_per_batch_loader_only": float(np.median(ld)),
                      "ms_host_draw_per_batch": t_draw, "s_loader_init": t_init,
                      "admissible_fraction": L.info["admissible_fraction"],
                      "bytes_per_batch": sum(batch_bytes(a.batch, a.window).values())}))


if __name__ == "__main__":
    main()
