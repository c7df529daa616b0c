#!/usr/bin/env python3
"""Exact Euclidean distance transform throughput (csrc/edt.hip, mvp_gan/src/distance.py) on the 8192^2
scenes of tools/fill_voids_bench.py (disc holes of 30 % and 2 %, and "tiles": six missing 1024 x 1024 tiles, depth 512 px).
The seeds are the known pixels of the scene.  Times tg_edt (ops.edt, with dist_m) uncapped and at the default evaluation cap
(the last of evaluate_raster.DEPTH_EDGES_M, 50 m at 1 m cells) with device events after warm-up, and prints one JSON line per
scene: ms per call, GB/s against the algorithmic bytes (1 B seed read, 2 B column distance written and read, 4 B d2 written,
4 B dist_m written = 13 B per pixel) and the share of the HBM floor at --hbm-tbs (6.3 TB/s, the rate tools/resample_bench.py
measured).  Then, on the scene of tools/evaluate_raster_bench.py, terrain_errors with and without depth_edges_m.

    python tools/edt_bench.py [--size 8192] [--scenes 0.3 0.02 tiles] [--reps 3] [--warmup 1] [--no-terrain] [--empty [--empty-uncapped]]
    rocprofv3 --kernel-trace --stats -d prof -o p --output-format csv -- python tools/edt_bench.py --scenes tiles --no-terrain
    python tools/edt_bench.py --kstats prof/.../p_kernel_stats.csv --calls 8          # host only: per-kernel us and GB/s
(--calls: tg_edt calls of the profiled run, (reps + warmup) x 2 per scene; --empty adds the worst case, one seed in a corner,
at the cap; --empty-uncapped also without one, where the search is O(side) per pixel: run that at a smaller --size first)
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "terra-gan_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

BAND = 64


def kernel_bytes(H, W):
    """Bytes per tg_edt call each kernel must move at least."""
    n, nbw = H * W, -(-H // BAND) * W
    return {"edt_mask_kernel": n + nbw * 8, "edt_carry_kernel": nbw * (2 * 8 + 2 * 4), "edt_g_kernel": nbw * 16 + n * 2,
            "edt_row_kernel": n * (2 + 4 + 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--scenes", nargs="+", default=["0.3", "0.02", "tiles"], help="shares of disc holes, 'tiles', or 'none' alone")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="the measured HBM rate the floor is taken at")
    ap.add_argument("--no-terrain", action="store_true", help="skip the terrain_errors timing")
    ap.add_argument("--empty", action="store_true", help="also time a raster with a single seed, at the cap")
    ap.add_argument("--empty-uncapped", action="store_true", help="with --empty: also without a cap (O(side) per pixel)")
    ap.add_argument("--kstats", help="rocprofv3 kernel_stats.csv of a run of this tool: per-kernel us and GB/s")
    ap.add_argument("--calls", type=int, default=0, help="with --kstats: tg_edt calls of the profiled run")
    a = ap.parse_args()
    H = W = a.size
    if a.kstats:
        kb = kernel_bytes(H, W)
        rows = [r for r in csv.DictReader(open(a.kstats)) if "edt_" in r["Name"] or "depth_errors" in r["Name"]]
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        ks = {}
        for r in rows:
            name = r["Name"].split("(")[0].replace("void ", "")
            ns, calls = float(r["TotalDurationNs"]), int(r["Calls"])
            ent = {"us_per_launch": round(ns / calls / 1e3, 1), "launches": calls, "share": round(ns / tot, 4)}
            key = next((k for k in kb if k in name), None)
            if key:
                ent.update(bytes_per_launch=kb[key], GB_per_s=round(kb[key] * calls / ns, 1))
            ks[name] = ent
        print(json.dumps({"what": "edt kernels", "H": H, "W": W, "kernel_ms_per_call": round(tot / max(a.calls, 1) / 1e6, 3),
                          "kernels": ks}))
        return
    if not torch.cuda.is_available():
        sys.exit("edt_bench: needs an MI355X (no CPU timing)")
    from fill_voids_bench import scene
    from mvp_gan.src.distance import depth_px2
    from mvp_gan.src.evaluate_raster import DEPTH_EDGES_M, eval_holes, terrain_errors
    from tg_hip import ops as O
    dev = torch.device("cuda:0")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(a.warmup):
            out = fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps, out

    c = 1.0
    cap2 = depth_px2(DEPTH_EDGES_M[-1:], c)[0]
    nbytes = H * W * (1 + 2 + 2 + 4 + 4)
    floor_ms = nbytes / (a.hbm_tbs * 1e12) * 1e3

    def line(name, seed, caps):
        res = {"what": "edt", "H": H, "W": W, "scene": name, "unknown": int((seed == 0).sum().item()), "bytes": nbytes,
               "hbm_floor_ms": round(floor_ms, 4)}
        for tag, cp in caps:
            ms, (d2, _) = timed(lambda: O.edt(seed, cp, c))
            res.update({f"ms_{tag}": round(ms, 3), f"GB_per_s_{tag}": round(nbytes / ms / 1e6, 1),
                        f"of_floor_{tag}": round(floor_ms / ms, 4), f"max_d2_{tag}": int(d2.max().item())})
        res.update(cap2=cap2, reps=a.reps, warmup=a.warmup)
        print(json.dumps(res), flush=True)

    for name in (a.scenes if a.scenes != ["none"] else []):
        z, keep = scene(H, W, name)
        seed, _ = O.objmask_known(torch.from_numpy(z).to(dev), torch.from_numpy(keep).to(dev), None, transposed=False)
        line(name, seed, (("uncapped", 0), ("capped", cap2)))
    if a.empty:
        seed = torch.zeros(H, W, dtype=torch.uint8, device=dev)
        seed[0, 0] = 1
        line("one seed", seed, (("capped", cap2),) + ((("uncapped", 0),) if a.empty_uncapped else ()))
    if not a.no_terrain:
        from tests import objmask_oracle as OR
        z, _ = OR.scene(H, W, 0)
        zd = torch.from_numpy(z).to(dev)
        hm, keep, info = eval_holes(zd, split="test", block=1024, tile=256, seed=0)
        pred = zd + torch.randn(zd.shape, generator=torch.Generator(device=dev).manual_seed(0), device=dev) * hm
        ms0, rep0 = timed(lambda: terrain_errors(zd, pred, hm, keep, cellsize=c))
        ms1, rep1 = timed(lambda: terrain_errors(zd, pred, hm, keep, cellsize=c, depth_edges_m=DEPTH_EDGES_M))
        ms2, _ = timed(lambda: terrain_errors(zd, pred, hm, keep, cellsize=c))
        print(json.dumps({"what": "terrain_errors", "H": H, "W": W, "hole_px": info["holes"], "scored": rep0["pixels"]["scored"],
                          "ms_plain": round(ms0, 3), "ms_by_depth": round(ms1, 3), "ms_plain_again": round(ms2, 3),
                          "added_ms": round(ms1 - (ms0 + ms2) / 2, 3), "added_share": round(ms1 / ((ms0 + ms2) / 2) - 1, 4),
                          "by_depth_pixels": [k["pixels"] for k in rep1["by_depth"]["classes"]], "reps": a.reps,
                          "warmup": a.warmup}), flush=True)


if __name__ == "__main__":
    main()
