#!/usr/bin/env python3
"""Natural-neighbour (discrete Sibson) void fill throughput (csrc/natural.hip, mvp_gan/src/natural.py) on
the 8192^2 scenes of tools/idw_bench.py (disc holes of 30 % and 2 %, and "tiles": six missing 1024 x 1024 tiles) at radius 8, 16
and 32.  Times with device events, 3 calls after 1 warm-up: the parts on ready tensors (the feature transform, the gather, the
tile maxima alone, tg_natural_fill whole; the fill kernel is the difference of the last two) and the complete
natural_neighbour_voids call, per radius; ns_per_void_px_* is the fill kernel's time over the void pixels.  Beside them the same
call of interpolate_voids, krige_voids and fill_voids on the same scene in the same run, for scale, and the histogram of the
void depths (distance_to_known, in pixels) that explains how the times of the scenes relate: the kernel's work per void pixel
grows with the square of the depth around it, up to the radius.  One JSON line per scene, printed and written to --out.

    python tools/natural_bench.py [--size 8192] [--scenes 0.3 0.02 tiles] [--radii 8 16 32] [--reps 3] [--warmup 1]
                                  [--no-fill-voids] [--out profiles/natural_8192.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "terra-gan_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEPTH_EDGES_PX = (1, 2, 4, 8, 16, 32)                    # classes [1, 2), [2, 4), .. [32, inf) of the void pixels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--scenes", nargs="+", default=["0.3", "0.02", "tiles"], help="shares of disc holes, or 'tiles'")
    ap.add_argument("--radii", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-fill-voids", action="store_true", help="skip the fill_voids timing of the same scene")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "natural_8192.jsonl"))
    a = ap.parse_args()
    H = W = a.size
    if not torch.cuda.is_available():
        sys.exit("natural_bench: needs an MI355X (no CPU timing)")
    from fill_voids_bench import scene
    from mvp_gan.src import raster_args as R
    from mvp_gan.src.distance import distance_to_known
    from mvp_gan.src.fill_voids import fill_voids
    from mvp_gan.src.interpolate import interpolate_voids
    from mvp_gan.src.kriging import krige_voids
    from mvp_gan.src.natural import natural_neighbour_voids
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

    lines = []
    for name in a.scenes:
        z, keep = scene(H, W, name)
        zd, kd = torch.from_numpy(z).to(dev), torch.from_numpy(keep).to(dev)
        zt, known = R.upload_known(zd, kd, None, "natural_bench")
        void = int((known == 0).sum().item())
        res = {"what": "natural", "H": H, "W": W, "scene": name, "void_px": void, "reps": a.reps, "warmup": a.warmup}
        dist, dinfo = distance_to_known(zd, kd)
        depth = dist[known == 0]
        edges = torch.tensor(DEPTH_EDGES_PX + (float("inf"),), dtype=torch.float32, device=dev)
        hist = [int(((depth >= lo) & (depth < hi)).sum().item()) for lo, hi in zip(edges[:-1], edges[1:])]
        res.update(depth_edges_px=list(DEPTH_EDGES_PX), depth_hist=hist, max_depth_px=round(float(depth.max().item()), 2),
                   mean_depth2_px2=round(float((depth.double() ** 2).mean().item()), 2))
        ms, (d2, idx) = timed(lambda: O.edt_nearest(known, 0))
        res.update(ms_transform=round(ms, 3))
        ms, (nn, _) = timed(lambda: O.gather_fill(zt, known, idx))
        res.update(ms_gather=round(ms, 3))
        for r in a.radii:
            ms_max, _ = timed(lambda: O.natural_tile_maxima(d2, r))
            ms_all, (_, counts, sup) = timed(lambda: O.natural_fill(nn, d2, known, r, 0, want_support=True))
            ms_kernel = ms_all - ms_max
            ms_call, (_, info) = timed(lambda: natural_neighbour_voids(zd, kd, radius=r))
            res.update({f"ms_tile_maxima_r{r}": round(ms_max, 3), f"ms_natural_fill_r{r}": round(ms_all, 3),
                        f"ms_fill_kernel_r{r}": round(ms_kernel, 3),
                        f"ns_per_void_px_r{r}": round(ms_kernel * 1e6 / max(void, 1), 3),
                        f"ms_natural_neighbour_voids_r{r}": round(ms_call, 3), f"max_support_r{r}": info["max_support"],
                        f"mean_support_r{r}": round(float(sup.sum().item()) / max(void, 1), 2),
                        f"unfilled_r{r}": info["unfilled"]})
        ms, _ = timed(lambda: interpolate_voids(zd, kd))
        res.update(ms_idw=round(ms, 3))
        ms, _ = timed(lambda: krige_voids(zd, kd))
        res.update(ms_krige_voids=round(ms, 3))
        if not a.no_fill_voids:
            solver = "pcg" if name == "tiles" else "mg"
            ms, (_, finfo) = timed(lambda: fill_voids(zd, kd, solver=solver))
            res.update(ms_fill_voids=round(ms, 3), fill_voids_solver=solver, fill_voids_cycles=finfo["cycles"])
        lines.append(res)
        print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
