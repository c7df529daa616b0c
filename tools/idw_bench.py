#!/usr/bin/env python3
"""Feature transform, nearest-neighbour and eight-direction inverse-distance fill throughput (csrc/edt.hip, csrc/idw.hip,
mvp_gan/src/distance.py, mvp_gan/src/interpolate.py) on the 8192^2 scenes of tools/fill_voids_bench.py
(disc holes of 30 % and 2 %, and "tiles": six missing 1024 x 1024 tiles).  Times complete calls of nearest_known,
interpolate_voids(method="nearest"), interpolate_voids(method="idw") and the latter with smooth=3 with device events, 3 calls
after 1 warm-up, and prints one JSON line per scene: per call the ms, the GB/s against the algorithmic bytes below and the share
of the HBM floor at --hbm-tbs (6.3 TB/s, the rate tools/resample_bench.py measured), and beside them the fill_voids time of the
same scene in the same run (default solver; pcg for the tiles scene).

Algorithmic bytes per pixel (every array once; the gathers of the fills and the workspace words are not counted):
  known mask (tg_objmask_known)  4 dem + 4 mask + 1 known                                    =  9
  feature transform              1 seed + 2 + 2 column distance + 4 d2 + 4 idx               = 13
  nearest_known                  known + transform + 4 d2 in + 4 metres out                  = 30
  nearest fill                   known + transform + 4 dem + 1 known + 4 idx + 4 out         = 35
  idw fill                       known + 4 x 1 known (one per family of lines) + 1 word and carries + 1 known + 4 dem + 4 out = 23
  smooth step                    4 in + 1 known + 4 out                                      =  9 each

    python tools/idw_bench.py [--size 8192] [--scenes 0.3 0.02 tiles] [--reps 3] [--warmup 1] [--no-fill-voids]
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

BYTES_PER_PX = {"nearest_known": 30, "nearest": 35, "idw": 23, "idw_smooth3": 23 + 3 * 9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--scenes", nargs="+", default=["0.3", "0.02", "tiles"], help="shares of disc holes, or 'tiles'")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="the measured HBM rate the floor is taken at")
    ap.add_argument("--no-fill-voids", action="store_true", help="skip the fill_voids timing of the same scene")
    a = ap.parse_args()
    H = W = a.size
    if not torch.cuda.is_available():
        sys.exit("idw_bench: needs an MI355X (no CPU timing)")
    from fill_voids_bench import scene
    from mvp_gan.src.distance import nearest_known
    from mvp_gan.src.fill_voids import fill_voids
    from mvp_gan.src.interpolate import interpolate_voids
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

    for name in a.scenes:
        z, keep = scene(H, W, name)
        zd, kd = torch.from_numpy(z).to(dev), torch.from_numpy(keep).to(dev)
        calls = {"nearest_known": lambda: nearest_known(zd, kd)[2],
                 "nearest": lambda: interpolate_voids(zd, kd, method="nearest")[1],
                 "idw": lambda: interpolate_voids(zd, kd)[1],
                 "idw_smooth3": lambda: interpolate_voids(zd, kd, smooth=3)[1]}
        res = {"what": "idw", "H": H, "W": W, "scene": name, "reps": a.reps, "warmup": a.warmup}
        for tag, fn in calls.items():
            ms, info = timed(fn)
            nbytes = H * W * BYTES_PER_PX[tag]
            floor_ms = nbytes / (a.hbm_tbs * 1e12) * 1e3
            res.update({f"ms_{tag}": round(ms, 3), f"GB_per_s_{tag}": round(nbytes / ms / 1e6, 1),
                        f"of_floor_{tag}": round(floor_ms / ms, 4)})
            if tag == "nearest_known":
                res.update(unknown=info["unknown"], max_m=info["max_m"])
            else:
                res.update({f"unfilled_{tag}": info["unfilled"], f"by_nearest_{tag}": info["by_nearest"]})
        if not a.no_fill_voids:
            solver = "pcg" if name == "tiles" else "mg"
            ms, (_, finfo) = timed(lambda: fill_voids(zd, kd, solver=solver))
            res.update(ms_fill_voids=round(ms, 3), fill_voids_solver=solver, fill_voids_cycles=finfo["cycles"],
                       fill_voids_converged=finfo["converged"])
            for tag in ("nearest", "idw", "idw_smooth3"):
                res[f"fill_voids_over_{tag}"] = round(ms / res[f"ms_{tag}"], 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
