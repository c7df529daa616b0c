#!/usr/bin/env python3
"""Depression fill throughput (mvp_gan/src/fill_depressions.py, csrc/depfill.hip) on the 8192^2 scenes of
tools/fill_voids_bench.py (disc holes of 30 % and 2 %, six missing tiles), their voids filled first with interpolate_voids so
that the raster is complete and the only outlets are on its edge, plus the scene "basins": the same terrain without voids and
with 2000 synthetic closed basins dug into it.  Prints one JSON line per scene: ms per fill_depressions call and per relax()
(the sweeps alone, with their host syncs) by device events, the sweeps, tile visits, raised pixels and depressions, GB/s of the
sweeps against the algorithmic bytes of a tile visit, and in the same run ms per fill_voids call on the same scene, for scale.

    python tools/fill_depressions_bench.py [--size 8192] [--scenes 0.3 0.02 tiles basins] [--reps 3] [--warmup 1]
        [--connectivity 8] [--check-every 8]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "terra-gan_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

TILE = 64
# One tile visit: z (4 B), known (1 B) and W (4 B) of its 64 x 64 pixels and W of the 260 halo pixels in, W of the tile out.
# The write-back happens only when the visit lowered a value, so this is the most a visit moves.
VISIT_BYTES = TILE * TILE * (4 + 1 + 4 + 4) + (4 * TILE + 4) * 4
BASINS = 2000


def basins(z, n, seed):
    """Dig n round closed basins (radius 3..24 px, 0.5..6 m deep at the centre) into z."""
    rng = np.random.default_rng(seed)
    H, W = z.shape
    out = z.copy()
    for _ in range(n):
        r = int(rng.integers(3, 25))
        cy, cx = int(rng.integers(r, H - r)), int(rng.integers(r, W - r))
        y, x = np.mgrid[-r:r + 1, -r:r + 1]
        d = np.clip(1.0 - np.hypot(y, x) / r, 0.0, None) * rng.uniform(0.5, 6.0)
        out[cy - r:cy + r + 1, cx - r:cx + r + 1] -= d.astype(np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--scenes", nargs="+", default=["0.3", "0.02", "tiles", "basins"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--connectivity", type=int, choices=(8, 4), default=8)
    ap.add_argument("--check-every", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fill_depressions_bench: needs an MI355X (no CPU timing)")
    from fill_voids_bench import scene
    from mvp_gan.src.fill_depressions import fill_depressions, relax
    from mvp_gan.src.fill_voids import fill_voids
    from mvp_gan.src.interpolate import interpolate_voids
    H = W = a.size
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
        if name == "basins":
            z, keep = scene(H, W, "0.0")
            z, keep = basins(z, BASINS, 1), np.ones_like(keep)
        else:
            z, keep = scene(H, W, name)
        zd, kd = torch.from_numpy(z).to(dev), torch.from_numpy(keep).to(dev)
        ms_fv = None
        if name != "basins":
            ms_fv, _ = timed(lambda: fill_voids(zd, kd))
            full, finfo = interpolate_voids(zd, kd)
            assert finfo["unfilled"] == 0
        else:
            full = zd
        known = torch.ones(H, W, dtype=torch.uint8, device=dev)
        ms, (out, info) = timed(lambda: fill_depressions(full, connectivity=a.connectivity, check_every=a.check_every))
        ms_rx, rx = timed(lambda: relax(full, known, a.connectivity, check_every=a.check_every))
        print(json.dumps({"what": "fill_depressions", "H": H, "W": W, "scene": name, "connectivity": a.connectivity,
                          "check_every": a.check_every, "ms_per_call": round(ms, 3), "ms_sweeps": round(ms_rx, 3),
                          "sweeps": info["sweeps"], "tile_visits": info["tile_visits"], "tiles": (H // TILE) * (W // TILE),
                          "raised": info["raised"], "depressions": info["depressions"], "volume_m3": info["volume_m3"],
                          "max_depth_m": info["max_depth_m"], "converged": info["converged"], "visit_bytes": VISIT_BYTES,
                          "sweeps_GB_per_s": round(rx[3] * VISIT_BYTES / (ms_rx * 1e6), 1),
                          "fill_voids_ms_per_call": None if ms_fv is None else round(ms_fv, 3), "reps": a.reps,
                          "warmup": a.warmup}), flush=True)


if __name__ == "__main__":
    main()
