#!/usr/bin/env python3
"""MFD accumulation, slope and wetness throughput (mvp_gan/src/flow_routing.py, csrc/mfd.hip) on the 8192^2
scenes of tools/fill_depressions_bench.py (disc holes of 30 % and 2 %, six missing tiles, their voids filled first with
interpolate_voids; "basins": the same terrain without voids and with 2000 closed basins dug into it).  Every scene is routed once
(route_known, timed for scale); on that routing it prints one JSON line: ms of the setup pass, of the sweeps (with their host
syncs) and of the finish pass by device events, the sweeps and tile visits, GB/s of the sweep kernel against the algorithmic bytes
of a tile visit, and ms of the slope and wetness kernels.

    python tools/mfd_bench.py [--size 8192] [--scenes 0.3 0.02 tiles basins] [--exponent 1] [--reps 3] [--warmup 1]
        [--check-every 8]
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

TILE = 64
# One tile visit: A (8 B), S (8 B) and w (4 B) of the 66 x 66 pixels with the halo and the donor bytes of the 64 x 64 in; out, at
# most, A of the tile (only the pixels the visit made final are written).
VISIT_BYTES = (TILE + 2) * (TILE + 2) * (8 + 8 + 4) + TILE * TILE * (1 + 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--scenes", nargs="+", default=["0.3", "0.02", "tiles", "basins"])
    ap.add_argument("--exponent", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check-every", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mfd_bench: needs an MI355X (no CPU timing)")
    from fill_depressions_bench import BASINS, basins
    from fill_voids_bench import scene
    from mvp_gan.src.flow_routing import mfd_sweeps, route_known
    from mvp_gan.src.interpolate import interpolate_voids
    from tg_hip import ops as O
    H = W = a.size
    dev = torch.device("cuda:0")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, reps=a.reps, warmup=a.warmup):
        for _ in range(warmup):
            out = fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, out

    for name in a.scenes:
        if name == "basins":
            z, keep = scene(H, W, "0.0")
            z = basins(z, BASINS, 1)
            full = torch.from_numpy(z).to(dev)
        else:
            z, keep = scene(H, W, name)
            full, finfo = interpolate_voids(torch.from_numpy(z).to(dev), torch.from_numpy(keep).to(dev))
            assert finfo["unfilled"] == 0
        known = torch.ones(H, W, dtype=torch.uint8, device=dev)
        ms_route, (direction, _, rinfo, w) = timed(lambda: route_known(full, known, 1.0, check_every=a.check_every,
                                                                       return_surface=True), reps=1, warmup=0)
        ws = O.mfd_ws(H, W, dev)
        ms_setup, (A, counts) = timed(lambda: O.mfd_setup(w, known, direction, a.exponent, ws))
        c0 = counts.cpu().tolist()

        def sweeps():
            # setup again outside the clock is not possible inside one event pair: its time is taken off below
            A2, c2 = O.mfd_setup(w, known, direction, a.exponent, ws)
            return (A2,) + mfd_sweeps(w, a.exponent, A2, c2, ws, a.check_every)
        ms_both, (A, nsweeps, visits) = timed(sweeps)
        ms_sweeps = ms_both - ms_setup
        ms_finish, (acc, out) = timed(lambda: O.mfd_finish(A, direction, ws))
        amax, mass = out.cpu().tolist()
        ms_slope, slope = timed(lambda: O.terrain_slope(w, known, 1.0))
        ms_twi, _ = timed(lambda: O.wetness(acc, slope, known, 1.0, 1e-3))
        print(json.dumps({"what": "mfd_accumulation", "H": H, "W": W, "scene": name, "exponent": a.exponent,
                          "check_every": a.check_every, "ms_setup": round(ms_setup, 3), "ms_sweeps": round(ms_sweeps, 3),
                          "ms_finish": round(ms_finish, 3), "sweeps": nsweeps, "tile_visits": visits,
                          "tiles": (H // TILE) * (W // TILE), "dispersive": c0[0], "single": c0[1], "sinks": c0[2],
                          "max_accumulation_mfd": amax, "mass_rel_err": abs(mass - H * W) / (H * W), "visit_bytes": VISIT_BYTES,
                          "sweeps_GB_per_s": round(visits * VISIT_BYTES / (ms_sweeps * 1e6), 1),
                          "route_known_ms": round(ms_route, 3), "flat_sweeps": rinfo["flat_sweeps"],
                          "ms_slope": round(ms_slope, 3), "ms_wetness": round(ms_twi, 3), "reps": a.reps, "warmup": a.warmup}),
              flush=True)


if __name__ == "__main__":
    main()
