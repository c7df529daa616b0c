#!/usr/bin/env python3
"""Flow routing throughput (mvp_gan/src/flow_routing.py, csrc/flow.hip) on the 8192^2 scenes of
tools/fill_depressions_bench.py (disc holes of 30 % and 2 %, six missing tiles, their voids filled first with interpolate_voids;
"basins": the terrain without voids and with 2000 closed basins dug into it).  Prints one JSON line per scene: ms per
flow_routing call (fill included) by device events; the stages on the filled surface, each between its own pair of events, host
syncs included: slope, flat sweeps, flat directions, accumulation; the flat sweeps, tile visits and accumulation rounds; the
flat cells and the largest contributing area; and in the same run ms per fill_depressions call on the same scene, for scale.

    python tools/flow_routing_bench.py [--size 8192] [--scenes 0.3 0.02 tiles basins] [--reps 3] [--warmup 1] [--check-every 8]
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
# One tile visit of the flat sweep: w (4 B) and D (4 B) of its 64 x 64 pixels and of the 260 halo pixels in, D of the tile out.
# The write-back happens only when the visit lowered a value, and a tile without an undecided pixel stops after the loads.
VISIT_BYTES = TILE * TILE * (4 + 4 + 4) + (4 * TILE + 4) * 8
# One round of the doubling: next and S in, next and S out, the zeroed S, two atomics' worth of S (4 B each) per pixel.
ROUND_BYTES_PER_PIXEL = 4 + 4 + 4 + 4 + 4 + 8
STAGES = ("slope", "flat_sweeps", "flat_dirs", "accumulation")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--scenes", nargs="+", default=["0.3", "0.02", "tiles", "basins"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check-every", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("flow_routing_bench: needs an MI355X (no CPU timing)")
    from fill_depressions_bench import BASINS, basins
    from fill_voids_bench import scene
    from mvp_gan.src.fill_depressions import fill_depressions
    from mvp_gan.src.flow_routing import accumulate, flow_routing, resolve_flats
    from mvp_gan.src.interpolate import interpolate_voids
    from tg_hip import ops as O
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
            full = torch.from_numpy(basins(z, BASINS, 1)).to(dev)
        else:
            z, keep = scene(H, W, name)
            full, finfo = interpolate_voids(torch.from_numpy(z).to(dev), torch.from_numpy(keep).to(dev))
            assert finfo["unfilled"] == 0
        known = torch.ones(H, W, dtype=torch.uint8, device=dev)
        ms_fd, (surface, _) = timed(lambda: fill_depressions(full, check_every=a.check_every))
        ms, (_, _, info) = timed(lambda: flow_routing(full, check_every=a.check_every))
        # the stages on the filled surface, one chain per repetition
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
        tot = dict.fromkeys(STAGES, 0.0)
        ws = O.flow_ws(H, W, dev)
        for rep in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            ev[0].record()
            d, D, _ = O.flow_slope(surface, known, ws)
            ev[1].record()
            sweeps, visits, conv = resolve_flats(surface, D, ws, check_every=a.check_every)
            ev[2].record()
            O.flow_flat_dir(surface, D, d)
            ev[3].record()
            _, _, rounds = accumulate(d, ws, a.check_every)
            ev[4].record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                for i, s in enumerate(STAGES):
                    tot[s] += ev[i].elapsed_time(ev[i + 1]) / a.reps
        assert conv and rounds == info["acc_rounds"]
        print(json.dumps({"what": "flow_routing", "H": H, "W": W, "scene": name, "check_every": a.check_every,
                          "ms_per_call": round(ms, 3), **{"ms_" + s: round(tot[s], 3) for s in STAGES},
                          "flat_sweeps": sweeps, "tile_visits": visits, "tiles": (H // TILE) * (W // TILE), "acc_rounds": rounds,
                          "flat_cells": info["flat_cells"], "pits": info["pits"], "max_accumulation": info["max_accumulation"],
                          "converged": info["converged"], "visit_bytes": VISIT_BYTES,
                          "flat_sweeps_GB_per_s": round(visits * VISIT_BYTES / (tot["flat_sweeps"] * 1e6), 1),
                          "accumulation_GB_per_s": round(rounds * H * W * ROUND_BYTES_PER_PIXEL / (tot["accumulation"] * 1e6), 1),
                          "fill_depressions_ms_per_call": round(ms_fd, 3), "reps": a.reps, "warmup": a.warmup}), flush=True)


if __name__ == "__main__":
    main()
