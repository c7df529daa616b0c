#!/usr/bin/env python3
"""Harmonic void fill throughput (mvp_gan/src/fill_voids.py, csrc/voidfill.hip) on tools/raster_bench.py's synthetic 8192^2
terrain with its disc holes (30 % and 2 % by default).  Times complete fill_voids calls and back-to-back V-cycles with device
events after warm-up, and with --evaluate an evaluate_raster(baseline="laplace") call; prints one JSON line per scene: ms per
call, cycles, ms per cycle, the contraction of the change per cycle, the active tiles per level and the algorithmic bytes of
the level passes per cycle.

    python tools/fill_voids_bench.py [--size 8192] [--holes 0.3 0.02] [--reps 3] [--warmup 1] [--evaluate]
    rocprofv3 --kernel-trace --stats -d prof -o p --output-format csv -- python tools/fill_voids_bench.py --holes 0.3
    python tools/fill_voids_bench.py --kstats prof/.../p_kernel_stats.csv --pass-bytes '{"down0": B, ...}'
(the profiled run's cycles are the launches of vf_coarsest_kernel, one per cycle; setup and finish kernels count per launch)
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

TILE_PX = 32 * 64
HDR_TILES = 24                 # byte offset of the per-level active tile counts in the workspace header


def pass_bytes(levels, tiles):
    """Algorithmic bytes per cycle of the down and up passes, level 0 and the coarse levels apart: each active tile's cells
    once (values in and out, flags, the level's right-hand side, the restricted / prolongated quarter of the next level;
    level 0's up pass also reads the old values for the change).  Halo re-reads are not counted."""
    out = {"down0": 0, "up0": 0, "down": 0, "up": 0}
    for l, t in enumerate(tiles[:len(levels) - 1]):
        px = t * TILE_PX
        rhs = 4 if l else 0
        sfx = "0" if l == 0 else ""
        out["down" + sfx] += px * ((4 if l == 0 else 0) + 1 + 4 + rhs) + px // 4 * (4 + 1)
        out["up" + sfx] += px * (4 + 1 + 4 + rhs + (4 if l == 0 else 0)) + px // 4 * 4
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--holes", type=float, nargs="+", default=[0.3, 0.02])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--evaluate", action="store_true", help="also time evaluate_raster(baseline='laplace') on the 1st scene")
    ap.add_argument("--kstats", help="rocprofv3 kernel_stats.csv of a run of this tool: per-kernel us and GB/s")
    ap.add_argument("--pass-bytes", default="{}", help="with --kstats: pass_bytes_per_cycle of the profiled scene (JSON)")
    a = ap.parse_args()
    H = W = a.size
    if a.kstats:
        rows = list(csv.DictReader(open(a.kstats)))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        cycles = sum(int(r["Calls"]) for r in rows if "vf_coarsest_kernel" in r["Name"])
        pb = json.loads(a.pass_bytes)
        per_cycle = {"<false, true>": pb.get("down0", 0), "<true, true>": pb.get("up0", 0), "<false, false>": pb.get("down", 0),
                     "<true, false>": pb.get("up", 0)}
        per_launch = {"vf_known_kernel": H * W * (4 + 4 + 1),           # dem, mask in; flags out
                      "vf_init_kernel": H * W * (4 + 1 + 8),            # dem, flags in; both value buffers out
                      "vf_finish_kernel": H * W * (4 + 1 + 4 + 4)}      # dem, flags, values in; raster out
        ks = {}
        for r in rows:
            name = r["Name"].split("(")[0].replace("void ", "")
            ns = float(r["TotalDurationNs"])
            ent = {"us_total": round(ns / 1e3, 1), "launches": int(r["Calls"]), "share": round(ns / tot, 4)}
            key = next((k for k in per_cycle if k in name), None)
            nb = per_cycle[key] * cycles if key else next((v * int(r["Calls"]) for k, v in per_launch.items() if k in name), 0)
            if nb:
                ent.update(bytes=nb, GB_per_s=round(nb / ns, 1))
            ks[name] = ent
        print(json.dumps({"what": "fill_voids kernels", "H": H, "W": W, "cycles": cycles, "kernel_ms": round(tot / 1e6, 3),
                          "kernels": ks}))
        return
    if not torch.cuda.is_available():
        sys.exit("fill_voids_bench: needs an MI355X (no CPU timing)")
    from mvp_gan.src.fill_voids import fill_voids, vfill_levels
    from raster_bench import synth
    from tg_hip import ops as O
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

    levels = vfill_levels(H, W)
    for frac in a.holes:
        z, keep = synth(H, W, frac, 0)
        zd, kd = torch.from_numpy(z).to(dev), torch.from_numpy(keep).to(dev)
        ms, (out, info) = timed(lambda: fill_voids(zd, kd), a.reps)
        # back-to-back cycles without the per-cycle read, and the change per cycle
        ws = O.vfill_ws(H, W, dev)
        O.vfill_setup(zd, kd, None, ws)
        ch = torch.empty(1, dtype=torch.int32, device=dev)
        hist = []
        for _ in range(info["cycles"]):
            O.vfill_cycle(H, W, ws, ch)
            hist.append(float(np.array([ch.item() & 0xffffffff], np.uint32).view(np.float32)[0]))
        tiles = np.frombuffer(ws[HDR_TILES:HDR_TILES + 4 * len(levels)].cpu().numpy().tobytes(), np.int32).tolist()
        O.vfill_setup(zd, kd, None, ws)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(info["cycles"]):
            O.vfill_cycle(H, W, ws, ch)
        e1.record()
        torch.cuda.synchronize()
        ms_cyc = e0.elapsed_time(e1) / max(info["cycles"], 1)
        ratios = [hist[i + 1] / hist[i] for i in range(len(hist) - 1) if hist[i] > 0]
        pb = pass_bytes(levels, tiles)
        res = {"what": "fill_voids", "H": H, "W": W, "holes": frac, "unknown": info["unknown"], "ms_per_call": round(ms, 3),
               "cycles": info["cycles"], "ms_per_cycle": round(ms_cyc, 3), "converged": info["converged"],
               "contraction_median": round(float(np.median(ratios)), 3) if ratios else None,
               "contraction_max": round(max(ratios), 3) if ratios else None, "change": [float("%.3g" % v) for v in hist],
               "levels": len(levels), "active_tiles": tiles[:len(levels) - 1], "pass_bytes_per_cycle": pb,
               "pass_GB_per_s": round(sum(pb.values()) / (ms_cyc * 1e6), 1),
               "reps": a.reps, "warmup": a.warmup}
        if a.evaluate and frac == a.holes[0]:
            from mvp_gan.src.evaluate_raster import evaluate_raster, eval_holes
            from mvp_gan.src.models import PConvUNet
            torch.manual_seed(0)
            G = PConvUNet().to(dev)
            ms_e, (rep, _) = timed(lambda: evaluate_raster(G, zd, cellsize=1.0, baseline="laplace"), 1)
            hm, ekeep, _ = eval_holes(zd, split="test")
            ms_f, _ = timed(lambda: fill_voids(zd, ekeep), a.reps)
            res.update(evaluate_baseline_ms=round(ms_e, 3), baseline_fill_ms=round(ms_f, 3),
                       baseline_share=round(ms_f / ms_e, 4), gan_rmse=round(rep["height"]["rmse"], 4),
                       laplace_rmse=round(rep["baseline"]["height"]["rmse"], 4))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
