#!/usr/bin/env python3
"""Harmonic void fill throughput (mvp_gan/src/fill_voids.py, csrc/voidfill.hip) on tools/raster_bench.py's synthetic 8192^2
terrain with its disc holes (30 % and 2 % by default) and, as the scene "tiles", with six missing 1024 x 1024 tiles aligned
to multiples of 1024 (9.4 % of the raster: a mosaic with tiles missing), for --solver mg, pcg or both.  Times complete
fill_voids calls and back-to-back V-cycles with device
events after warm-up, and with --evaluate an evaluate_raster(baseline="laplace") call; prints one JSON line per scene: ms per
call, cycles, ms per cycle, the contraction of the change per cycle, the active tiles per level and the algorithmic bytes of
the level passes per cycle.  Where mg does not converge within fill_voids' default budget the scene is timed again with
max_cycles=200 and the line says so ("max_cycles": 200).  With --method biharmonic the same scenes are
filled by the minimum-curvature fill: a line then holds ms per call, the outer iterations ("cycles"), the V-cycles, ms per outer
iteration and ms per V-cycle, to set next to --solver pcg of the harmonic fill.

    python tools/fill_voids_bench.py [--size 8192] [--holes 0.3 0.02 tiles] [--solver mg pcg] [--method laplace|biharmonic [--inner 3]] [--reps 3] [--warmup 1] [--evaluate]
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


MISSING_TILES = ((1, 1), (1, 2), (3, 5), (4, 0), (6, 6), (7, 3))       # of 8 x 8: two adjacent, two on the raster's border


def scene(H, W, holes):
    """-> (z, keep): raster_bench's terrain with disc holes of the given share, or with the missing tiles."""
    from raster_bench import synth
    if holes != "tiles":
        return synth(H, W, float(holes), 0)
    z, keep = synth(H, W, 0.0, 0)
    keep = np.ones_like(keep)
    t = H // 8
    for ty, tx in MISSING_TILES:
        keep[ty * t:(ty + 1) * t, tx * (W // 8):(tx + 1) * (W // 8)] = 0
    return z, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--holes", nargs="+", default=["0.3", "0.02"], help="shares of disc holes, or 'tiles'")
    ap.add_argument("--solver", nargs="+", choices=("mg", "pcg"), default=["mg"])
    ap.add_argument("--method", choices=("laplace", "biharmonic"), default="laplace")
    ap.add_argument("--inner", type=int, default=3, help="biharmonic: V-cycles per approximate Laplace solve")
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
        px0 = pb.get("px0", 0)                                          # level 0's active pixels, for the pcg passes
        per_cycle.update({"vf_pcg_step_kernel": px0 * (4 + 4 + 4 + 1 + 4 + 4),     # x, p, z, flags in; x', r out
                          "vf_pcg_dot_kernel": px0 * (4 + 4 + 4 + 4),              # r, z, x' in; x' out
                          "vf_pcg_dir_kernel": px0 * (4 + 4 + 1 + 4)})             # z, p, flags in; p out
        if any("vf_pcg_step_kernel" in r["Name"] for r in rows):
            # a pcg run: level 0's preconditioner passes share the coarse levels' instantiations, so their rows mix both
            per_cycle["<false, false>"] = per_cycle["<true, false>"] = 0
        per_launch = {"vf_known_kernel": H * W * (4 + 4 + 1),           # dem, mask in; flags out
                      "vf_init_kernel": H * W * (4 + 1 + 8),            # dem, flags in; both value buffers out
                      "vf_finish_kernel": H * W * (4 + 1 + 4 + 4)}      # dem, flags, values in; raster out
        ks = {}
        for r in rows:
            name = r["Name"].split("(")[0].replace("void ", "")
            ns = float(r["TotalDurationNs"])
            ent = {"us_total": round(ns / 1e3, 1), "launches": int(r["Calls"]), "share": round(ns / tot, 4)}
            key = next((k for k in per_cycle if k in name), None)
            if key:
                nb = per_cycle[key] * (int(r["Calls"]) if key.startswith("vf_pcg") else cycles)
            else:
                nb = next((v * int(r["Calls"]) for k, v in per_launch.items() if k in name), 0)
            if nb:
                ent.update(bytes=nb, GB_per_s=round(nb / ns, 1))
            ks[name] = ent
        print(json.dumps({"what": "fill_voids kernels", "H": H, "W": W, "cycles": cycles, "kernel_ms": round(tot / 1e6, 3),
                          "kernels": ks}))
        return
    if not torch.cuda.is_available():
        sys.exit("fill_voids_bench: needs an MI355X (no CPU timing)")
    from mvp_gan.src.fill_voids import fill_voids, vfill_levels
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

    def bits(t):
        return float(np.array([int(t) & 0xffffffff], np.uint32).view(np.float32)[0])

    levels = vfill_levels(H, W)
    for frac in a.holes:
        z, keep = scene(H, W, frac)
        zd, kd = torch.from_numpy(z).to(dev), torch.from_numpy(keep).to(dev)
        if a.method == "biharmonic":
            ms, (out, info) = timed(lambda: fill_voids(zd, kd, method="biharmonic", inner=a.inner), a.reps)
            ws, bws = O.vfill_ws(H, W, dev), O.vfill_bih_ws(H, W, dev)
            st = torch.zeros(2, dtype=torch.int32, device=dev)
            hist = []
            for timing in (False, True):
                O.vfill_setup(zd, kd, None, ws)
                O.vfill_bih_start(H, W, ws, bws, a.inner)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(info["cycles"]):
                    O.vfill_bih_iter(H, W, ws, bws, a.inner, st)
                    if not timing:
                        hist.append(bits(st[0].item()))
                e1.record()
                torch.cuda.synchronize()
            ms_it = e0.elapsed_time(e1) / max(info["cycles"], 1)
            tiles = np.frombuffer(ws[HDR_TILES:HDR_TILES + 4 * len(levels)].cpu().numpy().tobytes(), np.int32).tolist()
            print(json.dumps({"what": "fill_voids", "method": "biharmonic", "inner": a.inner, "H": H, "W": W, "holes": frac,
                              "unknown": info["unknown"], "ms_per_call": round(ms, 3), "cycles": info["cycles"],
                              "vcycles": info["vcycles"], "ms_per_iteration": round(ms_it, 3),
                              "ms_per_vcycle": round(ms_it / (2 * a.inner), 3), "converged": info["converged"],
                              "restarts": info["restarts"], "change": [float("%.3g" % v) for v in hist],
                              "levels": len(levels), "active_tiles": tiles[:len(levels) - 1],
                              "workspace_GB": round((ws.numel() + bws.numel()) / 1e9, 3), "reps": a.reps,
                              "warmup": a.warmup}), flush=True)
            continue
        for solver in a.solver:
            budget = 50
            ms, (out, info) = timed(lambda: fill_voids(zd, kd, solver=solver), a.reps)
            if not info["converged"] and solver == "mg":
                budget = 200
                ms, (out, info) = timed(lambda: fill_voids(zd, kd, solver=solver, max_cycles=budget), a.reps)
            # back-to-back cycles without the per-cycle read, and the change per cycle
            ws = O.vfill_ws(H, W, dev)
            pws = O.vfill_pcg_ws(H, W, dev) if solver == "pcg" else None
            st = torch.zeros(2, dtype=torch.int32, device=dev)

            def start():
                O.vfill_setup(zd, kd, None, ws)
                if pws is not None:
                    O.vfill_pcg_start(H, W, ws, pws)

            def cycle():
                if pws is None:
                    O.vfill_cycle(H, W, ws, st[:1])
                else:
                    O.vfill_pcg_iter(H, W, ws, pws, st)

            start()
            hist = []
            for _ in range(info["cycles"]):
                cycle()
                hist.append(bits(st[0].item()))
            tiles = np.frombuffer(ws[HDR_TILES:HDR_TILES + 4 * len(levels)].cpu().numpy().tobytes(), np.int32).tolist()
            start()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(info["cycles"]):
                cycle()
            e1.record()
            torch.cuda.synchronize()
            ms_cyc = e0.elapsed_time(e1) / max(info["cycles"], 1)
            ratios = [hist[i + 1] / hist[i] for i in range(len(hist) - 1) if hist[i] > 0]
            pb = pass_bytes(levels, tiles)
            pb["px0"] = tiles[0] * TILE_PX
            res = {"what": "fill_voids", "H": H, "W": W, "holes": frac, "solver": solver, "max_cycles": budget,
                   "unknown": info["unknown"], "ms_per_call": round(ms, 3),
                   "cycles": info["cycles"], "ms_per_cycle": round(ms_cyc, 3), "converged": info["converged"],
                   "restarts": info.get("restarts", 0),
                   "contraction_median": round(float(np.median(ratios)), 3) if ratios else None,
                   "contraction_max": round(max(ratios), 3) if ratios else None, "change": [float("%.3g" % v) for v in hist],
                   "levels": len(levels), "active_tiles": tiles[:len(levels) - 1], "pass_bytes_per_cycle": pb,
                   "reps": a.reps, "warmup": a.warmup}
            if solver == "mg":
                res["pass_GB_per_s"] = round((sum(pb.values()) - pb["px0"]) / (ms_cyc * 1e6), 1)
            if a.evaluate and frac == a.holes[0] and solver == a.solver[0]:
                from mvp_gan.src.evaluate_raster import evaluate_raster, eval_holes
                from mvp_gan.src.models import PConvUNet
                torch.manual_seed(0)
                G = PConvUNet().to(dev)
                ms_e, (rep, _) = timed(lambda: evaluate_raster(G, zd, cellsize=1.0, baseline="laplace", solver=solver), 1)
                hm, ekeep, _ = eval_holes(zd, split="test")
                ms_f, _ = timed(lambda: fill_voids(zd, ekeep, solver=solver), a.reps)
                res.update(evaluate_baseline_ms=round(ms_e, 3), baseline_fill_ms=round(ms_f, 3),
                           baseline_share=round(ms_f / ms_e, 4), gan_rmse=round(rep["height"]["rmse"], 4),
                           laplace_rmse=round(rep["baseline"]["height"]["rmse"], 4))
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
