#!/usr/bin/env python3
"""Empirical variogram and ordinary-kriging fill throughput (csrc/kriging.hip, mvp_gan/src/kriging.py) on
the 8192^2 scenes of tools/fill_voids_bench.py (disc holes of 30 % and 2 %).  Times with device events, 3 calls after 1 warm-up:
the two variogram kernels (ops.variogram on ready tensors), the tg_rayfill that makes the hits, the krige kernel alone for each of
the three models (the power model as fitted to the scene, the other two with the fitted value at 32 px as their sill), and the
complete krige_voids calls with a fitted and with a given variogram; beside them interpolate_voids(method="idw") and fill_voids on
the same scene in the same run, for scale.  ns_per_void_px_* is the krige kernel's time over the void pixels (the known pixels
cost it a copy).  One JSON line per scene, printed and written to --out.

    python tools/kriging_bench.py [--size 8192] [--scenes 0.3 0.02] [--reps 3] [--warmup 1] [--no-fill-voids]
                                  [--out profiles/kriging_8192.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--scenes", nargs="+", default=["0.3", "0.02"], help="shares of disc holes, or 'tiles'")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-fill-voids", action="store_true", help="skip the fill_voids timing of the same scene")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kriging_8192.jsonl"))
    a = ap.parse_args()
    H = W = a.size
    if not torch.cuda.is_available():
        sys.exit("kriging_bench: needs an MI355X (no CPU timing)")
    from dataclasses import asdict

    from fill_voids_bench import scene
    from mvp_gan.src import raster_args as R
    from mvp_gan.src.fill_voids import fill_voids
    from mvp_gan.src.interpolate import interpolate_voids
    from mvp_gan.src.kriging import VGM_OCTAVES, Variogram, assemble_variogram, fit_variogram, krige_voids
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
        zt, known = R.upload_known(zd, kd, None, "kriging_bench")
        void = int((known == 0).sum().item())
        res = {"what": "kriging", "H": H, "W": W, "scene": name, "void_px": void, "reps": a.reps, "warmup": a.warmup}
        ws = O.variogram_ws(H, W, dev)
        ms, (counts, sums) = timed(lambda: O.variogram(zt, known, VGM_OCTAVES, ws))
        emp = assemble_variogram(counts.cpu().numpy(), sums.cpu().numpy(), cellsize=1.0, octaves=VGM_OCTAVES)
        fit, rms = fit_variogram(emp)
        res.update(ms_variogram=round(ms, 3), pairs=int(emp["pairs"].sum()), variogram=asdict(fit), fit_rms_ln=round(rms, 4))
        ms, (_, rc, hits) = timed(lambda: O.rayfill(zt, known, 0, 2.0, want_hits=True))
        res.update(ms_rayfill_hits=round(ms, 3), no_hit_px=int(rc.cpu().tolist()[2]))
        sill = float(fit.gamma(32.0))
        for vg in (fit, Variogram("exponential", 0.0, sill, 32.0), Variogram("spherical", 0.0, sill, 64.0)):
            ms, (_, var, kc) = timed(lambda: O.krige(zt, known, hits, 1.0, vg.model, vg.nugget, vg.scale, vg.shape))
            res.update({f"ms_krige_{vg.model}": round(ms, 3), f"ns_per_void_px_{vg.model}": round(ms * 1e6 / max(void, 1), 3)})
        res["krige_over_rayfill"] = round(res["ms_krige_power"] / res["ms_rayfill_hits"], 2)
        ms, (_, _, info) = timed(lambda: krige_voids(zd, kd))
        res.update(ms_krige_voids_fitted=round(ms, 3), unfilled=info["unfilled"], by_nearest=info["by_nearest"],
                   max_variance=info["max_variance"])
        ms, _ = timed(lambda: krige_voids(zd, kd, variogram=fit))
        res.update(ms_krige_voids_given=round(ms, 3))
        ms, _ = timed(lambda: interpolate_voids(zd, kd))
        res.update(ms_idw=round(ms, 3), krige_voids_over_idw=round(res["ms_krige_voids_fitted"] / ms, 2))
        if not a.no_fill_voids:
            solver = "pcg" if name == "tiles" else "mg"
            ms, (_, finfo) = timed(lambda: fill_voids(zd, kd, solver=solver))
            res.update(ms_fill_voids=round(ms, 3), fill_voids_solver=solver, fill_voids_cycles=finfo["cycles"],
                       fill_voids_over_krige_voids=round(ms / res["ms_krige_voids_fitted"], 2))
        lines.append(res)
        print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
