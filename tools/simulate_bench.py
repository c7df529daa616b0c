#!/usr/bin/env python3
"""Conditional-simulation throughput (csrc/simulate.hip, mvp_gan/src/simulate.py) on the 8192^2 scenes of
tools/fill_voids_bench.py (disc holes of 30 % and 2 %).  Times with device events, 3 calls after 1 warm-up, per realisation:
tg_sim_field at 64, 256 and 512 waves without the nugget term and at 256 waves with it, the second tg_krige (of u, over the hits of
the first), tg_sim_combine with and without the running sums, tg_sim_stats, and the whole simulate_voids call (keep=False) at 1 and
at --realisations realisations next to krige_voids with the same variogram.  ns_per_px_wave_* is the field kernel's time over
pixels x waves, the figure that says what bounds it.  One JSON line per scene, printed and written to --out.

    python tools/simulate_bench.py [--size 8192] [--scenes 0.3 0.02] [--reps 3] [--warmup 1] [--realisations 4]
                                   [--out profiles/simulate_8192.jsonl]
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
    ap.add_argument("--realisations", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simulate_8192.jsonl"))
    a = ap.parse_args()
    H = W = a.size
    if not torch.cuda.is_available():
        sys.exit("simulate_bench: needs an MI355X (no CPU timing)")
    from dataclasses import asdict

    from fill_voids_bench import scene
    from mvp_gan.src import raster_args as R
    from mvp_gan.src import simulate as S
    from mvp_gan.src.kriging import VGM_OCTAVES, assemble_variogram, fit_variogram, krige_voids
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
        zt, known = R.upload_known(zd, kd, None, "simulate_bench")
        void = int((known == 0).sum().item())
        counts, sums = O.variogram(zt, known, VGM_OCTAVES)
        fit, _ = fit_variogram(assemble_variogram(counts.cpu().numpy(), sums.cpu().numpy(), cellsize=1.0, octaves=VGM_OCTAVES))
        res = {"what": "simulate", "H": H, "W": W, "scene": name, "void_px": void, "reps": a.reps, "warmup": a.warmup,
               "variogram": asdict(fit)}
        u = None
        for n, amp in ((64, 0.0), (256, 0.0), (512, 0.0), (256, 0.1)):
            tab = S.upload_waves(S.with_phases(S.spectral_waves(fit, 1.0, n, 0), 0, 0), dev)
            ms, u = timed(lambda: O.sim_field(H, W, tab, (0, 0), amp, 0, 0))
            tag = f"{n}_nugget" if amp else str(n)
            res.update({f"ms_sim_field_{tag}": round(ms, 3), f"ns_per_px_wave_{tag}": round(ms * 1e6 / (H * W * n), 5)})
        _, _, hits = O.rayfill(zt, known, 0, 2.0, want_hits=True)
        vg = (1.0, fit.model, fit.nugget, fit.scale, fit.shape)
        ms, (zk, _, _) = timed(lambda: O.krige(zt, known, hits, *vg))
        res["ms_krige_z"] = round(ms, 3)
        ms, (uk, _, _) = timed(lambda: O.krige(u, known, hits, *vg))
        res["ms_krige_u"] = round(ms, 3)
        ms, _ = timed(lambda: O.sim_combine(zt, known, zk, u, uk))
        res["ms_sim_combine"] = round(ms, 3)
        s1, s2 = (torch.zeros(H, W, dtype=torch.float64, device=dev) for _ in range(2))
        ms, _ = timed(lambda: O.sim_combine(zt, known, zk, u, uk, s1, s2))
        res["ms_sim_combine_sums"] = round(ms, 3)
        ms, _ = timed(lambda: O.sim_stats(zk, s1, s2, a.warmup + a.reps))
        res["ms_sim_stats"] = round(ms, 3)
        del s1, s2, uk, u, zk
        ms, _ = timed(lambda: krige_voids(zd, kd, variogram=fit))
        res["ms_krige_voids"] = round(ms, 3)
        ms, _ = timed(lambda: S.simulate_voids(zd, kd, variogram=fit, keep=False))
        res.update(ms_simulate_voids_1=round(ms, 3), simulate_1_over_krige_voids=round(ms / res["ms_krige_voids"], 2))
        ms, (_, _, _, info) = timed(lambda: S.simulate_voids(zd, kd, variogram=fit, realisations=a.realisations, keep=False))
        res.update({"realisations": a.realisations, "ms_simulate_voids_n": round(ms, 3),
                    "ms_per_realisation": round((ms - res["ms_simulate_voids_1"]) / max(a.realisations - 1, 1), 3),
                    "sd_mean": info["sd_mean"], "sd_max": info["sd_max"], "unfilled": info["unfilled"]})
        lines.append(res)
        print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
