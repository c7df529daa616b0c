#!/usr/bin/env python3
"""Seam correction throughput (mvp_gan/src/seam_correct.py, csrc/seam.hip) on tools/raster_bench.py's synthetic 8192^2 terrain
with its disc holes, filled with the truth plus an offset per hole (the holes are labelled on the GPU; the offset is a hash of
the label, up to +-1.5 m).  Times complete correct_seams calls and, in the same run on the same hole map, complete fill_voids
calls, with device events after warm-up; with --inpaint also an inpaint_raster(seam="harmonic") call with a random-weight
generator, and the correction's share of it.  Prints one JSON line: ms per call of both, the cycles of both, the counts, the
hole and 8-neighbour ring RMSE before and after, and the algorithmic bytes of the two kernels per launch.

    python tools/seam_bench.py [--size 8192] [--holes 0.3] [--order 1] [--reps 3] [--warmup 1] [--inpaint]
    rocprofv3 --kernel-trace --stats -d prof -o p --output-format csv -- python tools/seam_bench.py --no-fill-voids
    python tools/seam_bench.py --kstats prof/.../p_kernel_stats.csv
"""
import argparse
import csv
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "terra-gan_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def kernel_bytes(H, W):
    """Algorithmic bytes per launch: every raster once."""
    return {"seam_delta_kernel": H * W * (4 + 4 + 4 + 4),        # dem, mask, filled in; delta out
            "seam_apply_kernel": H * W * (4 + 4 + 4 + 4 + 4)}    # dem, mask, filled, delta in; raster out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--holes", type=float, default=0.3)
    ap.add_argument("--order", type=int, choices=(0, 1), default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-fill-voids", action="store_true", help="skip the fill_voids comparison (for a profiled run)")
    ap.add_argument("--inpaint", action="store_true", help="also time inpaint_raster with and without seam='harmonic'")
    ap.add_argument("--kstats", help="rocprofv3 kernel_stats.csv of a run of this tool: per-kernel us and GB/s")
    a = ap.parse_args()
    H = W = a.size
    kb = kernel_bytes(H, W)
    if a.kstats:
        rows = list(csv.DictReader(open(a.kstats)))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        ks = {}
        for r in rows:
            name = r["Name"].split("(")[0].replace("void ", "")
            ns = float(r["TotalDurationNs"])
            ent = {"us_total": round(ns / 1e3, 1), "launches": int(r["Calls"]), "us_per_launch": round(ns / 1e3 / int(r["Calls"]), 1),
                   "share": round(ns / tot, 4)}
            nb = next((v * int(r["Calls"]) for k, v in kb.items() if k in name), 0)
            if nb:
                ent.update(bytes=nb, GB_per_s=round(nb / ns, 1))
            ks[name] = ent
        print(json.dumps({"what": "correct_seams kernels", "H": H, "W": W, "kernel_ms": round(tot / 1e6, 3), "kernels": ks}))
        return
    if not torch.cuda.is_available():
        sys.exit("seam_bench: needs an MI355X (no CPU timing)")
    from mvp_gan.src.fill_voids import fill_voids
    from mvp_gan.src.seam_correct import correct_seams
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

    z, keep = synth(H, W, a.holes, 0)
    zd, kd = torch.from_numpy(z).to(dev), torch.from_numpy(keep).to(dev)
    hole = kd == 0
    labels, _ = O.objmask_components(hole.to(torch.uint8))
    off = 1.5 * torch.sin(labels.to(torch.float32) * 12.9898)           # one offset per hole
    gd = torch.where(hole, zd + off, torch.full_like(zd, float("nan")))
    ms, (out, info) = timed(lambda: correct_seams(zd, gd, kd, order=a.order), a.reps)

    # 8-neighbour ring of the holes, as evaluate_raster scores it
    near = torch.nn.functional.max_pool2d(kd[None, None], 3, 1, 1)[0, 0] > 0
    ring8 = hole & near
    rmse = lambda p, sel: math.sqrt(float(((p - zd)[sel].double() ** 2).mean()))
    res = {"what": "correct_seams", "H": H, "W": W, "holes": a.holes, "order": a.order, "ms_per_call": round(ms, 3),
           "cycles": info["cycles"], "converged": info["converged"], "ring": info["ring"], "interior": info["interior"],
           "unfilled": info["unfilled"], "max_delta": round(info["max_delta"], 4),
           "hole_rmse": [round(rmse(gd, hole), 4), round(rmse(out, hole), 4)],
           "ring8_rmse": [round(rmse(gd, ring8), 4), round(rmse(out, ring8), 4)],
           "kernel_bytes_per_launch": kb, "reps": a.reps, "warmup": a.warmup}
    if not a.no_fill_voids:
        ms_f, (_, finfo) = timed(lambda: fill_voids(zd, kd), a.reps)
        res.update(fill_voids_ms_per_call=round(ms_f, 3), fill_voids_cycles=finfo["cycles"],
                   fill_voids_converged=finfo["converged"], ratio_to_fill_voids=round(ms / ms_f, 3))
    if a.inpaint:
        from mvp_gan.src.inpaint_raster import inpaint_raster
        from mvp_gan.src.models import PConvUNet
        torch.manual_seed(0)
        G = PConvUNet().to(dev)
        ms_0, _ = timed(lambda: inpaint_raster(G, zd, kd), 1)
        ms_s, (_, iinfo) = timed(lambda: inpaint_raster(G, zd, kd, seam="harmonic", seam_order=a.order), 1)
        res.update(inpaint_ms=round(ms_0, 3), inpaint_seam_ms=round(ms_s, 3), seam_share=round((ms_s - ms_0) / ms_s, 4),
                   inpaint_seam_cycles=iinfo["seam"]["cycles"], inpaint_seam_converged=iinfo["seam"]["converged"])
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
