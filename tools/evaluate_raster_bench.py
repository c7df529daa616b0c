#!/usr/bin/env python3
"""Held-out scoring throughput (mvp_gan/src/evaluate_raster.py) on the seeded synthetic scene of tests/objmask_oracle.py, 8192^2
at 1 m by default, as tools/object_mask_bench.py builds it, with a seeded random generator.  Times complete calls with device
events after warm-up and prints one JSON line: ms per eval_holes, terrain_errors and evaluate_raster call, and the share of the
metric pipeline (eval_holes + terrain_errors) in an evaluate_raster call.

    python tools/evaluate_raster_bench.py [--size 8192] [--reps 3] [--warmup 1] [--no-inpaint]
    rocprofv3 --kernel-trace --stats -d prof -o p --output-format csv -- python tools/evaluate_raster_bench.py --no-inpaint
    python tools/evaluate_raster_bench.py --kstats prof/.../p_kernel_stats.csv --scored N --holes N     # host only
"""
import argparse
import csv
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "terra-gan_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def kernel_bytes(H, W, cells, tile, hole_px):
    """Bytes per metric-pipeline call each kernel must move at least (the bench calls eval_holes and terrain_errors once each
    per rep).  eval_holes: dem in, holes u8 + keep f32 out, the cell masks in; components (cc_*): holes in, labels + area
    written; hole_table: labels; terrain_errors: z, p, keep, holes, labels in, two selection buffers out; select: 3 passes
    over each selection buffer."""
    n = H * W
    return {
        "hole_mask_kernel": cells * tile * tile * 4,
        "eval_holes_kernel": n * (4 + 1 + 4) + cells * tile * tile * 4,
        "cc_local_kernel": n * (1 + 4 + 4),
        "hole_table_kernel": n * 4,
        "terrain_errors_kernel": n * (4 + 4 + 4 + 1 + 4 + 4 + 4) + hole_px * 4,
        "select_hist_kernel": 2 * 3 * n * 4,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-inpaint", action="store_true", help="time eval_holes and terrain_errors only")
    ap.add_argument("--kstats", help="rocprofv3 kernel_stats.csv of a --no-inpaint run of this tool: per-kernel us and GB/s")
    ap.add_argument("--cells", type=int, default=0, help="with --kstats: eligible cells of the timed run (its JSON line)")
    ap.add_argument("--hole-px", type=int, default=0, help="with --kstats: hole pixels of the timed run")
    a = ap.parse_args()
    H = W = a.size
    tile, block, c = 256, 1024, 1.0
    res = {"what": "evaluate_raster", "H": H, "W": W, "cellsize": c, "tile": tile, "block": block}
    if a.kstats:
        kb = kernel_bytes(H, W, a.cells, tile, a.hole_px)
        rows = list(csv.DictReader(open(a.kstats)))
        calls = a.reps + a.warmup
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        ks = {}
        for r in rows:
            name = r["Name"].split("(")[0]
            key = next((k for k in kb if k in name), None)
            ns = float(r["TotalDurationNs"])
            ent = {"us_per_call": round(ns / calls / 1e3, 1), "launches_per_call": int(r["Calls"]) // calls,
                   "share": round(ns / tot, 4)}
            if key:
                ent.update(bytes_per_call=kb[key], GB_per_s=round(kb[key] * calls / ns, 1))
            ks[name] = ent
        res.update(kernel_ms_per_call=round(tot / calls / 1e6, 3), kernels=ks)
        print(json.dumps(res))
        return
    if not torch.cuda.is_available():
        sys.exit("evaluate_raster_bench: needs an MI355X (no CPU timing)")
    from mvp_gan.src.evaluate_raster import eval_holes, evaluate_raster, terrain_errors
    from tests import objmask_oracle as OR
    dev = torch.device("cuda:0")
    z, _ = OR.scene(H, W, 0)
    zd = torch.from_numpy(z).to(dev)
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

    ms_h, (hm, keep, info) = timed(lambda: eval_holes(zd, split="test", block=block, tile=tile, seed=0))
    pred = zd + torch.randn(zd.shape, generator=torch.Generator(device=dev).manual_seed(0), device=dev) * hm
    ms_t, rep = timed(lambda: terrain_errors(zd, pred, hm, keep, cellsize=c))
    res.update(eval_holes_ms=round(ms_h, 3), terrain_errors_ms=round(ms_t, 3), cells=info["cells"], hole_px=info["holes"],
               holes=rep["holes"]["count"], scored=rep["pixels"]["scored"])
    if not a.no_inpaint:
        from mvp_gan.src.models import PConvUNet
        torch.manual_seed(0)
        G = PConvUNet().to(dev)
        ms_e, (rep, _) = timed(lambda: evaluate_raster(G, zd, cellsize=c, split="test", block=block, tile=tile, seed=0))
        res.update(evaluate_raster_ms=round(ms_e, 3), metric_share=round((ms_h + ms_t) / ms_e, 4),
                   height_rmse=round(rep["height"]["rmse"], 4))
    res.update(reps=a.reps, warmup=a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
