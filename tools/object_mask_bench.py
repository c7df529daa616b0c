#!/usr/bin/env python3
"""Object detector throughput (mvp_gan/src/object_mask.py) on the seeded synthetic scene of tests/objmask_oracle.py, 8192^2
at 1 m by default, and what it adds to inpaint_raster.  Times complete calls with device events after warm-up and prints one
JSON line: object_mask ms and Mpx/s, inpaint_raster ms with and without `objects` on the same raster, and the algorithmic
bytes of each kernel (divide them by the kernel times of a separate `rocprofv3 --kernel-trace --stats` run for GB/s).

    python tools/object_mask_bench.py [--size 8192] [--reps 3] [--warmup 1] [--no-inpaint]
    rocprofv3 --kernel-trace --stats -d prof -o p --output-format csv -- python tools/object_mask_bench.py --no-inpaint
    python tools/object_mask_bench.py --kstats prof/.../p_kernel_stats.csv     # host only: per-kernel us, share, GB/s
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "terra-gan_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def kernel_bytes(H, W, n_steps, flagged):
    """Bytes per object_mask call each kernel must move at least.  Column pass: fp32 in + out, plus the uint8 known map where
    it masks; the fused last pass also reads s and known and writes flags; transpose: fp32 in + out."""
    n = H * W
    return {
        "objmask_known_kernel": n * (4 + 1 + 1),
        "morph_col_kernel": n_steps * n * ((4 + 4 + 1) * 2 + (4 + 4) + (4 + 4 + 4 + 1 + 1)),
        "objmask_transpose_kernel": n_steps * 2 * n * 8,
        "cc_local_kernel": n * (1 + 4 + 4),
        "cc_border_kernel": n * 4 * 3 // 32,       # the labels of the tile-border pixels (3 of 32 rows / columns of a tile)
        "cc_compress_kernel": flagged * 8,
        "objmask_filter_kernel": n * (4 + 1 + 1 + 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-inpaint", action="store_true", help="time object_mask only")
    ap.add_argument("--kstats", help="rocprofv3 kernel_stats.csv of a --no-inpaint run of this tool: per-kernel GB/s and shares")
    a = ap.parse_args()
    from mvp_gan.src.object_mask import ObjectSpec, object_mask, schedule
    from tests import objmask_oracle as OR
    H = W = a.size
    spec = ObjectSpec()
    radii = schedule(spec, 1.0)[0]
    res = {"what": "object_mask", "H": H, "W": W, "cellsize": 1.0, "radii": radii}
    z, truth = OR.scene(H, W, 0)
    if a.kstats:
        flagged = int(truth.sum())            # host only: the flagged count is about the object area
        kb = kernel_bytes(H, W, len(radii), flagged)
        rows = list(csv.DictReader(open(a.kstats)))
        calls = a.reps + a.warmup
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        ks = {}
        for name, nbytes in kb.items():
            rs = [r for r in rows if r["Name"].startswith(name) or name in r["Name"]]
            if rs:
                ns = sum(float(r["TotalDurationNs"]) for r in rs)
                ks[name] = {"us_per_call": round(ns / calls / 1e3, 1), "launches_per_call": sum(int(r["Calls"]) for r in rs) // calls,
                            "share": round(ns / tot, 4), "GB_per_s": round(nbytes * calls / ns, 1), "bytes_per_call": nbytes}
        res.update(kernel_ms_per_call=round(tot / calls / 1e6, 3), kernels=ks)
        print(json.dumps(res))
        return
    if not torch.cuda.is_available():
        sys.exit("object_mask_bench: needs an MI355X (no CPU timing)")
    dev = torch.device("cuda:0")
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

    ms, (o, _, info) = timed(lambda: object_mask(zd, cellsize=1.0, spec=spec))
    on = o.cpu().numpy() != 0
    res.update(object_mask_ms=round(ms, 3), mpx_per_s=round(H * W / ms / 1e3, 1), objects=info["objects"],
               object_frac=round(float(on.mean()), 4), recall=round(float(on[truth].mean()), 5))
    if not a.no_inpaint:
        from mvp_gan.src.inpaint_raster import inpaint_raster
        from mvp_gan.src.models import PConvUNet
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from raster_bench import synth
        md = torch.from_numpy(synth(H, W, 0.3, 0)[1]).to(dev)     # raster_bench's 30 % disc holes: windows to run without objects
        torch.manual_seed(0)
        G = PConvUNet().to(dev)
        ms_plain, _ = timed(lambda: inpaint_raster(G, zd, md, window=512, overlap=64, batch=16))
        ms_obj, _ = timed(lambda: inpaint_raster(G, zd, md, window=512, overlap=64, batch=16, objects=spec, cellsize=1.0))
        res.update(inpaint_ms=round(ms_plain, 3), inpaint_objects_ms=round(ms_obj, 3),
                   object_mask_share=round(ms / ms_obj, 4))
    res.update(reps=a.reps, warmup=a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
