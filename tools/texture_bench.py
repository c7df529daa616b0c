#!/usr/bin/env python3
"""Throughput of the texture row (mvp_gan/src/evaluate_raster.py texture_errors, csrc/texture.hip) on the seeded synthetic scene of
tests/objmask_oracle.py, 8192^2 at 1 m by default, with the test-split holes of eval_holes (tile 256, block 1024), as
tools/evaluate_raster_bench.py builds them.  Times complete calls with device events after warm-up: texture_errors, the two kernels
alone (ops.texture_compare on ready tensors) and terrain_errors on the same inputs for scale; then once more with every pixel
selected, which switches the tile skip off.  One JSON line per case, printed and written to --out.

Bytes: "alg_bytes" is what the statistic must read at least: sel everywhere, and z, p and known over the tiles that hold a sel
pixel.  "staged_bytes" is what the kernel requests: sel everywhere, and z, p and known over the 64 x 96 staged image of each such
tile (three times the tile: the 16-px halo).  GB/s = bytes / the time of the two kernels.

    python tools/texture_bench.py [--size 8192] [--reps 3] [--warmup 1] [--octaves 5] [--evaluate] [--out profiles/texture_8192.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "terra-gan_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

TY, TX, HALO = 32, 64, 16


def tiles_with_sel(sel):
    """How many 32 x 64 tiles of the kernel's grid hold a nonzero pixel of sel (uint8 [H][W] HIP tensor)."""
    H, W = sel.shape
    pad = torch.nn.functional.pad(sel, (0, -W % TX, 0, -H % TY))
    return int(pad.view(pad.shape[0] // TY, TY, pad.shape[1] // TX, TX).amax(dim=(1, 3)).count_nonzero().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--octaves", type=int, default=5)
    ap.add_argument("--evaluate", action="store_true", help="also time an evaluate_raster call with a seeded generator, without and "
                                                            "with texture=True: the share of the row in the call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_8192.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("texture_bench: needs an MI355X (no CPU timing)")
    from mvp_gan.src.evaluate_raster import _fill_upload, eval_holes, evaluate_raster, terrain_errors, texture_errors
    from tests import objmask_oracle as OR
    from tg_hip import ops as O
    H = W = a.size
    tile, block, c = 256, 1024, 1.0
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

    hm, keep, info = eval_holes(zd, split="test", block=block, tile=tile, seed=0)
    pred = zd + torch.randn(zd.shape, generator=torch.Generator(device=dev).manual_seed(0), device=dev) * hm
    ms_terrain, _ = timed(lambda: terrain_errors(zd, pred, hm, keep, cellsize=c))
    lines = []
    for case, holes in (("test_holes", hm), ("all_pixels", torch.ones_like(hm))):
        ms_call, d = timed(lambda: texture_errors(zd, pred, holes, cellsize=c, octaves=a.octaves))
        zt, pt, sel, known = _fill_upload(zd, pred, holes, None, None)
        ws = O.texture_ws(H, W, dev)
        ms_k, _ = timed(lambda: O.texture_compare(zt, pt, sel, known, a.octaves, ws))
        staged = tiles_with_sel(sel)
        tiles = -(-H // TY) * -(-W // TX)
        alg = H * W + staged * TY * TX * 9
        req = H * W + staged * (TY + 2 * HALO) * (TX + 2 * HALO) * 9
        lines.append({"what": "texture", "case": case, "H": H, "W": W, "cellsize": c, "tile": tile, "block": block,
                      "octaves": a.octaves, "sel_px": int(sel.count_nonzero().item()), "tiles": tiles, "tiles_staged": staged,
                      "texture_errors_ms": round(ms_call, 3), "texture_kernels_ms": round(ms_k, 3),
                      "terrain_errors_ms": round(ms_terrain, 3), "alg_bytes": alg, "alg_GB_per_s": round(alg / ms_k / 1e6, 1),
                      "staged_bytes": req, "staged_GB_per_s": round(req / ms_k / 1e6, 1),
                      "triples": [s["triples"] for s in d["scales"]], "log_ratio_rms": d["log_ratio_rms"],
                      "reps": a.reps, "warmup": a.warmup})
    if a.evaluate:
        from mvp_gan.src.models import PConvUNet
        torch.manual_seed(0)
        G = PConvUNet().to(dev)
        kw = dict(cellsize=c, split="test", block=block, tile=tile, seed=0)
        ms_plain, _ = timed(lambda: evaluate_raster(G, zd, **kw))
        ms_tex, _ = timed(lambda: evaluate_raster(G, zd, texture=True, texture_octaves=a.octaves, **kw))
        lines[0].update(evaluate_raster_ms=round(ms_plain, 3), evaluate_raster_texture_ms=round(ms_tex, 3),
                        texture_share=round(lines[0]["texture_errors_ms"] / ms_tex, 4))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
