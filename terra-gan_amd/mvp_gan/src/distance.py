"""Distance from every pixel of a raster to the nearest known pixel, in metres, on the GPU (csrc/edt.hip).

The reliability layer of a void-filled DEM: how far is this pixel from measured terrain.  A pixel is known by the rule of
inpaint_raster (mask != 0, finite, != nodata; tg_objmask_known); the distance is the exact Euclidean distance between pixel
centres, computed as an int32 squared distance in pixels (a side is at most 32767 px) and converted once:
dist = float32(cellsize * sqrt(float64(d2))).  Known pixels have distance 0; a raster without a known pixel has +inf everywhere.
max_distance (metres) caps the result at the smallest pixel distance that reaches it, which also bounds the cost of the search
in rasters with large unknown regions.

nearest_known returns the same distance and, per pixel, which known pixel is the nearest (the feature transform, DESIGN.md
section 8t; mvp_gan/src/interpolate.py fills voids from it).

Two calls on the same inputs return bitwise-equal tensors.

CLI: python -m mvp_gan.src.distance --dem in.asc --out depth.asc [--mask m.png|m.asc] [--nodata v] [--max-distance m]
     (cellsize from the header; +inf is written as the NODATA value)
"""
import argparse
import math

import numpy as np
import torch

from . import raster_args as R

MAX_SIDE = 32767                      # TG_EDT_MAX_SIDE: 2 * 32767^2 < 2^31
FAR = 0x7fffffff                      # TG_EDT_FAR


def depth_px2(edges_m, cellsize, who="depth_px2"):
    """Distances in metres -> squared pixel distances: per edge the smallest integer t with sqrt(t) * cellsize >= edge in
    fp64, the arithmetic of the distance itself, so d2 >= t exactly when the distance in metres is >= edge.  ValueError for an
    edge that is not finite and > 0, or beyond every int32 squared distance."""
    c = R.cellsize(cellsize, who)
    out = []
    for e in edges_m:
        try:
            e = float(e)
        except (TypeError, ValueError):
            e = math.nan
        if not math.isfinite(e) or e <= 0:
            raise ValueError(f"{who}: distance {e!r} m must be finite and > 0")
        r = e / c
        if r * r >= FAR - 4:
            raise ValueError(f"{who}: distance {e} m is {r:.6g} px at cellsize {c}: beyond every distance in a raster of "
                             f"{MAX_SIDE} px a side")
        t = max(0, math.floor(r * r) - 2)
        while math.sqrt(t) * c < e:
            t += 1
        out.append(t)
    return out


def px2_m(d2, cellsize):
    """The metres of a squared pixel distance, rounded as the kernel rounds them (fp64 sqrt and multiply, then float32)."""
    return math.inf if d2 >= FAR else float(np.float32(cellsize * math.sqrt(float(d2))))


def check_args(dem, mask, cellsize, max_distance, who="distance_to_known"):
    """Host-side rejection before any launch; -> (H, W, cellsize, cap2)."""
    shape = R.raster_shape(dem, mask, who, max_side=MAX_SIDE)
    c = R.cellsize(cellsize, who)
    cap2 = 0
    if max_distance is not None:
        try:
            cap2 = depth_px2([max_distance], c, who)[0]
        except ValueError as e:
            raise ValueError(f"{who}: max_distance {max_distance!r}: {e}") from None
    return shape[0], shape[1], c, cap2


@torch.no_grad()
def distance_to_known(dem, mask=None, *, nodata=None, cellsize=1.0, max_distance=None):
    """dem: float32 [H][W] (numpy or HIP tensor); mask: same shape, nonzero = known (optional).  Returns (dist float32 HIP
    tensor [H][W] in metres, info dict: known, unknown, max_m (inf without a known pixel), cap_m (None without max_distance,
    else the metres of the cap: the smallest pixel distance >= max_distance), capped (pixels at the cap; 0 without one))."""
    from tg_hip import ops as O
    H, W, c, cap2 = check_args(dem, mask, cellsize, max_distance)
    _, seed = R.upload_known(dem, mask, nodata, "distance_to_known")
    d2, dist = O.edt(seed, cap2, c)
    known = int(seed.count_nonzero().item())
    info = {"known": known, "unknown": H * W - known, "max_m": px2_m(int(d2.max().item()), c) if known else math.inf,
            "cap_m": px2_m(cap2, c) if cap2 else None, "capped": int((d2 == cap2).count_nonzero().item()) if cap2 else 0}
    return dist, info


@torch.no_grad()
def nearest_known(dem, mask=None, *, nodata=None, cellsize=1.0, max_distance=None):
    """distance_to_known, plus which known pixel is the nearest (the feature transform, tg_edt_nearest).
    Returns (dist float32 HIP tensor [H][W] in metres, index int32 HIP tensor [H][W] = y * W + x of the nearest known pixel,
    the smallest row and then the smallest column among those at the smallest distance, -1 where no known pixel is in reach:
    none at all, or none nearer than the cap of max_distance; info as distance_to_known's)."""
    from tg_hip import ops as O
    H, W, c, cap2 = check_args(dem, mask, cellsize, max_distance, who="nearest_known")
    _, seed = R.upload_known(dem, mask, nodata, "nearest_known")
    d2, index = O.edt_nearest(seed, cap2)
    dist = torch.where(d2 == FAR, math.inf, c * d2.double().sqrt()).float()      # fp64 sqrt and multiply, rounded once
    known = int(seed.count_nonzero().item())
    info = {"known": known, "unknown": H * W - known, "max_m": px2_m(int(d2.max().item()), c) if known else math.inf,
            "cap_m": px2_m(cap2, c) if cap2 else None, "capped": int((d2 == cap2).count_nonzero().item()) if cap2 else 0}
    return dist, index, info


# ---- CLI ------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="Distance from every cell of an ESRI ASCII grid to the nearest known cell, in metres.")
    ap.add_argument("--dem", required=True, help="input .asc raster (NODATA_value cells are unknown)")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = known")
    ap.add_argument("--nodata", type=float, help="nodata value (default: the .asc header's NODATA_value)")
    ap.add_argument("--max-distance", type=float, help="cap the distance at this many metres (bounds the search)")
    ap.add_argument("--out", required=True, help="output .asc raster of distances in metres")
    return ap


def main(argv=None):
    from .asc import asc_nodata, read_inputs, with_nodata, write_asc
    a = build_parser().parse_args(argv)
    dem, header, mask, nodata, cellsize = read_inputs(a)
    dist, info = distance_to_known(dem, mask, nodata=nodata, cellsize=cellsize, max_distance=a.max_distance)
    out = dist.cpu().numpy()
    far = np.isinf(out)
    if far.any():
        header = with_nodata(header)
        out = np.where(far, np.float32(asc_nodata(header)), out)
    write_asc(a.out, out, header)
    cap = "" if info["cap_m"] is None else f", {info['capped']} at the cap of {info['cap_m']:.6g} m"
    print(f"{a.out}: {info['known']} known / {info['unknown']} unknown pixels, largest distance {info['max_m']:.6g} m{cap}")
    return info


if __name__ == "__main__":
    main()
