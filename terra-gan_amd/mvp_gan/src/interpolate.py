"""The cheap end of the void-fill ladder on the GPU: nearest neighbour and eight-direction inverse-distance weighting
(csrc/edt.hip, csrc/idw.hip).  The order of the baselines is nearest, IDW, harmonic, thin-plate
(fill_voids), GAN (inpaint_raster); these two cost O(1) per pixel after the scans, whatever the depth of the void.

A pixel is known by the rule of inpaint_raster, fill_voids and distance_to_known (mask != 0, finite, != nodata;
tg_objmask_known).

  method="idw"      eight rays leave every void pixel (N, NE, E, SE, S, SW, W, NW) and stop at the first known pixel; the fill is
                    the mean of the heights hit, weighted by distance^-power (fp64, rounded to fp32 once; the cell size cancels).
                    A ray longer than max_distance does not count.  A pixel no ray serves takes the nearest known pixel
                    (fallback="nearest", if that is within max_distance) or stays NaN (fallback=None).  This is the scheme of
                    gdal_fillnodata; like it, an 8-ray fill shows streaks across wide voids, and `smooth` trades them for blur.
  method="nearest"  every void pixel takes the height of the nearest known pixel (exact Euclidean distance; among equals the
                    smallest row, then the smallest column), NaN where none is within max_distance.
  smooth=n          n Jacobi steps (0..64) of a 3x3 mean over the filled pixels, for both methods; known pixels never move.

max_distance (metres) becomes lim2 = ray_px2(max_distance, cellsize), the largest squared pixel distance still within it, so
"within max_distance" is decided exactly, on integers.  Two calls on the same inputs return bitwise-equal tensors.

CLI: python -m mvp_gan.src.interpolate --dem in.asc --out out.asc [--mask m.png] [--nodata v] [--method idw|nearest]
         [--power p] [--max-distance m] [--smooth n] [--no-fallback]          (cellsize from the header; NaN -> NODATA_value)
"""
import argparse
import math

import torch

from . import raster_args as R
from .distance import FAR, MAX_SIDE

METHODS = ("idw", "nearest")
MAX_SMOOTH = 64
MAX_POWER = 8.0


def ray_px2(max_distance, cellsize, who="ray_px2"):
    """Metres -> squared pixels: the largest integer n with cellsize * sqrt(n) <= max_distance in fp64, the arithmetic of the
    distance itself, so d2 <= n exactly when the distance in metres is <= max_distance.  ValueError for a distance that is not
    finite and > 0, is shorter than one cell (no pixel would be in reach), or is beyond every int32 squared distance."""
    c = R.cellsize(cellsize, who)
    try:
        e = float(max_distance)
    except (TypeError, ValueError):
        e = math.nan
    if not math.isfinite(e) or e <= 0:
        raise ValueError(f"{who}: max_distance {max_distance!r} m must be finite and > 0")
    r = e / c
    if r * r >= FAR - 4:
        raise ValueError(f"{who}: max_distance {e} m is {r:.6g} px at cellsize {c}: beyond every distance in a raster of "
                         f"{MAX_SIDE} px a side")
    t = math.floor(r * r) + 2
    while t > 0 and c * math.sqrt(t) > e:
        t -= 1
    while c * math.sqrt(t + 1) <= e:
        t += 1
    if t < 1:
        raise ValueError(f"{who}: max_distance {e} m is shorter than one cell of {c} m: no pixel is in reach")
    return t


def check_args(dem, mask, method, power, max_distance, cellsize, smooth, fallback, who="interpolate_voids"):
    """Host-side rejection before any launch; -> (H, W, cellsize, power, lim2 (0: no limit), smooth)."""
    shape = R.raster_shape(dem, mask, who, max_side=MAX_SIDE)
    if method not in METHODS:
        raise ValueError(f"{who}: method {method!r} must be one of {METHODS}")
    if fallback not in (None, "nearest"):
        raise ValueError(f"{who}: fallback {fallback!r} must be None or 'nearest'")
    try:
        p = float(power)
    except (TypeError, ValueError):
        p = math.nan
    if not (math.isfinite(p) and 0.0 < p <= MAX_POWER):
        raise ValueError(f"{who}: power {power!r} must lie in (0, {MAX_POWER:g}]")
    if isinstance(smooth, bool) or not isinstance(smooth, int) or not 0 <= smooth <= MAX_SMOOTH:
        raise ValueError(f"{who}: smooth {smooth!r} must be an integer in [0, {MAX_SMOOTH}]")
    c = R.cellsize(cellsize, who)
    lim2 = 0 if max_distance is None else ray_px2(max_distance, c, who)
    return shape[0], shape[1], c, p, lim2, smooth


@torch.no_grad()
def interpolate_voids(dem, mask=None, *, nodata=None, method="idw", power=2.0, max_distance=None, cellsize=1.0, smooth=0,
                      fallback="nearest"):
    """dem: float32 [H][W] (numpy or HIP tensor); mask: same shape, nonzero = known (optional).  Returns (raster float32 HIP
    tensor [H][W]: the known pixels bit for bit, the voids filled, NaN where nothing was in reach; info dict: unknown, filled,
    by_nearest (filled from the nearest known pixel), unfilled, method, power, smooth, max_distance, lim2 (None without
    max_distance))."""
    from tg_hip import ops as O
    H, W, c, p, lim2, smooth = check_args(dem, mask, method, power, max_distance, cellsize, smooth, fallback)
    z, known = R.upload_known(dem, mask, nodata, "interpolate_voids")
    cap2 = lim2 + 1 if lim2 else 0                              # idx >= 0 exactly where d2 <= lim2
    if method == "nearest":
        _, idx = O.edt_nearest(known, cap2)
        out, counts = O.gather_fill(z, known, idx)
        filled, unfilled = counts.cpu().tolist()
        by_nearest = filled
    else:
        out, counts, _ = O.rayfill(z, known, lim2, p)
        by_rays, by_nearest, unfilled = counts.cpu().tolist()
        if unfilled and fallback == "nearest":                  # rare without a limit: pay for the transform only then
            d2, idx = O.edt_nearest(known, cap2)
            out, counts, _ = O.rayfill(z, known, lim2, p, d2, idx)
            by_rays, by_nearest, unfilled = counts.cpu().tolist()
        filled = by_rays + by_nearest
    if smooth:
        out = O.void_smooth(out, known, smooth)
    info = {"unknown": filled + unfilled, "filled": filled, "by_nearest": by_nearest, "unfilled": unfilled, "method": method,
            "power": p, "smooth": smooth, "max_distance": None if max_distance is None else float(max_distance),
            "lim2": lim2 or None}
    return out, info


# ---- CLI ------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="Fill the voids of an ESRI ASCII grid DSM by eight-direction inverse-distance "
                                             "weighting or by the nearest known cell.")
    ap.add_argument("--dem", required=True, help="input .asc raster (NODATA_value cells are voids)")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = known, 0 = void")
    ap.add_argument("--nodata", type=float, help="nodata value (default: the .asc header's NODATA_value)")
    ap.add_argument("--method", choices=METHODS, default="idw")
    ap.add_argument("--power", type=float, default=2.0, help="idw: weights are distance^-power, in (0, 8]")
    ap.add_argument("--max-distance", type=float, help="known cells farther than this many metres do not count")
    ap.add_argument("--smooth", type=int, default=0, help="3x3 mean steps over the filled cells (0..64)")
    ap.add_argument("--no-fallback", action="store_true", help="idw: leave the cells no ray serves unfilled")
    ap.add_argument("--out", required=True, help="output .asc raster")
    return ap


def main(argv=None):
    from .asc import read_inputs, with_nodata, write_asc
    a = build_parser().parse_args(argv)
    dem, header, mask, nodata, cellsize = read_inputs(a)
    out, info = interpolate_voids(dem, mask, nodata=nodata, method=a.method, power=a.power, max_distance=a.max_distance,
                                  cellsize=cellsize, smooth=a.smooth, fallback=None if a.no_fallback else "nearest")
    write_asc(a.out, out.cpu().numpy(), with_nodata(header) if info["unfilled"] else header)
    print(f"{a.out}: {info['unknown']} void pixels, {info['filled']} filled by {a.method} ({info['by_nearest']} from the "
          f"nearest known cell), {info['unfilled']} left unfilled")
    return info


if __name__ == "__main__":
    main()
