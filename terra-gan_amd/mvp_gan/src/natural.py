"""Natural-neighbour (Sibson) void fill on the GPU, in its raster form: discrete Sibson interpolation (Park et al. 2006;
csrc/natural.hip).  The rung of the baseline ladder between the ray fills (IDW, kriging) and the global
solves (fill_voids): local and smooth, without a direction bias, a parameter to tune or a linear system.

A pixel is known by the rule of the other raster tools (mask != 0, finite, != nodata; tg_objmask_known).  The known pixels are
the sites.

  d2(q), idx(q)  the exact feature transform of the known map, without a cap (edt_nearest; its tie rule is part of the fill);
  nn(q)          the nearest fill: z(q) on a known pixel, z[idx(q)] on a void one (gather_fill);
  c(q)           min(d2(q), radius^2), radius an integer in [1, 32];
  out(p)         for a void pixel p the mean of nn(q) over the raster pixels q with |p - q|^2 < c(q) (integers, strictly): the
                 pixels that p, inserted as a site, would take from their nearest site.  q = p always counts, a known q never.
                 The sum runs in float64 in row-major order of q and is divided and rounded to float32 once.
  support(p)     the number of those q: the discrete area of the Voronoi cell p would claim (0 on known pixels).

A void deeper than `radius` fills without any fallback: deep inside, the nearest fill is averaged over the open disc of that
radius.  With radius=1 the result is the nearest fill.  max_distance (metres) becomes lim2 = ray_px2(max_distance, cellsize) as
in interpolate_voids; a void pixel farther than that from every known pixel stays NaN (the limit masks the output only).  Two
calls on the same inputs return bitwise-equal tensors.

CLI: python -m mvp_gan.src.natural --dem in.asc --out out.asc [--mask m.png|m.asc] [--nodata v] [--radius r]
         [--max-distance m] [--support-out s.asc]                         (cellsize from the header; NaN -> NODATA_value)
"""
import argparse
import numbers

import numpy as np
import torch

from . import raster_args as R
from .distance import MAX_SIDE
from .interpolate import ray_px2

MAX_RADIUS = 32                                           # tg_natural_fill's


def check_args(dem, mask, radius, max_distance, cellsize, support=False, who="natural_neighbour_voids"):
    """Host-side rejection before any launch; -> (H, W, cellsize, radius, lim2 (0: no limit))."""
    shape = R.raster_shape(dem, mask, who, max_side=MAX_SIDE)
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, numbers.Integral) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"{who}: radius {radius!r} must be an integer in [1, {MAX_RADIUS}]")
    if not isinstance(support, (bool, np.bool_)):
        raise ValueError(f"{who}: support {support!r} must be True or False")
    c = R.cellsize(cellsize, who)
    lim2 = 0 if max_distance is None else ray_px2(max_distance, c, who)
    return shape[0], shape[1], c, int(radius), lim2


@torch.no_grad()
def natural_neighbour_voids(dem, mask=None, *, nodata=None, cellsize=1.0, radius=32, max_distance=None, support=False):
    """dem: float32 [H][W] (numpy or HIP tensor); mask: same shape, nonzero = known (optional).  Returns (raster float32 HIP
    tensor [H][W]: the known pixels bit for bit, the voids filled, NaN where nothing was in reach; info dict: unknown, filled,
    unfilled, method "natural", radius, max_distance, lim2 (None without max_distance), max_support), or with support=True
    (raster, support int32 HIP tensor [H][W], info).  info["max_support"] is part of every result, so the support plane is
    written and its maximum read back (one device synchronisation) whether or not `support` asks for the plane itself."""
    from tg_hip import ops as O
    who = "natural_neighbour_voids"
    _, _, _, radius, lim2 = check_args(dem, mask, radius, max_distance, cellsize, support, who)
    z, known = R.upload_known(dem, mask, nodata, who)
    d2, idx = O.edt_nearest(known, 0)
    nn, _ = O.gather_fill(z, known, idx)
    out, counts, sup = O.natural_fill(nn, d2, known, radius, lim2, want_support=True)
    filled, unfilled = counts.cpu().tolist()
    info = {"unknown": filled + unfilled, "filled": filled, "unfilled": unfilled, "method": "natural", "radius": radius,
            "max_distance": None if max_distance is None else float(max_distance), "lim2": lim2 or None,
            "max_support": int(sup.max().item())}
    return (out, sup, info) if support else (out, info)


# ---- CLI ------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="Fill the voids of an ESRI ASCII grid DSM by natural-neighbour (discrete Sibson) "
                                             "interpolation.")
    ap.add_argument("--dem", required=True, help="input .asc raster (NODATA_value cells are voids)")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = known, 0 = void")
    ap.add_argument("--nodata", type=float, help="nodata value (default: the .asc header's NODATA_value)")
    ap.add_argument("--radius", type=int, default=MAX_RADIUS, help=f"the largest disc a void cell hands its height to, in cells "
                                                                   f"(1..{MAX_RADIUS}); 1 is the nearest fill")
    ap.add_argument("--max-distance", type=float, help="void cells farther than this many metres from every known cell stay void")
    ap.add_argument("--out", required=True, help="output .asc raster")
    ap.add_argument("--support-out", help="write the number of contributing cells of every filled cell (.asc)")
    return ap


def main(argv=None):
    from .asc import read_inputs, with_nodata, write_asc
    a = build_parser().parse_args(argv)
    dem, header, mask, nodata, cellsize = read_inputs(a)
    out, sup, info = natural_neighbour_voids(dem, mask, nodata=nodata, cellsize=cellsize, radius=a.radius,
                                             max_distance=a.max_distance, support=True)
    write_asc(a.out, out.cpu().numpy(), with_nodata(header) if info["unfilled"] else header)
    if a.support_out:
        write_asc(a.support_out, sup.cpu().numpy().astype(np.float32), header)
    print(f"{a.out}: {info['unknown']} void pixels, {info['filled']} filled by natural neighbours (radius {info['radius']}, "
          f"largest support {info['max_support']}), {info['unfilled']} left unfilled")
    return info


if __name__ == "__main__":
    main()
