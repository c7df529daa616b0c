"""The relief of a raster at each scale: RMS second differences at the lags 1, 2, 4, 8, 16 px, on the GPU (csrc/texture.hip,
DESIGN.md section 8ad).

The one-surface form of evaluate_raster's texture row (texture_errors): the same kernel with the fill equal to the truth.  A triple
is a centre pixel, a unit step u along an axis ("axial": (0, 1), (1, 0)) or along a diagonal ("diagonal": (1, 1), (1, -1)) and a
lag h = 2^j px; it counts when the centre lies in `where` and the centre and both arms x - hu, x + hu are known (mask != 0,
finite, != nodata; tg_objmask_known).  Per scale, rms = sqrt(mean(((z(x - hu) + z(x + hu)) - 2 z(x))^2)) in float64, summed in a
fixed order: two calls return equal numbers.  It describes a DEM or a region of one, for example to check that a fine-tuning
raster has the relief of the target terrain.

CLI: python -m mvp_gan.src.texture --dem in.asc [--mask m.png|m.asc] [--nodata v] [--octaves n] [--json out.json]
     (cellsize from the header; one line per scale)
"""
import argparse
import json
import math

import torch

from . import raster_args as R
from .evaluate_raster import TEX_OCTAVES, check_octaves, texture_scales

WHO = "texture_spectrum"


@torch.no_grad()
def texture_spectrum(dem, mask=None, *, nodata=None, cellsize=1.0, octaves=5, where=None):
    """dem: float32 [H][W] (numpy or HIP tensor); mask: same shape, nonzero = known (optional); where: same shape, nonzero = the
    centres that count (default: every pixel).  -> {"octaves", "scales": [{"lag_px", "class", "lag_m", "triples", "rms"}]} in
    ascending lag; rms is None at a scale without a triple."""
    from tg_hip import ops as O
    c = R.cellsize(cellsize, WHO)
    shape = R.raster_shape(dem, mask, WHO)
    if where is not None and R.shape(where) != shape:
        raise ValueError(f"{WHO}: where {R.shape(where)} differs from the dem {shape}")
    octaves = check_octaves(octaves, WHO)
    z, known = R.upload_known(dem, mask, nodata, WHO)
    sel = torch.ones_like(known) if where is None else R.to_u8(where, z.device, "where", WHO, nonzero=True)
    counts, sums = O.texture_compare(z, z, sel, known, octaves)
    counts, sums = counts.cpu().tolist(), sums.cpu().tolist()
    scales = [{"lag_px": h, "class": name, "lag_m": lag_m, "triples": counts[s],
               "rms": math.sqrt(sums[s][0] / counts[s]) if counts[s] else None}
              for s, (h, name, lag_m) in enumerate(texture_scales(octaves, c))]
    return {"octaves": octaves, "scales": scales}


def scale_line(s):
    rms = "n/a" if s["rms"] is None else f"{s['rms']:.6g} m"
    return f"lag {s['lag_px']:2d} px {s['class']:8s} {s['lag_m']:.6g} m: rms second difference {rms} over {s['triples']} triples"


# ---- CLI ------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="RMS second differences of an ESRI ASCII grid at the lags 1, 2, 4, .. px.")
    ap.add_argument("--dem", required=True, help="input .asc raster (NODATA_value cells are unknown)")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = known")
    ap.add_argument("--nodata", type=float, help="nodata value (default: the .asc header's NODATA_value)")
    ap.add_argument("--octaves", type=int, default=TEX_OCTAVES, help=f"the number of lags 1, 2, 4, .. px, an integer in 1..{TEX_OCTAVES}")
    ap.add_argument("--json", help="write the spectrum here")
    return ap


def main(argv=None):
    from .asc import read_inputs
    ap = build_parser()
    a = ap.parse_args(argv)
    if not 1 <= a.octaves <= TEX_OCTAVES:
        ap.error(f"--octaves must lie in [1, {TEX_OCTAVES}]")
    dem, _, mask, nodata, cellsize = read_inputs(a)
    d = texture_spectrum(dem, mask, nodata=nodata, cellsize=cellsize, octaves=a.octaves)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(d, f, indent=1)
    for s in d["scales"]:
        print(scale_line(s))
    return d


if __name__ == "__main__":
    main()
