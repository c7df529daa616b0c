"""Above-ground objects (buildings, vegetation) found in the DSM alone, on the GPU (csrc/objmask.hip).

The reference draws its masks from aerial imagery with OpenCV heuristics (utils/mask_processing/core.py); this project never
reads imagery, so the object map comes from the heights:

  - known pixel: mask != 0 (if given), finite, and != nodata (if given), the rule of inpaint_raster;
  - progressive morphological filter (Zhang et al. 2003): s_0 = z, s_{k+1} = open_{r_k}(s_k) with square windows of radius
    r_k clipped at the raster border, erosion and dilation over the known pixels only; a known pixel is flagged when
    s_k - s_{k+1} > dh_k (fp32) for some k;
  - radii r_k = 2^k while 2^k < r_max = ceil(max_size_m / (2 cellsize)), then r_max; thresholds dh_0 = dh0,
    dh_k = min(slope (w_k - w_{k-1}) cellsize + dh0, dhmax) with w = 2 r + 1, computed in float64 and rounded once to float32;
  - 8-connected components of the flagged pixels with fewer than min_area_px = ceil(min_area_m2 / cellsize^2) pixels are
    dropped; the survivors are dilated by buffer_px = round(buffer_m / cellsize) (half away from zero) with the same clipped
    square window: the object map O;
  - keep mask = known and not O: the mask inpaint_raster fills to bare earth.

Known limitation: clipped windows flag a band up to r_max wide along the raster border and along large unknown regions
wherever terrain slope x r_max > dhmax.

CLI: python -m mvp_gan.src.object_mask --dem in.asc --out keep.png|keep.asc [--max-size --slope --dh0 --dhmax --min-area
         --buffer] [--mask m.png|m.asc] [--objects-out objects.png|objects.asc]
"""
import argparse
import math
from dataclasses import dataclass, fields

import numpy as np
import torch

from . import raster_args as R


@dataclass(frozen=True)
class ObjectSpec:
    max_size_m: float = 64.0      # largest object side the filter removes
    slope: float = 0.15           # terrain slope allowance (m/m)
    dh0: float = 0.3              # initial height threshold (m)
    dhmax: float = 2.5            # largest height threshold (m)
    min_area_m2: float = 4.0      # smaller components are dropped
    buffer_m: float = 1.0         # dilation of the surviving objects

    def check(self):
        for f in fields(self):
            v = getattr(self, f.name)
            if not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
                raise ValueError(f"ObjectSpec: {f.name} = {v!r} must be finite and >= 0")
        if self.dh0 > self.dhmax:
            raise ValueError(f"ObjectSpec: dh0 {self.dh0} > dhmax {self.dhmax}")


def schedule(spec, cellsize):
    """-> (radii [int], thresholds float32 array, min_area_px, buffer_px) of `spec` at `cellsize` metres per pixel."""
    spec.check()
    c = R.cellsize(cellsize, "object_mask")
    r_max = math.ceil(spec.max_size_m / (2.0 * c))
    radii, k = [], 0
    while 2 ** k < r_max:
        radii.append(2 ** k)
        k += 1
    radii.append(r_max)
    dh = []
    for i, r in enumerate(radii):
        if i == 0:
            dh.append(spec.dh0)
        else:
            dw = (2 * r + 1) - (2 * radii[i - 1] + 1)
            dh.append(min(spec.slope * dw * c + spec.dh0, spec.dhmax))
    min_area = math.ceil(spec.min_area_m2 / (c * c))
    buffer_px = math.floor(spec.buffer_m / c + 0.5)
    return radii, np.array(dh, dtype=np.float64).astype(np.float32), min_area, buffer_px


def pmf(z, known, known_t, radii, thresholds):
    """The filter on the device: -> (flags uint8 [H][W], final surface s_K float32 [H][W])."""
    from tg_hip import ops as O
    flags = torch.zeros(z.shape, dtype=torch.uint8, device=z.device)
    bufs = [torch.empty_like(z) for _ in range(4)]
    s = z
    for r, dh in zip(radii, thresholds):
        t0, t1, out = [b for b in bufs if b is not s][:3]
        s = O.objmask_pmf_step(s, known, known_t, r, float(dh), flags, t0, t1, out)
    return flags, s


@torch.no_grad()
def object_mask(dem, mask=None, *, nodata=None, cellsize, spec=ObjectSpec()):
    """dem: float32 [H][W] in metres (numpy or HIP tensor); mask: same shape, nonzero = known (optional).
    Returns (objects uint8 HIP tensor [H][W], keep float32 HIP tensor [H][W], info dict: flagged, objects, removed,
    object_pixels, radii, thresholds, min_area_px, buffer_px)."""
    from tg_hip import ops as O
    radii, dh, min_area, buffer_px = schedule(spec, cellsize)
    if buffer_px > O.OBJMASK_MAX_BUFFER:
        raise ValueError(f"object_mask: buffer {spec.buffer_m} m is {buffer_px} px at cellsize {cellsize}, "
                         f"more than {O.OBJMASK_MAX_BUFFER}")
    if min_area >= 2 ** 31:
        raise ValueError(f"object_mask: min_area {spec.min_area_m2} m^2 is {min_area} px, more than any raster here")
    R.raster_shape(dem, None, "object_mask")
    z, m, nodata, _ = R.upload(dem, mask, nodata, "object_mask")
    if m is not None and m.shape != z.shape:
        raise ValueError(f"object_mask: mask {tuple(m.shape)} differs from the dem {tuple(z.shape)}")
    known, known_t = O.objmask_known(z, m, nodata)
    flags, _ = pmf(z, known, known_t, radii, dh)
    labels, area = O.objmask_components(flags)
    objects, keep, counts = O.objmask_filter(known, labels, area, min_area, buffer_px)
    c = counts.cpu().tolist()                                   # the one host sync
    info = {"flagged": c[0], "objects": c[1], "removed": c[2], "object_pixels": c[3], "radii": radii,
            "thresholds": [float(t) for t in dh], "min_area_px": min_area, "buffer_px": buffer_px}
    return objects, keep, info


# ---- CLI ------------------------------------------------------------------------------------------------------------
def add_spec_args(ap):
    d = ObjectSpec()
    ap.add_argument("--max-size", type=float, default=d.max_size_m, help="largest object side in metres")
    ap.add_argument("--slope", type=float, default=d.slope, help="terrain slope allowance (m/m)")
    ap.add_argument("--dh0", type=float, default=d.dh0, help="initial height threshold (m)")
    ap.add_argument("--dhmax", type=float, default=d.dhmax, help="largest height threshold (m)")
    ap.add_argument("--min-area", type=float, default=d.min_area_m2, help="smallest object area (m^2)")
    ap.add_argument("--buffer", type=float, default=d.buffer_m, help="buffer around objects (m)")


def spec_from_args(a):
    return ObjectSpec(max_size_m=a.max_size, slope=a.slope, dh0=a.dh0, dhmax=a.dhmax, min_area_m2=a.min_area,
                      buffer_m=a.buffer)


def main(argv=None):
    from .asc import read_inputs, write_mask
    ap = argparse.ArgumentParser(description="Find above-ground objects in an ESRI ASCII grid DSM; write the keep mask.")
    ap.add_argument("--dem", required=True, help="input .asc raster (NODATA_value cells are unknown)")
    ap.add_argument("--out", required=True, help="keep mask (.png or .asc): nonzero = keep, 0 = object or unknown")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = known")
    ap.add_argument("--objects-out", help="optional object map (.png or .asc): nonzero = object")
    add_spec_args(ap)
    a = ap.parse_args(argv)
    dem, header, mask, nodata, cellsize = read_inputs(a)
    objects, keep, info = object_mask(dem, mask, nodata=nodata, cellsize=cellsize, spec=spec_from_args(a))
    write_mask(a.out, keep.cpu().numpy(), header)
    if a.objects_out:
        write_mask(a.objects_out, objects.cpu().numpy(), header)
    print(f"{a.out}: {info['objects']} objects ({info['object_pixels']} px), {info['removed']} components below "
          f"{info['min_area_px']} px removed, {info['flagged']} px flagged")
    return info


if __name__ == "__main__":
    main()
