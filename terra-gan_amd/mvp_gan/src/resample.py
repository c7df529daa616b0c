"""Resample a DSM raster between its cell size and the cell size a generator was trained at (csrc/resample.hip, DESIGN.md
section 8m), and back, so that the raster entry points can run the generator at its own ground sampling distance.

Semantics:
  - the scale p / q is the working cell size over the source cell size, a fraction with q <= 64 in [1/4, 16];
  - per axis, in units of 1/q source pixel: source pixel i covers [i q, (i+1) q), output pixel I covers [I p, (I+1) p) clipped
    to [0, N q), and the output has ceil(N q / p) pixels: both grids are anchored at the top-left corner and the output cell
    size is exactly the target;
  - known pixel: mask != 0 (if a mask is given), finite, and != nodata (if given), as everywhere else;
  - to a coarser grid (p >= q): area weights, the integer overlaps; an output pixel is known iff the known part of its clipped
    footprint is at least min_coverage of it (decided in integers), and its value is the weighted mean of the known taps;
  - to a finer grid (p <= q): an output pixel is known iff the source pixel that contains its centre is; its value is the
    Catmull-Rom bicubic where all 16 taps are known, else the bilinear over the known ones of the 4 nearest;
  - both evaluate about a pivot tap, so a footprint of one repeated value returns that value bit for bit.

resample_back is the return trip: the other kernel onto the native grid, with the native raster's known pixels copied
through bit for bit.

CLI: python -m mvp_gan.src.resample --dem in.asc --cellsize-out 1.0 --out out.asc [--mask m.png|m.asc] [--min-coverage 0.5]
"""
import argparse
import math
from collections import namedtuple
from fractions import Fraction

import torch

from . import raster_args as R

MAX_DENOMINATOR = 64
MIN_SCALE, MAX_SCALE = Fraction(1, 4), Fraction(16)
COVERAGE_DENOMINATOR = 1000

ResamplePlan = namedtuple("ResamplePlan", "Ho Wo p q rows cols")
AreaTaps = namedtuple("AreaTaps", "start weights")                     # source pixels start .. start + len(weights) - 1
InterpTaps = namedtuple("InterpTaps", "taps cubic linear centre")      # see interp_axis


def resample_scale(cellsize, target_cellsize):
    """-> Fraction p / q = target_cellsize / cellsize with q <= 64.  ValueError when the ratio is no such fraction to 1e-6
    relative, or lies outside [1/4, 16]."""
    c, t = float(cellsize), float(target_cellsize)
    if not (math.isfinite(c) and math.isfinite(t) and c > 0 and t > 0):
        raise ValueError(f"resample: cell sizes {cellsize!r} -> {target_cellsize!r} must be positive and finite")
    ratio = t / c
    fr = Fraction(ratio).limit_denominator(MAX_DENOMINATOR)
    if abs(float(fr) - ratio) > 1e-6 * ratio:
        raise ValueError(f"resample: the scale {ratio!r} ({cellsize} -> {target_cellsize}) is no fraction with a denominator of "
                         f"at most {MAX_DENOMINATOR} (nearest {fr})")
    if not MIN_SCALE <= fr <= MAX_SCALE:
        raise ValueError(f"resample: the scale {fr} ({cellsize} -> {target_cellsize}) is outside [{MIN_SCALE}, {MAX_SCALE}]")
    return fr


def coverage_fraction(min_coverage):
    """-> (Nn, D) = Fraction(min_coverage).limit_denominator(1000), min_coverage in (0, 1]."""
    if isinstance(min_coverage, bool) or not isinstance(min_coverage, (int, float, Fraction)):
        raise ValueError(f"resample: min_coverage {min_coverage!r} must be a number in (0, 1]")
    if not 0 < min_coverage <= 1:
        raise ValueError(f"resample: min_coverage {min_coverage!r} must be in (0, 1]")
    fr = Fraction(min_coverage).limit_denominator(COVERAGE_DENOMINATOR)
    if fr <= 0:
        raise ValueError(f"resample: min_coverage {min_coverage!r} is below 1/{COVERAGE_DENOMINATOR}")
    return fr.numerator, fr.denominator


def area_axis(N, p, q):
    """One axis to a coarser grid (p >= q): per output pixel I the AreaTaps of its clipped footprint, weights[k] the integer
    overlap of [I p, (I+1) p) clipped to [0, N q) with source pixel start + k."""
    No = -(-N * q // p)
    out = []
    for I in range(No):
        lo, hi = I * p, min((I + 1) * p, N * q)
        i0, i1 = lo // q, -(-hi // q)
        out.append(AreaTaps(i0, tuple(min((i + 1) * q, hi) - max(i * q, lo) for i in range(i0, i1))))
    return out


def interp_axis(N, p, q):
    """One axis to a finer grid (p <= q): per output pixel I, whose centre lies at source coordinate
    ((2 I + 1) p - q) / (2 q) = f + r / m with m = 2 q, InterpTaps of
      taps    the indices f - 1 .. f + 2 clamped to the raster,
      cubic   their Catmull-Rom (Keys a = -0.5) weights times 2 m^3 (integers),
      linear  the bilinear weights of taps[1] and taps[2] times m (integers),
      centre  the position in taps (1 or 2) of the source pixel that contains the centre."""
    No = -(-N * q // p)
    m = 2 * q
    out = []
    for I in range(No):
        f, r = divmod((2 * I + 1) * p - q, m)
        cubic = (-r ** 3 + 2 * r * r * m - r * m * m, 3 * r ** 3 - 5 * r * r * m + 2 * m ** 3,
                 -3 * r ** 3 + 4 * r * r * m + r * m * m, r ** 3 - r * r * m)
        out.append(InterpTaps(tuple(min(max(f - 1 + k, 0), N - 1) for k in range(4)), cubic, (m - r, r), 1 if r < q else 2))
    return out


def resample_plan(H, W, p, q):
    """Host-only plan of an H x W raster at scale p / q: ResamplePlan(Ho, Wo, p, q, rows, cols), rows / cols the per-axis taps
    and integer weights (area_axis when p >= q, else interp_axis)."""
    H, W, p, q = int(H), int(W), int(p), int(q)
    if H < 1 or W < 1:
        raise ValueError(f"resample_plan: empty raster {H}x{W}")
    if p < 1 or q < 1 or q > MAX_DENOMINATOR or not MIN_SCALE <= Fraction(p, q) <= MAX_SCALE:
        raise ValueError(f"resample_plan: scale {p}/{q} must lie in [{MIN_SCALE}, {MAX_SCALE}] with a denominator of at most "
                         f"{MAX_DENOMINATOR}")
    axis = area_axis if p >= q else interp_axis
    return ResamplePlan(-(-H * q // p), -(-W * q // p), p, q, axis(H, p, q), axis(W, p, q))


def resampled_header(header, shape, cellsize, target_cellsize, out_shape):
    """The ESRI grid header of the resampled raster: the top-left corner stays where it is, so xllcorner is unchanged and
    yllcorner' = yllcorner + H c - Ho c'.  (key, value string) pairs in the input's order; a *llcenter header keeps that form."""
    H, Ho, Wo = int(shape[0]), int(out_shape[0]), int(out_shape[1])
    c, t = float(cellsize), float(target_cellsize)
    out = []
    for k, v in header:
        kl = k.lower()
        if kl == "ncols":
            v = str(Wo)
        elif kl == "nrows":
            v = str(Ho)
        elif kl == "cellsize":
            v = repr(t)
        elif kl == "yllcorner":
            v = repr(float(v) + H * c - Ho * t)
        elif kl == "yllcenter":
            v = repr(float(v) - c / 2 + H * c - Ho * t + t / 2)
        elif kl == "xllcenter":
            v = repr(float(v) - c / 2 + t / 2)
        out.append((k, v))
    return out


# ---- GPU path -------------------------------------------------------------------------------------------------------
def _inputs(dem, mask, nodata, who):
    device = R.device(who)
    z = R.to_f32(dem, device, "dem", who)
    if z.dim() != 2:
        raise ValueError(f"{who}: dem must be [H, W], got {tuple(z.shape)}")
    m = None if mask is None else R.to_f32(mask, device, "mask", who, binary=True)
    if m is not None and m.shape != z.shape:
        raise ValueError(f"{who}: mask {tuple(m.shape)} differs from the dem {tuple(z.shape)}")
    return z, m, R.nodata_value(nodata)


def resample_to(z, m, nodata, scale, min_coverage=0.5):
    """(z, m) HIP tensors to the grid of `scale` (a Fraction) -> (raster, known mask, n_nan device counter); scale 1 is the
    input with its unknown pixels set to NaN."""
    from tg_hip import ops as O
    p, q = scale.numerator, scale.denominator
    if p >= q:
        return O.resample_area(z, m, nodata, p, q, *coverage_fraction(min_coverage))
    return O.resample_interp(z, m, nodata, p, q)


def resample_raster(dem, mask=None, *, nodata=None, cellsize, target_cellsize, min_coverage=0.5):
    """dem: float32 [H][W] (numpy or HIP tensor) of cell size `cellsize`; mask: same shape, 1 = keep, 0 = hole (optional).
    Returns (raster float32 HIP tensor [Ho][Wo] at `target_cellsize` with NaN at the unknown pixels, known mask float32 1 / 0,
    info dict: scale "p/q", shape, cellsize, known, unknown)."""
    scale = resample_scale(cellsize, target_cellsize)
    coverage_fraction(min_coverage)
    z, m, nodata = _inputs(dem, mask, nodata, "resample_raster")
    out, known, n_nan = resample_to(z, m, nodata, scale, min_coverage)
    unknown = int(n_nan.item())
    info = {"scale": f"{scale.numerator}/{scale.denominator}", "shape": tuple(out.shape), "cellsize": float(target_cellsize),
            "known": out.numel() - unknown, "unknown": unknown}
    return out, known, info


def resample_back(work, dem, mask=None, *, nodata=None, scale):
    """The return trip: `work`, a raster on the grid that `scale` (working / native cell size, a Fraction or "p/q") makes of
    dem's, brought back to dem's grid.  Known pixels of (dem, mask, nodata) come back bit for bit; a hole gets the interpolated
    working surface when the working grid is coarser, the area mean over its finite working pixels when it is finer, and NaN
    where there is none.  Returns (raster float32 HIP tensor [H][W], number of NaN pixels as a device int32 [1])."""
    from tg_hip import ops as O
    scale = Fraction(scale)
    z, m, nodata = _inputs(dem, mask, nodata, "resample_back")
    p, q = scale.numerator, scale.denominator
    if not isinstance(work, torch.Tensor) or tuple(work.shape) != (-(-z.shape[0] * q // p), -(-z.shape[1] * q // p)):
        raise ValueError(f"resample_back: the working raster {tuple(getattr(work, 'shape', ()))} is not the {scale} grid of the "
                         f"dem {tuple(z.shape)}")
    fn = O.resample_interp if p >= q else O.resample_area     # back at q / p: any finite working pixel makes an area mean
    extra = {} if p >= q else {"cov_num": 0, "cov_den": 1}
    out, _, n_nan = fn(work, None, None, q, p, keep=(z, m, nodata), out_shape=tuple(z.shape), **extra)
    return out, n_nan


# ---- CLI ------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="Resample an ESRI ASCII grid DSM to another cell size on the GPU.")
    ap.add_argument("--dem", required=True, help="input .asc raster (NODATA_value cells are unknown)")
    ap.add_argument("--cellsize-out", type=float, required=True, help="cell size of the output, in the header's units")
    ap.add_argument("--out", required=True, help="output .asc raster")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = keep, 0 = unknown")
    ap.add_argument("--min-coverage", type=float, default=0.5,
                    help="to a coarser grid: the known share of its footprint an output cell needs, in (0, 1]")
    return ap


def main(argv=None):
    from .asc import read_inputs, with_nodata, write_asc
    a = build_parser().parse_args(argv)
    dem, header, mask, nodata, c = read_inputs(a)
    out, _, info = resample_raster(dem, mask, nodata=nodata, cellsize=c, target_cellsize=a.cellsize_out,
                                   min_coverage=a.min_coverage)
    write_asc(a.out, out.cpu().numpy(), with_nodata(resampled_header(header, dem.shape, c, a.cellsize_out, out.shape)))
    print(f"{a.out}: scale {info['scale']}, {info['shape'][0]}x{info['shape'][1]} at cellsize {info['cellsize']:g}, "
          f"{info['known']} known / {info['unknown']} unknown")
    return info


if __name__ == "__main__":
    main()
