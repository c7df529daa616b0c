"""Remove the seams of a filled DSM: a harmonic delta surface on the GPU (csrc/seam.hip).

A fill of the holes of a DSM (inpaint_raster's, or any other) meets the measured terrain with a step, and carries an offset
and a tilt per hole.  The delta-surface fill of DEM void filling removes them: take the mismatch on the rim of each hole,
interpolate it harmonically into the hole, and add it to the fill.  The correction is a pure function of (dem, known mask,
filled raster):

  - known K: mask != 0 (if given), finite, and != nodata (if given; a NaN nodata is ignored), the rule of inpaint_raster;
  - a hole pixel is filled when `filled` is finite there and unfilled otherwise; `filled` at known pixels is ignored;
  - ring I: the filled hole pixels with a known 4-neighbour inside the raster; interior U': the other filled hole pixels;
  - ring target of p in I with g = filled[p]: over the directions up, left, right, down whose neighbour q is known,
    e = 2 z_q - z_q2 when order == 1 and q2 = p + 2 dir is inside the raster and known, else e = z_q;
    d_p = (sum (e - g)) / n in fp32, summed in that order;
  - the delta raster D is d_p on I, 0 on K and on the unfilled holes, NaN on U'; fill_voids(D) solves U' harmonically;
  - result: known pixels as `dem` bit for bit, filled holes g + D in fp32 (ring pixels become their target), unfilled holes NaN.

order 1 continues a plane exactly; order 0 is more robust when the known rim is noisy.  When no hole pixel has a known
neighbour (nothing is known, or no hole is filled) the fill comes back unchanged at the holes.

Two calls on the same inputs return bitwise-equal rasters and equal info.

CLI: python -m mvp_gan.src.seam_correct --dem in.asc --filled fill.asc [--mask keep.png|keep.asc] [--nodata v] [--order 0|1]
         [--tol t] [--max-cycles n] [--solver mg|pcg] --out out.asc
"""
import argparse
import numpy as np
import torch

from . import raster_args as R
from .fill_voids import SOLVERS, check_args, check_solver

ORDERS = (0, 1)
MAX_CYCLES = 200               # the budget of inpaint_raster's fallback: holes as wide as a window converge slowly


def check_seam_args(dem, filled, mask, order, tol, max_cycles, who="correct_seams"):
    """Host-side rejection before any launch; -> (H, W)."""
    H, W, _ = check_args(dem, mask, "laplace", tol, max_cycles, None, None, who=who)
    if R.shape(filled) != (H, W):
        raise ValueError(f"{who}: filled {R.shape(filled)} differs from the dem {(H, W)}")
    if isinstance(order, bool) or order not in ORDERS:
        raise ValueError(f"{who}: order {order!r} must be one of {ORDERS}")
    return H, W


@torch.no_grad()
def correct_seams(dem, filled, mask=None, *, nodata=None, order=1, tol=None, max_cycles=MAX_CYCLES, solver="mg"):
    """dem, filled: float32 [H][W] in metres (numpy or HIP tensor); mask: same shape, nonzero = known (optional).
    Returns (raster float32 HIP tensor [H][W], info dict: ring, interior, unfilled, order, max_delta, cycles, change, tol,
    converged; solver: the fill_voids solver of the delta surface, "pcg" adds solver and restarts to the info)."""
    from tg_hip import ops as O
    from .fill_voids import fill_voids
    check_seam_args(dem, filled, mask, order, tol, max_cycles)
    check_solver(solver, who="correct_seams")
    device = R.device("correct_seams")
    z = R.to_f32(dem, device, "dem", "correct_seams")
    g = R.to_f32(filled, device, "filled", "correct_seams")
    m = None if mask is None else R.to_f32(mask, device, "mask", "correct_seams", binary=True)
    nodata = R.nodata_value(nodata)
    delta, counts = O.seam_delta(z, m, nodata, g, order)
    ring, interior, unfilled, bits = counts.cpu().tolist()      # the one sync before the solve
    info = {"ring": ring, "interior": interior, "unfilled": unfilled, "order": int(order), "max_delta": R.bits_f32(bits)}
    if ring:
        delta, f = fill_voids(delta, tol=tol, max_cycles=max_cycles, solver=solver)
        info.update(cycles=f["cycles"], change=f["change"], tol=f["tol"], converged=f["converged"])
        if solver != "mg":
            info.update(solver=solver, restarts=f["restarts"])
    else:
        # no rim to correct against: g + (-0) = g bit for bit
        delta = torch.full_like(delta, -0.0)
        info.update(cycles=0, change=0.0, tol=0.0 if tol is None else float(tol), converged=True)
        if solver != "mg":
            info.update(solver=solver, restarts=0)
    return O.seam_apply(z, m, nodata, g, delta), info


# ---- CLI ------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="Remove the seams of a filled ESRI ASCII grid DSM by a harmonic delta surface.")
    ap.add_argument("--dem", required=True, help="the measured .asc raster (NODATA_value cells are holes)")
    ap.add_argument("--filled", required=True, help="the filled .asc raster of the same size (its NODATA_value cells are unfilled)")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = known, 0 = hole")
    ap.add_argument("--nodata", type=float, help="nodata value of the dem (default: its header's NODATA_value)")
    ap.add_argument("--order", type=int, choices=ORDERS, default=1,
                    help="1: continue the known slope across the rim (exact on planes); 0: the rim value (robust to noise)")
    ap.add_argument("--tol", type=float, help="stop when a cycle changes no delta by more (default 1e-6 x the delta's range)")
    ap.add_argument("--max-cycles", type=int, default=MAX_CYCLES)
    ap.add_argument("--solver", choices=SOLVERS, default="mg",
                    help="solver of the delta surface: V-cycles, or conjugate gradients around them for large or aligned holes")
    ap.add_argument("--out", required=True, help="output .asc raster")
    return ap


def main(argv=None):
    from .asc import asc_nodata, read_asc, read_mask, with_nodata, write_asc
    a = build_parser().parse_args(argv)
    dem, header = read_asc(a.dem)                  # not read_inputs: the filled raster is read and checked before the mask
    fill, fh = read_asc(a.filled)
    if fill.shape != dem.shape:
        raise ValueError(f"{a.filled} is {fill.shape[0]}x{fill.shape[1]}, the dem {dem.shape[0]}x{dem.shape[1]}")
    fnd = asc_nodata(fh)
    if fnd is not None:
        fill = np.where(fill == np.float32(fnd), np.float32(np.nan), fill)       # unfilled cells stay unfilled
    mask = read_mask(a.mask, dem.shape) if a.mask else None
    nodata = a.nodata if a.nodata is not None else asc_nodata(header)
    out, info = correct_seams(dem, fill, mask, nodata=nodata, order=a.order, tol=a.tol, max_cycles=a.max_cycles,
                              solver=a.solver)
    write_asc(a.out, out.cpu().numpy(), with_nodata(header) if info["unfilled"] else header)
    print(f"{a.out}: {info['ring']} ring / {info['interior']} interior pixels, max_delta {info['max_delta']:.4g} m, "
          f"{info['cycles']} cycles, converged {info['converged']}")
    if not info["converged"]:
        print(f"warning: not converged: last change {info['change']:.3g} > tol {info['tol']:.3g} after {info['cycles']} cycles")
    return info


if __name__ == "__main__":
    main()
