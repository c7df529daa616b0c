"""Inpaint a whole DSM raster: overlapping windows, per-window min-max over the known pixels, generator in eval mode,
results blended back in metres on the GPU (csrc/raster.hip).

The reference cannot do this: it min-max scales each source grid to a uint8 512^2 PNG, losing the absolute heights
(utils/data_extraction.py:60-115), and never reassembles the tiles (main_pipeline.py:497-530).

Semantics:
  - known pixel: mask != 0 (if a mask is given; 1 = keep, 0 = hole), finite, and != nodata (if given);
  - window plan per axis: w = min(window, N), s = w - overlap, starts 0, s, 2s, ... with the last clamped to N - w;
  - per window lo / hi = min / max over its known pixels; network input x = (z - lo) / (hi - lo) at known pixels, 0 at
    holes (0 everywhere when hi == lo); output in metres lo + out * (hi - lo);
  - only windows with >= 1 known pixel and >= 1 hole run through the generator;
  - a hole gets sum_j w_j * metres_j / sum_j w_j over the running windows covering it (window row, then column), with
    w = r_y * r_x, r(t) = min(1, (t+0.5)/overlap, (w-t-0.5)/overlap) and the ramp of a raster-border side replaced by 1;
  - known pixels are returned bit for bit; a hole no running window covers is NaN and counted in info["unfilled"].

With `objects` (an object_mask.ObjectSpec) the above-ground objects are found on the GPU first (mvp_gan/src/object_mask.py)
and the keep mask, known and not an object, replaces `mask`: the result is bare earth.

With fallback="laplace" the holes no running window covers are filled by fill_voids (mvp_gan/src/fill_voids.py) on the
blended raster, every finite pixel fixed: known and GAN-filled pixels come back bit for bit, and info["fallback"] reports the
interpolated pixels, the cycles and whether they converged.  info["unfilled"] counts the holes still NaN at the end.

With seam="harmonic" the blended raster goes through correct_seams (mvp_gan/src/seam_correct.py) with
the mask the blend used, before any fallback: the filled holes meet the known terrain without a step, and info["seam"] holds
the correction's info.

With model_cellsize (and cellsize) the generator runs at its own ground sampling distance (mvp_gan/src/resample.py, DESIGN.md
section 8m): after the object removal, the raster and its known pixels are resampled to the working grid of that cell size,
the windows above run there (window and overlap are then in working pixels), and the result returns to the native grid with
the known pixels' bits copied through; the seam correction and the fallback then run on the native grid as always.
info["resample"] holds the scale, the working shape and cell size and the hole counts of both grids.

With tta = 2, 4 or 8 (test-time augmentation) every running window goes through the generator under the
first tta of the eight flips and rotations of the square (the transforms RasterWindowLoader trains under), each output is
mapped back, and the blend takes the per-window mean of the members.  inpaint_raster_tta also returns the spread raster in
metres: per hole sqrt(sum_j w_j (var_j (hi_j - lo_j)^2 + (metres_j - out)^2) / sum_j w_j) with var_j the sample variance of
window j's members, 0 at known pixels, NaN where no window filled.  The default tta=1 is the path above, unchanged.

CLI: python -m mvp_gan.src.inpaint_raster --dem in.asc [--mask m.png|m.asc] --checkpoint ck.pth --out out.asc
         [--remove-objects [spec flags] [--objects-out objects.png|objects.asc]] [--fallback laplace] [--solver mg|pcg]
         [--seam harmonic [--seam-order 0|1]] [--model-cellsize 1.0 [--min-coverage 0.5]]
         [--tta 2|4|8 [--spread-out spread.asc]]
"""
import argparse
from collections import namedtuple

import numpy as np
import torch

from . import raster_args as R

MIN_SIDE = 40          # smallest window side the generator is tested at (fixture g72x40b3)
FALLBACK_MAX_CYCLES = 200
SEAMS = ("harmonic",)
TTA_OPS = (0, 1, 2, 3, 4, 5, 6, 7)     # the transforms of csrc/raster_train.hip (src_of): tta members are TTA_OPS[:tta]
TTAS = (1, 2, 4, 8)

Plan = namedtuple("Plan", "H W wh ww overlap ys xs")


def _axis_starts(N, w, overlap):
    s = w - overlap
    n = -(-(N - w) // s) + 1
    return [min(i * s, N - w) for i in range(n)]


def plan_windows(H, W, window=512, overlap=64):
    """Host-only window plan: Plan(H, W, wh, ww, overlap, ys, xs), window (iy, ix) covering
    rows ys[iy] .. ys[iy] + wh and columns xs[ix] .. xs[ix] + ww."""
    H, W, window, overlap = int(H), int(W), int(window), int(overlap)
    if H < 1 or W < 1:
        raise ValueError(f"plan_windows: empty raster {H}x{W}")
    wh, ww = min(window, H), min(window, W)
    if min(wh, ww) < MIN_SIDE:
        raise ValueError(f"plan_windows: window {wh}x{ww} (raster {H}x{W}, window {window}) has a side below {MIN_SIDE} px")
    if not 0 <= overlap < min(wh, ww):
        raise ValueError(f"plan_windows: overlap {overlap} must be in [0, {min(wh, ww)}) for window {wh}x{ww}")
    return Plan(H, W, wh, ww, overlap, _axis_starts(H, wh, overlap), _axis_starts(W, ww, overlap))


def window_ramp(w, overlap, first=False, last=False):
    """1-D blend weight r(t), t = 0..w-1 (float64); `first` / `last`: that side of the window lies on the raster border."""
    t = np.arange(w, dtype=np.float64)
    r = np.ones(w, dtype=np.float64)
    if overlap > 0:
        if not first:
            r = np.minimum(r, (t + 0.5) / overlap)
        if not last:
            r = np.minimum(r, (w - t - 0.5) / overlap)
    return r


# ---- GPU path -------------------------------------------------------------------------------------------------------
def _load_generator(generator_or_checkpoint, device):
    from .models.generator import PConvUNet
    if isinstance(generator_or_checkpoint, PConvUNet):
        return generator_or_checkpoint
    generator = PConvUNet().to(device)                          # as evaluate() loads it
    ckpt = torch.load(generator_or_checkpoint, map_location=device)
    generator.load_state_dict(ckpt["generator_state_dict"] if isinstance(ckpt, dict) and "generator_state_dict" in ckpt else ckpt)
    return generator


def check_seam_options(seam, seam_order, who="inpaint_raster"):
    if seam is not None and seam not in SEAMS:
        raise ValueError(f"{who}: seam {seam!r} must be None or one of {SEAMS}")
    if isinstance(seam_order, bool) or seam_order not in (0, 1):
        raise ValueError(f"{who}: seam_order {seam_order!r} must be 0 or 1")


def check_resample_options(cellsize, model_cellsize, min_coverage, who="inpaint_raster"):
    """-> the scale working / native cell size as a Fraction, or None when nothing is to be resampled."""
    from .resample import coverage_fraction, resample_scale
    coverage_fraction(min_coverage)
    if model_cellsize is None:
        return None
    if cellsize is None:
        raise ValueError(f"{who}: model_cellsize needs cellsize, the raster's metres per pixel")
    scale = resample_scale(cellsize, model_cellsize)
    return None if scale == 1 else scale


def check_tta(tta, shape, window, scale=None, who="inpaint_raster"):
    """tta must be one of TTAS; all eight members need square windows on the grid the windows run on (`shape`, resampled by
    `scale` when there is one).  Host only."""
    if isinstance(tta, bool) or tta not in TTAS:
        raise ValueError(f"{who}: tta {tta!r} must be one of {TTAS}")
    if tta == 8 and len(shape) == 2:
        H, W = shape if scale is None else (-(-n * scale.denominator // scale.numerator) for n in shape)
        wh, ww = min(int(window), H), min(int(window), W)
        if wh != ww:
            raise ValueError(f"{who}: tta=8 transposes the windows and needs them square, but a {H}x{W} raster with window "
                             f"{window} has {wh}x{ww} windows; use tta=4 (the flips)")


def _tta_windows(generator_or_checkpoint, z, m, nodata, pl, cp, lo, hi, run, run_of_d, batch, device, tta):
    """The running windows under the transforms TTA_OPS[:tta]: gather every (window, op) pair of a chunk, run the generator,
    undo the transforms into the per-window mean and variance, blend -> (mean raster, spread raster, unfilled counter)."""
    from tg_hip import engine as E
    from tg_hip import ops as O
    ops = np.array(TTA_OPS[:tta], dtype=np.int32)
    wmean = torch.empty(run.size, pl.wh, pl.ww, dtype=torch.float32, device=device)
    wvar = torch.empty_like(wmean)
    if run.size:
        P = _load_generator(generator_or_checkpoint, device)._tensors()
        items_d = torch.from_numpy(np.repeat(run, tta)).to(device)             # window of every (window, op) pair
        nw = min(max(1, batch // tta), run.size)                                # windows per chunk
        xb = torch.empty(nw * tta, pl.wh, pl.ww, dtype=torch.float32, device=device)
        mb, gb = torch.empty_like(xb), torch.empty_like(xb)
        for b0 in range(0, run.size, nw):
            b1 = min(b0 + nw, run.size)
            n = (b1 - b0) * tta
            x, mk = O.raster_gather_ops(z, m, cp, lo, hi, items_d[b0 * tta:b1 * tta], np.tile(ops, b1 - b0), nodata,
                                        x=xb[:n], m=mb[:n])
            for s0 in range(0, n, batch):                                       # never more than `batch` items per forward
                s1 = min(s0 + batch, n)
                E.generator_forward(P, x[s0:s1], mk[s0:s1], training=False, out=gb[s0:s1])
            O.raster_tta_reduce(gb[:n].view(b1 - b0, tta, pl.wh, pl.ww), ops, mean=wmean[b0:b1], var=wvar[b0:b1])
    return O.raster_blend_tta(z, m, cp, lo, hi, run_of_d, wmean, wvar, nodata)


def _inpaint_windows(generator_or_checkpoint, z, m, nodata, window, overlap, batch, device, tta=1):
    """The window pipeline on one grid -> (raster, its window count, the windows run, the unfilled counter on the device, with
    tta > 1 the spread raster, else None)."""
    from tg_hip import engine as E
    from tg_hip import ops as O
    pl = plan_windows(*z.shape, window=window, overlap=overlap)
    cp = O.raster_plan(pl.H, pl.W, pl.wh, pl.ww, pl.overlap, len(pl.ys), len(pl.xs))
    nwin = len(pl.ys) * len(pl.xs)

    lo, hi, counts = O.raster_window_stats(z, m, cp, nodata)
    c = counts.cpu().numpy()                                    # the one host sync before the result
    run = np.flatnonzero((c[:, 0] > 0) & (c[:, 1] > 0)).astype(np.int32)
    run_of = np.full(nwin, -1, dtype=np.int32)
    run_of[run] = np.arange(run.size, dtype=np.int32)
    run_of_d = torch.from_numpy(run_of).to(device)

    if tta > 1:
        out, spread, unfilled = _tta_windows(generator_or_checkpoint, z, m, nodata, pl, cp, lo, hi, run, run_of_d, batch, device,
                                             tta)
        return out, nwin, int(run.size), unfilled, spread
    wout = torch.empty(run.size, pl.wh, pl.ww, dtype=torch.float32, device=device)
    if run.size:
        P = _load_generator(generator_or_checkpoint, device)._tensors()
        run_d = torch.from_numpy(run).to(device)
        nb = min(batch, run.size)
        xb = torch.empty(nb, pl.wh, pl.ww, dtype=torch.float32, device=device)
        mb = torch.empty_like(xb)
        for b0 in range(0, run.size, nb):
            b1 = min(b0 + nb, run.size)
            x, mk = O.raster_gather(z, m, cp, lo, hi, run_d[b0:b1], nodata, x=xb[:b1 - b0], m=mb[:b1 - b0])
            E.generator_forward(P, x, mk, training=False, out=wout[b0:b1])
    out, unfilled = O.raster_blend(z, m, cp, lo, hi, run_of_d, wout, nodata)
    return out, nwin, int(run.size), unfilled, None


def _tta_info(spread, z, m, nodata, tta):
    """info["tta"]: the members and the mean and largest spread over the filled holes (not known, finite spread), in metres."""
    from tg_hip import ops as O
    known = O.objmask_known(z, m, nodata, transposed=False)[0]
    s = spread[(known == 0) & torch.isfinite(spread)].double()
    return {"members": int(tta), "mean_spread_m": float(s.mean().item()) if s.numel() else 0.0,
            "max_spread_m": float(s.max().item()) if s.numel() else 0.0}


@torch.no_grad()
def inpaint_raster(generator_or_checkpoint, dem, mask=None, *, nodata=None, window=512, overlap=64, batch=16, objects=None,
                   cellsize=None, fallback=None, seam=None, seam_order=1, model_cellsize=None, min_coverage=0.5,
                   solver="mg", tta=1):
    """dem: float32 [H][W] in metres (numpy or HIP tensor); mask: same shape, 1 = keep, 0 = hole (optional).
    objects: an ObjectSpec to remove the above-ground objects first (cellsize, metres per pixel, is then required).
    fallback: None or "laplace": fill the holes no running window covers with fill_voids.
    seam: None or "harmonic": correct the filled holes towards the known terrain around them (correct_seams, seam_order 0 or 1).
    solver: the fill_voids solver of the seam correction and the fallback, "mg" or "pcg" (DESIGN.md section 8n); with "pcg" the
    fallback runs with fill_voids' default budget and its info gains solver and restarts.
    model_cellsize: the cell size the generator was trained at; when it differs from cellsize (then required) the windows run
    on the raster resampled to it (min_coverage: the known share of its footprint a coarser working pixel needs to be known).
    Returns (raster float32 HIP tensor [H][W], info dict: windows, run, unfilled, with objects the object_mask info under
    "objects", with a working grid its description under "resample", with a seam correction its info under "seam", with a
    fallback its pixels, cycles and converged flag under "fallback").
    tta: 1, 2, 4 or 8: run every window under the transforms TTA_OPS[:tta] (identity, the two flips, the half turn, then the
    four transposing ones, which need square windows) and return the mean of the members; the seam
    correction and the fallback act on that mean, and info["tta"] holds members, mean_spread_m and max_spread_m over the
    filled holes.  inpaint_raster_tta returns the spread raster as well.  With tta=1 nothing changes."""
    out, _, info = _inpaint(generator_or_checkpoint, dem, mask, nodata=nodata, window=window, overlap=overlap, batch=batch,
                            objects=objects, cellsize=cellsize, fallback=fallback, seam=seam, seam_order=seam_order,
                            model_cellsize=model_cellsize, min_coverage=min_coverage, solver=solver, tta=tta)
    return out, info


@torch.no_grad()
def inpaint_raster_tta(generator_or_checkpoint, dem, mask=None, *, tta=8, **kwargs):
    """inpaint_raster(..., tta=tta) with the uncertainty map: -> (raster, spread, info).  spread: float32 HIP tensor [H][W] in
    metres, the standard deviation of the fill under the tta transforms (with overlapping windows: of their mixture, the
    disagreement between the windows included); 0 at known pixels, NaN where no window filled (the holes left unfilled, and
    those that only the fallback fills: they have no ensemble).  The seam correction does not change it.  tta: 2, 4 or 8."""
    if tta == 1:
        raise ValueError("inpaint_raster_tta: one member has no spread; tta must be 2, 4 or 8")
    return _inpaint(generator_or_checkpoint, dem, mask, tta=tta, who="inpaint_raster_tta", **kwargs)


@torch.no_grad()
def _inpaint(generator_or_checkpoint, dem, mask=None, *, nodata=None, window=512, overlap=64, batch=16, objects=None,
             cellsize=None, fallback=None, seam=None, seam_order=1, model_cellsize=None, min_coverage=0.5, solver="mg", tta=1,
             who="inpaint_raster"):
    """inpaint_raster and inpaint_raster_tta -> (raster, spread raster or None with tta=1, info)."""
    from .fill_voids import check_solver
    scale = check_resample_options(cellsize, model_cellsize, min_coverage)
    check_solver(solver, who="inpaint_raster")
    check_tta(tta, R.shape(dem), window, scale, who=who)
    device = R.device("inpaint_raster")
    if batch < 1:
        raise ValueError(f"inpaint_raster: batch {batch} < 1")
    if fallback not in (None, "laplace"):
        raise ValueError(f"inpaint_raster: fallback {fallback!r} must be None or 'laplace'")
    check_seam_options(seam, seam_order)
    z = R.to_f32(dem, device, "dem", "inpaint_raster")
    if z.dim() != 2:
        raise ValueError(f"inpaint_raster: dem must be [H, W], got {tuple(z.shape)}")
    m = None if mask is None else R.to_f32(mask, device, "mask", "inpaint_raster", binary=True)
    if m is not None and m.shape != z.shape:
        raise ValueError(f"inpaint_raster: mask {tuple(m.shape)} differs from the dem {tuple(z.shape)}")
    oinfo = None
    if objects is not None:
        from .object_mask import object_mask
        _, m, oinfo = object_mask(z, m, nodata=nodata, cellsize=cellsize, spec=objects)
    nodata = R.nodata_value(nodata)
    rinfo = None
    if scale is None:
        out, nwin, nrun, unfilled, spread = _inpaint_windows(generator_or_checkpoint, z, m, nodata, window, overlap, batch, device,
                                                             tta)
    else:
        from tg_hip import ops as O
        from .resample import resample_back, resample_to
        Hw, Ww = (-(-n * scale.denominator // scale.numerator) for n in z.shape)
        if min(Hw, Ww) < MIN_SIDE:
            raise ValueError(f"inpaint_raster: the working grid {Hw}x{Ww} (raster {z.shape[0]}x{z.shape[1]} at scale {scale}) has "
                             f"a side below {MIN_SIDE} px")
        zw, _, holes_w = resample_to(z, m, nodata, scale, min_coverage)
        holes = O.raster_count_unknown(z, m, nodata)               # the native holes: one read of the raster, nothing written
        outw, nwin, nrun, unfilled_w, spread = _inpaint_windows(generator_or_checkpoint, zw, None, None, window, overlap, batch,
                                                                device, tta)
        out, unfilled = resample_back(outw, z, m, nodata=nodata, scale=scale)
        if spread is not None:
            # the same return trip with a zero raster for the DEM and the native known pixels as its mask: they come back as 0
            known = O.objmask_known(z, m, nodata, transposed=False)[0].float()
            spread, _ = resample_back(spread, torch.zeros_like(z), known, scale=scale)
            spread.clamp_(min=0)             # the bicubic trip back from a coarser grid undershoots next to zeros; NaN stays
        rinfo = {"scale": f"{scale.numerator}/{scale.denominator}", "shape": (Hw, Ww), "cellsize": float(model_cellsize),
                 "holes": int(holes.item()), "working_holes": int(holes_w.item()), "working_unfilled": int(unfilled_w.item())}
    info = {"windows": nwin, "run": nrun, "unfilled": int(unfilled.item())}
    if oinfo is not None:
        info["objects"] = oinfo
    if rinfo is not None:
        info["resample"] = rinfo
    if spread is not None:
        info["tta"] = _tta_info(spread, z, m, nodata, tta)
    if seam is not None:
        from .seam_correct import correct_seams
        out, info["seam"] = correct_seams(z, out, m, nodata=nodata, order=seam_order, solver=solver)
    if fallback is not None:
        info["fallback"] = {"pixels": info["unfilled"], "cycles": 0, "converged": True}
        if info["unfilled"]:
            from .fill_voids import fill_voids
            # every finite pixel fixed: only the NaN holes change.  They are the voids wider than a window, where a V-cycle
            # contracts the change by about 0.77, hence a larger budget than fill_voids' default
            # with the plain cycle; conjugate gradients need no such budget
            if solver == "mg":
                out, finfo = fill_voids(out, method=fallback, max_cycles=FALLBACK_MAX_CYCLES)
            else:
                out, finfo = fill_voids(out, method=fallback, solver=solver)
            info["fallback"] = {"pixels": finfo["unknown"], "cycles": finfo["cycles"], "converged": finfo["converged"]}
            if solver != "mg":
                info["fallback"].update(solver=solver, restarts=finfo["restarts"])
            info["unfilled"] = finfo["unfilled"]
    return out, spread, info


# ---- CLI ------------------------------------------------------------------------------------------------------------
def build_parser():
    from .object_mask import add_spec_args
    ap = argparse.ArgumentParser(description="Inpaint the holes of an ESRI ASCII grid DSM with a TERRA-GAN generator.")
    ap.add_argument("--dem", required=True, help="input .asc raster (NODATA_value cells are holes)")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = keep, 0 = hole")
    ap.add_argument("--checkpoint", required=True, help="generator checkpoint (.pth), loaded as evaluate() does")
    ap.add_argument("--out", required=True, help="output .asc raster")
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--remove-objects", action="store_true",
                    help="find above-ground objects in the DSM (cellsize from the header) and inpaint them to bare earth")
    ap.add_argument("--objects-out", help="with --remove-objects: write the object map (.png or .asc, nonzero = object)")
    ap.add_argument("--fallback", choices=("laplace",),
                    help="fill the holes no window reaches by harmonic interpolation (fill_voids) instead of leaving NaN")
    ap.add_argument("--solver", choices=("mg", "pcg"), default="mg",
                    help="solver of --fallback and --seam: V-cycles, or conjugate gradients around them (large or aligned voids)")
    ap.add_argument("--seam", choices=SEAMS,
                    help="correct the filled holes towards the known terrain around them: no step at the hole outlines")
    ap.add_argument("--seam-order", type=int, choices=(0, 1), default=1,
                    help="with --seam: 1 continues the known slope across the rim, 0 takes the rim value (robust to noise)")
    ap.add_argument("--model-cellsize", type=float,
                    help="cell size the checkpoint was trained at: run the windows on the raster resampled to it (the raster's "
                         "cell size comes from the header); --window and --overlap are then in resampled pixels")
    ap.add_argument("--min-coverage", type=float, default=0.5,
                    help="with a coarser --model-cellsize: the known share of its footprint a resampled cell needs, in (0, 1]")
    ap.add_argument("--tta", type=int, choices=TTAS, default=1,
                    help="test-time augmentation: run every window under this many flips / rotations and write their mean "
                         "(8 needs square windows); costs that many generator passes")
    ap.add_argument("--spread-out", help="with --tta above 1: write the spread of the members (.asc, metres; 0 at known cells)")
    add_spec_args(ap)
    return ap


def parse_args(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.objects_out and not a.remove_objects:
        ap.error("--objects-out needs --remove-objects")
    if a.spread_out and a.tta == 1:
        ap.error("--spread-out needs --tta above 1")
    return a


def main(argv=None):
    from .asc import read_inputs, with_nodata, write_asc, write_mask
    from .object_mask import object_mask, spec_from_args
    a = parse_args(argv)
    dem, header, mask, nodata, cellsize = read_inputs(a)
    if a.remove_objects:                      # what inpaint_raster(objects=...) does, keeping the object map for --objects-out
        objects, mask, oinfo = object_mask(dem, mask, nodata=nodata, cellsize=cellsize, spec=spec_from_args(a))
        if a.objects_out:
            write_mask(a.objects_out, objects.cpu().numpy(), header)
        print(f"{oinfo['objects']} objects, {oinfo['object_pixels']} px removed")
    out, spread, info = _inpaint(a.checkpoint, dem, mask, nodata=nodata, window=a.window, overlap=a.overlap, batch=a.batch,
                                 fallback=a.fallback, seam=a.seam, seam_order=a.seam_order, cellsize=cellsize,
                                 model_cellsize=a.model_cellsize, min_coverage=a.min_coverage, solver=a.solver, tta=a.tta)
    write_asc(a.out, out.cpu().numpy(), with_nodata(header) if info["unfilled"] else header)
    print(f"{a.out}: {info['windows']} windows, {info['run']} run, {info['unfilled']} holes left unfilled")
    if "tta" in info:
        tt = info["tta"]
        print(f"tta {tt['members']}: spread over the filled holes mean {tt['mean_spread_m']:.4g} m, max {tt['max_spread_m']:.4g} m")
        if a.spread_out:
            s = spread.cpu().numpy()
            write_asc(a.spread_out, s, with_nodata(header) if np.isnan(s).any() else header)
    if "resample" in info:
        rs = info["resample"]
        print(f"working grid {rs['shape'][0]}x{rs['shape'][1]} at cellsize {rs['cellsize']:g} (scale {rs['scale']}): "
              f"{rs['holes']} holes, {rs['working_holes']} on the working grid, {rs['working_unfilled']} left unfilled there")
    if "seam" in info:
        sm = info["seam"]
        print(f"seam {a.seam}: {sm['ring']} ring / {sm['interior']} interior pixels, max_delta {sm['max_delta']:.4g} m, "
              f"{sm['cycles']} cycles, converged {sm['converged']}")
        if not sm["converged"]:
            print("warning: the seam correction did not converge")
    if "fallback" in info:
        fb = info["fallback"]
        print(f"fallback {a.fallback}: {fb['pixels']} px, {fb['cycles']} cycles, converged {fb['converged']}")
        if not fb["converged"]:
            print("warning: the fallback fill did not converge")
    return info


if __name__ == "__main__":
    main()
