"""Ordinary kriging of the voids of a DEM with its variance map, and the empirical semivariogram, on the GPU (csrc/kriging.hip,
DESIGN.md section 8ae).  The rung of the baseline ladder between IDW and the harmonic fill, and the one fill that says how far to
trust each pixel: the kriging variance is in m^2 and scales with the raster's own variogram.

A pixel is known by the rule of the other raster tools (mask != 0, finite, != nodata; tg_objmask_known).

  Variogram            gamma(h) in m^2 for h in metres, gamma(0) = 0:
                         power        nugget + scale * h^shape                      0 < shape < 2
                         exponential  nugget + scale * (1 - exp(-h / shape))        shape > 0 (metres)
                         spherical    nugget + scale * (1.5 r - 0.5 r^3)            r = min(h / shape, 1), shape > 0 (metres)
  empirical_variogram  half the mean squared first difference of the known pixels at the lags 1, 2, .. 32 px along the axes and
                       along the diagonals, every unordered pair once, summed in float64 in a fixed order.
  fit_variogram        the power model through an empirical table: a weighted line through (ln h, ln gamma).  No GPU.
  krige_voids          the samples of a void pixel are the first known pixels along eight rays (N, NE, E, SE, S, SW, W, NW;
                       interpolate_voids' rays, so max_distance and fallback mean what they mean there); the estimate and its
                       variance solve the ordinary-kriging system of those at most eight samples in float64.  A pixel no ray
                       serves takes the nearest known pixel and twice the variogram at its distance (fallback="nearest") or stays
                       NaN.  Without a variogram the power model is fitted to this raster's known pixels.

Two calls on the same inputs return bitwise-equal tensors.

CLI: python -m mvp_gan.src.kriging --dem in.asc --out filled.asc [--variance-out var.asc] [--mask m.png|m.asc] [--nodata v]
         [--model power|exponential|spherical --nugget n --scale s --shape p] [--max-distance m] [--no-fallback]
         [--variogram-json v.json]       (cellsize from the header; NaN -> NODATA_value; nothing is fitted with --nugget, --scale
         or --shape given)
"""
import argparse
import json
import math
from dataclasses import asdict, dataclass

import numpy as np
import torch

from . import raster_args as R
from .interpolate import check_args

MODELS = ("power", "exponential", "spherical")            # the index is tg_krige's model
VGM_OCTAVES = 6                                           # TG_VGM_OCTAVES: lags 1, 2, 4, 8, 16, 32 px
VGM_CLASSES = ("axial", "diagonal")                       # scale index = 2 * octave + class
SHAPE_CLIP = (0.05, 1.95)                                 # fit_variogram keeps the power inside (0, 2)


@dataclass(frozen=True)
class Variogram:
    """A variogram model; rejects what tg_krige rejects."""
    model: str = "power"
    nugget: float = 0.0
    scale: float = 1.0
    shape: float = 1.0

    def __post_init__(self):
        if self.model not in MODELS:
            raise ValueError(f"Variogram: model {self.model!r} must be one of {MODELS}")
        for name in ("nugget", "scale", "shape"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"Variogram: {name} {v!r} must be a finite number")
            object.__setattr__(self, name, float(v))
        if self.nugget < 0:
            raise ValueError(f"Variogram: nugget {self.nugget!r} must be >= 0")
        if self.scale <= 0:
            raise ValueError(f"Variogram: scale {self.scale!r} must be > 0")
        if self.shape <= 0 or (self.model == "power" and self.shape >= 2):
            raise ValueError(f"Variogram: shape {self.shape!r} must lie in (0, 2) for the power model, else be > 0")

    def gamma(self, h):
        """gamma(h) in float64 (numpy), h in metres; 0 at h = 0.  The one host-side definition."""
        h = np.asarray(h, np.float64)
        nug, sc, sh = np.float64(self.nugget), np.float64(self.scale), np.float64(self.shape)
        if self.model == "power":
            with np.errstate(divide="ignore"):
                g = nug + sc * np.exp2(sh * np.log2(h))                 # h^shape as the kernel takes it; h = 0 is replaced below
        elif self.model == "exponential":
            g = nug + sc * (np.float64(1.0) - np.exp(-h / sh))
        else:
            r = np.minimum(h / sh, np.float64(1.0))
            g = nug + sc * (np.float64(1.5) * r - np.float64(0.5) * ((r * r) * r))
        return np.where(h > 0, g, np.float64(0.0))


def check_octaves(octaves, who="empirical_variogram"):
    import numbers
    if isinstance(octaves, (bool, np.bool_)) or not isinstance(octaves, numbers.Integral) or not 1 <= octaves <= VGM_OCTAVES:
        raise ValueError(f"{who}: octaves {octaves!r} must be an integer in [1, {VGM_OCTAVES}]")
    return int(octaves)


def variogram_scales(octaves, cellsize):
    """[(lag_px, class name, lag_m)] in scale-index order: L c for the axial class, L c sqrt(2) for the diagonal class."""
    return [(1 << j, name, (1 << j) * cellsize * (math.sqrt(2.0) if k else 1.0))
            for j in range(octaves) for k, name in enumerate(VGM_CLASSES)]


def assemble_variogram(counts, sums, *, cellsize, octaves):
    """The empirical table from tg_variogram's numbers (pure: no GPU): gamma = sums / (2 pairs), NaN at a lag without a pair."""
    octaves = check_octaves(octaves, "assemble_variogram")
    c = R.cellsize(cellsize, "assemble_variogram")
    pairs = np.asarray(counts, np.int64)[:2 * octaves]
    s = np.asarray(sums, np.float64)[:2 * octaves]
    with np.errstate(invalid="ignore", divide="ignore"):
        gamma = np.where(pairs > 0, s / (np.float64(2.0) * pairs.astype(np.float64)), np.nan)
    sc = variogram_scales(octaves, c)
    return {"octaves": octaves, "cellsize": c, "lag_px": [h for h, _, _ in sc], "class": [n for _, n, _ in sc],
            "lags_m": np.array([m for _, _, m in sc], np.float64), "gamma": gamma, "pairs": pairs}


@torch.no_grad()
def empirical_variogram(dem, mask=None, *, nodata=None, cellsize=1.0, octaves=6):
    """dem: float32 [H][W] (numpy or HIP tensor); mask: same shape, nonzero = known (optional).  -> {"lags_m", "gamma", "pairs"
    (numpy arrays of 2 * octaves scales in ascending lag), "lag_px", "class", "octaves", "cellsize"}."""
    from tg_hip import ops as O
    who = "empirical_variogram"
    c = R.cellsize(cellsize, who)
    R.raster_shape(dem, mask, who)
    octaves = check_octaves(octaves, who)
    z, known = R.upload_known(dem, mask, nodata, who)
    counts, sums = O.variogram(z, known, octaves)
    return assemble_variogram(counts.cpu().numpy(), sums.cpu().numpy(), cellsize=c, octaves=octaves)


def fit_variogram(emp, min_pairs=30):
    """The power model through an empirical table (empirical_variogram's dict, or any with lags_m, gamma and pairs): the line
    through (ln h, ln gamma) by least squares weighted by the pairs, over the scales with pairs >= min_pairs and gamma > 0;
    shape = the slope clipped to SHAPE_CLIP, scale = exp(the weighted mean of ln gamma - shape ln h), nugget = 0.
    -> (Variogram, the weighted rms residual in ln units).  ValueError with fewer than two usable scales.  Pure: no GPU."""
    h = np.asarray(emp["lags_m"], np.float64)
    g = np.asarray(emp["gamma"], np.float64)
    n = np.asarray(emp["pairs"], np.float64)
    if not (h.shape == g.shape == n.shape and h.ndim == 1):
        raise ValueError("fit_variogram: lags_m, gamma and pairs must be sequences of one length")
    ok = (n >= min_pairs) & np.isfinite(g) & (g > 0) & np.isfinite(h) & (h > 0)
    if int(ok.sum()) < 2 or np.unique(h[ok]).size < 2:
        raise ValueError(f"fit_variogram: {int(ok.sum())} scales with at least {min_pairs} pairs and gamma > 0, two are needed: "
                         "pass a Variogram instead (variogram=..., or --model / --nugget / --scale / --shape)")
    x, y, w = np.log(h[ok]), np.log(g[ok]), n[ok] / n[ok].sum()
    xm, ym = float((w * x).sum()), float((w * y).sum())
    slope = float((w * (x - xm) * (y - ym)).sum() / (w * (x - xm) ** 2).sum())
    shape = min(max(slope, SHAPE_CLIP[0]), SHAPE_CLIP[1])
    intercept = ym - shape * xm
    rms = math.sqrt(float((w * (y - (intercept + shape * x)) ** 2).sum()))
    return Variogram("power", 0.0, math.exp(intercept), shape), rms


def check_variogram(variogram, who="krige_voids"):
    if variogram is not None and not isinstance(variogram, Variogram):
        raise ValueError(f"{who}: variogram {variogram!r} must be None (fit the power model) or a Variogram")
    return variogram


@torch.no_grad()
def krige_voids(dem, mask=None, *, nodata=None, cellsize=1.0, variogram=None, max_distance=None, fallback="nearest"):
    """dem: float32 [H][W] (numpy or HIP tensor); mask: same shape, nonzero = known (optional).  Returns (filled float32 HIP
    tensor [H][W]: the known pixels bit for bit, the voids kriged, NaN where nothing was in reach; variance float32 HIP tensor
    [H][W] in m^2: 0 on known pixels, NaN where filled is; info dict: unknown, filled, by_nearest, unfilled, variogram (a dict),
    fitted, max_variance, max_distance, lim2 (None without max_distance))."""
    from tg_hip import ops as O
    who = "krige_voids"
    _, _, c, _, lim2, _ = check_args(dem, mask, "idw", 2.0, max_distance, cellsize, 0, fallback, who=who)
    check_variogram(variogram, who)
    z, known = R.upload_known(dem, mask, nodata, who)
    fitted = variogram is None
    if fitted:
        counts, sums = O.variogram(z, known, VGM_OCTAVES)
        variogram, _ = fit_variogram(assemble_variogram(counts.cpu().numpy(), sums.cpu().numpy(), cellsize=c,
                                                        octaves=VGM_OCTAVES))
    _, counts, hits = O.rayfill(z, known, lim2, 2.0, want_hits=True)
    d2 = idx = None
    if counts.cpu().tolist()[2] and fallback == "nearest":      # rare without a limit: pay for the transform only then
        d2, idx = O.edt_nearest(known, lim2 + 1 if lim2 else 0)  # idx >= 0 exactly where d2 <= lim2
    out, var, counts = O.krige(z, known, hits, c, variogram.model, variogram.nugget, variogram.scale, variogram.shape, d2, idx)
    by_rays, by_nearest, unfilled = counts.cpu().tolist()
    filled = by_rays + by_nearest
    info = {"unknown": filled + unfilled, "filled": filled, "by_nearest": by_nearest, "unfilled": unfilled,
            "variogram": asdict(variogram), "fitted": fitted,
            "max_variance": float(torch.nan_to_num(var, nan=0.0).max().item()),
            "max_distance": None if max_distance is None else float(max_distance), "lim2": lim2 or None}
    return out, var, info


# ---- CLI ------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="Fill the voids of an ESRI ASCII grid DSM by ordinary kriging over eight rays, "
                                             "with the kriging variance.")
    ap.add_argument("--dem", required=True, help="input .asc raster (NODATA_value cells are voids)")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = known, 0 = void")
    ap.add_argument("--nodata", type=float, help="nodata value (default: the .asc header's NODATA_value)")
    ap.add_argument("--model", choices=MODELS, default="power")
    ap.add_argument("--nugget", type=float, help="m^2, >= 0 (default 0)")
    ap.add_argument("--scale", type=float, help="power: m^2 per m^shape; else the sill above the nugget in m^2 (default 1)")
    ap.add_argument("--shape", type=float, help="power: the exponent in (0, 2); else the range in metres (default 1)")
    ap.add_argument("--max-distance", type=float, help="known cells farther than this many metres do not count")
    ap.add_argument("--no-fallback", action="store_true", help="leave the cells no ray serves unfilled")
    ap.add_argument("--out", required=True, help="output .asc raster")
    ap.add_argument("--variance-out", help="write the kriging variance (.asc, m^2)")
    ap.add_argument("--variogram-json", help="write the empirical variogram of the known cells and the model used here")
    return ap


def main(argv=None):
    from .asc import read_inputs, with_nodata, write_asc
    ap = build_parser()
    a = ap.parse_args(argv)
    given = any(v is not None for v in (a.nugget, a.scale, a.shape))
    if a.model != "power" and not given:
        ap.error("only the power model is fitted: give --nugget, --scale or --shape with --model " + a.model)
    vg = None
    if given:
        try:
            vg = Variogram(a.model, 0.0 if a.nugget is None else a.nugget, 1.0 if a.scale is None else a.scale,
                           1.0 if a.shape is None else a.shape)
        except ValueError as e:
            ap.error(str(e))
    dem, header, mask, nodata, cellsize = read_inputs(a)
    out, var, info = krige_voids(dem, mask, nodata=nodata, cellsize=cellsize, variogram=vg, max_distance=a.max_distance,
                                 fallback=None if a.no_fallback else "nearest")
    hdr = with_nodata(header) if info["unfilled"] else header
    write_asc(a.out, out.cpu().numpy(), hdr)
    if a.variance_out:
        write_asc(a.variance_out, var.cpu().numpy(), hdr)
    if a.variogram_json:
        emp = empirical_variogram(dem, mask, nodata=nodata, cellsize=cellsize)
        table = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in emp.items()}
        table["gamma"] = [None if g != g else g for g in table["gamma"]]
        with open(a.variogram_json, "w") as f:
            json.dump({"empirical": table, "variogram": info["variogram"], "fitted": info["fitted"]}, f, indent=1)
    v = info["variogram"]
    print(f"{a.out}: {info['unknown']} void pixels, {info['filled']} kriged ({info['by_nearest']} from the nearest known cell), "
          f"{info['unfilled']} left unfilled; {v['model']} variogram{' (fitted)' if info['fitted'] else ''} nugget {v['nugget']:.6g} "
          f"scale {v['scale']:.6g} shape {v['shape']:.6g}; largest variance {info['max_variance']:.6g} m2")
    return info


if __name__ == "__main__":
    main()
