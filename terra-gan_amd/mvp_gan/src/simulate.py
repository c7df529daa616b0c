"""Conditional simulation of the voids of a DEM on the GPU (csrc/simulate.hip): surfaces that keep the known
pixels bit for bit, have the raster's own variogram inside the voids and scatter around the kriged fill with the kriging variance.
Where krige_voids answers "what is the best estimate and how far off may it be", a realisation is one surface that could be there:
it can be routed, differenced and flooded, which a variance map cannot.

A realisation is conditioned by kriging, z_s = krige(z) + (u - krige(u)): u is an unconditional random field with the model
variogram on the raster's grid and both krigings use the samples of krige_voids (the first known pixels along eight rays), so the
weights are the same and u - krige(u) is a draw of the kriging error.

  spectral_waves      the integer wave table of u = sum_k a_k cos(2 pi (f_k . x + phase_k)): frequencies on a log-spaced spiral
                      from 1 / outer_px turn per pixel upwards, folded into |f| <= 1/2, squared amplitudes from the model's
                      spectral density, one global factor fitted to the model over the lags 1 .. 32 px.  Pure numpy, float64.
  realised_variogram  the closed-form variogram of a table: sum_k a_k^2 / 2 (1 - cos(2 pi f_k . h)) + nugget.
  simulate_voids      n realisations, their mean and standard deviation.  Realisation r draws its phases from (seed, r) and its
                      nugget noise from the hash stream (seed, r): it does not depend on how many are requested, and a tile with
                      its origin set gets the bits of the whole raster's u.

Two calls on the same inputs return bitwise-equal tensors.

CLI: python -m mvp_gan.src.simulate --dem in.asc --out sim_{r}.asc [--realisations n --seed s --mean-out m.asc --sd-out sd.asc]
         [--mask m.png|m.asc] [--nodata v] [--model power|exponential --nugget n --scale s --shape p] [--waves n]
         [--max-distance m] [--no-fallback]        ({r} in --out is the realisation's number; it is required with n > 1)
"""
import argparse
import math
from dataclasses import asdict

import numpy as np
import torch

from . import raster_args as R
from .interpolate import check_args
from .kriging import MODELS, VGM_OCTAVES, Variogram, assemble_variogram, check_variogram, fit_variogram

MAX_WAVES = 512                                           # TG_SIM_MAX_WAVES
MAX_REALISATIONS = 4096
FIT_LAGS = 32                                             # the global factor is fitted over the lags 1 .. 32 px
FOLD_TURNS = 4.0                                          # the rings reach this many turns per pixel before they fold
GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))
WAVE_DTYPE = np.dtype([("fx", "<i4"), ("fy", "<i4"), ("phase", "<u4"), ("amp", "<f4")])


def lag_vectors(lags=FIT_LAGS):
    """int64 [4 * lags][2] of (dy, dx): per lag L = 1 .. lags the steps (0, L), (L, 0) (axial) and (L, L), (L, -L) (diagonal),
    empirical_variogram's directions."""
    return np.array([v for L in range(1, lags + 1) for v in ((0, L), (L, 0), (L, L), (L, -L))], np.int64)


def _count(v, lo, hi, name, who):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{who}: {name} {v!r} must be an integer in [{lo}, {hi}]")
    return int(v)


def _cosine_sum(waves, lags):
    """sum_k a_k^2 / 2 (1 - cos(2 pi f_k . h)) per lag vector h (dy, dx) in pixels, float64; the phase f_k . h is reduced mod 1
    in integers first, so a long lag loses nothing."""
    lags = np.asarray(lags, np.int64).reshape(-1, 2)
    fx, fy = waves["fx"].astype(np.int64), waves["fy"].astype(np.int64)
    t = (fy[None, :] * lags[:, 0:1] + fx[None, :] * lags[:, 1:2]) & 0xffffffff
    a2 = waves["amp"].astype(np.float64) ** 2
    return (0.5 * a2[None, :] * (1.0 - np.cos(2.0 * np.pi * (t.astype(np.float64) / 2.0 ** 32)))).sum(1)


def realised_variogram(waves, nugget, lags):
    """gamma_N(h) of the field a wave table gives, float64 per lag vector (dy, dx) in pixels: sum_k a_k^2 / 2 (1 - cos(2 pi f_k .
    h)) + nugget, 0 at h = 0."""
    lags = np.asarray(lags, np.int64).reshape(-1, 2)
    return np.where((lags != 0).any(1), _cosine_sum(waves, lags) + np.float64(nugget), 0.0)


def spectral_waves(variogram, cellsize, waves=256, seed=0, outer_px=4096):
    """-> a WAVE_DTYPE array [waves] with phase 0: wave k has the frequency rho_k (cos th_k, sin th_k) in turns per pixel, rho_k
    log-spaced between 1 / outer_px and FOLD_TURNS (the middle of the k-th of `waves` rings), th_k = k * the golden angle + a
    rotation drawn from numpy.random.Generator(PCG64(seed)), stored as Q32 integers mod one turn: every stored |f| <= 1/2, and a
    ring above 1/2 turn per pixel folds onto the grid as sampling the continuous field folds it.  Without those rings the table
    lacks what a rough model has above the Nyquist frequency, a third of gamma(1 px) at shape 1.  a_k^2
    is proportional to the model's 2-D spectral density at omega = 2 pi rho_k / cellsize times the area of the ring, ~ rho_k^2:
    |omega|^-(2 + shape) for the power model, (1 / shape^2 + |omega|^2)^-3/2 for the exponential one.  One factor scales all
    a_k^2 so that realised_variogram matches the model's gamma above its nugget in least squares of the relative residual over
    lag_vectors().  The spherical model is refused.  variogram: a Variogram (or anything with its fields: a scale of 0 gives zero
    amplitudes).  Does not depend on the raster."""
    who = "spectral_waves"
    n = _count(waves, 1, MAX_WAVES, "waves", who)
    seed = _count(seed, 0, 2 ** 32 - 1, "seed", who)
    outer = _count(outer_px, 4, 1 << 30, "outer_px", who)
    c = R.cellsize(cellsize, who)
    model, scale, shape = variogram.model, float(variogram.scale), float(variogram.shape)
    if model == "spherical":
        raise ValueError(f"{who}: the spherical model has no usable spectral density; simulate with the power or the exponential "
                         "model")
    if model not in MODELS:
        raise ValueError(f"{who}: model {model!r} must be 'power' or 'exponential'")
    if not (math.isfinite(scale) and scale >= 0 and math.isfinite(shape) and shape > 0 and (model != "power" or shape < 2)):
        raise ValueError(f"{who}: scale {scale!r} must be >= 0 and shape {shape!r} lie in (0, 2) for the power model, else be > 0")
    k = np.arange(n, dtype=np.float64)
    lo, hi = 1.0 / outer, FOLD_TURNS
    rho = lo * (hi / lo) ** ((k + 0.5) / n)
    rot = np.random.Generator(np.random.PCG64(seed)).uniform(0.0, 2.0 * np.pi)
    th = k * GOLDEN_ANGLE + rot
    omega = 2.0 * np.pi * rho / c                                        # radians per metre
    dens = omega ** -(2.0 + shape) if model == "power" else (1.0 / shape ** 2 + omega ** 2) ** -1.5
    a2 = dens * rho * rho
    a2 = a2 / a2.max()
    out = np.zeros(n, WAVE_DTYPE)
    q = lambda v: (np.rint(v * 2.0 ** 32).astype(np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)    # mod one turn
    out["fx"], out["fy"] = q(rho * np.cos(th)), q(rho * np.sin(th))
    out["amp"] = np.sqrt(a2).astype(np.float32)
    if scale == 0:
        out["amp"] = 0
        return out
    lags = lag_vectors()
    g = _cosine_sum(out, lags)
    h = c * np.sqrt((lags.astype(np.float64) ** 2).sum(1))
    target = Variogram(model, 0.0, scale, shape).gamma(h)
    ratio = g / target                                                   # least squares of the relative residual factor * ratio - 1
    factor = float(ratio.sum() / (ratio * ratio).sum())
    out["amp"] = (np.sqrt(factor * a2)).astype(np.float32)
    return out


def realisation_phases(seed, realisation, n):
    """The uint32 phases of realisation r: numpy.random.Generator(PCG64([seed, r])), one draw of n words."""
    return np.random.Generator(np.random.PCG64([int(seed), int(realisation)])).integers(0, 2 ** 32, int(n), dtype=np.uint32)


def with_phases(table, seed, realisation):
    out = table.copy()
    out["phase"] = realisation_phases(seed, realisation, len(table))
    return out


def upload_waves(table, dev):
    """A WAVE_DTYPE array as the int32 [n][4] tensor tg_sim_field reads."""
    return torch.from_numpy(np.ascontiguousarray(table).view(np.int32).reshape(-1, 4).copy()).to(dev)


def check_sim_args(realisations, seed, waves, origin, who="simulate_voids"):
    n = _count(realisations, 1, MAX_REALISATIONS, "realisations", who)
    seed = _count(seed, 0, 2 ** 32 - 1, "seed", who)
    waves = _count(waves, 1, MAX_WAVES, "waves", who)
    try:
        y0, x0 = origin
    except (TypeError, ValueError):
        raise ValueError(f"{who}: origin {origin!r} must be (row, column)") from None
    return n, seed, waves, (_count(y0, 0, 2 ** 32 - 1, "origin row", who), _count(x0, 0, 2 ** 32 - 1, "origin column", who))


@torch.no_grad()
def simulate_voids(dem, mask=None, *, nodata=None, cellsize=1.0, variogram=None, realisations=1, seed=0, waves=256,
                   max_distance=None, fallback="nearest", keep=True, origin=(0, 0), table=None):
    """dem: float32 [H][W] (numpy or HIP tensor); mask: same shape, nonzero = known (optional).  Returns (sims float32 HIP tensor
    [n][H][W], or None with keep=False: the known pixels bit for bit, the voids simulated, NaN where krige_voids leaves NaN; mean,
    sd float32 HIP tensors [H][W] over the realisations, None with realisations == 1: sd is 0 on known pixels; info dict:
    krige_voids' counters, variogram, fitted, waves, seed, realisations, sd_mean and sd_max over the filled voids (None without
    sd)).  origin: the (row, column) of this raster's first pixel in a larger one, so that tiles share one field.  table: a
    WAVE_DTYPE array to use in place of spectral_waves' (its phases are replaced per realisation)."""
    from tg_hip import ops as O
    who = "simulate_voids"
    _, _, c, _, lim2, _ = check_args(dem, mask, "idw", 2.0, max_distance, cellsize, 0, fallback, who=who)
    check_variogram(variogram, who)
    n, seed, waves, origin = check_sim_args(realisations, seed, waves, origin, who)
    if variogram is not None and variogram.model == "spherical":
        raise ValueError(f"{who}: the spherical model has no usable spectral density; simulate with the power or the exponential "
                         "model")
    if table is not None and not (isinstance(table, np.ndarray) and table.dtype == WAVE_DTYPE and table.ndim == 1
                                  and 1 <= len(table) <= MAX_WAVES):
        raise ValueError(f"{who}: table must be a WAVE_DTYPE array of 1 .. {MAX_WAVES} waves")
    z, known = R.upload_known(dem, mask, nodata, who)
    fitted = variogram is None
    if fitted:
        counts, sums = O.variogram(z, known, VGM_OCTAVES)
        variogram, _ = fit_variogram(assemble_variogram(counts.cpu().numpy(), sums.cpu().numpy(), cellsize=c,
                                                        octaves=VGM_OCTAVES))
    if table is None:
        table = spectral_waves(variogram, c, waves, seed)
    nugget_amp = math.sqrt(variogram.nugget)
    _, counts, hits = O.rayfill(z, known, lim2, 2.0, want_hits=True)
    d2 = idx = None
    if counts.cpu().tolist()[2] and fallback == "nearest":
        d2, idx = O.edt_nearest(known, lim2 + 1 if lim2 else 0)
    vg = (c, variogram.model, variogram.nugget, variogram.scale, variogram.shape)
    zk, _, counts = O.krige(z, known, hits, *vg, d2, idx)
    by_rays, by_nearest, unfilled = counts.cpu().tolist()
    H, W = z.shape
    s1 = s2 = None
    if n > 1:
        s1 = torch.zeros(H, W, dtype=torch.float64, device=z.device)
        s2 = torch.zeros(H, W, dtype=torch.float64, device=z.device)
    sims = torch.empty(n, H, W, dtype=torch.float32, device=z.device) if keep else None
    for r in range(n):
        u = O.sim_field(H, W, upload_waves(with_phases(table, seed, r), z.device), origin, nugget_amp, seed, r)
        uk, _, _ = O.krige(u, known, hits, *vg, d2, idx)
        out = O.sim_combine(z, known, zk, u, uk, s1, s2)
        if keep:
            sims[r] = out
    mean = sd = sd_mean = sd_max = None
    if n > 1:
        mean, sd = O.sim_stats(zk, s1, s2, n)
        void = (known == 0) & ~torch.isnan(sd)
        if bool(void.any()):
            sd_mean, sd_max = float(sd[void].double().mean().item()), float(sd[void].max().item())
    filled = by_rays + by_nearest
    info = {"unknown": filled + unfilled, "filled": filled, "by_nearest": by_nearest, "unfilled": unfilled,
            "variogram": asdict(variogram), "fitted": fitted, "waves": len(table), "seed": seed, "realisations": n,
            "sd_mean": sd_mean, "sd_max": sd_max,
            "max_distance": None if max_distance is None else float(max_distance), "lim2": lim2 or None}
    return sims, mean, sd, info


# ---- CLI ------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="Draw conditional simulations of the voids of an ESRI ASCII grid DSM: kriged "
                                             "realisations with the raster's own variogram.")
    ap.add_argument("--dem", required=True, help="input .asc raster (NODATA_value cells are voids)")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = known, 0 = void")
    ap.add_argument("--nodata", type=float, help="nodata value (default: the .asc header's NODATA_value)")
    ap.add_argument("--model", choices=("power", "exponential"), default="power")
    ap.add_argument("--nugget", type=float, help="m^2, >= 0 (default 0)")
    ap.add_argument("--scale", type=float, help="power: m^2 per m^shape; else the sill above the nugget in m^2 (default 1)")
    ap.add_argument("--shape", type=float, help="power: the exponent in (0, 2); else the range in metres (default 1)")
    ap.add_argument("--realisations", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--waves", type=int, default=256, help=f"cosines of the random field, 1 .. {MAX_WAVES}")
    ap.add_argument("--max-distance", type=float, help="known cells farther than this many metres do not count")
    ap.add_argument("--no-fallback", action="store_true", help="leave the cells no ray serves unfilled")
    ap.add_argument("--out", required=True, help="output .asc raster; {r} is replaced by the realisation's number")
    ap.add_argument("--mean-out", help="write the mean of the realisations (.asc)")
    ap.add_argument("--sd-out", help="write their standard deviation (.asc, m)")
    return ap


def main(argv=None):
    from .asc import read_inputs, with_nodata, write_asc
    ap = build_parser()
    a = ap.parse_args(argv)
    given = any(v is not None for v in (a.nugget, a.scale, a.shape))
    if a.model != "power" and not given:
        ap.error("only the power model is fitted: give --nugget, --scale or --shape with --model " + a.model)
    if a.realisations > 1 and "{r}" not in a.out:
        ap.error("--out needs {r} with more than one realisation")
    if a.realisations < 2 and (a.mean_out or a.sd_out):
        ap.error("--mean-out and --sd-out need at least two realisations")
    vg = None
    try:
        if given:
            vg = Variogram(a.model, 0.0 if a.nugget is None else a.nugget, 1.0 if a.scale is None else a.scale,
                           1.0 if a.shape is None else a.shape)
        check_sim_args(a.realisations, a.seed, a.waves, (0, 0))
    except ValueError as e:
        ap.error(str(e))
    dem, header, mask, nodata, cellsize = read_inputs(a)
    sims, mean, sd, info = simulate_voids(dem, mask, nodata=nodata, cellsize=cellsize, variogram=vg, realisations=a.realisations,
                                          seed=a.seed, waves=a.waves, max_distance=a.max_distance,
                                          fallback=None if a.no_fallback else "nearest")
    hdr = with_nodata(header) if info["unfilled"] else header
    for r in range(a.realisations):
        write_asc(a.out.replace("{r}", str(r)), sims[r].cpu().numpy(), hdr)
    if a.mean_out:
        write_asc(a.mean_out, mean.cpu().numpy(), hdr)
    if a.sd_out:
        write_asc(a.sd_out, sd.cpu().numpy(), hdr)
    v = info["variogram"]
    spread = "" if info["sd_mean"] is None else f"; sd over the voids mean {info['sd_mean']:.6g} m, max {info['sd_max']:.6g} m"
    print(f"{a.out}: {info['realisations']} realisations of {info['unknown']} void pixels, {info['filled']} simulated "
          f"({info['by_nearest']} from the nearest known cell), {info['unfilled']} left unfilled; {v['model']} variogram"
          f"{' (fitted)' if info['fitted'] else ''} nugget {v['nugget']:.6g} scale {v['scale']:.6g} shape {v['shape']:.6g}, "
          f"{info['waves']} waves, seed {info['seed']}{spread}")
    return info


if __name__ == "__main__":
    main()
