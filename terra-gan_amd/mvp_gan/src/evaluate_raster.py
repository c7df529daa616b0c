"""Score inpainting on held-out raster blocks: terrain errors in metres on the GPU (csrc/terrain_eval.hip).

The reference scores 8-bit tiles only, and this project's tile metrics (PSNR, SSIM, boundary MSE) are unitless.  Here holes
are cut into measured terrain of the held-out blocks, the holed raster is inpainted with inpaint_raster unchanged, and the
result is compared against the truth:

  - valid pixel V: mask != 0, finite, != nodata (the rule of inpaint_raster); Obj: the object_mask map (with `objects`);
  - hole cells: a grid of `tile`-px cells aligned at (0, 0), block % tile == 0; a cell is eligible when its block (by, bx)
    has (bx - by) mod 3 == SPLITS[split] (RasterWindowLoader's rule: with the same block, test cells never share a pixel with
    a training window); split None: every cell;
  - the holes of a cell are RasterWindowLoader's primitives at side `tile`, drawn from
    SeedSequence([seed, 7, split tag, cy, cx]) (tag 3 for split None) and rasterised by tg_hole_masks, clipped to the raster;
    so a cell's holes do not depend on the raster's extent;
  - Hol = V and cell hole and not Obj; K = V and not Hol and not Obj (the mask inpaint_raster sees); Obj pixels are filled but
    never scored;
  - S = Hol and finite(p); e = p - z (fp32), a = |e|; T = S pixels whose 3x3 neighbourhood lies inside the raster, is valid and
    has finite p: slope (Horn, fp64, degrees), gradient and 5-point Laplacian errors; ring R = S pixels with an 8-neighbour
    in K;
  - holes = 8-connected components of Hol (label = smallest linear index); area classes by pixels * cellsize^2;
  - per-hole sums are sum rint(min(a, 2^15) * 2^16) in int64 (exact, order-independent; < 8 um per pixel);
  - quantiles by nearest rank: sorted ascending, element ceil(q n) - 1, selected exactly on the GPU.

With depth_edges_m (metres, e.g. DEPTH_EDGES_M) the report also says how deep into the holes the errors sit: the exact Euclidean
distance of every pixel to the nearest pixel of K (csrc/edt.hip; capped at the last edge, beyond which
every pixel is in the last class anyway) puts each scored pixel into a depth class, report["by_depth"] = {"cap_m", "classes":
[{"lo_m", "hi_m", "pixels", "mae", "rmse", "max"}]}, and each entry of holes["worst"] gains "depth_m", the hole's largest
distance to K (saturating at cap_m).  Without it the report has neither key and no further kernel runs.

Two calls on the same inputs return bitwise-equal tensors and an equal report.

With baseline="laplace" the same keep mask is also filled by harmonic interpolation (fill_voids; with
baseline="biharmonic" by the minimum-curvature fill of section 8q, the stronger baseline on slope and curvature) and
report["baseline"] holds that fill's full terrain_errors report on the same holes, plus "method" and the fill info: the number
a GAN has to beat.  fallback and seam are passed to inpaint_raster; with seam="harmonic" report["seam"] holds the info of the
seam correction (mvp_gan/src/seam_correct.py), and the ring errors show what it did.

With compare=("idw", "nearest") the same keep mask is also filled by interpolate_voids with its defaults (mvp_gan/src/interpolate.py,
DESIGN.md section 8t: the cheap end of the baseline ladder) and report["compare"][name] holds that fill's terrain_errors report
on the same holes and depth classes, plus "method" and the fill info under "fill".  Without it the report has no "compare" key.

With sinks=True the report also says whether a fill drains (sink_errors; mvp_gan/src/fill_depressions.py):
the depressions of the truth and of the fill are filled over the same known pixels, and report["sinks"] = {"truth", "pred":
{"cells", "volume_m3", "max_depth_m", "depressions", "converged"}, "excess_volume_m3", "excess_cells"} counts the closed pits
inside the holes; report["baseline"] and every report["compare"][name] gain the same key for their fills.  Without it the report
has no "sinks" key and nothing more runs.

With drainage=True the report also says whether water crosses a fill the way it crosses the true terrain (drainage_errors;
mvp_gan/src/flow_routing.py): both surfaces are routed over the same known pixels, and report["drainage"]
compares their D8 directions, outlets, contributing areas and stream networks (accumulation >= stream_cells) inside the holes, in
integers; report["baseline"] and every report["compare"][name] gain the same key.  Without it the report has no "drainage" key
and nothing more runs.

With flood=True the report also says whether a flood map made from a fill wets the ground that one made from the true terrain
wets (flood_errors): both surfaces are routed as above, each side's height above its nearest drainage (HAND;
streams of stream_cells cells) is taken, and report["flood"] compares the two HAND planes and the flood extents HAND <= stage at
flood_stages_m inside the holes, in integers; report["baseline"] and every report["compare"][name] gain the same key.  Without it
the report has no "flood" key and nothing more runs.

With wetness=True the report also says whether a fill keeps the hillslopes (wetness_errors): both surfaces
are routed as above, each side's topographic wetness index ln(a / tan(beta)) is taken from a multiple-flow-direction accumulation
and Horn's slope, and report["wetness"] holds the bias, MAE, RMSE and largest difference of the two inside the holes;
report["baseline"] and every report["compare"][name] gain the same key.  Without it the report has no "wetness" key and nothing
more runs.

With texture=True the report also says whether a fill has the relief of the terrain at each scale (texture_errors; DESIGN.md
section 8ad): the second differences of the fill and of the truth over the same triples of pixels centred in the holes, at the lags
1, 2, .. 2^(texture_octaves - 1) px along the axes and along the diagonals, and report["texture"] holds per scale the RMS of both,
their ratio and their correlation; report["baseline"] and every report["compare"][name] gain the same key.  Without it the report
has no "texture" key and nothing more runs.

With kriging=True (or a kriging.Variogram) the same keep mask is also filled by ordinary kriging (krige_voids; mvp_gan/src/kriging.py,
DESIGN.md section 8ae; True fits the power variogram to the kept pixels) and report["kriging"] holds that fill's terrain_errors report
on the same holes and depth classes, "method", the fill info under "fill", the model under "variogram", every optional row above by
the same calls, and "calibration" = {"cells", "mean_z2", "within_1sigma", "within_2sigma"}: over the scored pixels with a finite
variance > 0, z^2 = error^2 / variance, its mean and the shares with |error| <= sigma and <= 2 sigma.  Without it the report has no
"kriging" key and nothing more runs.

With simulate=n (n >= 2) the same keep mask is also simulated n times (simulate_voids; mvp_gan/src/simulate.py, DESIGN.md section
8ah) and report["simulation"] holds the terrain_errors report of the mean of the realisations on the same holes and depth classes,
"calibration" of their sd^2, "texture" of realisation 0 (the row that kriging's smooth fill fails), "variogram" and "realisations".
Without it the report has no "simulation" key and nothing more runs.

With natural=True the same keep mask is also filled by natural-neighbour interpolation (natural_neighbour_voids; mvp_gan/src/natural.py,
DESIGN.md section 8ai; natural_radius cells) and report["natural"] holds that fill's terrain_errors report on the same holes and depth
classes, "method", the fill info under "fill" and every optional row above by the same calls.  Without it the report has no
"natural" key and nothing more runs.

CLI: python -m mvp_gan.src.evaluate_raster --dem in.asc --checkpoint ck.pth [--mask m] [--nodata v]
         [--split test|val|train|all] [--block 1024 --tile 256 --seed 0] [--window 512 --overlap 64 --batch 16]
         [--remove-objects [spec flags]] [--json report.json] [--pred-out pred.asc] [--holes-out holes.png|holes.asc]
         [--baseline laplace|biharmonic] [--fallback laplace] [--seam harmonic] [--solver mg|pcg] [--model-cellsize 1.0 [--min-coverage 0.5]]
         [--by-depth [E ...]] [--compare idw nearest] [--sinks] [--drainage [--stream-cells n] [--stream-tol m]]
         [--flood [--flood-stages s ...]] [--wetness [--exponent e] [--min-slope s]]
         [--texture [--octaves n]] [--kriging] [--tta 2|4|8] [--simulate n] [--natural [--natural-radius r]]
     python -m mvp_gan.src.evaluate_raster --dem in.asc --pred filled.asc --holes holes.png [...]   (score another fill)
"""
import argparse
import json
import math
from dataclasses import asdict

import numpy as np
import torch

from . import raster_args as R
from .utils.raster_dataset import SPLITS, HoleSpec, fit_primitives, primitive_draws

MIN_TILE, MAX_TILE = 40, 1024
AREA_EDGES_M2 = (100.0, 1000.0, 10000.0)
QUANTILES = (0.5, 0.9, 0.95, 0.99)
DEPTH_EDGES_M = (2.0, 5.0, 10.0, 25.0, 50.0)      # --by-depth given bare: class bounds in metres from the known terrain
FIX = 2.0 ** 16                       # fixed-point scale of the per-hole sums
CLAMP = 2.0 ** 15                     # metres: larger per-pixel errors are clamped in the per-hole sums
MAX_CLASSES = 8
BATCH_BYTES = 256 << 20               # cell masks rasterised per batch
WHO = "evaluate_raster"               # the name at the head of every device and upload message of this module
HOLE_COLS = ("label", "area", "scored", "sum", "max", "y0", "x0", "y1", "x1")
SUMS = ("s_e", "s_a", "s_a2", "t_ds", "t_ds2", "t_dg2", "t_dl2", "r_a", "r_a2", "rt_dg2")     # then per class: a, a^2
COUNTS = ("valid", "holes", "objects", "scored", "unfilled", "ring", "slope_scored", "ring_slope", "clamped", "max_bits")


# ---- host-side plan -------------------------------------------------------------------------------------------------
def check_plan(H, W, split, block, tile, holes, who="eval_holes"):
    if split is not None and split not in SPLITS:
        raise ValueError(f"{who}: split {split!r} must be None or one of {tuple(SPLITS)}")
    tile, block = int(tile), int(block)
    if not MIN_TILE <= tile <= MAX_TILE:
        raise ValueError(f"{who}: tile {tile} out of range [{MIN_TILE}, {MAX_TILE}]")
    if block < tile or block % tile:
        raise ValueError(f"{who}: block {block} must be a positive multiple of the tile {tile}")
    holes.check(tile)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"{who}: raster must be [H, W] with H*W < 2^31, got {H}x{W}")
    return tile, block


def eligible_cells(H, W, split, block, tile):
    """bool [ceil(H / tile)][ceil(W / tile)]: the cells that get holes."""
    ncy, ncx = -(-H // tile), -(-W // tile)
    if split is None:
        return np.ones((ncy, ncx), bool)
    by = (np.arange(ncy) * tile // block)[:, None]
    bx = (np.arange(ncx) * tile // block)[None, :]
    return (bx - by) % 3 == SPLITS[split]


def native_cells(block, tile, scale, who="evaluate_raster"):
    """Block and tile sides counted in working pixels of `scale` (working / native cell size, a Fraction, or None for the
    native grid itself) -> the same ground lengths in native pixels.  RasterWindowLoader(model_cellsize=...) picks its blocks
    on the working grid: working block b covers native pixels [b block scale, (b + 1) block scale), so with the block and
    the tile converted here the native blocks are the loader's, index for index, and eligible_cells keeps its promise that a
    test cell shares no pixel with the ground of a train or val block.  ValueError when a side is no whole number of native
    pixels."""
    if scale is None:
        return int(block), int(tile)
    b, t = int(block) * scale, int(tile) * scale
    if b.denominator != 1 or t.denominator != 1:
        raise ValueError(f"{who}: block {block} and tile {tile} working pixels at scale {scale} are {b} and {t} native pixels; "
                         f"both must be whole numbers for the held-out cells to match the training blocks")
    return int(b), int(t)


def cell_rng(seed, split, cy, cx):
    tag = 3 if split is None else SPLITS[split]
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), 7, tag, int(cy), int(cx)])))


def cell_primitives(seed, split, cells, tile, holes):
    """-> (prims int32 [P][8], offsets int32 [n+1]) of the cells [(cy, cx)]: draw_primitives(cell_rng(...), 1, tile, holes)
    per cell, the draws made per cell and fitted in one vectorised pass."""
    draws = [primitive_draws(cell_rng(seed, split, cy, cx), 1, tile, holes) for cy, cx in cells]
    d = {k: np.concatenate([x[k] for x in draws]) for k in draws[0]}
    return fit_primitives(d, tile, holes)


def class_px(edges_m2, cellsize):
    """The smallest area in pixels of each class above the first: min px with px * cellsize^2 >= edge."""
    c2 = cellsize * cellsize
    out = []
    for e in edges_m2:
        t = max(0, math.floor(e / c2) - 2)
        while t * c2 < e:
            t += 1
        out.append(t)
    return out


def _check_edges(edges):
    edges = [float(e) for e in edges]
    if len(edges) > MAX_CLASSES - 1 or any(not math.isfinite(e) or e <= 0 for e in edges) or edges != sorted(edges):
        raise ValueError(f"terrain_errors: area_edges_m2 {edges} must be at most {MAX_CLASSES - 1} increasing finite values > 0")
    return edges


def _check_depth_edges(edges):
    """None, or 1 .. MAX_CLASSES - 1 strictly increasing finite distances in metres > 0."""
    if edges is None:
        return None
    try:
        edges = [float(e) for e in edges]
    except (TypeError, ValueError):
        raise ValueError(f"terrain_errors: depth_edges_m {edges!r} must be a sequence of numbers") from None
    if not 1 <= len(edges) <= MAX_CLASSES - 1 or any(not math.isfinite(e) or e <= 0 for e in edges) or \
            any(b <= a for a, b in zip(edges, edges[1:])):
        raise ValueError(f"terrain_errors: depth_edges_m {edges} must be 1 .. {MAX_CLASSES - 1} increasing finite values > 0")
    return edges


def _check_quantiles(qs):
    qs = [float(q) for q in qs]
    if not 1 <= len(qs) <= 8 or any(not 0 < q <= 1 for q in qs):
        raise ValueError(f"terrain_errors: quantiles {qs} must be 1 .. 8 values in (0, 1]")
    return qs


def rank(q, n):
    """0-based nearest rank of quantile q among n sorted values."""
    return min(max(math.ceil(q * n) - 1, 0), n - 1)


# ---- evaluation holes -----------------------------------------------------------------------------------------------
@torch.no_grad()
def eval_holes(dem, mask=None, *, nodata=None, split="test", block=1024, tile=256, holes=HoleSpec(), seed=0, objects=None,
               cellsize=None):
    """-> (holes uint8 [H][W] = Hol, keep float32 [H][W] = K, info) as HIP tensors; info: cells, valid, holes, objects,
    and with `objects` the object_mask info under "object_mask"."""
    from tg_hip import ops as O
    H, W = R.raster_shape(dem, mask, "eval_holes")
    tile, block = check_plan(H, W, split, block, tile, holes)
    if objects is not None:
        cellsize = R.cellsize(cellsize, "eval_holes")
    z, m, nodata, device = R.upload(dem, mask, nodata, WHO)
    obj, oinfo = None, None
    if objects is not None:
        from .object_mask import object_mask
        obj, _, oinfo = object_mask(z, m, nodata=nodata, cellsize=cellsize, spec=objects)
    el = eligible_cells(H, W, split, block, tile)
    ncy, ncx = el.shape
    cell_of = np.full((ncy, ncx), -1, np.int32)
    hmap = torch.empty(H, W, dtype=torch.uint8, device=device)
    keep = torch.empty(H, W, dtype=torch.float32, device=device)
    counts = torch.zeros(3, dtype=torch.int64, device=device)
    cap = max(1, min(BATCH_BYTES // (4 * tile * tile), 65535))
    if int(el.sum(1).max()) > cap:
        raise ValueError(f"eval_holes: {int(el.sum(1).max())} cells in one row of {tile}-px cells, more than {cap} per batch")
    cy0 = 0
    while cy0 < ncy:
        cy1, n = cy0, 0
        while cy1 < ncy and n + int(el[cy1].sum()) <= cap:
            n += int(el[cy1].sum())
            cy1 += 1
        cells = np.argwhere(el[cy0:cy1]) + [cy0, 0]
        masks, cof = None, None
        if len(cells):
            cell_of[cells[:, 0], cells[:, 1]] = np.arange(len(cells), dtype=np.int32)
            prims, offsets = cell_primitives(seed, split, cells.tolist(), tile, holes)
            pd = torch.from_numpy(prims).to(device)
            masks = O.hole_masks(pd, torch.from_numpy(offsets).to(device), tile)
            cof = torch.from_numpy(cell_of).to(device)
        O.eval_holes(z, m, nodata, obj, masks, cof, tile, cy0 * tile, min(cy1 * tile, H), hmap, keep, counts)
        cy0 = cy1
    c = counts.cpu().tolist()
    info = {"cells": int(el.sum()), "valid": c[0], "holes": c[1], "objects": c[2]}
    if oinfo is not None:
        info["object_mask"] = oinfo
    return hmap, keep, info


@torch.no_grad()
def holes_from_map(dem, hole_map, mask=None, *, nodata=None, objects=None, cellsize=None):
    """Holes given as a map (nonzero = hole, e.g. the --holes-out of an earlier run) -> (holes uint8, keep float32, info) with
    the rules of eval_holes: Hol = V and hole and not Obj, K = V and not hole and not Obj."""
    from tg_hip import ops as O
    H, W = R.raster_shape(dem, mask, "holes_from_map")
    if R.shape(hole_map) != (H, W):
        raise ValueError(f"holes_from_map: hole map {R.shape(hole_map)} differs from the dem {(H, W)}")
    if objects is not None:
        cellsize = R.cellsize(cellsize, "holes_from_map")
    z, m, nodata, device = R.upload(dem, mask, nodata, WHO)
    obj, oinfo = None, None
    if objects is not None:
        from .object_mask import object_mask
        obj, _, oinfo = object_mask(z, m, nodata=nodata, cellsize=cellsize, spec=objects)
    hmap = torch.empty(H, W, dtype=torch.uint8, device=device)
    keep = torch.empty(H, W, dtype=torch.float32, device=device)
    counts = torch.zeros(3, dtype=torch.int64, device=device)
    O.eval_holes(z, m, nodata, obj, None, None, MAX_TILE, 0, H, hmap, keep, counts,
                 hole_in=R.to_u8(hole_map, device, "hole map", WHO, nonzero=True, reuse=True))
    c = counts.cpu().tolist()
    info = {"cells": 0, "valid": c[0], "holes": c[1], "objects": c[2]}
    if oinfo is not None:
        info["object_mask"] = oinfo
    return hmap, keep, info


# ---- the report -----------------------------------------------------------------------------------------------------
def _mean(s, n):
    return float(s) / n if n else math.nan


def _rms(s, n):
    return math.sqrt(float(s) / n) if n else math.nan


def assemble_report(counts, sums, table, qa, qs, *, cellsize, edges_m2, quantiles, top, depth=None):
    """The report from the raw results: counts {COUNTS}, sums {SUMS + class_a / class_a2 lists}, table int64 [n][9] sorted by
    label, qa: the height quantile values, qs: the slope error p90.  depth (optional): {"edges_m", "cap_d2", "counts",
    "sum_a", "sum_a2", "max_bits": one per depth class, "hole_d2": the largest squared pixel distance per row of table}."""
    c2 = cellsize * cellsize
    n = counts
    ns, nt, nr, nrt = n["scored"], n["slope_scored"], n["ring"], n["ring_slope"]
    rep = {"pixels": {k: int(n[k]) for k in ("valid", "holes", "scored", "unfilled", "ring", "slope_scored", "objects",
                                              "clamped")}}
    h = {"bias": _mean(sums["s_e"], ns), "mae": _mean(sums["s_a"], ns), "rmse": _rms(sums["s_a2"], ns),
         "max": R.bits_f32(n["max_bits"]) if ns else math.nan,
         "quantiles": {repr(q): float(v) for q, v in zip(quantiles, qa)}}
    h["le90"] = h["quantiles"].get(repr(0.9), math.nan)
    rep["height"] = h
    rep["slope_deg"] = {"mae": _mean(sums["t_ds"], nt), "rmse": _rms(sums["t_ds2"], nt), "p90": float(qs),
                        "gradient_rmse": _rms(sums["t_dg2"], nt), "laplacian_rmse": _rms(sums["t_dl2"], nt)}
    rep["ring"] = {"mae": _mean(sums["r_a"], nr), "rmse": _rms(sums["r_a2"], nr), "gradient_rmse": _rms(sums["rt_dg2"], nrt)}
    table = np.asarray(table, np.int64).reshape(-1, len(HOLE_COLS))
    px = class_px(edges_m2, cellsize)
    cls = np.zeros(len(table), np.int64)
    for t in px:
        cls += table[:, 1] >= t
    bounds = [0.0] + list(edges_m2) + [math.inf]
    rep["by_area"] = []
    for k in range(len(edges_m2) + 1):
        sel = cls == k
        npx = int(table[sel, 2].sum())
        rep["by_area"].append({"lo_m2": bounds[k], "hi_m2": bounds[k + 1], "holes": int(sel.sum()), "pixels": npx,
                               "mae": _mean(sums["class_a"][k], npx), "rmse": _rms(sums["class_a2"][k], npx)})
    sc = table[:, 2]
    mae = np.where(sc > 0, table[:, 3] / FIX / np.maximum(sc, 1), -1.0)
    order = [i for i in np.lexsort((table[:, 0], -mae)) if sc[i] > 0][:int(top)]
    rep["holes"] = {"count": int(len(table)), "worst": [
        {"label": int(table[i, 0]), "bbox": [int(v) for v in table[i, 5:9]], "area_m2": float(table[i, 1]) * c2,
         "scored": int(sc[i]), "mae": float(mae[i]), "max": R.bits_f32(table[i, 4])} for i in order]}
    if depth is not None:
        from .distance import px2_m
        db = [0.0] + list(depth["edges_m"]) + [math.inf]
        rep["by_depth"] = {"cap_m": px2_m(depth["cap_d2"], cellsize), "classes": [
            {"lo_m": db[k], "hi_m": db[k + 1], "pixels": int(depth["counts"][k]),
             "mae": _mean(depth["sum_a"][k], int(depth["counts"][k])), "rmse": _rms(depth["sum_a2"][k], int(depth["counts"][k])),
             "max": R.bits_f32(depth["max_bits"][k]) if depth["counts"][k] else math.nan} for k in range(len(db) - 1)]}
        for h, i in zip(rep["holes"]["worst"], order):
            h["depth_m"] = px2_m(int(depth["hole_d2"][i]), cellsize)
    return rep


@torch.no_grad()
def terrain_errors(dem, pred, holes, keep, *, cellsize, mask=None, nodata=None, area_edges_m2=AREA_EDGES_M2,
                   quantiles=QUANTILES, top=10, depth_edges_m=None):
    """The report (a plain dict json.dump can write) of pred against the truth dem on the holes; model-free, so any fill can be
    scored on the same holes.  holes: nonzero = evaluation hole; keep: nonzero = known to the model.  depth_edges_m: class
    bounds in metres of the distance to the nearest pixel of K (valid and keep) for "by_depth"; None: no such section."""
    from tg_hip import ops as O
    c = R.cellsize(cellsize, "terrain_errors")
    H, W = R.raster_shape(dem, mask, "terrain_errors")
    for t, nm in ((pred, "pred"), (holes, "holes"), (keep, "keep")):
        if R.shape(t) != (H, W):
            raise ValueError(f"terrain_errors: {nm} {R.shape(t)} differs from the dem {(H, W)}")
    edges = _check_edges(area_edges_m2)
    qs = _check_quantiles(quantiles)
    dedges = _check_depth_edges(depth_edges_m)
    if dedges is not None:
        from .distance import MAX_SIDE, depth_px2
        if max(H, W) > MAX_SIDE:
            raise ValueError(f"terrain_errors: depth_edges_m needs sides of at most {MAX_SIDE} px, got {H}x{W}")
        dpx2 = depth_px2(dedges, c, "terrain_errors: depth_edges_m")
    if int(top) < 0:
        raise ValueError(f"terrain_errors: top {top} < 0")
    device = R.device(WHO)
    z, p = R.to_f32(dem, device, "dem", WHO), R.to_f32(pred, device, "pred", WHO)
    hm = R.to_u8(holes, device, "holes", WHO, nonzero=True, reuse=True)
    k = R.to_f32(keep, device, "keep", WHO, binary=True)
    m = None if mask is None else R.to_f32(mask, device, "mask", WHO, binary=True)
    nodata = R.nodata_value(nodata)

    labels, area = O.objmask_components(hm)
    cap = 4096
    while True:
        table, slot, count = O.hole_table(labels, area, cap, slot=None)
        nh = int(count.item())
        if nh <= cap:
            break
        cap = nh
    table = table[:nh]
    sums, counts, sel_a, sel_s = O.terrain_errors(z, p, m, nodata, hm, k, labels, slot, table, c, class_px(edges, c))
    cn = dict(zip(COUNTS, counts.cpu().tolist()))
    s = sums.cpu().numpy()
    sd = dict(zip(SUMS, s[:len(SUMS)].tolist()))
    ncls = len(edges) + 1
    sd["class_a"] = s[len(SUMS)::2][:ncls].tolist()
    sd["class_a2"] = s[len(SUMS) + 1::2][:ncls].tolist()
    ns, nt = cn["scored"], cn["slope_scored"]
    qa = O.select_f32(sel_a, [rank(q, ns) for q in qs]).cpu().tolist() if ns else [math.nan] * len(qs)
    q90 = O.select_f32(sel_s, [rank(0.9, nt)]).cpu().tolist()[0] if nt else math.nan
    tb = table.cpu().numpy()
    by_label = np.argsort(tb[:, 0], kind="stable")
    tb = tb[by_label]
    depth = None
    if dedges is not None:
        seeds, _ = O.objmask_known(z, k, nodata, transposed=False)          # K: valid and kept
        d2, _ = O.edt(seeds, dpx2[-1])
        dsums, dcounts, dmax, hole_d2 = O.depth_errors(sel_a, d2, labels, slot, nh, dpx2)
        ds = dsums.cpu().numpy()
        depth = {"edges_m": dedges, "cap_d2": dpx2[-1], "counts": dcounts.cpu().tolist(), "sum_a": ds[0::2].tolist(),
                 "sum_a2": ds[1::2].tolist(), "max_bits": (dmax.cpu().numpy().view(np.uint32)).tolist(),
                 "hole_d2": hole_d2.cpu().numpy()[by_label]}
    return assemble_report(cn, sd, tb, qa, q90, cellsize=c, edges_m2=edges, quantiles=qs, top=top, depth=depth)


# ---- end to end -----------------------------------------------------------------------------------------------------
BASELINES = ("laplace", "biharmonic")
FLOOD_STAGES_M = (0.5, 1.0, 2.0, 5.0)                  # the default stages of flood_errors
FLOOD_MAX_STAGES = 8                                   # TG_FLOOD_MAX_STAGES


def _check_fill_options(baseline, fallback, who="evaluate_raster"):
    if baseline is not None and baseline not in BASELINES:
        raise ValueError(f"{who}: baseline {baseline!r} must be None or one of {BASELINES}")
    if fallback not in (None, "laplace"):
        raise ValueError(f"{who}: fallback {fallback!r} must be None or 'laplace'")


@torch.no_grad()
def baseline_report(dem, holes, keep, *, cellsize, mask=None, nodata=None, method="laplace", area_edges_m2=AREA_EDGES_M2,
                    quantiles=QUANTILES, top=10, solver="mg", depth_edges_m=None, sinks=False, drainage=False, stream_cells=1000,
                    stream_tol_m=None, flood=False, flood_stages_m=FLOOD_STAGES_M, wetness=False, wetness_exponent=1,
                    wetness_min_slope=1e-3, texture=False, texture_octaves=5):
    """The baseline fill of the keep mask (fill_voids) scored on the holes: terrain_errors' report plus "method" and the
    fill info under "fill"; with sinks also sink_errors' dict under "sinks", with drainage drainage_errors' under "drainage",
    with flood flood_errors' under "flood", with wetness wetness_errors' under "wetness", with texture texture_errors' under
    "texture"."""
    from .fill_voids import fill_voids
    device = R.device(WHO)
    z = R.to_f32(dem, device, "dem", WHO)
    k = R.to_f32(keep, device, "keep", WHO, binary=True)
    bpred, finfo = fill_voids(z, k, nodata=R.nodata_value(nodata), method=method, solver=solver)
    rep = terrain_errors(z, bpred, holes, k, cellsize=cellsize, mask=mask, nodata=nodata, area_edges_m2=area_edges_m2,
                         quantiles=quantiles, top=top, depth_edges_m=depth_edges_m)
    rep["method"] = method
    rep["fill"] = finfo
    if sinks:
        rep["sinks"] = sink_errors(z, bpred, holes, cellsize=cellsize, mask=mask, nodata=nodata)
    if drainage:
        rep["drainage"] = drainage_errors(z, bpred, holes, cellsize=cellsize, mask=mask, nodata=nodata, stream_cells=stream_cells,
                                          stream_tol_m=stream_tol_m)
    if flood:
        rep["flood"] = flood_errors(z, bpred, holes, cellsize=cellsize, mask=mask, nodata=nodata, stream_cells=stream_cells,
                                    stages_m=flood_stages_m)
    if wetness:
        rep["wetness"] = wetness_errors(z, bpred, holes, cellsize=cellsize, mask=mask, nodata=nodata, exponent=wetness_exponent,
                                        min_slope=wetness_min_slope)
    if texture:
        rep["texture"] = texture_errors(z, bpred, holes, cellsize=cellsize, mask=mask, nodata=nodata, octaves=texture_octaves)
    return rep


COMPARES = ("idw", "nearest")


def _check_compare(compare, who="evaluate_raster"):
    """None, or a sequence of distinct names out of COMPARES -> a tuple (empty for None)."""
    if compare is None:
        return ()
    if isinstance(compare, str):
        compare = (compare,)
    try:
        names = tuple(compare)
    except TypeError:
        raise ValueError(f"{who}: compare {compare!r} must be None or a sequence out of {COMPARES}") from None
    if any(n not in COMPARES for n in names) or len(set(names)) != len(names):
        raise ValueError(f"{who}: compare {compare!r} must be None or distinct names out of {COMPARES}")
    return names


def assemble_compare(reports, infos, sinks=None, drainage=None, flood=None, wetness=None, texture=None):
    """{name: report + "method" + "fill"} from the terrain_errors reports and the interpolate_voids infos by name; with sinks
    ({name: sink_errors' dict}) also "sinks", with drainage ({name: drainage_errors' dict}) also "drainage", with flood ({name:
    flood_errors' dict}) also "flood", with wetness ({name: wetness_errors' dict}) also "wetness", with texture ({name: texture_errors'
    dict}) also "texture"."""
    out = {}
    for name, rep in reports.items():
        out[name] = dict(rep)
        out[name]["method"] = name
        out[name]["fill"] = infos[name]
        if sinks is not None:
            out[name]["sinks"] = sinks[name]
        if drainage is not None:
            out[name]["drainage"] = drainage[name]
        if flood is not None:
            out[name]["flood"] = flood[name]
        if wetness is not None:
            out[name]["wetness"] = wetness[name]
        if texture is not None:
            out[name]["texture"] = texture[name]
    return out


@torch.no_grad()
def compare_report(dem, holes, keep, names, *, cellsize, mask=None, nodata=None, area_edges_m2=AREA_EDGES_M2,
                   quantiles=QUANTILES, top=10, depth_edges_m=None, sinks=False, drainage=False, stream_cells=1000,
                   stream_tol_m=None, flood=False, flood_stages_m=FLOOD_STAGES_M, wetness=False, wetness_exponent=1,
                   wetness_min_slope=1e-3, texture=False, texture_octaves=5):
    """The interpolate_voids fills `names` of the keep mask, each scored on the holes like baseline_report's fill."""
    from .interpolate import interpolate_voids
    device = R.device(WHO)
    z = R.to_f32(dem, device, "dem", WHO)
    k = R.to_f32(keep, device, "keep", WHO, binary=True)
    reports, infos, snk, drn, fld, wet, tex = {}, {}, {}, {}, {}, {}, {}
    for name in _check_compare(names):
        pred, infos[name] = interpolate_voids(z, k, nodata=R.nodata_value(nodata), method=name, cellsize=cellsize)
        reports[name] = terrain_errors(z, pred, holes, k, cellsize=cellsize, mask=mask, nodata=nodata,
                                       area_edges_m2=area_edges_m2, quantiles=quantiles, top=top, depth_edges_m=depth_edges_m)
        if sinks:
            snk[name] = sink_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata)
        if drainage:
            drn[name] = drainage_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, stream_cells=stream_cells,
                                        stream_tol_m=stream_tol_m)
        if flood:
            fld[name] = flood_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, stream_cells=stream_cells,
                                     stages_m=flood_stages_m)
        if wetness:
            wet[name] = wetness_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, exponent=wetness_exponent,
                                       min_slope=wetness_min_slope)
        if texture:
            tex[name] = texture_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, octaves=texture_octaves)
    return assemble_compare(reports, infos, snk if sinks else None, drn if drainage else None, fld if flood else None,
                            wet if wetness else None, tex if texture else None)


def _check_kriging(kriging, who="evaluate_raster"):
    """False or None -> None (no kriging row); True -> True (fit the power model); a kriging.Variogram -> itself."""
    if kriging is None or kriging is False:
        return None
    if kriging is True:
        return True
    from .kriging import Variogram
    if isinstance(kriging, Variogram):
        return kriging
    raise ValueError(f"{who}: kriging {kriging!r} must be False, True or a kriging.Variogram")


def assemble_calibration(cells, sum_z2, within1, within2):
    """The calibration dict from the counts over the scored pixels with a finite variance > 0, z^2 = err^2 / var (pure: no GPU):
    a calibrated variance has mean_z2 near 1, within_1sigma near 0.68 and within_2sigma near 0.95; None without cells."""
    cells = int(cells)
    if not cells:
        return {"cells": 0, "mean_z2": None, "within_1sigma": None, "within_2sigma": None}
    return {"cells": cells, "mean_z2": float(sum_z2) / cells, "within_1sigma": int(within1) / cells,
            "within_2sigma": int(within2) / cells}


def calibration(dem, pred, variance, holes):
    """Is |error| <= sigma about 68 % of the time: over the pixels of holes (nonzero = hole) with a finite pred and a finite
    variance > 0, z^2 = (pred - dem)^2 / variance in float64 (torch reductions on the device: not a hot path)."""
    device = R.device(WHO)
    z = R.to_f32(dem, device, "dem", WHO).double()
    p = R.to_f32(pred, device, "pred", WHO).double()
    v = R.to_f32(variance, device, "variance", WHO).double()
    sel = (R.to_u8(holes, device, "holes", WHO, nonzero=True, reuse=True) != 0) & torch.isfinite(p) & torch.isfinite(v) & (v > 0)
    z2 = ((p - z) ** 2 / v)[sel]
    return assemble_calibration(z2.numel(), z2.sum().item(), (z2 <= 1.0).sum().item(), (z2 <= 4.0).sum().item())


@torch.no_grad()
def kriging_report(dem, holes, keep, *, cellsize, mask=None, nodata=None, variogram=None, area_edges_m2=AREA_EDGES_M2,
                   quantiles=QUANTILES, top=10, depth_edges_m=None, sinks=False, drainage=False, stream_cells=1000,
                   stream_tol_m=None, flood=False, flood_stages_m=FLOOD_STAGES_M, wetness=False, wetness_exponent=1,
                   wetness_min_slope=1e-3, texture=False, texture_octaves=5):
    """The krige_voids fill of the keep mask (mvp_gan/src/kriging.py; variogram None: the power model fitted to the kept pixels)
    scored on the holes like a compare_report fill: terrain_errors' report plus "method", the fill info under "fill", the model
    under "variogram", the optional rows by the same calls, and "calibration" (calibration's dict) of the kriging variance."""
    from .kriging import krige_voids
    device = R.device(WHO)
    z = R.to_f32(dem, device, "dem", WHO)
    k = R.to_f32(keep, device, "keep", WHO, binary=True)
    pred, var, finfo = krige_voids(z, k, nodata=R.nodata_value(nodata), cellsize=cellsize, variogram=variogram)
    rep = terrain_errors(z, pred, holes, k, cellsize=cellsize, mask=mask, nodata=nodata, area_edges_m2=area_edges_m2,
                         quantiles=quantiles, top=top, depth_edges_m=depth_edges_m)
    rep["method"] = "kriging"
    rep["fill"] = finfo
    rep["variogram"] = finfo["variogram"]
    if sinks:
        rep["sinks"] = sink_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata)
    if drainage:
        rep["drainage"] = drainage_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, stream_cells=stream_cells,
                                          stream_tol_m=stream_tol_m)
    if flood:
        rep["flood"] = flood_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, stream_cells=stream_cells,
                                    stages_m=flood_stages_m)
    if wetness:
        rep["wetness"] = wetness_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, exponent=wetness_exponent,
                                        min_slope=wetness_min_slope)
    if texture:
        rep["texture"] = texture_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, octaves=texture_octaves)
    rep["calibration"] = calibration(z, pred, var, holes)
    return rep


def _check_natural(natural, who="evaluate_raster"):
    """False or None -> False (no natural-neighbour row); True -> True."""
    if natural is None or natural is False:
        return False
    if natural is True:
        return True
    raise ValueError(f"{who}: natural {natural!r} must be False or True")


@torch.no_grad()
def natural_report(dem, holes, keep, *, cellsize, mask=None, nodata=None, radius=32, area_edges_m2=AREA_EDGES_M2,
                   quantiles=QUANTILES, top=10, depth_edges_m=None, sinks=False, drainage=False, stream_cells=1000,
                   stream_tol_m=None, flood=False, flood_stages_m=FLOOD_STAGES_M, wetness=False, wetness_exponent=1,
                   wetness_min_slope=1e-3, texture=False, texture_octaves=5):
    """The natural-neighbour fill of the keep mask (natural_neighbour_voids; mvp_gan/src/natural.py)
    scored on the holes like a compare_report fill: terrain_errors' report plus "method", the fill info under "fill" and the
    optional rows by the same calls."""
    from .natural import natural_neighbour_voids
    device = R.device(WHO)
    z = R.to_f32(dem, device, "dem", WHO)
    k = R.to_f32(keep, device, "keep", WHO, binary=True)
    pred, finfo = natural_neighbour_voids(z, k, nodata=R.nodata_value(nodata), cellsize=cellsize, radius=radius)
    rep = terrain_errors(z, pred, holes, k, cellsize=cellsize, mask=mask, nodata=nodata, area_edges_m2=area_edges_m2,
                         quantiles=quantiles, top=top, depth_edges_m=depth_edges_m)
    rep["method"] = "natural"
    rep["fill"] = finfo
    if sinks:
        rep["sinks"] = sink_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata)
    if drainage:
        rep["drainage"] = drainage_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, stream_cells=stream_cells,
                                          stream_tol_m=stream_tol_m)
    if flood:
        rep["flood"] = flood_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, stream_cells=stream_cells,
                                    stages_m=flood_stages_m)
    if wetness:
        rep["wetness"] = wetness_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, exponent=wetness_exponent,
                                        min_slope=wetness_min_slope)
    if texture:
        rep["texture"] = texture_errors(z, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, octaves=texture_octaves)
    return rep


def _check_simulate(simulate, who="evaluate_raster"):
    """0, None or False -> 0 (no simulation row); an integer in [2, 4096] -> itself: the mean and the deviation need two."""
    if simulate is None or simulate is False or (simulate == 0 and isinstance(simulate, int)):
        return 0
    if isinstance(simulate, bool) or not isinstance(simulate, int) or not 2 <= simulate <= 4096:
        raise ValueError(f"{who}: simulate {simulate!r} must be 0 (off) or a number of realisations in [2, 4096]")
    return simulate


@torch.no_grad()
def simulation_report(dem, holes, keep, *, cellsize, realisations, mask=None, nodata=None, variogram=None, seed=0,
                      area_edges_m2=AREA_EDGES_M2, quantiles=QUANTILES, top=10, depth_edges_m=None, texture_octaves=5):
    """Conditional simulation of the keep mask (simulate_voids; mvp_gan/src/simulate.py; variogram None:
    the power model fitted to the kept pixels) scored on the holes: terrain_errors' report of the mean of the realisations plus
    "method", the info under "fill", "variogram", "realisations", "calibration" (calibration's dict) of sd^2 against the mean's
    errors, and "texture" (texture_errors' dict) of realisation 0: one surface, where the mean is as smooth as kriging."""
    from .simulate import simulate_voids
    n = _check_simulate(realisations, "simulation_report")
    if not n:
        raise ValueError("simulation_report: realisations must be at least 2")
    device = R.device(WHO)
    z = R.to_f32(dem, device, "dem", WHO)
    k = R.to_f32(keep, device, "keep", WHO, binary=True)
    nd = R.nodata_value(nodata)
    _, mean, sd, finfo = simulate_voids(z, k, nodata=nd, cellsize=cellsize, variogram=variogram, realisations=n, seed=seed,
                                        keep=False)
    from .kriging import Variogram
    first, _, _, _ = simulate_voids(z, k, nodata=nd, cellsize=cellsize, variogram=Variogram(**finfo["variogram"]), seed=seed)
    rep = terrain_errors(z, mean, holes, k, cellsize=cellsize, mask=mask, nodata=nodata, area_edges_m2=area_edges_m2,
                         quantiles=quantiles, top=top, depth_edges_m=depth_edges_m)
    rep["method"] = "simulation"
    rep["fill"] = finfo
    rep["variogram"] = finfo["variogram"]
    rep["realisations"] = n
    rep["calibration"] = calibration(z, mean, sd * sd, holes)
    rep["texture"] = texture_errors(z, first[0], holes, cellsize=cellsize, mask=mask, nodata=nodata, octaves=texture_octaves)
    return rep


def calibration_summary(c):
    """One line for a calibration dict."""
    f = lambda v, spec: "n/a" if v is None else format(v, spec)
    return (f"calibration: mean z2 {f(c['mean_z2'], '.3f')}, {f(c['within_1sigma'], '.3f')} within 1 sigma, "
            f"{f(c['within_2sigma'], '.3f')} within 2 sigma over {c['cells']} px")


# ---- a fill against the truth: what sink_errors, drainage_raw, flood_raw, wetness_raw and texture_raw open with -----------
def _fill_shapes(dem, pred, holes, mask, cellsize, who):
    """Host-side rejection before any launch; -> (cellsize, (H, W))."""
    c = R.cellsize(cellsize, who)
    shape = R.raster_shape(dem, mask, who)
    if R.shape(pred) != shape or R.shape(holes) != shape:
        raise ValueError(f"{who}: pred {R.shape(pred)} and holes {R.shape(holes)} must have the dem's shape {shape}")
    return c, shape


def _fill_upload(dem, pred, holes, mask, nodata):
    """-> (z, p float32 [H][W], sel uint8 [H][W]: nonzero = hole, known uint8 [H][W]: the pixels known in both surfaces)."""
    from tg_hip import ops as O
    device = R.device(WHO)
    z = R.to_f32(dem, device, "dem", WHO)
    p = R.to_f32(pred, device, "pred", WHO)
    m = None if mask is None else R.to_f32(mask, device, "mask", WHO, binary=True)
    sel = R.to_u8(holes, device, "holes", WHO, nonzero=True, reuse=True)
    kz, _ = O.objmask_known(z, m, R.nodata_value(nodata), transposed=False)
    kp, _ = O.objmask_known(p, None, None, transposed=False)           # a fill may leave NaN
    return z, p, sel, kz & kp


# ---- sinks: does a fill drain ---------------------------------------------------------------------------------------------
def assemble_sinks(truth, pred):
    """The sinks dict from two sides' raw numbers, each {"counts": tg_depfill_stats' [raised, unreached, counted], "sums":
    [depth sum in m, largest depth in m], "depressions", "converged", "cellsize"} (pure: no GPU)."""
    from .fill_depressions import stats_dict

    def side(r):
        st = stats_dict(r["counts"], r["sums"], float(r["cellsize"]))
        return {"cells": st["cells"], "volume_m3": st["volume_m3"], "max_depth_m": st["max_depth_m"],
                "depressions": int(r["depressions"]), "converged": bool(r["converged"])}
    t, p = side(truth), side(pred)
    return {"truth": t, "pred": p, "excess_volume_m3": p["volume_m3"] - t["volume_m3"], "excess_cells": p["cells"] - t["cells"]}


@torch.no_grad()
def sink_errors(dem, pred, holes, *, cellsize, mask=None, nodata=None, connectivity=8):
    """The closed pits a fill put into the holes, against those the true terrain has there.  The depressions of dem and of
    pred are filled (fill_depressions' iteration) over one known mask, the pixels known in both, so both have the same outlets;
    the raised pixels are counted inside holes (nonzero = hole).  -> {"truth": {...}, "pred": {...}, "excess_volume_m3",
    "excess_cells"}; a side holds cells (raised pixels in the holes), volume_m3, max_depth_m, depressions (8-connected
    components of the raised pixels in the holes) and converged."""
    from tg_hip import ops as O
    from .fill_depressions import CONNECTIVITIES, count_depressions, relax
    who = "sink_errors"
    c, _ = _fill_shapes(dem, pred, holes, mask, cellsize, who)
    if isinstance(connectivity, bool) or connectivity not in CONNECTIVITIES:
        raise ValueError(f"{who}: connectivity {connectivity!r} must be 8 or 4")
    z, p, sel, known = _fill_upload(dem, pred, holes, mask, nodata)
    raw = []
    for surf in (z, p):
        w, _, _, _, converged = relax(surf, known, connectivity)
        counts, sums = O.depfill_stats(surf, w, known, sel)
        _, _, flags = O.depfill_finish(surf, w, known, want_flags=True)
        raw.append({"counts": counts.cpu().tolist(), "sums": sums.cpu().tolist(), "converged": converged, "cellsize": c,
                    "depressions": count_depressions(flags & (sel != 0))})
    return assemble_sinks(*raw)


def sinks_summary(s):
    """One line for a sinks dict."""
    return (f"sinks: {s['pred']['cells']} px / {s['pred']['volume_m3']:.6g} m3 in {s['pred']['depressions']} pits (truth "
            f"{s['truth']['cells']} px / {s['truth']['volume_m3']:.6g} m3 in {s['truth']['depressions']}), excess "
            f"{s['excess_volume_m3']:.6g} m3")


# ---- drainage: does water cross a fill as it crosses the truth -----------------------------------------------------------
def stream_tolerance(cellsize, stream_tol_m=None, who="drainage_errors"):
    """-> (tolerance in metres, tol2 = floor((tolerance / cellsize)^2) in pixels^2).  None means 3 cells: 3.0 * cellsize and
    tol2 = 9 exactly.  Otherwise tol2 is computed in exact rational arithmetic on the two doubles as given (fractions.Fraction),
    so no rounding can move it across an integer; it must be below 2^31 - 1."""
    from fractions import Fraction
    c = R.cellsize(cellsize, who)
    if stream_tol_m is None:
        return 3.0 * c, 9
    try:
        t = float(stream_tol_m)
    except (TypeError, ValueError):
        t = math.nan
    if isinstance(stream_tol_m, bool) or not (t >= 0 and t < math.inf):
        raise ValueError(f"{who}: stream_tol_m {stream_tol_m!r} must be None or a finite number >= 0")
    tol2 = math.floor((Fraction(t) / Fraction(c)) ** 2)
    if tol2 >= 2 ** 31 - 1:
        raise ValueError(f"{who}: stream_tol_m {t!r} is {tol2} px^2 at cellsize {c!r}: must be below 2^31 - 1")
    return t, tol2


def _check_stream_cells(n, who):
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n < 2 ** 31:
        raise ValueError(f"{who}: stream_cells {n!r} must be an integer in [1, 2^31)")
    return n


def assemble_drainage(counts, truth, pred, *, cellsize, stream_cells, stream_tol_m):
    """The drainage dict from tg_flow_compare's counters (a sequence of FLOW_COMPARE_COUNTS integers, ops.FLOW_COMPARE_NAMES)
    and the two sides' routing numbers, each {"pits", "flat_cells", "converged", "rounds"} (pure: no GPU).  Shares are taken
    of the cells compared, within_45 of the cells both sides route (codes 1..8); distances are cellsize * sqrt(an exact
    integer or a ratio of two); a share or mean with a zero denominator is None."""
    (cells, dir_equal, dir_routed, dir_within, same, od2_sum, od2_max, oct_sum, st_t, st_p, st_b, p_match, p_far, p_sum, p_max,
     t_match, t_far, t_sum, t_max) = (int(v) for v in counts)
    c = float(cellsize)
    ratio = lambda a, b: a / b if b else None
    rms = lambda s2, n: c * math.sqrt(s2 / n) if n else None
    dist = lambda d2, n: c * math.sqrt(d2) if n else None
    side = lambda r: {"pits": int(r["pits"]), "flat_cells": int(r["flat_cells"]), "converged": bool(r["converged"]),
                      "rounds": int(r["rounds"])}
    return {"cells": cells, "stream_cells": int(stream_cells), "stream_tol_m": float(stream_tol_m),
            "direction": {"equal": ratio(dir_equal, cells), "within_45": ratio(dir_within, dir_routed), "routed": dir_routed},
            "outlet": {"same": ratio(same, cells), "shift_rms_m": rms(od2_sum, cells), "shift_max_m": dist(od2_max, cells)},
            "area": {"octave_mae": ratio(oct_sum, cells)},
            "streams": {"truth_cells": st_t, "pred_cells": st_p, "both_cells": st_b,
                        "precision": ratio(p_match, st_p), "recall": ratio(t_match, st_t),
                        "pred_to_truth_rms_m": rms(p_sum, st_p - p_far), "pred_to_truth_max_m": dist(p_max, st_p - p_far),
                        "truth_to_pred_rms_m": rms(t_sum, st_t - t_far), "truth_to_pred_max_m": dist(t_max, st_t - t_far),
                        "pred_far": p_far, "truth_far": t_far},
            "truth": side(truth), "pred": side(pred)}


@torch.no_grad()
def drainage_raw(dem, pred, holes, *, cellsize, mask=None, nodata=None, stream_cells=1000, stream_tol_m=None):
    """drainage_errors' measurement -> (counts: tg_flow_compare's counters as a list of ints, [truth side, pred side], tolerance in
    metres, tol2)."""
    from tg_hip import ops as O
    from .flow_routing import route_known, streams, watersheds
    who = "drainage_errors"
    c, (H, W) = _fill_shapes(dem, pred, holes, mask, cellsize, who)
    if max(H, W) > 32767:
        raise ValueError(f"{who}: needs sides of at most 32767 px (exact int32 squared distances), got {H}x{W}")
    _check_stream_cells(stream_cells, who)
    tol_m, tol2 = stream_tolerance(c, stream_tol_m, who)
    z, p, sel, known = _fill_upload(dem, pred, holes, mask, nodata)
    sides, grids = [], []
    for surf in (z, p):
        direction, acc, info = route_known(surf, known, c, fill=True)
        basin, _, winfo = watersheds(direction, cellsize=c)
        d2, _ = O.edt(streams(acc, stream_cells))
        grids.append((direction, basin, acc, d2))
        sides.append({"pits": info["pits"], "flat_cells": info["flat_cells"], "converged": info["converged"],
                      "rounds": winfo["rounds"]})
    (dt, bt, at, d2t), (dp, bp, ap, d2p) = grids
    counts = O.flow_compare(sel, dt, dp, bt, bp, at, ap, d2t, d2p, stream_cells, tol2)
    return counts.cpu().tolist(), sides, tol_m, tol2


def drainage_errors(dem, pred, holes, *, cellsize, mask=None, nodata=None, stream_cells=1000, stream_tol_m=None):
    """How water crosses a fill, against how it crosses the true terrain.  dem and pred are routed (flow_routing's chain with
    fill=True) over one known mask, the pixels known in both, so both have the same outlets; watersheds gives every pixel its
    outlet, the pixels with an accumulation >= stream_cells are a side's streams, and tg_edt gives the exact squared distance
    to each side's streams.  Inside holes (nonzero = hole) one pass counts, in integers: equal and near-equal directions,
    equal outlets and the distance between the two, the octaves between the two contributing areas, and the stream pixels of
    each side within stream_tol_m (None: 3 cells; stream_tolerance) of the other's.  -> assemble_drainage's dict."""
    counts, sides, tol_m, _ = drainage_raw(dem, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata,
                                           stream_cells=stream_cells, stream_tol_m=stream_tol_m)
    return assemble_drainage(counts, sides[0], sides[1], cellsize=R.cellsize(cellsize, "drainage_errors"),
                             stream_cells=stream_cells, stream_tol_m=tol_m)


def drainage_summary(d):
    """One line for a drainage dict."""
    f = lambda v, spec: "n/a" if v is None else format(v, spec)
    s = d["streams"]
    return (f"drainage: {f(d['direction']['equal'], '.3f')} equal directions, {f(d['outlet']['same'], '.3f')} same outlet (shift rms "
            f"{f(d['outlet']['shift_rms_m'], '.4g')} m) over {d['cells']} px; streams >= {d['stream_cells']} cells: precision "
            f"{f(s['precision'], '.3f')}, recall {f(s['recall'], '.3f')} within {d['stream_tol_m']:g} m, largest displacement "
            f"{f(s['pred_to_truth_max_m'], '.4g')} m")


# ---- flood: does a flood map made from a fill wet the ground the truth's does -----------------------------------------------
def check_flood_stages(stages_m, who="flood_errors"):
    """1 to 8 stages in metres, each finite and > 0 and strictly increasing, also after the rounding to float32 the kernel gets
    them in -> a tuple of floats (the float32 values)."""
    try:
        vals = [float(v) for v in stages_m]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: flood stages {stages_m!r} must be a sequence of numbers") from None
    if any(isinstance(v, bool) for v in stages_m) or not 1 <= len(vals) <= FLOOD_MAX_STAGES:
        raise ValueError(f"{who}: flood stages {stages_m!r} must be 1 to {FLOOD_MAX_STAGES} numbers")
    with np.errstate(over="ignore"):
        f = np.array(vals, np.float64).astype(np.float32)
    if not (np.isfinite(f).all() and (f > 0).all()):
        raise ValueError(f"{who}: flood stages {stages_m!r} must be finite and > 0")
    if not (np.diff(f) > 0).all():
        raise ValueError(f"{who}: flood stages {stages_m!r} must be strictly increasing")
    return tuple(float(v) for v in f)


def assemble_flood(counts, stages_m, *, stream_cells):
    """The flood dict from tg_flood_compare's counters (a sequence of at least 6 + 3 * len(stages_m) integers) (pure: no GPU).
    hand: mean absolute, mean signed (fill minus truth) and largest difference of the two HAND planes over the cells compared,
    from the exact integer sums in 1/1024 m; per stage the cells each side wets (HAND <= stage), those both wet, the critical
    success index both / (truth + pred - both), precision both / pred and recall both / truth; None on a zero denominator."""
    c = [int(v) for v in counts]
    stages = [float(s) for s in stages_m]
    if len(c) < 6 + 3 * len(stages):
        raise ValueError(f"assemble_flood: {len(c)} counters for {len(stages)} stages")
    cells, und_t, und_p, abs_q, bias_q, max_bits = c[:6]
    ratio = lambda a, b: a / b if b else None
    out = {"cells": cells, "stream_cells": int(stream_cells), "undrained_truth": und_t, "undrained_pred": und_p,
           "hand": {"mae_m": ratio(abs_q / 1024, cells), "bias_m": ratio(bias_q / 1024, cells),
                    "max_m": R.bits_f32(max_bits) if cells else None},
           "stages": []}
    for i, s in enumerate(stages):
        t, p, b = c[6 + 3 * i:9 + 3 * i]
        out["stages"].append({"stage_m": s, "truth_cells": t, "pred_cells": p, "both_cells": b, "csi": ratio(b, t + p - b),
                              "precision": ratio(b, p), "recall": ratio(b, t)})
    return out


@torch.no_grad()
def flood_raw(dem, pred, holes, *, cellsize, mask=None, nodata=None, stream_cells=1000, stages_m=FLOOD_STAGES_M):
    """flood_errors' measurement -> (counts: tg_flood_compare's counters as a list of ints, the stages as given to the kernel,
    [truth side, pred side]: each hand_from_routing's info)."""
    from tg_hip import ops as O
    from .flow_routing import hand_from_routing, route_known
    who = "flood_errors"
    c, _ = _fill_shapes(dem, pred, holes, mask, cellsize, who)
    _check_stream_cells(stream_cells, who)
    stages = check_flood_stages(stages_m, who)
    z, p, sel, known = _fill_upload(dem, pred, holes, mask, nodata)
    hands, sides = [], []
    for surf in (z, p):
        direction, acc, _, w = route_known(surf, known, c, fill=True, return_surface=True)
        stream = ((acc >= stream_cells) & (direction != 0)).to(torch.uint8)
        h, _, hinfo = hand_from_routing(w, direction, stream, c)
        hands.append(h)
        sides.append(hinfo)
    counts = O.flood_compare(sel, hands[0], hands[1], stages)
    return counts.cpu().tolist(), stages, sides


def flood_errors(dem, pred, holes, *, cellsize, mask=None, nodata=None, stream_cells=1000, stages_m=FLOOD_STAGES_M):
    """Does a flood map made from a fill wet the ground that one made from the true terrain wets.  dem and pred are routed
    (flow_routing's chain with fill=True) over one known mask, the pixels known in both; each side's height above the nearest
    drainage (flow_routing.hand_from_routing) is taken against its own streams (accumulation >= stream_cells); the flood extent
    of a side at stage s is HAND <= s.  Inside holes (nonzero = hole) one pass counts in integers, over the pixels where both
    sides are drained: the HAND differences, and per stage the cells each side wets and those both wet.  -> assemble_flood's
    dict."""
    counts, stages, _ = flood_raw(dem, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, stream_cells=stream_cells,
                                  stages_m=stages_m)
    return assemble_flood(counts, stages, stream_cells=stream_cells)


def flood_summary(d):
    """One line for a flood dict."""
    f = lambda v, spec: "n/a" if v is None else format(v, spec)
    st = ", ".join(f"{s['stage_m']:g} m {f(s['csi'], '.3f')}" for s in d["stages"])
    return (f"flood: HAND MAE {f(d['hand']['mae_m'], '.4g')} m, bias {f(d['hand']['bias_m'], '.4g')} m, max "
            f"{f(d['hand']['max_m'], '.4g')} m over {d['cells']} px (streams >= {d['stream_cells']} cells; undrained "
            f"{d['undrained_truth']} truth / {d['undrained_pred']} fill); CSI by stage: {st}")


# ---- wetness: does a fill keep the hillslopes' contributing area and slope ----------------------------------------------------
def assemble_wetness(counts, sums):
    """The wetness dict from tg_wetness_compare's numbers (counts: cells, the bits of the largest |d|; sums: of d, |d|, d * d)
    (pure: no GPU): cells, and bias, mae, rmse and max of the TWI difference fill minus truth; None without cells."""
    cells, bits = (int(v) for v in counts)
    sd, sa, s2 = (float(v) for v in sums)
    if not cells:
        return {"cells": 0, "bias": None, "mae": None, "rmse": None, "max": None}
    return {"cells": cells, "bias": sd / cells, "mae": sa / cells, "rmse": math.sqrt(s2 / cells), "max": R.bits_f32(bits)}


@torch.no_grad()
def wetness_raw(dem, pred, holes, *, cellsize, mask=None, nodata=None, exponent=1, min_slope=1e-3):
    """wetness_errors' measurement -> (counts, sums as lists, [truth side, pred side]: each wetness_known's info)."""
    from tg_hip import ops as O
    from .flow_routing import check_exponent, check_min_slope, wetness_known
    who = "wetness_errors"
    c, _ = _fill_shapes(dem, pred, holes, mask, cellsize, who)
    check_exponent(exponent, who)
    check_min_slope(min_slope, who)
    z, p, sel, known = _fill_upload(dem, pred, holes, mask, nodata)
    twis, sides = [], []
    for surf in (z, p):
        twi, _, _, info = wetness_known(surf, known, c, fill=True, exponent=exponent, min_slope=min_slope)
        twis.append(twi)
        sides.append(info)
    counts, sums = O.wetness_compare(sel, twis[0], twis[1])
    return counts.cpu().tolist(), sums.cpu().tolist(), sides


def wetness_errors(dem, pred, holes, *, cellsize, mask=None, nodata=None, exponent=1, min_slope=1e-3):
    """Does a fill keep the hillslopes' wetness.  dem and pred are routed (flow_routing's chain with fill=True) over one known
    mask, the pixels known in both, exactly as drainage_errors routes them; each side's topographic wetness index
    (flow_routing.wetness_known: the multiple-flow-direction accumulation at `exponent`, Horn's slope not below min_slope) is
    taken, and inside holes (nonzero = hole), where both are finite, d = twi_pred - twi_truth in float32 is summed in float64 in a
    fixed order.  -> {"cells", "bias", "mae", "rmse", "max"} (assemble_wetness)."""
    counts, sums, _ = wetness_raw(dem, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, exponent=exponent,
                                  min_slope=min_slope)
    return assemble_wetness(counts, sums)


def wetness_summary(d):
    """One line for a wetness dict."""
    f = lambda v, spec: "n/a" if v is None else format(v, spec)
    return (f"wetness: TWI bias {f(d['bias'], '.4g')}, MAE {f(d['mae'], '.4g')}, RMSE {f(d['rmse'], '.4g')}, max "
            f"{f(d['max'], '.4g')} over {d['cells']} px")


# ---- texture: does a fill have the relief of the terrain at each scale ------------------------------------------------------
TEX_OCTAVES = 5                       # TG_TEX_OCTAVES: lags 1, 2, 4, 8, 16 px
TEX_CLASSES = ("axial", "diagonal")   # scale index = 2 * octave + class


def check_octaves(octaves, who="texture_errors"):
    """An integer in 1..TEX_OCTAVES (numpy's integers too, no bool, no float) -> a plain int."""
    import numbers
    if isinstance(octaves, (bool, np.bool_)) or not isinstance(octaves, numbers.Integral) or not 1 <= octaves <= TEX_OCTAVES:
        raise ValueError(f"{who}: octaves {octaves!r} must be an integer in [1, {TEX_OCTAVES}]")
    return int(octaves)


def texture_scales(octaves, cellsize):
    """[(lag_px, class name, lag_m)] in scale-index order: ascending lag."""
    return [(1 << j, name, (1 << j) * cellsize * (math.sqrt(2.0) if k else 1.0))
            for j in range(octaves) for k, name in enumerate(TEX_CLASSES)]


def assemble_texture(counts, sums, *, cellsize, octaves):
    """The texture dict from tg_texture_compare's numbers (counts [10]: triples per scale; sums [10][3]: of d_z d_z, d_p d_p,
    d_z d_p) (pure: no GPU): per scale of the requested octaves the lag, the triples, the RMS second difference of the truth and
    of the fill, their ratio fill / truth and their correlation; log_ratio_rms = sqrt(mean(ln(ratio)^2)) over the scales_scored
    scales where both RMS are > 0.  None stands for a value that is not defined."""
    octaves = check_octaves(octaves, "assemble_texture")
    c = R.cellsize(cellsize, "assemble_texture")
    scales, logs = [], []
    for s, (h, name, lag_m) in enumerate(texture_scales(octaves, c)):
        n = int(counts[s])
        szz, spp, szp = (float(v) for v in sums[s])
        t_rms = math.sqrt(szz / n) if n else None
        f_rms = math.sqrt(spp / n) if n else None
        ratio = f_rms / t_rms if n and szz != 0 and t_rms > 0 else None      # t_rms == 0 with szz != 0: szz / n underflowed
        den = szz * spp
        corr = szp / math.sqrt(den) if n and den != 0 else None
        scales.append({"lag_px": h, "class": name, "lag_m": lag_m, "triples": n, "truth_rms": t_rms, "fill_rms": f_rms,
                       "ratio": ratio, "corr": corr})
        if n and t_rms > 0 and f_rms > 0:
            logs.append(math.log(ratio))
    return {"octaves": octaves, "scales": scales, "scales_scored": len(logs),
            "log_ratio_rms": math.sqrt(sum(v * v for v in logs) / len(logs)) if logs else None}


@torch.no_grad()
def texture_raw(dem, pred, holes, *, cellsize, mask=None, nodata=None, octaves=5):
    """texture_errors' measurement -> (counts [10], sums [10][3] as lists)."""
    from tg_hip import ops as O
    who = "texture_errors"
    _fill_shapes(dem, pred, holes, mask, cellsize, who)
    octaves = check_octaves(octaves, who)
    z, p, sel, known = _fill_upload(dem, pred, holes, mask, nodata)
    counts, sums = O.texture_compare(z, p, sel, known, octaves)
    return counts.cpu().tolist(), sums.cpu().tolist()


def texture_errors(dem, pred, holes, *, cellsize, mask=None, nodata=None, octaves=5):
    """Does a fill have the relief of the terrain at each scale.  Over the triples (centre in holes (nonzero = hole), two arms
    at the lag h = 1, 2, .. 2^(octaves - 1) px along the axes or along the diagonals, all three pixels known in both surfaces; the
    arms may lie outside the holes, where pred is the dem, so the seam is measured too) the second differences
    (s(x - hu) + s(x + hu)) - 2 s(x) of dem and pred are taken in float64 and their squares and product summed in a fixed order.
    -> {"octaves", "scales": [{"lag_px", "class", "lag_m", "triples", "truth_rms", "fill_rms", "ratio", "corr"}], "scales_scored",
    "log_ratio_rms"} (assemble_texture)."""
    c = R.cellsize(cellsize, "texture_errors")
    counts, sums = texture_raw(dem, pred, holes, cellsize=cellsize, mask=mask, nodata=nodata, octaves=octaves)
    return assemble_texture(counts, sums, cellsize=c, octaves=octaves)


def texture_summary(d):
    """One line for a texture dict: ratio and correlation at the shortest and at the longest scored scale, and log_ratio_rms."""
    f = lambda v, spec: "n/a" if v is None else format(v, spec)
    scored = [s for s in d["scales"] if s["truth_rms"] and s["fill_rms"]]
    ends = [scored[0], scored[-1]] if scored else [None, None]
    parts = []
    for s in ends:
        if s is None:
            parts.append("n/a")
        else:
            parts.append(f"{s['lag_px']} px {s['class']} ratio {f(s['ratio'], '.3f')} corr {f(s['corr'], '.3f')}")
    return (f"texture: second differences fill / truth, {parts[0]}; {parts[1]}; log-ratio RMS {f(d['log_ratio_rms'], '.3f')} over "
            f"{d['scales_scored']} of {len(d['scales'])} scales")


@torch.no_grad()
def evaluate_raster(generator_or_checkpoint, dem, mask=None, *, nodata=None, cellsize, split="test", block=1024, tile=256,
                    holes=HoleSpec(), seed=0, window=512, overlap=64, batch=16, objects=None, area_edges_m2=AREA_EDGES_M2,
                    quantiles=QUANTILES, top=10, baseline=None, fallback=None, seam=None, model_cellsize=None, min_coverage=0.5,
                    solver="mg", depth_edges_m=None, compare=None, sinks=False, drainage=False, stream_cells=1000, stream_tol_m=None,
                    flood=False, flood_stages_m=FLOOD_STAGES_M, wetness=False, wetness_exponent=1, wetness_min_slope=1e-3,
                    texture=False, texture_octaves=5, kriging=False, tta=1, simulate=0, natural=False, natural_radius=32):
    """eval_holes -> inpaint_raster(mask=keep) -> terrain_errors.  Returns (report, pred float32 HIP tensor [H][W]).
    baseline="laplace" adds report["baseline"]; fallback, seam, model_cellsize and min_coverage are passed to inpaint_raster
    (the holes are cut and scored on the native grid, in metres: block and tile are native pixels, see native_cells for a
    checkpoint whose training blocks were picked on the working grid), and seam="harmonic" adds report["seam"].  solver is the
    fill_voids solver of the baseline, the seam correction and the fallback ("mg" or "pcg"); "pcg" shows in their infos.
    depth_edges_m adds "by_depth" to the report and, on the same classes, to report["baseline"].  compare: names out of COMPARES,
    adds report["compare"][name], the interpolate_voids fill of the same keep mask scored on the same holes and classes.
    sinks=True adds sink_errors' dict under "sinks" to the report, to report["baseline"] and to every report["compare"][name];
    drainage=True adds drainage_errors' dict (streams of stream_cells cells, matched within stream_tol_m) under "drainage" to the
    same three places; flood=True adds flood_errors' dict (HAND against streams of stream_cells cells, flood extents at
    flood_stages_m) under "flood" to the same three places; wetness=True adds wetness_errors' dict (the TWI from the
    multiple-flow-direction accumulation at wetness_exponent, slopes not below wetness_min_slope) under "wetness" to the same
    three places; texture=True adds texture_errors' dict (second differences at texture_octaves octaves of lags) under "texture" to
    the same three places.  kriging=True (or a kriging.Variogram; True fits the power model to the kept pixels) adds
    report["kriging"], kriging_report's dict: the krige_voids fill of the same keep mask scored on the same holes and classes, with
    the same optional rows and the calibration of its variance.  tta (1, 2, 4 or 8) is passed to the inpainting; above 1 the
    prediction is the mean of the members and report["spread"] = {"members", "mean_m", "max_m", "calibration"}: the spread over
    the filled holes in metres and calibration's dict of spread^2 over the scored holes, the row kriging's variance is judged
    by.  simulate=n (n >= 2 realisations; 0: off) adds report["simulation"], simulation_report's dict: the mean of n conditional
    simulations of the same keep mask scored on the same holes and classes, the calibration of their sd^2 and the texture of
    realisation 0; with a kriging.Variogram given as kriging it simulates under that model, else under the fitted one.
    natural=True adds report["natural"], natural_report's dict: the natural-neighbour fill (natural_neighbour_voids at
    natural_radius) of the same keep mask scored on the same holes and classes, with the same optional rows."""
    rep, pred, _ = _evaluate(generator_or_checkpoint, dem, mask, nodata=nodata, cellsize=cellsize, split=split, block=block,
                             tile=tile, holes=holes, seed=seed, window=window, overlap=overlap, batch=batch, objects=objects,
                             area_edges_m2=area_edges_m2, quantiles=quantiles, top=top, baseline=baseline, fallback=fallback,
                             seam=seam, model_cellsize=model_cellsize, min_coverage=min_coverage, solver=solver,
                             depth_edges_m=depth_edges_m, compare=compare, sinks=sinks, drainage=drainage,
                             stream_cells=stream_cells, stream_tol_m=stream_tol_m, flood=flood, flood_stages_m=flood_stages_m,
                             wetness=wetness, wetness_exponent=wetness_exponent, wetness_min_slope=wetness_min_slope,
                             texture=texture, texture_octaves=texture_octaves, kriging=kriging, tta=tta,
                             simulate=simulate, natural=natural, natural_radius=natural_radius)
    return rep, pred


def _evaluate(generator_or_checkpoint, dem, mask, *, nodata, cellsize, split, block, tile, holes, seed, window, overlap, batch,
              objects, area_edges_m2, quantiles, top, baseline=None, fallback=None, seam=None, model_cellsize=None,
              min_coverage=0.5, solver="mg", depth_edges_m=None, compare=None, sinks=False, drainage=False, stream_cells=1000,
              stream_tol_m=None, flood=False, flood_stages_m=FLOOD_STAGES_M, wetness=False, wetness_exponent=1,
              wetness_min_slope=1e-3, texture=False, texture_octaves=5, kriging=False, tta=1, simulate=0, natural=False,
              natural_radius=32):
    """evaluate_raster, plus the hole map."""
    from .fill_voids import check_solver
    from .inpaint_raster import check_resample_options, check_seam_options, check_tta, inpaint_raster, inpaint_raster_tta
    _check_fill_options(baseline, fallback)
    compare = _check_compare(compare)
    kriging = _check_kriging(kriging)
    simulate = _check_simulate(simulate)
    natural = _check_natural(natural)
    check_solver(solver, who="evaluate_raster")
    check_seam_options(seam, 1, who="evaluate_raster")
    c = R.cellsize(cellsize, "evaluate_raster")
    scale = check_resample_options(c, model_cellsize, min_coverage, who="evaluate_raster")
    H, W = R.raster_shape(dem, mask, "evaluate_raster")
    check_tta(tta, (H, W), window, scale, who="evaluate_raster")
    if compare and max(H, W) > 32767:
        raise ValueError(f"evaluate_raster: compare needs sides of at most 32767 px, got {H}x{W}")
    if kriging is not None and max(H, W) > 32767:
        raise ValueError(f"evaluate_raster: kriging needs sides of at most 32767 px, got {H}x{W}")
    if natural:
        from .natural import check_args as check_natural_args
        check_natural_args(dem, mask, natural_radius, None, c, who="evaluate_raster")
    if simulate:
        if max(H, W) > 32767:
            raise ValueError(f"evaluate_raster: simulate needs sides of at most 32767 px, got {H}x{W}")
        if kriging not in (None, True) and kriging.model == "spherical":
            raise ValueError("evaluate_raster: simulate has no spherical model; give the power or the exponential one")
        check_octaves(texture_octaves, "evaluate_raster")
    if drainage:
        if max(H, W) > 32767:
            raise ValueError(f"evaluate_raster: drainage needs sides of at most 32767 px, got {H}x{W}")
        _check_stream_cells(stream_cells, "evaluate_raster")
        stream_tolerance(c, stream_tol_m, "evaluate_raster")
    if flood:
        _check_stream_cells(stream_cells, "evaluate_raster")
        check_flood_stages(flood_stages_m, "evaluate_raster")
    if wetness:
        from .flow_routing import check_exponent, check_min_slope
        check_exponent(wetness_exponent, "evaluate_raster")
        check_min_slope(wetness_min_slope, "evaluate_raster")
    if texture:
        check_octaves(texture_octaves, "evaluate_raster")
    check_plan(H, W, split, block, tile, holes, who="evaluate_raster")
    _check_edges(area_edges_m2)
    _check_quantiles(quantiles)
    _check_depth_edges(depth_edges_m)
    z, m, _, _ = R.upload(dem, mask, None, WHO)
    hm, keep, hinfo = eval_holes(z, m, nodata=nodata, split=split, block=block, tile=tile, holes=holes, seed=seed,
                                 objects=objects, cellsize=c)
    spread = None
    if tta == 1:
        pred, iinfo = inpaint_raster(generator_or_checkpoint, z, keep, nodata=nodata, window=window, overlap=overlap, batch=batch,
                                     fallback=fallback, seam=seam, cellsize=c, model_cellsize=model_cellsize,
                                     min_coverage=min_coverage, solver=solver)
    else:
        pred, spread, iinfo = inpaint_raster_tta(generator_or_checkpoint, z, keep, tta=tta, nodata=nodata, window=window,
                                                 overlap=overlap, batch=batch, fallback=fallback, seam=seam, cellsize=c,
                                                 model_cellsize=model_cellsize, min_coverage=min_coverage, solver=solver)
    sinfo = iinfo.get("seam")
    rep = terrain_errors(z, pred, hm, keep, cellsize=c, mask=m, nodata=nodata, area_edges_m2=area_edges_m2,
                         quantiles=quantiles, top=top, depth_edges_m=depth_edges_m)
    rep.update(params(c, split, block, tile, seed, holes, window, overlap))
    rep["cells"] = hinfo["cells"]
    rep["inpaint"] = iinfo
    if sinfo is not None:
        rep["seam"] = sinfo
    if spread is not None:
        tt = iinfo["tta"]
        rep["spread"] = {"members": tt["members"], "mean_m": tt["mean_spread_m"], "max_m": tt["max_spread_m"],
                         "calibration": calibration(z, pred, spread * spread, hm)}
    if sinks:
        rep["sinks"] = sink_errors(z, pred, hm, cellsize=c, mask=m, nodata=nodata)
    drn = {"drainage": bool(drainage), "stream_cells": stream_cells, "stream_tol_m": stream_tol_m, "flood": bool(flood),
           "flood_stages_m": flood_stages_m, "wetness": bool(wetness), "wetness_exponent": wetness_exponent,
           "wetness_min_slope": wetness_min_slope, "texture": bool(texture), "texture_octaves": texture_octaves}
    if drainage:
        rep["drainage"] = drainage_errors(z, pred, hm, cellsize=c, mask=m, nodata=nodata, stream_cells=stream_cells,
                                          stream_tol_m=stream_tol_m)
    if flood:
        rep["flood"] = flood_errors(z, pred, hm, cellsize=c, mask=m, nodata=nodata, stream_cells=stream_cells,
                                    stages_m=flood_stages_m)
    if wetness:
        rep["wetness"] = wetness_errors(z, pred, hm, cellsize=c, mask=m, nodata=nodata, exponent=wetness_exponent,
                                        min_slope=wetness_min_slope)
    if texture:
        rep["texture"] = texture_errors(z, pred, hm, cellsize=c, mask=m, nodata=nodata, octaves=texture_octaves)
    if baseline is not None:
        rep["baseline"] = baseline_report(z, hm, keep, cellsize=c, mask=m, nodata=nodata, method=baseline,
                                          area_edges_m2=area_edges_m2, quantiles=quantiles, top=top, solver=solver,
                                          depth_edges_m=depth_edges_m, sinks=bool(sinks), **drn)
    if compare:
        rep["compare"] = compare_report(z, hm, keep, compare, cellsize=c, mask=m, nodata=nodata, area_edges_m2=area_edges_m2,
                                        quantiles=quantiles, top=top, depth_edges_m=depth_edges_m, sinks=bool(sinks), **drn)
    if kriging is not None:
        rep["kriging"] = kriging_report(z, hm, keep, cellsize=c, mask=m, nodata=nodata,
                                        variogram=None if kriging is True else kriging, area_edges_m2=area_edges_m2,
                                        quantiles=quantiles, top=top, depth_edges_m=depth_edges_m, sinks=bool(sinks), **drn)
    if simulate:
        rep["simulation"] = simulation_report(z, hm, keep, cellsize=c, realisations=simulate, mask=m, nodata=nodata,
                                              variogram=None if kriging in (None, True) else kriging, seed=seed,
                                              area_edges_m2=area_edges_m2, quantiles=quantiles, top=top,
                                              depth_edges_m=depth_edges_m, texture_octaves=texture_octaves)
    if natural:
        rep["natural"] = natural_report(z, hm, keep, cellsize=c, mask=m, nodata=nodata, radius=natural_radius,
                                        area_edges_m2=area_edges_m2, quantiles=quantiles, top=top, depth_edges_m=depth_edges_m,
                                        sinks=bool(sinks), **drn)
    return rep, pred, hm


def params(cellsize, split, block, tile, seed, holes, window=None, overlap=None):
    hs = asdict(holes)
    hs["kinds"] = list(hs["kinds"])
    return {"cellsize": cellsize, "split": split, "block": int(block), "tile": int(tile), "seed": int(seed), "hole_spec": hs,
            "window": window, "overlap": overlap}


def summary(rep):
    """One line: height RMSE, LE90, slope MAE, ring RMSE; with "by_depth" also the height MAE of each depth class."""
    line = (f"height RMSE {rep['height']['rmse']:.4f} m, LE90 {rep['height']['le90']:.4f} m, slope MAE "
            f"{rep['slope_deg']['mae']:.3f} deg, ring RMSE {rep['ring']['rmse']:.4f} m over {rep['pixels']['scored']} px in "
            f"{rep['holes']['count']} holes")
    if "by_depth" in rep:
        line += "; MAE by depth " + ", ".join(f"{k['lo_m']:g}+ m {k['mae']:.4f}" for k in rep["by_depth"]["classes"])
    return line


# ---- CLI ------------------------------------------------------------------------------------------------------------
def build_parser():
    from .inpaint_raster import SEAMS
    from .object_mask import add_spec_args
    ap = argparse.ArgumentParser(description="Score inpainting of an ESRI ASCII grid DSM on held-out holes, in metres.")
    ap.add_argument("--dem", required=True, help="truth .asc raster (NODATA_value cells are never scored)")
    ap.add_argument("--checkpoint", help="generator checkpoint (.pth) to inpaint the holes with")
    ap.add_argument("--pred", help="scoring mode: an inpainted .asc raster to score instead of running a checkpoint")
    ap.add_argument("--holes", help="scoring mode: the hole map (.png or .asc, nonzero = hole) of an earlier --holes-out")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = valid")
    ap.add_argument("--nodata", type=float, help="nodata value (default: the .asc header's NODATA_value)")
    ap.add_argument("--split", choices=("test", "val", "train", "all"), default="test")
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--remove-objects", action="store_true",
                    help="find above-ground objects (cellsize from the header): filled but never scored")
    add_spec_args(ap)
    ap.add_argument("--json", help="write the report here")
    ap.add_argument("--pred-out", help="write the prediction (.asc)")
    ap.add_argument("--holes-out", help="write the evaluation holes (.png or .asc, nonzero = hole)")
    ap.add_argument("--baseline", choices=BASELINES,
                    help="also score a harmonic or a minimum-curvature interpolation (fill_voids) of the same holes: a second "
                         "summary line")
    ap.add_argument("--fallback", choices=("laplace",),
                    help="checkpoint mode: fill the holes no window reaches by harmonic interpolation")
    ap.add_argument("--solver", choices=("mg", "pcg"), default="mg",
                    help="solver of --baseline, --fallback and --seam: V-cycles, or conjugate gradients around them")
    ap.add_argument("--seam", choices=SEAMS,
                    help="checkpoint mode: correct the filled holes towards the known terrain around them (seam_correct)")
    ap.add_argument("--model-cellsize", type=float,
                    help="checkpoint mode: cell size the checkpoint was trained at; the windows run on the raster resampled to "
                         "it, the scoring stays on the native grid")
    ap.add_argument("--min-coverage", type=float, default=0.5,
                    help="with a coarser --model-cellsize: the known share of its footprint a resampled cell needs, in (0, 1]")
    ap.add_argument("--by-depth", type=float, nargs="*", metavar="E",
                    help="also report the height errors by distance to the known terrain: class bounds in metres (given bare: "
                         + " ".join(f"{e:g}" for e in DEPTH_EDGES_M) + "); the baseline is scored on the same classes")
    ap.add_argument("--compare", nargs="+", choices=COMPARES, metavar="NAME",
                    help="also score these interpolate_voids fills of the same holes (" + ", ".join(COMPARES) + "): one more "
                         "summary line each")
    ap.add_argument("--kriging", action="store_true",
                    help="also score the ordinary-kriging fill of the same holes (krige_voids, the power variogram fitted to "
                         "the kept cells) and the calibration of its variance: two more summary lines")
    ap.add_argument("--natural", action="store_true",
                    help="also score the natural-neighbour fill of the same holes (natural_neighbour_voids): one more summary "
                         "line, and one per optional row")
    ap.add_argument("--natural-radius", type=int, default=32, metavar="R",
                    help="with --natural: the radius of the fill in cells, an integer in 1..32")
    ap.add_argument("--simulate", type=int, default=0, metavar="N",
                    help="also draw N >= 2 conditional simulations of the same holes (simulate_voids) and score their mean, the "
                         "calibration of their spread and the texture of the first: three more summary lines")
    ap.add_argument("--tta", type=int, choices=(1, 2, 4, 8), default=1,
                    help="test-time augmentation of the inpainting (needs --checkpoint): the mean of this many flips / rotations "
                         "of every window is scored, and the calibration of their spread gets a summary line")
    ap.add_argument("--sinks", action="store_true",
                    help="also fill the depressions of the truth and of every scored fill and report the closed pits each fill "
                         "put into the holes (cells, volume, count): one more summary line per fill")
    ap.add_argument("--drainage", action="store_true",
                    help="also route the truth and every scored fill (D8 after a depression fill) and compare directions, "
                         "outlets, contributing areas and stream networks inside the holes: one more summary line per fill")
    ap.add_argument("--stream-cells", type=int, default=1000,
                    help="with --drainage: a cell is a stream when its contributing area is at least this many cells")
    ap.add_argument("--stream-tol", type=float, metavar="M",
                    help="with --drainage: a stream cell is matched when the other side has one within this many metres "
                         "(default: 3 cells)")
    ap.add_argument("--flood", action="store_true",
                    help="also compare flood maps: the height above the nearest drainage (streams of --stream-cells cells) of the "
                         "truth and of every scored fill, and the flood extents at --flood-stages inside the holes: one more "
                         "summary line per fill")
    ap.add_argument("--flood-stages", type=float, nargs="+", metavar="S", default=list(FLOOD_STAGES_M),
                    help="with --flood: 1 to 8 water stages above the drainage in metres, increasing (default: "
                         + " ".join(f"{s:g}" for s in FLOOD_STAGES_M) + ")")
    ap.add_argument("--wetness", action="store_true",
                    help="also compare the topographic wetness index ln(a / tan(beta)) of the truth and of every scored fill "
                         "inside the holes (a from a multiple-flow-direction accumulation): one more summary line per fill")
    ap.add_argument("--exponent", type=int, default=1,
                    help="with --wetness: the exponent of the multiple-flow-direction rule, an integer in 1..8")
    ap.add_argument("--min-slope", type=float, default=1e-3, help="with --wetness: slopes below this count as this (> 0)")
    ap.add_argument("--texture", action="store_true",
                    help="also compare the relief of every scored fill with the truth's at each scale: RMS second differences at "
                         "the lags 1, 2, 4, .. px over triples centred in the holes, their ratio and correlation: one more summary "
                         "line per fill")
    ap.add_argument("--octaves", type=int, default=TEX_OCTAVES,
                    help=f"with --texture: the number of lags 1, 2, 4, .. px, an integer in 1..{TEX_OCTAVES}")
    return ap


def main(argv=None):
    from .asc import asc_nodata, read_asc, read_inputs, read_mask, with_nodata, write_asc, write_mask
    from .object_mask import spec_from_args
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.stream_cells < 1:
        ap.error("--stream-cells must be >= 1")
    if a.stream_tol is not None and not (a.stream_tol >= 0 and a.stream_tol < math.inf):
        ap.error("--stream-tol must be finite and >= 0")
    try:
        check_flood_stages(a.flood_stages, "--flood-stages")
    except ValueError as e:
        ap.error(str(e))
    if not 1 <= a.exponent <= 8:
        ap.error("--exponent must lie in [1, 8]")
    if not (a.min_slope > 0 and a.min_slope < math.inf):
        ap.error("--min-slope must be finite and > 0")
    if not 1 <= a.octaves <= TEX_OCTAVES:
        ap.error(f"--octaves must lie in [1, {TEX_OCTAVES}]")
    try:
        _check_simulate(a.simulate, "--simulate")
    except ValueError as e:
        ap.error(str(e))
    if not 1 <= a.natural_radius <= 32:
        ap.error("--natural-radius must lie in [1, 32]")
    if bool(a.checkpoint) == bool(a.pred):
        ap.error("give exactly one of --checkpoint and --pred")
    if bool(a.pred) != bool(a.holes):
        ap.error("--pred and --holes go together")
    if a.fallback and a.pred:
        ap.error("--fallback needs --checkpoint")
    if a.seam and a.pred:
        ap.error("--seam needs --checkpoint")
    if a.model_cellsize is not None and a.pred:
        ap.error("--model-cellsize needs --checkpoint")
    if a.tta != 1 and a.pred:
        ap.error("--tta needs --checkpoint")
    dem, header, mask, nodata, c = read_inputs(a)
    objects = spec_from_args(a) if a.remove_objects else None
    split = None if a.split == "all" else a.split
    depth_edges = None if a.by_depth is None else (tuple(a.by_depth) or DEPTH_EDGES_M)
    if a.checkpoint:
        rep, pred, hm = _evaluate(a.checkpoint, dem, mask, nodata=nodata, cellsize=c, split=split, block=a.block, tile=a.tile,
                                  holes=HoleSpec(), seed=a.seed, window=a.window, overlap=a.overlap, batch=a.batch,
                                  objects=objects, area_edges_m2=AREA_EDGES_M2, quantiles=QUANTILES, top=10,
                                  baseline=a.baseline, fallback=a.fallback, seam=a.seam, model_cellsize=a.model_cellsize,
                                  min_coverage=a.min_coverage, solver=a.solver, depth_edges_m=depth_edges,
                                  compare=a.compare, sinks=a.sinks, drainage=a.drainage, stream_cells=a.stream_cells,
                                  stream_tol_m=a.stream_tol, flood=a.flood, flood_stages_m=tuple(a.flood_stages),
                                  wetness=a.wetness, wetness_exponent=a.exponent, wetness_min_slope=a.min_slope,
                                  texture=a.texture, texture_octaves=a.octaves, kriging=a.kriging, tta=a.tta,
                                  simulate=a.simulate, natural=a.natural, natural_radius=a.natural_radius)
    else:
        p, ph = read_asc(a.pred)
        if p.shape != dem.shape:
            raise ValueError(f"{a.pred} is {p.shape[0]}x{p.shape[1]}, the dem {dem.shape[0]}x{dem.shape[1]}")
        pnd = asc_nodata(ph)
        if pnd is not None:
            p = np.where(p == np.float32(pnd), np.float32(np.nan), p)     # unfilled cells stay unfilled
        hm, keep, _ = holes_from_map(dem, read_mask(a.holes, dem.shape), mask, nodata=nodata, objects=objects, cellsize=c)
        rep = terrain_errors(dem, p, hm, keep, cellsize=c, mask=mask, nodata=nodata, depth_edges_m=depth_edges)
        rep.update(params(c, split, a.block, a.tile, a.seed, HoleSpec()))
        if a.sinks:
            rep["sinks"] = sink_errors(dem, p, hm, cellsize=c, mask=mask, nodata=nodata)
        drn = {"drainage": a.drainage, "stream_cells": a.stream_cells, "stream_tol_m": a.stream_tol, "flood": a.flood,
               "flood_stages_m": tuple(a.flood_stages), "wetness": a.wetness, "wetness_exponent": a.exponent,
               "wetness_min_slope": a.min_slope, "texture": a.texture, "texture_octaves": a.octaves}
        if a.drainage:
            rep["drainage"] = drainage_errors(dem, p, hm, cellsize=c, mask=mask, nodata=nodata, stream_cells=a.stream_cells,
                                              stream_tol_m=a.stream_tol)
        if a.flood:
            rep["flood"] = flood_errors(dem, p, hm, cellsize=c, mask=mask, nodata=nodata, stream_cells=a.stream_cells,
                                        stages_m=tuple(a.flood_stages))
        if a.wetness:
            rep["wetness"] = wetness_errors(dem, p, hm, cellsize=c, mask=mask, nodata=nodata, exponent=a.exponent,
                                            min_slope=a.min_slope)
        if a.texture:
            rep["texture"] = texture_errors(dem, p, hm, cellsize=c, mask=mask, nodata=nodata, octaves=a.octaves)
        if a.baseline:
            rep["baseline"] = baseline_report(dem, hm, keep, cellsize=c, mask=mask, nodata=nodata, method=a.baseline,
                                              solver=a.solver, depth_edges_m=depth_edges, sinks=a.sinks, **drn)
        if a.compare:
            rep["compare"] = compare_report(dem, hm, keep, a.compare, cellsize=c, mask=mask, nodata=nodata,
                                            depth_edges_m=depth_edges, sinks=a.sinks, **drn)
        if a.kriging:
            rep["kriging"] = kriging_report(dem, hm, keep, cellsize=c, mask=mask, nodata=nodata, depth_edges_m=depth_edges,
                                            sinks=a.sinks, **drn)
        if a.simulate:
            rep["simulation"] = simulation_report(dem, hm, keep, cellsize=c, realisations=a.simulate, mask=mask, nodata=nodata,
                                                  seed=a.seed, depth_edges_m=depth_edges, texture_octaves=a.octaves)
        if a.natural:
            rep["natural"] = natural_report(dem, hm, keep, cellsize=c, mask=mask, nodata=nodata, radius=a.natural_radius,
                                            depth_edges_m=depth_edges, sinks=a.sinks, **drn)
        pred = None
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rep, f, indent=1)
    if a.pred_out and pred is not None:
        out = pred.cpu().numpy()
        write_asc(a.pred_out, out, with_nodata(header) if np.isnan(out).any() else header)
    if a.holes_out and hm is not None:
        write_mask(a.holes_out, hm.cpu().numpy(), header)
    print(summary(rep))
    if "spread" in rep:
        sp = rep["spread"]
        print(f"tta {sp['members']}: spread mean {sp['mean_m']:.4g} m, max {sp['max_m']:.4g} m; {calibration_summary(sp['calibration'])}")
    if "sinks" in rep:
        print(sinks_summary(rep["sinks"]))
    if "drainage" in rep:
        print(drainage_summary(rep["drainage"]))
    if "flood" in rep:
        print(flood_summary(rep["flood"]))
    if "wetness" in rep:
        print(wetness_summary(rep["wetness"]))
    if "texture" in rep:
        print(texture_summary(rep["texture"]))
    if "seam" in rep:
        sm = rep["seam"]
        print(f"seam {a.seam}: {sm['ring']} ring / {sm['interior']} interior pixels, max_delta {sm['max_delta']:.4g} m, "
              f"{sm['cycles']} cycles, converged {sm['converged']}")
    if "baseline" in rep:
        how = "" if a.solver == "mg" else f" (solver {a.solver})"
        print(f"baseline {rep['baseline']['method']}{how}: {summary(rep['baseline'])}")
        if "sinks" in rep["baseline"]:
            print(f"baseline {rep['baseline']['method']} {sinks_summary(rep['baseline']['sinks'])}")
        if "drainage" in rep["baseline"]:
            print(f"baseline {rep['baseline']['method']} {drainage_summary(rep['baseline']['drainage'])}")
        if "flood" in rep["baseline"]:
            print(f"baseline {rep['baseline']['method']} {flood_summary(rep['baseline']['flood'])}")
        if "wetness" in rep["baseline"]:
            print(f"baseline {rep['baseline']['method']} {wetness_summary(rep['baseline']['wetness'])}")
        if "texture" in rep["baseline"]:
            print(f"baseline {rep['baseline']['method']} {texture_summary(rep['baseline']['texture'])}")
    for name, r in rep.get("compare", {}).items():
        print(f"compare {name}: {summary(r)}")
        if "sinks" in r:
            print(f"compare {name} {sinks_summary(r['sinks'])}")
        if "drainage" in r:
            print(f"compare {name} {drainage_summary(r['drainage'])}")
        if "flood" in r:
            print(f"compare {name} {flood_summary(r['flood'])}")
        if "wetness" in r:
            print(f"compare {name} {wetness_summary(r['wetness'])}")
        if "texture" in r:
            print(f"compare {name} {texture_summary(r['texture'])}")
    if "kriging" in rep:
        r = rep["kriging"]
        print(f"kriging: {summary(r)}")
        print(f"kriging {calibration_summary(r['calibration'])}")
        for key, line in (("sinks", sinks_summary), ("drainage", drainage_summary), ("flood", flood_summary),
                          ("wetness", wetness_summary), ("texture", texture_summary)):
            if key in r:
                print(f"kriging {line(r[key])}")
    if "simulation" in rep:
        r = rep["simulation"]
        print(f"simulation, mean of {r['realisations']}: {summary(r)}")
        print(f"simulation {calibration_summary(r['calibration'])}")
        print(f"simulation, realisation 0: {texture_summary(r['texture'])}")
    if "natural" in rep:
        r = rep["natural"]
        print(f"natural, radius {r['fill']['radius']}: {summary(r)}")
        for key, line in (("sinks", sinks_summary), ("drainage", drainage_summary), ("flood", flood_summary),
                          ("wetness", wetness_summary), ("texture", texture_summary)):
            if key in r:
                print(f"natural {line(r[key])}")
    return rep


if __name__ == "__main__":
    main()
