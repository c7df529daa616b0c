"""Fill the depressions (closed pits) of a DEM on the GPU (csrc/depfill.hip): the surface a flood or runoff
model needs, and a measure of what a void fill does to the drainage (evaluate_raster's sink statistics).

A pixel is known by the rule of inpaint_raster, fill_voids and interpolate_voids (mask != 0, finite, != nodata;
tg_objmask_known).  An outlet is a known pixel on the raster's edge or with an unknown neighbour: water leaves through the edge
and into voids (RichDEM's convention).  Every known pixel is raised to

    W(p) = min over paths of known pixels from p to an outlet of the max of z along the path,

the level at which water standing on p spills; paths are 8-connected (connectivity=8, the default) or 4-connected.  Unknown
pixels come back NaN.  Only min and max of float32 values are taken, so the result is exact: bitwise equal to a priority-flood
(Barnes et al. 2014) on the CPU, bitwise reproducible, and every value is either z's own or the bits of some other known z.  No
epsilon gradient is put on the filled flats.

The GPU iterates W <- max(z, min(W, min over the neighbours W)) from W = z at the outlets and +inf elsewhere, tile by tile, only
where something changed; `check_every` sweeps are enqueued between two looks at the change counter (one host sync each), at most
`max_sweeps` in all.  If that limit stops the iteration, info["converged"] is False, every finite value is still >= the exact
one, and the pixels no value has reached are NaN (info["unreached"]).

info: known, unknown, outlets, raised (pixels above z), unreached, depressions (the 8-connected components of the raised pixels,
whatever `connectivity` is), depth_sum_m (the fp64 sum of the rises, in a fixed order: bitwise reproducible), volume_m3 =
cellsize^2 * depth_sum_m, max_depth_m, sweeps, tile_visits (both may differ between runs; the raster does not), converged,
connectivity.

CLI: python -m mvp_gan.src.fill_depressions --dem in.asc --out filled.asc [--mask m.png|m.asc] [--nodata v]
         [--connectivity 4|8] [--depth-out depth.asc] [--max-sweeps n]       (cellsize from the header; NaN -> NODATA_value)
"""
import argparse

import torch

from . import raster_args as R

CONNECTIVITIES = (8, 4)
MAX_SWEEPS = 4096
CHECK_EVERY = 8


def check_args(dem, mask, cellsize, connectivity, max_sweeps, check_every, who="fill_depressions"):
    """Host-side rejection before any launch; -> (H, W, cellsize)."""
    shape = R.raster_shape(dem, mask, who, what="dem must be [H, W], non-empty")
    if isinstance(connectivity, bool) or connectivity not in CONNECTIVITIES:
        raise ValueError(f"{who}: connectivity {connectivity!r} must be 8 or 4")
    R.count(max_sweeps, 1, "max_sweeps", who)
    R.count(check_every, 1, "check_every", who)
    return shape[0], shape[1], R.cellsize(cellsize, who)


def run_until_unchanged(enqueue, changed, cap, check_every):
    """enqueue(n) queues n steps, the last of which counts what it changed into `changed` (int32 [1] on the device); at most
    `cap` steps, one host sync per check_every -> (steps enqueued, converged)."""
    steps, converged = 0, False
    while steps < cap and not converged:
        n = min(check_every, cap - steps)
        enqueue(n)
        steps += n
        converged = int(changed.item()) == 0
    return steps, converged


def run_doubling(enqueue, state, max_rounds, check_every, who):
    """enqueue(k, n) queues rounds k .. k + n - 1 of a pointer doubling and its (live pointers, rounds that ran) into `state`
    (int32 [2] on the device); one host sync per check_every rounds -> rounds that ran."""
    k, left, rounds = 0, 1, 0
    while left and k < max_rounds:
        n = min(check_every, max_rounds - k)
        enqueue(k, n)
        k += n
        left, rounds = state.cpu().tolist()
    if left:
        raise RuntimeError(f"{who}: the direction grid has a cycle")
    return rounds


def relax(z, known, connectivity=8, max_sweeps=MAX_SWEEPS, check_every=CHECK_EVERY):
    """The iteration on device tensors: z float32 [H][W], known uint8 [H][W] -> (w float32 [H][W] as tg_depfill_sweep leaves
    it, outlets, sweeps, tile_visits, converged).  One host sync per check_every sweeps."""
    from tg_hip import ops as O
    H, W = z.shape
    ws = O.depfill_ws(H, W, z.device)
    w = O.depfill_init(z, known, connectivity, ws)
    outlets = int((w == z).count_nonzero().item())              # after init W == z exactly at the outlets (NaN != NaN)
    changed = torch.zeros(1, dtype=torch.int32, device=z.device)
    visits = torch.zeros(1, dtype=torch.int64, device=z.device)
    sweeps, converged = run_until_unchanged(lambda n: O.depfill_sweep(z, known, connectivity, n, w, changed, visits, ws), changed,
                                            max_sweeps, check_every)
    return w, outlets, sweeps, int(visits.item()), converged


def stats_dict(counts, sums, cellsize):
    """tg_depfill_stats' numbers -> {cells, unreached, counted, depth_sum_m, volume_m3, max_depth_m} (pure)."""
    c = [int(v) for v in counts]
    s = [float(v) for v in sums]
    return {"cells": c[0], "unreached": c[1], "counted": c[2], "depth_sum_m": s[0], "volume_m3": cellsize * cellsize * s[0],
            "max_depth_m": s[1]}


def count_depressions(flags):
    """The number of 8-connected components of flags (uint8 [H][W]) through tg_objmask_components."""
    from tg_hip import ops as O
    H, W = flags.shape
    labels, _ = O.objmask_components(flags)
    own = torch.arange(H * W, dtype=torch.int32, device=flags.device).view(H, W)
    return int((labels == own).count_nonzero().item())          # a component's label is the index of one of its pixels


@torch.no_grad()
def fill_depressions(dem, mask=None, *, nodata=None, cellsize=1.0, connectivity=8, max_sweeps=MAX_SWEEPS,
                     check_every=CHECK_EVERY, want_depth=False):
    """dem: float32 [H][W] (numpy or HIP tensor); mask: same shape, nonzero = known (optional).  Returns (raster float32 HIP
    tensor [H][W], info) or, with want_depth, (raster, depth float32 [H][W] = raster - dem: 0 where not raised, NaN where the
    raster is, info)."""
    from tg_hip import ops as O
    H, W, c = check_args(dem, mask, cellsize, connectivity, max_sweeps, check_every)
    z, known = R.upload_known(dem, mask, nodata, "fill_depressions")
    w, outlets, sweeps, visits, converged = relax(z, known, connectivity, max_sweeps, check_every)
    counts, sums = O.depfill_stats(z, w, known)
    out, depth, flags = O.depfill_finish(z, w, known, want_depth=want_depth, want_flags=True)
    st = stats_dict(counts.cpu().tolist(), sums.cpu().tolist(), c)
    info = {"known": st["counted"], "unknown": H * W - st["counted"], "outlets": outlets, "raised": st["cells"],
            "unreached": st["unreached"], "depressions": count_depressions(flags), "depth_sum_m": st["depth_sum_m"],
            "volume_m3": st["volume_m3"], "max_depth_m": st["max_depth_m"], "sweeps": sweeps, "tile_visits": visits,
            "converged": converged, "connectivity": connectivity}
    return (out, depth, info) if want_depth else (out, info)


# ---- CLI ------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="Fill the depressions (closed pits) of an ESRI ASCII grid DEM: every cell is raised "
                                             "to the level at which it drains to the grid's edge or into a void.")
    ap.add_argument("--dem", required=True, help="input .asc raster (NODATA_value cells are voids: water leaves into them)")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = known, 0 = void")
    ap.add_argument("--nodata", type=float, help="nodata value (default: the .asc header's NODATA_value)")
    ap.add_argument("--connectivity", type=int, choices=CONNECTIVITIES, default=8, help="water flows to 8 or to 4 neighbours")
    ap.add_argument("--max-sweeps", type=int, default=MAX_SWEEPS, help="stop after this many sweeps even if not converged")
    ap.add_argument("--depth-out", help="also write the depth of the fill (.asc): filled - dem")
    ap.add_argument("--out", required=True, help="output .asc raster")
    return ap


def main(argv=None):
    from .asc import read_inputs, with_nodata, write_asc
    a = build_parser().parse_args(argv)
    dem, header, mask, nodata, cellsize = read_inputs(a)
    out, depth, info = fill_depressions(dem, mask, nodata=nodata, cellsize=cellsize, connectivity=a.connectivity,
                                        max_sweeps=a.max_sweeps, want_depth=True)
    if info["unknown"] or info["unreached"]:
        header = with_nodata(header)
    write_asc(a.out, out.cpu().numpy(), header)
    if a.depth_out:
        write_asc(a.depth_out, depth.cpu().numpy(), header)
    how = "" if info["converged"] else f" (NOT converged after {info['sweeps']} sweeps: {info['unreached']} cells unreached)"
    print(f"{a.out}: {info['raised']} of {info['known']} cells raised in {info['depressions']} depressions, volume "
          f"{info['volume_m3']:.6g} m3, deepest {info['max_depth_m']:.6g} m, {info['sweeps']} sweeps{how}")
    return info


if __name__ == "__main__":
    main()
