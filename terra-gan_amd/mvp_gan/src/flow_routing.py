"""D8 flow directions, flat resolution and flow accumulation of a DEM on the GPU (csrc/flow.hip): the
direction grid, the contributing area and the stream network of a bare-earth model.

A pixel is known by the rule of fill_depressions (mask != 0, finite, != nodata; tg_objmask_known).  An outlet is a known pixel on
the raster's edge or with an unknown 8-neighbour.  With fill=True (the default) the depressions are filled first
(fill_depressions' relax / finish at connectivity 8, on the same known mask) and the filled surface w is routed; with fill=False
the raster is routed as given.

direction (uint8): 0 unknown; 1..8 the receiver E, SE, S, SW, W, NW, N, NE (ESRI: 1 << (code - 1), to_esri); OUT = 9, an outlet
that drains off the raster or into a void; PIT = 255, no receiver.  Equal candidates are taken in the order E, S, W, N, SE, SW,
NW, NE.

  slope step   for a known neighbour n of p: d = w(p) - w(n) in float32, s = d for a cardinal n and d * float32(0x1.6a09e6p-1)
               for a diagonal one.  If some s > 0, p flows to the neighbour with the largest s; otherwise an outlet gets OUT and
               any other pixel is undecided.
  flats        D = 0 on decided pixels; for an undecided pixel D(p) is the smallest number of 8-connected steps through pixels of
               p's own height to a decided pixel of that height ("towards lower" of Barnes et al. 2014, independent of the
               schedule).  p flows to the neighbour of its height with D(p) - 1; with no such path (D infinite) it is a PIT: a
               true pit or a closed flat of an unfilled input.  On a converged fill there are none.
  accumulation A(p) = 1 + the sum of A(q) over the pixels q whose receiver is p: int32, in cells, exact; 0 at unknown pixels.
               OUT and PIT pixels accumulate and pass nothing on.

Everything is exact: bitwise equal to the numpy oracle of tests/flow_oracle.py and bitwise reproducible.  `check_every` flat
sweeps (and doubling rounds of the accumulation) are enqueued between two read-backs, at most `max_sweeps` sweeps for the fill
and as many for the flats.  If a limit stops either, info["converged"] is False: the flat pixels no distance has reached are PIT,
the others follow a decreasing D, and direction is still a forest.

info: known, unknown, outlets, flat_cells (pixels that got their code from D), pits, max_accumulation, max_area_m2 = cellsize^2 *
max_accumulation, flat_sweeps, tile_visits (both may differ between runs; the rasters do not), acc_rounds, converged, filled.

CLI: python -m mvp_gan.src.flow_routing --dem in.asc --dir-out d.asc --acc-out a.asc [--mask m.png|m.asc] [--nodata v]
         [--no-fill] [--esri] [--streams-out s.asc --min-cells n] [--max-sweeps n]       (cellsize from the header)
"""
import argparse
import math

import numpy as np
import torch

from .fill_depressions import CHECK_EVERY, MAX_SWEEPS, check_args

OUT, PIT, UNKNOWN = 9, 255, 0
FAR = 0x7fffffff
ACC_MAX_ROUNDS = 32
# code -> ESRI: unknown 255, 1..8 -> 1, 2, 4, ..., 128, OUT and PIT 0
_ESRI = np.zeros(256, np.uint8)
_ESRI[0] = 255
_ESRI[1:9] = 1 << np.arange(8)


def to_esri(direction):
    """Codes (numpy or tensor, uint8) -> ESRI flow directions: 1 = E, 2 = SE, ..., 128 = NE; OUT and PIT 0; unknown 255."""
    if isinstance(direction, torch.Tensor):
        if direction.dtype != torch.uint8:
            raise ValueError(f"to_esri: direction must be uint8, got {direction.dtype}")
        return torch.from_numpy(_ESRI).to(direction.device)[direction.long()]
    d = np.asarray(direction)
    if d.dtype != np.uint8:
        raise ValueError(f"to_esri: direction must be uint8, got {d.dtype}")
    return _ESRI[d]


def streams(accumulation, min_cells):
    """-> uint8 mask (numpy or tensor, as the input): 1 where accumulation >= min_cells (an integer >= 1)."""
    if isinstance(min_cells, bool) or not isinstance(min_cells, int) or min_cells < 1:
        raise ValueError(f"streams: min_cells {min_cells!r} must be an integer >= 1")
    if isinstance(accumulation, torch.Tensor):
        return (accumulation >= min_cells).to(torch.uint8)
    return (np.asarray(accumulation) >= min_cells).astype(np.uint8)


def resolve_flats(w, D, ws, max_sweeps=MAX_SWEEPS, check_every=CHECK_EVERY):
    """The flat sweeps on device tensors (w float32 [H][W], D and ws as ops.flow_slope leaves them) -> (sweeps, tile_visits,
    converged).  One host sync per check_every sweeps."""
    from tg_hip import ops as O
    changed = torch.zeros(1, dtype=torch.int32, device=w.device)
    visits = torch.zeros(1, dtype=torch.int64, device=w.device)
    sweeps, converged = 0, False
    while sweeps < max_sweeps and not converged:
        n = min(check_every, max_sweeps - sweeps)
        O.flow_flat_sweep(w, n, D, changed, visits, ws)
        sweeps += n
        converged = int(changed.item()) == 0
    return sweeps, int(visits.item()), converged


def accumulate(direction, ws, check_every=CHECK_EVERY):
    """The accumulation of a direction grid (uint8 HIP tensor [H][W]) -> (acc int32 [H][W], max, rounds).  One host sync per
    check_every rounds of the doubling."""
    from tg_hip import ops as O
    H, W = direction.shape
    O.flow_accum_init(direction, ws)
    state = torch.empty(2, dtype=torch.int32, device=direction.device)
    k, left, rounds = 0, 1, 0
    while left and k < ACC_MAX_ROUNDS:
        n = min(check_every, ACC_MAX_ROUNDS - k)
        O.flow_accum(H, W, k, n, state, ws)
        k += n
        left, rounds = state.cpu().tolist()
    if left:
        raise RuntimeError("flow_routing: the direction grid has a cycle")      # cannot happen: (w, D) decreases along every edge
    acc, amax = O.flow_accum_finish(H, W, rounds, ws)
    return acc, int(amax.item()), rounds


@torch.no_grad()
def flow_routing(dem, mask=None, *, nodata=None, cellsize=1.0, fill=True, max_sweeps=MAX_SWEEPS, check_every=CHECK_EVERY):
    """dem: float32 [H][W] (numpy or HIP tensor); mask: same shape, nonzero = known (optional).  Returns (direction uint8 HIP
    tensor [H][W], accumulation int32 HIP tensor [H][W], info)."""
    from tg_hip import ops as O
    from .fill_depressions import relax
    from .fill_voids import _device_f32
    who = "flow_routing"
    H, W, c = check_args(dem, mask, cellsize, 8, max_sweeps, check_every, who=who)
    if not isinstance(fill, bool):
        raise ValueError(f"{who}: fill {fill!r} must be True or False")
    if not torch.cuda.is_available():
        raise RuntimeError("flow_routing: no HIP device visible; this build has no CPU path")
    device = torch.device("cuda", torch.cuda.current_device())
    z = _device_f32(dem, device, "dem", who=who)
    m = None if mask is None else _device_f32(mask, device, "mask", binary=True, who=who)
    if nodata is not None and math.isnan(nodata):
        nodata = None                                           # NaN is never a value: non-finite pixels are unknown already
    known, _ = O.objmask_known(z, m, nodata, transposed=False)
    converged = True
    if fill:
        state, _, _, _, converged = relax(z, known, 8, max_sweeps, check_every)
        w, _, _ = O.depfill_finish(z, state, known)             # NaN where the fill has not arrived: such a pixel ends as a PIT
    else:
        w = z
    ws = O.flow_ws(H, W, device)
    direction, D, c0 = O.flow_slope(w, known, ws)
    sweeps, visits, flat_converged = resolve_flats(w, D, ws, max_sweeps, check_every)
    c1 = O.flow_flat_dir(w, D, direction)
    acc, amax, rounds = accumulate(direction, ws, check_every)
    nknown, outlets = c0.cpu().tolist()
    flat_cells, pits = c1.cpu().tolist()
    info = {"known": nknown, "unknown": H * W - nknown, "outlets": outlets, "flat_cells": flat_cells, "pits": pits,
            "max_accumulation": amax, "max_area_m2": c * c * amax, "flat_sweeps": sweeps, "tile_visits": visits,
            "acc_rounds": rounds, "converged": bool(converged and flat_converged), "filled": fill}
    return direction, acc, info


# ---- CLI ------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description="D8 flow directions and flow accumulation of an ESRI ASCII grid DEM: depressions "
                                             "are filled, flats resolved towards their outlets, contributing areas counted.")
    ap.add_argument("--dem", required=True, help="input .asc raster (NODATA_value cells are voids: water leaves into them)")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = known, 0 = void")
    ap.add_argument("--nodata", type=float, help="nodata value (default: the .asc header's NODATA_value)")
    ap.add_argument("--no-fill", action="store_true", help="route the raster as given: its pits and closed flats become PIT")
    ap.add_argument("--esri", action="store_true", help="write ESRI direction codes (1, 2, 4, ..., 128; 0 = outlet or pit; 255 "
                                                        "= void) instead of 1..8, 9 = OUT, 255 = PIT, 0 = void")
    ap.add_argument("--max-sweeps", type=int, default=MAX_SWEEPS, help="stop the fill and the flat resolution after this many "
                                                                       "sweeps each even if not converged")
    ap.add_argument("--streams-out", help="also write the stream mask (.asc): 1 where the accumulation >= --min-cells")
    ap.add_argument("--min-cells", type=int, help="stream threshold in cells (required with --streams-out)")
    ap.add_argument("--dir-out", required=True, help="output .asc raster of direction codes")
    ap.add_argument("--acc-out", required=True, help="output .asc raster of the flow accumulation in cells")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if (a.streams_out is None) != (a.min_cells is None):
        ap.error("--streams-out and --min-cells go together")
    if a.min_cells is not None and a.min_cells < 1:
        ap.error("--min-cells must be >= 1")
    return a


def write_int_asc(path, arr, header):
    """An integer grid under read_asc's header, without its NODATA_value (every code is a value); exact for any int32."""
    from .inpaint_raster import asc_value
    arr = np.asarray(arr)
    if arr.shape != (int(asc_value(header, "nrows")), int(asc_value(header, "ncols"))):
        raise ValueError(f"write_int_asc: array {arr.shape} does not match the header")
    with open(path, "w") as f:
        for k, v in header:
            if k.lower() != "nodata_value":
                f.write(f"{k} {v}\n")
        for row in arr.astype(np.int64):
            f.write(" ".join(map(str, row.tolist())) + "\n")


def main(argv=None):
    from .inpaint_raster import _read_mask, asc_nodata, asc_value, read_asc
    a = parse_args(argv)
    dem, header = read_asc(a.dem)
    mask = _read_mask(a.mask, dem.shape) if a.mask else None
    nodata = a.nodata if a.nodata is not None else asc_nodata(header)
    direction, acc, info = flow_routing(dem, mask, nodata=nodata, cellsize=float(asc_value(header, "cellsize")),
                                        fill=not a.no_fill, max_sweeps=a.max_sweeps)
    write_int_asc(a.dir_out, (to_esri(direction) if a.esri else direction).cpu().numpy(), header)
    write_int_asc(a.acc_out, acc.cpu().numpy(), header)
    if a.streams_out:
        write_int_asc(a.streams_out, streams(acc, a.min_cells).cpu().numpy(), header)
    how = "" if info["converged"] else f" (NOT converged after {info['flat_sweeps']} flat sweeps: unresolved flat cells are pits)"
    print(f"{a.dir_out}: {info['known']} cells, {info['outlets']} outlets, {info['flat_cells']} flat cells, {info['pits']} pits, "
          f"largest contributing area {info['max_accumulation']} cells = {info['max_area_m2']:.6g} m2, "
          f"{info['flat_sweeps']} flat sweeps, {info['acc_rounds']} accumulation rounds{how}")
    return info


if __name__ == "__main__":
    main()
