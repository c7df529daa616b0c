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

watersheds(direction, pour_points) follows every pixel's path to its end by a gather-only pointer doubling (csrc/drainage.hip,
DESIGN.md section 8w): the basin of every pixel (the pixel its water ends at, or a pour point on the way) and the length of the
path there in metres, exact and bitwise reproducible.

stream_network(direction, accumulation, min_cells) gives the streams their structure: the class of every
stream pixel (head, interior, junction), the link it belongs to and its Strahler order; hand(dem, ...) the height of every pixel
above the drainage pixel its water reaches first and the flow length to it.  Exact and bitwise reproducible as well.

mfd_accumulation(dem, ...) is the contributing area by a multiple-flow-direction rule (csrc/mfd.hip): on
hillslopes, where D8 draws parallel stripes, every pixel spreads over all its lower neighbours; terrain_slope(dem, ...) is Horn's
slope and wetness_index(dem, ...) the topographic wetness index ln(a / tan(beta)) built on the two.  The accumulation is float64
in a fixed order, bitwise equal to tests/mfd_oracle.py and bitwise reproducible.

CLI: python -m mvp_gan.src.flow_routing --dem in.asc --dir-out d.asc --acc-out a.asc [--mask m.png|m.asc] [--nodata v]
         [--no-fill] [--esri] [--streams-out s.asc --min-cells n] [--max-sweeps n]       (cellsize from the header)
         [--basins-out b.asc [--pour p.png|p.asc] [--compact]] [--length-out l.asc]
         [--order-out o.asc] [--links-out l.asc] [--hand-out h.asc [--hand-distance-out d.asc] [--min-order k]]   (with --min-cells)
         [--mfd-acc-out m.asc] [--slope-out s.asc] [--twi-out t.asc [--min-slope s]] [--exponent e]
"""
import argparse
import math
import numbers

import numpy as np
import torch

from . import raster_args as R
from .fill_depressions import CHECK_EVERY, MAX_SWEEPS, check_args, run_doubling, run_until_unchanged

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
    sweeps, converged = run_until_unchanged(lambda n: O.flow_flat_sweep(w, n, D, changed, visits, ws), changed, max_sweeps,
                                            check_every)
    return sweeps, int(visits.item()), converged


def accumulate(direction, ws, check_every=CHECK_EVERY):
    """The accumulation of a direction grid (uint8 HIP tensor [H][W]) -> (acc int32 [H][W], max, rounds).  One host sync per
    check_every rounds of the doubling."""
    from tg_hip import ops as O
    H, W = direction.shape
    O.flow_accum_init(direction, ws)
    state = torch.empty(2, dtype=torch.int32, device=direction.device)
    # a cycle cannot happen in flow_routing's own grids: (w, D) decreases along every edge
    rounds = run_doubling(lambda k, n: O.flow_accum(H, W, k, n, state, ws), state, ACC_MAX_ROUNDS, check_every, "flow_routing")
    acc, amax = O.flow_accum_finish(H, W, rounds, ws)
    return acc, int(amax.item()), rounds


@torch.no_grad()
def flow_routing(dem, mask=None, *, nodata=None, cellsize=1.0, fill=True, max_sweeps=MAX_SWEEPS, check_every=CHECK_EVERY):
    """dem: float32 [H][W] (numpy or HIP tensor); mask: same shape, nonzero = known (optional).  Returns (direction uint8 HIP
    tensor [H][W], accumulation int32 HIP tensor [H][W], info)."""
    return route_raster(dem, mask, nodata, cellsize, fill, max_sweeps, check_every, "flow_routing")[:3]


def route_raster(dem, mask, nodata, cellsize, fill, max_sweeps, check_every, who):
    """flow_routing's checks, upload and known mask -> (direction, accumulation, info, w: the surface that was routed)."""
    z, known, c = _upload(dem, mask, nodata, cellsize, fill, max_sweeps, check_every, who)
    return route_known(z, known, c, fill=fill, max_sweeps=max_sweeps, check_every=check_every, return_surface=True)


def _upload(dem, mask, nodata, cellsize, fill, max_sweeps, check_every, who):
    """flow_routing's checks, upload and known mask -> (z float32 [H][W], known uint8 [H][W], cellsize)."""
    _, _, c = check_args(dem, mask, cellsize, 8, max_sweeps, check_every, who=who)
    if not isinstance(fill, bool):
        raise ValueError(f"{who}: fill {fill!r} must be True or False")
    z, known = R.upload_known(dem, mask, nodata, who)
    return z, known, c


def route_known(z, known, cellsize, *, fill=True, max_sweeps=MAX_SWEEPS, check_every=CHECK_EVERY, return_surface=False):
    """flow_routing's body on device tensors with a ready known mask: z float32 [H][W], known uint8 [H][W] (tg_objmask_known's
    map, or the intersection of two) -> (direction, accumulation, info); with return_surface=True also w, the surface that was
    routed (the filled one with fill=True, else z itself)."""
    from tg_hip import ops as O
    from .fill_depressions import relax
    H, W = z.shape
    c = cellsize
    device = z.device
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
    if return_surface:
        return direction, acc, info, w
    return direction, acc, info


# ---- watersheds and flow length ---------------------------------------------------------------------------------------
SQRT2 = 1.4142135623730951


def check_watershed_args(direction, pour_points, cellsize, compact, check_every, who="watersheds"):
    """Host-side rejection before any launch; -> (H, W, cellsize)."""
    shape = R.raster_shape(direction, None, who, what="direction must be [H, W], non-empty")
    dt = direction.dtype if isinstance(direction, (torch.Tensor, np.ndarray)) else None
    if dt not in (torch.uint8, np.dtype(np.uint8)):
        raise ValueError(f"{who}: direction must be a uint8 grid of flow_routing's codes, got {dt}")
    if pour_points is not None and R.shape(pour_points) != shape:
        raise ValueError(f"{who}: pour_points {R.shape(pour_points)} differs from the direction grid {shape}")
    if not isinstance(compact, bool):
        raise ValueError(f"{who}: compact {compact!r} must be True or False")
    R.count(check_every, 1, "check_every", who)
    return shape[0], shape[1], R.cellsize(cellsize, who)


def basin_doubling(d, pour, ws, check_every=CHECK_EVERY):
    """The doubling on device tensors (d uint8 [H][W], pour uint8 [H][W] or None) -> (rounds, pour points used, ignored); the
    records stay in ws for ops.flow_basin_finish.  One host sync per check_every rounds."""
    from tg_hip import ops as O
    H, W = d.shape
    pc = O.flow_basin_init(d, pour, ws)
    rounds = basin_rounds(H, W, ws, check_every)
    used, ignored = pc.cpu().tolist()
    return rounds, used, ignored


def basin_rounds(H, W, ws, check_every=CHECK_EVERY, who="watersheds"):
    """The rounds of the doubling on the start records in ws (ops.flow_basin_init's or ops.stream_class's) -> rounds that ran."""
    from tg_hip import ops as O
    state = torch.empty(2, dtype=torch.int32, device=ws.device)
    return run_doubling(lambda k, n: O.flow_basin(H, W, k, n, state, ws), state, ACC_MAX_ROUNDS, check_every, who)


def compact_labels(basin):
    """basin int32 [H][W] of terminal indices (-1 unknown) -> the rank 1..n of the terminal in raster order, 0 where unknown."""
    flat = basin.reshape(-1)
    idx = torch.arange(flat.numel(), dtype=torch.int32, device=flat.device)
    rank = torch.cumsum((flat == idx).to(torch.int32), 0, dtype=torch.int32)
    out = rank[flat.clamp(min=0).long()]
    return torch.where(flat >= 0, out, torch.zeros_like(out)).reshape(basin.shape)


@torch.no_grad()
def watersheds(direction, pour_points=None, *, cellsize=1.0, compact=False, check_every=CHECK_EVERY):
    """direction: uint8 [H][W] of flow_routing's codes (numpy or HIP tensor); pour_points: same shape, nonzero = pour point
    (optional).  Every pixel's path is followed to its last pixel T: an OUT, a PIT, a pour point, or a pixel whose receiver
    lies off the raster.  Returns (basin int32 HIP tensor [H][W]: T as y * W + x, -1 where unknown; with compact=True the rank
    1..n of T in raster order, 0 where unknown; length_m float32 HIP tensor [H][W] = float32(cellsize * (nc + sqrt(2) nd)) for
    nc cardinal and nd diagonal steps to T, in float64 with SQRT2; info: basins, rounds, longest_steps, max_length_m,
    pour_points, pour_ignored).  Exact and bitwise reproducible (csrc/drainage.hip)."""
    from tg_hip import ops as O
    who = "watersheds"
    H, W, c = check_watershed_args(direction, pour_points, cellsize, compact, check_every, who)
    device = R.device(who)
    d = R.to_u8(direction, device, "direction", who)
    if bool(torch.any(d == 254)):
        raise ValueError(f"{who}: the direction grid holds the code 254 (undecided): route it to the end first")
    pour = None if pour_points is None else R.to_u8(pour_points, device, "pour_points", who, nonzero=True)
    ws = O.flow_basin_ws(H, W, device)
    rounds, used, ignored = basin_doubling(d, pour, ws, check_every)
    basin, _, _, length, counts = O.flow_basin_finish(H, W, rounds, ws, c)
    terminals, longest, bits = counts.cpu().tolist()
    if compact:
        basin = compact_labels(basin)
    info = {"basins": terminals, "rounds": rounds, "longest_steps": longest, "max_length_m": R.bits_f32(bits),
            "pour_points": used, "pour_ignored": ignored}
    return basin, length, info


# ---- stream network: classes, links, Strahler order ------------------------------------------------------------------
ORDER_MAX_ROUNDS = 65536


def _min_cells(n, who):
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n < 2 ** 31:
        raise ValueError(f"{who}: min_cells {n!r} must be an integer in [1, 2^31)")
    return n


def check_stream_args(direction, accumulation, min_cells, cellsize, max_rounds, check_every, who="stream_network"):
    """Host-side rejection before any launch; -> (H, W, cellsize)."""
    H, W, c = check_watershed_args(direction, None, cellsize, False, check_every, who)
    if R.shape(accumulation) != (H, W):
        raise ValueError(f"{who}: accumulation {R.shape(accumulation)} differs from the direction grid {(H, W)}")
    dt = accumulation.dtype if isinstance(accumulation, (torch.Tensor, np.ndarray)) else None
    if dt not in (torch.int32, np.dtype(np.int32)):
        raise ValueError(f"{who}: accumulation must be an int32 grid of flow_routing's counts, got {dt}")
    _min_cells(min_cells, who)
    R.count(max_rounds, 1, "max_rounds", who)
    return H, W, c


def order_rounds(d, cls, top, order, max_rounds=ORDER_MAX_ROUNDS, check_every=CHECK_EVERY):
    """The Strahler iteration on device tensors (order as ops.stream_class leaves it, in place) -> (rounds enqueued, converged).
    One host sync per check_every rounds; the junction list is torch.nonzero on the class plane."""
    from tg_hip import ops as O
    junctions = torch.nonzero(cls.reshape(-1) == O.STREAM_JUNCTION).reshape(-1).to(torch.int32)
    if junctions.numel() == 0:
        return 0, True
    changed = torch.zeros(1, dtype=torch.int32, device=d.device)
    return run_until_unchanged(lambda n: O.stream_order(d, cls, top, junctions, n, order, changed), changed, max_rounds,
                               check_every)


def network_known(d, acc, min_cells, cellsize, max_rounds=ORDER_MAX_ROUNDS, check_every=CHECK_EVERY):
    """stream_network's body on device tensors (d uint8 [H][W] without the code 254, acc int32 [H][W]) -> (order, link, info)."""
    from tg_hip import ops as O
    H, W = d.shape
    ws = O.flow_basin_ws(H, W, d.device)
    cls, node, c0 = O.stream_class(d, acc, min_cells, ws)
    link_rounds = basin_rounds(H, W, ws, check_every, "stream_network")
    top, _, _, _, c1 = O.flow_basin_finish(H, W, link_rounds, ws, cellsize)
    rounds, converged = order_rounds(d, cls, top, node, max_rounds, check_every)
    order, c2 = O.stream_order_finish(cls, top, node)
    cells, heads, junctions, outlets = c0.cpu().tolist()
    oc = c2.cpu().tolist()
    nb = O.STREAM_ORDER_BINS
    info = {"stream_cells": cells, "heads": heads, "junctions": junctions, "outlets": outlets, "links": heads + junctions,
            "max_order": oc[0], "cells_by_order": oc[1:1 + nb], "links_by_order": oc[1 + nb:1 + 2 * nb],
            "link_rounds": link_rounds, "order_rounds": rounds, "converged": converged,
            "longest_link_m": R.bits_f32(c1.cpu().tolist()[2])}
    return order, top, info


@torch.no_grad()
def stream_network(direction, accumulation, min_cells, *, cellsize=1.0, max_rounds=ORDER_MAX_ROUNDS, check_every=CHECK_EVERY):
    """direction: uint8 [H][W] of flow_routing's codes; accumulation: int32 [H][W] (both numpy or HIP tensors); a stream pixel
    has direction != 0 and accumulation >= min_cells.  Returns (order uint8 HIP tensor [H][W]: the Strahler order, 0 off the
    streams; link int32 HIP tensor [H][W]: the linear index y * W + x of the head or junction at the upstream end of the pixel's
    link, -1 off the streams; info: stream_cells, heads, junctions, outlets (stream pixels whose receiver is no stream pixel),
    links, max_order, cells_by_order and links_by_order (orders 1..15, higher ones in the last), link_rounds, order_rounds (may
    differ between runs; the rasters do not), converged, longest_link_m).  If max_rounds stops the order iteration, converged
    is False and every order is a lower bound.  Exact and bitwise reproducible (csrc/drainage.hip)."""
    who = "stream_network"
    H, W, c = check_stream_args(direction, accumulation, min_cells, cellsize, max_rounds, check_every, who)
    device = R.device(who)
    d = R.to_u8(direction, device, "direction", who)
    if bool(torch.any(d == 254)):
        raise ValueError(f"{who}: the direction grid holds the code 254 (undecided): route it to the end first")
    acc = R.to_i32(accumulation, device, "accumulation", who)
    return network_known(d, acc, min_cells, c, max_rounds, check_every)


# ---- height above the nearest drainage -------------------------------------------------------------------------------
def hand_from_routing(w, direction, stream, cellsize, check_every=CHECK_EVERY):
    """HAND on device tensors: w float32 [H][W] the routed surface, direction uint8 [H][W], stream uint8 [H][W] the drainage
    mask.  Every path is followed to its first drainage pixel (watersheds with the mask as pour points) -> (hand float32 [H][W] =
    w(p) - w(T(p)) where T(p) is a drainage pixel, NaN elsewhere; distance_m float32 [H][W]: the flow length to T(p), NaN where
    not drained; info: drained, undrained, stream_cells, max_hand_m, rounds)."""
    from tg_hip import ops as O
    H, W = direction.shape
    ws = O.flow_basin_ws(H, W, direction.device)
    rounds, _, _ = basin_doubling(direction, stream, ws, check_every)
    basin, _, _, length, _ = O.flow_basin_finish(H, W, rounds, ws, cellsize)
    h, dist, counts = O.hand(w, basin, stream, length)
    drained, undrained, cells, bits = counts.cpu().tolist()
    return h, dist, {"drained": drained, "undrained": undrained, "stream_cells": cells, "max_hand_m": R.bits_f32(bits),
                     "rounds": rounds}


@torch.no_grad()
def hand(dem, mask=None, *, nodata=None, cellsize=1.0, min_cells=1000, min_order=1, fill=True, max_sweeps=MAX_SWEEPS,
         check_every=CHECK_EVERY):
    """Height above the nearest drainage of a DEM (inputs as flow_routing).  The raster is routed; the drainage is the stream
    pixels (accumulation >= min_cells) of Strahler order >= min_order (stream_network runs only for min_order > 1); every pixel
    is followed down to its first drainage pixel T.  Returns (hand float32 HIP tensor [H][W] = w(p) - w(T(p)) on the routed
    surface w (the filled one with fill=True), one float32 subtract, >= 0, 0 on the drainage, NaN where the path ends off the
    drainage or the pixel is unknown; distance_m float32 HIP tensor [H][W]: the flow length to T(p), NaN likewise; info:
    flow_routing's numbers plus drained, undrained, stream_cells, max_hand_m, rounds, and "network" with min_order > 1; orders
    that have not converged raise a RuntimeError, since lower bounds would leave links out of the drainage).  The
    flood extent at stage h is hand <= h."""
    who = "hand"
    _min_cells(min_cells, who)
    _min_order(min_order, who)
    direction, acc, info, w = route_raster(dem, mask, nodata, cellsize, fill, max_sweeps, check_every, who)
    return hand_routed(w, direction, acc, info, R.cellsize(cellsize, who), min_cells, min_order, check_every)[:3]


def _min_order(k, who):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 255:
        raise ValueError(f"{who}: min_order {k!r} must be an integer in [1, 255]")
    return k


def hand_routed(w, direction, acc, info, c, min_cells, min_order=1, check_every=CHECK_EVERY, max_rounds=ORDER_MAX_ROUNDS):
    """hand's second half on a routing -> (hand, distance_m, info updated, the drainage mask).  Orders that max_rounds stopped
    short are lower bounds and would leave links out of the drainage, so that is an error here and not a flag."""
    if min_order > 1:
        order, _, ninfo = network_known(direction, acc, min_cells, c, max_rounds, check_every)
        if not ninfo["converged"]:
            raise RuntimeError(f"hand: the Strahler orders have not converged after {ninfo['order_rounds']} rounds, so the "
                               f"drainage of order >= {min_order} is not known")
        stream = (order >= min_order).to(torch.uint8)
        info["network"] = ninfo
    else:
        stream = ((acc >= min_cells) & (direction != 0)).to(torch.uint8)
    h, dist, hinfo = hand_from_routing(w, direction, stream, c, check_every)
    info.update(hinfo)
    return h, dist, info, stream


# ---- multiple flow directions, slope, wetness --------------------------------------------------------------------------
MIN_SLOPE = 1e-3


def check_exponent(exponent, who="mfd_accumulation"):
    """An integer (Python's or numpy's, not a bool) in 1..8 -> int."""
    if isinstance(exponent, (bool, np.bool_)) or not isinstance(exponent, numbers.Integral) or not 1 <= exponent <= 8:
        raise ValueError(f"{who}: exponent {exponent!r} must be an integer in [1, 8]")
    return int(exponent)


def check_min_slope(min_slope, who="wetness_index"):
    """A finite real number (Python's or numpy's, not a bool) > 0, also as float32 -> float."""
    ok = not isinstance(min_slope, (bool, np.bool_)) and isinstance(min_slope, numbers.Real)
    if ok:
        with np.errstate(over="ignore"):
            f = float(np.float32(min_slope))
        ok = 0 < f < math.inf
    if not ok:
        raise ValueError(f"{who}: min_slope {min_slope!r} must be a finite number > 0 (in float32 as well)")
    return float(min_slope)


def mfd_sweeps(w, exponent, A, counts, ws, check_every=CHECK_EVERY):
    """The sweeps of the MFD accumulation on device tensors (A, counts and ws as ops.mfd_setup leaves them) to the end ->
    (sweeps enqueued, tile_visits).  One host sync per check_every sweeps.  Every block of sweeps makes at least one pixel final
    (a pixel that is lowest in (w, D) among those not final has only final donors), so there is no limit to set."""
    from tg_hip import ops as O
    left, visits = counts.cpu().tolist()[3:5]
    sweeps = 0
    while left:
        O.mfd_sweep(w, exponent, check_every, A, counts, ws)
        sweeps += check_every
        now, visits = counts.cpu().tolist()[3:5]
        if now == left:
            raise RuntimeError("mfd_accumulation: the flow graph has a cycle")     # cannot happen: every edge goes down in (w, D)
        left = now
    return sweeps, visits


def mfd_known(w, known, direction, *, exponent=1, check_every=CHECK_EVERY, ws=None):
    """mfd_accumulation's second half on a routing (w float32, known uint8, direction uint8, all [H][W] on the device) ->
    (accumulation float32 [H][W], A float64 [H][W], info: dispersive, single, sinks, mfd_sweeps, mfd_tile_visits,
    max_accumulation_mfd, mass_out, exponent)."""
    from tg_hip import ops as O
    exponent = check_exponent(exponent)
    H, W = w.shape
    if ws is None:
        ws = O.mfd_ws(H, W, w.device)
    A, counts = O.mfd_setup(w, known, direction, exponent, ws)
    dispersive, single, sinks = counts.cpu().tolist()[:3]
    sweeps, visits = mfd_sweeps(w, exponent, A, counts, ws, check_every)
    acc, out = O.mfd_finish(A, direction, ws)
    amax, mass = out.cpu().tolist()
    info = {"dispersive": dispersive, "single": single, "sinks": sinks, "mfd_sweeps": sweeps, "mfd_tile_visits": visits,
            "max_accumulation_mfd": amax, "mass_out": mass, "exponent": exponent}
    return acc, A, info


@torch.no_grad()
def mfd_accumulation(dem, mask=None, *, nodata=None, cellsize=1.0, fill=True, exponent=1, max_sweeps=MAX_SWEEPS,
                     check_every=CHECK_EVERY):
    """Contributing area by a multiple-flow-direction rule (csrc/mfd.hip; inputs as flow_routing).  The
    raster is routed as flow_routing routes it; on the routed surface w a known pixel q gives each lower known neighbour n_j the
    fraction t_j / S of what it holds, t_j = (w(q) - w(n_j)) ** exponent times 2 ** (-(exponent + 1) / 2) for a diagonal n_j
    (Quinn et al. 1991 at exponent 1, Holmgren 1994 above), S their sum; a pixel without a lower neighbour (a flat pixel) gives
    all to its D8 receiver; OUT and PIT pixels give nothing.  A(p) = 1 + the sum of fraction * A(q) over the donors q, in
    float64 in a fixed order.  exponent: an integer in 1..8; 1 spreads widest, large ones approach D8.  max_sweeps limits the
    fill and the flats as in flow_routing; the MFD sweeps run to the end.  Returns (accumulation float32 HIP tensor [H][W] in
    cells, 0 at unknown pixels; info: flow_routing's plus dispersive, single, sinks (pixels by what they give), mfd_sweeps,
    mfd_tile_visits (both may differ between runs; the raster does not), max_accumulation_mfd, mass_out (the sum of A over the
    sinks: the number of known pixels up to rounding) and exponent).  Bitwise equal to tests/mfd_oracle.py and bitwise
    reproducible."""
    who = "mfd_accumulation"
    exponent = check_exponent(exponent, who)
    z, known, c = _upload(dem, mask, nodata, cellsize, fill, max_sweeps, check_every, who)
    direction, _, info, w = route_known(z, known, c, fill=fill, max_sweeps=max_sweeps, check_every=check_every,
                                        return_surface=True)
    acc, _, minfo = mfd_known(w, known, direction, exponent=exponent, check_every=check_every)
    info.update(minfo)
    return acc, info


@torch.no_grad()
def terrain_slope(dem, mask=None, *, nodata=None, cellsize=1.0):
    """Horn's slope tan(beta) of a DEM as given (no fill): float32 HIP tensor [H][W], NaN at unknown pixels; a neighbour off
    the raster or unknown counts as the centre height.  In float32, in the operation order of tests/mfd_oracle.py."""
    from tg_hip import ops as O
    z, known, c = _upload(dem, mask, nodata, cellsize, True, 1, 1, "terrain_slope")
    return O.terrain_slope(z, known, c)


def wetness_known(z, known, cellsize, *, fill=True, exponent=1, min_slope=MIN_SLOPE, max_sweeps=MAX_SWEEPS,
                  check_every=CHECK_EVERY):
    """wetness_index's body on device tensors with a ready known mask (as route_known) -> (twi, accumulation, slope, info)."""
    from tg_hip import ops as O
    exponent = check_exponent(exponent, "wetness_index")
    min_slope = check_min_slope(min_slope)
    direction, _, info, w = route_known(z, known, cellsize, fill=fill, max_sweeps=max_sweeps, check_every=check_every,
                                        return_surface=True)
    acc, _, minfo = mfd_known(w, known, direction, exponent=exponent, check_every=check_every)
    info.update(minfo)
    slope = O.terrain_slope(w, known, cellsize)
    twi = O.wetness(acc, slope, known, cellsize, min_slope)
    info["min_slope"] = min_slope
    return twi, acc, slope, info


@torch.no_grad()
def wetness_index(dem, mask=None, *, nodata=None, cellsize=1.0, fill=True, exponent=1, min_slope=MIN_SLOPE,
                  max_sweeps=MAX_SWEEPS, check_every=CHECK_EVERY):
    """The topographic wetness index ln(a / tan(beta)) of a DEM (inputs as flow_routing): a = float32(A) * float32(cellsize),
    the specific catchment area in metres from mfd_accumulation; tan(beta) Horn's slope of the routed surface (the filled one
    with fill=True), not below min_slope (> 0); twi = logf(a / fmaxf(slope, min_slope)) in float32.  Returns (twi, accumulation,
    slope: float32 HIP tensors [H][W], twi and slope NaN at unknown pixels; info: mfd_accumulation's plus min_slope)."""
    who = "wetness_index"
    check_exponent(exponent, who)
    check_min_slope(min_slope, who)
    z, known, c = _upload(dem, mask, nodata, cellsize, fill, max_sweeps, check_every, who)
    return wetness_known(z, known, c, fill=fill, exponent=exponent, min_slope=min_slope, max_sweeps=max_sweeps,
                         check_every=check_every)


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
    ap.add_argument("--min-cells", type=int, help="stream threshold in cells (required with --streams-out, --order-out, "
                                                  "--links-out and --hand-out)")
    ap.add_argument("--order-out", help="also write the Strahler order of the streams (.asc): 0 off the streams")
    ap.add_argument("--links-out", help="also write the stream links (.asc): the linear index y * ncols + x of the head or "
                                        "junction at the upstream end of a stream cell's link, -1 off the streams")
    ap.add_argument("--hand-out", help="also write the height above the nearest drainage in metres (.asc, full float32 precision; "
                                       "NODATA_value where a cell's path ends off the drainage)")
    ap.add_argument("--hand-distance-out", help="with --hand-out: also write the flow length to that drainage cell in metres (.asc)")
    ap.add_argument("--min-order", type=int, default=1, help="with --hand-out: the drainage is the streams of at least this "
                                                             "Strahler order (default 1: every stream)")
    ap.add_argument("--basins-out", help="also write the watershed labels (.asc): the linear index y * ncols + x of the pixel each "
                                         "cell drains to, -1 = void")
    ap.add_argument("--pour", help="pour points for --basins-out (.png or .asc of the raster's size): nonzero = a cell where "
                                   "paths end, so that its upstream area is a basin of its own")
    ap.add_argument("--compact", action="store_true", help="with --basins-out: number the basins 1..n in raster order of their "
                                                           "outlets, 0 = void")
    ap.add_argument("--length-out", help="also write the flow length to the outlet in metres (.asc, full float32 precision)")
    ap.add_argument("--mfd-acc-out", help="also write the multiple-flow-direction contributing area in cells (.asc, full float32 "
                                          "precision): every cell spreads over all its lower neighbours (--exponent)")
    ap.add_argument("--exponent", type=int, default=1, help="with --mfd-acc-out or --twi-out: a lower neighbour gets a share "
                                                            "proportional to its drop to this power, an integer in 1..8 "
                                                            "(default 1: widest spreading; large values approach D8)")
    ap.add_argument("--slope-out", help="also write Horn's slope tan(beta) of the routed surface (.asc)")
    ap.add_argument("--twi-out", help="also write the topographic wetness index ln(a / tan(beta)) (.asc), a the specific catchment "
                                      "area in metres from the multiple-flow-direction accumulation")
    ap.add_argument("--min-slope", type=float, default=MIN_SLOPE, help="with --twi-out: slopes below this count as this (> 0)")
    ap.add_argument("--dir-out", required=True, help="output .asc raster of direction codes")
    ap.add_argument("--acc-out", required=True, help="output .asc raster of the flow accumulation in cells")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    wants = [f for f, v in (("--streams-out", a.streams_out), ("--order-out", a.order_out), ("--links-out", a.links_out),
                            ("--hand-out", a.hand_out)) if v is not None]
    if bool(wants) != (a.min_cells is not None):
        ap.error("--min-cells goes together with --streams-out, --order-out, --links-out or --hand-out")
    if a.min_cells is not None and a.min_cells < 1:
        ap.error("--min-cells must be >= 1")
    if a.hand_distance_out and not a.hand_out:
        ap.error("--hand-distance-out needs --hand-out")
    if a.min_order != 1 and not a.hand_out:
        ap.error("--min-order needs --hand-out")
    if not 1 <= a.min_order <= 255:
        ap.error("--min-order must lie in [1, 255]")
    if a.compact and not a.basins_out:
        ap.error("--compact needs --basins-out")
    if a.pour and not (a.basins_out or a.length_out):
        ap.error("--pour needs --basins-out or --length-out")
    if not 1 <= a.exponent <= 8:
        ap.error("--exponent must lie in [1, 8]")
    if a.exponent != 1 and not (a.mfd_acc_out or a.twi_out):
        ap.error("--exponent needs --mfd-acc-out or --twi-out")
    if not (a.min_slope > 0 and a.min_slope < math.inf):
        ap.error("--min-slope must be finite and > 0")
    if a.min_slope != MIN_SLOPE and not a.twi_out:
        ap.error("--min-slope needs --twi-out")
    return a


def main(argv=None):
    from .asc import read_inputs, read_mask, with_nodata, write_asc, write_int_asc
    a = parse_args(argv)
    dem, header, mask, nodata, cs = read_inputs(a)
    direction, acc, info, w = route_raster(dem, mask, nodata, cs, not a.no_fill, a.max_sweeps, CHECK_EVERY, "flow_routing")
    write_int_asc(a.dir_out, (to_esri(direction) if a.esri else direction).cpu().numpy(), header)
    write_int_asc(a.acc_out, acc.cpu().numpy(), header)
    if a.streams_out:
        write_int_asc(a.streams_out, streams(acc, a.min_cells).cpu().numpy(), header)
    if a.order_out or a.links_out:
        order, link, ninfo = network_known(direction, acc, a.min_cells, cs)
        if a.order_out:
            write_int_asc(a.order_out, order.cpu().numpy(), header)
        if a.links_out:
            write_int_asc(a.links_out, link.cpu().numpy(), header)
        info["network"] = ninfo
        print(f"{a.order_out or a.links_out}: {ninfo['stream_cells']} stream cells in {ninfo['links']} links ({ninfo['heads']} "
              f"heads, {ninfo['junctions']} junctions, {ninfo['outlets']} outlets), largest Strahler order {ninfo['max_order']}, "
              f"longest link {ninfo['longest_link_m']:.9g} m, {ninfo['link_rounds']} link rounds, {ninfo['order_rounds']} order "
              f"rounds" + ("" if ninfo["converged"] else " (NOT converged: the orders are lower bounds)"))
    if a.hand_out:
        h, dist, _, _ = hand_routed(w, direction, acc, info, cs, a.min_cells, a.min_order)
        fh = with_nodata(header)
        write_asc(a.hand_out, h.cpu().numpy(), fh)
        if a.hand_distance_out:
            write_asc(a.hand_distance_out, dist.cpu().numpy(), fh)
        print(f"{a.hand_out}: {info['drained']} cells drain to {info['stream_cells']} drainage cells (order >= {a.min_order}), "
              f"{info['undrained']} do not; largest height above drainage {info['max_hand_m']:.9g} m, {info['rounds']} rounds")
    if a.mfd_acc_out or a.slope_out or a.twi_out:
        from tg_hip import ops as O
        known = (direction != 0).to(torch.uint8)                    # every known pixel has a code
        fh = with_nodata(header)
        if a.slope_out or a.twi_out:
            slope = O.terrain_slope(w, known, cs)
            if a.slope_out:
                write_asc(a.slope_out, slope.cpu().numpy(), fh)
        if a.mfd_acc_out or a.twi_out:
            macc, _, minfo = mfd_known(w, known, direction, exponent=a.exponent)
            info.update(minfo)
            if a.mfd_acc_out:
                write_asc(a.mfd_acc_out, macc.cpu().numpy(), [(k, v) for k, v in header if k.lower() != "nodata_value"])
            if a.twi_out:
                write_asc(a.twi_out, O.wetness(macc, slope, known, cs, check_min_slope(a.min_slope, "--min-slope")).cpu().numpy(), fh)
            print(f"{a.mfd_acc_out or a.twi_out}: exponent {minfo['exponent']}, {minfo['dispersive']} cells spread, "
                  f"{minfo['single']} give to one neighbour, {minfo['sinks']} sinks; largest contributing area "
                  f"{minfo['max_accumulation_mfd']:.9g} cells, {minfo['mass_out']:.9g} cells leave, {minfo['mfd_sweeps']} sweeps")
    if a.basins_out or a.length_out:
        pour = read_mask(a.pour, dem.shape) if a.pour else None
        basin, length, winfo = watersheds(direction, pour, cellsize=cs, compact=a.compact)
        if a.basins_out:
            write_int_asc(a.basins_out, basin.cpu().numpy(), header)
        if a.length_out:
            write_asc(a.length_out, length.cpu().numpy(), [(k, v) for k, v in header if k.lower() != "nodata_value"])
        info["watersheds"] = winfo
        print(f"{a.basins_out or a.length_out}: {winfo['basins']} basins, longest path {winfo['longest_steps']} steps = "
              f"{winfo['max_length_m']:.9g} m, {winfo['rounds']} rounds, {winfo['pour_points']} pour points"
              + (f" ({winfo['pour_ignored']} on voids ignored)" if winfo["pour_ignored"] else ""))
    how = "" if info["converged"] else f" (NOT converged after {info['flat_sweeps']} flat sweeps: unresolved flat cells are pits)"
    print(f"{a.dir_out}: {info['known']} cells, {info['outlets']} outlets, {info['flat_cells']} flat cells, {info['pits']} pits, "
          f"largest contributing area {info['max_accumulation']} cells = {info['max_area_m2']:.6g} m2, "
          f"{info['flat_sweeps']} flat sweeps, {info['acc_rounds']} accumulation rounds{how}")
    return info


if __name__ == "__main__":
    main()
