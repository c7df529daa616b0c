"""CPU oracle of the watersheds, the flow length and the drainage comparison (csrc/drainage.hip, mvp_gan/src/flow_routing.py
watersheds, mvp_gan/src/evaluate_raster.py drainage_errors), numpy only (scipy for the distances).

For a direction grid of tests/flow_oracle.py (without UNDECIDED) and optional pour points: T(p), the last pixel of p's path, and
nc(p), nd(p), the cardinal and diagonal steps to it, in two independent forms: a walk along a topological order, and the doubling
recurrence of the GPU.  Unknown pixels have T = -1 and no steps.  A pour point on a known pixel is a terminal whatever its code."""
import math
from collections import deque

import numpy as np

from tests import depfill_oracle as DO
from tests import flow_oracle as FO

SQRT2 = 1.4142135623730951
EDT_FAR = 0x7fffffff
NAMES = ("cells", "dir_equal", "dir_routed", "dir_within_45", "same_outlet", "outlet_d2_sum", "outlet_d2_max",
         "area_octave_sum", "streams_truth", "streams_pred", "streams_both", "pred_matched", "pred_far", "pred_d2_sum",
         "pred_d2_max", "truth_matched", "truth_far", "truth_d2_sum", "truth_d2_max")


def next0(code, pour=None):
    """-> (next int64 [H * W], pour points used, pour points ignored)."""
    nxt = FO.receivers(code)
    used = ignored = 0
    if pour is not None:
        pp = np.asarray(pour).ravel() != 0
        kn = code.ravel() != 0
        nxt[pp & kn] = -1
        used, ignored = int((pp & kn).sum()), int((pp & ~kn).sum())
    return nxt, used, ignored


def first_steps(code, nxt):
    """(c0, d0) per pixel: (1, 0) for a cardinal code with a pointer, (0, 1) for a diagonal one, else (0, 0)."""
    c = code.ravel().astype(np.int64)
    live = nxt >= 0
    card = live & (c % 2 == 1)                                     # 1, 3, 5, 7 = E, S, W, N
    return card.astype(np.int64), (live & ~card).astype(np.int64)


def paths_walk(code, pour=None):
    """T, nc, nd by walking: the pixels are taken downstream-first (the reverse of Kahn's order), so a pixel's receiver is done
    before it.  -> (T int64 [H][W], nc, nd int64 [H][W], the longest path in steps)."""
    nxt, _, _ = next0(code, pour)
    n = nxt.size
    kn = code.ravel() != 0
    c0, d0 = first_steps(code, nxt)
    indeg = np.bincount(nxt[nxt >= 0], minlength=n)
    q = deque(np.nonzero((indeg == 0) & kn)[0].tolist())
    order = []
    while q:
        p = q.popleft()
        order.append(p)
        r = nxt[p]
        if r >= 0:
            indeg[r] -= 1
            if indeg[r] == 0:
                q.append(int(r))
    assert len(order) == int(kn.sum()), "the direction grid has a cycle"
    T = np.full(n, -1, np.int64)
    nc = np.zeros(n, np.int64)
    nd = np.zeros(n, np.int64)
    for p in reversed(order):
        r = nxt[p]
        if r < 0:
            T[p] = p
        else:
            T[p], nc[p], nd[p] = T[r], nc[r] + c0[p], nd[r] + d0[p]
    s = code.shape
    return T.reshape(s), nc.reshape(s), nd.reshape(s), int((nc + nd).max()) if n else 0


def paths_doubling(code, pour=None, max_rounds=None):
    """The recurrence of the GPU: state (next, last, nc, nd), every right-hand side from the state before the round.
    -> (last, nc, nd int64 [H][W], rounds run); with max_rounds the state after that many rounds (or the end, if sooner)."""
    nxt, _, _ = next0(code, pour)
    n = nxt.size
    last = np.where(code.ravel() != 0, np.arange(n, dtype=np.int64), -1)
    nc, nd = first_steps(code, nxt)
    rounds = 0
    while (nxt >= 0).any() and (max_rounds is None or rounds < max_rounds):
        live = nxt >= 0
        q = nxt[live]
        last2, nc2, nd2, n2 = last.copy(), nc.copy(), nd.copy(), nxt.copy()
        last2[live] = last[q]
        nc2[live] = nc[live] + nc[q]
        nd2[live] = nd[live] + nd[q]
        n2[live] = nxt[q]
        last, nc, nd, nxt, rounds = last2, nc2, nd2, n2, rounds + 1
        assert rounds <= 32
    s = code.shape
    return last.reshape(s), nc.reshape(s), nd.reshape(s), rounds


def length_m(nc, nd, cellsize):
    """float32(cellsize * (nc + SQRT2 * nd)) in float64: one multiply, one add, one multiply, one rounding."""
    diag = np.float64(SQRT2) * nd.astype(np.float64)
    return (np.float64(cellsize) * (nc.astype(np.float64) + diag)).astype(np.float32)


def compact(T):
    """The rank 1..n of every pixel's terminal in raster order, 0 where unknown (np.unique sorts the indices)."""
    out = np.zeros(T.shape, np.int32)
    kn = T >= 0
    _, inv = np.unique(T[kn], return_inverse=True)
    out[kn] = inv.ravel() + 1
    return out


def watersheds(code, pour=None, cellsize=1.0):
    """-> dict(T, nc, nd, length, rounds, basins, longest, max_length, used, ignored)."""
    T, nc, nd, longest = paths_walk(code, pour)
    _, used, ignored = next0(code, pour)
    rounds = 0
    while (1 << rounds) <= longest:
        rounds += 1
    ln = length_m(nc, nd, cellsize)
    idx = np.arange(T.size, dtype=np.int64).reshape(T.shape)
    return {"T": T, "nc": nc, "nd": nd, "length": ln, "rounds": rounds, "basins": int((T == idx).sum()), "longest": longest,
            "max_length": float(ln.max()) if ln.size else 0.0, "used": used, "ignored": ignored}


def stream_d2(stream):
    """Exact squared pixel distance to the nearest stream pixel (int64), EDT_FAR without one."""
    from scipy.ndimage import distance_transform_edt
    stream = np.asarray(stream) != 0
    if not stream.any():
        return np.full(stream.shape, EDT_FAR, np.int64)
    d = distance_transform_edt(~stream)
    return np.rint(d * d).astype(np.int64)


def compare(sel, dir_t, dir_p, basin_t, basin_p, acc_t, acc_p, d2_t, d2_p, stream_cells, tol2):
    """The counters of tg_flow_compare with plain numpy -> dict by NAMES (Python ints)."""
    W = dir_t.shape[1]
    s = (np.asarray(sel) != 0) & (dir_t != 0) & (dir_p != 0)
    ct, cp = dir_t[s].astype(np.int64), dir_p[s].astype(np.int64)
    bt, bp = basin_t[s].astype(np.int64), basin_p[s].astype(np.int64)
    at, ap = acc_t[s].astype(np.int64), acc_p[s].astype(np.int64)
    dt, dp = d2_t[s].astype(np.int64), d2_p[s].astype(np.int64)
    routed = (ct <= 8) & (cp <= 8)
    diff = np.abs(ct - cp)
    diff = np.minimum(diff, 8 - diff)
    ok = (bt >= 0) & (bp >= 0)
    od2 = np.where(ok, (bt // W - bp // W) ** 2 + (bt % W - bp % W) ** 2, 0)
    octave = lambda a: np.array([int(v).bit_length() - 1 for v in np.maximum(a, 1)], np.int64)
    st, sp = at >= stream_cells, ap >= stream_cells
    out = {"cells": int(s.sum()), "dir_equal": int((ct == cp).sum()), "dir_routed": int(routed.sum()),
           "dir_within_45": int((routed & (diff <= 1)).sum()), "same_outlet": int((bt == bp).sum()),
           "outlet_d2_sum": int(od2.sum()), "outlet_d2_max": int(od2.max()) if od2.size else 0,
           "area_octave_sum": int(np.abs(octave(at) - octave(ap)).sum()),
           "streams_truth": int(st.sum()), "streams_pred": int(sp.sum()), "streams_both": int((st & sp).sum())}
    for side, on, d in (("pred", sp, dt), ("truth", st, dp)):
        v = d[on]
        near = v[v != EDT_FAR]
        out[side + "_matched"] = int((v <= tol2).sum())
        out[side + "_far"] = int((v == EDT_FAR).sum())
        out[side + "_d2_sum"] = int(near.sum())
        out[side + "_d2_max"] = int(near.max()) if near.size else 0
    return out


def drainage(z, pred, holes, cellsize, stream_cells, tol2, tol_m):
    """drainage_errors with the oracles -> (counters dict, report dict, the two routings)."""
    z, pred = np.asarray(z, np.float32), np.asarray(pred, np.float32)
    known = DO.known_map(z) & DO.known_map(pred)
    sides = []
    for s in (z, pred):
        r = FO.route(np.where(known, s, np.float32(np.nan)), fill=True)
        w = watersheds(r["dir"], None, cellsize)
        r.update(T=w["T"], basin_rounds=w["rounds"], d2=stream_d2(r["acc"] >= stream_cells))
        sides.append(r)
    t, p = sides
    c = compare(holes, t["dir"], p["dir"], t["T"], p["T"], t["acc"], p["acc"], t["d2"], p["d2"], stream_cells, tol2)
    cs = float(cellsize)
    ratio = lambda a, b: a / b if b else None
    rms = lambda s2, n: cs * math.sqrt(s2 / n) if n else None
    dist = lambda d2, n: cs * math.sqrt(d2) if n else None
    side = lambda r: {"pits": r["pits"], "flat_cells": r["flat_cells"], "converged": True, "rounds": r["basin_rounds"]}
    n = c["cells"]
    np_, nt = c["streams_pred"] - c["pred_far"], c["streams_truth"] - c["truth_far"]
    rep = {"cells": n, "stream_cells": stream_cells, "stream_tol_m": float(tol_m),
           "direction": {"equal": ratio(c["dir_equal"], n), "within_45": ratio(c["dir_within_45"], c["dir_routed"]),
                         "routed": c["dir_routed"]},
           "outlet": {"same": ratio(c["same_outlet"], n), "shift_rms_m": rms(c["outlet_d2_sum"], n),
                      "shift_max_m": dist(c["outlet_d2_max"], n)},
           "area": {"octave_mae": ratio(c["area_octave_sum"], n)},
           "streams": {"truth_cells": c["streams_truth"], "pred_cells": c["streams_pred"], "both_cells": c["streams_both"],
                       "precision": ratio(c["pred_matched"], c["streams_pred"]),
                       "recall": ratio(c["truth_matched"], c["streams_truth"]),
                       "pred_to_truth_rms_m": rms(c["pred_d2_sum"], np_), "pred_to_truth_max_m": dist(c["pred_d2_max"], np_),
                       "truth_to_pred_rms_m": rms(c["truth_d2_sum"], nt), "truth_to_pred_max_m": dist(c["truth_d2_max"], nt),
                       "pred_far": c["pred_far"], "truth_far": c["truth_far"]},
           "truth": side(t), "pred": side(p)}
    return c, rep, sides


# ---- the scene of the drainage tests --------------------------------------------------------------------------------------
HOLES = ((30, 80, 40, 100), (110, 170, 20, 70), (90, 150, 110, 180))
STREAM_CELLS, TOL_PX, CELLSIZE = 100, 3, 2.0


def scene():
    """The 192x192 terrain of tests/test_hip_terrain_eval.py at 2 m, three rectangular holes, and a fill that joins the two rim
    pixels of every hole row by a straight line.  -> (z, pred, holes uint8)"""
    from tests.test_hip_terrain_eval import _terrain
    z = np.asarray(_terrain(192, 192, CELLSIZE, 21), np.float32)
    pred = z.copy()
    holes = np.zeros(z.shape, np.uint8)
    for y0, y1, x0, x1 in HOLES:
        holes[y0:y1, x0:x1] = 1
        for y in range(y0, y1):
            a, b = np.float64(z[y, x0 - 1]), np.float64(z[y, x1])
            t = (np.arange(x0, x1) - (x0 - 1)) / np.float64(x1 - (x0 - 1))
            pred[y, x0:x1] = (a + (b - a) * t).astype(np.float32)
    return z, pred, holes
