"""CPU checks of the watersheds and the drainage comparison (csrc/drainage.hip, mvp_gan/src/flow_routing.py watersheds,
mvp_gan/src/evaluate_raster.py drainage_errors): the two forms of T, nc and nd in tests/drainage_oracle.py
against each other and against the defining properties, pour points, the conditions the GPU scene must meet, the report assembly
and the tolerance, host-side rejection by the five C entry points, the ops and the Python API, the workspace query and the CLI
parsers, all without a GPU.  Every comparison is exact."""
import ctypes as C
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import drainage_oracle as DR
from tests import flow_oracle as FO
from tests.test_flow_cpu import _rasters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tg_flow_basin_ws_bytes", "tg_flow_basin_init", "tg_flow_basin", "tg_flow_basin_finish", "tg_flow_compare")


@pytest.fixture(scope="module", autouse=True)
def contract():
    """The oracle implements what include/terragan_hip.h states."""
    txt = " ".join(open(os.path.join(ROOT, "include", "terragan_hip.h")).read().replace("* ", "").split())
    for name in NAMES:
        assert name + "(" in txt, name
    assert "(float)(cellsize ((double)nc + 1.4142135623730951 (double)nd))" in txt.replace("* ", "")
    assert "#define TG_FLOW_BASIN_COUNTS 3 " in txt and f"#define TG_FLOW_COMPARE_COUNTS {len(DR.NAMES)} " in txt
    return txt


def _pour(code, rng, share=0.03):
    return (rng.random(code.shape) < share).astype(np.uint8)


def test_two_forms_of_the_paths_agree():
    rng = np.random.default_rng(5)
    n = multi = 0
    for z in _rasters():
        for fill in (False, True):
            r = FO.route(z, fill=fill)
            code, acc = r["dir"], r["acc"]
            idx = np.arange(code.size).reshape(code.shape)
            for pour in (None, _pour(code, rng)):
                T, nc, nd, longest = DR.paths_walk(code, pour)
                T2, nc2, nd2, rounds = DR.paths_doubling(code, pour)
                np.testing.assert_array_equal(T, T2)
                np.testing.assert_array_equal(nc, nc2)
                np.testing.assert_array_equal(nd, nd2)
                w = DR.watersheds(code, pour, 0.5)
                assert rounds == w["rounds"] and longest == w["longest"]
                kn = code != 0
                assert (T[~kn] == -1).all() and (nc[~kn] == 0).all() and (nd[~kn] == 0).all() and (T[kn] >= 0).all()
                np.testing.assert_array_equal(T.ravel()[T[kn]], T[kn])                       # T(T(p)) == T(p)
                term = kn & (T == idx)
                assert (nc[term] == 0).all() and (nd[term] == 0).all() and w["basins"] == int(term.sum())
                nxt, used, ignored = DR.next0(code, pour)
                live = nxt.reshape(code.shape) >= 0
                assert ((nc + nd)[live] >= 1).all() and not (term & live).any() and (term | live | ~kn).all()
                np.testing.assert_array_equal(w["length"], (0.5 * (nc + DR.SQRT2 * nd)).astype(np.float32))
                if pour is None:
                    # the pixels of a basin number acc[T]
                    size = np.bincount(T[kn], minlength=code.size).reshape(code.shape)
                    np.testing.assert_array_equal(size[term], acc[term])
                    assert ((code == FO.OUT) | (code == FO.PIT))[term].all() and used == ignored == 0
                else:
                    pk = (pour != 0) & kn
                    assert term[pk].all() and used == int(pk.sum()) and ignored == int(((pour != 0) & ~kn).sum())
                    multi += used
                np.testing.assert_array_equal(DR.compact(T) == 0, ~kn)
                n += 1
    assert n >= 160 and multi > 500


def test_rounds_of_the_recurrence_follow_the_invariant():
    """last_k(p) is the pixel min(2^k - 1, remaining) steps downstream; nc_k + nd_k counts the first min(2^k, remaining) edges."""
    z, order = FO.serpentine()
    code = FO.route(z, fill=False)["dir"]
    T, nc, nd, _ = DR.paths_walk(code)
    rem = (nc + nd).ravel()
    nxt = FO.receivers(code)
    for k in (0, 1, 3, 5):
        last, c, d, rounds = DR.paths_doubling(code, max_rounds=k)
        assert rounds == k
        want = np.arange(code.size)
        for _ in range((1 << k) - 1):
            want = np.where(nxt[want] >= 0, nxt[want], want)
        kn = code.ravel() != 0
        np.testing.assert_array_equal(last.ravel()[kn], want[kn])
        np.testing.assert_array_equal((c + d).ravel(), np.minimum(1 << k, rem))


def test_pour_point_splits_the_serpentine():
    z, order = FO.serpentine()
    code = FO.route(z, fill=False)["dir"]
    w0 = DR.watersheds(code)
    on = order >= 0
    # the water cuts every corner of the channel by two diagonal steps (0.04 m * 0x1.6a09e6p-1 beats 0.02 m), so the path from
    # the head has 8129 steps (8130 from the wall pixel above it) where the channel has 8255 places; along the channel the steps
    # still fall with the place
    steps = (w0["nc"] + w0["nd"])[on][np.argsort(order[on])]
    assert order.max() == 8255 and steps[0] == w0["longest"] - 1 == 8129 and w0["rounds"] == 13 and steps[-1] == 0
    assert (np.diff(steps) <= 0).all() and (np.diff(steps) >= -1).all() and int(w0["nd"][on].max()) == 126
    np.testing.assert_array_equal(steps[-120:], np.arange(119, -1, -1))          # the last row is straight
    mouth = int(np.flatnonzero(order.ravel() == order.max())[0])
    assert (w0["T"][on] == mouth).all()
    pour = (order == 4000).astype(np.uint8)
    pp = int(np.flatnonzero(pour.ravel())[0])
    w = DR.watersheds(code, pour)
    assert (w["T"][on & (order <= 4000)] == pp).all() and (w["T"][on & (order > 4000)] == mouth).all()
    up = on & (order <= 4000)
    np.testing.assert_array_equal((w["nc"] + w["nd"])[up], (w0["nc"] + w0["nd"])[up] - (w0["nc"] + w0["nd"]).ravel()[pp])
    assert (w0["nc"] + w0["nd"]).ravel()[pp] > 4000 and int((w["nc"] + w["nd"])[up].max()) > 3900
    assert w["used"] == 1 and w["ignored"] == 0 and w["basins"] == w0["basins"] + 1
    # a pour point on an unknown pixel is ignored
    code2 = code.copy()
    code2[0, 0] = 0
    pour[0, 0] = 1
    w2 = DR.watersheds(code2, pour)
    assert w2["used"] == 1 and w2["ignored"] == 1 and w2["T"][0, 0] == -1


def test_scene_conditions():
    """No row of the drainage report may be vacuous on the scene of the GPU test."""
    z, pred, holes = DR.scene()
    tol2 = DR.TOL_PX ** 2
    c, rep, sides = DR.drainage(z, pred, holes, DR.CELLSIZE, DR.STREAM_CELLS, tol2, DR.TOL_PX * DR.CELLSIZE)
    print(c, rep)
    assert c["cells"] == int(holes.sum()) == 10200
    assert c["streams_truth"] >= 500 and c["streams_pred"] >= 500
    shares = (rep["direction"]["equal"], rep["direction"]["within_45"], rep["outlet"]["same"], rep["streams"]["precision"],
              rep["streams"]["recall"], c["streams_both"] / c["streams_pred"], c["streams_both"] / c["streams_truth"])
    assert all(0.05 < s < 0.95 for s in shares), shares
    assert c["outlet_d2_max"] > tol2 and c["pred_far"] == 0 and c["truth_far"] == 0
    assert c["pred_d2_max"] > tol2 and c["truth_d2_max"] > tol2 and c["area_octave_sum"] > 0
    assert all(s["pits"] == 0 for s in sides)
    # the distances: scipy's against brute force on a corner of the scene
    st = sides[0]["acc"][:48, :40] >= 20
    ys, xs = np.nonzero(st)
    y, x = np.mgrid[0:48, 0:40]
    brute = ((y[..., None] - ys) ** 2 + (x[..., None] - xs) ** 2).min(-1)
    np.testing.assert_array_equal(DR.stream_d2(st), brute)
    assert (DR.stream_d2(np.zeros((3, 4), bool)) == DR.EDT_FAR).all()


def test_compare_counters_by_hand():
    """One pixel per counter."""
    z = np.zeros((1, 8), np.int32)
    one = lambda **kw: DR.compare(np.ones((1, 8), np.uint8), kw.get("dt", z.astype(np.uint8) + 1), kw.get("dp", z.astype(np.uint8) + 1),
                                  kw.get("bt", z), kw.get("bp", z), kw.get("at", z + 1), kw.get("ap", z + 1), kw.get("d2t", z),
                                  kw.get("d2p", z), 4, 2)
    base = one()
    assert base["cells"] == base["dir_equal"] == base["dir_routed"] == base["dir_within_45"] == base["same_outlet"] == 8
    assert all(base[k] == 0 for k in DR.NAMES[5:])
    dp = np.array([[1, 2, 8, 3, 5, 9, 255, 0]], np.uint8)                  # equal, 45, 45 cyclic, 90, 180, OUT, PIT, unknown
    c = one(dp=dp)
    assert (c["cells"], c["dir_equal"], c["dir_routed"], c["dir_within_45"]) == (7, 1, 5, 3)
    c = one(bp=np.array([[0, 7, 0, 0, 0, 0, 0, 3]], np.int32))
    assert (c["same_outlet"], c["outlet_d2_sum"], c["outlet_d2_max"]) == (6, 58, 49)
    c = one(at=np.array([[1, 2, 3, 4, 7, 8, 1023, 1024]], np.int32))
    assert c["area_octave_sum"] == 0 + 1 + 1 + 2 + 2 + 3 + 9 + 10 and (c["streams_truth"], c["streams_pred"], c["streams_both"]) == (5, 0, 0)
    far = DR.EDT_FAR
    c = one(at=z + 4, d2p=np.array([[0, 1, 2, 3, 4, 100, far, far]], np.int32))
    assert (c["truth_matched"], c["truth_far"], c["truth_d2_sum"], c["truth_d2_max"]) == (3, 2, 110, 100)
    assert (c["pred_matched"], c["pred_far"], c["pred_d2_sum"], c["pred_d2_max"], c["streams_pred"]) == (0, 0, 0, 0, 0)
    c = one(ap=np.array([[4, 4, 4, 1, 1, 1, 1, 1]], np.int32), at=np.array([[4, 1, 1, 1, 1, 1, 1, 1]], np.int32),
            d2t=np.array([[0, 2, 3, 9, 9, 9, 9, 9]], np.int32))
    assert (c["streams_truth"], c["streams_pred"], c["streams_both"], c["pred_matched"], c["pred_d2_sum"], c["pred_d2_max"]) == \
        (1, 3, 1, 2, 5, 3)


# ---- the report -----------------------------------------------------------------------------------------------------------
def test_assemble_drainage_and_tolerance():
    from mvp_gan.src.evaluate_raster import assemble_drainage, drainage_summary, stream_tolerance
    from tg_hip import ops as O
    assert O.FLOW_COMPARE_NAMES == DR.NAMES and O.FLOW_COMPARE_COUNTS == len(DR.NAMES) == 19 and O.FLOW_BASIN_COUNTS == 3
    side = {"pits": 0, "flat_cells": 5, "converged": True, "rounds": 8}
    cnt = dict(zip(DR.NAMES, (200, 50, 180, 90, 40, 800, 25, 300, 20, 10, 5, 8, 1, 36, 16, 15, 0, 80, 49)))
    d = assemble_drainage([cnt[k] for k in DR.NAMES], side, dict(side, pits=2), cellsize=2.0, stream_cells=100, stream_tol_m=6.0)
    assert d == {"cells": 200, "stream_cells": 100, "stream_tol_m": 6.0,
                 "direction": {"equal": 0.25, "within_45": 0.5, "routed": 180},
                 "outlet": {"same": 0.2, "shift_rms_m": 4.0, "shift_max_m": 10.0},
                 "area": {"octave_mae": 1.5},
                 "streams": {"truth_cells": 20, "pred_cells": 10, "both_cells": 5, "precision": 0.8, "recall": 0.75,
                             "pred_to_truth_rms_m": 4.0, "pred_to_truth_max_m": 8.0, "truth_to_pred_rms_m": 4.0,
                             "truth_to_pred_max_m": 14.0, "pred_far": 1, "truth_far": 0},
                 "truth": side, "pred": dict(side, pits=2)}
    assert "precision 0.800" in drainage_summary(d) and "recall 0.750" in drainage_summary(d)
    # zero denominators: None, never a division
    zero = assemble_drainage([0] * 19, side, side, cellsize=2.0, stream_cells=100, stream_tol_m=6.0)
    assert zero["direction"] == {"equal": None, "within_45": None, "routed": 0}
    assert zero["outlet"] == {"same": None, "shift_rms_m": None, "shift_max_m": None} and zero["area"] == {"octave_mae": None}
    assert all(zero["streams"][k] is None for k in ("precision", "recall", "pred_to_truth_rms_m", "pred_to_truth_max_m",
                                                    "truth_to_pred_rms_m", "truth_to_pred_max_m"))
    assert "n/a" in drainage_summary(zero)
    # every pred stream far: no mean, no maximum, precision 0
    cnt2 = dict(cnt, pred_far=10, pred_matched=0, pred_d2_sum=0, pred_d2_max=0)
    d2 = assemble_drainage([cnt2[k] for k in DR.NAMES], side, side, cellsize=2.0, stream_cells=100, stream_tol_m=6.0)
    assert d2["streams"]["pred_to_truth_rms_m"] is None and d2["streams"]["pred_to_truth_max_m"] is None
    assert d2["streams"]["precision"] == 0.0 and d2["streams"]["pred_far"] == 10
    # tol2 = floor((tol / cellsize)^2), exactly
    assert stream_tolerance(2.0) == (6.0, 9) and stream_tolerance(0.1) == (3.0 * 0.1, 9) and stream_tolerance(0.7)[1] == 9
    assert stream_tolerance(2.0, 6.0) == (6.0, 9) and stream_tolerance(2.0, 5.999999)[1] == 8
    assert stream_tolerance(1.0, 0.0) == (0.0, 0) and stream_tolerance(1.0, math.sqrt(2.0))[1] == 2    # sqrt(2)^2 > 2 as doubles
    assert stream_tolerance(1.0, math.sqrt(3.0))[1] == 2                                                 # sqrt(3)^2 < 3 as doubles
    assert stream_tolerance(0.5, 10)[1] == 400 and stream_tolerance(1.0, 46340.5)[1] == 2147441940
    from fractions import Fraction
    for c, t in ((0.3, 0.9), (0.1, 0.3), (1e-3, 3e-3), (7.0, 21.0), (0.7, 2.1)):
        assert stream_tolerance(c, t)[1] == math.floor((Fraction(t) / Fraction(c)) ** 2)
    for bad in (-1.0, math.nan, math.inf, "x", True):
        with pytest.raises(ValueError, match="stream_tol_m"):
            stream_tolerance(1.0, bad)
    with pytest.raises(ValueError, match="2\\^31"):
        stream_tolerance(1.0, 46341.0)
    with pytest.raises(ValueError, match="cellsize"):
        stream_tolerance(0.0)


# ---- host-side rejection ---------------------------------------------------------------------------------------------------
def _lib():
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    return L, L.load()


def test_c_entry_points_reject_without_gpu():
    L, lib = _lib()
    f = [C.c_void_p(0x1000 * (i + 1)) for i in range(16)]
    big = 1 << 40

    def err(rc, msg):
        assert rc == -1 and msg in lib.tg_last_error(), (rc, lib.tg_last_error())

    init = lambda H, W, d=f[0], pour=f[1], cnt=f[2], ws=f[3], nb=big: lib.tg_flow_basin_init(d, pour, H, W, cnt, ws, nb, None)
    rnd = lambda H, W, k0=0, n=1, st=f[4], ws=f[3], nb=big: lib.tg_flow_basin(H, W, k0, n, st, ws, nb, None)
    fin = lambda H, W, rounds=0, c=1.0, b=f[5], nc=f[6], nd=f[7], ln=f[8], cnt=f[2], ws=f[3], nb=big: \
        lib.tg_flow_basin_finish(H, W, rounds, c, b, nc, nd, ln, cnt, ws, nb, None)
    names = ("sel", "dt", "dp", "bt", "bp", "at", "ap", "d2t", "d2p", "cnt")

    def cmp_(H, W, sc=1, tol2=0, **kw):
        a = {k: f[i] for i, k in enumerate(names)}
        a.update(kw)
        return lib.tg_flow_compare(a["sel"], a["dt"], a["dp"], a["bt"], a["bp"], a["at"], a["ap"], a["d2t"], a["d2p"], H, W, sc,
                                   tol2, a["cnt"], None)
    for H, W in ((0, 5), (5, 0), (-1, 5), (5, -1), (1 << 16, 1 << 15), (1 << 30, 2)):
        for call in (init, rnd, fin):
            err(call(H, W), b"must be non-empty with H*W < 2^31")
        assert lib.tg_flow_basin_ws_bytes(H, W) == 0
    for H, W in ((0, 5), (5, 0), (-1, 5), (32768, 1), (1, 32768), (1, 40000)):
        err(cmp_(H, W), b"both sides must lie in [1, 32767]")
    for kw in ({"d": None}, {"cnt": None}, {"ws": None}):
        err(init(8, 8, **kw), b"null pointer")
    for kw in ({"st": None}, {"ws": None}):
        err(rnd(8, 8, **kw), b"null pointer")
    for kw in ({"b": None}, {"cnt": None}, {"ws": None}):
        err(fin(8, 8, **kw), b"null pointer")
    for k in names:
        err(cmp_(8, 8, **{k: None}), b"null pointer")
    for k0, n in ((-1, 1), (0, 0), (0, 33), (32, 1), (20, 13), (33, 1), (0, -1)):
        err(rnd(8, 8, k0=k0, n=n), b"rounds")
    for rounds in (-1, 33):
        err(fin(8, 8, rounds=rounds), b"rounds")
    for c in (0.0, -1.0, math.nan, math.inf):
        err(fin(8, 8, c=c), b"cellsize")
    for sc in (0, -5):
        err(cmp_(8, 8, sc=sc), b"stream_cells")
    for t in (-1, 0x7fffffff):
        err(cmp_(8, 8, tol2=t), b"tol2")
    for H, W in ((8, 8), (129, 4097), (32767, 32767)):
        short = lib.tg_flow_basin_ws_bytes(H, W) - 1
        for call in (init, rnd, fin):
            err(call(H, W, nb=short), b"workspace")
    for call in (init, rnd, fin):
        err(call(8, 8, ws=C.c_void_p(0x1008)), b"aligned")


def test_ws_query_covers_the_layout_and_grows():
    """256 control bytes, then two planes of H W records of 16 bytes (32 bytes per pixel), each rounded up to 256 bytes."""
    L, lib = _lib()
    up = lambda n: -(-n // 256) * 256
    shapes = [(1, 1), (1, 2049), (2049, 1), (63, 65), (64, 64), (65, 63), (257, 1101), (1501, 2099), (4097, 513), (8191, 8193),
              (32767, 3), (3, 32767), (32767, 32767), (46340, 46340), (1, (1 << 31) - 1)]
    for H, W in shapes:
        assert lib.tg_flow_basin_ws_bytes(H, W) == 256 + 2 * up(16 * H * W)
    for H, W in shapes[:-3]:
        for dh, dw in ((1, 0), (0, 1), (64, 0), (0, 255), (2, 2)):
            assert lib.tg_flow_basin_ws_bytes(H + dh, W + dw) >= lib.tg_flow_basin_ws_bytes(H, W)
    P, I, SZ, D, I32 = C.c_void_p, C.c_int, C.c_size_t, C.c_double, C.c_int32
    assert L.SIGNATURES["tg_flow_basin_ws_bytes"] == (SZ, [I, I])
    assert L.SIGNATURES["tg_flow_basin_init"] == (I, [P, P, I, I, P, P, SZ, P])
    assert L.SIGNATURES["tg_flow_basin"] == (I, [I, I, I, I, P, P, SZ, P])
    assert L.SIGNATURES["tg_flow_basin_finish"] == (I, [I, I, I, D, P, P, P, P, P, P, SZ, P])
    assert L.SIGNATURES["tg_flow_compare"] == (I, [P, P, P, P, P, P, P, P, P, I, I, I32, I32, P, P])
    assert (L.TG_FLOW_BASIN_COUNTS, L.TG_FLOW_COMPARE_COUNTS) == (3, 19)


def test_ops_reject_before_any_launch():
    import torch
    from tg_hip import lib as L
    from tg_hip import ops as O
    d = torch.zeros(4, 4, dtype=torch.uint8)
    i32 = torch.zeros(4, 4, dtype=torch.int32)
    ws = torch.zeros(4096, dtype=torch.uint8)
    st = torch.zeros(2, dtype=torch.int32)
    for call in (lambda: O.flow_basin_init(d, None, ws), lambda: O.flow_basin_init(d, d, ws), lambda: O.flow_basin(4, 4, 0, 1, st, ws),
                 lambda: O.flow_basin_finish(4, 4, 0, ws), lambda: O.flow_compare(d, d, d, i32, i32, i32, i32, i32, i32, 1, 0),
                 lambda: O.flow_basin_init(np.zeros((4, 4), np.uint8), None, ws)):
        with pytest.raises(L.TgError):
            call()
    with pytest.raises(L.TgError, match="2\\^31"):
        O.flow_basin_ws(1 << 16, 1 << 15, "cpu")
    assert O.flow_basin_ws(130, 70, "cpu").numel() == _lib()[1].tg_flow_basin_ws_bytes(130, 70)
    with pytest.raises(L.TgError, match="32767"):
        O.flow_compare(torch.zeros(1, 40000, dtype=torch.uint8), d, d, i32, i32, i32, i32, i32, i32, 1, 0)


def test_python_rejects_bad_arguments():
    import torch
    from mvp_gan.src import evaluate_raster as ER
    from mvp_gan.src import flow_routing as FR
    d = np.ones((8, 8), np.uint8)
    with pytest.raises(ValueError, match="H, W"):
        FR.watersheds(np.zeros((2, 3, 4), np.uint8))
    with pytest.raises(ValueError, match="H, W"):
        FR.watersheds(np.zeros((0, 4), np.uint8))
    with pytest.raises(ValueError, match="2\\^31"):
        FR.watersheds(np.broadcast_to(np.uint8(0), (1 << 16, 1 << 15)))
    for bad in (d.astype(np.int32), d.astype(np.float32), torch.ones(8, 8, dtype=torch.int64), [[1, 2], [3, 4]]):
        with pytest.raises(ValueError, match="uint8"):
            FR.watersheds(bad)
    with pytest.raises(ValueError, match="pour_points"):
        FR.watersheds(d, np.ones((8, 9)))
    for c in (0.0, -1.0, math.nan, math.inf, None, "x"):
        with pytest.raises(ValueError, match="cellsize"):
            FR.watersheds(d, cellsize=c)
    for n in (0, -1, 1.5, "3", None, True, (1 << 20) + 1):
        with pytest.raises(ValueError, match="check_every"):
            FR.watersheds(d, check_every=n)
    for b in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="compact"):
            FR.watersheds(d, compact=b)
    sig = inspect.signature(FR.watersheds).parameters
    assert list(sig)[:2] == ["direction", "pour_points"] and sig["pour_points"].default is None
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[2:])
    assert [(k, sig[k].default) for k in list(sig)[2:]] == [("cellsize", 1.0), ("compact", False), ("check_every", 8)]
    assert FR.SQRT2 == DR.SQRT2 == math.sqrt(2.0)
    # drainage_errors and evaluate_raster
    z = np.zeros((8, 8), np.float32)
    with pytest.raises(ValueError, match="shape"):
        ER.drainage_errors(z, np.zeros((8, 9), np.float32), z, cellsize=1.0)
    with pytest.raises(ValueError, match="shape"):
        ER.drainage_errors(z, z, np.zeros((9, 8), np.uint8), cellsize=1.0)
    with pytest.raises(ValueError, match="cellsize"):
        ER.drainage_errors(z, z, z, cellsize=0.0)
    for n in (0, -1, 1.5, "3", None, True, 2 ** 31):
        with pytest.raises(ValueError, match="stream_cells"):
            ER.drainage_errors(z, z, z, cellsize=1.0, stream_cells=n)
    with pytest.raises(ValueError, match="stream_tol_m"):
        ER.drainage_errors(z, z, z, cellsize=1.0, stream_tol_m=-1.0)
    wide = np.broadcast_to(np.float32(0), (1, 40000))
    with pytest.raises(ValueError, match="32767"):
        ER.drainage_errors(wide, wide, wide, cellsize=1.0)
    sig = inspect.signature(ER.drainage_errors).parameters
    assert list(sig)[:3] == ["dem", "pred", "holes"]
    assert [(k, sig[k].default) for k in list(sig)[3:]] == [("cellsize", inspect.Parameter.empty), ("mask", None), ("nodata", None),
                                                            ("stream_cells", 1000), ("stream_tol_m", None)]
    for fn in (ER.evaluate_raster, ER.baseline_report, ER.compare_report):
        sig = inspect.signature(fn).parameters
        assert (sig["drainage"].default, sig["stream_cells"].default, sig["stream_tol_m"].default) == (False, 1000, None)


def test_no_cpu_path(monkeypatch):
    import torch
    from mvp_gan.src.evaluate_raster import drainage_errors
    from mvp_gan.src.flow_routing import watersheds
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        watersheds(np.ones((8, 8), np.uint8))
    z = np.zeros((8, 8), np.float32)
    with pytest.raises(RuntimeError, match="no HIP device|no CPU path"):
        drainage_errors(z, z, z, cellsize=1.0)


def test_compare_report_assembly_threads_drainage():
    from mvp_gan.src.evaluate_raster import assemble_compare
    raw = {"idw": {"height": 1}, "nearest": {"height": 2}}
    infos = {"idw": {"a": 1}, "nearest": {"a": 2}}
    cmp = assemble_compare(raw, infos)
    assert all("drainage" not in cmp[k] and set(cmp[k]) == {"height", "method", "fill"} for k in cmp)
    a, b = {"cells": 1}, {"cells": 2}
    cmp = assemble_compare(raw, infos, None, {"idw": a, "nearest": b})
    assert cmp["idw"]["drainage"] is a and cmp["nearest"]["drainage"] is b and "sinks" not in cmp["idw"] and "drainage" not in raw["idw"]


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_parsers():
    from mvp_gan.src.evaluate_raster import build_parser as eval_parser
    from mvp_gan.src.flow_routing import parse_args
    base = ["--dem", "in.asc", "--dir-out", "d.asc", "--acc-out", "a.asc"]
    a = parse_args(base)
    assert (a.basins_out, a.pour, a.compact, a.length_out) == (None, None, False, None)
    a = parse_args(base + ["--basins-out", "b.asc", "--pour", "p.png", "--compact", "--length-out", "l.asc"])
    assert (a.basins_out, a.pour, a.compact, a.length_out) == ("b.asc", "p.png", True, "l.asc")
    a = parse_args(base + ["--length-out", "l.asc", "--pour", "p.asc"])
    assert (a.basins_out, a.pour, a.length_out) == (None, "p.asc", "l.asc")
    for bad in (base + ["--compact"], base + ["--pour", "p.png"], base + ["--length-out", "l.asc", "--compact"],
                base + ["--basins-out"], base + ["--compact", "yes", "--basins-out", "b.asc"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
    cwd = os.path.join(ROOT, "terra-gan_amd")
    r = subprocess.run([sys.executable, "-m", "mvp_gan.src.flow_routing", "--help"], cwd=cwd, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--basins-out", "--pour", "--compact", "--length-out"):
        assert flag in r.stdout
    ebase = ["--dem", "in.asc", "--checkpoint", "ck.pth"]
    a = eval_parser().parse_args(ebase)
    assert (a.drainage, a.stream_cells, a.stream_tol) == (False, 1000, None)
    a = eval_parser().parse_args(ebase + ["--drainage", "--stream-cells", "250", "--stream-tol", "4.5", "--baseline", "laplace"])
    assert (a.drainage, a.stream_cells, a.stream_tol, a.baseline) == (True, 250, 4.5, "laplace")
    for bad in (ebase + ["--drainage", "yes"], ebase + ["--stream-cells", "x"], ebase + ["--stream-tol"]):
        with pytest.raises(SystemExit):
            eval_parser().parse_args(bad)
