"""CPU checks of the feature transform and the directional inverse-distance, nearest-neighbour and smoothing fills (csrc/edt.hip,
csrc/idw.hip, mvp_gan/src/distance.py, mvp_gan/src/interpolate.py, mvp_gan/src/evaluate_raster.py): the numpy oracle against
tests/edt_oracle.py, scipy and its own defining properties, the metres limit, host-side rejection by the C entry points and the
Python API, the workspace queries, the CLI parsers and the compare report, all without a GPU."""
import ctypes as C
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import edt_oracle as EO
from tests import idw_oracle as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def contract():
    """The oracle implements the contract include/terragan_hip.h states: the tie rule and the order of the directions."""
    txt = " ".join(open(os.path.join(ROOT, "include", "terragan_hip.h")).read().split())
    for name in ("tg_edt_nearest_ws_bytes", "tg_edt_nearest", "tg_rayfill_ws_bytes", "tg_rayfill", "tg_gather_fill",
                 "tg_void_smooth"):
        assert name + "(" in txt, name
    assert "the smallest row, among those the smallest column" in txt
    assert "N, NE, E, SE, S, SW, W, NW, (dy, dx) = " + ", ".join(f"({dy},{dx})" for dy, dx in IO.DIRS) in txt.replace("* ", "")
    return txt


def _masks():
    rng = np.random.default_rng(5)
    out = [rng.random((40, 40)) < 0.02, rng.random((33, 17)) < 0.3, rng.random((1, 40)) < 0.1, rng.random((40, 1)) < 0.1,
           rng.random((25, 40)) < 0.005, np.zeros((9, 13), bool), np.ones((5, 4), bool)]
    lone = np.zeros((40, 31), bool)
    lone[39, 30] = True
    out.append(lone)
    pair = np.zeros((21, 21), bool)                          # ties: above / below and left / right of the centre
    pair[[3, 17], 10] = True
    pair[10, [3, 17]] = True
    out.append(pair)
    return out


def test_feature_transform_oracle():
    for s in _masks():
        H, W = s.shape
        d2, idx = IO.nearest(s)
        np.testing.assert_array_equal(d2, EO.edt_d2(s))
        if not s.any():
            assert (idx == -1).all() and (d2 == IO.FAR).all()
            continue
        iy, ix = np.divmod(idx.astype(np.int64), W)
        y, x = np.mgrid[0:H, 0:W]
        assert s[iy, ix].all()                                              # the index is a seed
        np.testing.assert_array_equal((y - iy) ** 2 + (x - ix) ** 2, d2)    # at that distance
        ys, xs = np.nonzero(s)
        for py in range(H):                                                 # and the lexicographic minimum among those
            for px in range(W):
                at = (ys - py) ** 2 + (xs - px) ** 2 == d2[py, px]
                assert (int(iy[py, px]), int(ix[py, px])) == min(zip(ys[at].tolist(), xs[at].tolist()))
        for cap2 in (1, 2, 25):
            c2, ci = IO.nearest(s, cap2)
            np.testing.assert_array_equal(c2, EO.edt_d2(s, cap2))
            np.testing.assert_array_equal(ci, np.where(d2 >= cap2, -1, idx))
    d2, idx = IO.nearest(_masks()[-1])
    assert idx[10, 10] == 3 * 21 + 10 and idx[10, 9] == 10 * 21 + 3       # the row above wins; then the nearer column


def test_feature_transform_oracle_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for s in _masks():
        if not s.any():
            continue
        dist, ind = ndi.distance_transform_edt(~s, return_indices=True)
        d2, idx = IO.nearest(s)
        y, x = np.mgrid[0:s.shape[0], 0:s.shape[1]]
        np.testing.assert_array_equal((y - ind[0]) ** 2 + (x - ind[1]) ** 2, d2)      # its tie rule differs: distances only
        np.testing.assert_array_equal(np.rint(dist * dist).astype(np.int64), d2)


def test_ray_px2():
    from mvp_gan.src.interpolate import ray_px2
    assert ray_px2(1.25, 0.25) == 25 and ray_px2(5.0, 1.0) == 25 and ray_px2(2.5, 2.5) == 1 and ray_px2(10.0, 2.5) == 16
    assert ray_px2(1.0, 1 / 3) == 9 and ray_px2(1.5, 1.0) == 2                       # sqrt(2) <= 1.5 < sqrt(3)
    rng = np.random.default_rng(11)
    for c in (0.25, 1.0, 1 / 3, 2.5, 0.37):
        for e in rng.uniform(c, 300.0, 20).tolist() + [c * 7, c, c * math.sqrt(2.0) * 1.0000001, c * math.sqrt(2.0) * 0.9999999]:
            n = ray_px2(e, c)
            assert n == IO.ray_px2(e, c)
            assert c * math.sqrt(n) <= e < c * math.sqrt(n + 1)
    for bad in (0.0, -1.0, math.nan, math.inf, "x", None):
        with pytest.raises(ValueError, match="finite"):
            ray_px2(bad, 1.0)
    with pytest.raises(ValueError, match="beyond"):
        ray_px2(50000.0, 1.0)
    with pytest.raises(ValueError, match="shorter than one cell"):
        ray_px2(0.9, 1.0)
    with pytest.raises(ValueError, match="cellsize"):
        ray_px2(1.0, 0.0)
    assert IO.ray_px2(0.9, 1.0) == 0


def test_fill_oracle_properties():
    rng = np.random.default_rng(17)
    known = rng.random((40, 50)) < 0.05
    z = (1000 + rng.normal(0, 3, (40, 50))).astype(np.float32)
    ft = IO.nearest(known)
    for power in (2.0, 1.0, 1.5):
        out, counts, lo, hi = IO.rayfill(z, known, 0, power, *ft)
        assert sum(counts) == int((~known).sum()) and counts[2] == 0
        np.testing.assert_array_equal(out[known].view(np.int32), z[known].view(np.int32))
        rays = ~np.isnan(lo)
        assert (out[rays] >= lo[rays]).all() and (out[rays] <= hi[rays]).all()       # a convex combination
        const, _, _, _ = IO.rayfill(np.full_like(z, 321.125), known, 0, power, *ft)
        assert (const == np.float32(321.125)).all()                                  # a constant field comes back constant
    one = np.zeros((9, 11), bool)
    one[4, 5] = True
    z1 = np.zeros((9, 11), np.float32)
    z1[4, 5] = 7.5
    out, counts, _, _ = IO.rayfill(z1, one, 0, 2.0)                                  # a single seed: its value along 8 rays
    hit = (IO.ray_hits(one) != 0).any(axis=0)
    assert counts == [int(hit.sum()), 0, 98 - int(hit.sum())] and (out[hit] == 7.5).all() and np.isnan(out[~hit & ~one]).all()
    assert int(hit.sum()) == 4 + 4 + 5 + 5 + 4 * 4                                   # column, row and the four diagonals
    out, counts, _, _ = IO.rayfill(z1, one, 0, 2.0, *IO.nearest(one))
    assert counts[2] == 0 and (out == 7.5).all()
    out, counts = IO.gather_fill(z1, one, IO.nearest(one, 5)[1])                     # d2 < 5 only
    assert counts == [12, 86] and (out[~np.isnan(out)] == 7.5).all()
    h = IO.ray_hits(one, 2)
    assert int((h != 0).sum()) == 8 and set(np.unique(h)) == {0, 1}
    # smoothing: known and NaN pixels stay, a constant stays, one step is the clipped 3x3 mean
    a = np.array([[1, 2, np.nan], [4, 5, 6], [7, 8, 9]], np.float32)
    kn = np.zeros((3, 3), bool)
    kn[0, 0] = True
    sm = IO.smooth(a, kn, 1)
    assert sm[0, 0] == 1 and np.isnan(sm[0, 2]) and sm[1, 1] == np.float32(42 / 8) and sm[2, 2] == np.float32(28 / 4)
    assert sm[0, 1] == np.float32(18 / 5)
    assert (IO.smooth(np.full((5, 6), 2.5, np.float32), np.zeros((5, 6), bool), 4) == 2.5).all()


# ---- host-side rejection ---------------------------------------------------------------------------------------------------
def _lib():
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    return L, L.load()


def test_c_entry_points_reject_without_gpu():
    L, lib = _lib()
    f = [C.c_void_p(0x1000 * (i + 1)) for i in range(12)]
    big = 1 << 40

    def err(rc, msg):
        assert rc == -1 and msg in lib.tg_last_error(), (rc, lib.tg_last_error())

    ft = lambda H, W, seed=f[0], d2=f[1], idx=f[2], ws=f[3], nb=big: lib.tg_edt_nearest(seed, H, W, 0, d2, idx, ws, nb, None)
    rf = lambda H, W, z=f[0], kn=f[1], power=2.0, d2=None, idx=None, out=f[2], counts=f[3], ws=f[4], nb=big: \
        lib.tg_rayfill(z, kn, H, W, 0, power, d2, idx, out, None, counts, ws, nb, None)
    gf = lambda H, W, z=f[0], kn=f[1], idx=f[2], out=f[3], counts=f[4]: lib.tg_gather_fill(z, kn, idx, H, W, out, counts, None)
    sm = lambda H, W, a=f[0], kn=f[1], out=f[2]: lib.tg_void_smooth(a, kn, H, W, out, None)
    for H, W in ((0, 5), (5, 0), (-1, 5), (32768, 5), (5, 32768), (1 << 16, 1 << 15)):
        for call in (ft, rf, gf, sm):
            err(call(H, W), b"sides")
        assert lib.tg_edt_nearest_ws_bytes(H, W) == 0 and lib.tg_rayfill_ws_bytes(H, W) == 0
    for kw in ({"seed": None}, {"d2": None}, {"idx": None}, {"ws": None}):
        err(ft(8, 8, **kw), b"null pointer")
    err(ft(8, 8, nb=lib.tg_edt_nearest_ws_bytes(8, 8) - 1), b"workspace")
    err(ft(32767, 32767, nb=lib.tg_edt_nearest_ws_bytes(32767, 32767) - 1), b"workspace")
    for kw in ({"z": None}, {"kn": None}, {"out": None}, {"counts": None}, {"ws": None}):
        err(rf(8, 8, **kw), b"null pointer")
    err(rf(8, 8, d2=f[5]), b"go together")
    err(rf(8, 8, idx=f[5]), b"go together")
    err(rf(8, 8, out=f[0]), b"alias")
    for p in (0.0, -2.0, 8.5, math.nan, math.inf):
        err(rf(8, 8, power=p), b"power")
    err(rf(8, 8, nb=lib.tg_rayfill_ws_bytes(8, 8) - 1), b"workspace")
    err(rf(32767, 32767, nb=lib.tg_rayfill_ws_bytes(32767, 32767) - 1), b"workspace")
    for kw in ({"z": None}, {"kn": None}, {"idx": None}, {"out": None}, {"counts": None}):
        err(gf(8, 8, **kw), b"null pointer")
    err(gf(8, 8, out=f[0]), b"alias")
    for kw in ({"a": None}, {"kn": None}, {"out": None}):
        err(sm(8, 8, **kw), b"null pointer")
    err(sm(8, 8, out=f[0]), b"distinct")


def test_ws_queries_cover_the_layout_and_grow():
    """tg_edt_nearest: tg_edt's workspace (the side of the nearest seed rides in bit 15 of the uint16 column distance).
    tg_rayfill: per family of lines a 64-bit word and two int32 positions per 64-pixel band and line; W lines of ceil(H / 64)
    bands (columns), H lines of ceil(W / 64) bands (rows), and twice W + H - 1 lines of ceil(H / 64) bands (diagonals)."""
    _, lib = _lib()
    shapes = [(1, 1), (1, 2049), (2049, 1), (63, 65), (64, 64), (65, 63), (257, 1101), (1501, 2099), (4097, 513), (8191, 8193),
              (32767, 3), (3, 32767), (32767, 32767)]
    for H, W in shapes:
        nbh, nbw = -(-H // 64), -(-W // 64)
        assert lib.tg_edt_nearest_ws_bytes(H, W) == lib.tg_edt_ws_bytes(H, W) >= nbh * W * 16 + H * W * 2
        need = 16 * (nbh * W + nbw * H + 2 * nbh * (W + H - 1))
        assert need <= lib.tg_rayfill_ws_bytes(H, W) <= need + 12 * 256
    for H, W in shapes[:-1]:
        for dh, dw in ((1, 0), (0, 1), (64, 0), (0, 255), (2, 2)):
            if max(H + dh, W + dw) <= 32767:
                assert lib.tg_rayfill_ws_bytes(H + dh, W + dw) >= lib.tg_rayfill_ws_bytes(H, W)
                assert lib.tg_edt_nearest_ws_bytes(H + dh, W + dw) >= lib.tg_edt_nearest_ws_bytes(H, W)


def test_python_rejects_bad_arguments():
    from mvp_gan.src.distance import nearest_known
    from mvp_gan.src.evaluate_raster import COMPARES, evaluate_raster
    from mvp_gan.src.interpolate import METHODS, interpolate_voids
    z = np.zeros((8, 8), np.float32)
    for fn in (nearest_known, interpolate_voids):
        with pytest.raises(ValueError, match="H, W"):
            fn(np.zeros((2, 3, 4), np.float32))
        with pytest.raises(ValueError, match="H, W"):
            fn(np.zeros((0, 4), np.float32))
        with pytest.raises(ValueError, match="32767"):
            fn(np.broadcast_to(np.float32(0), (1, 32768)))
        with pytest.raises(ValueError, match="32767"):
            fn(np.broadcast_to(np.float32(0), (32768, 2)))
        with pytest.raises(ValueError, match="mask"):
            fn(z, np.ones((8, 9)))
        for c in (0.0, -1.0, math.nan, math.inf, None, "x"):
            with pytest.raises(ValueError, match="cellsize"):
                fn(z, cellsize=c)
        for md in (0.0, -3.0, math.nan, math.inf, "far", 1e6):
            with pytest.raises(ValueError, match="max_distance"):
                fn(z, max_distance=md)
    with pytest.raises(ValueError, match="max_distance"):
        interpolate_voids(z, max_distance=0.5)                               # shorter than one cell
    for m in ("laplace", "biharmonic", "IDW", None, 2):
        with pytest.raises(ValueError, match="method"):
            interpolate_voids(z, method=m)
    for p in (0.0, -1.0, 8.5, math.nan, math.inf, "x", None):
        with pytest.raises(ValueError, match="power"):
            interpolate_voids(z, power=p)
    for s in (-1, 65, 1.5, "3", None, True):
        with pytest.raises(ValueError, match="smooth"):
            interpolate_voids(z, smooth=s)
    for fb in ("laplace", "idw", 0, True):
        with pytest.raises(ValueError, match="fallback"):
            interpolate_voids(z, fallback=fb)
    for cmp in ("laplace", ("idw", "biharmonic"), ("idw", "idw"), 5, ("nearest", None)):
        with pytest.raises(ValueError, match="compare"):
            evaluate_raster("missing.pth", z, cellsize=1.0, compare=cmp)
    with pytest.raises(ValueError, match="baseline"):
        evaluate_raster("missing.pth", z, cellsize=1.0, baseline="idw")      # the baselines stay fill_voids' methods
    assert METHODS == COMPARES == ("idw", "nearest")
    assert inspect.signature(evaluate_raster).parameters["compare"].default is None
    sig = inspect.signature(interpolate_voids).parameters
    assert [(k, sig[k].default) for k in list(sig)[2:]] == [("nodata", None), ("method", "idw"), ("power", 2.0),
                                                            ("max_distance", None), ("cellsize", 1.0), ("smooth", 0),
                                                            ("fallback", "nearest")]
    sig = inspect.signature(nearest_known).parameters
    assert list(sig) == ["dem", "mask", "nodata", "cellsize", "max_distance"]


def test_no_cpu_path(monkeypatch):
    import torch
    from mvp_gan.src.distance import nearest_known
    from mvp_gan.src.interpolate import interpolate_voids
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    z = np.zeros((8, 8), np.float32)
    for fn in (nearest_known, interpolate_voids):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(z)


def test_ops_reject_before_any_launch():
    import torch
    from tg_hip import lib as L
    from tg_hip import ops as O
    with pytest.raises(L.TgError, match="seed"):
        O.edt_nearest(np.zeros((4, 4), np.uint8))
    with pytest.raises(L.TgError, match="seed"):
        O.edt_nearest(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(L.TgError, match="32767"):
        O.edt_nearest(torch.zeros(1, 1, dtype=torch.uint8).expand(2, 32768))
    for fn in (O.rayfill, O.gather_fill, O.void_smooth):
        with pytest.raises(L.TgError):
            fn(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.uint8), *([torch.zeros(4, 4, dtype=torch.int32)]
                                                                           if fn is O.gather_fill else []))


# ---- CLI parsers and the report ----------------------------------------------------------------------------------------------
def test_cli_parsers():
    from mvp_gan.src.evaluate_raster import build_parser as eval_parser
    from mvp_gan.src.interpolate import build_parser
    a = build_parser().parse_args(["--dem", "in.asc", "--out", "o.asc"])
    assert (a.dem, a.out, a.mask, a.nodata, a.method, a.power, a.max_distance, a.smooth, a.no_fallback) == \
        ("in.asc", "o.asc", None, None, "idw", 2.0, None, 0, False)
    a = build_parser().parse_args(["--dem", "in.asc", "--out", "o.asc", "--mask", "m.png", "--nodata", "-9999", "--method",
                                   "nearest", "--power", "1.5", "--max-distance", "50", "--smooth", "3", "--no-fallback"])
    assert (a.mask, a.nodata, a.method, a.power, a.max_distance, a.smooth, a.no_fallback) == \
        ("m.png", -9999.0, "nearest", 1.5, 50.0, 3, True)
    for bad in (["--dem", "in.asc"], ["--dem", "in.asc", "--out", "o.asc", "--method", "laplace"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(bad)
    for base in (["--dem", "in.asc", "--checkpoint", "g.pth"], ["--dem", "in.asc", "--pred", "p.asc", "--holes", "h.png"]):
        assert eval_parser().parse_args(base).compare is None
        assert eval_parser().parse_args(base + ["--compare", "idw"]).compare == ["idw"]
        a = eval_parser().parse_args(base + ["--compare", "idw", "nearest", "--baseline", "laplace", "--by-depth"])
        assert a.compare == ["idw", "nearest"] and a.baseline == "laplace" and a.by_depth == []
        for bad in (["--compare"], ["--compare", "laplace"], ["--baseline", "idw"]):
            with pytest.raises(SystemExit):
                eval_parser().parse_args(base + bad)
    r = subprocess.run([sys.executable, "-m", "mvp_gan.src.interpolate", "--help"], cwd=os.path.join(ROOT, "terra-gan_amd"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--dem", "--out", "--mask", "--nodata", "--method", "--power", "--max-distance", "--smooth", "--no-fallback"):
        assert flag in r.stdout


def test_compare_report_assembly():
    from mvp_gan.src.evaluate_raster import assemble_compare
    from tests.test_edt_cpu import _raw_report
    depth = {"edges_m": [2.0, 5.0, 10.0], "cap_d2": 25, "counts": [6, 0, 4, 0, 0, 0, 0, 0],
             "sum_a": [5.0, 0.0, 6.0, 0.0] + [0.0] * 4, "sum_a2": [9.0, 0.0, 11.5, 0.0] + [0.0] * 4,
             "max_bits": [0] * 8, "hole_d2": np.array([25, 2], np.int32)}
    raw = {"idw": _raw_report(depth), "nearest": _raw_report(None)}
    infos = {"idw": {"unknown": 12, "filled": 12, "by_nearest": 1, "unfilled": 0, "method": "idw", "power": 2.0, "smooth": 0,
                     "max_distance": None, "lim2": None},
             "nearest": {"unknown": 12, "filled": 12, "by_nearest": 12, "unfilled": 0, "method": "nearest", "power": 2.0,
                         "smooth": 0, "max_distance": None, "lim2": None}}
    cmp = assemble_compare(raw, infos)
    assert list(cmp) == ["idw", "nearest"]
    for name in cmp:
        assert cmp[name]["method"] == name and cmp[name]["fill"] == infos[name]
        assert {k: v for k, v in cmp[name].items() if k not in ("method", "fill")} == raw[name]
        assert "method" not in raw[name]                                  # the terrain_errors report is not modified
    assert "by_depth" in cmp["idw"] and "by_depth" not in cmp["nearest"]
    assert set(cmp["idw"]) - set(raw["idw"]) == {"method", "fill"}         # baseline_report's shape
