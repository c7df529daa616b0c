"""CPU checks of the distance to the nearest known pixel and the errors by depth (csrc/edt.hip, mvp_gan/src/distance.py,
mvp_gan/src/evaluate_raster.py): the numpy oracle against scipy and against a per-pixel brute force, the metres thresholds,
host-side rejection by the C entry points and the Python API, the workspace queries, the CLI parsers and the report assembly,
all without a GPU."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import edt_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layouts():
    rng = np.random.default_rng(3)
    out = [np.ones((1, 1), np.uint8), rng.random((1, 300)) < 0.01, rng.random((300, 1)) < 0.01, rng.random((7, 300)) < 0.01,
           rng.random((130, 67)) < 0.2, rng.random((65, 257)) < 0.002]
    one = np.zeros((65, 257), bool)
    one[:, 100] = rng.random(65) < 0.3
    out.append(one)
    row = np.zeros((65, 257), bool)
    row[40] = rng.random(257) < 0.1
    out.append(row)
    corner = np.zeros((130, 67), bool)
    corner[129, 0] = True
    out.append(corner)
    return [np.ascontiguousarray(s, dtype=np.uint8) for s in out if s.any()]


def test_oracle_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for s in _layouts():
        want = ndi.distance_transform_edt(s == 0)
        got = EO.edt_d2(s)
        np.testing.assert_array_equal(got, np.rint(want * want).astype(np.int64))
        np.testing.assert_allclose(EO.metres(got, 2.5), 2.5 * want, rtol=1e-6)


def test_oracle_against_brute_force():
    rng = np.random.default_rng(5)
    cases = [rng.random((40, 40)) < 0.02, rng.random((33, 17)) < 0.3, rng.random((1, 40)) < 0.1, rng.random((40, 1)) < 0.1,
             np.zeros((9, 13), bool), np.ones((5, 4), bool)]
    lone = np.zeros((40, 31), bool)
    lone[39, 30] = True
    cases.append(lone)
    for s in cases:
        np.testing.assert_array_equal(EO.edt_d2(s), EO.brute_d2(s))
    assert (EO.edt_d2(cases[4]) == EO.FAR).all() and (EO.edt_d2(cases[5]) == 0).all()
    assert EO.edt_d2(lone)[0, 0] == 39 * 39 + 30 * 30


def test_oracle_cap_and_metres():
    rng = np.random.default_rng(7)
    s = rng.random((50, 90)) < 0.003
    full = EO.edt_d2(s)
    assert full.max() > 400
    for cap2 in (1, 2, 25, 400):
        np.testing.assert_array_equal(EO.edt_d2(s, cap2), np.minimum(full, cap2))
    np.testing.assert_array_equal(EO.edt_d2(np.zeros((4, 5), bool), 9), np.full((4, 5), 9))
    m = EO.metres(np.array([[0, 1, 2, 25, EO.FAR]]), 0.25)
    assert m.dtype == np.float32 and m[0, :4].tolist() == [0.0, 0.25, float(np.float32(0.25 * math.sqrt(2.0))), 1.25]
    assert np.isinf(m[0, 4])


def test_depth_px2_thresholds():
    from mvp_gan.src.distance import depth_px2, px2_m
    assert depth_px2([2, 5, 10, 25, 50], 1.0) == [4, 25, 100, 625, 2500]
    assert depth_px2([2, 5, 10], 0.25) == [64, 400, 1600]
    assert depth_px2([2.5, 5, 10, 25], 2.5) == [1, 4, 16, 100]
    assert depth_px2([1, 2, 10], 1 / 3) == [9, 36, 900]
    assert depth_px2([1.5], 1.0) == [3] and depth_px2([1e-9], 1.0) == [1]      # sqrt(2) < 1.5 <= sqrt(3)
    rng = np.random.default_rng(11)
    for c in (0.25, 1.0, 1 / 3, 2.5, 0.37):
        edges = sorted(rng.uniform(0.01, 300.0, 20).tolist()) + [c * 7, c * math.sqrt(2.0) * 1.0000001]
        got = depth_px2(edges, c)
        assert got == EO.depth_px2(edges, c)
        for e, t in zip(edges, got):
            assert math.sqrt(t) * c >= e and (t == 0 or math.sqrt(t - 1) * c < e)
    assert px2_m(25, 0.25) == 1.25 and math.isinf(px2_m(EO.FAR, 1.0))
    for bad in (0.0, -1.0, math.nan, math.inf, "x", None):
        with pytest.raises(ValueError, match="finite"):
            depth_px2([bad], 1.0)
    with pytest.raises(ValueError, match="beyond"):
        depth_px2([50000.0], 1.0)
    with pytest.raises(ValueError, match="cellsize"):
        depth_px2([1.0], 0.0)


def test_oracle_depth_classes():
    a = np.array([np.nan, 0.5, 1.0, 2.0, np.nan, 4.0, 0.25], np.float32)
    d2 = np.array([0, 1, 3, 4, 100, 24, 25], np.int32)
    r = EO.depth_classes(a, d2, [4, 25])
    assert r["counts"] == [2, 2, 1, 0, 0, 0, 0, 0]
    assert r["sum_a"][:3] == [1.5, 6.0, 0.25] and r["sum_a2"][:3] == [1.25, 20.0, 0.0625]
    assert r["max_bits"][:4] == [int(np.float32(v).view(np.uint32)) for v in (1.0, 4.0, 0.25)] + [0]
    lab = np.array([[-1, 3, 3], [7, -1, 3]], np.int32)
    assert EO.hole_max_d2(lab, np.array([[9, 1, 4], [2, 8, 5]])) == {3: 5, 7: 2}


def test_ring_is_depth_one_or_two():
    """A pixel has an 8-neighbour among the seeds exactly when 1 <= d2 <= 2."""
    rng = np.random.default_rng(13)
    s = rng.random((60, 70)) < 0.05
    d2 = EO.edt_d2(s)
    p = np.pad(s, 1)
    nb = np.zeros_like(s)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                nb |= p[dy:dy + 60, dx:dx + 70]
    np.testing.assert_array_equal(nb & ~s, (d2 >= 1) & (d2 <= 2))


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

    cls = L.TgDepthClasses(2, 0)
    cls.d2[0], cls.d2[1] = 4, 25
    edt = lambda H, W, seed=f[0], d2=f[1], dist=None, c=1.0, ws=f[2], nb=big: lib.tg_edt(seed, H, W, 0, c, d2, dist, ws, nb, None)
    de = lambda H, W, n=1, cl=cls, a=f[0], hd=f[6], nb=big: lib.tg_depth_errors(a, f[1], f[2], f[3], n, H, W, C.byref(cl), f[4],
                                                                               f[5], hd, f[7], nb, None)
    for H, W in ((0, 5), (5, 0), (-1, 5), (32768, 5), (5, 32768), (1 << 16, 1 << 15)):
        err(edt(H, W), b"sides")
        err(de(H, W), b"sides")
        err(lib.tg_depth_errors_finish(H, W, f[0], big, f[1], None), b"sides")
        assert lib.tg_edt_ws_bytes(H, W) == 0 and lib.tg_depth_errors_ws_bytes(H, W) == 0
    err(edt(8, 8, seed=None), b"null pointer")
    err(edt(8, 8, d2=None), b"null pointer")
    err(edt(8, 8, ws=None), b"null pointer")
    for c in (0.0, -1.0, math.nan, math.inf):
        err(edt(8, 8, dist=f[3], c=c), b"cellsize")
    err(edt(8, 8, nb=lib.tg_edt_ws_bytes(8, 8) - 1), b"workspace")
    err(edt(32767, 32767, nb=lib.tg_edt_ws_bytes(32767, 32767) - 1), b"workspace")
    err(de(8, 8, a=None), b"null pointer")
    err(de(8, 8, hd=None), b"null pointer")
    err(de(8, 8, n=-1), b"nholes")
    err(de(8, 8, nb=lib.tg_depth_errors_ws_bytes(8, 8) - 1), b"workspace")
    err(de(8, 8, cl=L.TgDepthClasses(8, 0)), b"class edges")
    err(de(8, 8, cl=L.TgDepthClasses(-1, 0)), b"class edges")
    dec = L.TgDepthClasses(2, 0)
    dec.d2[0], dec.d2[1] = 10, 5
    err(de(8, 8, cl=dec), b"nondecreasing")
    err(lib.tg_depth_errors_finish(8, 8, None, big, f[1], None), b"null pointer")
    err(lib.tg_depth_errors_finish(8, 8, f[0], 0, f[1], None), b"workspace")


def test_constants_mirror_the_header():
    L, _ = _lib()
    txt = open(os.path.join(ROOT, "include", "terragan_hip.h")).read()
    assert "TG_EDT_FAR = 0x7fffffff, TG_EDT_MAX_SIDE = 32767" in txt and "TG_DEPTH_MAX_CLASSES = 8" in txt
    assert (L.TG_EDT_FAR, L.TG_EDT_MAX_SIDE, L.TG_DEPTH_MAX_CLASSES) == (0x7fffffff, 32767, 8)
    assert C.sizeof(L.TgDepthClasses) == 8 + 4 * 7
    assert 2 * L.TG_EDT_MAX_SIDE ** 2 < 2 ** 31 <= 2 * (L.TG_EDT_MAX_SIDE + 1) ** 2
    from mvp_gan.src import distance as D
    from mvp_gan.src import evaluate_raster as E
    assert (D.FAR, D.MAX_SIDE) == (L.TG_EDT_FAR, L.TG_EDT_MAX_SIDE) and E.MAX_CLASSES == L.TG_DEPTH_MAX_CLASSES
    assert E.DEPTH_EDGES_M == (2, 5, 10, 25, 50)


def test_ws_queries_cover_the_kernels_extents_and_grow():
    """tg_edt: a 64-bit word and two int32 rows per 64-row band and column, and the uint16 column distances; tg_depth_errors:
    16 doubles per workgroup, min(ceil(H W / 256), 2048) workgroups."""
    _, lib = _lib()
    shapes = [(1, 1), (1, 2049), (2049, 1), (63, 65), (64, 64), (65, 63), (257, 1100), (1501, 2099), (4097, 513), (8192, 8192),
              (32767, 3), (3, 32767), (32767, 32767)]
    for H, W in shapes:
        nb = -(-H // 64)
        assert lib.tg_edt_ws_bytes(H, W) >= nb * W * 16 + H * W * 2
        assert lib.tg_depth_errors_ws_bytes(H, W) >= min(-(-H * W // 256), 2048) * 16 * 8
    for H, W in shapes[:-1]:
        for dh, dw in ((1, 0), (0, 1), (64, 0), (0, 255)):
            if max(H + dh, W + dw) <= 32767:
                assert lib.tg_edt_ws_bytes(H + dh, W + dw) >= lib.tg_edt_ws_bytes(H, W)
                assert lib.tg_depth_errors_ws_bytes(H + dh, W + dw) >= lib.tg_depth_errors_ws_bytes(H, W)


def test_python_rejects_bad_arguments():
    from mvp_gan.src.distance import distance_to_known
    from mvp_gan.src.evaluate_raster import baseline_report, evaluate_raster, terrain_errors
    z = np.zeros((8, 8), np.float32)
    with pytest.raises(ValueError, match="H, W"):
        distance_to_known(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError, match="H, W"):
        distance_to_known(np.zeros((0, 4), np.float32))
    with pytest.raises(ValueError, match="32767"):
        distance_to_known(np.broadcast_to(np.float32(0), (1, 32768)))
    with pytest.raises(ValueError, match="32767"):
        distance_to_known(np.broadcast_to(np.float32(0), (32768, 2)))
    with pytest.raises(ValueError, match="mask"):
        distance_to_known(z, np.ones((8, 9)))
    for c in (0.0, -1.0, math.nan, math.inf, None, "x"):
        with pytest.raises(ValueError, match="cellsize"):
            distance_to_known(z, cellsize=c)
    for md in (0.0, -3.0, math.nan, math.inf, "far", 1e6):
        with pytest.raises(ValueError, match="max_distance"):
            distance_to_known(z, max_distance=md)
    for edges in ((), (5, 2), (2, 2), (0, 10), (-1,), (math.inf,), (math.nan,), tuple(range(1, 9)), ("a",), 5):
        with pytest.raises(ValueError, match="depth_edges_m"):
            terrain_errors(z, z, z, z, cellsize=1.0, depth_edges_m=edges)
        with pytest.raises(ValueError, match="depth_edges_m"):
            evaluate_raster("missing.pth", z, cellsize=1.0, depth_edges_m=edges)
    with pytest.raises(ValueError, match="depth_edges_m"):
        terrain_errors(z, z, z, z, cellsize=0.001, depth_edges_m=(2, 50))        # 50 m is 50000 px: no raster is that wide
    wide = np.broadcast_to(np.float32(0), (1, 32768))
    with pytest.raises(ValueError, match="32767"):
        terrain_errors(wide, wide, wide, wide, cellsize=1.0, depth_edges_m=(2, 5))
    import inspect
    for fn in (terrain_errors, baseline_report, evaluate_raster):
        assert inspect.signature(fn).parameters["depth_edges_m"].default is None


def test_ops_reject_before_any_launch():
    """The tensor-level wrappers check type, shape and range first: a numpy array is no HIP tensor."""
    import torch
    from tg_hip import lib as L
    from tg_hip import ops as O
    with pytest.raises(L.TgError, match="seed"):
        O.edt(np.zeros((4, 4), np.uint8))
    with pytest.raises(L.TgError, match="seed"):
        O.edt(torch.zeros(4, 4, dtype=torch.uint8))                       # on the CPU
    with pytest.raises(L.TgError, match="32767"):
        O.edt(torch.zeros(1, 1, dtype=torch.uint8).expand(2, 32768))
    with pytest.raises(L.TgError, match="d2"):
        O.depth_errors(torch.zeros(16), torch.zeros(4, 4, dtype=torch.int32), None, None, 0, [4])
    assert (O.EDT_FAR, O.EDT_MAX_SIDE, O.DEPTH_MAX_CLASSES) == (0x7fffffff, 32767, 8)


# ---- CLI parsers and the report ----------------------------------------------------------------------------------------------
def test_cli_parsers():
    from mvp_gan.src.distance import build_parser as dist_parser
    from mvp_gan.src.evaluate_raster import DEPTH_EDGES_M, build_parser as eval_parser
    a = dist_parser().parse_args(["--dem", "in.asc", "--out", "d.asc"])
    assert (a.dem, a.out, a.mask, a.nodata, a.max_distance) == ("in.asc", "d.asc", None, None, None)
    a = dist_parser().parse_args(["--dem", "in.asc", "--out", "d.asc", "--mask", "m.png", "--nodata", "-9999", "--max-distance",
                                  "50"])
    assert (a.mask, a.nodata, a.max_distance) == ("m.png", -9999.0, 50.0)
    with pytest.raises(SystemExit):
        dist_parser().parse_args(["--dem", "in.asc"])
    base = ["--dem", "in.asc", "--checkpoint", "g.pth"]
    assert eval_parser().parse_args(base).by_depth is None
    assert eval_parser().parse_args(base + ["--by-depth"]).by_depth == []
    assert eval_parser().parse_args(base + ["--by-depth", "--baseline", "laplace"]).by_depth == []
    assert eval_parser().parse_args(base + ["--by-depth", "1", "2.5", "40"]).by_depth == [1.0, 2.5, 40.0]
    assert DEPTH_EDGES_M == (2.0, 5.0, 10.0, 25.0, 50.0)
    r = subprocess.run([sys.executable, "-m", "mvp_gan.src.distance", "--help"], cwd=os.path.join(ROOT, "terra-gan_amd"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--dem", "--out", "--mask", "--nodata", "--max-distance"):
        assert flag in r.stdout


def _raw_report(depth):
    from mvp_gan.src.evaluate_raster import COUNTS, SUMS, assemble_report
    counts = dict(zip(COUNTS, (100, 12, 0, 10, 2, 6, 4, 2, 0, int(np.float32(3.0).view(np.uint32)))))
    sums = dict(zip(SUMS, (1.0, 11.0, 20.5, 1.0, 1.0, 1.0, 1.0, 5.0, 9.0, 1.0)))
    sums["class_a"], sums["class_a2"] = [11.0, 0.0], [20.5, 0.0]
    bits = lambda v: int(np.float32(v).view(np.uint32))
    table = np.array([[5, 8, 7, int(8.0 * 2 ** 16), bits(3.0), 0, 5, 2, 8], [40, 4, 3, int(3.0 * 2 ** 16), bits(1.5), 4, 0, 5, 1]],
                     np.int64)
    return assemble_report(counts, sums, table, [1.0], 0.5, cellsize=2.0, edges_m2=[100.0], quantiles=[0.5], top=10, depth=depth)


def test_report_assembly_with_and_without_depth():
    bits = lambda v: int(np.float32(v).view(np.uint32))
    plain = _raw_report(None)
    assert "by_depth" not in plain and all("depth_m" not in h for h in plain["holes"]["worst"])
    depth = {"edges_m": [2.0, 5.0, 10.0], "cap_d2": 25, "counts": [6, 0, 4, 0, 0, 0, 0, 0],
             "sum_a": [5.0, 0.0, 6.0, 0.0] + [0.0] * 4, "sum_a2": [9.0, 0.0, 11.5, 0.0] + [0.0] * 4,
             "max_bits": [bits(1.5), 0, bits(3.0), 0, 0, 0, 0, 0], "hole_d2": np.array([25, 2], np.int32)}
    rep = _raw_report(depth)
    bd = rep["by_depth"]
    assert bd["cap_m"] == 10.0 and len(bd["classes"]) == 4
    assert [(k["lo_m"], k["hi_m"], k["pixels"]) for k in bd["classes"]] == [(0.0, 2.0, 6), (2.0, 5.0, 0), (5.0, 10.0, 4),
                                                                            (10.0, math.inf, 0)]
    assert bd["classes"][0]["mae"] == 5.0 / 6 and bd["classes"][0]["rmse"] == math.sqrt(9.0 / 6) and bd["classes"][0]["max"] == 1.5
    assert bd["classes"][2]["mae"] == 1.5 and bd["classes"][2]["max"] == 3.0
    for k in (1, 3):                                                   # an empty class: NaN with 0 pixels, as by_area
        assert all(math.isnan(bd["classes"][k][key]) for key in ("mae", "rmse", "max"))
    worst = rep["holes"]["worst"]
    assert [h["label"] for h in worst] == [5, 40]
    assert worst[0]["depth_m"] == 10.0 and worst[1]["depth_m"] == float(np.float32(2.0 * math.sqrt(2.0)))
    for h, p in zip(worst, plain["holes"]["worst"]):
        assert {k: v for k, v in h.items() if k != "depth_m"} == p
    assert {k: v for k, v in rep.items() if k not in ("by_depth", "holes")} == {k: v for k, v in plain.items() if k != "holes"}
    from mvp_gan.src.evaluate_raster import summary
    assert summary(rep).startswith(summary(plain)) and "by depth" in summary(rep) and "by depth" not in summary(plain)
