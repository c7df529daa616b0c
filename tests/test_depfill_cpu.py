"""CPU checks of the depression fill (csrc/depfill.hip, mvp_gan/src/fill_depressions.py, the sink statistics of
mvp_gan/src/evaluate_raster.py): the two forms of the oracle in tests/depfill_oracle.py against each other and against the
defining properties, host-side rejection by the five C entry points, the ops and the Python API, the workspace query, the CLI
parsers and the sinks dict, all without a GPU."""
import ctypes as C
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import depfill_oracle as DO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def contract():
    """The oracle implements what include/terragan_hip.h states."""
    txt = " ".join(open(os.path.join(ROOT, "include", "terragan_hip.h")).read().replace("* ", "").split())
    for name in ("tg_depfill_ws_bytes", "tg_depfill_init", "tg_depfill_sweep", "tg_depfill_stats", "tg_depfill_finish"):
        assert name + "(" in txt, name
    assert "An outlet is a known pixel on the raster's edge or with an unknown conn-neighbour" in txt
    assert "min over conn-connected paths of known pixels from p to an outlet of the max of z along the path" in txt
    return txt


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rasters():
    """40 rasters up to 30x30: with and without voids, real and integer-rounded heights (plateaus and ties)."""
    rng = np.random.default_rng(42)
    out = []
    for i in range(40):
        H, W = (int(v) for v in rng.integers(1, 31, 2))
        z = (1000 + rng.normal(0, 3, (H, W))).astype(np.float32)
        if i % 2:
            z = np.rint(z)
        if i % 4 >= 2:
            z[rng.random((H, W)) < 0.05] = np.nan
        out.append(z)
    out.append((1000 + rng.normal(0, 3, (30, 30))).astype(np.float32))
    return out


def test_priority_flood_equals_relaxation_bitwise():
    n = 0
    for z in _rasters():
        known = DO.known_map(z)
        for conn in (8, 4):
            a = DO.priority_flood(z, known, conn)
            b, _ = DO.relax(z, known, conn)
            np.testing.assert_array_equal(_bits(a)[known], _bits(b)[known])
            assert np.isnan(a[~known]).all() and np.isnan(b[~known]).all()
            n += 1
    assert n >= 60


def test_oracle_properties():
    rng = np.random.default_rng(7)
    for z in _rasters()[::3]:
        known = DO.known_map(z)
        H, W = z.shape
        for conn in (8, 4):
            w = DO.priority_flood(z, known, conn)
            o = DO.outlets(known, conn)
            assert (w[known] >= z[known]).all() and not np.isinf(w[known]).any()
            np.testing.assert_array_equal(_bits(w)[o], _bits(z)[o])
            assert np.isin(_bits(w)[known], _bits(z)[known]).all()                   # every value is the bits of a known z
            again = DO.priority_flood(np.where(known, w, z), known, conn)
            np.testing.assert_array_equal(_bits(again)[known], _bits(w)[known])      # idempotent
            pad = np.full((H + 2, W + 2), np.inf, np.float32)
            pad[1:-1, 1:-1] = np.where(known, w, np.float32(np.inf))
            low = np.full((H, W), np.inf, np.float32)
            for dy, dx in DO.neighbours(conn):
                low = np.minimum(low, pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
            assert not (known & ~o & (w < low)).any()                                # no pit is left off the outlets
            up = np.where(known, z + rng.uniform(0, 2, z.shape).astype(np.float32), z)
            w2 = DO.priority_flood(up, known, conn)
            assert (w2[known] >= w[known]).all()                                     # monotone in z
            out, depth, flags = DO.finish(z, w, known)
            st = DO.stats(z, w, known)
            assert st["raised"] == int(flags.sum()) and st["unreached"] == 0 and st["counted"] == int(known.sum())
            assert st["depth_sum"] == pytest.approx(float(depth[known].astype(np.float64).sum()), rel=1e-6, abs=1e-9)
            np.testing.assert_array_equal(_bits(out)[known & (flags == 0)], _bits(z)[known & (flags == 0)])
    flat = np.full((7, 9), 1000.5, np.float32)
    np.testing.assert_array_equal(DO.priority_flood(flat, DO.known_map(flat)), flat)
    pit = np.array([[1003, 1002, 1004], [1001, 990, 1005], [1006, 1002.5, 1007]], np.float32)
    for conn in (8, 4):
        w = DO.priority_flood(pit, DO.known_map(pit), conn)
        assert w[1, 1] == 1001 and int((w != pit).sum()) == 1
    z = DO.gap_scene()
    w8, w4 = (DO.priority_flood(z, DO.known_map(z), c) for c in (8, 4))
    np.testing.assert_array_equal(w8, z)                                             # drains through the diagonal gap
    assert (w4[3:6, 3:6] == 1020).all() and int((w4 != z).sum()) == 9                # and not under 4
    st = DO.stats(z, w4, DO.known_map(z))
    assert (st["raised"], st["depth_sum"], st["max_depth"]) == (9, 270.0, 30.0) and DO.depressions(w4 > z) == 1
    sel = np.zeros(z.shape, np.uint8)
    sel[3, :] = 1
    assert DO.stats(z, w4, DO.known_map(z), sel)["raised"] == 3
    # a void inside is an outlet; the start of the relaxation and a stopped one
    z = DO.bowl(np.full((21, 21), 1000.0, np.float32), 10, 10, 6, 990.0, 0.5)
    assert DO.stats(z, DO.priority_flood(z, DO.known_map(z)), DO.known_map(z))["raised"] > 100
    z[10, 11] = np.nan
    known = DO.known_map(z)
    assert DO.stats(z, DO.priority_flood(z, known), known)["raised"] == 0
    w0 = DO.relax_start(z, known)
    assert np.isnan(w0[10, 11]) and w0[10, 10] == z[10, 10] and np.isinf(w0[5, 5]) and w0[0, 3] == z[0, 3]
    w1, steps = DO.relax(z, known, 8, max_steps=2)
    assert steps == 2 and np.isinf(w1[known]).any() and (w1[known] >= DO.priority_flood(z, known)[known]).all()
    out, depth, flags = DO.finish(z, w1, known)
    np.testing.assert_array_equal(np.isnan(out), ~known | np.isinf(w1))
    assert DO.stats(z, w1, known)["unreached"] == int(np.isinf(w1).sum())


def test_spiral_scene():
    z, channel = DO.spiral_scene()
    wall = z == 1100
    assert z.shape == (130, 130) and int(wall.sum()) + int(channel.sum()) == 128 * 128 and int(channel.sum()) == 12477
    from scipy import ndimage
    assert ndimage.label(wall)[1] == 1                                               # one 4-connected wall
    assert ndimage.label(channel, structure=np.ones((3, 3), int))[1] == 1            # one channel, even 8-connected
    assert z[channel].min() >= 990 and z[channel].max() < 1000 and z[4, 0] == 1040
    lanes = (wall[65, 1:65].astype(int)[1:] - wall[65, 1:65].astype(int)[:-1] == 1).sum()
    assert lanes >= 15                                                               # pitch 4: 16 turns of the wall


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

    init = lambda H, W, z=f[0], kn=f[1], conn=8, w=f[2], ws=f[3], nb=big: lib.tg_depfill_init(z, kn, H, W, conn, w, ws, nb, None)
    sweep = lambda H, W, z=f[0], kn=f[1], conn=8, n=1, w=f[2], ch=f[4], vis=f[5], ws=f[3], nb=big: \
        lib.tg_depfill_sweep(z, kn, H, W, conn, n, w, ch, vis, ws, nb, None)
    stats = lambda H, W, z=f[0], w=f[2], kn=f[1], sel=None, counts=f[6], sums=f[7], ws=f[3], nb=big: \
        lib.tg_depfill_stats(z, w, kn, sel, H, W, counts, sums, ws, nb, None)
    fin = lambda H, W, z=f[0], w=f[2], kn=f[1], out=f[8], depth=None, flags=None: \
        lib.tg_depfill_finish(z, w, kn, H, W, out, depth, flags, None)
    for H, W in ((0, 5), (5, 0), (-1, 5), (5, -1), (1 << 16, 1 << 15), (1 << 30, 2)):
        for call in (init, sweep, stats, fin):
            err(call(H, W), b"must be non-empty with H*W < 2^31")
        assert lib.tg_depfill_ws_bytes(H, W) == 0
    for kw in ({"z": None}, {"kn": None}, {"w": None}, {"ws": None}):
        err(init(8, 8, **kw), b"null pointer")
        err(sweep(8, 8, **kw), b"null pointer")
    for kw in ({"ch": None}, {"vis": None}):
        err(sweep(8, 8, **kw), b"null pointer")
    for conn in (0, 6, -8, 16):
        err(init(8, 8, conn=conn), b"connectivity")
        err(sweep(8, 8, conn=conn), b"connectivity")
    for n in (0, -1, (1 << 20) + 1):
        err(sweep(8, 8, n=n), b"sweeps")
    err(init(8, 8, w=f[0]), b"alias")
    err(sweep(8, 8, w=f[0]), b"alias")
    for H, W in ((8, 8), (129, 4097), (32767, 32767)):
        short = lib.tg_depfill_ws_bytes(H, W) - 1
        err(init(H, W, nb=short), b"workspace")
        err(sweep(H, W, nb=short), b"workspace")
        err(stats(H, W, nb=short), b"workspace")
    for kw in ({"z": None}, {"w": None}, {"kn": None}, {"counts": None}, {"sums": None}, {"ws": None}):
        err(stats(8, 8, **kw), b"null pointer")
    for kw in ({"z": None}, {"w": None}, {"kn": None}, {"out": None}):
        err(fin(8, 8, **kw), b"null pointer")
    for kw in ({"out": f[0]}, {"out": f[2]}, {"depth": f[0]}, {"depth": f[2]}):
        err(fin(8, 8, **kw), b"alias")


def test_ws_query_covers_the_layout_and_grows():
    """256 control bytes, two dirty planes of a byte per 64x64 tile, 40 bytes per workgroup of the statistics,
    min(1024, ceil(H W / 4096)) of them; each part rounded up to 256 bytes."""
    _, lib = _lib()
    up = lambda n: -(-n // 256) * 256
    shapes = [(1, 1), (1, 2049), (2049, 1), (63, 65), (64, 64), (65, 63), (257, 1101), (1501, 2099), (4097, 513), (8191, 8193),
              (32767, 3), (3, 32767), (32767, 32767), (46340, 46340), (1, (1 << 31) - 1)]
    for H, W in shapes:
        tiles = -(-H // 64) * -(-W // 64)
        nstat = min(1024, -(-H * W // 4096))
        assert lib.tg_depfill_ws_bytes(H, W) == 256 + 2 * up(tiles) + up(40 * nstat)
    for H, W in shapes[:-3]:
        for dh, dw in ((1, 0), (0, 1), (64, 0), (0, 255), (2, 2)):
            assert lib.tg_depfill_ws_bytes(H + dh, W + dw) >= lib.tg_depfill_ws_bytes(H, W)
    L, _ = _lib()
    P, I, SZ = C.c_void_p, C.c_int, C.c_size_t
    assert L.SIGNATURES["tg_depfill_ws_bytes"] == (SZ, [I, I])
    assert L.SIGNATURES["tg_depfill_init"] == (I, [P, P, I, I, I, P, P, SZ, P])
    assert L.SIGNATURES["tg_depfill_sweep"] == (I, [P, P, I, I, I, I, P, P, P, P, SZ, P])
    assert L.SIGNATURES["tg_depfill_stats"] == (I, [P, P, P, P, I, I, P, P, P, SZ, P])
    assert L.SIGNATURES["tg_depfill_finish"] == (I, [P, P, P, I, I, P, P, P, P])


def test_python_rejects_bad_arguments():
    from mvp_gan.src.evaluate_raster import evaluate_raster, sink_errors
    from mvp_gan.src.fill_depressions import fill_depressions
    z = np.zeros((8, 8), np.float32)
    with pytest.raises(ValueError, match="H, W"):
        fill_depressions(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError, match="H, W"):
        fill_depressions(np.zeros((0, 4), np.float32))
    with pytest.raises(ValueError, match="2\\^31"):
        fill_depressions(np.broadcast_to(np.float32(0), (1 << 16, 1 << 15)))
    with pytest.raises(ValueError, match="mask"):
        fill_depressions(z, np.ones((8, 9)))
    for c in (0.0, -1.0, math.nan, math.inf, None, "x"):
        with pytest.raises(ValueError, match="cellsize"):
            fill_depressions(z, cellsize=c)
    for conn in (0, 6, 16, "8", None, 8.5, True):
        with pytest.raises(ValueError, match="connectivity"):
            fill_depressions(z, connectivity=conn)
        with pytest.raises(ValueError, match="connectivity"):
            sink_errors(z, z, z, cellsize=1.0, connectivity=conn)
    for n in (0, -1, 1.5, "3", None, True, (1 << 20) + 1):
        with pytest.raises(ValueError, match="max_sweeps"):
            fill_depressions(z, max_sweeps=n)
        with pytest.raises(ValueError, match="check_every"):
            fill_depressions(z, check_every=n)
    with pytest.raises(ValueError, match="cellsize"):
        sink_errors(z, z, z, cellsize=0.0)
    with pytest.raises(ValueError, match="shape"):
        sink_errors(z, np.zeros((8, 9), np.float32), z, cellsize=1.0)
    with pytest.raises(ValueError, match="shape"):
        sink_errors(z, z, np.zeros((7, 8), np.uint8), cellsize=1.0)
    sig = inspect.signature(fill_depressions).parameters
    assert [(k, sig[k].default) for k in list(sig)[2:]] == [("nodata", None), ("cellsize", 1.0), ("connectivity", 8),
                                                            ("max_sweeps", 4096), ("check_every", 8), ("want_depth", False)]
    assert inspect.signature(evaluate_raster).parameters["sinks"].default is False
    sig = inspect.signature(sink_errors).parameters
    assert list(sig) == ["dem", "pred", "holes", "cellsize", "mask", "nodata", "connectivity"] and sig["connectivity"].default == 8


def test_no_cpu_path(monkeypatch):
    import torch
    from mvp_gan.src.evaluate_raster import sink_errors
    from mvp_gan.src.fill_depressions import fill_depressions
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    z = np.zeros((8, 8), np.float32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fill_depressions(z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sink_errors(z, z, z, cellsize=1.0)


def test_ops_reject_before_any_launch():
    import torch
    from tg_hip import lib as L
    from tg_hip import ops as O
    z, k = torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.uint8)
    ws = torch.zeros(4096, dtype=torch.uint8)
    ch, vis = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64)
    for call in (lambda: O.depfill_init(z, k, 8, ws), lambda: O.depfill_sweep(z, k, 8, 1, z.clone(), ch, vis, ws),
                 lambda: O.depfill_stats(z, z.clone(), k), lambda: O.depfill_finish(z, z.clone(), k),
                 lambda: O.depfill_init(np.zeros((4, 4), np.float32), k, 8, ws)):
        with pytest.raises(L.TgError):
            call()
    with pytest.raises(L.TgError, match="2\\^31"):
        O.depfill_ws(1 << 16, 1 << 15, "cpu")
    assert O.depfill_ws(130, 70, "cpu").numel() == _lib()[1].tg_depfill_ws_bytes(130, 70)


# ---- CLI parsers and the report ----------------------------------------------------------------------------------------------
def test_cli_parsers():
    from mvp_gan.src.evaluate_raster import build_parser as eval_parser
    from mvp_gan.src.fill_depressions import build_parser
    a = build_parser().parse_args(["--dem", "in.asc", "--out", "o.asc"])
    assert (a.dem, a.out, a.mask, a.nodata, a.connectivity, a.depth_out, a.max_sweeps) == \
        ("in.asc", "o.asc", None, None, 8, None, 4096)
    a = build_parser().parse_args(["--dem", "in.asc", "--out", "o.asc", "--mask", "m.png", "--nodata", "-9999", "--connectivity",
                                   "4", "--depth-out", "d.asc", "--max-sweeps", "17"])
    assert (a.mask, a.nodata, a.connectivity, a.depth_out, a.max_sweeps) == ("m.png", -9999.0, 4, "d.asc", 17)
    for bad in (["--dem", "in.asc"], ["--out", "o.asc"], ["--dem", "in.asc", "--out", "o.asc", "--connectivity", "6"],
                ["--dem", "in.asc", "--out", "o.asc", "--max-sweeps", "x"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(bad)
    for base in (["--dem", "in.asc", "--checkpoint", "g.pth"], ["--dem", "in.asc", "--pred", "p.asc", "--holes", "h.png"]):
        assert eval_parser().parse_args(base).sinks is False
        a = eval_parser().parse_args(base + ["--sinks", "--baseline", "laplace", "--compare", "idw"])
        assert a.sinks is True and a.baseline == "laplace" and a.compare == ["idw"]
        with pytest.raises(SystemExit):
            eval_parser().parse_args(base + ["--sinks", "yes"])
    cwd = os.path.join(ROOT, "terra-gan_amd")
    r = subprocess.run([sys.executable, "-m", "mvp_gan.src.fill_depressions", "--help"], cwd=cwd, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--dem", "--out", "--mask", "--nodata", "--connectivity", "--depth-out", "--max-sweeps"):
        assert flag in r.stdout


def test_sinks_dict_assembly():
    from mvp_gan.src.evaluate_raster import assemble_compare, assemble_sinks, sinks_summary
    from mvp_gan.src.fill_depressions import stats_dict
    truth = {"counts": [10, 0, 500], "sums": [12.5, 3.0], "depressions": 2, "converged": True, "cellsize": 2.0}
    pred = {"counts": [35, 0, 500], "sums": [40.25, 4.5], "depressions": 5, "converged": True, "cellsize": 2.0}
    s = assemble_sinks(truth, pred)
    assert list(s) == ["truth", "pred", "excess_volume_m3", "excess_cells"]
    assert s["truth"] == {"cells": 10, "volume_m3": 50.0, "max_depth_m": 3.0, "depressions": 2, "converged": True}
    assert s["pred"] == {"cells": 35, "volume_m3": 161.0, "max_depth_m": 4.5, "depressions": 5, "converged": True}
    assert s["excess_volume_m3"] == 111.0 and s["excess_cells"] == 25
    same = assemble_sinks(truth, truth)
    assert same["excess_volume_m3"] == 0.0 and same["excess_cells"] == 0 and same["truth"] == same["pred"]
    assert assemble_sinks(pred, truth)["excess_cells"] == -25
    line = sinks_summary(s)
    assert "35 px" in line and "161 m3" in line and "5 pits" in line and "excess 111 m3" in line
    assert stats_dict([3, 1, 9], [2.5, 1.5], 0.5) == {"cells": 3, "unreached": 1, "counted": 9, "depth_sum_m": 2.5,
                                                      "volume_m3": 0.625, "max_depth_m": 1.5}
    # the report assembly without sinks has no "sinks" key; with it, one per fill
    raw = {"idw": {"height": {"rmse": 1.0}}, "nearest": {"height": {"rmse": 2.0}}}
    infos = {"idw": {"method": "idw"}, "nearest": {"method": "nearest"}}
    cmp = assemble_compare(raw, infos)
    assert all("sinks" not in cmp[k] and set(cmp[k]) == {"height", "method", "fill"} for k in cmp)
    cmp = assemble_compare(raw, infos, {"idw": s, "nearest": same})
    assert cmp["idw"]["sinks"] is s and cmp["nearest"]["sinks"] is same and "sinks" not in raw["idw"]
