"""CPU-only checks of the kriging tools (mvp_gan/src/kriging.py, csrc/kriging.hip): the oracle against
itself (the bordered system against the reduced Cholesky form the kernel uses, and the closed forms for one and two samples),
fit_variogram, the variogram's pair counts in closed form, and the interface: what is refused before any launch, the exports, the
workspace query, the defaults."""
import ctypes as C
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import kriging_oracle as KO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _models():
    from mvp_gan.src.kriging import Variogram
    return [Variogram("power", 0.0, 0.02, 1.5), Variogram("power", 0.01, 0.02, 1.0), Variogram("power", 0.0, 0.02, 1.9),
            Variogram("exponential", 0.0, 4.0, 30.0), Variogram("spherical", 0.05, 4.0, 25.0),
            Variogram("spherical", 0.0, 4.0, 5.0)]


def _config(rng, n, reach=40):
    """n samples, one per ray, at random distances; the heights near 1000 m."""
    rays = rng.permutation(8)[:n]
    k = rng.integers(1, reach, n)
    off = np.array(KO.DIRS, np.int64)[rays] * k[:, None]
    return off, 1000.0 + rng.normal(0, 3.0, n)


# ---- the oracle against itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mi", range(6))
def test_bordered_system_agrees_with_the_reduced_cholesky_form(mi):
    vg = _models()[mi]
    rng = np.random.default_rng(100 + mi)
    for t in range(160):
        n = 1 + t % 8
        off, zs = _config(rng, n)
        c = (0.5, 2.5)[t % 2]
        s = KO.bordered(off[None], zs[None], vg, c)
        est, var, w = KO.reduced(off, zs, vg, c)
        assert abs(est - s["est"][0]) <= 1e-10, (n, est, s["est"][0])
        assert abs(var - s["var"][0]) <= 1e-10 * max(1.0, s["var"][0]), (n, var, s["var"][0])
        np.testing.assert_allclose(w, s["w"][0], rtol=0, atol=1e-10)
        assert abs(s["w"][0].sum() - 1.0) <= 1e-12 and var >= 0
        # a constant added to the heights moves the estimate by it and leaves the variance alone
        s2 = KO.bordered(off[None], zs[None] + 250.0, vg, c)
        assert abs(s2["est"][0] - s["est"][0] - 250.0) <= 1e-9 and s2["var"][0] == s["var"][0]
        assert KO.reduced(off, np.full(n, 1234.5), vg, c)[0] == 1234.5      # the residual form: exactly constant


@pytest.mark.parametrize("mi", range(6))
def test_one_and_two_samples_in_closed_form(mi):
    vg = _models()[mi]
    for c in (0.5, 2.5):
        for k in (1, 3, 17):
            for ray in range(8):
                off = np.array(KO.DIRS, np.int64)[[ray]] * k
                h = c * math.sqrt(k * k * KO.SCALE[ray])
                s = KO.bordered(off[None], np.array([[1003.25]]), vg, c)
                assert s["est"][0] == 1003.25 and abs(s["var"][0] - 2 * float(vg.gamma(h))) <= 1e-12 * s["var"][0]
                assert KO.reduced(off, np.array([1003.25]), vg, c)[:2] == (1003.25, 2 * float(vg.gamma(h)))
        for a, b in ((1, 1), (2, 7), (30, 4)):
            off = np.array([[0, a], [0, -b]], np.int64)                   # E and W: opposite rays
            s = KO.bordered(off[None], np.array([[1000.0, 1002.0]]), vg, c)
            g = lambda d: float(vg.gamma(c * d))
            w1 = 0.5 + (g(b) - g(a)) / (2 * g(a + b))
            assert abs(s["w"][0][0] - w1) <= 1e-12 and abs(s["w"][0].sum() - 1) <= 1e-14


def test_gamma_definition():
    from mvp_gan.src.kriging import Variogram
    h = np.array([0.0, 0.5, 5.0, 25.0, 80.0])
    p, e, s = Variogram("power", 0.01, 0.02, 1.5), Variogram("exponential", 0.0, 4.0, 30.0), Variogram("spherical", 0.05, 4.0, 25.0)
    np.testing.assert_array_equal(p.gamma(h)[1:], 0.01 + 0.02 * np.exp2(1.5 * np.log2(h[1:])))    # h^shape as the kernel takes it
    np.testing.assert_allclose(p.gamma(h)[1:], 0.01 + 0.02 * h[1:] ** 1.5, rtol=1e-14)
    np.testing.assert_array_equal(e.gamma(h)[1:], 4.0 * (1.0 - np.exp(-h[1:] / 30.0)))
    r = np.minimum(h[1:] / 25.0, 1.0)
    np.testing.assert_array_equal(s.gamma(h)[1:], 0.05 + 4.0 * (1.5 * r - 0.5 * (r * r * r)))
    assert p.gamma(h)[0] == e.gamma(h)[0] == s.gamma(h)[0] == 0.0 and s.gamma(h)[-1] == s.gamma(h)[-2] == 4.05
    assert p.gamma(h).dtype == np.float64 and float(p.gamma(4.0)) == 0.01 + 0.02 * 8.0


# ---- fit_variogram ------------------------------------------------------------------------------------------------------------
def _table(gamma, pairs=1000, cellsize=2.0, octaves=6):
    from mvp_gan.src.kriging import variogram_scales
    lags = np.array([m for _, _, m in variogram_scales(octaves, cellsize)])
    return {"lags_m": lags, "gamma": np.array([gamma(h) for h in lags]), "pairs": np.full(len(lags), pairs)}


def test_fit_recovers_a_power_law():
    from mvp_gan.src.kriging import Variogram, fit_variogram
    for scale, shape in ((0.02, 1.5), (3.0, 0.4), (1e-4, 1.9)):
        emp = _table(lambda h: scale * h ** shape)
        emp["pairs"] = np.arange(1, 13) * 100                             # any weights: the table is exact
        vg, rms = fit_variogram(emp)
        assert isinstance(vg, Variogram) and vg.model == "power" and vg.nugget == 0.0
        assert abs(vg.scale / scale - 1) <= 1e-12 and abs(vg.shape - shape) <= 1e-12 and rms <= 1e-12
    # lists, and scales below min_pairs or without a value are left out
    emp = _table(lambda h: 0.5 * h ** 1.0)
    emp = {k: v.tolist() for k, v in emp.items()}
    emp["gamma"][3], emp["pairs"][3] = 77.0, 29
    emp["gamma"][5] = float("nan")
    emp["gamma"][7] = 0.0
    vg, rms = fit_variogram(emp)
    assert abs(vg.scale - 0.5) <= 1e-12 and abs(vg.shape - 1.0) <= 1e-12
    assert fit_variogram(emp, min_pairs=29)[1] > 0.1


def test_fit_clips_a_plane_and_raises_on_too_few_scales():
    from mvp_gan.src.kriging import fit_variogram
    vg, rms = fit_variogram(_table(lambda h: 0.125 * h * h))              # a plane: gamma = g^2 h^2 / 2, slope 2
    assert vg.shape == 1.95 and rms > 0 and vg.scale > 0
    vg, _ = fit_variogram(_table(lambda h: 3.0))                          # pure nugget: slope 0
    assert vg.shape == 0.05
    one = _table(lambda h: 0.02 * h ** 1.5)
    one["pairs"] = np.array([1000] + [29] * 11)
    for emp in (one, _table(lambda h: 0.0), _table(lambda h: float("nan")), _table(lambda h: 1.0, octaves=1, pairs=3)):
        with pytest.raises(ValueError, match="pass a Variogram"):
            fit_variogram(emp)


# ---- pair counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 300), (300, 1), (33, 65), (130, 67), (32, 33)])
def test_pair_counts_in_closed_form(H, W):
    z = np.zeros((H, W), np.float32)
    pairs, sums = KO.variogram(z, np.ones((H, W), np.uint8))
    np.testing.assert_array_equal(pairs, KO.pair_counts_full(H, W))
    assert (sums == 0).all()
    for j in range(6):
        L = 1 << j
        assert pairs[2 * j] == H * max(W - L, 0) + max(H - L, 0) * W
        assert pairs[2 * j + 1] == 2 * max(H - L, 0) * max(W - L, 0)


def test_oracle_variogram_of_a_plane_and_assembly():
    from mvp_gan.src.kriging import assemble_variogram, fit_variogram
    y, x = np.mgrid[0:40, 0:50]
    z = (1000 + 0.5 * x + 0.25 * y).astype(np.float32)
    pairs, sums = KO.variogram(z, np.ones(z.shape, np.uint8))
    emp = assemble_variogram(pairs, sums, cellsize=2.0, octaves=6)
    assert emp["lags_m"][0] == 2.0 and emp["lags_m"][1] == 2.0 * math.sqrt(2.0) and emp["lags_m"][10] == 64.0
    assert emp["lag_px"] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32] and emp["class"][:2] == ["axial", "diagonal"]
    want0 = (0.25 * 40 * 49 + 0.0625 * 39 * 50) / (2 * (40 * 49 + 39 * 50))
    assert emp["gamma"][0] == want0 and list(emp["pairs"]) == list(pairs)
    assert fit_variogram(emp)[0].shape == 1.95
    none = assemble_variogram(np.zeros(12, np.int64), np.zeros(12), cellsize=1.0, octaves=6)
    assert np.isnan(none["gamma"]).all()
    assert len(assemble_variogram(pairs, sums, cellsize=1.0, octaves=2)["gamma"]) == 4


# ---- the interface ------------------------------------------------------------------------------------------------------------
def test_variogram_rejects_what_the_kernel_rejects():
    from mvp_gan.src.kriging import MODELS, Variogram
    assert MODELS == ("power", "exponential", "spherical")
    v = Variogram()
    assert (v.model, v.nugget, v.scale, v.shape) == ("power", 0.0, 1.0, 1.0)
    with pytest.raises(Exception):
        v.scale = 2.0                                                     # frozen
    for kw in ({"model": "gaussian"}, {"nugget": -1e-9}, {"nugget": math.inf}, {"nugget": math.nan}, {"scale": 0.0},
               {"scale": -1.0}, {"scale": math.inf}, {"shape": 0.0}, {"shape": 2.0}, {"shape": 2.5}, {"shape": math.nan},
               {"model": "spherical", "shape": 0.0}, {"model": "exponential", "shape": math.inf}, {"scale": "1"},
               {"nugget": True}):
        with pytest.raises(ValueError, match="Variogram"):
            Variogram(**kw)
    assert Variogram("spherical", 0, 4, 25).shape == 25.0 and Variogram("power", shape=1.999).shape == 1.999


def test_krige_voids_and_evaluate_raster_reject_before_any_launch():
    from mvp_gan.src.evaluate_raster import evaluate_raster
    from mvp_gan.src.kriging import Variogram, empirical_variogram, krige_voids
    z = np.zeros((8, 8), np.float32)
    for kw, msg in (({"variogram": "power"}, "Variogram"), ({"variogram": (0, 1, 1)}, "Variogram"), ({"cellsize": 0}, "cellsize"),
                    ({"max_distance": -1.0}, "max_distance"), ({"max_distance": 0.5, "cellsize": 1.0}, "shorter than one cell"),
                    ({"fallback": "idw"}, "fallback"), ({"mask": np.ones((8, 9))}, "mask")):
        with pytest.raises(ValueError, match=msg):
            krige_voids(z, **kw)
    with pytest.raises(ValueError, match="krige_voids"):
        krige_voids(np.zeros((2, 3, 4), np.float32))
    for bad in (0, 7, 2.0, True):
        with pytest.raises(ValueError, match="octaves"):
            empirical_variogram(z, octaves=bad)
    for bad in ("power", 1, 0.5, {"model": "power"}):
        with pytest.raises(ValueError, match="kriging"):
            evaluate_raster(None, z, cellsize=1.0, kriging=bad)
    sig = inspect.signature(evaluate_raster).parameters
    assert sig["kriging"].default is False and sig["compare"].default is None
    sig = inspect.signature(krige_voids).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("mask", None), ("nodata", None), ("cellsize", 1.0),
                                                            ("variogram", None), ("max_distance", None),
                                                            ("fallback", "nearest")]
    assert inspect.signature(empirical_variogram).parameters["octaves"].default == 6
    assert isinstance(Variogram(), Variogram)


def test_methods_and_compares_are_untouched():
    from mvp_gan.src import evaluate_raster as ER
    from mvp_gan.src.interpolate import METHODS
    assert METHODS == ER.COMPARES == ("idw", "nearest")
    assert list(inspect.signature(ER.assemble_compare).parameters)[-1] == "texture"
    assert "kriging" in inspect.signature(ER._evaluate).parameters and callable(ER.kriging_report)
    assert "variogram" in inspect.signature(ER.kriging_report).parameters


def test_no_cpu_path(monkeypatch):
    import torch
    from mvp_gan.src.kriging import empirical_variogram, krige_voids
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    z = np.zeros((8, 8), np.float32)
    for fn in (krige_voids, empirical_variogram):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(z)


def test_calibration_assembly():
    from mvp_gan.src.evaluate_raster import assemble_calibration, calibration_summary
    c = assemble_calibration(200, 260.0, 130, 188)
    assert c == {"cells": 200, "mean_z2": 1.3, "within_1sigma": 0.65, "within_2sigma": 0.94}
    assert "0.650 within 1 sigma" in calibration_summary(c)
    c = assemble_calibration(0, 0.0, 0, 0)
    assert c == {"cells": 0, "mean_z2": None, "within_1sigma": None, "within_2sigma": None} and "n/a" in calibration_summary(c)


def test_exports_and_workspace_query():
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    from tg_hip import ops as O
    lib = L.load()
    for s in ("tg_variogram_ws_bytes", "tg_variogram", "tg_krige"):
        assert hasattr(lib, s) and s in L.SIGNATURES
    assert (L.TG_VGM_OCTAVES, L.TG_VGM_SCALES) == (O.VGM_OCTAVES, O.VGM_SCALES) == (6, 12)
    assert O.VGM_MODELS == ("power", "exponential", "spherical")
    hdr = open(os.path.join(ROOT, "include", "terragan_hip.h")).read()
    assert "#define TG_VGM_OCTAVES 6" in hdr and "#define TG_VGM_SCALES 12" in hdr
    q = lib.tg_variogram_ws_bytes
    assert q(0, 5) == q(5, 0) == q(-1, 5) == q(65536, 32768) == 0
    sizes = [q(n, n) for n in (1, 31, 32, 33, 64, 65, 500, 1000, 2000, 4096, 8192, 30000)]
    assert sizes[0] == 12 * 8 and sizes == sorted(sizes) and sizes[-1] == sizes[-2] == 2048 * 12 * 8
    assert all(q(h, w) <= q(h + 7, w) and q(h, w) <= q(h, w + 13) for h in (1, 40, 700) for w in (1, 90, 3000))


def test_c_side_rejects_before_any_launch():
    from tg_hip import lib as L
    lib = L.load()
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(C.addressof(buf) + 1024)
    r = C.c_void_p(C.addressof(buf) + 2048)
    ok = dict(cellsize=1.0, model=0, nugget=0.0, scale=1.0, shape=1.0)

    def krige(H=4, W=4, z=p, out=q, var=r, d2=None, idx=None, **kw):
        a = dict(ok, **kw)
        return lib.tg_krige(z, p, p, H, W, a["cellsize"], a["model"], a["nugget"], a["scale"], a["shape"], d2, idx, out, var, p,
                            None)
    for kw, msg in ((dict(H=0), b"sides"), (dict(W=32768), b"sides"), (dict(z=None), b"null pointer"), (dict(var=None), b"null"),
                    (dict(d2=p), b"go together"), (dict(idx=p), b"go together"), (dict(out=p), b"distinct"),
                    (dict(var=q), b"distinct"), (dict(cellsize=0.0), b"cellsize"), (dict(cellsize=math.nan), b"cellsize"),
                    (dict(model=3), b"model"), (dict(model=-1), b"model"), (dict(nugget=-0.5), b"nugget"),
                    (dict(nugget=math.inf), b"nugget"), (dict(scale=0.0), b"scale"), (dict(scale=math.nan), b"scale"),
                    (dict(shape=2.0), b"shape"), (dict(shape=0.0), b"shape"), (dict(shape=math.nan), b"shape"),
                    (dict(model=1, shape=0.0), b"shape"), (dict(model=2, shape=math.inf), b"shape")):
        assert krige(**kw) == -1 and msg in lib.tg_last_error(), (kw, lib.tg_last_error())
    vg = lambda H=4, W=4, z=p, octaves=6, ws=p, nb=1 << 20: lib.tg_variogram(z, p, H, W, octaves, p, p, ws, nb, None)
    for kw, msg in ((dict(H=0), b"non-empty"), (dict(z=None), b"null pointer z"), (dict(ws=None), b"null pointer ws"),
                    (dict(octaves=0), b"octaves"), (dict(octaves=7), b"octaves"), (dict(nb=95), b"workspace")):
        assert vg(**kw) == -1 and msg in lib.tg_last_error(), (kw, lib.tg_last_error())


def test_ops_reject_before_any_launch():
    import torch
    from tg_hip import lib as L
    from tg_hip import ops as O
    z, k = torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="variogram"):
        O.variogram(z, k)                                                 # not on the device
    with pytest.raises(ValueError, match="variogram"):
        O.variogram(np.zeros((4, 4), np.float32), k)
    with pytest.raises(L.TgError):
        O.krige(z, k, torch.zeros(8, 4, 4, dtype=torch.uint16), 1.0, "power", 0.0, 1.0, 1.0)


def test_cli_parsers():
    from mvp_gan.src.evaluate_raster import build_parser as eval_parser
    from mvp_gan.src.kriging import build_parser
    a = build_parser().parse_args(["--dem", "in.asc", "--out", "o.asc"])
    assert (a.dem, a.out, a.mask, a.nodata, a.model, a.nugget, a.scale, a.shape, a.max_distance, a.no_fallback, a.variance_out,
            a.variogram_json) == ("in.asc", "o.asc", None, None, "power", None, None, None, None, False, None, None)
    a = build_parser().parse_args(["--dem", "in.asc", "--out", "o.asc", "--variance-out", "v.asc", "--model", "spherical", "--nugget",
                                   "0.05", "--scale", "4", "--shape", "25", "--max-distance", "50", "--no-fallback",
                                   "--variogram-json", "v.json", "--mask", "m.png", "--nodata", "-9999"])
    assert (a.model, a.nugget, a.scale, a.shape, a.max_distance, a.no_fallback, a.variance_out, a.variogram_json) == \
        ("spherical", 0.05, 4.0, 25.0, 50.0, True, "v.asc", "v.json")
    for bad in (["--dem", "in.asc"], ["--dem", "in.asc", "--out", "o.asc", "--model", "gaussian"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(bad)
    for base in (["--dem", "in.asc", "--checkpoint", "g.pth"], ["--dem", "in.asc", "--pred", "p.asc", "--holes", "h.png"]):
        assert eval_parser().parse_args(base).kriging is False
        assert eval_parser().parse_args(base + ["--kriging"]).kriging is True
    r = subprocess.run([sys.executable, "-m", "mvp_gan.src.kriging", "--help"], cwd=os.path.join(ROOT, "terra-gan_amd"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--dem", "--out", "--variance-out", "--mask", "--nodata", "--model", "--nugget", "--scale", "--shape",
                 "--max-distance", "--no-fallback", "--variogram-json"):
        assert flag in r.stdout
