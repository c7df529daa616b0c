"""CPU-only checks of the conditional simulation (mvp_gan/src/simulate.py, csrc/simulate.hip): the cosine
polynomial of the mirror against numpy over every reduced argument, the wave table, the statistics of the mirror's fields against
the figures recorded in tests/golden/simulate_stats.json (`python -m tests.simulate_cases` writes it), and the interface: what is
refused before any launch, the exports, the defaults.  None of the figures involves the kernel: tests/test_hip_simulate.py holds the
kernel to the mirror bit for bit."""
import ctypes as C
import inspect
import json
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from tests import simulate_cases as SC
from tests import simulate_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(SC.GOLDEN) as f:
        return json.load(f)


# ---- the cosine polynomial ----------------------------------------------------------------------------------------------------
def test_cosine_polynomial_over_every_reduced_argument(golden):
    """All 4 * 2^24 (quadrant, fraction) pairs against np.cos in float64 at the same angle.  The recorded figure is this
    measurement; the margin of one float32 ulp of 1 covers the rounding of the recorded number and nothing else."""
    err = SC.cosine_max_error()
    print("cosine max abs error", err, "recorded", golden["cosine_max_abs_error"])
    assert err <= golden["cosine_max_abs_error"] + 2.0 ** -23


def test_cosine_polynomial_at_the_quadrant_ends_and_coefficients():
    q = np.arange(4, dtype=np.uint32)
    c = SO.cos_reduced(q, np.zeros(4, np.uint32))                         # 0, 1/4, 1/2, 3/4 turn
    assert c.dtype == np.float32 and c[0] == 1.0 and c[2] == -1.0 and abs(c[1]) <= 2.0 ** -22 and c[3] == -c[1]
    assert SO.cos_phase(np.array([0], np.uint32))[0] == 1.0 and SO.cos_phase(np.array([1 << 31], np.uint32))[0] == -1.0
    # the low six bits of the phase are truncated
    assert SO.cos_phase(np.array([12345 << 6], np.uint32))[0] == SO.cos_phase(np.array([(12345 << 6) + 63], np.uint32))[0]
    want = [(-1) ** j * (math.pi / 2) ** (2 * j) / math.factorial(2 * j) for j in range(8)]
    assert [float(c) for c in SO.COEF] == [float(np.float32(w)) for w in want]
    src = open(os.path.join(ROOT, "terra-gan_amd", "csrc", "simulate.hip")).read()
    for h in ("0x1.3bd3ccp+0f", "0x1.03c1f0p-2f", "0x1.55d3c8p-6f", "0x1.e1f506p-11f", "0x1.a6d1f2p-16f", "0x1.f9d38ap-22f",
              "0x1.b6e250p-28f", "0x7feb352du", "0x846ca68bu", "0x9e3779b9u", "393210"):
        assert h in src, h
    assert "#pragma clang fp contract(off)" in src


def test_mirror_hash_and_nugget_term():
    assert SO.mix(np.array([0], np.uint32))[0] == 0 and SO.mix(np.array([1], np.uint32))[0] != 1
    v = SO.mix(np.arange(1 << 16, dtype=np.uint32))
    assert len(np.unique(v)) == 1 << 16                                   # the mix is a bijection
    g = SO.nugget_term(64, 96, (5, 7), 3, 1)
    assert abs(g.mean()) < 0.06 and abs(g.var() - 1.0) < 0.06             # 6144 draws of a unit-variance sum: sd 0.013 and 0.018
    assert np.array_equal(g[10:20, 30:40], SO.nugget_term(10, 10, (15, 37), 3, 1))
    assert not np.array_equal(g, SO.nugget_term(64, 96, (5, 7), 3, 2)) and not np.array_equal(g, SO.nugget_term(64, 96, (5, 7), 4, 1))
    assert np.array_equal(g * 2.0 ** 16, np.rint(g * 2.0 ** 16)) and np.abs(g).max() < 6.0


# ---- the wave table -----------------------------------------------------------------------------------------------------------
def test_spectral_waves_table():
    from mvp_gan.src import simulate as S
    from mvp_gan.src.kriging import Variogram
    vg = Variogram("power", 0.0, 0.05, 1.2)
    a, b = S.spectral_waves(vg, 2.0, 256, 7), S.spectral_waves(vg, 2.0, 256, 7)
    assert a.dtype == S.WAVE_DTYPE and a.dtype.itemsize == 16 and a.shape == (256,) and a.tobytes() == b.tobytes()
    assert S.spectral_waves(vg, 2.0, 256, 8).tobytes() != a.tobytes()     # another rotation
    ratio = S.spectral_waves(vg, 2.0, 256, 8)["amp"] / a["amp"]           # the spectrum's shape stays; the fitted factor moves a little
    np.testing.assert_allclose(ratio, ratio[0], rtol=1e-6)
    assert abs(ratio[0] - 1.0) < 0.05
    for t in (a, S.spectral_waves(Variogram("exponential", 0.1, 4.0, 30.0), 0.5, 512, 1), S.spectral_waves(vg, 1.0, 1, 0)):
        f = np.stack([t["fx"], t["fy"]]).astype(np.float64) / 2.0 ** 32
        assert np.abs(f).max() <= 0.5 and (t["phase"] == 0).all() and np.isfinite(t["amp"]).all() and (t["amp"] > 0).all()
    zero = S.spectral_waves(SimpleNamespace(model="power", nugget=0.0, scale=0.0, shape=1.2), 2.0, 64, 0)
    assert (zero["amp"] == 0).all() and np.array_equal(zero["fx"], S.spectral_waves(vg, 2.0, 64, 0)["fx"])
    # the amplitudes scale with the root of the model's scale and the table does not know the raster
    c = S.spectral_waves(Variogram("power", 0.0, 0.2, 1.2), 2.0, 256, 7)
    np.testing.assert_allclose(c["amp"], 2.0 * a["amp"], rtol=1e-6)
    assert list(inspect.signature(S.spectral_waves).parameters) == ["variogram", "cellsize", "waves", "seed", "outer_px"]
    with pytest.raises(ValueError, match="spherical"):
        S.spectral_waves(Variogram("spherical", 0.0, 4.0, 25.0), 1.0)
    for kw, msg in ((dict(waves=0), "waves"), (dict(waves=513), "waves"), (dict(waves=2.0), "waves"), (dict(seed=-1), "seed"),
                    (dict(seed=True), "seed"), (dict(outer_px=2), "outer_px"), (dict(cellsize=0.0), "cellsize")):
        with pytest.raises(ValueError, match=msg):
            S.spectral_waves(vg, **{"cellsize": 1.0, **kw})
    # phases: per (seed, realisation), not per count
    p = S.realisation_phases(3, 5, 256)
    assert p.dtype == np.uint32 and np.array_equal(p, S.realisation_phases(3, 5, 256))
    assert not np.array_equal(p, S.realisation_phases(3, 6, 256)) and not np.array_equal(p, S.realisation_phases(4, 5, 256))
    w = S.with_phases(a, 3, 5)
    assert np.array_equal(w["phase"], p) and np.array_equal(w["fx"], a["fx"]) and (a["phase"] == 0).all()


def test_realised_variogram_closed_form():
    from mvp_gan.src import simulate as S
    t = np.zeros(2, S.WAVE_DTYPE)
    t["fx"], t["fy"], t["amp"] = [1 << 30, 0], [0, 1 << 29], [2.0, 3.0]     # 1/4 turn per px along x, 1/8 along y
    lags = [(0, 0), (0, 1), (0, 2), (1, 0), (4, 4), (0, 4)]
    want = [0.0, 2.0 * (1 - 0.0) + 0.5, 2.0 * 2 + 0.5, 4.5 * (1 - math.sqrt(0.5)) + 0.5, 4.5 * 2 + 0.5, 0.5]
    np.testing.assert_allclose(S.realised_variogram(t, 0.5, lags), want, rtol=0, atol=1e-12)
    v = S.lag_vectors()
    assert v.shape == (128, 2) and v[:4].tolist() == [[0, 1], [1, 0], [1, 1], [1, -1]] and v[-1].tolist() == [32, -32]


@pytest.mark.parametrize("waves", SC.WAVES)
@pytest.mark.parametrize("name", list(SC.MODELS))
def test_realised_variogram_against_the_model(golden, name, waves):
    """The closed-form variogram of the table against Variogram.gamma at the 64 lags (1 .. 32 px, axial and diagonal), the
    largest relative error over 8 rotations; recorded per case, asserted at the recorded figure x 1.25."""
    rec = golden["table_rel_error"][f"{name}/{waves}"]
    errs = [SC.table_error(SC.MODELS[name], waves, s) for s in range(SC.ROTATIONS)]
    print(name, waves, "relative error per rotation", errs, "recorded", rec)
    assert max(errs) <= rec * 1.25


def test_mirror_field_has_the_realised_variogram(golden):
    """256 x 256 mirror fields, 16 seeds: the empirical variogram against the closed form.  About the mirror, not the kernel."""
    err = SC.field_error()
    print("field relative error", err, "recorded", golden["field_rel_error"])
    assert err <= golden["field_rel_error"] * 1.25


def test_conditional_spread_of_the_mirror(golden):
    """64 realisations of a 96 x 96 scene at 20 % known, 4 seeds: the mean over the void pixels of d^2 / sigma^2_krige."""
    r = SC.spread_ratios()
    print("spread ratios", r, "recorded", golden["spread_ratio_mean"], "+-", golden["spread_ratio_spread"])
    assert abs(float(np.mean(r)) - golden["spread_ratio_mean"]) <= 2.0 * golden["spread_ratio_spread"]


def test_golden_records_every_case(golden):
    assert sorted(golden["table_rel_error"]) == sorted(f"{n}/{w}" for n in SC.MODELS for w in SC.WAVES)
    assert [tuple(v[:1]) + tuple(v[3:]) for v in SC.MODELS.values()] == [("power", 0.5), ("power", 1.0), ("power", 1.5), ("power", 1.9),
                                                                         ("exponential", 8.0), ("exponential", 40.0)]
    assert (SC.SPREAD["side"], SC.SPREAD["known"], SC.SPREAD["realisations"], SC.SPREAD["seeds"]) == (96, 0.2, 64, 4)
    assert (SC.FIELD_SIDE, SC.FIELD_SEEDS, SC.ROTATIONS, SC.WAVES) == (256, 16, 8, (64, 256, 512))
    assert 0 < golden["cosine_max_abs_error"] < 2.0 ** -21 and len(golden["spread_ratios"]) == 4


# ---- the mirror's combine and statistics --------------------------------------------------------------------------------------
def test_mirror_combine_and_stats():
    rng = np.random.default_rng(0)
    z = (500 + rng.normal(0, 5, (6, 7))).astype(np.float32)
    kn = rng.random((6, 7)) < 0.4
    zk = np.where(kn, z, z + 1).astype(np.float32)
    zk[0, 0], kn[0, 0] = np.nan, False
    s1, s2 = np.zeros((6, 7)), np.zeros((6, 7))
    ds = []
    for r in range(5):
        u, uk = rng.normal(0, 1, (6, 7)).astype(np.float32), rng.normal(0, 1, (6, 7)).astype(np.float32)
        uk[0, 0] = np.nan
        out = SO.combine(z, kn, zk, u, uk, s1, s2)
        assert np.array_equal(out[kn], z[kn]) and np.isnan(out[0, 0])
        want = (zk.astype(np.float64) + (u.astype(np.float64) - uk.astype(np.float64))).astype(np.float32)
        assert np.array_equal(out[~kn][1:], want[~kn][1:]) and np.abs(out - (zk + (u - uk)))[~kn][1:].max() <= 2.0 ** -14
        ds.append(u.astype(np.float64) - uk.astype(np.float64))
    mean, sd, _ = SO.stats(zk, s1, s2, 5)
    assert (sd[kn] == 0).all() and np.isnan(sd[0, 0]) and np.isnan(mean[0, 0]) and np.array_equal(mean[kn], z[kn])
    d = np.stack(ds)
    v = ~kn
    v[0, 0] = False
    np.testing.assert_allclose(sd[v], d.std(0, ddof=1)[v], rtol=1e-6)
    np.testing.assert_allclose(mean[v], (zk + d.mean(0))[v], rtol=1e-6)


# ---- refusals, exports, defaults ----------------------------------------------------------------------------------------------
def test_simulate_voids_and_evaluate_raster_reject_before_any_launch():
    from mvp_gan.src.evaluate_raster import _check_simulate, evaluate_raster, simulation_report
    from mvp_gan.src.kriging import Variogram
    from mvp_gan.src.simulate import simulate_voids
    z = np.zeros((8, 8), np.float32)
    for kw, msg in (({"variogram": "power"}, "Variogram"), ({"cellsize": 0}, "cellsize"), ({"max_distance": -1.0}, "max_distance"),
                    ({"fallback": "idw"}, "fallback"), ({"mask": np.ones((8, 9))}, "mask"), ({"realisations": 0}, "realisations"),
                    ({"realisations": 2.0}, "realisations"), ({"realisations": True}, "realisations"), ({"seed": -1}, "seed"),
                    ({"seed": 2 ** 32}, "seed"), ({"waves": 0}, "waves"), ({"waves": 513}, "waves"), ({"origin": 3}, "origin"),
                    ({"origin": (0, -1)}, "origin"), ({"origin": (2 ** 32, 0)}, "origin"),
                    ({"variogram": Variogram("spherical", 0.0, 4.0, 25.0)}, "spherical"), ({"table": np.zeros(4)}, "table")):
        with pytest.raises(ValueError, match=msg):
            simulate_voids(z, **kw)
    with pytest.raises(ValueError, match="simulate_voids"):
        simulate_voids(np.zeros((2, 3, 4), np.float32))
    for bad in (1, -1, 2.0, True, "4", 4097):
        with pytest.raises(ValueError, match="simulate"):
            evaluate_raster(None, z, cellsize=1.0, simulate=bad)
    assert _check_simulate(0) == _check_simulate(None) == _check_simulate(False) == 0 and _check_simulate(4) == 4
    with pytest.raises(ValueError, match="spherical"):
        evaluate_raster(None, z, cellsize=1.0, simulate=4, kriging=Variogram("spherical", 0.0, 4.0, 25.0))
    with pytest.raises(ValueError, match="realisations"):
        simulation_report(z, z, z, cellsize=1.0, realisations=1)
    assert inspect.signature(evaluate_raster).parameters["simulate"].default == 0
    sig = inspect.signature(simulate_voids).parameters
    assert [(k, v.default) for k, v in sig.items()][1:13] == [
        ("mask", None), ("nodata", None), ("cellsize", 1.0), ("variogram", None), ("realisations", 1), ("seed", 0), ("waves", 256),
        ("max_distance", None), ("fallback", "nearest"), ("keep", True), ("origin", (0, 0)), ("table", None)]
    from mvp_gan.src.simulate import spectral_waves
    assert [(k, v.default) for k, v in inspect.signature(spectral_waves).parameters.items()][2:] == [("waves", 256), ("seed", 0),
                                                                                                      ("outer_px", 4096)]


def test_no_cpu_path(monkeypatch):
    import torch
    from mvp_gan.src.simulate import simulate_voids
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        simulate_voids(np.zeros((8, 8), np.float32))


def test_exports():
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    from tg_hip import ops as O
    lib = L.load()
    for s in ("tg_sim_field", "tg_sim_combine", "tg_sim_stats"):
        assert hasattr(lib, s) and s in L.SIGNATURES
    assert L.TG_SIM_MAX_WAVES == O.SIM_MAX_WAVES == 512
    from mvp_gan.src import simulate as S
    assert S.MAX_WAVES == 512
    hdr = open(os.path.join(ROOT, "include", "terragan_hip.h")).read()
    assert "#define TG_SIM_MAX_WAVES 512" in hdr
    assert all(callable(getattr(O, n)) for n in ("sim_field", "sim_combine", "sim_stats"))
    build = open(os.path.join(ROOT, "terra-gan_amd", "build.py")).read()
    assert '"simulate.hip"' in build


def test_c_side_rejects_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    lib = L.load()
    buf = (C.c_char * 8192)()
    base = (C.addressof(buf) + 15) & ~15
    p, q, r, s = (C.c_void_p(base + 1024 * i) for i in range(4))

    def field(u=p, H=4, W=4, x0=0, y0=0, waves=q, n=4, amp=0.0):
        return lib.tg_sim_field(u, H, W, x0, y0, waves, n, amp, 0, 0, None)
    for kw, msg in ((dict(H=0), b"sides"), (dict(W=32768), b"sides"), (dict(u=None), b"null pointer"), (dict(waves=None), b"null"),
                    (dict(waves=C.c_void_p(base + 4)), b"aligned"), (dict(n=0), b"n_waves"), (dict(n=513), b"n_waves"),
                    (dict(x0=-1), b"origin"), (dict(y0=1 << 32), b"origin"), (dict(amp=-1.0), b"nugget_amp"),
                    (dict(amp=math.nan), b"nugget_amp"), (dict(amp=math.inf), b"nugget_amp")):
        assert field(**kw) == -1 and msg in lib.tg_last_error(), (kw, lib.tg_last_error())

    def combine(out=p, z=q, known=q, zk=r, u=r, uk=r, s1=None, s2=None, H=4, W=4):
        return lib.tg_sim_combine(out, z, known, zk, u, uk, s1, s2, H, W, None)
    for kw, msg in ((dict(H=0), b"non-empty"), (dict(out=None), b"null pointer"), (dict(uk=None), b"null pointer"),
                    (dict(s1=s), b"go together"), (dict(s2=s), b"go together"), (dict(s1=s, s2=s), b"distinct"),
                    (dict(out=q), b"alias"), (dict(out=r), b"alias")):
        assert combine(**kw) == -1 and msg in lib.tg_last_error(), (kw, lib.tg_last_error())

    def stats(mean=p, sd=q, zk=r, s1=s, s2=s, n=4, H=4, W=4):
        return lib.tg_sim_stats(mean, sd, zk, s1, s2, n, H, W, None)
    for kw, msg in ((dict(W=0), b"non-empty"), (dict(mean=None), b"null pointer"), (dict(s2=None), b"null pointer"),
                    (dict(n=1), b"n 1"), (dict(n=0), b"n 0"), (dict(sd=p), b"distinct"), (dict(zk=q), b"distinct")):
        assert stats(**kw) == -1 and msg in lib.tg_last_error(), (kw, lib.tg_last_error())


def test_ops_reject_before_any_launch():
    import torch
    from tg_hip import ops as O
    w = torch.zeros(4, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="sim_field"):
        O.sim_field(4, 4, w)                                              # not on the device
    with pytest.raises(ValueError, match="sim_field"):
        O.sim_field(0, 4, w)
    with pytest.raises(ValueError, match="sim_field"):
        O.sim_field(4, 4.0, w)
    z, k = torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="sim_combine"):
        O.sim_combine(z, k, z, z, z)
    with pytest.raises(ValueError, match="sim_stats"):
        O.sim_stats(z, z.double(), z.double(), 2)


def test_cli_parsers():
    from mvp_gan.src.evaluate_raster import build_parser as eval_parser
    from mvp_gan.src.simulate import build_parser, main
    a = build_parser().parse_args(["--dem", "in.asc", "--out", "s_{r}.asc"])
    assert (a.dem, a.out, a.mask, a.nodata, a.model, a.nugget, a.scale, a.shape, a.realisations, a.seed, a.waves, a.max_distance,
            a.no_fallback, a.mean_out, a.sd_out) == ("in.asc", "s_{r}.asc", None, None, "power", None, None, None, 1, 0, 256, None,
                                                     False, None, None)
    a = build_parser().parse_args(["--dem", "in.asc", "--out", "s_{r}.asc", "--realisations", "8", "--seed", "3", "--mean-out", "m.asc",
                                   "--sd-out", "sd.asc", "--model", "exponential", "--scale", "4", "--shape", "25", "--waves", "64"])
    assert (a.realisations, a.seed, a.mean_out, a.sd_out, a.model, a.scale, a.shape, a.waves) == \
        (8, 3, "m.asc", "sd.asc", "exponential", 4.0, 25.0, 64)
    for bad in (["--dem", "in.asc"], ["--dem", "in.asc", "--out", "o.asc", "--model", "spherical"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(bad)
    for bad in (["--realisations", "2", "--out", "o.asc"], ["--mean-out", "m.asc", "--out", "o.asc"], ["--waves", "600", "--out", "o.asc"],
                ["--model", "exponential", "--out", "o.asc"]):
        with pytest.raises(SystemExit):
            main(["--dem", "in.asc"] + bad)                               # refused before the raster is read
    for base in (["--dem", "in.asc", "--checkpoint", "g.pth"], ["--dem", "in.asc", "--pred", "p.asc", "--holes", "h.png"]):
        assert eval_parser().parse_args(base).simulate == 0
        assert eval_parser().parse_args(base + ["--simulate", "4"]).simulate == 4
    r = subprocess.run([sys.executable, "-m", "mvp_gan.src.simulate", "--help"], cwd=os.path.join(ROOT, "terra-gan_amd"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
