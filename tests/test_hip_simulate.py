"""GPU checks of the conditional simulation (csrc/simulate.hip, mvp_gan/src/simulate.py): tg_sim_field bit
for bit against the numpy mirror (tests/simulate_oracle.py), the exact identities of the whole path, a realisation against the
float64 kriging oracle within the bound of section 8ae, tg_sim_stats against the mirror, the CLI and the evaluation row."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import kriging_oracle as KO
from tests import simulate_oracle as SO
from tests.test_hip_kriging import _dirty_raster, _heights, _random, _t

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 300), (300, 1), (33, 65), (130, 67)]
WAVES = (1, 63, 256, 512)
ORIGINS = ((0, 0), (32700, 32700), (17, 2 ** 31 - 40))            # (row, column): the last one's columns cross 2^31
POWER, EXPO = ("power", 0.0, 0.02, 1.5), ("exponential", 0.0, 4.0, 30.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def _vg(spec):
    from mvp_gan.src.kriging import Variogram
    return Variogram(*spec)


def _table(n, seed=0, r=0, spec=POWER, c=1.0):
    from mvp_gan.src import simulate as S
    return S.with_phases(S.spectral_waves(_vg(spec), c, n, seed), seed, r)


def _field(dev, H, W, tab, origin=(0, 0), amp=0.0, seed=0, r=0):
    from mvp_gan.src.simulate import upload_waves
    from tg_hip import ops as O
    return O.sim_field(H, W, upload_waves(tab, dev), origin, amp, seed, r).cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(got, want):
    """Bit for bit, but for the sign and payload of a NaN, which numpy and the device choose differently."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    i = np.int32 if got.dtype == np.float32 else np.int64
    np.testing.assert_array_equal(got[~nan].view(i), want[~nan].view(i))


# ---- tg_sim_field, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_field_is_the_mirror_bit_for_bit(dev, H, W):
    for n in WAVES:
        tab = _table(n, seed=n, r=2)
        for origin in ORIGINS:
            for amp in (0.0, 0.3):
                got = _field(dev, H, W, tab, origin, amp, 11, 2)
                want = SO.field(H, W, tab, origin, amp, 11, 2)
                np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"{n} waves, origin {origin}, nugget {amp}")
    assert np.isfinite(got).all() and (got.size == 1 or got.std() > 0)


def test_field_of_a_tile_two_calls_and_streams(dev):
    H, W = 130, 67
    tab = _table(256, seed=4, r=1)
    for origin in ((0, 0), (2 ** 31 - 70, 2 ** 32 - 40)):               # the second one wraps 2^32 inside the raster
        whole = _field(dev, H, W, tab, origin, 0.25, 4, 1)
        np.testing.assert_array_equal(_bits(whole), _bits(SO.field(H, W, tab, origin, 0.25, 4, 1)))
        o = ((origin[0] + 64) % 2 ** 32, (origin[1] + 32) % 2 ** 32)
        tile = _field(dev, H - 64, W - 32, tab, o, 0.25, 4, 1)
        np.testing.assert_array_equal(_bits(tile), _bits(whole[64:, 32:]))
        np.testing.assert_array_equal(_bits(whole), _bits(_field(dev, H, W, tab, origin, 0.25, 4, 1)))
    base = _field(dev, H, W, tab, (0, 0), 0.25, 4, 1)
    quiet = _field(dev, H, W, tab, (0, 0), 0.0, 4, 1)
    assert not np.array_equal(base, quiet)
    np.testing.assert_array_equal(_bits(quiet), _bits(_field(dev, H, W, tab, (0, 0), 0.0, 9, 7)))       # no nugget: no hash
    assert not np.array_equal(base, _field(dev, H, W, tab, (0, 0), 0.25, 4, 2))                         # the realisation's stream
    assert not np.array_equal(base, _field(dev, H, W, tab, (0, 0), 0.25, 5, 1))                         # the seed's
    # more than one workgroup along a row, and a row that ends inside a lane's second pixel
    wide = _field(dev, 3, 1024 + 300, tab, (5, 7), 0.25, 4, 1)
    np.testing.assert_array_equal(_bits(wide), _bits(SO.field(3, 1324, tab, (5, 7), 0.25, 4, 1)))


def test_ops_refuse(dev):
    from mvp_gan.src.simulate import upload_waves
    from tg_hip import ops as O
    w = upload_waves(_table(8), dev)
    for kw in (dict(origin=(-1, 0)), dict(origin=(0, 2 ** 32)), dict(nugget_amp=-1.0), dict(nugget_amp=math.nan), dict(seed=-1),
               dict(realisation=2 ** 32)):
        with pytest.raises(ValueError, match="sim_field"):
            O.sim_field(4, 4, w, **kw)
    for bad in (w.float(), w[:, :3].contiguous(), torch.zeros(513, 4, dtype=torch.int32, device=dev), w[:0]):
        with pytest.raises(ValueError, match="waves"):
            O.sim_field(4, 4, bad)
    z, k = torch.zeros(4, 4, device=dev), torch.zeros(4, 4, dtype=torch.uint8, device=dev)
    s = torch.zeros(4, 4, dtype=torch.float64, device=dev)
    for args, msg in (((z, k, z, z, z, s), "go together"), ((z, k, z, z, z, s, s), "distinct"), ((z, k, z[:3], z, z), "zk"),
                      ((z, k, z, z, z, s, s.float()), "s2")):
        with pytest.raises(ValueError, match=msg):
            O.sim_combine(*args)
    for n in (1, 0, 2.0, True):
        with pytest.raises(ValueError, match="n "):
            O.sim_stats(z, s, s.clone(), n)


# ---- exact identities of the whole path ---------------------------------------------------------------------------------------
def test_realisations_do_not_depend_on_their_number_and_keep_known_pixels(dev):
    from mvp_gan.src.kriging import krige_voids
    from mvp_gan.src.simulate import simulate_voids
    z, known = _heights(130, 67, 1), _random(130, 67, 0.2, 21)
    vg = _vg(("power", 0.01, 0.02, 1.5))
    s4, m4, sd4, i4 = simulate_voids(z, known, cellsize=2.0, variogram=vg, realisations=4, seed=3)
    s8, m8, sd8, i8 = simulate_voids(_t(dev, z), _t(dev, known), cellsize=2.0, variogram=vg, realisations=8, seed=3)
    assert s4.shape == (4, 130, 67) and s4.dtype == torch.float32 and m4.shape == sd4.shape == (130, 67)
    assert torch.equal(s4.view(torch.int32), s8[:4].view(torch.int32))
    again = simulate_voids(z, known, cellsize=2.0, variogram=vg, realisations=4, seed=3)
    for a, b in zip((s4, m4, sd4), again[:3]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert again[3] == i4 and not torch.equal(s4[0], s4[1])
    assert not torch.equal(s4[0], simulate_voids(z, known, cellsize=2.0, variogram=vg, seed=4)[0][0])
    one, m1, sd1, i1 = simulate_voids(z, known, cellsize=2.0, variogram=vg, seed=3)
    assert m1 is None and sd1 is None and i1["sd_mean"] is None and torch.equal(one[0].view(torch.int32), s4[0].view(torch.int32))
    none, m, sd, _ = simulate_voids(z, known, cellsize=2.0, variogram=vg, realisations=4, seed=3, keep=False)
    assert none is None and torch.equal(m.view(torch.int32), m4.view(torch.int32)) and torch.equal(sd, sd4)
    kn = known != 0
    for r in range(8):
        np.testing.assert_array_equal(_bits(s8[r].cpu().numpy())[kn], _bits(z)[kn])
    fill, var, kinfo = krige_voids(z, known, cellsize=2.0, variogram=vg)
    assert {k: i4[k] for k in kinfo if k != "max_variance"} == {k: v for k, v in kinfo.items() if k != "max_variance"}
    assert (i4["waves"], i4["seed"], i4["realisations"], i8["realisations"]) == (256, 3, 4, 8)
    sdn = sd8.cpu().numpy()
    assert (sdn[kn] == 0).all() and (sdn[~kn] > 0).all() and i8["sd_max"] == float(sdn.max())
    assert i8["sd_mean"] == pytest.approx(float(sdn[~kn].astype(np.float64).mean()), rel=1e-12)
    # the spread is the kriging error's: 8 draws per pixel, 7000 pixels
    ratio = float((sdn[~kn].astype(np.float64) ** 2 / var.cpu().numpy()[~kn]).mean())
    assert 0.7 < ratio < 1.3, ratio


def test_zero_amplitudes_give_the_kriged_fill(dev):
    from mvp_gan.src import simulate as S
    from mvp_gan.src.kriging import krige_voids
    z, mask = _dirty_raster(100, 150, 32)
    vg = _vg(POWER)
    tab = S.spectral_waves(vg, 0.5, 64, 0)
    tab["amp"] = 0
    for md, fb in ((None, "nearest"), (3.2, "nearest"), (3.2, None)):
        fill, _, kinfo = krige_voids(z, mask, nodata=-9999.0, cellsize=0.5, variogram=vg, max_distance=md, fallback=fb)
        sims, mean, sd, info = S.simulate_voids(z, mask, nodata=-9999.0, cellsize=0.5, variogram=vg, realisations=2, table=tab,
                                                max_distance=md, fallback=fb)
        nan = torch.isnan(fill)
        assert bool(nan.any()) == (md is not None) and info["unfilled"] == kinfo["unfilled"] == int(nan.sum())
        assert info["by_nearest"] == kinfo["by_nearest"] and info["lim2"] == kinfo["lim2"] and info["waves"] == 64
        for s in (sims[0], sims[1], mean):
            assert torch.equal(torch.isnan(s), nan) and torch.equal(s[~nan].view(torch.int32), fill[~nan].view(torch.int32))
        assert torch.equal(torch.isnan(sd), nan) and bool((sd[~nan] == 0).all())


def test_holes_of_every_kind_max_distance_and_the_fallback(dev):
    from mvp_gan.src.kriging import krige_voids
    from mvp_gan.src.simulate import simulate_voids
    z, mask = _dirty_raster(100, 150, 32)
    K = (mask != 0) & np.isfinite(z) & (z != np.float32(-9999.0))
    vg = _vg(EXPO)
    for md, fb in ((None, "nearest"), (3.2, "nearest"), (3.2, None)):
        fill, _, kinfo = krige_voids(z, mask, nodata=-9999.0, cellsize=0.5, variogram=vg, max_distance=md, fallback=fb)
        sims, mean, sd, info = simulate_voids(z, mask, nodata=-9999.0, cellsize=0.5, variogram=vg, realisations=3, seed=1,
                                              max_distance=md, fallback=fb)
        s, f = sims.cpu().numpy(), fill.cpu().numpy()
        for r in range(3):
            np.testing.assert_array_equal(_bits(s[r])[K], _bits(z)[K])
            np.testing.assert_array_equal(np.isnan(s[r]), np.isnan(f))
        assert (info["unknown"], info["filled"], info["unfilled"]) == (int((~K).sum()), kinfo["filled"], kinfo["unfilled"])
        assert np.array_equal(np.isnan(sd.cpu().numpy()), np.isnan(f)) and np.array_equal(np.isnan(mean.cpu().numpy()), np.isnan(f))
        void = ~K & ~np.isnan(f)
        assert (s[0][void] != f[void]).mean() > 0.99 and np.abs(s[0] - f)[void].max() < 20.0
    assert info["unfilled"] > 0


def test_a_shift_of_the_heights_shifts_the_realisation(dev):
    """sims - krige on z and on z + 100 m.  u and krige(u) do not see the heights, so d = u - krige(u) is the same double in
    both runs and a run returns fl32(zk + d): the deviation it shows, sims - zk, is d plus the rounding of that one sum, at most
    half an ulp of the result.  Two runs, two such roundings: the deviations agree within one fp32 ulp of the (larger) heights."""
    from mvp_gan.src.kriging import krige_voids
    from mvp_gan.src.simulate import simulate_voids
    z, known = _heights(130, 67, 1), _random(130, 67, 0.2, 21)
    vg = _vg(POWER)
    dev_of = []
    for zz in (z, (z + np.float32(100.0)).astype(np.float32)):
        fill, _, _ = krige_voids(zz, known, cellsize=2.0, variogram=vg)
        sims, _, _, _ = simulate_voids(zz, known, cellsize=2.0, variogram=vg, realisations=2, seed=6)
        dev_of.append((sims.double() - fill.double()[None]).cpu().numpy())
        top = sims.abs().max(0).values.cpu().numpy()
    diff = np.abs(dev_of[0] - dev_of[1])
    assert (diff <= KO.ulp32(top)[None]).all(), float((diff / KO.ulp32(top)[None]).max())
    assert np.abs(dev_of[0])[:, known == 0].mean() > 100 * KO.ulp32(1100.0)        # there is a deviation to speak of


def test_all_known_none_known_and_one_row(dev):
    from mvp_gan.src.simulate import simulate_voids
    vg = _vg(POWER)
    z = _heights(20, 30, 8)
    sims, mean, sd, info = simulate_voids(z, cellsize=1.0, variogram=vg, realisations=2)
    assert all(torch.equal(s.view(torch.int32), _t(dev, z).view(torch.int32)) for s in (sims[0], sims[1], mean))
    assert bool((sd == 0).all()) and (info["unknown"], info["sd_mean"], info["sd_max"]) == (0, None, None)
    sims, mean, sd, info = simulate_voids(np.full((9, 11), np.nan, np.float32), variogram=vg, realisations=2)
    assert all(bool(torch.isnan(t).all()) for t in (sims, mean, sd)) and (info["unknown"], info["filled"], info["sd_mean"]) == (99, 0, None)
    with pytest.raises(ValueError, match="pass a Variogram"):
        simulate_voids(np.full((9, 11), np.nan, np.float32))
    z, known = _heights(1, 300, 5), _random(1, 300, 0.2, 25)
    sims, mean, sd, info = simulate_voids(z, known, cellsize=0.5, variogram=vg, realisations=3, origin=(7, 2 ** 31 - 100))
    kn = known != 0
    s = sims.cpu().numpy()
    assert info["unfilled"] == 0 and np.isfinite(s).all() and all(np.array_equal(_bits(s[r])[kn], _bits(z)[kn]) for r in range(3))
    assert bool((sd[_t(dev, known) == 0] > 0).all())
    # a tile of a larger raster with its origin set draws the same field: the same void, the same samples, the same bits
    big, bk = _heights(96, 160, 9), _random(96, 160, 0.2, 29)
    bk[32:64, 48:112] = 1
    bk[40:56, 60:100] = 0                                                # a void whose rays all end inside the tile
    whole = simulate_voids(big, bk, cellsize=1.0, variogram=vg, seed=2)[0][0]
    tile = simulate_voids(big[32:64, 48:112], bk[32:64, 48:112], cellsize=1.0, variogram=vg, seed=2, origin=(32, 48))[0][0]
    assert torch.equal(tile.view(torch.int32), whole[32:64, 48:112].view(torch.int32))
    assert not torch.equal(tile, simulate_voids(big[32:64, 48:112], bk[32:64, 48:112], cellsize=1.0, variogram=vg, seed=2)[0][0])


# ---- a realisation against the oracle -----------------------------------------------------------------------------------------
def _scenes():
    sparse = _random(257, 300, 0.001, 41)
    return {"p20": (_heights(130, 67, 1), _random(130, 67, 0.2, 21)), "sparse": (_heights(257, 300, 2), sparse)}


@pytest.fixture(scope="module")
def oracle_scenes():
    return {name: (z, known, KO.ray_hits(known), KO.nearest(known)) for name, (z, known) in _scenes().items()}


@pytest.mark.parametrize("spec", [POWER, EXPO], ids=lambda s: s[0])
@pytest.mark.parametrize("name", ["p20", "sparse"])
def test_a_realisation_is_the_oracle_within_the_bound(dev, oracle_scenes, name, spec):
    """Per void pixel |sim - (zk + (u - uk))| <= bound(zk) + bound(uk) + ulp32 / 2: the bound of section 8ae on either kriging,
    0.5 ulp32 + 64 * 2^-52 * cond * sum |w_i v_i| with v the heights and then the field, and half an ulp of the result for the
    one rounding of the combine."""
    from mvp_gan.src import simulate as S
    z, known, hits, ft = oracle_scenes[name]
    vg, c, seed, r = _vg(spec), 2.5, 5, 1
    sims, _, _, info = S.simulate_voids(z, known, cellsize=c, variogram=vg, realisations=2, seed=seed)
    got = sims[r].cpu().numpy()
    H, W = z.shape
    u = SO.field(H, W, S.with_phases(S.spectral_waves(vg, c, 256, seed), seed, r), (0, 0), math.sqrt(vg.nugget), seed, r)
    wz, wu = KO.krige(z, known, hits, vg, c, *ft), KO.krige(u, known, hits, vg, c, *ft)
    assert (info["filled"] - info["by_nearest"], info["by_nearest"], info["unfilled"]) == tuple(wz["counts"])
    void = known == 0
    want = wz["out"] + (u.astype(np.float64) - wu["out"])
    bound = wz["est_bound"] + wu["est_bound"] + 0.5 * KO.ulp32(want)
    err = np.abs(got.astype(np.float64) - want)
    assert np.isfinite(got).all() and (err[void] <= bound[void]).all(), (float((err - bound)[void].max()), int((err > bound)[void].sum()))
    np.testing.assert_array_equal(_bits(got)[~void], _bits(z)[~void])
    assert np.median((bound / KO.ulp32(want))[void]) < 1.1               # in effect a rounding or two of the fp32 result
    assert np.abs(want - wz["out"])[void].std() > 0.01                   # and the draw is no small change to the fill


# ---- the statistics -----------------------------------------------------------------------------------------------------------
def test_stats_are_the_mirror(dev):
    """5 realisations through the ops.  The running sums are the mirror's bit for bit (one thread per pixel, the same doubles in
    the same order); the mean is within half an fp32 ulp of zk + s1 / n; the sd is held to the two-pass definition in long
    double: the one-pass variance (s2 - s1^2 / n) / (n - 1) carries at most (3 n + 4) 2^-52 s2 / (n - 1) of rounding (n 2^-52 s2
    from the sum of squares, 2 n 2^-52 s1^2 / n <= 2 n 2^-52 s2 from the square of the sum, 4 2^-52 s2 from the last three
    operations), |sqrt a - sqrt b| <= min(sqrt |a - b|, |a - b| / sqrt b), and half an fp32 ulp for the result."""
    from mvp_gan.src import simulate as S
    from tg_hip import ops as O
    z, mask = _dirty_raster(100, 150, 34)
    K = ((mask != 0) & np.isfinite(z) & (z != np.float32(-9999.0))).astype(np.uint8)
    zc = np.where(K != 0, z, np.float32(0))
    vg, c, n = _vg(("power", 0.01, 0.02, 1.5)), 0.5, 5
    dz, dk = _t(dev, zc), _t(dev, K)
    _, _, hits = O.rayfill(dz, dk, 40, 2.0, want_hits=True)               # a limit: some pixels stay unfilled
    args = (c, vg.model, vg.nugget, vg.scale, vg.shape)
    zk, _, counts = O.krige(dz, dk, hits, *args)
    assert counts.cpu().tolist()[2] > 0
    s1, s2 = (torch.zeros(100, 150, dtype=torch.float64, device=dev) for _ in range(2))
    m1, m2, ds = np.zeros((100, 150)), np.zeros((100, 150)), []
    tab = S.spectral_waves(vg, c, 63, 1)
    for r in range(n):
        u = O.sim_field(100, 150, S.upload_waves(S.with_phases(tab, 1, r), dev), (0, 0), 0.1, 1, r)
        uk, _, _ = O.krige(u, dk, hits, *args)
        out = O.sim_combine(dz, dk, zk, u, uk, s1, s2)
        plain = O.sim_combine(dz, dk, zk, u, uk)
        assert torch.equal(out.view(torch.int32), plain.view(torch.int32))
        un, ukn = u.cpu().numpy(), uk.cpu().numpy()
        want = SO.combine(zc, K, zk.cpu().numpy(), un, ukn, m1, m2)
        _same(out.cpu().numpy(), want)
        ds.append(un.astype(np.longdouble) - ukn.astype(np.longdouble))
    _same(s1.cpu().numpy(), m1)
    _same(s2.cpu().numpy(), m2)
    mean, sd = (t.cpu().numpy() for t in O.sim_stats(zk, s1, s2, n))
    zkn = zk.cpu().numpy()
    nan, kn = np.isnan(zkn), K != 0
    assert nan.any() and np.isnan(mean[nan]).all() and np.isnan(sd[nan]).all() and not np.isnan(mean[~nan]).any()
    assert (sd[kn] == 0).all() and not np.signbit(sd[kn]).any() and np.array_equal(_bits(mean)[kn], _bits(zc)[kn])
    ok = ~nan & ~kn
    m64 = zkn.astype(np.float64) + m1 / n
    assert (np.abs(mean.astype(np.float64) - m64)[ok] <= 0.5 * KO.ulp32(m64)[ok]).all()
    d = np.stack(ds)
    true_v = (((d - d.mean(0)) ** 2).sum(0) / (n - 1)).astype(np.float64)
    true_sd = np.sqrt(true_v)
    bv = (3 * n + 4) * 2.0 ** -52 * m2 / (n - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = np.minimum(np.sqrt(bv), np.where(true_sd > 0, bv / true_sd, np.inf)) + 0.5 * KO.ulp32(true_sd)
    err = np.abs(sd.astype(np.float64) - true_sd)
    assert (err[ok] <= bound[ok]).all(), float((err - bound)[ok].max())
    assert (bound[ok] <= 0.51 * KO.ulp32(true_sd)[ok]).all()             # the fp64 part is small change here
    ms, ss, _ = SO.stats(zkn, m1, m2, n)
    np.testing.assert_array_equal(_bits(mean)[~nan], _bits(ms)[~nan])
    np.testing.assert_array_equal(_bits(sd)[~nan], _bits(ss)[~nan])


# ---- the CLI and the evaluation row -------------------------------------------------------------------------------------------
def test_cli_round_trip(dev, tmp_path):
    from mvp_gan.src.asc import read_asc
    from mvp_gan.src.simulate import simulate_voids
    from tests.test_hip_terrain_eval import _write_asc
    H, W, c = 100, 150, 0.5
    z, mask = _dirty_raster(H, W, 33)
    z[np.isnan(z)] = -9999.0
    dem, mpath, out, mout, sout = (str(tmp_path / n) for n in ("dem.asc", "mask.asc", "sim_{r}.asc", "mean.asc", "sd.asc"))
    _write_asc(dem, z, c, -9999)
    _write_asc(mpath, mask, c)
    r = subprocess.run([sys.executable, "-m", "mvp_gan.src.simulate", "--dem", dem, "--out", out, "--mask", mpath, "--realisations",
                        "3", "--seed", "2", "--mean-out", mout, "--sd-out", sout, "--model", "exponential", "--nugget", "0.02",
                        "--scale", "6", "--shape", "40", "--waves", "64", "--max-distance", "2", "--no-fallback"],
                       cwd=os.path.join(ROOT, "terra-gan_amd"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    zr, _ = read_asc(dem)
    sims, mean, sd, info = simulate_voids(zr, mask, nodata=-9999.0, cellsize=c, variogram=_vg(("exponential", 0.02, 6.0, 40.0)),
                                          realisations=3, seed=2, waves=64, max_distance=2.0, fallback=None)
    assert info["unfilled"] > 0 and f"3 realisations of {info['unknown']} void pixels" in r.stdout and "64 waves, seed 2" in r.stdout
    files = [out.replace("{r}", str(k)) for k in range(3)] + [mout, sout]
    for path, want in zip(files, list(sims) + [mean, sd]):
        got, hdr = read_asc(path)
        w = want.cpu().numpy()
        assert dict(hdr)["cellsize"] == str(c) and (got[np.isnan(w)] == -9999.0).all()
        np.testing.assert_array_equal(_bits(got)[~np.isnan(w)], _bits(w)[~np.isnan(w)])          # 9 digits: bit for bit
    bad = subprocess.run([sys.executable, "-m", "mvp_gan.src.simulate", "--dem", dem, "--out", str(tmp_path / "one.asc"),
                          "--realisations", "2"], cwd=os.path.join(ROOT, "terra-gan_amd"), capture_output=True, text=True,
                         timeout=600)
    assert bad.returncode == 2 and "{r}" in bad.stderr


def test_evaluate_raster_simulate(dev):
    """End to end on the small scene of tests/test_hip_kriging.py: the GAN, kriging and the simulation on the same holes and
    depth classes; a run without the keyword has the report it had."""
    from mvp_gan.src.evaluate_raster import eval_holes, evaluate_raster, summary, texture_errors
    from mvp_gan.src.kriging import Variogram
    from mvp_gan.src.models import PConvUNet
    from mvp_gan.src.simulate import simulate_voids
    from tests.test_hip_terrain_eval import _terrain
    torch.manual_seed(7)
    G = PConvUNet().to(dev)
    H, W, c = 400, 520, 2.0
    z = _terrain(H, W, c, 8)
    kw = dict(cellsize=c, block=160, tile=80, window=128, overlap=16, depth_edges_m=(2, 5, 10), kriging=True, texture=True,
              texture_octaves=3)
    rep, pred = evaluate_raster(G, z, simulate=4, **kw)
    plain, pred0 = evaluate_raster(G, z, **kw)
    assert torch.equal(pred, pred0) and "simulation" not in plain
    assert list(plain) == [k for k in rep if k != "simulation"]
    assert json.dumps({k: v for k, v in rep.items() if k != "simulation"}) == json.dumps(plain)
    r, kr = rep["simulation"], rep["kriging"]
    assert {"calibration", "texture", "variogram", "realisations", "method", "fill", "by_depth", "height", "pixels"} <= set(r)
    assert r["method"] == "simulation" and r["realisations"] == 4 and r["variogram"] == kr["variogram"] == r["fill"]["variogram"]
    assert r["fill"]["fitted"] is True and r["fill"]["realisations"] == 4 and r["fill"]["unknown"] == kr["fill"]["unknown"]
    assert r["pixels"] == kr["pixels"] and r["holes"]["count"] == kr["holes"]["count"] and "by depth" in summary(r)
    key = lambda q: [(k["lo_m"], k["hi_m"], k["pixels"]) for k in q["by_depth"]["classes"]]
    assert key(r) == key(kr) == key(rep) and math.isfinite(r["height"]["rmse"])
    hm, keep, _ = eval_holes(z, split="test", block=160, tile=80)
    vg = Variogram(**r["variogram"])
    _, mean, sd, info = simulate_voids(z, keep, cellsize=c, variogram=vg, realisations=4, keep=False)
    assert dict(info, fitted=True) == r["fill"]
    cal = r["calibration"]
    cells = int(((hm != 0) & torch.isfinite(mean) & (sd > 0)).sum())
    assert cal["cells"] == cells == r["pixels"]["scored"] > 0
    z2 = ((mean.double() - _t(dev, z).double()) ** 2 / (sd * sd).double())[(hm != 0) & (sd > 0)]
    assert cal["mean_z2"] == pytest.approx(float(z2.mean()), rel=1e-12) and 0 < cal["within_1sigma"] <= cal["within_2sigma"] <= 1
    first = simulate_voids(z, keep, cellsize=c, variogram=vg)[0][0]
    assert r["texture"] == texture_errors(z, first, hm, cellsize=c, octaves=3)
    # what the row is for: the kriged fill is too smooth (a ratio below 1); a realisation is nearer 1 at the shortest lag and over
    # the scales together
    ratio = lambda t: t["scales"][0]["ratio"]
    print("texture ratio at 1 px: kriging", ratio(kr["texture"]), "realisation 0", ratio(r["texture"]), "log-ratio RMS",
          kr["texture"]["log_ratio_rms"], r["texture"]["log_ratio_rms"])
    assert ratio(kr["texture"]) < 1 and abs(math.log(ratio(r["texture"]))) < abs(math.log(ratio(kr["texture"])))
    assert r["texture"]["log_ratio_rms"] < kr["texture"]["log_ratio_rms"]
    with pytest.raises(ValueError, match="simulate"):
        evaluate_raster(G, z, simulate=1, **kw)
    json.dumps(rep)
