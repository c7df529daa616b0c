"""GPU checks of the exact Euclidean distance transform and the errors by depth (csrc/edt.hip, mvp_gan/src/distance.py,
mvp_gan/src/evaluate_raster.py) against the numpy oracle in tests/edt_oracle.py.  Every comparison of d2 and dist_m is bit for
bit; counts, maxima and per-hole depths are exact; the fp64 class sums hold to rtol 1e-12, the tolerance of the height sums of
the terrain errors."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import edt_oracle as EO
from tests import terrain_eval_oracle as TO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 64                                  # rows per band of the column pass (EDT_BAND in csrc/edt.hip)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def _edt(dev, seed, cap2=0, cellsize=None):
    from tg_hip import ops as O
    d2, dist = O.edt(torch.from_numpy(np.ascontiguousarray(seed, dtype=np.uint8)).to(dev), cap2, cellsize)
    return d2.cpu().numpy(), None if dist is None else dist.cpu().numpy()


def _check(dev, seed, cap2=0, cellsize=None, want=None):
    want = EO.edt_d2(seed, cap2) if want is None else want
    d2, dist = _edt(dev, seed, cap2, cellsize)
    assert d2.dtype == np.int32
    np.testing.assert_array_equal(d2, want)
    if cellsize is not None:
        np.testing.assert_array_equal(dist.view(np.int32), EO.metres(want, cellsize).view(np.int32))
    return d2


def _random(H, W, p, seed):
    return (np.random.default_rng(seed).random((H, W)) < p).astype(np.uint8)


def _layouts():
    out = {"1x1 seed": np.ones((1, 1), np.uint8), "1x1 none": np.zeros((1, 1), np.uint8),
           "1x300": _random(1, 300, 0.01, 1), "300x1": _random(300, 1, 0.01, 2), "7x300": _random(7, 300, 0.01, 3),
           "130x67": _random(130, 67, 0.2, 4)}
    for j, (y, x) in enumerate(((0, 0), (0, 66), (129, 0), (129, 66))):
        s = np.zeros((130, 67), np.uint8)
        s[y, x] = 1
        out[f"130x67 corner {j}"] = s
    col = np.zeros((65, 257), np.uint8)
    col[:, 200] = _random(65, 1, 0.2, 5)[:, 0]
    col[64, 200] = 1
    out["65x257 one column"] = col
    row = np.zeros((65, 257), np.uint8)
    row[3] = _random(1, 257, 0.05, 6)[0]
    row[3, 17] = 1
    out["65x257 one row"] = row
    out["257x1100 all"] = np.ones((257, 1100), np.uint8)
    out["257x1100 none"] = np.zeros((257, 1100), np.uint8)
    return out


LAYOUTS = _layouts()


@pytest.fixture(scope="module")
def big():
    """257 x 1100, p = 0.001: the largest d2 is in the thousands, so searches cross many 256-column strides and several
    bands, and some columns hold no seed.  The uncapped reference is computed once and shared."""
    seed = _random(257, 1100, 0.001, 7)
    want = EO.edt_d2(seed)
    assert want.max() > 2000 and (seed.sum(0) == 0).any()
    return seed, want


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layouts_bit_for_bit(dev, name):
    seed = LAYOUTS[name]
    d2 = _check(dev, seed, cellsize=1.0)
    if not seed.any():
        _, dist = _edt(dev, seed, cellsize=3.0)
        assert (d2 == EO.FAR).all() and np.isposinf(dist).all()


def test_big_case_caps_metres_and_determinism(dev, big):
    from tg_hip import ops as O
    seed, want = big
    _check(dev, seed, want=want)
    for cap2 in (1, 2, 25, 10000):
        _check(dev, seed, cap2, cellsize=1.0, want=np.minimum(want, cap2))
    for c in (0.25, 2.5):
        _check(dev, seed, cellsize=c, want=want)
    s = torch.from_numpy(seed).to(dev)
    a, b = O.edt(s, 0, 0.25), O.edt(s, 0, 0.25)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    none = np.zeros((70, 300), np.uint8)                      # a cap without any seed: the cap everywhere
    _check(dev, none, 49, cellsize=2.0, want=np.full((70, 300), 49, np.int32))


@pytest.mark.parametrize("H,W", [(BAND - 1, 70), (BAND, 70), (BAND + 1, 70), (2 * BAND + 1, 33), (40, 255), (40, 256), (40, 257),
                                 (3, 513)])
def test_route_boundaries(dev, H, W):
    """The column pass works in bands of 64 rows: H at the band height - 1, exactly and + 1, and two bands and a row, with
    seeds so sparse that the nearest one often lies in another band.  No route depends on W (the row of column distances is
    staged in LDS at every admitted width), but the kernels stride the columns by 256, so W straddles that too."""
    seed = _random(H, W, 0.004, H * 1000 + W)
    seed[H - 1, 0] = 1
    _check(dev, seed, cellsize=0.5)
    seed[:] = 0
    seed[0, W - 1] = 1                                         # one seed in the first band only: carried down every band
    _check(dev, seed)
    _check(dev, seed[::-1].copy())                             # and carried up


def test_largest_admitted_width(dev):
    """W = TG_EDT_MAX_SIDE: the row kernel's LDS request at its largest (2 B x 32767), and the largest k^2 + g^2."""
    from tg_hip import lib as L
    W = L.TG_EDT_MAX_SIDE
    seed = np.zeros((2, W), np.uint8)
    seed[1, 0] = 1
    x = np.arange(W, dtype=np.int64)
    want = np.stack([x * x + 1, x * x]).astype(np.int32)
    _check(dev, seed, want=want)
    _check(dev, seed, 10 ** 9, cellsize=0.5, want=np.minimum(want, 10 ** 9))


# ---- errors by depth -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    """300 x 420 at 2 m with invalid pixels and holes rasterised by tg_hole_masks (the evaluation cells); the raw kernel results
    and the oracle's d2, shared by the depth tests."""
    from mvp_gan.src.evaluate_raster import class_px, eval_holes
    from tg_hip import ops as O
    from tests.test_hip_terrain_eval import _terrain
    H, W, c = 300, 420, 2.0
    rng = np.random.default_rng(21)
    z = _terrain(H, W, c, 21)
    mask = (rng.random((H, W)) > 0.01).astype(np.float32)
    z[rng.random((H, W)) < 0.004] = np.nan
    z[rng.random((H, W)) < 0.003] = -9999.0
    hm, keep, info = eval_holes(z, mask, nodata=-9999.0, split=None, block=120, tile=60, seed=4)
    holes, keepn = hm.cpu().numpy(), keep.cpu().numpy()
    assert info["holes"] > 2000
    p = (np.where(np.isfinite(z), z, 0) + rng.normal(0, 1.0, (H, W)) * (holes != 0)).astype(np.float32)
    p[rng.random((H, W)) < 0.02] = np.nan
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    zd, pd, md = t(z), t(p), t(mask)
    labels, area = O.objmask_components(hm)
    table, slot, count = O.hole_table(labels, area, H * W)
    n = int(count.item())
    sums, counts, sel_a, _ = O.terrain_errors(zd, pd, md, -9999.0, hm, keep, labels, slot, table[:n], c,
                                              class_px([100.0, 1000.0, 10000.0], c))
    K = (keepn != 0) & np.isfinite(z) & (z != np.float32(-9999.0))
    return dict(H=H, W=W, c=c, z=z, p=p, mask=mask, holes=holes, keep=keepn, K=K, d2=EO.edt_d2(K), labels=labels, slot=slot,
                table=table[:n], n=n, sel_a=sel_a, zd=zd, keepd=keep, sums=sums.cpu().numpy(), counts=counts.cpu().tolist())


def test_depth_errors_against_oracle(dev, scene):
    from mvp_gan.src.distance import depth_px2
    from tg_hip import ops as O
    s = scene
    edges = depth_px2([2, 5, 10, 25, 50], s["c"])
    assert edges == [1, 7, 25, 157, 625]
    seeds, _ = O.objmask_known(s["zd"], s["keepd"], -9999.0, transposed=False)
    np.testing.assert_array_equal(seeds.cpu().numpy() != 0, s["K"])
    sel_a = s["sel_a"].cpu().numpy()
    labels = s["labels"].cpu().numpy()
    for cap2 in (0, edges[-1], 30):
        d2, _ = O.edt(seeds, cap2)
        want_d2 = np.minimum(s["d2"], cap2) if cap2 else s["d2"]
        np.testing.assert_array_equal(d2.cpu().numpy(), want_d2)
        for cls in (edges, edges[:1], [], [1, 1, 2, 2, 3, 4, 10 ** 9]):
            sums, counts, max_bits, hole_d2 = O.depth_errors(s["sel_a"], d2, s["labels"], s["slot"], s["n"], cls)
            ref = EO.depth_classes(sel_a, want_d2, cls)
            assert counts.cpu().tolist() == ref["counts"]
            assert max_bits.cpu().numpy().view(np.uint32).tolist() == ref["max_bits"]
            got = sums.cpu().numpy()
            np.testing.assert_allclose(got[0::2], ref["sum_a"], rtol=1e-12)
            np.testing.assert_allclose(got[1::2], ref["sum_a2"], rtol=1e-12)
            per_hole = EO.hole_max_d2(labels, want_d2)
            rows = s["table"][:, 0].cpu().numpy()
            assert len(per_hole) == s["n"]
            assert hole_d2.cpu().tolist() == [per_hole[int(l)] for l in rows]
            again = O.depth_errors(s["sel_a"], d2, s["labels"], s["slot"], s["n"], cls)
            assert all(torch.equal(x, y) for x, y in zip(again, (sums, counts, max_bits, hole_d2)))
    sums, counts, max_bits, hole_d2 = O.depth_errors(s["sel_a"], d2, s["labels"], s["slot"], 0, edges)       # no per-hole rows
    assert hole_d2.numel() == 0 and counts.cpu().tolist() == EO.depth_classes(sel_a, want_d2, edges)["counts"]


def test_depth_invariants(dev, scene):
    from mvp_gan.src.evaluate_raster import COUNTS, SUMS
    from tg_hip import ops as O
    s = scene
    cn = dict(zip(COUNTS, s["counts"]))
    sd = dict(zip(SUMS, s["sums"][:len(SUMS)].tolist()))
    seeds, _ = O.objmask_known(s["zd"], s["keepd"], -9999.0, transposed=False)
    d2, _ = O.edt(seeds, 625)
    sums, counts, _, _ = O.depth_errors(s["sel_a"], d2, s["labels"], s["slot"], s["n"], [1, 3, 25, 157, 625])
    counts, sums = counts.cpu().tolist(), sums.cpu().numpy()
    assert sum(counts) == cn["scored"] > 0
    np.testing.assert_allclose(sums[0::2].sum(), sd["s_a"], rtol=1e-12)          # = height.mae x scored
    np.testing.assert_allclose(sums[1::2].sum(), sd["s_a2"], rtol=1e-12)
    assert counts[0] == 0                                                          # no scored pixel is in K
    assert counts[1] == cn["ring"]                                                 # d2 in {1, 2}: an 8-neighbour in K
    scored = ~np.isnan(s["sel_a"].cpu().numpy()).reshape(s["H"], s["W"])
    assert int((scored & (s["d2"] >= 1) & (s["d2"] <= 2)).sum()) == cn["ring"]


def test_terrain_errors_by_depth(dev, scene):
    from mvp_gan.src.evaluate_raster import terrain_errors
    s = scene
    kw = dict(cellsize=s["c"], mask=s["mask"], nodata=-9999.0)
    args = (s["z"], s["p"], s["holes"], s["keep"])
    plain = terrain_errors(*args, **kw)
    ref, _ = TO.report(s["z"], s["p"], s["holes"], s["keep"], s["c"], s["mask"], -9999.0)
    assert "by_depth" not in plain and all("depth_m" not in h for h in plain["holes"]["worst"])
    assert plain["pixels"] == ref["pixels"] and plain["holes"] == ref["holes"]         # what it was before the option
    assert json.dumps(terrain_errors(*args, depth_edges_m=None, **kw)) == json.dumps(plain)
    edges = (2.0, 5.0, 10.0, 25.0, 50.0)
    rep = terrain_errors(*args, depth_edges_m=edges, **kw)
    assert json.dumps(terrain_errors(*args, depth_edges_m=edges, **kw)) == json.dumps(rep)
    for k in plain:
        if k != "holes":
            assert json.dumps(rep[k]) == json.dumps(plain[k]), k
    assert rep["holes"]["count"] == plain["holes"]["count"]
    for h, q in zip(rep["holes"]["worst"], plain["holes"]["worst"]):
        assert {k: v for k, v in h.items() if k != "depth_m"} == q
    assert set(rep) - set(plain) == {"by_depth"}
    px2 = EO.depth_px2(edges, s["c"])
    cap = np.minimum(s["d2"], px2[-1])
    want = EO.depth_classes(s["sel_a"].cpu().numpy(), cap, px2)
    bd = rep["by_depth"]
    assert bd["cap_m"] == 50.0 and [k["lo_m"] for k in bd["classes"]] == [0.0] + list(edges)
    assert [k["hi_m"] for k in bd["classes"]] == list(edges) + [math.inf]
    assert [k["pixels"] for k in bd["classes"]] == want["counts"][:6] and sum(want["counts"][6:]) == 0
    for k, n, sa, sa2, mb in zip(bd["classes"], want["counts"], want["sum_a"], want["sum_a2"], want["max_bits"]):
        if n:
            np.testing.assert_allclose([k["mae"], k["rmse"]], [sa / n, math.sqrt(sa2 / n)], rtol=1e-12)
            assert k["max"] == float(np.array([mb], np.uint32).view(np.float32)[0])
        else:
            assert math.isnan(k["mae"]) and math.isnan(k["rmse"]) and math.isnan(k["max"])
    per_hole = EO.hole_max_d2(s["labels"].cpu().numpy(), cap)
    for h in rep["holes"]["worst"]:
        assert h["depth_m"] == float(EO.metres(np.array([per_hole[h["label"]]]), s["c"])[0]) <= bd["cap_m"]
    # device tensors in, the same report out
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rep2 = terrain_errors(t(s["z"]), t(s["p"]), t(s["holes"]), t(s["keep"]), cellsize=s["c"], mask=t(s["mask"]), nodata=-9999.0,
                          depth_edges_m=edges)
    assert json.dumps(rep2) == json.dumps(rep)


def test_evaluate_raster_by_depth_with_baseline(dev):
    """End to end on the small scene of tests/test_hip_terrain_eval.py's CLI test: the GAN's curve and the baseline's on
    identical classes."""
    from mvp_gan.src.evaluate_raster import evaluate_raster, summary
    from mvp_gan.src.models import PConvUNet
    from tests.test_hip_terrain_eval import _terrain
    torch.manual_seed(7)
    G = PConvUNet().to(dev)
    H, W, c = 400, 520, 2.0
    z = _terrain(H, W, c, 8)
    kw = dict(cellsize=c, block=160, tile=80, window=128, overlap=16, baseline="laplace")
    rep, pred = evaluate_raster(G, z, depth_edges_m=(2, 5, 10), **kw)
    plain, pred0 = evaluate_raster(G, z, **kw)
    assert torch.equal(pred, pred0) and "by_depth" not in plain and "by_depth" not in plain["baseline"]
    for k in plain:
        if k not in ("holes", "baseline"):
            assert json.dumps(rep[k]) == json.dumps(plain[k]), k
    a, b = rep["by_depth"], rep["baseline"]["by_depth"]
    assert a["cap_m"] == b["cap_m"] == 10.0 and len(a["classes"]) == 4
    key = lambda bd: [(k["lo_m"], k["hi_m"], k["pixels"]) for k in bd["classes"]]
    assert key(a) == key(b) and sum(k["pixels"] for k in a["classes"]) == rep["pixels"]["scored"] > 0
    assert a["classes"][0]["pixels"] == 0                              # c = 2 m: nothing unknown is nearer than one pixel
    depth = {h["label"]: h["depth_m"] for h in rep["holes"]["worst"]}
    assert all(2.0 <= d <= 10.0 for d in depth.values())
    for h in rep["baseline"]["holes"]["worst"]:                        # the same holes: the same depths
        assert depth.get(h["label"], h["depth_m"]) == h["depth_m"]
    assert "by depth" in summary(rep) and "by depth" in summary(rep["baseline"])


# ---- the public API and the CLI -------------------------------------------------------------------------------------------
def _dirty_raster(H, W, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(100, 5, (H, W)).astype(np.float32)
    mask = np.ones((H, W), np.float32)
    mask[20:60, 30:90] = 0                                  # a masked block
    z[70:90, 10:25] = np.nan                                # a NaN hole
    z[5:15, 100:140] = -9999.0                              # a nodata hole
    z[rng.random((H, W)) < 0.01] = np.nan
    return z, mask


def test_distance_to_known(dev):
    from mvp_gan.src.distance import distance_to_known
    H, W, c = 100, 150, 0.5
    z, mask = _dirty_raster(H, W, 31)
    K = (mask != 0) & np.isfinite(z) & (z != np.float32(-9999.0))
    want = EO.edt_d2(K)
    dist, info = distance_to_known(z, mask, nodata=-9999.0, cellsize=c)
    np.testing.assert_array_equal(dist.cpu().numpy().view(np.int32), EO.metres(want, c).view(np.int32))
    assert info == {"known": int(K.sum()), "unknown": int((~K).sum()), "max_m": float(EO.metres(want, c).max()), "cap_m": None,
                    "capped": 0}
    assert info["max_m"] >= 10.0                            # the masked block is 40 rows deep: 20 px = 10 m
    dist, info = distance_to_known(torch.from_numpy(z).to(dev), torch.from_numpy(mask).to(dev), nodata=-9999.0, cellsize=c,
                                   max_distance=3.2)
    cap2 = 41                                               # 3.2 m / 0.5 m = 6.4 px, 6.4^2 = 40.96: d2 = 41 = 4^2 + 5^2 reaches it
    cap_m = float(np.float32(0.5 * math.sqrt(41.0)))
    wc = np.minimum(want, cap2)
    np.testing.assert_array_equal(dist.cpu().numpy().view(np.int32), EO.metres(wc, c).view(np.int32))
    assert info == {"known": int(K.sum()), "unknown": int((~K).sum()), "max_m": cap_m, "cap_m": cap_m, "capped": int((want >= 41).sum())}
    assert info["capped"] > 0
    # without mask and nodata the nodata cells count as terrain; a NaN nodata is no value
    dist, info = distance_to_known(z, nodata=math.nan)
    K2 = np.isfinite(z)
    np.testing.assert_array_equal(dist.cpu().numpy().view(np.int32), EO.metres(EO.edt_d2(K2), 1.0).view(np.int32))
    dist, info = distance_to_known(np.full((9, 11), np.nan, np.float32), cellsize=2.0)
    assert np.isposinf(dist.cpu().numpy()).all() and info == {"known": 0, "unknown": 99, "max_m": math.inf, "cap_m": None,
                                                                "capped": 0}
    dist, info = distance_to_known(np.full((9, 11), np.nan, np.float32), cellsize=2.0, max_distance=4.0)
    assert (dist.cpu().numpy() == 4.0).all() and info["max_m"] == math.inf and info["cap_m"] == 4.0 and info["capped"] == 99


def test_cli_round_trip(dev, tmp_path):
    from mvp_gan.src.asc import read_asc
    from tests.test_hip_terrain_eval import _write_asc
    H, W, c = 100, 150, 0.5
    z, mask = _dirty_raster(H, W, 32)
    z[np.isnan(z)] = -9999.0
    dem, mpath, out = (str(tmp_path / n) for n in ("dem.asc", "mask.asc", "depth.asc"))
    _write_asc(dem, z, c, -9999)
    _write_asc(mpath, mask, c)
    K = (mask != 0) & (z != np.float32(-9999.0))
    cwd = os.path.join(ROOT, "terra-gan_amd")
    run = lambda args: subprocess.run([sys.executable, "-m", "mvp_gan.src.distance", "--dem", dem, "--out", out] + args, cwd=cwd,
                                      capture_output=True, text=True, timeout=600)
    r = run(["--mask", mpath])
    assert r.returncode == 0, r.stderr
    assert f"{int(K.sum())} known" in r.stdout
    got, hdr = read_asc(out)
    np.testing.assert_array_equal(got.view(np.int32), EO.metres(EO.edt_d2(K), c).view(np.int32))
    assert dict(hdr)["cellsize"] == str(c)
    r = run(["--max-distance", "2"])
    assert r.returncode == 0, r.stderr
    got, _ = read_asc(out)
    K = z != np.float32(-9999.0)
    np.testing.assert_array_equal(got.view(np.int32), EO.metres(EO.edt_d2(K, 16), c).view(np.int32))
    # a raster without a known cell: +inf is written as the NODATA value
    _write_asc(dem, np.full((6, 7), -9999.0, np.float32), c, -9999)
    r = run([])
    assert r.returncode == 0, r.stderr
    got, _ = read_asc(out)
    assert (got == -9999.0).all()
