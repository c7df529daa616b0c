"""GPU checks of the held-out terrain errors (csrc/terrain_eval.hip, mvp_gan/src/evaluate_raster.py) against the numpy oracle
in tests/terrain_eval_oracle.py: evaluation holes bit for bit, counts / per-hole table / quantiles exact, fp64 statistics to
rtol 1e-12 (height) and 1e-9 (slope, gradient, Laplacian), the exact selection, edge cases, determinism, evaluate_raster end to
end and the CLIs."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import terrain_eval_oracle as TO
from tests.test_hip_object_mask import _dirty

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def G(dev):
    from mvp_gan.src.models import PConvUNet
    torch.manual_seed(7)
    return PConvUNet().to(dev)


def _terrain(H, W, c, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64) * c
    z = 200 + 0.05 * x - 0.03 * y + 8 * np.sin(x / 180.0) * np.cos(y / 130.0) + rng.normal(0, 0.2, (H, W))
    return z.astype(np.float32)


def _compare(rep, ref):
    assert rep["pixels"] == ref["pixels"]
    assert rep["holes"] == ref["holes"]
    for k in ("bias", "mae", "rmse"):
        np.testing.assert_allclose(rep["height"][k], ref["height"][k], rtol=1e-12, equal_nan=True)
    assert np.array_equal(rep["height"]["max"], ref["height"]["max"], equal_nan=True)
    assert json.dumps(rep["height"]["quantiles"]) == json.dumps(ref["height"]["quantiles"])
    for k in ("mae", "rmse", "gradient_rmse", "laplacian_rmse"):
        np.testing.assert_allclose(rep["slope_deg"][k], ref["slope_deg"][k], rtol=1e-9, equal_nan=True)
    a, b = np.float32(rep["slope_deg"]["p90"]), np.float32(ref["slope_deg"]["p90"])
    assert (np.isnan(a) and np.isnan(b)) or abs(int(a.view(np.int32)) - int(b.view(np.int32))) <= 1, (a, b)
    for k in ("mae", "rmse"):
        np.testing.assert_allclose(rep["ring"][k], ref["ring"][k], rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(rep["ring"]["gradient_rmse"], ref["ring"]["gradient_rmse"], rtol=1e-9, equal_nan=True)
    for x, y in zip(rep["by_area"], ref["by_area"]):
        assert {k: x[k] for k in ("lo_m2", "hi_m2", "holes", "pixels")} == {k: y[k] for k in ("lo_m2", "hi_m2", "holes", "pixels")}
        np.testing.assert_allclose([x["mae"], x["rmse"]], [y["mae"], y["rmse"]], rtol=1e-12, equal_nan=True)


EVAL_SHAPES = [(1, 1), (1, 517), (517, 1), (37, 1031), (300, 460), (1500, 2100)]


@pytest.mark.parametrize("H,W", EVAL_SHAPES)
def test_eval_holes_against_oracle(dev, H, W):
    from mvp_gan.src.evaluate_raster import eval_holes
    from mvp_gan.src.utils.raster_dataset import HoleSpec
    from tg_hip import ops as O
    from tests.objmask_oracle import known_map
    z, mask = _dirty(H, W, H + 3 * W)
    rng = np.random.default_rng(H * W)
    objects = (rng.random((H, W)) < 0.05).astype(np.uint8)
    tile, block = (40, 80) if max(H, W) < 600 else (100, 200)
    for split in ("test", None):
        hole = TO.cell_hole_map(H, W, split, block, tile, HoleSpec(), 3)
        for obj in (None, objects):
            want_h, want_k, want_c = TO.eval_holes(z, mask, -9999.0, obj, hole)
            zd, md = torch.from_numpy(z).to(dev), torch.from_numpy(mask).to(dev)
            hd = torch.empty(H, W, dtype=torch.uint8, device=dev)
            kd = torch.empty(H, W, dtype=torch.float32, device=dev)
            cd = torch.zeros(3, dtype=torch.int64, device=dev)
            O.eval_holes(zd, md, -9999.0, None if obj is None else torch.from_numpy(obj).to(dev), None, None, 1024, 0, H, hd, kd,
                         cd, hole_in=torch.from_numpy(hole.astype(np.uint8)).to(dev))
            np.testing.assert_array_equal(hd.cpu().numpy(), want_h)
            np.testing.assert_array_equal(kd.cpu().numpy(), want_k)
            assert cd.cpu().tolist() == want_c
            if obj is None:
                h, k, info = eval_holes(z, mask, nodata=-9999.0, split=split, block=block, tile=tile, seed=3)
                np.testing.assert_array_equal(h.cpu().numpy(), want_h)
                np.testing.assert_array_equal(k.cpu().numpy(), want_k)
                assert [info["valid"], info["holes"], info["objects"]] == want_c
    assert known_map(z, mask, -9999.0).sum() == want_c[0]


def _case(H, W, seed, c=2.0, unfilled=0.02):
    """A truth raster with invalid pixels, holes from a random hole map, a prediction with noise and some NaN."""
    rng = np.random.default_rng(seed)
    z = _terrain(H, W, c, seed)
    mask = (rng.random((H, W)) > 0.01).astype(np.float32)
    z[rng.random((H, W)) < 0.005] = np.nan
    z[rng.random((H, W)) < 0.003] = -9999.0
    hole = np.zeros((H, W), bool)
    for _ in range(max(1, H * W // 4000)):
        y, x = rng.integers(0, H), rng.integers(0, W)
        r = int(rng.integers(0, 12))
        hole[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
    hole[0, :] = True                                        # holes on the raster border
    obj = (rng.random((H, W)) < 0.01).astype(np.uint8)
    holes, keep, _ = TO.eval_holes(z, mask, -9999.0, obj, hole)
    p = (np.where(np.isfinite(z), z, 0) + rng.normal(0, 1.0, (H, W)) * (hole * 1.0)).astype(np.float32)
    p[rng.random((H, W)) < unfilled] = np.nan
    return z, p, mask, holes, keep


@pytest.mark.parametrize("H,W,c", [(3, 3, 1.0), (37, 1031, 0.5), (300, 460, 2.0), (1500, 2100, 2.0)])
def test_terrain_errors_against_oracle(dev, H, W, c):
    from mvp_gan.src.evaluate_raster import terrain_errors
    z, p, mask, holes, keep = _case(H, W, H + W)
    rep = terrain_errors(z, p, holes, keep, cellsize=c, mask=mask, nodata=-9999.0)
    ref, r = TO.report(z, p, holes, keep, c, mask, -9999.0)
    assert rep["pixels"]["scored"] > 0 or H * W < 20
    _compare(rep, ref)
    rep2 = terrain_errors(torch.from_numpy(z).to(dev), torch.from_numpy(p).to(dev), torch.from_numpy(holes).to(dev),
                          torch.from_numpy(keep).to(dev), cellsize=c, mask=torch.from_numpy(mask).to(dev), nodata=-9999.0)
    assert json.dumps(rep2) == json.dumps(rep)                      # determinism, NaN included


def test_terrain_errors_raw_table_and_counts(dev):
    """The per-hole table and the counters straight from the kernels, bit for bit."""
    from tg_hip import ops as O
    from mvp_gan.src.evaluate_raster import COUNTS, class_px
    H, W, c = 400, 700, 1.0
    z, p, mask, holes, keep = _case(H, W, 9)
    r = TO.raw(z, p, holes, keep, c, mask, -9999.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    labels, area = O.objmask_components(t(holes))
    table, slot, count = O.hole_table(labels, area, H * W)
    n = int(count.item())
    sums, counts, sel_a, sel_s = O.terrain_errors(t(z), t(p), t(mask), -9999.0, t(holes), t(keep), labels, slot, table[:n], c,
                                                  class_px([100.0, 1000.0, 10000.0], c))
    tb = table[:n].cpu().numpy()
    np.testing.assert_array_equal(tb[np.argsort(tb[:, 0])], r["table"])
    assert dict(zip(COUNTS, counts.cpu().tolist())) == r["counts"]
    np.testing.assert_array_equal(sel_a.cpu().numpy().view(np.int32), r["sel_a"].ravel().view(np.int32))
    got_s, want_s = sel_s.cpu().numpy(), r["sel_s"].ravel()
    assert (np.isnan(got_s) == np.isnan(want_s)).all()
    # per pixel the fp64 slopes may round differently (fused multiply-adds on the device): near ds = 0 that is all of ds
    np.testing.assert_allclose(got_s[~np.isnan(got_s)], want_s[~np.isnan(want_s)], rtol=1e-6, atol=1e-9)


def test_edge_cases(dev):
    from mvp_gan.src.evaluate_raster import terrain_errors
    H, W, c = 64, 96, 1.0
    z = _terrain(H, W, c, 1)
    none = np.zeros((H, W), np.uint8)
    rep = terrain_errors(z, z, none, np.ones((H, W), np.float32), cellsize=c)
    assert rep["pixels"]["holes"] == 0 and rep["holes"] == {"count": 0, "worst": []}
    assert math.isnan(rep["height"]["mae"]) and math.isnan(rep["slope_deg"]["p90"]) and math.isnan(rep["ring"]["rmse"])
    hole = np.zeros((H, W), bool)
    hole[10:30, 20:50] = True
    hole[0:3, 0:5] = True                                    # on the border: not in T
    hole[50, 80] = True                                      # one pixel
    hole[60, 90] = True
    holes, keep, _ = TO.eval_holes(z, None, None, None, hole)
    rep = terrain_errors(z, z, holes, keep, cellsize=c)      # p == z
    assert rep["height"]["mae"] == 0 and rep["height"]["max"] == 0 and rep["slope_deg"]["rmse"] == 0
    assert all(v == 0 for v in rep["height"]["quantiles"].values())
    ref, r = TO.report(z, z, holes, keep, c)
    _compare(rep, ref)
    assert not r["T"][0].any() and r["T"][1, 1:4].all() and rep["holes"]["count"] == 4
    p = z.copy()
    p[hole] = np.nan                                         # all unfilled
    rep = terrain_errors(z, p, holes, keep, cellsize=c)
    assert rep["pixels"]["unfilled"] == hole.sum() and rep["pixels"]["scored"] == 0 and math.isnan(rep["height"]["rmse"])
    assert rep["holes"]["count"] == 4 and rep["holes"]["worst"] == []
    every = np.ones((H, W), np.uint8)                        # one hole spanning the raster
    p = z + np.float32(0.25)
    rep = terrain_errors(z, p, every, np.zeros((H, W), np.float32), cellsize=c)
    ref, _ = TO.report(z, p, every, np.zeros((H, W), np.float32), c)
    _compare(rep, ref)
    assert rep["holes"]["count"] == 1 and rep["holes"]["worst"][0]["bbox"] == [0, 0, H - 1, W - 1]
    assert rep["pixels"]["ring"] == 0 and rep["pixels"]["slope_scored"] == (H - 2) * (W - 2)


def test_select_f32_against_sort(dev):
    from tg_hip import ops as O
    rng = np.random.default_rng(0)
    cases = [np.array([1.5], np.float32), np.zeros(1000, np.float32),
             np.array([0, 1e-45, 2e-45, 1e-40, 1.17e-38, 0, 3, 3, 3, np.inf], np.float32),
             rng.integers(0, 5, 10001).astype(np.float32),
             np.abs(rng.standard_cauchy(3_000_001)).astype(np.float32)]
    mixed = rng.normal(0, 10, 200_000).astype(np.float32)
    mixed[::7] = np.nan
    cases.append(mixed)                                      # negatives and NaN are skipped
    for v in cases:
        keep = v[~np.isnan(v) & (v.view(np.int32) >= 0)]
        s = np.sort(keep)
        n = s.size
        ks = sorted({0, n - 1, n // 2, (9 * n) // 10, max(n - 2, 0), n, -1, min(3, n - 1)})[:8]
        got = O.select_f32(torch.from_numpy(v).to(dev), ks).cpu().numpy()
        for k, g in zip(ks, got):
            if 0 <= k < n:
                assert g.view(np.int32) == s[k].view(np.int32), (v.size, k, g, s[k])
            else:
                assert np.isnan(g)


def test_evaluate_raster_end_to_end(dev, G):
    from mvp_gan.src.evaluate_raster import eval_holes, evaluate_raster, terrain_errors
    from mvp_gan.src.inpaint_raster import inpaint_raster
    from mvp_gan.src.object_mask import ObjectSpec
    H, W, c = 1500, 2100, 2.0
    z = _terrain(H, W, c, 4)
    z[700:720, 100:200] = np.nan
    kw = dict(cellsize=c, split="test", block=512, tile=128, seed=2, window=256, overlap=32, batch=8)
    rep, pred = evaluate_raster(G, z, **kw)
    h, keep, _ = eval_holes(z, split="test", block=512, tile=128, seed=2)
    hn, kn = h.cpu().numpy() != 0, keep.cpu().numpy() != 0
    yy, xx = np.nonzero(hn)
    assert hn.any() and (((xx // 512) - (yy // 512)) % 3 == 2).all()
    ref_pred, _ = inpaint_raster(G, z, keep, window=256, overlap=32, batch=8)
    np.testing.assert_array_equal(pred.cpu().numpy().view(np.int32), ref_pred.cpu().numpy().view(np.int32))
    np.testing.assert_array_equal(pred.cpu().numpy()[kn].view(np.int32), z[kn].view(np.int32))
    ref = terrain_errors(z, ref_pred, h, keep, cellsize=c)
    assert all(rep[k] == ref[k] or json.dumps(rep[k]) == json.dumps(ref[k]) for k in ref)
    rep2, pred2 = evaluate_raster(G, z, **kw)
    assert json.dumps(rep2) == json.dumps(rep) and torch.equal(pred2, pred)
    assert rep["pixels"]["scored"] > 0 and math.isfinite(rep["height"]["rmse"]) and rep["tile"] == 128
    # with objects: no object pixel is scored
    spec = ObjectSpec()
    zo = z.copy()
    zo[300:330, 400:440] += 10.0                             # a building in a test block
    rep_o, _ = evaluate_raster(G, zo, objects=spec, **kw)
    from mvp_gan.src.object_mask import object_mask
    obj = object_mask(zo, cellsize=c, spec=spec)[0].cpu().numpy() != 0
    ho, _, _ = eval_holes(zo, split="test", block=512, tile=128, seed=2, objects=spec, cellsize=c)
    assert obj.any() and not (ho.cpu().numpy().astype(bool) & obj).any()
    assert rep_o["pixels"]["objects"] == int((obj & np.isfinite(zo)).sum())


def _write_asc(path, a, c, nodata=None):
    from mvp_gan.src.asc import write_asc
    hdr = [("ncols", str(a.shape[1])), ("nrows", str(a.shape[0])), ("xllcorner", "0"), ("yllcorner", "0"), ("cellsize", str(c))]
    if nodata is not None:
        hdr.append(("NODATA_value", str(nodata)))
    write_asc(path, a, hdr)


def test_clis(dev, G, tmp_path):
    H, W, c = 400, 520, 2.0
    z = _terrain(H, W, c, 8)
    dem = str(tmp_path / "dem.asc")
    _write_asc(dem, z, c, -9999)
    ck = str(tmp_path / "g.pth")
    torch.save({"generator_state_dict": G.state_dict()}, ck)
    env = dict(os.environ)
    cwd = os.path.join(ROOT, "terra-gan_amd")
    common = ["--block", "160", "--tile", "80", "--window", "128", "--overlap", "16"]
    js, pr, ho = (str(tmp_path / n) for n in ("r.json", "pred.asc", "holes.png"))
    run = lambda args: subprocess.run([sys.executable, "-m", "mvp_gan.src.evaluate_raster", "--dem", dem] + args, cwd=cwd,
                                      capture_output=True, text=True, timeout=600, env=env)
    r = run(["--checkpoint", ck, "--json", js, "--pred-out", pr, "--holes-out", ho] + common)
    assert r.returncode == 0, r.stderr
    assert "height RMSE" in r.stdout and os.path.exists(pr) and os.path.exists(ho)
    rep = json.load(open(js))
    js2 = str(tmp_path / "r2.json")
    r = run(["--pred", pr, "--holes", ho, "--json", js2] + common)
    assert r.returncode == 0, r.stderr
    rep2 = json.load(open(js2))
    for k in ("pixels", "height", "slope_deg", "ring", "by_area", "holes"):
        assert json.dumps(rep2[k]) == json.dumps(rep[k]), k
    ej = str(tmp_path / "ev.json")
    r = subprocess.run([sys.executable, "-m", "mvp_gan.src.train_raster", "--dem", dem, "--out", str(tmp_path / "ft.pth"),
                        "--init", ck, "--window", "64", "--batch", "2", "--steps", "1", "--val-steps", "1", "--epochs", "1",
                        "--evaluate", "--eval-json", ej], cwd=cwd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "test split: height RMSE" in r.stdout
    ev = json.load(open(ej))
    assert ev["split"] == "test" and ev["tile"] == 64 and ev["block"] == 256 and ev["pixels"]["holes"] > 0
