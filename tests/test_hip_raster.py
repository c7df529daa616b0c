"""GPU checks of whole-raster inpainting (csrc/raster.hip, mvp_gan/src/inpaint_raster.py) against the numpy oracle in
tests/raster_oracle.py: stats and gather bit for bit, blend against float64, end to end against inpaint_batch, the
known-pixel and unfilled-hole rules, shift invariance, determinism, batch size and the CLI."""
import math

import numpy as np
import pytest
import torch

from tests import raster_oracle as RO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def G(dev):
    from mvp_gan.src.models import PConvUNet
    torch.manual_seed(5)
    G = PConvUNet()
    g = torch.Generator().manual_seed(6)
    for m in G.modules():                       # non-trivial running statistics
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    return G.to(dev)


def _cp(plan):
    from tg_hip import ops as O
    return O.raster_plan(plan.H, plan.W, plan.wh, plan.ww, plan.overlap, len(plan.ys), len(plan.xs))


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.view(np.int32)


def _tol(z, k):
    """Test 2's bound: 1e-6 max|z| + 1e-6 range of the known heights (fp32 rounding of lo + out (hi - lo) and of the
    weighted mean, each a few ulp of max|z|, against a float64 oracle)."""
    zk = z[k].astype(np.float64)
    return 1e-6 * np.abs(zk).max() + 1e-6 * (zk.max() - zk.min())


def test_stats_and_gather_bitwise(dev):
    """NaN, nodata, an all-hole window, an all-known window and a constant (hi == lo) window."""
    from mvp_gan.src.inpaint_raster import plan_windows
    from tg_hip import ops as O
    H, W = 300, 260
    plan = plan_windows(H, W, 128, 16)                          # ys 0,112,172  xs 0,112,132
    assert (plan.ys, plan.xs) == ([0, 112, 172], [0, 112, 132])
    z = RO.terrain(H, W, 11)
    z[:, 0] = -z[:, 0]                                          # negative heights too
    z[172:, :128] = np.float32(431.25)                          # window (2,0) constant over its known pixels ...
    mask = np.ones((H, W), np.float32)
    mask[:128, :128] = 0                                        # window (0,0): all holes
    hole = RO.disc_holes(172, 132, 0.2, 12, 3, 10)
    mask[:172, :132][hole] = 0
    mask[250, 60] = 0                                           # ... with one hole
    z[150, 200] = np.nan                                        # inside windows (1,1) and (1,2)
    z[140, 100] = np.inf
    z[130, 50] = -9999.0
    z[20, 200] = -9999.0
    nodata = -9999.0
    lo, hi, cnt = O.raster_window_stats(torch.from_numpy(z).to(dev), torch.from_numpy(mask).to(dev), _cp(plan), nodata)
    rlo, rhi, rcnt = RO.stats(z, plan, mask, nodata)
    np.testing.assert_array_equal(cnt.cpu().numpy(), rcnt)
    np.testing.assert_array_equal(_bits(lo.cpu().numpy()), _bits(rlo))
    np.testing.assert_array_equal(_bits(hi.cpu().numpy()), _bits(rhi))
    assert rcnt[0].tolist() == [0, 128 * 128]                   # the all-hole window
    assert rcnt[8][1] == 0                                      # the all-known window (2,2)
    assert rlo[6] == rhi[6] == np.float32(431.25) and rcnt[6][1] == 1
    nwin = len(plan.ys) * len(plan.xs)
    idx = torch.arange(nwin, dtype=torch.int32, device=dev).flip(0).contiguous()
    x, m = O.raster_gather(torch.from_numpy(z).to(dev), torch.from_numpy(mask).to(dev), _cp(plan), lo, hi, idx, nodata)
    rx, rm = RO.gather(z, plan, rlo, rhi, idx.cpu().numpy(), mask, nodata)
    np.testing.assert_array_equal(_bits(x.cpu().numpy()), _bits(rx))
    np.testing.assert_array_equal(m.cpu().numpy(), rm)
    # without mask and nodata: only the non-finite pixels are holes
    lo2, hi2, cnt2 = O.raster_window_stats(torch.from_numpy(z).to(dev), None, _cp(plan))
    rlo2, rhi2, rcnt2 = RO.stats(z, plan)
    np.testing.assert_array_equal(cnt2.cpu().numpy(), rcnt2)
    np.testing.assert_array_equal(_bits(lo2.cpu().numpy()), _bits(rlo2))
    np.testing.assert_array_equal(_bits(hi2.cpu().numpy()), _bits(rhi2))
    x2, m2 = O.raster_gather(torch.from_numpy(z).to(dev), None, _cp(plan), lo2, hi2, idx[:4].contiguous())
    rx2, rm2 = RO.gather(z, plan, rlo2, rhi2, idx[:4].cpu().numpy())
    np.testing.assert_array_equal(_bits(x2.cpu().numpy()), _bits(rx2))
    np.testing.assert_array_equal(m2.cpu().numpy(), rm2)


def test_blend_against_float64(dev):
    from mvp_gan.src.inpaint_raster import plan_windows
    from tg_hip import ops as O
    H, W = 1500, 2100
    plan = plan_windows(H, W, 512, 64)
    nwin = len(plan.ys) * len(plan.xs)
    z = RO.terrain(H, W, 21)
    hole = RO.disc_holes(H, W, 0.3, 22, 10, 60)
    mask = (~hole).astype(np.float32)
    zd, md = torch.from_numpy(z).to(dev), torch.from_numpy(mask).to(dev)
    lo, hi, cnt = O.raster_window_stats(zd, md, _cp(plan))
    rng = np.random.default_rng(23)
    run_of = np.full(nwin, -1, np.int32)
    ran = np.sort(rng.choice(nwin, nwin - 3, replace=False))   # three windows did not run
    run_of[ran] = rng.permutation(ran.size)                     # any row order of the output buffer
    wout = rng.random((ran.size, plan.wh, plan.ww)).astype(np.float32)
    out, unfilled = O.raster_blend(zd, md, _cp(plan), lo, hi, torch.from_numpy(run_of).to(dev), torch.from_numpy(wout).to(dev))
    ref, runf = RO.blend(z, plan, lo.cpu().numpy(), hi.cpu().numpy(), run_of, wout, mask)
    got = out.cpu().numpy()
    k = mask != 0
    np.testing.assert_array_equal(_bits(got[k]), _bits(z[k]))
    assert int(unfilled.item()) == runf
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    f = ~k & ~np.isnan(ref)
    err = np.abs(got[f] - ref[f]).max()
    assert err <= _tol(z, k), (err, _tol(z, k))
    out2, _ = O.raster_blend(zd, md, _cp(plan), lo, hi, torch.from_numpy(run_of).to(dev), torch.from_numpy(wout).to(dev))
    np.testing.assert_array_equal(_bits(out2.cpu().numpy()), _bits(got))


def test_single_window_matches_inpaint_batch(dev, G):
    from mvp_gan.src.evaluate import inpaint_batch
    from mvp_gan.src.inpaint_raster import inpaint_raster, plan_windows
    z = RO.terrain(512, 512, 31)
    mask = (~RO.disc_holes(512, 512, 0.3, 32)).astype(np.float32)
    was = G.training
    out, info = inpaint_raster(G, z, mask)
    assert G.training == was                                    # eval-mode forward without touching the flag
    assert info == {"windows": 1, "run": 1, "unfilled": 0}
    plan = plan_windows(512, 512)
    lo, hi, _ = RO.stats(z, plan, mask)
    x, m = RO.gather(z, plan, lo, hi, [0], mask)
    o = inpaint_batch(G, torch.from_numpy(x[:, None]).to(dev), torch.from_numpy(m[:, None]).to(dev))
    o = o.cpu().numpy()[0, 0].astype(np.float64)
    ref = np.where(mask != 0, z, float(lo[0]) + o * (float(hi[0]) - float(lo[0])))
    got = out.cpu().numpy()
    assert out.dtype == torch.float32 and out.is_cuda and got.shape == (512, 512)
    np.testing.assert_array_equal(_bits(got[mask != 0]), _bits(z[mask != 0]))
    err = np.abs(got - ref).max()
    assert err <= 1e-6 * (float(hi[0]) - float(lo[0])), err


def test_known_pixels_and_unfilled_holes(dev, G):
    from mvp_gan.src.inpaint_raster import inpaint_raster, plan_windows
    H, W = 600, 640
    plan = plan_windows(H, W, 256, 32)                          # ys 0,224,344
    assert plan.ys == [0, 224, 344] and plan.xs[1] == 224
    z = RO.terrain(H, W, 41)
    mask = (~RO.disc_holes(H, W, 0.15, 42, 5, 20)).astype(np.float32)
    mask[:256, :256] = 0                                        # window (0,0) has no known pixel: it does not run
    z[400, 500] = np.nan                                        # non-finite and nodata pixels are holes too
    z[410, 30] = -32768.0
    out, info = inpaint_raster(G, torch.from_numpy(z).to(dev), torch.from_numpy(mask).to(dev), nodata=-32768.0,
                               window=256, overlap=32, batch=4)
    got = out.cpu().numpy()
    k = RO.known(z, mask, -32768.0)
    _, _, cnt = RO.stats(z, plan, mask, -32768.0)
    assert cnt[0][0] == 0 and info["run"] == int(((cnt[:, 0] > 0) & (cnt[:, 1] > 0)).sum())
    np.testing.assert_array_equal(_bits(got[k]), _bits(z[k]))
    only00 = np.zeros((H, W), bool)
    only00[:224, :224] = True                                   # covered by window (0,0) alone
    np.testing.assert_array_equal(np.isnan(got), only00)
    assert info["unfilled"] == 224 * 224 and info["windows"] == 9 and info["run"] >= 7
    assert np.isfinite(got[400, 500]) and np.isfinite(got[410, 30])


def test_shift_invariance(dev, G):
    from mvp_gan.src.inpaint_raster import inpaint_raster
    z = RO.terrain(700, 900, 51, base=20.0, relief=80.0)
    mask = (~RO.disc_holes(700, 900, 0.3, 52)).astype(np.float32)
    a, _ = inpaint_raster(G, z, mask)
    b, _ = inpaint_raster(G, z + np.float32(1000), mask)
    a, b = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64) - 1000
    k = mask != 0
    rng_ = float(z[k].max() - z[k].min())
    err = np.abs(a - b).max()
    assert err <= 1e-4 * rng_, (err, rng_)


def test_determinism_and_batch_size(dev, G):
    from mvp_gan.src.inpaint_raster import inpaint_raster
    z = RO.terrain(1100, 1000, 61)
    mask = (~RO.disc_holes(1100, 1000, 0.3, 62)).astype(np.float32)
    a, ia = inpaint_raster(G, z, mask, batch=8)
    b, ib = inpaint_raster(G, z, mask, batch=8)
    assert ia == ib and ia["run"] == 9 and ia["unfilled"] == 0
    np.testing.assert_array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    c, ic = inpaint_raster(G, z, mask, batch=1)
    assert ic == ia
    k = mask != 0
    err = np.abs(a.cpu().numpy().astype(np.float64) - c.cpu().numpy()).max()
    assert err <= _tol(z, k), (err, _tol(z, k))


def test_cli_asc_in_asc_out(dev, G, tmp_path):
    from mvp_gan.src.asc import read_asc, write_asc
    from mvp_gan.src.inpaint_raster import main
    H, W = 120, 100
    z = RO.terrain(H, W, 71)
    z[RO.disc_holes(H, W, 0.2, 72, 3, 8)] = -9999.0
    hdr = [("ncols", str(W)), ("nrows", str(H)), ("xllcorner", "400000.0"), ("yllcorner", "300000.0"), ("cellsize", "2"),
           ("NODATA_value", "-9999")]
    write_asc(tmp_path / "in.asc", z, hdr)
    torch.save({"generator_state_dict": G.state_dict()}, tmp_path / "g.pth")
    info = main(["--dem", str(tmp_path / "in.asc"), "--checkpoint", str(tmp_path / "g.pth"), "--out", str(tmp_path / "out.asc"),
                 "--window", "64", "--overlap", "16", "--batch", "3"])
    assert info["windows"] == 6 and info["run"] == 6 and info["unfilled"] == 0
    got, hdr2 = read_asc(tmp_path / "out.asc")
    assert hdr2 == hdr
    k = z != -9999.0
    np.testing.assert_array_equal(_bits(got[k]), _bits(z[k]))
    assert (got[~k] != -9999.0).all() and np.isfinite(got).all()
    assert (got[~k] > 700).all() and (got[~k] < 1100).all()     # filled in metres, inside the windows' ranges
    m = np.full((H, W + 1), 255, np.uint8)
    from PIL import Image
    Image.fromarray(m, mode="L").save(tmp_path / "m.png")
    with pytest.raises(ValueError, match="no resizing"):
        main(["--dem", str(tmp_path / "in.asc"), "--mask", str(tmp_path / "m.png"), "--checkpoint", str(tmp_path / "g.pth"),
              "--out", str(tmp_path / "o2.asc")])


def test_shared_upload(dev):
    """mvp_gan/src/raster_args.py: the upload every raster tool opens with, on a 5x7 raster with one NaN pixel, one nodata
    pixel and one masked pixel."""
    from mvp_gan.src import raster_args as R
    from tg_hip import ops as O
    z = (np.arange(35, dtype=np.float32).reshape(5, 7) * np.float32(1.1) - 7).astype(np.float32)
    z[0, 0] = -0.0
    z[1, 2] = np.nan
    z[3, 4] = -9999.0
    mask = np.ones((5, 7), np.uint8)
    mask[2, 5] = 0
    mask[4, 1] = 7                                              # any nonzero value is 1
    bits = lambda t: t.view(torch.int32)
    za, ma, nd, d = R.upload(z, mask, -9999, "test")
    assert d == torch.device("cuda", torch.cuda.current_device()) and nd == -9999.0 and type(nd) is float
    assert za.dtype == ma.dtype == torch.float32 and za.is_contiguous() and ma.is_contiguous() and za.device == ma.device == d
    np.testing.assert_array_equal(_bits(za.cpu().numpy()), _bits(z))
    np.testing.assert_array_equal(ma.cpu().numpy(), (mask != 0).astype(np.float32))
    wide = torch.zeros(5, 14, dtype=torch.float32, device=dev)
    wide[:, ::2] = torch.from_numpy(z).to(dev)
    view = wide[:, ::2]                                         # the same dem as a non-contiguous HIP tensor view
    assert not view.is_contiguous()
    zb, mb, ndb, _ = R.upload(view, torch.from_numpy(mask).to(dev), math.nan, "test")
    assert ndb is None and zb.is_contiguous() and torch.equal(bits(zb), bits(za)) and torch.equal(bits(mb), bits(ma))
    for other in (mask != 0, mask.astype(np.float32), torch.from_numpy(mask != 0).to(dev),
                  torch.from_numpy((mask != 0).astype(np.float32)).to(dev)):
        assert torch.equal(bits(R.upload(z, other, None, "test")[1]), bits(ma))        # uint8, bool and float32 masks agree
    assert R.upload(z, None, None, "test")[1] is None
    zk, known = R.upload_known(z, mask, -9999, "test")
    want, _ = O.objmask_known(za, ma, -9999.0, transposed=False)
    assert known.dtype == torch.uint8 and torch.equal(known, want) and torch.equal(bits(zk), bits(za))
    k = np.ones((5, 7), np.uint8)
    k[1, 2] = k[3, 4] = k[2, 5] = 0
    np.testing.assert_array_equal(known.cpu().numpy(), k)
    # a uint8 map on the device is read where it lies (evaluate_raster's holes); anything else is converted
    h = torch.from_numpy(mask).to(dev)
    assert R.to_u8(h, dev, "holes", "test", nonzero=True, reuse=True).data_ptr() == h.data_ptr()
    fresh = R.to_u8(h, dev, "holes", "test", nonzero=True)
    assert fresh.data_ptr() != h.data_ptr() and fresh.cpu().tolist() == (mask != 0).astype(np.uint8).tolist()
    strided = torch.zeros(5, 14, dtype=torch.uint8, device=dev)[:, ::2]
    assert R.to_u8(strided, dev, "holes", "test", nonzero=True, reuse=True).is_contiguous()
    moved = R.to_u8(torch.from_numpy(mask), dev, "holes", "test", nonzero=True, reuse=True)     # a CPU tensor: moved, not refused
    assert moved.device == d and torch.equal(moved, fresh)
    with pytest.raises(ValueError, match="^test: dem is on cpu; pass a numpy array or a HIP tensor$"):
        R.upload(torch.from_numpy(z), None, None, "test")
