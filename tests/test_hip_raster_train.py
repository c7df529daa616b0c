"""GPU checks of training from a whole raster (csrc/raster_train.hip, mvp_gan/src/utils/raster_dataset.py) against the
numpy oracle in tests/raster_train_oracle.py: hole masks and sampled windows bit for bit, determinism, a train step fed by
the loader against one fed with the oracle's tensors, train() end to end with a validation loader, and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import raster_oracle as RO
from tests import raster_train_oracle as TO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _rand_prims(rng, side, n, per):
    """n windows of `per` random primitives of every kind, many of them partly outside the window."""
    prims = []
    for _ in range(n * per):
        k = int(rng.integers(0, 3))
        cy, cx = rng.integers(-side, 2 * side + 1, 2)
        if k == TO.STROKE:
            y1, x1 = rng.integers(-side, 2 * side + 1, 2) if rng.random() < 0.5 else (cy + rng.integers(-20, 21),
                                                                                       cx + rng.integers(-20, 21))
            prims.append([k, cy, cx, y1, x1, rng.integers(0, side // 8 + 1), 0, 0])
        else:
            u, v = rng.integers(-16, 17, 2)
            a, b = rng.integers(0, side // 3 + 1, 2)
            prims.append([k, cy, cx, a, b, u, v, 0])
    return np.array(prims, np.int32), (np.arange(n + 1) * per).astype(np.int32)


@pytest.mark.parametrize("side,n,per", [(40, 6, 32), (256, 4, 32), (1024, 2, 32), (100, 5, 3)])
def test_hole_masks_bitwise(dev, side, n, per):
    from tg_hip import ops as O
    rng = np.random.default_rng(side + per)
    prims, off = _rand_prims(rng, side, n, per)
    prims[0] = [TO.RECT, side // 2, side // 2, 5, 3, 0, 0, 0]          # direction (0, 0): covers nothing
    prims[1] = [TO.ELLIPSE, side // 2, side // 2, 0, 9, 3, 1, 0]       # a = 0: covers nothing
    prims[2] = [TO.STROKE, 3, 4, 3, 4, 6, 0, 0]                        # zero-length segment: a disc
    ref = TO.hole_masks(prims, off, side)
    got = O.hole_masks(torch.from_numpy(prims).to(dev), torch.from_numpy(off).to(dev), side).cpu().numpy()
    np.testing.assert_array_equal(_bits(got), _bits(ref))
    assert 0 < (ref == 0).mean() < 1
    # uneven counts, an empty window, more than 32 listed (only the first 32 are used)
    off2 = np.array([0, 0, 5, 5 + 33 if len(prims) >= 38 else len(prims)], np.int32)
    off2[-1] = min(off2[-1], len(prims))
    ref2 = TO.hole_masks(prims, off2, side)
    got2 = O.hole_masks(torch.from_numpy(prims).to(dev), torch.from_numpy(off2).to(dev), side).cpu().numpy()
    np.testing.assert_array_equal(_bits(got2), _bits(ref2))
    assert (ref2[0] == 1).all()


def test_hole_masks_from_loader_draws_bitwise(dev):
    from mvp_gan.src.utils.raster_dataset import RasterWindowLoader
    from tg_hip import ops as O
    L = RasterWindowLoader(RO.terrain(600, 600, 4), window=128, batch_size=16, seed=3)
    for b in range(3):
        d = L.draw(b)
        ref = TO.hole_masks(d["prims"], d["offsets"], 128)
        got = O.hole_masks(torch.from_numpy(d["prims"]).to(dev), torch.from_numpy(d["offsets"]).to(dev), 128).cpu().numpy()
        np.testing.assert_array_equal(_bits(got), _bits(ref))


def _sample_case(side=96, H=300, W=260, seed=1):
    rng = np.random.default_rng(seed)
    z = RO.terrain(H, W, seed)
    z[:, :40] = -z[:, :40]                                        # negative heights, and a -0
    z[7, 7] = np.float32(-0.0)
    z[200:, 160:] = np.float32(512.5)                             # a flat corner
    draws = [[y, x, op] for op in range(8) for y, x in ((0, 0), (H - side, W - side), (13, 71))]
    draws += [[H - side, W - side - 100, 3], [204, 164, 5]]       # the second one flat
    draws += [[5, 5, 0], [5, 5, 6]]                               # their extremes under holes (below)
    draws = np.array(draws, np.int32)
    n = len(draws)
    mask = (rng.random((n, side, side)) > 0.2).astype(np.float32)
    mask[-1] = 1
    mask[-2] = 1
    for w in (-2, -1):                                            # holes over the window's min and max
        y0, x0, op = draws[w]
        win = TO.transform(z[y0:y0 + side, x0:x0 + side], op)
        mask[w][np.unravel_index(win.argmin(), win.shape)] = 0
        mask[w][np.unravel_index(win.argmax(), win.shape)] = 0
    mask[4, :, :] = 0                                             # nothing known: lo = +inf, hi = -inf, x = 0
    return z, draws, mask


@pytest.mark.parametrize("norm_known", [1, 0])
def test_raster_sample_bitwise(dev, norm_known):
    from tg_hip import ops as O
    z, draws, mask = _sample_case()
    xr, lr, hr = TO.sample(z, draws, mask, norm_known)
    zd = torch.from_numpy(z).to(dev)
    x, lo, hi = O.raster_sample(zd, torch.from_numpy(draws).to(dev), torch.from_numpy(mask).to(dev), norm_known)
    np.testing.assert_array_equal(_bits(lo.cpu().numpy()), _bits(lr))
    np.testing.assert_array_equal(_bits(hi.cpu().numpy()), _bits(hr))
    np.testing.assert_array_equal(_bits(x.cpu().numpy()), _bits(xr))
    assert (xr[-3] == 0).all() and lr[-3] == hr[-3]               # flat window
    if norm_known:
        assert np.isinf(lr[4]) and (xr[4] == 0).all()
        assert xr[-2].min() < 0 and xr[-2].max() > 1              # hole targets leave [0, 1]
    else:
        assert xr[-2].min() == 0 and xr[-2].max() == 1
    # the known-pixel rule differs from the window rule exactly where an extreme is under a hole
    _, lo2, _ = O.raster_sample(zd, torch.from_numpy(draws).to(dev), torch.from_numpy(mask).to(dev), 1 - norm_known)
    assert lo2[-2].item() != lo[-2].item()


def test_raster_sample_at_sizes_and_rejected_draws(dev):
    """Sides 40 and 1024 (partial and many tiles); draws that leave the raster or carry a bad op get NaN and do not read
    outside it."""
    from tg_hip import ops as O
    for side, H, W in ((40, 41, 90), (1024, 1100, 1030)):
        rng = np.random.default_rng(side)
        z = RO.terrain(H, W, side)
        draws = np.array([[0, 0, 7], [H - side, W - side, 4], [1, 2, 1], [-1, 0, 0], [0, W - side + 1, 2], [0, 0, 8],
                          [H - side + 1, 0, 0], [0, -5, 3]], np.int32)
        mask = (rng.random((len(draws), side, side)) > 0.3).astype(np.float32)
        xr, lr, hr = TO.sample(z, draws, mask, 1)
        x, lo, hi = O.raster_sample(torch.from_numpy(z).to(dev), torch.from_numpy(draws).to(dev),
                                    torch.from_numpy(mask).to(dev))
        np.testing.assert_array_equal(_bits(x.cpu().numpy()), _bits(xr))
        np.testing.assert_array_equal(_bits(lo.cpu().numpy()), _bits(lr))
        np.testing.assert_array_equal(_bits(hi.cpu().numpy()), _bits(hr))
        assert np.isnan(xr[3:]).all() and np.isfinite(xr[:3]).all()


def test_kernels_deterministic(dev):
    from tg_hip import ops as O
    from mvp_gan.src.utils.raster_dataset import RasterWindowLoader
    z = RO.terrain(1500, 1400, 9)
    L = RasterWindowLoader(z, window=256, batch_size=16, seed=1)
    d = L.draw(0)
    p, off, dr = (torch.from_numpy(d[k]).to(dev) for k in ("prims", "offsets", "draws"))
    zd = torch.from_numpy(z).to(dev)
    outs = []
    for _ in range(2):
        m = O.hole_masks(p, off, 256)
        outs.append((m,) + O.raster_sample(zd, dr, m))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _models(dev, seed=0):
    from mvp_gan.src.models import Discriminator, PConvUNet
    from mvp_gan.src.utils.losses import InpaintingLoss
    torch.manual_seed(seed)
    G, D = PConvUNet().to(dev), Discriminator().to(dev)
    crit = InpaintingLoss(0.1, 0.1, device=torch.device("cpu")).to(dev)
    return G, D, crit, torch.optim.Adam(G.parameters(), lr=2e-4), torch.optim.Adam(D.parameters(), lr=2e-4)


def test_loader_batch_and_train_step_match_oracle(dev):
    from mvp_gan.src.train import train_step
    from mvp_gan.src.utils.raster_dataset import RasterWindowLoader
    z = RO.terrain(700, 640, 12)
    z[100:110, 50:600] = np.nan
    L = RasterWindowLoader(z, window=128, batch_size=4, steps_per_epoch=2, split="train", block=320, seed=5, device=dev)
    L.set_epoch(1)
    batches = list(L)
    assert len(batches) == 2 == len(L)
    d = L.draw(1)
    mask = TO.hole_masks(d["prims"], d["offsets"], 128)
    x, lo, hi = TO.sample(z, d["draws"], mask, 1)
    b = batches[1]
    assert b["image"].shape == (4, 1, 128, 128) and b["mask"].shape == (4, 1, 128, 128) and b["image"].is_cuda
    np.testing.assert_array_equal(_bits(b["mask"][:, 0].cpu().numpy()), _bits(mask))
    np.testing.assert_array_equal(_bits(b["image"][:, 0].cpu().numpy()), _bits(x))
    np.testing.assert_array_equal(_bits(b["lo"].cpu().numpy()), _bits(lo))
    np.testing.assert_array_equal(_bits(b["hi"].cpu().numpy()), _bits(hi))
    assert np.isfinite(x).all() and (mask == 0).any()
    outs = []
    for real, msk in ((b["image"], b["mask"]), (torch.from_numpy(x)[:, None].to(dev), torch.from_numpy(mask)[:, None].to(dev))):
        G, D, crit, oG, oD = _models(dev)
        G.train(), D.train()
        o = train_step(G, D, crit, oG, oD, real, msk)
        outs.append((o["gen"].clone(), float(o["g_total"]), float(o["d_loss"]), next(G.parameters()).detach().clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1:3] == outs[1][1:3] and torch.equal(outs[0][3], outs[1][3])


def test_train_end_to_end_from_raster(dev, tmp_path):
    from mvp_gan.src.inpaint_raster import inpaint_raster
    from mvp_gan.src.train import train
    from mvp_gan.src.utils.raster_dataset import RasterWindowLoader
    z = RO.terrain(640, 640, 21)
    kw = dict(window=128, batch_size=4, steps_per_epoch=2, block=160, seed=2, device=dev)
    tr, va = RasterWindowLoader(z, split="train", **kw), RasterWindowLoader(z, split="val", augment=False, **kw)
    G, D, _, oG, oD = _models(dev, 3)
    w0 = {k: v.detach().clone() for k, v in G.state_dict().items()}
    cfg = {"training": {"batch_size": 99, "learning_rate": 2e-4, "epochs": 2, "loss_weights": {"perceptual": 0.1, "tv": 0.1}}}
    ck = tmp_path / "ft.pth"
    res = train(tr, None, generator=G, discriminator=D, optimizer_G=oG, optimizer_D=oD, checkpoint_path=ck, config=cfg,
                val_img_dir=va)
    assert res["final_epoch"] == 1 and tr.epoch == 1
    assert np.isfinite(res["best_val_loss"])
    c = torch.load(ck, map_location="cpu", weights_only=False)
    assert {"epoch", "generator_state_dict", "discriminator_state_dict", "optimizer_G_state_dict", "optimizer_D_state_dict",
            "g_loss", "d_loss", "config", "val_g_loss", "val_d_loss"} <= set(c)
    assert np.isfinite([c["g_loss"], c["d_loss"], c["val_g_loss"], c["val_d_loss"]]).all()
    moved = [k for k, v in G.state_dict().items() if v.is_floating_point() and not torch.equal(v, w0[k])]
    assert len(moved) > 10
    mask = ~RO.disc_holes(300, 280, 0.1, 3, 4, 12)
    out, info = inpaint_raster(str(ck), z[:300, :280], mask, window=128, overlap=16)
    assert info["run"] > 0 and info["unfilled"] == 0 and torch.isfinite(out).all()


def test_cli_end_to_end(dev, tmp_path):
    from mvp_gan.src.asc import write_asc
    z = RO.terrain(330, 330, 8)
    z[10, 10] = -9999
    hdr = [("ncols", "330"), ("nrows", "330"), ("xllcorner", "0"), ("yllcorner", "0"), ("cellsize", "1"),
           ("NODATA_value", "-9999")]
    write_asc(tmp_path / "in.asc", z, hdr)
    env = dict(os.environ, TERRAGAN_ALLOW_STANDIN_VGG="1")
    cwd = os.path.join(ROOT, "terra-gan_amd")
    opts = ["--window", "64", "--batch", "2", "--steps", "2", "--epochs", "1", "--block", "110"]

    def run(*args):
        r = subprocess.run([sys.executable, "-m", *args], cwd=cwd, capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout

    out = run("mvp_gan.src.train_raster", "--dem", str(tmp_path / "in.asc"), "--out", str(tmp_path / "a.pth"), *opts)
    assert "init random" in out
    out = run("mvp_gan.src.train_raster", "--dem", str(tmp_path / "in.asc"), "--init", str(tmp_path / "a.pth"), "--out",
              str(tmp_path / "b.pth"), *opts)
    assert "init generator+discriminator+optimizer_G+optimizer_D" in out
    run("mvp_gan.src.inpaint_raster", "--dem", str(tmp_path / "in.asc"), "--checkpoint", str(tmp_path / "b.pth"), "--out",
        str(tmp_path / "o.asc"), "--window", "64", "--overlap", "8")
    assert (tmp_path / "o.asc").exists()
