"""CPU checks of test-time augmentation in inpaint_raster: the numpy mirrors of
tests/raster_tta_oracle.py, the argument checks that need no GPU, the host-side refusals of the new tg_raster_* entry points,
the parsers, and the sensitivity condition of the GPU equivariance test on the oracle's generator."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import raster_oracle as RO
from tests import raster_tta_oracle as TO


@pytest.mark.parametrize("shape,ops", [((5, 7), (0, 1, 2, 3)), ((6, 6), TO.OPS)])
def test_inverse_undoes_transform(shape, ops):
    x = np.arange(shape[0] * shape[1], dtype=np.float32).reshape(shape)
    for op in ops:
        t = TO.transform(x, op)
        assert t.shape == (shape if not op & 4 else shape[::-1])
        np.testing.assert_array_equal(TO.inverse(t, op), x)
        np.testing.assert_array_equal(TO.transform(TO.inverse(x, op), op), x)
        # the encoding itself, pixel by pixel
        for i in range(t.shape[0]):
            for j in range(t.shape[1]):
                a, b = (j, i) if op & 4 else (i, j)
                a = shape[0] - 1 - a if op & 2 else a
                b = shape[1] - 1 - b if op & 1 else b
                assert t[i, j] == x[a, b], (op, i, j)


def test_transforms_pairwise_different():
    x = np.arange(36, dtype=np.float32).reshape(6, 6)
    frames = [TO.transform(x, op) for op in TO.OPS]
    for p in range(8):
        for q in range(p + 1, 8):
            assert not np.array_equal(frames[p], frames[q]), (p, q)


def integer_frames(wh, ww, T):
    """base[i][j] = i ww + j; member t = transform(base, op_t) + t: mean base + (T - 1) / 2, squared deviations sum to 42, 5, 0.5."""
    base = np.arange(wh * ww, dtype=np.float32).reshape(wh, ww)
    return base, np.stack([TO.transform(base, op) + np.float32(t) for t, op in enumerate(TO.OPS[:T])])[None]


VAR_EXACT = {2: np.float32(0.5), 4: np.float32(5) / np.float32(3), 8: np.float32(6)}


@pytest.mark.parametrize("wh,ww,T", [(72, 72, 2), (72, 72, 4), (72, 72, 8), (100, 128, 2), (100, 128, 4)])
def test_mirror_reduce_closed_forms(wh, ww, T):
    base, g = integer_frames(wh, ww, T)
    mean, var = TO.reduce(g, TO.OPS[:T])
    assert mean.dtype == var.dtype == np.float32 and mean.shape == var.shape == (1, wh, ww)
    np.testing.assert_array_equal(mean[0], base + np.float32((T - 1) / 2))
    np.testing.assert_array_equal(var[0], np.full((wh, ww), VAR_EXACT[T]))


def test_tta_argument_checks_without_gpu():
    from mvp_gan.src.inpaint_raster import inpaint_raster, inpaint_raster_tta
    z = np.zeros((128, 128), np.float32)
    for bad in (3, 0, 16, True, 2.5, None):
        with pytest.raises(ValueError, match="tta"):
            inpaint_raster(None, z, tta=bad)
    with pytest.raises(ValueError, match="tta"):
        inpaint_raster_tta(None, z, tta=1)
    with pytest.raises(ValueError, match="tta=4"):
        inpaint_raster(None, np.zeros((100, 300), np.float32), window=128, tta=8)
    with pytest.raises(ValueError, match="tta=4"):
        inpaint_raster_tta(None, np.zeros((100, 300), np.float32), window=128)
    with pytest.raises(ValueError, match="tta=4"):                  # the windows run on the working grid: 200x600 at scale 2
        inpaint_raster(None, np.zeros((200, 600), np.float32), window=128, tta=8, cellsize=1.0, model_cellsize=2.0)


def test_library_refuses_on_the_host():
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    lib = L.load()
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails validation first
    plan = L.TgRasterPlan(100, 300, 100, 128, 16, 1, 3)
    ops = (C.c_int32 * 3)(0, 3, 4)
    rc = lib.tg_raster_gather_ops(fake, None, C.byref(plan), 0, 0.0, fake, fake, fake, ops, 3, fake, fake, None)
    assert rc == -1 and b"square" in lib.tg_last_error(), lib.tg_last_error()
    ops = (C.c_int32 * 2)(1, 8)
    rc = lib.tg_raster_gather_ops(fake, None, C.byref(plan), 0, 0.0, fake, fake, fake, ops, 2, fake, fake, None)
    assert rc == -1 and b"out of range" in lib.tg_last_error()
    rc = lib.tg_raster_gather_ops(fake, None, C.byref(plan), 0, 0.0, fake, fake, fake, None, 2, fake, fake, None)
    assert rc == -1 and b"null pointer" in lib.tg_last_error()
    ops = (C.c_int32 * 2)(0, 4)
    rc = lib.tg_raster_tta_reduce(fake, ops, 2, 1, 100, 128, fake, fake, None)
    assert rc == -1 and b"square" in lib.tg_last_error(), lib.tg_last_error()
    ops = (C.c_int32 * 3)(0, 1, 2)
    rc = lib.tg_raster_tta_reduce(fake, ops, 3, 1, 128, 128, fake, fake, None)
    assert rc == -1 and b"must be 2, 4 or 8" in lib.tg_last_error()
    rc = lib.tg_raster_blend_tta(fake, None, C.byref(plan), 0, 0.0, fake, fake, fake, fake, None, 2, fake, fake, fake, None)
    assert rc == -1 and b"null pointer" in lib.tg_last_error()


def test_parsers():
    from mvp_gan.src import evaluate_raster as ER
    from mvp_gan.src import inpaint_raster as IR
    base = ["--dem", "a.asc", "--checkpoint", "g.pth", "--out", "o.asc"]
    assert IR.parse_args(base).tta == 1 and IR.parse_args(base).spread_out is None
    a = IR.parse_args(base + ["--tta", "4", "--spread-out", "s.asc"])
    assert a.tta == 4 and a.spread_out == "s.asc"
    for argv in (base + ["--spread-out", "s.asc"], base + ["--tta", "1", "--spread-out", "s.asc"], base + ["--tta", "3"]):
        with pytest.raises(SystemExit):
            IR.parse_args(argv)
    ap = ER.build_parser()
    assert ap.parse_args(["--dem", "a.asc", "--checkpoint", "g.pth", "--tta", "4"]).tta == 4
    assert ap.parse_args(["--dem", "a.asc", "--checkpoint", "g.pth"]).tta == 1
    with pytest.raises(SystemExit):
        ap.parse_args(["--dem", "a.asc", "--checkpoint", "g.pth", "--tta", "5"])


def test_untrained_generator_is_not_equivariant():
    """The sensitivity condition of the GPU equivariance test: with one member (tta=1) the fill of a transformed raster,
    mapped back, differs from the fill of the raster by far more than the bound that test allows, here with the oracle's
    generator (randomly initialised, eval mode) on the same single-window setting."""
    from mvp_gan.src.inpaint_raster import plan_windows
    from oracle import terragan_oracle as Orc
    z = RO.terrain(128, 128, 81)
    mask = (~RO.disc_holes(128, 128, 0.3, 82, 5, 20)).astype(np.float32)
    plan = plan_windows(128, 128, 128, 16)
    lo, hi, _ = RO.stats(z, plan, mask)
    x, m = RO.gather(z, plan, lo, hi, [0], mask)
    torch.manual_seed(5)
    P = Orc.init_generator()

    def fill(op):
        with torch.no_grad():
            xt, mt = (torch.from_numpy(TO.transform(a, op))[:, None] for a in (x, m))
            return TO.inverse(Orc.generator_forward(P, xt, mt, training=False)[:, 0].numpy(), op)[0].astype(np.float64)

    k = mask != 0
    zk = z[k].astype(np.float64)
    bound = 1e-6 * np.abs(zk).max() + 1e-6 * (zk.max() - zk.min())      # _tol of tests/test_hip_raster.py
    ref = fill(0)
    for op in (1, 4, 7):
        diff = np.abs(fill(op) - ref)[~k].max() * (float(hi[0]) - float(lo[0]))
        print(f"op {op}: tta=1 fills differ by {diff:.4g} m, {diff / bound:.3g} x the bound {bound:.3g} m")
        assert diff > 100 * bound, (op, diff, bound)
