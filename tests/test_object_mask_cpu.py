"""CPU checks of the object detector (mvp_gan/src/object_mask.py, csrc/objmask.hip): the numpy oracle against brute force and
scipy, the radius / threshold schedule and unit conversions, and host-side rejection by the C entry points and the Python
API, all without a GPU."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import objmask_oracle as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spiral(H, W):
    """A one-pixel-wide spiral path whose rings are two pixels apart (one 8-connected component)."""
    a = np.zeros((H, W), bool)
    t, lft, b, rgt = 0, 0, H - 1, W - 1
    while t <= b and lft <= rgt:
        if lft > 0:
            a[t, lft - 1] = True                       # joins the previous ring's left column
        a[t, lft:rgt + 1] = True
        a[t:b + 1, rgt] = True
        if b > t:
            a[b, lft:rgt + 1] = True
        if rgt > lft:
            a[t + 2:b + 1, lft] = True
        t, lft, b, rgt = t + 2, lft + 2, b - 2, rgt - 2
    return a


@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (9, 1), (7, 11), (16, 5)])
@pytest.mark.parametrize("r", [0, 1, 2, 3, 6, 20])
def test_oracle_morph_against_brute_force(H, W, r):
    rng = np.random.default_rng(H * 100 + W + r)
    z = rng.normal(0, 5, (H, W)).astype(np.float32)
    known = rng.random((H, W)) > 0.35
    for op in (np.minimum, np.maximum):
        np.testing.assert_array_equal(OR.morph(z, known, r, op), OR.morph_brute(z, known, r, op))


def test_oracle_components_small_cases():
    f = np.array([[1, 0, 0, 1],
                  [0, 1, 0, 1],
                  [0, 0, 0, 0],
                  [1, 1, 0, 1]], bool)
    lab = OR.components(f)
    assert lab.tolist() == [[0, -1, -1, 3], [-1, 0, -1, 3], [-1, -1, -1, -1], [12, 12, -1, 15]]
    cb = (np.indices((9, 13)).sum(0) % 2 == 0)
    assert (OR.components(cb)[cb] == 0).all()                      # a checkerboard is one 8-connected component
    sp = spiral(41, 57)
    lab = OR.components(sp)
    assert sp.sum() > 41 * 57 // 3 and (lab[sp] == 0).all()
    assert (OR.components(np.zeros((5, 5), bool)) == -1).all()


def test_oracle_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    z = rng.normal(0, 3, (97, 131)).astype(np.float32)
    for r in (1, 4, 17, 200):
        k = 2 * r + 1
        np.testing.assert_array_equal(OR.morph(z, np.ones(z.shape, bool), r, np.minimum), ndi.grey_erosion(z, (k, k), mode="nearest"))
        np.testing.assert_array_equal(OR.morph(z, np.ones(z.shape, bool), r, np.maximum), ndi.grey_dilation(z, (k, k), mode="nearest"))
    for p in (0.3, 0.45, 0.6):
        f = rng.random((200, 257)) < p
        sl, n = ndi.label(f, structure=np.ones((3, 3)))
        idx = np.arange(f.size).reshape(f.shape)
        mins = np.asarray(ndi.minimum(idx, sl, index=np.arange(1, n + 1)), np.int64)
        np.testing.assert_array_equal(OR.components(f), np.where(sl > 0, mins[np.maximum(sl - 1, 0)], -1))


def test_oracle_opening_below_surface_and_quality():
    from mvp_gan.src.object_mask import ObjectSpec, schedule
    z, truth = OR.scene(512, 512, 2, buildings=25, trees=50)
    known = OR.known_map(z)
    known[100:140, 200:260] = False
    radii, dh, ma, bp = schedule(ObjectSpec(), 1.0)
    s = z
    for r in radii:
        d = OR.morph(OR.morph(s, known, r, np.minimum), known, r, np.maximum)
        assert (d[known] <= s[known]).all()                        # open_r(s) <= s at every known pixel
        s = d
    o, keep, counts, flags, _, _ = OR.object_mask(z, known, radii, dh, ma, bp)
    assert ((o != 0) & truth & known).sum() >= 0.99 * (truth & known).sum()
    assert counts[3] == o.sum() and counts[0] == flags.sum()
    np.testing.assert_array_equal(keep, (known & (o == 0)).astype(np.float32))


def test_schedule_and_units():
    from mvp_gan.src.object_mask import ObjectSpec, schedule
    radii, dh, ma, bp = schedule(ObjectSpec(), 1.0)
    assert radii == [1, 2, 4, 8, 16, 32] and ma == 4 and bp == 1
    assert dh.dtype == np.float32
    want = [0.3] + [min(0.15 * (2 * r - 2 * q) * 1.0 + 0.3, 2.5) for q, r in zip(radii[:-1], radii[1:])]
    np.testing.assert_array_equal(dh, np.array(want, np.float64).astype(np.float32))
    radii, dh, ma, bp = schedule(ObjectSpec(), 0.5)                # 0.5 m cells: r_max = 64, 16 px per 4 m^2, 2 px buffer
    assert radii == [1, 2, 4, 8, 16, 32, 64] and ma == 16 and bp == 2
    assert dh[1] == np.float32(0.15 * 2 * 0.5 + 0.3)
    radii, _, ma, bp = schedule(ObjectSpec(max_size_m=50.0, min_area_m2=5.0, buffer_m=2.5), 2.0)
    assert radii == [1, 2, 4, 8, 13] and ma == 2 and bp == 1       # ceil(50 / 4) = 13, ceil(5 / 4), floor(1.25 + 0.5)
    assert schedule(ObjectSpec(buffer_m=1.5), 1.0)[3] == 2         # half away from zero
    assert schedule(ObjectSpec(max_size_m=0.0), 1.0)[0] == [0]
    assert schedule(ObjectSpec(max_size_m=2.0), 1.0)[0] == [1]


@pytest.mark.parametrize("bad", [dict(slope=-0.1), dict(dh0=math.nan), dict(dhmax=math.inf), dict(min_area_m2=-1.0),
                                 dict(buffer_m=-0.5), dict(max_size_m=math.nan), dict(dh0=3.0, dhmax=2.5)])
def test_python_rejects_bad_spec(bad):
    from mvp_gan.src.object_mask import ObjectSpec, object_mask, schedule
    with pytest.raises(ValueError):
        schedule(ObjectSpec(**bad), 1.0)
    with pytest.raises(ValueError):                                 # before any device work
        object_mask(np.zeros((8, 8), np.float32), cellsize=1.0, spec=ObjectSpec(**bad))


@pytest.mark.parametrize("cellsize", [0.0, -1.0, math.nan, math.inf, None, "x"])
def test_python_rejects_bad_cellsize(cellsize):
    from mvp_gan.src.object_mask import ObjectSpec, object_mask
    with pytest.raises(ValueError, match="cellsize"):
        object_mask(np.zeros((8, 8), np.float32), cellsize=cellsize)
    with pytest.raises(ValueError, match="buffer"):
        object_mask(np.zeros((8, 8), np.float32), cellsize=0.01, spec=ObjectSpec(buffer_m=1.0))   # 100 px > 64


def test_python_rejects_bad_shape():
    from mvp_gan.src.object_mask import object_mask
    with pytest.raises(ValueError, match="H, W"):
        object_mask(np.zeros((2, 3, 4), np.float32), cellsize=1.0)
    with pytest.raises(ValueError, match="H, W"):
        object_mask(np.zeros((0, 4), np.float32), cellsize=1.0)


def test_c_entry_points_reject_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    lib = L.load()
    f = C.c_void_p(0x1000)               # never dereferenced: every call below fails validation first
    g = C.c_void_p(0x2000)
    h = C.c_void_p(0x3000)
    k = C.c_void_p(0x4000)

    def err(rc, msg):
        assert rc == -1 and msg in lib.tg_last_error(), (rc, lib.tg_last_error())

    for H, W in ((0, 5), (5, 0), (-1, 5), (1 << 16, 1 << 15)):
        err(lib.tg_objmask_known(f, None, H, W, 0, 0.0, g, None, None), b"H*W < 2^31")
        err(lib.tg_objmask_morph(f, None, H, W, 1, 0, g, h, None), b"H*W < 2^31")
        err(lib.tg_objmask_pmf_step(f, g, h, H, W, 1, 0.5, k, C.c_void_p(0x5000), C.c_void_p(0x6000), C.c_void_p(0x7000), None),
            b"H*W < 2^31")
        err(lib.tg_objmask_components(f, H, W, g, h, None), b"H*W < 2^31")
        err(lib.tg_objmask_filter(f, g, h, H, W, 4, 1, k, C.c_void_p(0x5000), C.c_void_p(0x6000), None), b"H*W < 2^31")
    err(lib.tg_objmask_known(None, None, 4, 4, 0, 0.0, g, None, None), b"null pointer")
    err(lib.tg_objmask_known(f, None, 4, 4, 0, 0.0, None, None, None), b"null pointer")
    err(lib.tg_objmask_morph(f, None, 4, 4, -1, 0, g, h, None), b"radius")
    err(lib.tg_objmask_morph(f, None, 4, 4, 1, 2, g, h, None), b"op 2")
    err(lib.tg_objmask_morph(f, None, 4, 4, 1, 0, None, h, None), b"null pointer")
    err(lib.tg_objmask_morph(f, None, 4, 4, 1, 0, g, f, None), b"distinct")
    p5, p6, p7 = C.c_void_p(0x5000), C.c_void_p(0x6000), C.c_void_p(0x7000)
    err(lib.tg_objmask_pmf_step(f, g, h, 4, 4, -2, 0.5, k, p5, p6, p7, None), b"radius")
    for dh in (-0.5, math.nan, math.inf):
        err(lib.tg_objmask_pmf_step(f, g, h, 4, 4, 1, dh, k, p5, p6, p7, None), b"threshold")
    err(lib.tg_objmask_pmf_step(f, g, None, 4, 4, 1, 0.5, k, p5, p6, p7, None), b"null pointer")
    err(lib.tg_objmask_pmf_step(f, g, h, 4, 4, 1, 0.5, k, k, p6, p7, None), b"distinct")
    err(lib.tg_objmask_components(f, 4, 4, None, h, None), b"null pointer")
    err(lib.tg_objmask_filter(f, g, h, 4, 4, -1, 1, k, p5, p6, None), b"min_area")
    err(lib.tg_objmask_filter(f, g, h, 4, 4, 4, 65, k, p5, p6, None), b"buffer")
    err(lib.tg_objmask_filter(f, g, h, 4, 4, 4, -1, k, p5, p6, None), b"buffer")
    err(lib.tg_objmask_filter(f, g, h, 4, 4, 4, 1, k, p5, None, None), b"null pointer")


def test_clis_list_the_object_flags_without_gpu():
    for mod, extra in (("mvp_gan.src.object_mask", ("--dem", "--out", "--mask", "--objects-out")),
                       ("mvp_gan.src.inpaint_raster", ("--remove-objects", "--objects-out")),
                       ("mvp_gan.src.train_raster", ("--remove-objects",))):
        r = subprocess.run([sys.executable, "-m", mod, "--help"], cwd=os.path.join(ROOT, "terra-gan_amd"), capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        for flag in extra + ("--max-size", "--slope", "--dh0", "--dhmax", "--min-area", "--buffer"):
            assert flag in r.stdout, (mod, flag)
