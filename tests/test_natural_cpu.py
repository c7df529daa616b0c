"""CPU checks of the natural-neighbour void fill (csrc/natural.hip, mvp_gan/src/natural.py): the numpy
oracle in tests/natural_oracle.py against the definition and its consequences, the host-side rejections, the C ABI and the
parsers.  Nothing here needs a GPU."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import idw_oracle as IO
from tests import natural_oracle as NO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.asarray(a, np.float32).view(np.int32)


def _scene(H, W, p, seed):
    rng = np.random.default_rng(seed)
    z = (1000.0 + rng.normal(0, 20.0, (H, W))).astype(np.float32)
    return z, (rng.random((H, W)) < p).astype(np.uint8)


def _same(a, b):
    for x, y in zip(a, b):
        if isinstance(x, list):
            assert x == y
        elif x.dtype == np.float32:
            np.testing.assert_array_equal(_bits(x), _bits(y))
        else:
            np.testing.assert_array_equal(x, y)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2, 3, 8, 32])
@pytest.mark.parametrize("lim2", [0, 2])
def test_vectorised_oracle_is_the_brute_force(radius, lim2):
    z, known = _scene(9, 11, 0.15, 5)
    assert 0 < known.sum() < 30
    _same(NO.natural(z, known, radius, lim2), NO.natural_brute(z, known, radius, lim2))
    one = np.zeros((9, 11), np.uint8)
    one[7, 2] = 1
    _same(NO.natural(z, one, radius, lim2), NO.natural_brute(z, one, radius, lim2))


def test_the_1x5_example():
    """[10, ., ., ., 20]: the centre (c = 4) ties and goes to the left site, so it hands 10 to itself and to both neighbours;
    the neighbours (c = 1) keep theirs to themselves."""
    z = np.array([[10, 0, 0, 0, 20]], np.float32)
    known = np.array([[1, 0, 0, 0, 1]], np.uint8)
    for fn in (NO.natural, NO.natural_brute):
        for radius in (2, 3, 32):
            out, support, counts, lo, hi = fn(z, known, radius)
            assert out.tolist() == [[10.0, 10.0, 10.0, 15.0, 20.0]]
            assert support.tolist() == [[0, 2, 1, 2, 0]] and counts == [3, 0]
            assert lo[0, 1:4].tolist() == [10.0, 10.0, 10.0] and hi[0, 1:4].tolist() == [10.0, 10.0, 20.0]
        out, support, counts, _, _ = fn(z, known, 1)
        assert out.tolist() == [[10.0, 10.0, 10.0, 20.0, 20.0]] and support.tolist() == [[0, 1, 1, 1, 0]]


def test_radius_one_is_the_nearest_fill():
    for H, W, p, seed in ((9, 11, 0.15, 6), (40, 31, 0.05, 7)):
        z, known = _scene(H, W, p, seed)
        out, support, counts, lo, hi = NO.natural(z, known, 1)
        want, wc = IO.gather_fill(z, known, IO.nearest(known)[1])
        np.testing.assert_array_equal(_bits(out), _bits(want))
        assert counts == wc and (support == (known == 0)).all()


def test_constant_field_and_bounds():
    z, known = _scene(40, 31, 0.05, 8)
    flat = np.full_like(z, 1234.5678)
    for radius in (2, 5, 32):
        out, support, counts, _, _ = NO.natural(flat, known, radius)
        assert (out == flat).all() and counts == [int((known == 0).sum()), 0]
        out, support, counts, lo, hi = NO.natural(z, known, radius)
        v = known == 0
        assert (lo[v] <= out[v]).all() and (out[v] <= hi[v]).all() and (support[v] >= 1).all()
        assert np.isnan(lo[~v]).all() and (support[~v] == 0).all()
        np.testing.assert_array_equal(_bits(out[~v]), _bits(z[~v]))
    assert (NO.natural(z, known, 32)[0] != NO.natural(z, known, 1)[0]).any()


def test_one_seed_radius_8_support_193():
    """Deep inside a void the fill is the nearest fill over the open disc of the radius: 193 lattice points with
    dy^2 + dx^2 < 64."""
    z, _ = _scene(40, 45, 0.5, 9)
    known = np.zeros((40, 45), np.uint8)
    known[20, 22] = 1
    out, support, counts, lo, hi = NO.natural(z, known, 8)
    assert sum(1 for dy in range(-7, 8) for dx in range(-7, 8) if dy * dy + dx * dx < 64) == 193
    assert support.max() == 193 and support[8, 8] == 193 and support[0, 0] < 193
    assert counts == [40 * 45 - 1, 0] and (out[known == 0] == z[20, 22]).all()


def test_none_known_and_limit():
    z, known = _scene(9, 11, 0.15, 5)
    out, support, counts, _, _ = NO.natural(z, np.zeros_like(known), 4)
    assert np.isnan(out).all() and counts == [0, 99]
    d2, _ = IO.nearest(known)
    free = NO.natural(z, known, 4)[0]
    out, support, counts, _, _ = NO.natural(z, known, 4, lim2=2)
    far = (known == 0) & (d2 > 2)
    assert far.any() and np.isnan(out[far]).all() and counts == [int(((known == 0) & ~far).sum()), int(far.sum())]
    np.testing.assert_array_equal(_bits(out[~far]), _bits(free[~far]))


# ---- host-side rejections ------------------------------------------------------------------------------------------------------
def test_check_args_rejections():
    from mvp_gan.src.natural import MAX_RADIUS, check_args, natural_neighbour_voids
    dem = np.zeros((8, 9), np.float32)
    assert MAX_RADIUS == 32
    assert check_args(dem, None, 32, None, 1.0) == (8, 9, 1.0, 32, 0)
    assert check_args(dem, np.ones((8, 9)), np.int64(5), 3.0, 2.0) == (8, 9, 2.0, 5, 2)
    for radius in (0, 33, 2.5, True, "8", None, -1):
        with pytest.raises(ValueError, match="radius"):
            check_args(dem, None, radius, None, 1.0)
        with pytest.raises(ValueError, match="radius"):
            natural_neighbour_voids(dem, radius=radius)
    with pytest.raises(ValueError, match="shorter than one cell"):
        check_args(dem, None, 8, 0.5, 1.0)
    with pytest.raises(ValueError, match="shorter than one cell"):
        natural_neighbour_voids(dem, max_distance=1.9, cellsize=2.0)
    for md in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_distance"):
            check_args(dem, None, 8, md, 1.0)
    with pytest.raises(ValueError, match="mask"):
        check_args(dem, np.ones((9, 8)), 8, None, 1.0)
    with pytest.raises(ValueError, match="mask"):
        natural_neighbour_voids(dem, np.ones((8, 8)))
    with pytest.raises(ValueError, match="cellsize"):
        check_args(dem, None, 8, None, 0.0)
    with pytest.raises(ValueError, match="support"):
        check_args(dem, None, 8, None, 1.0, support=1)
    for bad in (np.zeros((3,), np.float32), np.zeros((0, 4), np.float32), np.zeros((2, 32768), np.float32)):
        with pytest.raises(ValueError, match="natural_neighbour_voids"):
            check_args(bad, None, 8, None, 1.0)


def test_no_cpu_path(monkeypatch):
    import torch
    from mvp_gan.src.natural import natural_neighbour_voids
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        natural_neighbour_voids(np.zeros((8, 9), np.float32))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_build_list_and_host_side_rejections():
    hdr = open(os.path.join(ROOT, "include", "terragan_hip.h")).read()
    assert "size_t tg_natural_fill_ws_bytes(int H, int W);" in hdr and "int tg_natural_fill(const float* nn" in hdr
    build = open(os.path.join(ROOT, "terra-gan_amd", "build.py")).read()
    assert '"natural.hip"' in build and os.path.exists(os.path.join(ROOT, "terra-gan_amd", "csrc", "natural.hip"))
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    from tg_hip import ops as O
    lib = L.load()
    for s in ("tg_natural_fill_ws_bytes", "tg_natural_tile_maxima", "tg_natural_fill"):
        assert hasattr(lib, s) and s in L.SIGNATURES
    q = lib.tg_natural_fill_ws_bytes
    assert q(0, 5) == q(5, 0) == q(-1, 5) == q(32768, 5) == q(5, 32768) == 0
    th, tw = O.NATURAL_TILE
    for H, W in ((1, 1), (th, tw), (th + 1, tw + 1), (300, 1), (1, 300), (8192, 8192), (32767, 32767)):
        assert q(H, W) >= 2 * (-(-H // th)) * (-(-W // tw)) and q(H, W) % 256 == 0
    p = C.c_void_p(256)                                      # never dereferenced: every call below is rejected on the host
    ws = q(70, 90)
    call = lambda nn=p, d2=p, known=p, H=70, W=90, radius=8, out=C.c_void_p(512), counts=p, w=p, nbytes=ws: \
        lib.tg_natural_fill(nn, d2, known, H, W, radius, 0, out, None, counts, w, nbytes, None)
    for kw, msg in ((dict(nn=None), b"null pointer"), (dict(d2=None), b"null pointer"), (dict(known=None), b"null pointer"),
                    (dict(out=None), b"null pointer"), (dict(counts=None), b"null pointer"), (dict(w=None), b"null pointer"),
                    (dict(H=0), b"sides"), (dict(W=32768), b"sides"), (dict(radius=0), b"radius"), (dict(radius=33), b"radius"),
                    (dict(nbytes=ws - 1), b"workspace"), (dict(out=p), b"alias")):
        assert call(**kw) == -1 and msg in lib.tg_last_error(), (kw, lib.tg_last_error())
    assert lib.tg_natural_tile_maxima(None, 70, 90, 8, p, ws, None) == -1 and b"null pointer" in lib.tg_last_error()
    assert lib.tg_natural_tile_maxima(p, 70, 90, 40, p, ws, None) == -1 and b"radius" in lib.tg_last_error()
    assert lib.tg_natural_tile_maxima(p, 70, 90, 8, p, 0, None) == -1 and b"workspace" in lib.tg_last_error()


def test_ops_reject_before_any_launch():
    import torch
    from tg_hip import lib as L
    from tg_hip import ops as O
    z = torch.zeros(4, 4)
    with pytest.raises(L.TgError):
        O.natural_fill(z, torch.zeros(4, 4, dtype=torch.int32), torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(L.TgError):
        O.natural_fill(np.zeros((4, 4), np.float32), None, None)
    with pytest.raises(L.TgError):
        O.natural_tile_maxima(torch.zeros(4, 4, dtype=torch.int32))


# ---- the public surface ------------------------------------------------------------------------------------------------------------
def test_signatures_and_untouched_ladders():
    from mvp_gan.src import evaluate_raster as ER
    from mvp_gan.src.interpolate import METHODS
    from mvp_gan.src.natural import natural_neighbour_voids
    assert METHODS == ER.COMPARES == ("idw", "nearest")
    sig = inspect.signature(natural_neighbour_voids).parameters
    assert list(sig) == ["dem", "mask", "nodata", "cellsize", "radius", "max_distance", "support"]
    assert (sig["radius"].default, sig["max_distance"].default, sig["support"].default, sig["cellsize"].default) == \
        (32, None, False, 1.0)
    for fn in (ER.evaluate_raster, ER._evaluate):
        ps = inspect.signature(fn).parameters
        assert ps["natural"].default is False and ps["natural_radius"].default == 32
    assert callable(ER.natural_report) and "radius" in inspect.signature(ER.natural_report).parameters
    assert ER._check_natural(None) is False and ER._check_natural(False) is False and ER._check_natural(True) is True
    with pytest.raises(ValueError, match="natural"):
        ER._check_natural(8)


def test_cli_parsers():
    from mvp_gan.src.evaluate_raster import build_parser as eval_parser
    from mvp_gan.src.natural import build_parser
    a = build_parser().parse_args(["--dem", "in.asc", "--out", "o.asc"])
    assert (a.dem, a.out, a.mask, a.nodata, a.radius, a.max_distance, a.support_out) == ("in.asc", "o.asc", None, None, 32, None, None)
    a = build_parser().parse_args(["--dem", "in.asc", "--out", "o.asc", "--mask", "m.png", "--nodata", "-9999", "--radius", "8",
                                   "--max-distance", "50", "--support-out", "s.asc"])
    assert (a.mask, a.nodata, a.radius, a.max_distance, a.support_out) == ("m.png", -9999.0, 8, 50.0, "s.asc")
    for bad in (["--dem", "in.asc"], ["--dem", "in.asc", "--out", "o.asc", "--radius", "2.5"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(bad)
    for base in (["--dem", "in.asc", "--checkpoint", "g.pth"], ["--dem", "in.asc", "--pred", "p.asc", "--holes", "h.png"]):
        a = eval_parser().parse_args(base)
        assert a.natural is False and a.natural_radius == 32
        a = eval_parser().parse_args(base + ["--natural", "--natural-radius", "8"])
        assert a.natural is True and a.natural_radius == 8
    r = subprocess.run([sys.executable, "-m", "mvp_gan.src.natural", "--help"], cwd=os.path.join(ROOT, "terra-gan_amd"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--support-out" in r.stdout and "--radius" in r.stdout
