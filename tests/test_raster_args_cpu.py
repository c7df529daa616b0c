"""CPU checks of what the raster tools share: the argument checks and the upload of mvp_gan/src/raster_args.py (onto the CPU
device, which a numpy input may go to) and the pieces of mvp_gan/src/asc.py that every tool's main() opens and closes with."""
import argparse
import math

import numpy as np
import pytest
import torch

from mvp_gan.src import asc
from mvp_gan.src import raster_args as R

CPU = torch.device("cpu")


def test_shape_of_list_array_tensor():
    assert R.shape([[1, 2, 3], [4, 5, 6]]) == (2, 3)
    assert R.shape(np.zeros((4, 5))) == (4, 5)
    s = R.shape(torch.zeros(6, 7))
    assert s == (6, 7) and type(s) is tuple
    assert R.shape(3.0) == ()


@pytest.mark.parametrize("bad", [0, -1, math.nan, math.inf, None, "x"])
def test_cellsize_rejects(bad):
    with pytest.raises(ValueError, match=r"^some_tool: cellsize .* must be finite and > 0$"):
        R.cellsize(bad, "some_tool")


def test_cellsize_returns_float():
    c = R.cellsize("2.5", "t")
    assert c == 2.5 and type(c) is float
    assert R.cellsize(np.float32(0.5), "t") == 0.5


def test_nodata_value():
    assert R.nodata_value(None) is None
    assert R.nodata_value(math.nan) is None
    v = R.nodata_value(-9999)
    assert v == -9999.0 and type(v) is float


def test_raster_shape():
    assert R.raster_shape(np.zeros((1, 1)), None, "t") == (1, 1)
    assert R.raster_shape(np.zeros((3, 4)), np.ones((3, 4), bool), "t") == (3, 4)
    for bad in (np.zeros(5), np.zeros((2, 3, 4)), np.zeros((0, 4)), np.zeros((4, 0))):
        with pytest.raises(ValueError, match=r"^t: dem must be \[H, W\] with H\*W < 2\^31, got "):
            R.raster_shape(bad, None, "t")
    with pytest.raises(ValueError, match=r"^t: mask \(4, 3\) differs from the dem \(3, 4\)$"):
        R.raster_shape(np.zeros((3, 4)), np.zeros((4, 3)), "t")
    huge = np.broadcast_to(np.float32(0), (1 << 16, 1 << 15))                # H*W = 2^31, no memory behind it
    with pytest.raises(ValueError, match=r"H\*W < 2\^31"):
        R.raster_shape(huge, None, "t")
    assert R.raster_shape(huge, None, "t", max_side=1 << 16) == huge.shape   # max_side replaces the area limit
    assert R.raster_shape(np.zeros((4, 3)), None, "t", max_side=4) == (4, 3)
    with pytest.raises(ValueError, match=r"^t: dem must be \[H, W\] with sides in \[1, 4\], got \(5, 3\)$"):
        R.raster_shape(np.zeros((5, 3)), None, "t", max_side=4)
    with pytest.raises(ValueError, match=r"^t: direction must be \[H, W\], non-empty with H\*W < 2\^31, got \(5,\)$"):
        R.raster_shape(np.zeros(5), None, "t", what="direction must be [H, W], non-empty")


def test_bits_f32():
    assert R.bits_f32(0x3f800000) == 1.0
    neg0 = R.bits_f32(0x80000000)
    assert neg0 == 0.0 and math.copysign(1.0, neg0) == -1.0
    assert math.copysign(1.0, R.bits_f32(np.int32(-2 ** 31))) == -1.0        # the same bits read from an int32 counter
    assert R.bits_f32(np.array([1.5], np.float32).view(np.int32)[0]) == 1.5


def test_to_f32_numpy_onto_cpu():
    t = R.to_f32(np.arange(6, dtype=np.float64).reshape(2, 3) / 3, CPU, "dem", "t")
    assert t.dtype == torch.float32 and t.shape == (2, 3) and t.is_contiguous()
    np.testing.assert_array_equal(t.numpy(), (np.arange(6, dtype=np.float64).reshape(2, 3) / 3).astype(np.float32))
    f = np.asfortranarray(np.arange(15, dtype=np.float32).reshape(3, 5))
    assert not f.flags.c_contiguous
    t = R.to_f32(f, CPU, "dem", "t")
    assert t.is_contiguous() and t.stride() == (5, 1)
    np.testing.assert_array_equal(t.numpy(), f)
    t = R.to_f32(np.array([0, 2, -1, np.nan]), CPU, "mask", "t", binary=True)
    assert t.dtype == torch.float32 and t.tolist() == [0.0, 1.0, 1.0, 1.0]
    ro = np.arange(4, dtype=np.float32)
    ro.setflags(write=False)
    assert R.to_f32(ro, CPU, "dem", "t").tolist() == [0.0, 1.0, 2.0, 3.0]
    assert R.to_f32([[1, 2]], CPU, "dem", "t").tolist() == [[1.0, 2.0]]


def test_cpu_tensors_are_refused():
    x = torch.zeros(2, 2)
    with pytest.raises(ValueError, match=r"^some_tool: dem is on cpu; pass a numpy array or a HIP tensor$"):
        R.to_f32(x, CPU, "dem", "some_tool")
    with pytest.raises(ValueError, match=r"^some_tool: mask is on cpu; pass a numpy array or a HIP tensor$"):
        R.to_f32(x, CPU, "mask", "some_tool", binary=True)
    for kw in ({}, {"nonzero": True}):
        with pytest.raises(ValueError, match=r"^some_tool: holes is on cpu; pass a numpy array or a HIP tensor$"):
            R.to_u8(x.to(torch.uint8), CPU, "holes", "some_tool", **kw)
    with pytest.raises(ValueError, match=r"^some_tool: accumulation is on cpu; pass a numpy array or a HIP tensor$"):
        R.to_i32(x.to(torch.int32), CPU, "accumulation", "some_tool")


def test_to_u8_and_to_i32_numpy_onto_cpu():
    codes = np.array([[0, 9], [255, 3]], np.uint8)
    t = R.to_u8(codes, CPU, "direction", "t")
    assert t.dtype == torch.uint8 and t.tolist() == [[0, 9], [255, 3]]       # codes as given
    t = R.to_u8(np.array([[0.0, 0.5], [-3.0, np.nan]]), CPU, "pour_points", "t", nonzero=True)
    assert t.dtype == torch.uint8 and t.tolist() == [[0, 1], [1, 1]]
    ro = np.asfortranarray(np.arange(6, dtype=np.uint8).reshape(2, 3))
    ro.setflags(write=False)
    t = R.to_u8(ro, CPU, "direction", "t")
    assert t.is_contiguous() and t.tolist() == [[0, 1, 2], [3, 4, 5]]
    assert R.to_u8(np.array([True, False]), CPU, "holes", "t", nonzero=True).tolist() == [1, 0]
    # reuse, evaluate_raster's hole maps: a tensor on any device is taken, a contiguous uint8 one on dev is returned itself
    h = torch.tensor([[0.0, 2.0], [-1.0, 0.0]])
    t = R.to_u8(h, CPU, "holes", "t", nonzero=True, reuse=True)
    assert t.dtype == torch.uint8 and t.tolist() == [[0, 1], [1, 0]]
    h8 = torch.tensor([[0, 7], [1, 0]], dtype=torch.uint8)
    assert R.to_u8(h8, CPU, "holes", "t", nonzero=True, reuse=True) is h8
    t = R.to_u8(h8.t(), CPU, "holes", "t", nonzero=True, reuse=True)
    assert t.is_contiguous() and t.tolist() == [[0, 1], [1, 0]]
    a = R.to_i32(np.asfortranarray(np.array([[1, -2], [3, 2 ** 31 - 1]], np.int32)), CPU, "accumulation", "t")
    assert a.dtype == torch.int32 and a.is_contiguous() and a.tolist() == [[1, -2], [3, 2 ** 31 - 1]]


def test_count():
    assert R.count(1, 1, "check_every", "t") == 1 and R.count(1 << 20, 1, "max_sweeps", "t") == 1 << 20
    for bad in (0, (1 << 20) + 1, True, 2.0, None):
        with pytest.raises(ValueError, match=r"^t: check_every .* must be an integer in \[1, 2\^20\]$"):
            R.count(bad, 1, "check_every", "t")


def test_device_without_gpu():
    if torch.cuda.is_available():
        assert R.device("t") == torch.device("cuda", torch.cuda.current_device())
    else:
        with pytest.raises(RuntimeError, match=r"^some_tool: no HIP device visible; this build has no CPU path$"):
            R.device("some_tool")
        with pytest.raises(RuntimeError, match="^some_tool: no HIP device"):
            R.upload(np.zeros((2, 2)), None, None, "some_tool")


def test_with_nodata():
    base = [("ncols", "4"), ("nrows", "3"), ("xllcorner", "0"), ("yllcorner", "0"), ("cellsize", "1")]
    for key in ("NODATA_value", "nodata_value", "NODATA_VALUE"):
        h = base + [(key, "-1")]
        assert asc.with_nodata(h) is h
    out = asc.with_nodata(base)
    assert out == base + [("NODATA_value", "-9999")] and out is not base and len(base) == 5


def _grid(tmp_path, nodata_line=True):
    z = np.arange(12, dtype=np.float32).reshape(3, 4)
    z[1, 2] = -9999
    hdr = [("ncols", "4"), ("nrows", "3"), ("xllcorner", "10"), ("yllcorner", "20"), ("cellsize", "2.5")]
    if nodata_line:
        hdr.append(("NODATA_value", "-9999"))
    asc.write_asc(tmp_path / "dem.asc", z, hdr)
    return z, hdr


def test_read_inputs(tmp_path):
    z, hdr = _grid(tmp_path)
    ap = argparse.ArgumentParser()
    ap.add_argument("--dem")
    ap.add_argument("--mask")
    ap.add_argument("--nodata", type=float)
    dem, header, mask, nodata, cellsize = asc.read_inputs(ap.parse_args(["--dem", str(tmp_path / "dem.asc")]))
    np.testing.assert_array_equal(dem, z)
    assert dem.dtype == np.float32 and header == hdr and mask is None
    assert nodata == -9999.0 and cellsize == 2.5 and type(cellsize) is float
    assert asc.read_inputs(ap.parse_args(["--dem", str(tmp_path / "dem.asc"), "--nodata", "7"]))[3] == 7.0
    assert asc.read_inputs(ap.parse_args(["--dem", str(tmp_path / "dem.asc"), "--nodata", "0"]))[3] == 0.0   # 0 is a value
    assert asc.read_inputs(argparse.Namespace(dem=str(tmp_path / "dem.asc")))[2:4] == (None, -9999.0)    # no mask, no nodata flag
    _grid(tmp_path, nodata_line=False)
    assert asc.read_inputs(ap.parse_args(["--dem", str(tmp_path / "dem.asc")]))[3] is None
    assert asc.read_inputs(ap.parse_args(["--dem", str(tmp_path / "dem.asc"), "--nodata", "-1"]))[3] == -1.0


def test_read_inputs_mask(tmp_path):
    _, hdr = _grid(tmp_path)
    mk = np.array([[0, 1, 2, 0], [1, 0, 0, 5], [0, 0, 1, 1]], np.float32)
    asc.write_asc(tmp_path / "mask.asc", mk, hdr[:5])
    a = argparse.Namespace(dem=str(tmp_path / "dem.asc"), mask=str(tmp_path / "mask.asc"), nodata=None)
    mask = asc.read_inputs(a)[2]
    assert mask.dtype == bool
    np.testing.assert_array_equal(mask, mk != 0)
    wrong = [("ncols", "3"), ("nrows", "4")] + hdr[2:5]
    asc.write_asc(tmp_path / "wrong.asc", mk.T, wrong)
    a.mask = str(tmp_path / "wrong.asc")
    with pytest.raises(ValueError, match=r"is 4x3, the raster 3x4 \(no resizing\)"):
        asc.read_inputs(a)
