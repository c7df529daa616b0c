"""What every raster tool does with its arguments before its first kernel: the host-side checks of a raster and its mask, and
the upload of a numpy array or HIP tensor as a contiguous tensor on the current device.  `who` is the calling tool's name at the
head of every message.  tg_hip is imported inside the functions only: the tools import on a machine without the built library."""
import math

import numpy as np
import torch


# ---- checks ---------------------------------------------------------------------------------------------------------
def shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)


def cellsize(c, who):
    try:
        v = float(c)
    except (TypeError, ValueError):
        v = math.nan
    if not math.isfinite(v) or v <= 0:
        raise ValueError(f"{who}: cellsize {c!r} must be finite and > 0")
    return v


def count(v, lo, name, who):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= 1 << 20:
        raise ValueError(f"{who}: {name} {v!r} must be an integer in [{lo}, 2^20]")
    return v


def bits_f32(b):
    return float(np.array([int(b) & 0xffffffff], np.uint32).view(np.float32)[0])


def nodata_value(nodata):
    """NaN is never a value: non-finite pixels are unknown already."""
    return None if nodata is None or math.isnan(nodata) else float(nodata)


def raster_shape(dem, mask, who, max_side=None, what="dem must be [H, W]"):
    """-> (H, W) of a non-empty 2-D raster with H*W < 2^31 (with max_side: no side above it instead) whose mask, if any, has
    its shape.  `what` opens the message: the tools word it differently."""
    s = shape(dem)
    if len(s) != 2 or min(s) < 1 or (s[0] * s[1] >= 2 ** 31 if max_side is None else max(s) > max_side):
        limit = "H*W < 2^31" if max_side is None else f"sides in [1, {max_side}]"
        raise ValueError(f"{who}: {what} with {limit}, got {s}")
    if mask is not None and shape(mask) != s:
        raise ValueError(f"{who}: mask {shape(mask)} differs from the dem {s}")
    return s


# ---- upload ---------------------------------------------------------------------------------------------------------
def device(who):
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who}: no HIP device visible; this build has no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _on_device(a, what, who):
    if not a.is_cuda:
        raise ValueError(f"{who}: {what} is on {a.device}; pass a numpy array or a HIP tensor")


def to_f32(a, dev, what, who, binary=False):
    """A raster (binary: a mask, nonzero -> 1) as a contiguous float32 tensor on dev."""
    if isinstance(a, torch.Tensor):
        _on_device(a, what, who)
        if binary and a.dtype != torch.float32:
            a = a != 0
        return a.to(device=dev, dtype=torch.float32).contiguous()
    a = np.asarray(a)
    if binary:
        a = a != 0
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def to_u8(a, dev, what, who, nonzero=False, reuse=False):
    """A grid of codes (uint8 as given) or a map (nonzero: any numeric type, nonzero -> 1) as a contiguous uint8 tensor on dev.
    reuse: evaluate_raster's hole maps, as it always took them: a tensor that is one already comes back as it is, without a
    copy (its kernels read nonzero), and a tensor on any other device, the CPU included, is moved."""
    if isinstance(a, torch.Tensor):
        if reuse and a.dtype == torch.uint8 and a.device == dev and a.is_contiguous():
            return a
        if not reuse:
            _on_device(a, what, who)
        a = (a != 0) if nonzero else a
        return a.to(device=dev, dtype=torch.uint8).contiguous()
    a = np.asarray(a)
    a = (a != 0) if nonzero else a
    return torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).to(dev)      # a copy: the input may be read-only


def to_i32(a, dev, what, who):
    """An int32 grid (the caller has checked the type) as a contiguous tensor on dev."""
    if isinstance(a, torch.Tensor):
        _on_device(a, what, who)
        return a.to(device=dev).contiguous()
    return torch.from_numpy(np.array(a, dtype=np.int32, order="C")).to(dev)


def upload(dem, mask, nodata, who):
    """-> (z float32 [H][W], m float32 [H][W] of 0 / 1 or None, nodata or None, the device)."""
    dev = device(who)
    z = to_f32(dem, dev, "dem", who)
    m = None if mask is None else to_f32(mask, dev, "mask", who, binary=True)
    return z, m, nodata_value(nodata), dev


def upload_known(dem, mask, nodata, who):
    """upload, then the known map -> (z float32 [H][W], known uint8 [H][W]: mask != 0, finite and != nodata)."""
    from tg_hip import ops as O
    z, m, nodata, _ = upload(dem, mask, nodata, who)
    return z, O.objmask_known(z, m, nodata, transposed=False)[0]
