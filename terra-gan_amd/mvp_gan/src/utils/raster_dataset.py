"""Training windows sampled on the device from one whole float32 DSM in metres.

The reference trains on uint8 PNG tiles, each min-max scaled over all its pixels (utils/data_extraction.py:96-100): heights
are quantised to 256 levels per tile and the normalisation counts the holes, while inpaint_raster normalises each window
over its known pixels only.  RasterWindowLoader feeds train() straight from the raster instead:

  - a window origin is admissible when every pixel of the window is valid (mask != 0, finite, != nodata), so the target
    is defined everywhere; it is checked in O(1) against an int32 summed-area table of the invalid pixels, and origins
    are drawn by seeded rejection sampling;
  - with `split`, the raster is cut into `block`-sized blocks aligned at (0, 0); block (by, bx) belongs to split
    (bx - by) mod 3 -> train, val, test, and a window lies inside one block of its split, so splits never share a pixel;
  - `augment` draws one of the 8 dihedral transforms per window;
  - synthetic holes are unions of up to HoleSpec.max_prims rotated rectangles, rotated ellipses and thick segments whose
    centres (a segment: its first end point) lie inside the window.  Each primitive is charged an upper bound on the
    pixels it can cover (area + half perimeter + 1 of a convex set; 4 (a+1) (b+1) for the rectangle and the ellipse it
    contains) against a budget of f * window^2, f ~ U(min_fraction, max_fraction), so every window has a hole fraction
    <= max_fraction, at least one hole and at least one known pixel;
  - on the device, tg_hole_masks rasterises the masks and tg_raster_sample cuts the windows and normalises them,
    x = (z - lo) / (hi - lo), with lo / hi over the known pixels (norm="known", the rule of inpaint_raster) or over the
    whole window (norm="window").  x is written at every pixel, holes included: it is the training target; with
    norm="known" hole values may fall outside [0, 1].

With `objects` (an object_mask.ObjectSpec and the raster's cellsize) the above-ground objects are found on the GPU
(mvp_gan/src/object_mask.py) and become invalid pixels before the summed-area table is built: no target window holds a
roof or a tree crown.

Every draw is a pure function of (seed, split, epoch, rank, batch index) through numpy SeedSequence; split "val" and "test"
ignore the epoch, so their loss is comparable across epochs.  Per batch the host draws the parameters, makes one pinned,
double-buffered, non-blocking upload and two library calls.  The only host wait is on the upload of two batches back, before
its pinned buffer is rewritten.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

MIN_SIDE, MAX_SIDE, MAX_PRIMS = 40, 1024, 32
SPLITS = {"train": 0, "val": 1, "test": 2}
KINDS = {"rect": 0, "ellipse": 1, "stroke": 2}        # tg_hole_masks primitive kinds (terragan_hip.h)
NORMS = {"known": 1, "window": 0}
MAX_ROUNDS = 64                                       # rejection-sampling rounds per batch before giving up


@dataclass(frozen=True)
class HoleSpec:
    min_fraction: float = 0.02
    max_fraction: float = 0.30
    kinds: tuple = ("rect", "ellipse", "stroke")
    max_prims: int = 32

    def check(self, window):
        if not 0 < self.min_fraction <= self.max_fraction < 1:
            raise ValueError(f"HoleSpec: need 0 < min_fraction <= max_fraction < 1, got {self.min_fraction}, {self.max_fraction}")
        if self.min_fraction * window * window < 16:
            raise ValueError(f"HoleSpec: min_fraction {self.min_fraction} leaves fewer than 16 hole pixels in a {window}^2 window")
        if not self.kinds or any(k not in KINDS for k in self.kinds):
            raise ValueError(f"HoleSpec: kinds {self.kinds} must be a non-empty subset of {tuple(KINDS)}")
        if not 1 <= self.max_prims <= MAX_PRIMS:
            raise ValueError(f"HoleSpec: max_prims {self.max_prims} out of range [1, {MAX_PRIMS}]")


def prim_bound(prims):
    """Upper bound on the pixels each primitive [..., 8] can cover (int64): 4 (a+1) (b+1) for a rectangle or ellipse,
    ceil(area + half perimeter + 1) + 1 of the capsule for a segment (the + 1 absorbs float64 rounding)."""
    prims = np.asarray(prims, np.int64)
    k = prims[..., 0]
    box = 4 * (prims[..., 3] + 1) * (prims[..., 4] + 1)
    r = prims[..., 5].astype(np.float64)
    ln = np.hypot((prims[..., 3] - prims[..., 1]).astype(np.float64), (prims[..., 4] - prims[..., 2]).astype(np.float64))
    cap = np.ceil(2 * r * ln + math.pi * r * r + ln + math.pi * r + 1).astype(np.int64) + 1
    return np.where(k == KINDS["stroke"], cap, box)


def primitive_draws(rng, n, side, holes):
    """The random part of draw_primitives: every array it draws from `rng`, in the order it draws them."""
    K = holes.max_prims
    d = {"frac": rng.uniform(holes.min_fraction, holes.max_fraction, n)}
    kinds = np.array([KINDS[k] for k in holes.kinds])
    d["kind"] = kinds[rng.integers(0, len(kinds), (n, K))]
    d["share"] = rng.uniform(0.25, 1.0, (n, K))
    d["cy"], d["cx"] = rng.integers(0, side, (n, K)), rng.integers(0, side, (n, K))
    d["aspect"], d["lfrac"], d["rfrac"] = rng.uniform(0.2, 1.0, (n, K)), rng.uniform(0.5, 1.0, (n, K)), rng.uniform(0, 1, (n, K))
    d["ang"] = rng.uniform(0, 2 * math.pi, (n, K))
    d["uv"] = rng.integers(-16, 17, (n, K, 2))
    return d


def fit_primitives(d, side, holes):
    """The deterministic part of draw_primitives, elementwise over the windows: draws of several generators concatenated
    along axis 0 give the concatenation of their results."""
    w, K = side, holes.max_prims
    n = d["frac"].shape[0]
    rem = np.floor(d["frac"] * w * w).astype(np.int64)
    kind, cy, cx = d["kind"], d["cy"], d["cx"]
    aspect, lfrac, rfrac, ang = d["aspect"], d["lfrac"], d["rfrac"], d["ang"]
    share = d["share"].copy()
    share[:, 0] = 1.0                                        # the first primitive may use the whole budget: >= 1 hole
    uv = d["uv"].copy()
    uv[(uv == 0).all(-1)] = (1, 0)
    rmax = max(1, w // 32)
    prims = np.zeros((n, K, 8), np.int64)
    keep = np.zeros((n, K), bool)
    for k in range(K):
        if (rem < 16).all():
            break
        T = np.floor(rem * share[:, k])
        # rectangle / ellipse: 4 (a+1) (b+1) <= T with a, b >= 1
        b1 = np.maximum(2, np.floor(np.sqrt(np.maximum(T, 0) * aspect[:, k] / 4)))
        a1 = np.floor(T / (4 * b1))
        a, b = np.clip(a1 - 1, 0, w - 1), np.clip(b1 - 1, 0, w - 1)
        # segment: r with pi r^2 + pi r + 3 <= T, then a length whose capsule bound stays <= T after rounding the end
        rfit = np.floor((-math.pi + np.sqrt(math.pi ** 2 + 4 * math.pi * np.maximum(T - 3, 0))) / (2 * math.pi))
        r = np.minimum(np.floor(rfrac[:, k] * (rmax + 1)), np.minimum(rmax, rfit))
        lmax = np.maximum(T - math.pi * r * r - math.pi * r - 3, 0) / (2 * r + 1)
        ln = np.maximum(np.minimum(np.floor(lmax * lfrac[:, k]), w) - 1, 0)
        y1 = cy[:, k] + np.round(ln * np.sin(ang[:, k])).astype(np.int64)
        x1 = cx[:, k] + np.round(ln * np.cos(ang[:, k])).astype(np.int64)
        st = kind[:, k] == KINDS["stroke"]
        p = prims[:, k]
        p[:, 0], p[:, 1], p[:, 2] = kind[:, k], cy[:, k], cx[:, k]
        p[:, 3] = np.where(st, y1, a)
        p[:, 4] = np.where(st, x1, b)
        p[:, 5] = np.where(st, r, uv[:, k, 0])
        p[:, 6] = np.where(st, 0, uv[:, k, 1])
        bound = prim_bound(p)
        ok = (T >= 16) & (a1 >= 2) & (bound <= rem)
        keep[:, k] = ok
        rem -= np.where(ok, bound, 0)
    cnt = keep.sum(1)
    if (cnt == 0).any():
        raise RuntimeError("RasterWindowLoader: a window got no hole primitive")   # excluded by HoleSpec.check
    offsets = np.zeros(n + 1, np.int32)
    np.cumsum(cnt, out=offsets[1:])
    return prims[keep].astype(np.int32), offsets


def draw_primitives(rng, n, side, holes):
    """-> (prims int32 [P][8], offsets int32 [n+1]): hole primitives of n windows of side `side` within their budgets, drawn
    from `rng` (RasterWindowLoader's windows, evaluate_raster's cells)."""
    return fit_primitives(primitive_draws(rng, n, side, holes), side, holes)


def _host_f32(a, what):
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise ValueError(f"RasterWindowLoader: {what} is on {a.device}; pass a numpy array or a HIP tensor")
        return a.detach().float().cpu().numpy()
    return np.asarray(a)


class RasterWindowLoader:
    """Iterates {'image', 'mask'} as [B,1,w,w] fp32 device tensors (the ShardLoader contract) plus 'lo', 'hi' [B] in
    metres: image = the normalised window (the target), mask = 1 keep / 0 hole."""

    def __init__(self, dem, mask=None, *, nodata=None, window=256, batch_size=16, steps_per_epoch=None, split=None, block=None,
                 augment=True, norm="known", holes=HoleSpec(), seed=0, rank=0, world=1, device=None, objects=None, cellsize=None,
                 model_cellsize=None, min_coverage=0.5):
        if isinstance(window, (tuple, list)):
            if len(window) != 2 or int(window[0]) != int(window[1]):
                raise ValueError(f"RasterWindowLoader: window {tuple(window)} must be square")
            window = window[0]
        w = self.window = int(window)
        if not MIN_SIDE <= w <= MAX_SIDE:
            raise ValueError(f"RasterWindowLoader: window {w} out of range [{MIN_SIDE}, {MAX_SIDE}]")
        if norm not in NORMS:
            raise ValueError(f"RasterWindowLoader: norm {norm!r} must be one of {tuple(NORMS)}")
        if split is not None and split not in SPLITS:
            raise ValueError(f"RasterWindowLoader: split {split!r} must be None or one of {tuple(SPLITS)}")
        if not 1 <= int(batch_size) <= 65535:
            raise ValueError(f"RasterWindowLoader: batch_size {batch_size} out of range [1, 65535]")
        if not 0 <= int(rank) < int(world):
            raise ValueError(f"RasterWindowLoader: rank {rank} not in [0, world = {world})")
        holes.check(w)
        self.batch_size, self.split, self.augment, self.norm, self.holes = int(batch_size), split, bool(augment), norm, holes
        self.seed, self.rank, self.world, self.epoch = int(seed), int(rank), int(world), 0
        self.block = 4 * w if block is None else int(block)
        if self.block < w:
            raise ValueError(f"RasterWindowLoader: block {self.block} is smaller than the window {w}")

        scale = None
        if model_cellsize is not None:
            from ..inpaint_raster import check_resample_options
            scale = check_resample_options(cellsize, model_cellsize, min_coverage, who="RasterWindowLoader")
        z = _host_f32(dem, "dem")
        if z.ndim != 2:
            raise ValueError(f"RasterWindowLoader: dem must be [H, W], got {z.shape}")
        if scale is None:
            self._check_size(z.shape)
        valid = np.isfinite(z)
        if mask is not None:
            m = _host_f32(mask, "mask")
            if m.shape != z.shape:
                raise ValueError(f"RasterWindowLoader: mask {m.shape} differs from the dem {z.shape}")
            valid &= m != 0
        if nodata is not None and not math.isnan(nodata):
            valid &= z != np.float32(nodata)
        object_fraction = None
        if objects is not None:
            from ..object_mask import object_mask
            obj, _, _ = object_mask(z, None if mask is None else m, nodata=nodata, cellsize=cellsize, spec=objects)
            obj = obj.cpu().numpy() != 0
            object_fraction = float(obj.mean())
            valid &= ~obj
        if scale is not None:
            # the keep mask (valid and no object) goes through the resampling with the raster: once, here; everything below
            # and every window drawn later lives on the working grid
            from ..resample import resample_raster
            with torch.cuda.device(device):                     # None: the current device
                zw, _, _ = resample_raster(z, valid.astype(np.float32), cellsize=cellsize, target_cellsize=model_cellsize,
                                           min_coverage=min_coverage)
            dem = z = zw.cpu().numpy()
            valid = np.isfinite(z)
            self._check_size(z.shape)
        self.H, self.W = H, W = z.shape
        sat = np.zeros((H + 1, W + 1), np.int32)                # invalid pixels above and left of (y, x)
        np.cumsum(np.cumsum(~valid, axis=0, dtype=np.int32), axis=1, dtype=np.int32, out=sat[1:, 1:])
        self._sat = sat
        n_adm, n_org = self._count_admissible()
        if n_adm == 0:
            where = "" if split is None else f" inside one {self.block}-px block of split {split!r}"
            raise ValueError(f"RasterWindowLoader: no admissible {w}x{w} window (every pixel valid){where} in the "
                             f"{H}x{W} raster")
        self.info = {"admissible_origins": n_adm, "origins": n_org, "admissible_fraction": n_adm / n_org,
                     "valid_fraction": float(valid.mean())}
        if object_fraction is not None:
            self.info["object_fraction"] = object_fraction
        self.steps_per_epoch = max(1, -(-n_adm // (w * w * self.batch_size))) if steps_per_epoch is None else int(steps_per_epoch)
        if self.steps_per_epoch < 1:
            raise ValueError(f"RasterWindowLoader: steps_per_epoch {steps_per_epoch} < 1")
        self._cand = int(min(max(64, math.ceil(4 * self.batch_size / self.info["admissible_fraction"])), 1 << 20))

        # device state is set up on first iteration, so that the host side (draws, admissibility) works without a GPU
        self.device, self._dem_in, self.dem = device, dem if isinstance(dem, torch.Tensor) else z, None
        # upload layout (int32): draws [B][3] | offsets [B+1] | primitives [<= B * max_prims][8]
        self._cap = 4 * self.batch_size + 1 + 8 * self.batch_size * holes.max_prims
        self._pin, self._dev, self._ev = None, None, [None, None]

    def _check_size(self, shape):
        H, W = shape
        if self.window > H or self.window > W:
            raise ValueError(f"RasterWindowLoader: window {self.window} is larger than the raster {H}x{W}")
        if (H + 1) * (W + 1) >= 2 ** 31:
            raise ValueError(f"RasterWindowLoader: raster {H}x{W} too large for the int32 summed-area table")

    def _device_setup(self):
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if isinstance(self._dem_in, torch.Tensor):
            self.dem = self._dem_in.detach().to(device=self.device, dtype=torch.float32).contiguous()
        else:
            self.dem = torch.from_numpy(np.ascontiguousarray(self._dem_in, dtype=np.float32)).to(self.device)
        self._dem_in = None
        self._pin = [torch.empty(self._cap, dtype=torch.int32).pin_memory() for _ in range(2)]
        self._dev = [torch.empty(self._cap, dtype=torch.int32, device=self.device) for _ in range(2)]

    # ---- host side: admissibility and draws -------------------------------------------------------------------------------
    def _split_ok(self, y, x):
        """Origins whose window lies inside one block of the split (broadcasting y against x)."""
        if self.split is None:
            return np.ones(np.broadcast(y, x).shape, bool)
        bs, w = self.block, self.window
        by, bx = y // bs, x // bs
        return ((y + w - 1) // bs == by) & ((x + w - 1) // bs == bx) & ((bx - by) % 3 == SPLITS[self.split])

    def admissible(self, y, x):
        """bool: the w x w window at origin (y, x) has only valid pixels and lies inside one block of the split."""
        y, x, w, s = np.asarray(y, np.int64), np.asarray(x, np.int64), self.window, self._sat
        bad = s[y + w, x + w] - s[y, x + w] - s[y + w, x] + s[y, x]
        return (bad == 0) & self._split_ok(y, x)

    def _count_admissible(self):
        w, s = self.window, self._sat
        ny, nx = self.H - w + 1, self.W - w + 1
        xs = np.arange(nx)
        n = 0
        for y0 in range(0, ny, 256):
            y1 = min(y0 + 256, ny)
            bad = s[y0 + w:y1 + w, w:] - s[y0:y1, w:] - s[y0 + w:y1 + w, :nx] + s[y0:y1, :nx]
            n += int(((bad == 0) & self._split_ok(np.arange(y0, y1)[:, None], xs[None, :])).sum())
        return n, ny * nx

    def _rng(self, b):
        ep = self.epoch if self.split in (None, "train") else 0
        tag = 3 if self.split is None else SPLITS[self.split]
        return np.random.Generator(np.random.PCG64(np.random.SeedSequence([self.seed, tag, ep, self.rank, int(b)])))

    def _origins(self, rng, n):
        w, ys, xs = self.window, [], []
        got = 0
        for _ in range(MAX_ROUNDS):
            y = rng.integers(0, self.H - w + 1, self._cand)
            x = rng.integers(0, self.W - w + 1, self._cand)
            ok = self.admissible(y, x)
            ys.append(y[ok]), xs.append(x[ok])
            got += int(ok.sum())
            if got >= n:
                return np.concatenate(ys)[:n], np.concatenate(xs)[:n]
        raise RuntimeError(f"RasterWindowLoader: only {got} of {n} admissible origins after {MAX_ROUNDS} x {self._cand} draws "
                           f"(admissible fraction {self.info['admissible_fraction']:.2e})")

    def _primitives(self, rng, n):
        """-> (prims int32 [P][8], offsets int32 [n+1]): hole primitives of n windows within their budgets."""
        return draw_primitives(rng, n, self.window, self.holes)

    def draw(self, b):
        """Host draws of batch b of the current epoch: {'draws' int32 [B][3] = (y0, x0, op), 'prims' int32 [P][8],
        'offsets' int32 [B+1]}."""
        rng = self._rng(b)
        n = self.batch_size
        y, x = self._origins(rng, n)
        op = rng.integers(0, 8, n) if self.augment else np.zeros(n, np.int64)
        prims, offsets = self._primitives(rng, n)
        return {"draws": np.stack([y, x, op], 1).astype(np.int32), "prims": prims, "offsets": offsets}

    # ---- iteration ------------------------------------------------------------------------------------------------------
    def __len__(self):
        return self.steps_per_epoch

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __iter__(self):
        from tg_hip import ops as O
        if self.dem is None:
            self._device_setup()
        B, w = self.batch_size, self.window
        for bi in range(self.steps_per_epoch):
            d = self.draw(bi)
            P = d["prims"].shape[0]
            used = 4 * B + 1 + 8 * P
            slot = bi & 1
            if self._ev[slot] is not None:
                self._ev[slot].synchronize()         # the upload that last read this pinned buffer has finished
            pin = self._pin[slot].numpy()
            pin[:3 * B] = d["draws"].ravel()
            pin[3 * B:4 * B + 1] = d["offsets"]
            pin[4 * B + 1:used] = d["prims"].ravel()
            dev = self._dev[slot]
            dev[:used].copy_(self._pin[slot][:used], non_blocking=True)
            self._ev[slot] = torch.cuda.Event()
            self._ev[slot].record()
            mask = O.hole_masks(dev[4 * B + 1:used].view(P, 8), dev[3 * B:4 * B + 1], w)
            x, lo, hi = O.raster_sample(self.dem, dev[:3 * B].view(B, 3), mask, NORMS[self.norm])
            yield {"image": x.unsqueeze(1), "mask": mask.unsqueeze(1), "lo": lo, "hi": hi}
