"""Inputs shared by tests/test_pointwise_oracle_cpu.py (is the fp64 oracle right?) and tests/test_hip_pointwise.py (are the kernels
right by the oracle?): the same shapes, masks and option combinations in both, built with numpy from fixed seeds as fp32 arrays.
Also the plain fp32 PyTorch-CPU formulas that give the GPU tests their fp32 baseline e(cpu32)."""
import functools

import numpy as np
import torch

from tests import pointwise_oracle as PO

F32_EPS = 2.0 ** -24                # unit roundoff of fp32


def f32(x):
    """A Python float that fp32 holds exactly: weights and scalars go to the kernel (float arguments) and to the fp64 oracle
    as the same number."""
    return float(np.float32(x))


# ---- pixel losses --------------------------------------------------------------------------------------------------------
PL_SHAPES = [(1, 2, 2), (1, 2, 300), (1, 300, 2), (2, 33, 17), (3, 257, 129),
             (2, 513, 260),          # 131 reduction blocks: the finalize loop takes a second trip
             (1, 1500, 1400)]        # above the 1024-block reduction cap and the 2048-block elementwise cap
PL_MASKS = ["random", "ones", "zeros", "border_holes", "hole_corner", "hole_interior", "fractional", "faint"]
PL_OPTIONS = ["none", "l1w_binary", "l1w_fractional", "gscale", "gscale0", "accumulate", "nograd", "w_tv0", "w_bnd0", "human"]


def pl_cases():
    """(shape, mask kind, option): every mask at two shapes, every option at two shapes (one with the second finalize trip), every
    shape plain and with the options `human_guided_step` combines."""
    cases = []
    for shape in [(2, 33, 17), (3, 257, 129)]:
        cases += [(shape, mk, "none") for mk in PL_MASKS]
    for shape in [(2, 33, 17), (2, 513, 260)]:
        cases += [(shape, "random", op) for op in PL_OPTIONS]
    for shape in PL_SHAPES:
        cases += [(shape, "random", "none"), (shape, "border_holes", "human")]
    out = []
    for c in cases:
        if c not in out:
            out.append(c)
    return out


def pl_id(case):
    (B, H, W), mk, op = case
    return f"{B}x{H}x{W}-{mk}-{op}"


def make_mask(kind, shape, rng):
    B, H, W = shape
    if kind == "random":                        # 60 % valid
        return (rng.random(shape) < 0.6).astype(np.float32)
    if kind == "ones":
        return np.ones(shape, np.float32)
    if kind == "zeros":
        return np.zeros(shape, np.float32)
    m = np.ones(shape, np.float32)
    if kind == "border_holes":                  # holes on all four corners and in the middle of every border
        for y in (0, H - 1):
            for x in (0, W - 1, W // 2):
                m[:, y, x] = 0
        for x in (0, W - 1):
            m[:, H // 2, x] = 0
        m[-1, H // 2, W // 2] = 0
        return m
    if kind == "hole_corner":
        m[0, H - 1, W - 1] = 0
        return m
    if kind == "hole_interior":
        m[0, H // 2, W // 2] = 0
        return m
    if kind == "fractional":
        return rng.random(shape).astype(np.float32)
    if kind == "faint":                         # 0 < sum(band) < 1: the boundary term is switched off
        m[:] = 0.5
        m[0, H // 2, W // 2] = 0.55
        return m
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def pl_inputs(case):
    """-> dict of fp32 numpy arrays and the keyword arguments; pred == target on about 5 % of the pixels."""
    shape, mk, op = case
    rng = np.random.default_rng(abs(hash((shape, PL_MASKS.index(mk), PL_OPTIONS.index(op)))) % (2 ** 31))
    pred = rng.random(shape).astype(np.float32)
    target = rng.random(shape).astype(np.float32)
    tie = rng.random(shape) < 0.05
    target[tie] = pred[tie]
    mask = make_mask(mk, shape, rng)
    d = dict(pred=pred, target=target, mask=mask, w_l1=1.0, w_tv=f32(0.1), w_bnd=0.5, l1_weight=None, gscale=None, dpred0=None,
             want_grad=True)
    if op == "l1w_binary":
        d["l1_weight"] = (rng.random(shape) < 0.3).astype(np.float32)
    elif op == "l1w_fractional":
        d["l1_weight"] = rng.random(shape).astype(np.float32)
    elif op == "gscale":
        d["gscale"] = np.float32([0.37])
    elif op == "gscale0":
        d["gscale"] = np.float32([0.0])
    elif op == "accumulate":
        d["dpred0"] = rng.standard_normal(shape).astype(np.float32) * np.float32(1.0 / pred.size)
    elif op == "nograd":
        d["want_grad"] = False
    elif op == "w_tv0":
        d["w_tv"] = 0.0
    elif op == "w_bnd0":
        d["w_bnd"] = 0.0
    elif op == "human":                          # as human_guided_step calls it
        h = (rng.random(shape) < 0.2).astype(np.float32)
        d.update(mask=h if mk == "random" else mask, l1_weight=h, w_l1=f32(0.3), w_tv=0.0, w_bnd=f32(0.15),
                 gscale=np.float32([0.37]), dpred0=rng.standard_normal(shape).astype(np.float32) * np.float32(1.0 / pred.size))
    return d


@functools.lru_cache(maxsize=None)
def pl_oracle(case):
    d = pl_inputs(case)
    return PO.pixel_losses(d["pred"], d["target"], d["mask"], d["w_l1"], d["w_tv"], d["w_bnd"], l1_weight=d["l1_weight"],
                           gscale=d["gscale"], dpred0=d["dpred0"])


def _t(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def pl_torch(d, dtype, eps=1e-6):
    """The same closed forms in PyTorch-CPU at `dtype` -> (dict of the five scalars as Python floats, dpred tensor)."""
    p, t, m, lw, d0 = (_t(d[k], dtype) for k in ("pred", "target", "mask", "l1_weight", "dpred0"))
    B, H, W = p.shape
    n = p.numel()
    one = torch.ones((), dtype=dtype)
    w_l1, w_tv, w_bnd = (torch.tensor(d[k], dtype=dtype) for k in ("w_l1", "w_tv", "w_bnd"))
    diff = p - t
    ad = diff.abs()
    l1 = ((ad * lw) if lw is not None else ad).sum() / n
    hole = one - m
    xh = p * hole
    dh, dw = xh[:, 1:, :] - xh[:, :-1, :], xh[:, :, 1:] - xh[:, :, :-1]
    count_h, count_w = B * (H - 1) * W, B * H * (W - 1)
    tv = 2 * ((dh * dh).sum() / count_h + (dw * dw).sum() / count_w) / B
    mx = torch.nn.functional.max_pool2d(m[:, None], 3, 1, 1)[:, 0]
    mn = one - torch.nn.functional.max_pool2d((one - m)[:, None], 3, 1, 1)[:, 0]
    bd = (mx - mn).clamp(0, 1)
    den = bd.sum()
    on = bool(den >= 1)
    bnd = torch.zeros((), dtype=dtype)
    if on:
        bnd = (ad * bd).sum() / (den + torch.tensor(eps, dtype=dtype))
        if not bool(torch.isfinite(bnd)):
            bnd, on = torch.zeros((), dtype=dtype), False
    total = w_l1 * l1 + w_tv * tv + w_bnd * bnd
    gs = torch.ones((), dtype=dtype) if d["gscale"] is None else _t(d["gscale"], dtype)[0]
    sg = torch.sign(diff)
    g = (gs * w_l1 / n) * sg
    if lw is not None:
        g = g * lw
    c_h, c_w = gs * w_tv * 2 / (B * count_h) * 2, gs * w_tv * 2 / (B * count_w) * 2
    gh, gw = torch.zeros_like(p), torch.zeros_like(p)
    gh[:, 1:, :] += dh
    gh[:, :-1, :] -= dh
    gw[:, :, 1:] += dw
    gw[:, :, :-1] -= dw
    g = g + hole * (c_h * gh + c_w * gw)
    if on:
        g = g + (gs * w_bnd / (den + torch.tensor(eps, dtype=dtype))) * sg * bd
    if d0 is not None:
        g = d0 + g
    vals = dict(zip(PO.OUT5, (float(l1), float(tv), float(bnd), float(den), float(total))))
    return vals, g


# ---- reductions, head: element counts and logits ----------------------------------------------------------------------------------
RED_N = [1, 3, 255, 256, 257, 2053, 131072 + 7, 2 ** 21 + 2048 + 3]      # the last: above the 1024-block cap of the reductions
HEAD_N = [1, 257, 2053, 524288 + 5]                                       # the last: above the 2048-block elementwise cap
SATURATED = np.float32([30.0, -30.0, 90.0, -90.0, 0.0])


@functools.lru_cache(maxsize=None)
def logits(n, seed=0):
    """4 * randn with +-30, +-90 and 0 planted.  Not below 5 elements: where every logit saturates, fp32 holds nothing of
    sigmoid(z) - 1 or 1 - sigmoid(z) and a gradient made of them alone measures no kernel."""
    rng = np.random.default_rng(1000 + seed + n)
    z = (4.0 * rng.standard_normal(n)).astype(np.float32)
    if n >= SATURATED.size:
        z[rng.choice(n, size=SATURATED.size, replace=False)] = SATURATED
    return z


@functools.lru_cache(maxsize=None)
def l1_inputs(n, relu_gate):
    """(a, b) fp32; a == b on about 5 % of the elements; with relu_gate `a` is a ReLU output (about half exact zeros)."""
    rng = np.random.default_rng(2000 + n + (7 if relu_gate else 0))
    a = rng.standard_normal(n).astype(np.float32)
    if relu_gate:
        a = np.maximum(a, np.float32(0))
    b = rng.standard_normal(n).astype(np.float32)
    if relu_gate:
        b = np.maximum(b, np.float32(0))
    tie = rng.random(n) < 0.05
    b[tie] = a[tie]
    return a, b


def head_inputs(n, fractional):
    rng = np.random.default_rng(3000 + n + (1 if fractional else 0))
    z = logits(n, seed=5)
    x = rng.random(n).astype(np.float32)
    m = rng.random(n).astype(np.float32) if fractional else (rng.random(n) < 0.6).astype(np.float32)
    dout = rng.standard_normal(n).astype(np.float32)
    return z, x, m, dout


# ---- Adam --------------------------------------------------------------------------------------------------------------------
ADAM_CHUNK = 1 << 14
ADAM_SIZES = [1, 3, 4, 5, ADAM_CHUNK - 1, ADAM_CHUNK, ADAM_CHUNK + 1, 3 * ADAM_CHUNK + 2, 37]
ADAM_ZERO_GRAD_SEG = len(ADAM_SIZES) - 1                                    # the segment whose gradient is all zeros
ADAM_HYPER = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8)
ADAM_STEPS = [1, 2, 3, 1000]                                                # three consecutive steps from zero moments, then step 1000


@functools.lru_cache(maxsize=None)
def adam_data():
    """-> (p0 list, grads[step index] list): fp32 arrays per segment; gradients of very different magnitudes."""
    rng = np.random.default_rng(4000)
    p0 = [(1e-3 * rng.standard_normal(n)).astype(np.float32) for n in ADAM_SIZES]     # |p| ~ a few updates: an error in the update shows in p
    grads = []
    for _ in ADAM_STEPS:
        gs = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(np.float32) for n in ADAM_SIZES]
        gs[ADAM_ZERO_GRAD_SEG][:] = 0
        grads.append(gs)
    return p0, grads


@functools.lru_cache(maxsize=None)
def adam_oracle(grad_scale):
    """-> per step index, the list over segments of (p, m, v) in fp64, each step starting from the fp64 state of the one before.
    (The kernels start each step from their own fp32 state; the tests feed the oracle that state where they compare per step.)"""
    p0, grads = adam_data()
    out = []
    st = [(p.astype(np.float64), np.zeros(p.size), np.zeros(p.size)) for p in p0]
    for si, step in enumerate(ADAM_STEPS):
        st = [PO.adam(p, g, m, v, step=step, grad_scale=grad_scale, **ADAM_HYPER) for (p, m, v), g in zip(st, grads[si])]
        out.append(st)
    return out
