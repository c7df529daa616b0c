"""The pointwise kernels (csrc/pointwise.hip: pixel losses, L1 / BCE means, Adam, the sigmoid/composite head, layout transposes,
small elementwise helpers) at op level against the numpy fp64 oracle tests/pointwise_oracle.py (itself checked against float64
autograd in tests/test_pointwise_oracle_cpu.py), on the inputs of tests/pointwise_cases.py.

How a result is judged: the oracle is evaluated on the same fp32 inputs; the error is measured per element,
e(x) = max_i |x_i - ref_i| / (|ref_i| + 1e-3 max|ref|); the plain fp32 PyTorch-CPU formula of the same op is measured the same
way, and the kernel must satisfy e(hip) <= 4 e(cpu32) + 4 * 2**-24 (device expf / log1pf / division 1-2 ulp off a correctly
rounded host result, fused multiply-add contraction).  Nothing else sets the bound.  Copies, products, zeros and the paths of one
formula through different loops must agree bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pointwise_cases as PC
from tests import pointwise_oracle as PO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def judge(name, hip, cpu32, ref):
    """e(hip) <= 4 e(cpu32) + 4 * 2**-24, both measured against the fp64 oracle; prints the two figures."""
    hip = hip.detach().cpu().numpy() if torch.is_tensor(hip) else hip
    cpu32 = cpu32.detach().numpy() if torch.is_tensor(cpu32) else cpu32
    e_hip, e_cpu = PO.err(hip, ref), PO.err(cpu32, ref)
    print(f"MEASURE {name} e(hip)={e_hip:.3e} e(cpu32)={e_cpu:.3e}")
    assert e_hip <= 4 * e_cpu + 4 * PC.F32_EPS, f"{name}: e(hip) = {e_hip:.3e} > 4 * e(cpu32) = 4 * {e_cpu:.3e} + 4 * 2**-24"


def up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- pixel losses --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.pl_cases(), ids=PC.pl_id)
def test_pixel_losses(dev, case):
    from tg_hip import ops as O
    d = PC.pl_inputs(case)
    ref_vals, ref_dp = PC.pl_oracle(case)
    cpu_vals, cpu_dp = PC.pl_torch(d, torch.float32)
    pred, tgt, m, lw, gs = (up(d[k], dev) for k in ("pred", "target", "mask", "l1_weight", "gscale"))

    def run():
        dp0 = up(d["dpred0"], dev)
        return O.pixel_losses(pred, tgt, m, d["w_l1"], d["w_tv"], d["w_bnd"], l1_weight=lw, gscale=gs, dpred=dp0,
                              accumulate=dp0 is not None, want_grad=d["want_grad"])

    out5, dp = run()
    out5b, dpb = run()
    assert torch.equal(out5, out5b), "pixel_losses: two runs differ"
    vals = out5.cpu().numpy()
    assert np.isfinite(vals).all()
    for i, k in enumerate(PO.OUT5):
        judge(f"pixel_losses.{k}", vals[i:i + 1], np.float32([cpu_vals[k]]), np.float64([ref_vals[k]]))
    if not d["want_grad"]:
        assert dp is None
        return
    assert torch.equal(dp, dpb), "pixel_losses: two runs differ in dpred"
    assert dp.shape == pred.shape
    judge("pixel_losses.dpred", dp, cpu_dp, ref_dp)
    # pred == target: sign 0, so the L1 and boundary terms contribute exactly nothing; where the TV term is off as well
    # (weight 0, or a valid pixel: its factor 1 - mask is 0) the gradient is exactly 0 / exactly the accumulated-into value
    zero = (d["pred"] == d["target"]) & ((d["mask"] == 1) | (d["w_tv"] == 0.0))
    if d["gscale"] is not None and d["gscale"][0] == 0:
        zero[:] = True
    base = np.zeros_like(d["pred"]) if d["dpred0"] is None else d["dpred0"]
    assert np.array_equal(dp.cpu().numpy()[zero], base[zero]), "dpred: a zero contribution is not exactly zero"


def test_pixel_losses_refuses_raw_storage(dev):
    from tg_hip import ops as O
    from tg_hip.lib import TgError
    B, H, W = 2, 12, 10
    pred, tgt = torch.rand(B, H, W, device=dev), torch.rand(B, H, W, device=dev)
    m = (torch.rand(B, H, W, device=dev) < 0.6).float()
    O.pixel_losses(pred, tgt, m, 1.0, 0.1, 0.5)
    mt = (torch.rand(B, W, H, device=dev) < 0.6).float().transpose(1, 2)            # right shape, strided
    with pytest.raises(TgError, match="contiguous"):
        O.pixel_losses(pred, tgt, mt, 1.0, 0.1, 0.5)
    with pytest.raises(TgError, match="contiguous"):
        O.pixel_losses(pred, tgt, m, 1.0, 0.1, 0.5, dpred=torch.zeros(B, W, H, device=dev).transpose(1, 2), accumulate=True)
    with pytest.raises(TgError, match="elements"):
        O.pixel_losses(pred, tgt, m[:1], 1.0, 0.1, 0.5)
    with pytest.raises(TgError, match="elements"):
        O.pixel_losses(pred, tgt[:, :-1].contiguous(), m, 1.0, 0.1, 0.5)
    with pytest.raises(TgError, match="elements"):
        O.pixel_losses(pred, tgt, m, 1.0, 0.1, 0.5, dpred=torch.zeros(B, H, W - 1, device=dev), accumulate=True)
    with pytest.raises(TgError, match="elements"):
        O.pixel_losses(pred, tgt, m, 1.0, 0.1, 0.5, l1_weight=torch.ones(B, H, device=dev))
    with pytest.raises(TgError, match="one float"):
        O.pixel_losses(pred, tgt, m, 1.0, 0.1, 0.5, gscale=torch.ones(2, device=dev))
    with pytest.raises(TgError, match="float32"):
        O.pixel_losses(pred, tgt, m, 1.0, 0.1, 0.5, gscale=torch.ones(1, device=dev, dtype=torch.float64))


# ---- L1 mean ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["plain", "scaled", "nograd"])
@pytest.mark.parametrize("relu_gate", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("n", PC.RED_N)
def test_l1_mean(dev, n, relu_gate, opt):
    from tg_hip import ops as O
    a_np, b_np = PC.l1_inputs(n, relu_gate)
    coef = PC.f32(0.1) if opt == "scaled" else 1.0
    gs_np = np.float32([0.37]) if opt == "scaled" else None
    ref_val, ref_da = PO.l1_mean(a_np, b_np, coef=coef, gscale=gs_np, relu_gate=relu_gate)
    a32, b32 = t32(a_np), t32(b_np)
    d32 = a32 - b32
    out, da = O.l1_mean(up(a_np, dev), up(b_np, dev), coef=coef, gscale=up(gs_np, dev), want_grad=opt != "nograd", relu_gate=relu_gate)
    judge("l1_mean.value", out, d32.abs().mean().reshape(1), np.float64([ref_val]))
    if opt == "nograd":
        assert da is None
        return
    k32 = torch.tensor(coef, dtype=torch.float32) * (t32(gs_np)[0] if gs_np is not None else 1.0) / n
    da32 = k32 * torch.sign(d32)
    if relu_gate:
        da32 = da32 * (a32 > 0)
    judge("l1_mean.da", da, da32, ref_da)
    zero = (a_np == b_np) | ((a_np <= 0) if relu_gate else False)
    got = da.cpu().numpy()
    assert not got[zero].any(), "da: a tie or a closed gate is not exactly zero"
    assert got[~zero].all()


# ---- BCE with logits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["plain", "scaled"])
@pytest.mark.parametrize("target", [0.0, 1.0, PC.f32(0.9)])
@pytest.mark.parametrize("n", PC.RED_N)
def test_bce_logits(dev, n, target, opt):
    from tg_hip import ops as O
    z_np = PC.logits(n)
    coef = PC.f32(0.1) if opt == "scaled" else 1.0
    gs_np = np.float32([0.37]) if opt == "scaled" else None
    ref_val, ref_dz = PO.bce_logits(z_np, target, coef=coef, gscale=gs_np)
    z32 = t32(z_np)
    out, dz = O.bce_logits(up(z_np, dev), target, coef=coef, gscale=up(gs_np, dev))
    assert torch.isfinite(out).all() and torch.isfinite(dz).all()
    judge("bce_logits.value", out, F.binary_cross_entropy_with_logits(z32, torch.full_like(z32, target)).reshape(1), np.float64([ref_val]))
    k32 = torch.tensor(coef, dtype=torch.float32) * (t32(gs_np)[0] if gs_np is not None else 1.0) / n
    judge("bce_logits.dz", dz, k32 * (torch.sigmoid(z32) - target), ref_dz)
    out2, none = O.bce_logits(up(z_np, dev), target, coef=coef, want_grad=False)
    assert none is None and torch.equal(out2, out)


@pytest.mark.parametrize("n", [257, 2053, 131072 + 7])
def test_bce_logits_writes_only_its_slice(dev, n):
    """dz_out as one half of a stacked buffer: the other half stays as it was, bit for bit."""
    from tg_hip import ops as O
    z = up(PC.logits(n), dev)
    _, want = O.bce_logits(z, 1.0)
    for half in (0, 1):
        buf = torch.full((2, n), float("nan"), device=dev)
        fill = torch.randn(n, device=dev)
        buf[1 - half] = fill
        _, dz = O.bce_logits(z, 1.0, dz_out=buf[half])
        assert dz.data_ptr() == buf[half].data_ptr()
        assert torch.equal(buf[half], want) and torch.equal(buf[1 - half], fill)


# ---- generator head -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_dx", [False, True], ids=["dz", "dz_dx"])
@pytest.mark.parametrize("fractional", [False, True], ids=["binary", "fractional"])
@pytest.mark.parametrize("n", PC.HEAD_N)
def test_sigmoid_composite(dev, n, fractional, want_dx):
    from tg_hip import ops as O
    z_np, x_np, m_np, g_np = PC.head_inputs(n, fractional)
    z, x, m, g = (up(a, dev) for a in (z_np, x_np, m_np, g_np))
    z32, x32, m32, g32 = (t32(a) for a in (z_np, x_np, m_np, g_np))
    s32 = torch.sigmoid(z32)
    out = O.sigmoid_composite_fwd(z, x, m)
    pre = torch.full((n + 2,), 7.0, device=dev)
    out2 = O.sigmoid_composite_fwd(z, x, m, out=pre[1:n + 1])                 # preallocated: a view, its neighbours untouched
    assert out2.data_ptr() == pre[1:].data_ptr() and torch.equal(out2, out) and pre[0] == 7.0 and pre[n + 1] == 7.0
    assert torch.isfinite(out).all()
    judge("sigmoid_composite_fwd", out, s32 * (1 - m32) + x32 * m32, PO.sigmoid_composite_fwd(z_np, x_np, m_np))
    if not fractional:
        valid = m_np == 1
        assert np.array_equal(out.cpu().numpy()[valid], x_np[valid])           # s * 0 + x * 1: the input itself
    dz, dx = O.sigmoid_composite_bwd(g, z, m, want_dx=want_dx)
    ref_dz, ref_dx = PO.sigmoid_composite_bwd(g_np, z_np, m_np)
    assert torch.isfinite(dz).all()
    judge("sigmoid_composite_bwd.dz", dz, g32 * (1 - m32) * (1 - s32) * s32, ref_dz)
    if want_dx:
        assert torch.equal(dx.cpu(), g32 * m32)
    else:
        assert dx is None


def test_head_and_lincomb_refuse_raw_storage(dev):
    from tg_hip import ops as O
    from tg_hip.lib import TgError
    n = 48
    z, x, g = (torch.randn(n, device=dev) for _ in range(3))
    m = (torch.rand(n, device=dev) < 0.5).float()
    strided = torch.randn(2 * n, device=dev)[::2]
    assert not strided.is_contiguous() and strided.numel() == n
    for args in ((strided, x, m), (z, strided, m), (z, x, strided)):
        with pytest.raises(TgError, match="contiguous"):
            O.sigmoid_composite_fwd(*args)
    for args in ((z[:-1], x, m), (z, x, m[:-1]), (z, x, torch.ones(2 * n, device=dev))):
        with pytest.raises(TgError, match="elements"):
            O.sigmoid_composite_fwd(*args)
    with pytest.raises(TgError, match="elements"):
        O.sigmoid_composite_fwd(z, x, m, out=torch.empty(n - 1, device=dev))
    for args in ((strided, z, m), (g, strided, m), (g, z, strided)):
        with pytest.raises(TgError, match="contiguous"):
            O.sigmoid_composite_bwd(*args)
    for args in ((g, z[:-1], m), (g, z, m[:-1])):
        with pytest.raises(TgError, match="elements"):
            O.sigmoid_composite_bwd(*args)
    with pytest.raises(TgError, match="float32"):
        O.sigmoid_composite_fwd(z, x, m.double())
    for args in ((strided, x), (z, strided)):
        with pytest.raises(TgError, match="contiguous"):
            O.lincomb(args[0], 1.0, args[1], 1.0)
    with pytest.raises(TgError, match="elements"):
        O.lincomb(z, 1.0, x[:-1], 1.0)
    with pytest.raises(TgError, match="no CPU path"):
        O.lincomb(z, 1.0, x.cpu(), 1.0)


# ---- layout transposes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 1, 1), (2, 3, 5, 7), (1, 5, 17, 33), (2, 64, 9, 13), (1, 130, 8, 8), (1, 2, 513, 513),
                                   (2, 1, 9, 13)], ids=lambda s: "x".join(map(str, s)))
def test_layout_transposes_are_exact(dev, shape):
    from tg_hip import ops as O
    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(B * 1000 + Cc)
    x = torch.randn(shape, generator=g)
    y = O.nchw_to_nhwc(x.to(dev))
    assert y.shape == (B, H, W, Cc) and y.is_contiguous()
    assert torch.equal(y.cpu(), x.permute(0, 2, 3, 1).contiguous())
    back = O.nhwc_to_nchw(y)
    assert back.shape == shape and back.is_contiguous() and torch.equal(back.cpu(), x)
    # nhwc_to_nchw of data that is no transpose of anything the first kernel produced
    z = torch.randn(B, H, W, Cc, generator=g)
    assert torch.equal(O.nhwc_to_nchw(z.to(dev)).cpu(), z.permute(0, 3, 1, 2).contiguous())
    # a logical NCHW tensor that is not contiguous (channels_last storage)
    xs = x.to(dev).contiguous(memory_format=torch.channels_last) if H * W > 1 and Cc > 1 else x.to(dev).transpose(2, 3).contiguous().transpose(2, 3)
    assert torch.equal(O.nchw_to_nhwc(xs).cpu(), x.permute(0, 2, 3, 1).contiguous())


# ---- BN eval statistics, act_bwd ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [1, 3, 256, 257, 1024])
def test_bn_eval_stats(dev, Cc):
    from tg_hip import ops as O
    rng = np.random.default_rng(Cc)
    rm = rng.standard_normal(Cc).astype(np.float32)
    rv = (rng.random(Cc) * 10.0 ** rng.uniform(-6, 2, Cc)).astype(np.float32)
    rv[0] = 0.0
    if Cc > 1:
        rv[-1] = 1e-12
    mean, rstd = O.bn_eval_stats(up(rm, dev), up(rv, dev))
    ref_mean, ref_rstd = PO.bn_eval_stats(rm, rv, eps=PC.f32(O.BN_EPS))
    assert torch.equal(mean.cpu(), t32(rm)) and ref_mean.astype(np.float32).tolist() == rm.tolist()
    judge("bn_eval_stats.rstd", rstd, 1.0 / torch.sqrt(t32(rv) + torch.tensor(O.BN_EPS, dtype=torch.float32)), ref_rstd)


@pytest.mark.parametrize("act", [PO.ACT_NONE, PO.ACT_RELU, PO.ACT_LEAKY], ids=["none", "relu", "leaky"])
@pytest.mark.parametrize("rows,Cc", [(7, 1), (33, 3), (257, 64), (2049, 3), (8193, 64)])
def test_act_bwd_with_ratio(dev, rows, Cc, act):
    from tg_hip import ops as O
    rng = np.random.default_rng(rows + Cc)
    dout = rng.standard_normal((1, rows, 1, Cc)).astype(np.float32)
    out = rng.standard_normal((1, rows, 1, Cc)).astype(np.float32)
    if act == PO.ACT_RELU:
        out = np.maximum(out, np.float32(0))
    out[rng.random(out.shape) < 0.05] = 0                                     # exact zeros: the gate is `> 0`
    ratio = (9.0 / rng.integers(1, 10, (1, rows, 1))).astype(np.float32)
    ratio[rng.random(ratio.shape) < 0.2] = 0
    slope = PC.f32(0.2)
    for rt in (None, ratio):
        din = O.act_bwd(up(dout, dev), up(out, dev), act, slope, ratio=up(rt, dev), inplace=False)
        ref = PO.act_bwd(dout.reshape(rows, Cc), out.reshape(rows, Cc), act, slope, None if rt is None else rt.reshape(rows))
        g32 = t32(dout)
        if act != PO.ACT_NONE:
            g32 = g32 * torch.where(t32(out) > 0, torch.tensor(1.0), torch.tensor(0.0 if act == PO.ACT_RELU else slope))
        if rt is not None:
            g32 = g32 * t32(rt)[..., None]
        judge("act_bwd", din.reshape(rows, Cc), g32.reshape(rows, Cc), ref)
        assert torch.equal(din.cpu(), g32)                                     # products of the same fp32 factors in the same order
    d_in = up(dout, dev)
    assert O.act_bwd(d_in, up(out, dev), act, slope, ratio=up(ratio, dev)).data_ptr() == d_in.data_ptr()      # in place by default
    assert torch.equal(d_in.cpu(), g32)


# ---- elementwise helpers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 2053, 524288 + 5])
def test_mul_axpby_lincomb(dev, n):
    from tg_hip import ops as O
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ad, bd = a.to(dev), b.to(dev)
    assert torch.equal(O.mul(ad, bd).cpu(), a * b)
    keep = torch.full((n + 2,), 3.0, device=dev)
    prod = O.mul(ad, bd, keep=keep[1:n + 1])
    assert torch.equal(prod.cpu(), a * b) and torch.equal(keep[1:n + 1].cpu(), a) and keep[0] == 3.0 and keep[n + 1] == 3.0
    # y = a*x + b*y with b == 0 must not read y: NaN * 0 would be NaN
    y = torch.full((n,), float("nan"), device=dev)
    sa = PC.f32(0.37)
    assert O.axpby_(ad, sa, 0.0, y) is y
    assert torch.isfinite(y).all() and torch.equal(y.cpu(), torch.tensor(sa) * a)
    y2 = bd.clone()
    O.axpby_(ad, sa, PC.f32(-1.7), y2)
    ref = sa * a.double().numpy() + PC.f32(-1.7) * b.double().numpy()
    judge("axpby_", y2, torch.tensor(sa) * a + torch.tensor(PC.f32(-1.7)) * b, ref)
    judge("lincomb", O.lincomb(ad, sa, bd, PC.f32(-1.7)), torch.tensor(sa) * a + torch.tensor(PC.f32(-1.7)) * b, ref)
    assert torch.equal(ad.cpu(), a) and torch.equal(bd.cpu(), b)


@pytest.mark.parametrize("n", [1, 2, 15, 16])
def test_write_floats(dev, n):
    from tg_hip import lib as L
    from tg_hip import ops as O
    vals = (np.arange(16) * np.float32(1.1) - np.float32(3.3)).astype(np.float32)
    vals[0] = np.float32(-0.0)
    dst = torch.full((20,), 5.0, device=dev)
    L.check(L.load().tg_write_floats(C.c_void_p(dst[2:].data_ptr()), n, C.c_void_p(vals.ctypes.data), O._stream()), "tg_write_floats")
    keep = vals[:n].copy()
    vals[:] = 99                                                               # the values travelled with the launch
    got = dst.cpu().numpy()
    assert got[2:2 + n].tobytes() == keep.tobytes()
    assert (got[:2] == 5).all() and (got[2 + n:] == 5).all()


# ---- Adam --------------------------------------------------------------------------------------------------------------------
ADAM_VARIANTS = {"aligned": (0, 0, 0, 0), "off1": (1, 1, 1, 1), "off2": (2, 2, 2, 2), "off3": (3, 3, 3, 3), "g_off1": (0, 1, 0, 0)}
_adam_runs = {}


def _adam_layout():
    """First float of every segment in a backing buffer: multiples of 4, at least 8 guard floats apart."""
    starts, cur = [], 8
    for n in PC.ADAM_SIZES:
        starts.append(cur)
        cur = (cur + n + 3 + 8 + 3) // 4 * 4
    return starts, cur + 8


def adam_run(dev, variant, grad_scale, path):
    """All steps of PC.ADAM_STEPS through one entry point on segments laid out as `variant` says -> per step, per segment,
    (p, m, v) as CPU tensors.  Checks that no float outside the segments changed."""
    key = (variant, grad_scale, path)
    if key in _adam_runs:
        return _adam_runs[key]
    from tg_hip import lib as L
    from tg_hip import ops as O
    p0, grads = PC.adam_data()
    starts, total = _adam_layout()
    offs = ADAM_VARIANTS[variant]
    fills = (7.0, float("nan"), -3.0, 11.0)                                    # a gradient read out of its segment poisons the result
    bufs = [torch.full((total,), f, device=dev) for f in fills]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    views = [[b[s + o:s + o + n] for s, n in zip(starts, PC.ADAM_SIZES)] for b, o in zip(bufs, offs)]
    P, G, M, V = views
    for i, p in enumerate(p0):
        P[i].copy_(t32(p))
        M[i].zero_()
        V[i].zero_()
        assert (P[i].data_ptr() % 16 == 0) == (offs[0] == 0) and (G[i].data_ptr() % 16 == 0) == (offs[1] == 0)
    inside = [torch.zeros(total, dtype=torch.bool) for _ in bufs]
    for k, o in enumerate(offs):
        for s, n in zip(starts, PC.ADAM_SIZES):
            inside[k][s + o:s + o + n] = True
    guards0 = [b.cpu() for b in bufs]
    h = PC.ADAM_HYPER
    out = []
    for si, step in enumerate(PC.ADAM_STEPS):
        for i, g in enumerate(grads[si]):
            G[i].copy_(t32(g))
        if path == "single":
            for p, g, m, v in zip(P, G, M, V):
                O.adam_(p, g, m, v, h["lr"], h["beta1"], h["beta2"], h["eps"], step, grad_scale)
        elif path == "multi":
            O.adam_multi_(P, G, M, V, h["lr"], h["beta1"], h["beta2"], h["eps"], step, grad_scale)
        else:
            # tg_adam_multi_s, eagerly: the two floats of tg_adam_scalars, written by tg_write_floats into the arena's first slot
            lib = L.load()
            arena = O.AdamScalarArena(dev)
            host = np.zeros(2, np.float32)
            L.check(lib.tg_adam_scalars(h["lr"], h["beta1"], h["beta2"], step, C.c_void_p(host.ctypes.data)), "tg_adam_scalars")
            L.check(lib.tg_write_floats(C.c_void_p(arena.dev.data_ptr()), 2, C.c_void_p(host.ctypes.data), O._stream()), "tg_write_floats")
            arena.active = True
            assert O.adam_scalar_arena is None
            O.adam_scalar_arena = arena
            try:
                O.adam_multi_(P, G, M, V, h["lr"], h["beta1"], h["beta2"], h["eps"], step, grad_scale)
            finally:
                O.adam_scalar_arena = None
            assert arena.slots == [(h["lr"], h["beta1"], h["beta2"], step)]
        out.append([(p.cpu().clone(), m.cpu().clone(), v.cpu().clone()) for p, m, v in zip(P, M, V)])
        for k, nm in enumerate("pgmv"):
            now = bufs[k].cpu()
            a, b = now[~inside[k]], guards0[k][~inside[k]]
            assert a.numpy().tobytes() == b.numpy().tobytes(), f"adam {key} step {step}: a float outside the segments of {nm} changed"
    _adam_runs[key] = out
    return out


_adam_cpu32 = {}


def adam_cpu32(grad_scale):
    """torch.optim.Adam(foreach=False) in fp32 on the CPU over the same steps -> per step, per segment, (p, m, v)."""
    if grad_scale in _adam_cpu32:
        return _adam_cpu32[grad_scale]
    p0, grads = PC.adam_data()
    h = PC.ADAM_HYPER
    params = [torch.nn.Parameter(t32(p).clone()) for p in p0]
    opt = torch.optim.Adam(params, foreach=False, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
    out = []
    for si, step in enumerate(PC.ADAM_STEPS):
        for p, g in zip(params, grads[si]):
            p.grad = t32(g) * grad_scale                                       # exact for 1 and 0.5
            if step > 1:
                opt.state[p]["step"] = torch.tensor(float(step - 1))
        opt.step()
        out.append([(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params])
    _adam_cpu32[grad_scale] = out
    return out


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("variant", list(ADAM_VARIANTS))
def test_adam_multi_matches_oracle(dev, variant, grad_scale):
    hip = adam_run(dev, variant, grad_scale, "multi")
    ref, cpu = PC.adam_oracle(grad_scale), adam_cpu32(grad_scale)
    p0, _ = PC.adam_data()
    for si, step in enumerate(PC.ADAM_STEPS):
        for i, n in enumerate(PC.ADAM_SIZES):
            for k, nm in enumerate("pmv"):
                assert torch.isfinite(hip[si][i][k]).all()
                judge(f"adam.{nm}[step {step}, n {n}]", hip[si][i][k], cpu[si][i][k], ref[si][i][k])
        z = PC.ADAM_ZERO_GRAD_SEG
        assert torch.equal(hip[si][z][0], t32(p0[z])), "a zero gradient from zero moments moved the parameter"
        assert not hip[si][z][1].any() and not hip[si][z][2].any()


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_adam_entry_points_and_paths_agree_bit_for_bit(dev, grad_scale):
    """One formula, three loops (tg_adam; the 16-byte and the scalar loop of tg_adam_multi) and two ways the per-step scalars
    arrive (kernel arguments; tg_adam_scalars -> tg_write_floats -> device memory): the same bits on the same data."""
    want = adam_run(dev, "aligned", grad_scale, "multi")
    for variant, path in [("off1", "multi"), ("off2", "multi"), ("off3", "multi"), ("g_off1", "multi"), ("aligned", "single"),
                          ("off1", "single"), ("aligned", "multi_s"), ("off3", "multi_s")]:
        got = adam_run(dev, variant, grad_scale, path)
        for si, step in enumerate(PC.ADAM_STEPS):
            for i, n in enumerate(PC.ADAM_SIZES):
                for k, nm in enumerate("pmv"):
                    assert torch.equal(got[si][i][k], want[si][i][k]), \
                        f"{variant}/{path} differs from aligned/multi: {nm}, step {step}, segment of {n}"


@pytest.mark.parametrize("first,second", [(1000, 10), (10, 1000)])
def test_adam_multi_table_follows_the_element_counts(dev, first, second):
    """Views of another length at the SAME four pointers: the cached device table holds the first call's counts, so the key it
    is cached under must hold them too.  (1000, 10): elements 10.. must not be touched by the second call; (10, 1000): they
    must be updated."""
    from tg_hip import ops as O
    O._adam_tables.clear()
    h = PC.ADAM_HYPER
    rng = np.random.default_rng(77)
    bufs = [up(rng.standard_normal(1000).astype(np.float32), dev) for _ in range(2)] + [torch.zeros(1000, device=dev) for _ in range(2)]
    p, g, m, v = bufs
    ptrs = [b.data_ptr() for b in bufs]
    O.adam_multi_([p[:first]], [g[:first]], [m[:first]], [v[:first]], h["lr"], h["beta1"], h["beta2"], h["eps"], 1)
    mid = [b.cpu().clone() for b in bufs]
    O.adam_multi_([p[:second]], [g[:second]], [m[:second]], [v[:second]], h["lr"], h["beta1"], h["beta2"], h["eps"], 2)
    end = [b.cpu() for b in bufs]
    assert [b.data_ptr() for b in bufs] == ptrs
    lo, hi = min(first, second), max(first, second)
    for k in (0, 2, 3):
        assert not torch.equal(end[k][:lo], mid[k][:lo])                       # the common head is updated by both calls
        if second < first:
            assert torch.equal(end[k][lo:hi], mid[k][lo:hi]), f"{'pgmv'[k]}[{lo}:{hi}] was touched by a call on {second} elements"
        else:
            assert (end[k][lo:hi] != mid[k][lo:hi]).all(), f"{'pgmv'[k]}[{lo}:{hi}] was not updated by a call on {second} elements"
    # and what the second call computed is a step on exactly `second` elements
    g32 = end[1][:second]
    ref = PO.adam(mid[0][:second].numpy(), g32.numpy(), mid[2][:second].numpy(), mid[3][:second].numpy(), step=2, **h)
    m32 = mid[2][:second].clone().lerp_(g32, 1 - h["beta1"])
    v32 = mid[3][:second].clone().mul_(h["beta2"]).addcmul_(g32, g32, value=1 - h["beta2"])
    step_size, bc2_sqrt = PO.adam_scalars(h["lr"], h["beta1"], h["beta2"], 2)
    p32 = mid[0][:second].clone().addcdiv_(m32, (v32.sqrt() / bc2_sqrt).add_(h["eps"]), value=-step_size)
    for nm, k, c32, r in (("p", 0, p32, ref[0]), ("m", 2, m32, ref[1]), ("v", 3, v32, ref[2])):
        judge(f"adam.{nm}[table reuse {first}->{second}]", end[k][:second], c32, r)
    O._adam_tables.clear()
