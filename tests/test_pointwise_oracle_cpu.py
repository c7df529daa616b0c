"""Is tests/pointwise_oracle.py right?  The numpy fp64 oracle against float64 PyTorch autograd -- oracle/terragan_oracle's tv_loss and
boundary_loss, F.binary_cross_entropy_with_logits, torch.optim.Adam -- at the shapes and option combinations the GPU tests use
(tests/pointwise_cases.py), so that the oracle is known to be right before a kernel is judged by it.  Also what can be checked of
csrc/pointwise.hip without a GPU: the host-side argument checks of the C ABI, tg_adam_scalars, the key of adam_multi_'s table.

Bounds are multiples of U = 2**-52 in the measure of pointwise_oracle.err (per element, floor 1e-3 * max|ref|):
  * SCALAR = 64 U for sums and means: numpy and torch both sum pairwise, each within log2(n) / 2 <= 11 U of the exact sum of
    n <= 2.1 M non-negative terms; the few operations behind the sum add a handful of U.
  * FIELD = 2**14 U (3.6e-12) for per-element fields: an entry is a sum of at most 8 terms, each within a few U of its own
    magnitude, which is at most a few times max|ref|: 16 U * max|ref| absolutely, and the floor of the measure turns that into at
    most 16 U / 1e-3 <= 2**14 U where terms cancel.  A wrong stencil tap, sign or coefficient is off by 1e-3 or more."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pointwise_cases as PC
from tests import pointwise_oracle as PO

U = 2.0 ** -52
SCALAR = 64 * U
FIELD = 2 ** 14 * U


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


@pytest.mark.parametrize("case", PC.pl_cases(), ids=PC.pl_id)
def test_pixel_losses_oracle_equals_float64_autograd(case):
    from oracle import terragan_oracle as Orc
    d = PC.pl_inputs(case)
    vals, dp = PC.pl_oracle(case)
    pred = t64(d["pred"])[:, None].requires_grad_(True)
    tgt, m = t64(d["target"])[:, None], t64(d["mask"])[:, None]
    ad = (pred - tgt).abs()
    l1 = (ad * t64(d["l1_weight"])[:, None]).mean() if d["l1_weight"] is not None else ad.mean()
    tv = Orc.tv_loss(pred * (1 - m))
    bnd = Orc.boundary_loss(pred, tgt, m).double()
    total = d["w_l1"] * l1 + d["w_tv"] * tv + d["w_bnd"] * bnd
    gs = 1.0 if d["gscale"] is None else float(d["gscale"][0])
    (gs * total).backward()
    ref_dp = pred.grad[:, 0]
    if d["dpred0"] is not None:
        ref_dp = t64(d["dpred0"]) + ref_dp
    ref = dict(l1=l1.item(), tv=tv.item(), boundary=bnd.item(), band_sum=Orc.boundary_band(m).sum().item(), total=total.item())
    for k in PO.OUT5:
        e = PO.err(vals[k], ref[k])
        assert e <= SCALAR, f"{k}: oracle {vals[k]!r} autograd {ref[k]!r} e = {e / U:.1f} U"
    e = PO.err(dp, ref_dp.numpy())
    assert e <= FIELD, f"dpred: e = {e / U:.1f} U"
    # the closed form that gives the GPU tests their fp32 baseline is the same operation: at float64 it agrees as well
    vals_t, dp_t = PC.pl_torch(d, torch.float64)
    for k in PO.OUT5:
        assert PO.err(vals_t[k], vals[k]) <= SCALAR, k
    assert PO.err(dp_t.numpy(), dp) <= FIELD


def test_boundary_rules_of_the_oracle():
    """Empty band and sum(band) < 1: value 0 and no boundary gradient, as oracle.terragan_oracle.boundary_loss returns zeros."""
    for mk in ("ones", "zeros", "faint"):
        case = ((2, 33, 17), mk, "none")
        vals, dp = PC.pl_oracle(case)
        d = PC.pl_inputs(case)
        assert vals["boundary"] == 0.0 and vals["band_sum"] < 1.0
        assert (vals["band_sum"] > 0.0) == (mk == "faint")
        _, dp_nobnd = PO.pixel_losses(d["pred"], d["target"], d["mask"], d["w_l1"], d["w_tv"], 0.0)
        assert np.array_equal(dp, dp_nobnd)
    vals, _ = PC.pl_oracle(((2, 33, 17), "hole_interior", "none"))
    assert vals["band_sum"] == 9.0 and vals["boundary"] > 0.0
    vals, _ = PC.pl_oracle(((2, 33, 17), "hole_corner", "none"))
    assert vals["band_sum"] == 4.0


@pytest.mark.parametrize("relu_gate", [False, True])
@pytest.mark.parametrize("n", PC.RED_N)
def test_l1_mean_oracle_equals_float64_autograd(n, relu_gate):
    a_np, b_np = PC.l1_inputs(n, relu_gate)
    coef, gs = PC.f32(0.1), np.float32([0.37])
    val, da = PO.l1_mean(a_np, b_np, coef=coef, gscale=gs, relu_gate=relu_gate)
    a = t64(a_np).requires_grad_(True)
    loss = ((torch.relu(a) if relu_gate else a) - t64(b_np)).abs().mean()     # a >= 0 already: relu(a) is a, its gradient the gate
    (coef * float(gs[0]) * loss).backward()
    assert PO.err(val, loss.item()) <= SCALAR
    assert PO.err(da, a.grad.numpy()) <= FIELD
    zero = (a_np == b_np) | ((a_np <= 0) if relu_gate else False)
    assert zero.mean() > 0.03 or n < 256
    assert not da[zero].any() and da[~zero].all()


@pytest.mark.parametrize("target", [0.0, 1.0, PC.f32(0.9)])
@pytest.mark.parametrize("n", PC.RED_N)
def test_bce_oracle_equals_float64_autograd(n, target):
    z_np = PC.logits(n)
    coef, gs = PC.f32(0.1), np.float32([0.37])
    val, dz = PO.bce_logits(z_np, target, coef=coef, gscale=gs)
    z = t64(z_np).requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(z, torch.full_like(z, target))
    (coef * float(gs[0]) * loss).backward()
    assert np.isfinite(val) and np.isfinite(dz).all()
    assert PO.err(val, loss.item()) <= SCALAR
    assert PO.err(dz, z.grad.numpy()) <= FIELD
    if n >= PC.SATURATED.size:
        assert set(PC.SATURATED.tolist()) <= set(z_np.tolist())


@pytest.mark.parametrize("fractional", [False, True])
@pytest.mark.parametrize("n", PC.HEAD_N)
def test_head_oracle_equals_float64_autograd(n, fractional):
    z_np, x_np, m_np, g_np = PC.head_inputs(n, fractional)
    z, x = t64(z_np).requires_grad_(True), t64(x_np).requires_grad_(True)
    m = t64(m_np)
    out = torch.sigmoid(z) * (1 - m) + x * m
    out.backward(t64(g_np))
    dz, dx = PO.sigmoid_composite_bwd(g_np, z_np, m_np)
    fwd = PO.sigmoid_composite_fwd(z_np, x_np, m_np)
    assert np.isfinite(fwd).all() and np.isfinite(dz).all()
    assert PO.err(fwd, out.detach().numpy()) <= FIELD
    # d sigmoid = s (1 - s): torch forms 1 - s by subtraction, which at z = 30 (s = 1 - 9e-14) is good to 9e-14 / U = 400 U
    # only; the oracle forms it as sigmoid(-z).  Compared absolutely against the largest entry, as that error is absolute.
    assert np.abs(dz - z.grad.numpy()).max() <= 4 * U * np.abs(g_np).max()
    assert PO.err(dx, x.grad.numpy()) <= FIELD
    sat = np.isin(z_np, [90.0, -90.0])
    if n >= PC.SATURATED.size:
        assert sat.sum() >= 2 and (np.abs(dz[sat]) < 1e-30).all()            # and not NaN from inf * 0


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_adam_oracle_equals_float64_torch_adam(grad_scale):
    p0, grads = PC.adam_data()
    ref = PC.adam_oracle(grad_scale)
    params = [torch.nn.Parameter(t64(p)) for p in p0]
    opt = torch.optim.Adam(params, foreach=False, lr=PC.ADAM_HYPER["lr"], betas=(PC.ADAM_HYPER["beta1"], PC.ADAM_HYPER["beta2"]),
                           eps=PC.ADAM_HYPER["eps"])
    for si, step in enumerate(PC.ADAM_STEPS):
        for p, g in zip(params, grads[si]):
            p.grad = t64(g) * grad_scale
            if step > 1:
                opt.state[p]["step"] = torch.tensor(float(step - 1))
        opt.step()
        for i, p in enumerate(params):
            rp, rm, rv = ref[si][i]
            st = opt.state[p]
            for nm, a, b in (("p", rp, p.detach()), ("m", rm, st["exp_avg"]), ("v", rv, st["exp_avg_sq"])):
                e = PO.err(a, b.numpy())
                assert e <= FIELD, f"step {step} segment {i} {nm}: e = {e / U:.1f} U"
    zp = ref[-1][PC.ADAM_ZERO_GRAD_SEG][0]
    assert np.array_equal(zp, p0[PC.ADAM_ZERO_GRAD_SEG].astype(np.float64))   # zero gradient from zero moments: p unchanged


def test_bn_eval_stats_oracle_is_eval_mode_batchnorm():
    rng = np.random.default_rng(5)
    rm, rv = rng.standard_normal(7), np.abs(rng.standard_normal(7))
    rv[:2] = (0.0, 1e-12)
    mean, rstd = PO.bn_eval_stats(rm, rv, eps=1e-5)
    x = torch.from_numpy(rng.standard_normal((3, 7)))
    ref = F.batch_norm(x, torch.from_numpy(rm), torch.from_numpy(rv), training=False, eps=1e-5)
    assert PO.err((x.numpy() - mean) * rstd, ref.numpy()) <= FIELD


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    return L.load()


@pytest.mark.parametrize("step", [1, 2, 3, 1000, 100000])
def test_adam_scalars_are_the_oracles_rounded_to_fp32(lib, step):
    out = np.zeros(2, np.float32)
    assert lib.tg_adam_scalars(2e-4, 0.9, 0.999, step, C.c_void_p(out.ctypes.data)) == 0
    ref = PO.adam_scalars(2e-4, 0.9, 0.999, step)
    assert out[0] == np.float32(ref[0]) and out[1] == np.float32(ref[1]), (out, ref)
    assert lib.tg_adam_scalars(2e-4, 0.9, 0.999, 0, C.c_void_p(out.ctypes.data)) == -1
    assert lib.tg_adam_scalars(2e-4, 0.9, 0.999, 1, None) == -1 and b"tg_adam_scalars" in lib.tg_last_error()


NN = C.c_void_p(4096)          # a non-null pointer for calls that are refused before anything is launched or dereferenced


@pytest.mark.parametrize("chunk", [1, 2, 3, 6, 16383, 16386])
def test_adam_multi_refuses_chunks_that_are_no_multiple_of_4(lib, chunk):
    """The aligned path does 16-byte accesses from chunk * chunk_elems on: another chunk size would misalign them."""
    rc = lib.tg_adam_multi(NN, NN, 1, chunk, 2e-4, 0.9, 0.999, 1e-8, 1, 1.0, None)
    assert rc == -1 and b"multiple of 4" in lib.tg_last_error() and b"tg_adam_multi:" in lib.tg_last_error()
    rc = lib.tg_adam_multi_s(NN, NN, 1, chunk, 0.9, 0.999, 1e-8, NN, 1.0, None)
    assert rc == -1 and b"multiple of 4" in lib.tg_last_error() and b"tg_adam_multi_s:" in lib.tg_last_error()


def test_pointwise_null_and_zero_arguments_are_refused(lib):
    def refused(rc, name):
        assert rc == -1 and name in lib.tg_last_error(), (rc, lib.tg_last_error())

    ws = 1 << 20
    # pixel losses: null tensors, H or W of 1 (no differences to take), workspace too small
    refused(lib.tg_pixel_losses(None, NN, NN, None, 1, 4, 4, 1.0, 0.1, 0.5, 1e-6, None, NN, None, 0, NN, ws, None), b"tg_pixel_losses")
    refused(lib.tg_pixel_losses(NN, NN, None, None, 1, 4, 4, 1.0, 0.1, 0.5, 1e-6, None, NN, None, 0, NN, ws, None), b"tg_pixel_losses")
    refused(lib.tg_pixel_losses(NN, NN, NN, None, 1, 4, 4, 1.0, 0.1, 0.5, 1e-6, None, None, None, 0, NN, ws, None), b"tg_pixel_losses")
    for B, H, W in ((0, 4, 4), (1, 1, 4), (1, 4, 1)):
        refused(lib.tg_pixel_losses(NN, NN, NN, None, B, H, W, 1.0, 0.1, 0.5, 1e-6, None, NN, None, 0, NN, ws, None), b"bad dims")
    assert lib.tg_pixel_loss_ws_bytes(1, 64, 64) > 8
    refused(lib.tg_pixel_losses(NN, NN, NN, None, 1, 64, 64, 1.0, 0.1, 0.5, 1e-6, None, NN, None, 0, NN, 8, None), b"workspace")
    # reductions
    for fn in (lib.tg_l1_mean, lib.tg_l1_mean_relu):
        refused(fn(None, NN, 4, 1.0, None, NN, None, NN, ws, None), b"tg_l1_mean")
        refused(fn(NN, NN, 0, 1.0, None, NN, None, NN, ws, None), b"tg_l1_mean")
        refused(fn(NN, NN, 1 << 20, 1.0, None, NN, None, NN, 8, None), b"workspace")
    refused(lib.tg_bce_logits(None, 4, 1.0, 1.0, None, NN, None, NN, ws, None), b"tg_bce_logits")
    refused(lib.tg_bce_logits(NN, 0, 1.0, 1.0, None, NN, None, NN, ws, None), b"tg_bce_logits")
    refused(lib.tg_bce_logits(NN, 1 << 20, 1.0, 1.0, None, NN, None, NN, 8, None), b"workspace")
    # head
    refused(lib.tg_sigmoid_composite_fwd(NN, NN, None, 4, NN, None), b"tg_sigmoid_composite_fwd")
    refused(lib.tg_sigmoid_composite_fwd(NN, NN, NN, 0, NN, None), b"tg_sigmoid_composite_fwd")
    refused(lib.tg_sigmoid_composite_bwd(NN, None, NN, 4, NN, None, None), b"tg_sigmoid_composite_bwd")
    refused(lib.tg_sigmoid_composite_bwd(NN, NN, NN, 0, NN, None, None), b"tg_sigmoid_composite_bwd")
    # layouts, BN eval statistics, act_bwd
    for fn, nm in ((lib.tg_nchw_to_nhwc, b"tg_nchw_to_nhwc"), (lib.tg_nhwc_to_nchw, b"tg_nhwc_to_nchw")):
        refused(fn(None, 1, 2, 3, 4, NN, None), nm)
        refused(fn(NN, 1, 0, 3, 4, NN, None), nm)
    refused(lib.tg_bn_eval_stats(NN, None, 4, 1e-5, NN, NN, None), b"tg_bn_eval_stats")
    refused(lib.tg_bn_eval_stats(NN, NN, 0, 1e-5, NN, NN, None), b"tg_bn_eval_stats")
    refused(lib.tg_act_bwd(None, NN, 4, 4, 1, 0.0, None, NN, None), b"tg_act_bwd")
    refused(lib.tg_act_bwd(NN, NN, 0, 4, 1, 0.0, None, NN, None), b"tg_act_bwd")
    refused(lib.tg_act_bwd(NN, None, 4, 4, 1, 0.0, None, NN, None), b"forward output")
    # Adam and the elementwise helpers
    refused(lib.tg_adam(NN, None, NN, NN, 4, 2e-4, 0.9, 0.999, 1e-8, 1, 1.0, None), b"tg_adam")
    refused(lib.tg_adam(NN, NN, NN, NN, 0, 2e-4, 0.9, 0.999, 1e-8, 1, 1.0, None), b"tg_adam")
    refused(lib.tg_adam(NN, NN, NN, NN, 4, 2e-4, 0.9, 0.999, 1e-8, 0, 1.0, None), b"tg_adam")
    refused(lib.tg_adam_multi(None, NN, 1, 16384, 2e-4, 0.9, 0.999, 1e-8, 1, 1.0, None), b"tg_adam_multi")
    refused(lib.tg_adam_multi(NN, NN, 0, 16384, 2e-4, 0.9, 0.999, 1e-8, 1, 1.0, None), b"tg_adam_multi")
    refused(lib.tg_adam_multi(NN, NN, 1, 0, 2e-4, 0.9, 0.999, 1e-8, 1, 1.0, None), b"tg_adam_multi")
    refused(lib.tg_adam_multi(NN, NN, 1, 16384, 2e-4, 0.9, 0.999, 1e-8, 0, 1.0, None), b"tg_adam_multi")
    refused(lib.tg_adam_multi_s(NN, NN, 1, 16384, 0.9, 0.999, 1e-8, None, 1.0, None), b"tg_adam_multi_s")
    refused(lib.tg_adam_multi_s(NN, NN, 1, -4, 0.9, 0.999, 1e-8, NN, 1.0, None), b"tg_adam_multi_s")
    vals = np.zeros(16, np.float32)
    vp = C.c_void_p(vals.ctypes.data)
    for n in (0, 17):
        refused(lib.tg_write_floats(NN, n, vp, None), b"tg_write_floats")
    refused(lib.tg_write_floats(None, 2, vp, None), b"tg_write_floats")
    refused(lib.tg_write_floats(NN, 2, None, None), b"tg_write_floats")
    refused(lib.tg_axpby(None, 1.0, 0.0, NN, 4, None), b"tg_axpby")
    refused(lib.tg_axpby(NN, 1.0, 0.0, NN, 0, None), b"tg_axpby")
    refused(lib.tg_lincomb(NN, 1.0, None, 1.0, NN, 4, None), b"tg_lincomb")
    refused(lib.tg_lincomb(NN, 1.0, NN, 1.0, NN, 0, None), b"tg_lincomb")
    refused(lib.tg_mul(NN, None, NN, 4, None), b"tg_mul")
    refused(lib.tg_mul(NN, NN, NN, 0, None), b"tg_mul")
    refused(lib.tg_mul_keep(NN, NN, NN, None, 4, None), b"tg_mul_keep")
    refused(lib.tg_mul_keep(NN, NN, NN, NN, 0, None), b"tg_mul_keep")


def test_adam_table_key_distinguishes_equal_pointers_with_other_counts():
    """adam_multi_'s device table stores each segment's element count, so the count belongs to the key the table is cached under:
    views of other lengths at the same four pointers are another table."""
    from tg_hip import ops as O
    bufs = [torch.zeros(1000) for _ in range(4)]
    long_ = [[b[:1000]] for b in bufs]
    short = [[b[:10]] for b in bufs]
    assert [t[0].data_ptr() for t in long_] == [t[0].data_ptr() for t in short]
    k_long, k_short = O.adam_table_key(*long_), O.adam_table_key(*short)
    assert k_long != k_short
    assert k_long == O.adam_table_key(*[[b[:1000]] for b in bufs]) and hash(k_long) == hash(O.adam_table_key(*long_))
    # a 2-D view of the same storage and count is the same table; another pointer is not
    assert O.adam_table_key(*[[b.view(10, 100)] for b in bufs]) == k_long
    assert O.adam_table_key(*[[b[1:1000]] for b in bufs]) != O.adam_table_key(*[[b[:999]] for b in bufs])
    two = [[b[:10], b[500:600]] for b in bufs]
    two_other = [[b[:10], b[500:601]] for b in bufs]
    assert O.adam_table_key(*two) != O.adam_table_key(*two_other)
