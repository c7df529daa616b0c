"""tests/conv_oracle.py and tests/conv_cases.py on the CPU, for every case of the table: the fp64 oracle against float64 autograd
(F.conv2d, torch.nn.grad.conv2d_weight), the exactness condition of the integer run, fp32 PyTorch-CPU inside the a-priori bound
the kernels face, and the table's expected route against the Python restatement of the planners."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as CC
from tests import conv_oracle as CO


def _t(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _nchw(a, dtype):
    return _t(a, dtype).permute(0, 3, 1, 2)


def _act(v, kind, slope):
    return torch.relu(v) if kind == CO.ACT_RELU else (F.leaky_relu(v, slope) if kind == CO.ACT_LEAKY else v)


def _source(d, dtype):
    x = _nchw(d["x"], dtype)
    if d["bn"] is not None:
        mean, rstd, gamma, beta = (_t(t, dtype).view(1, -1, 1, 1) for t in d["bn"][:4])
        x = _act(((x - mean) * rstd) * gamma + beta, d["bn"][4], d["bn"][5])
    if d["mask"] is not None:
        x = x * _t(d["mask"], dtype).unsqueeze(1)
    return x


def torch_run(case, d, mode, dtype):
    """The case in plain PyTorch at `dtype`, in the oracle's layouts."""
    B, H, W, Cin, Cout, k, s, pad = case.geom
    w = _t(d["w"], dtype).permute(0, 3, 1, 2)
    a, sl = CC.fwd_act(case, mode)
    if case.op == "fwd":
        z = F.conv2d(_source(d, dtype), w, _t(d["bias"], dtype), s, pad)
        if d["ratio"] is not None:
            z = z * _t(d["ratio"], dtype).unsqueeze(1)
        return {"y": _act(z, a, sl).permute(0, 2, 3, 1)}
    dy = _nchw(d["dy"], dtype)
    if case.op == "dgrad":
        x = torch.zeros(B, Cin, H, W, dtype=dtype, requires_grad=True)
        F.conv2d(x, w, None, s, pad).backward(dy)
        dx = x.grad
        if d["mask"] is not None:
            dx = dx * _t(d["mask"], dtype).unsqueeze(1)
        if d["gate"] is not None:
            g = _nchw(d["gate"], dtype)
            dx = dx * torch.where(g > 0, torch.ones((), dtype=dtype), torch.full((), 0.0 if mode == "exact" else CC.LEAKY_SLOPE, dtype=dtype))
        if "map" in case.mods:
            dx = dx * _t(d["needed"], dtype).unsqueeze(1)
        if d["base"] is not None:
            dx = dx + _nchw(d["base"], dtype)
        return {"dx": dx.permute(0, 2, 3, 1)}
    dw = torch.nn.grad.conv2d_weight(_source(d, dtype), (Cout, Cin, k, k), dy, s, pad)
    out = {"dw": dw.permute(0, 2, 3, 1)}
    if "bias" in case.mods:
        out["db"] = dy.sum(dim=(0, 2, 3))
    return out


def _inputs(case, mode):
    d = CC.make_inputs(case, mode)
    if CC.needs_forward(case, mode):
        a = CC.forward_args(case, d, mode)
        y32 = torch_run(CC.Case("fwd", case.geom, "fwd", " ".join(case.mods - {"bias"}), (0, 0, 0)), dict(d, bias=None), mode,
                        torch.float32)["y"]
        assert tuple(y32.shape) == CO.conv_fwd(**a).val.shape
        d["dy"] = CC.backward_dy(case, d, mode, y32.numpy())
    return d


@pytest.mark.parametrize("case", CC.CASES, ids=[c.id for c in CC.CASES])
def test_expected_route_follows_from_the_geometry(case):
    routes, splits = CC.predict(case)
    assert routes == case.expect
    assert CC.splits_ok(case.splits, splits), (case.splits, splits)
    if isinstance(case.splits, tuple):
        assert splits == [case.splits]
        if case.id.startswith("multi") and "per_class" in case.id:
            assert len(set(case.splits)) > 1
    assert CC.slab_cap(case, routes) >= max(max(s) if isinstance(s, tuple) else s for s in splits)
    if case.op == "wgrad":
        assert CC.slab_cap(case, routes) >= CC.wgrad_slabs(case.geom, routes[0][2])


@pytest.mark.parametrize("mode", ["exact", "real"])
@pytest.mark.parametrize("case", CC.CASES, ids=[c.id for c in CC.CASES])
def test_oracle_against_autograd_and_fp32_inside_the_bound(case, mode):
    d = _inputs(case, mode)
    ref = CC.reference(case, d, mode)
    t64 = torch_run(case, d, mode, torch.float64)
    slabs = CC.slab_cap(case, case.expect)
    for name, r in ref.items():
        got = t64[name].numpy()
        assert got.shape == r.val.shape, (name, got.shape, r.val.shape)
        if mode == "exact":
            assert CO.exact_ok(r), f"{name}: max S = {float(r.S.max()):.0f} is not below 2^24"
            assert np.array_equal(got, r.val), name
            assert np.array_equal(np.rint(r.val), r.val)
        else:
            # two fp64 evaluations of the same sums: each inside n * 2^-53 * S of the true value
            assert bool((np.abs(got - r.val) <= 2 * CO.bound(r, slabs) * 2.0 ** -29).all()), name
    if mode == "real":
        t32 = torch_run(case, d, mode, torch.float32)
        for name, r in ref.items():
            q, where = CO.worst(t32[name].numpy(), r, slabs)
            assert q <= 1.0, f"{name}: fp32 PyTorch-CPU at {q:.3f} of the a-priori bound (element {where})"


def test_table_is_complete():
    """Every route value of SmallRoute and every MFMA tag of the direct kernels is expected by some case."""
    seen = {e for c in CC.CASES for e in c.expect}
    for cfg in (32, 33, 64, 65, 128, 129, 1064, 1128, 564, 628):
        assert (0, cfg, 0) in seen, cfg
    for bm in (32, 64, 128):
        assert (1, bm, 0) in seen, bm
    fwd = [CC.SR_C1MFMA + k for k in (7, 4, 3)] + [CC.SR_C1CONV + k for k in (7, 4, 3, 0)] + \
        [CC.SR_TO1CONVW + v for v in (31, 32, 41, 42)] + [CC.SR_TO1_LDS, CC.SR_TO1_LDS_BNIN, CC.SR_TO1_LDS_MAP] + \
        [CC.SR_TO1CONV64 + v for v in (33, 22, 44, 11, 21, 12)]
    for r in fwd:
        assert (2, CC.SMALL_FWD, r) in seen, r
    for r in (CC.SR_MULTI22_LDS, CC.SR_MULTI22):
        assert (2, CC.TO1_MULTI, r) in seen, r
    wg = [b + k for b in (CC.SR_C1WGRAD_MFMA, CC.SR_C1WGRAD_MFMA_BIAS, CC.SR_C1WGRAD) for k in (7, 4, 3)] + \
        [CC.SR_TO1WGRADW + 3, CC.SR_TO1WGRADW + 4, CC.SR_TO1WGRAD_LDS, CC.SR_TO1WGRAD_LDS_BNIN, CC.SR_TO1WGRAD64 + 3, CC.SR_TO1WGRAD64 + 4]
    for r in wg:
        assert (2, CC.SMALL_WGRAD, r) in seen, r
    assert len({c.env for c in CC.CASES if c.env}) <= 4
