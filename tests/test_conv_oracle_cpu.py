"""tests/conv_oracle.py and tests/conv_cases.py on the CPU, for every case of the table: the fp64 oracle against float64 autograd
(F.conv2d, torch.nn.grad.conv2d_weight), the exactness condition of the integer run, fp32 PyTorch-CPU inside the a-priori bound
the kernels face, and the table's expected route against the Python restatement of the planners.  For the bf16-mode cases
(conv_cases.B16_CASES) in addition: bf16_rne against torch's conversion, and that the rounded-operand reference tells a kernel
that stayed fp32 and one that truncates from one that rounds to nearest even."""
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


# ---- bf16 mode (conv_cases.B16_CASES) ------------------------------------------------------------------------------------------------
def test_bf16_rne_is_torch_bfloat16():
    """conv_oracle.bf16_rne against torch's fp32 -> bf16 conversion, bit for bit: normals, exact ties of both parities, +-0, values
    just below a power of two (the carry moves the exponent), the largest finite fp32 (-> inf) and subnormals."""
    rng = np.random.default_rng(16)
    bits = lambda *u: np.array(u, np.uint32).view(np.float32)
    ties = bits(0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x40FF8000, 0x40FE8000)
    below = bits(0x3FFFFFFF, 0x3FFF8000, 0x3FFF7FFF, 0xBFFFFFFF, 0x407FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF)
    sub = bits(0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x007F8000, 0x80008000, 0x80018000, 0x00800000)
    a = np.concatenate([rng.standard_normal(4096, dtype=np.float32), rng.standard_normal(512, dtype=np.float32) * np.float32(1e-3),
                        rng.integers(0, 0x7F800000, 4096, dtype=np.uint32).view(np.float32), ties, below, sub,
                        np.array([0.0, -0.0, 1.0, -1.0, 3.0, -3.0], np.float32)])
    got = CO.bf16_rne(a)
    want = torch.from_numpy(a).bfloat16().float().numpy()
    assert got.dtype == np.float32 and got.shape == a.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the ties go to the even neighbour, in both directions; the largest finite value leaves the range
    assert np.array_equal(CO.bf16_rne(ties[:4]).view(np.uint32), np.array([0x3F800000, 0x3F820000, 0xBF800000, 0xBF820000], np.uint32))
    assert np.isinf(CO.bf16_rne(bits(0x7F7FFFFF))[0]) and np.signbit(CO.bf16_rne(np.float32(-0.0)))
    assert CO.bf16_rne(np.ones((2, 3), np.float32)).shape == (2, 3)
    # truncation is another function, and differs where the dropped half is above a half
    assert np.array_equal(CO.bf16_trunc(ties[:2]).view(np.uint32), np.array([0x3F800000, 0x3F810000], np.uint32))


@pytest.mark.parametrize("case", CC.B16_CASES, ids=[c.id for c in CC.B16_CASES])
def test_bf16_expected_route_follows_from_the_geometry(case):
    assert case.prec == "bf16"
    routes, splits = CC.predict(case)
    assert routes == case.expect
    assert CC.splits_ok(case.splits, splits), (case.splits, splits)
    if isinstance(case.splits, tuple):
        assert splits == [case.splits]
    assert CC.slab_cap(case, routes) >= max(max(s) if isinstance(s, tuple) else s for s in splits)
    if case.op == "wgrad":
        assert CC.slab_cap(case, routes) >= CC.wgrad_slabs(case.geom, routes[0][2])
    # a case that keeps its fp32 kernel has that kernel's record; every other one a record of kind 3 that no other launcher writes
    kinds = {kind for kind, _, _ in case.expect}
    assert kinds == {3} if case.rounds else 3 not in kinds
    assert case.id.startswith("b16_keeps_") != case.rounds
    if case.id.startswith("b16_keeps_") and not case.setenv and case.id[len("b16_keeps_"):] in CC.BY_ID:
        assert case.expect == CC.BY_ID[case.id[len("b16_keeps_"):]].expect


def test_bf16_table_is_complete():
    """Every record of the four bf16 direct launchers is expected by some case, each at both tile sizes; no two launchers share one,
    and none is a cfg the benchmark's kernel report names."""
    seen = {e for c in CC.B16_CASES for e in c.expect}
    want = [3064, 3128, 3264, 3328, 3564, 3628, 3764, 3828]
    for cfg in want:
        assert (3, cfg, 0) in seen, cfg
    assert sorted(CC.B16_CFG.values()) + [3764, 3828] == want
    assert not set(want) & {4064, 4164, 4016, 4022, 4122, 4044, 1128, 1064}
    assert {e for e in seen if e[0] == 3} == {(3, cfg, 0) for cfg in want}


@pytest.mark.parametrize("case", CC.B16_CASES, ids=[c.id for c in CC.B16_CASES])
def test_bf16_exact_run_is_exact(case):
    """The integer run of a bf16 case: its operands are bf16 numbers (rounding leaves them alone), and every partial sum is an
    integer below 2^24, so the bf16 kernels owe the same bits as the fp32 ones."""
    d = _inputs(case, "exact")
    for name in CC.OPERANDS[case.op]:
        assert np.array_equal(CO.bf16_rne(d[name]), d[name]) and np.array_equal(CO.bf16_trunc(d[name]), d[name]), name
    ref = CC.reference(case, d, "exact")
    t64 = torch_run(case, d, "exact", torch.float64)
    for name, r in ref.items():
        assert CO.exact_ok(r), f"{name}: max S = {float(r.S.max()):.0f} is not below 2^24"
        assert np.array_equal(t64[name].numpy(), r.val) and np.array_equal(np.rint(r.val), r.val), name


@pytest.mark.parametrize("case", CC.B16_CASES, ids=[c.id for c in CC.B16_CASES])
def test_bf16_real_run_can_tell(case):
    """The real run of a bf16 case.  On a bf16 kernel: the reference on rounded operands agrees with float64 autograd on them;
    fp32 PyTorch-CPU on the rounded operands lies inside the bound (it is not vacuous that way), while the reference of a kernel
    that stayed fp32 (unrounded operands) and of one that truncates both lie OUTSIDE it (nor the other way): a condition on the
    table's inputs, not a measurement of the kernels.  A case that keeps its fp32 kernel: the plain fp32 check."""
    d = _inputs(case, "real")
    slabs = CC.slab_cap(case, case.expect)
    if not case.rounds:
        ref = CC.reference(case, d, "real")
        t32 = torch_run(case, d, "real", torch.float32)
        for name, r in ref.items():
            assert CO.worst(t32[name].numpy(), r, slabs)[0] <= 1.0, name
        return
    dr = CC.round_operands(case, d)
    ref = CC.reference(case, dr, "real")
    for name in CC.OPERANDS[case.op]:
        assert not np.array_equal(dr[name], d[name]), name
    t64, t32 = torch_run(case, dr, "real", torch.float64), torch_run(case, dr, "real", torch.float32)
    main = {"fwd": "y", "dgrad": "dx", "wgrad": "dw"}[case.op]
    r = ref[main]
    assert bool((np.abs(t64[main].numpy() - r.val) <= 2 * CO.bound(r, slabs) * 2.0 ** -29).all())
    q32 = CO.worst(t32[main].numpy(), r, slabs)[0]
    assert q32 <= 1.0, f"fp32 PyTorch-CPU on the rounded operands at {q32:.3f} of the a-priori bound"
    if "db" in ref:     # the bias gradient sums the dy as drawn
        plain = CC.reference(case, dict(d, dy_bias=d["dy"]), "real")["db"]
        assert np.array_equal(ref["db"].val, plain.val) and np.array_equal(ref["db"].S, plain.S)
    for what, rnd in (("unrounded", lambda a: a), ("truncated", CO.bf16_trunc)):
        other = CC.reference(case, CC.round_operands(case, d, rnd), "real")[main]
        q = CO.worst(other.val, r, slabs)[0]
        print(f"DISCRIMINATION {case.id} {main} {what} {q:.2f}")
        assert q > 1.0, f"the {what} operands' result lies within the bound ({q:.3f}): the real run could not tell"
