"""The Winograd kernels (csrc/wino.inc, wino16.inc, wino22.inc, wino44.inc), one kernel instantiation per case (tests/wino_cases.py),
on the helpers of tests/test_hip_direct_conv.py.

Every case asserts from the launch records that exactly the expected instantiation ran -- (kind, cfg, route) with route =
WinoRoute (csrc/igemm_params.h), and the split count -- and then faces the references of tests/conv_oracle.py, which hold no
measured number:
  - exact: small-integer data.  The transforms of F(2x2,3x3), F(3x3,2x2) and F(2x2,2x2) have coefficients +-1 and 1/2 only, so
    every intermediate of every summation order, split-K plan and work distribution is an fp32 (and, transformed, a bf16) number:
    torch.equal with the fp64 reference;
  - real: normals with ratio / LeakyReLU / gates / accumulate base; |hip - ref| <= n 2^-24 (S_w |scale| + |base|) per element,
    S_w the sum of absolute values of the Winograd-domain expression.  F(4x4,3x3), whose 1/6 and 1/24 round, faces this run only;
  - rounded, the bf16 kernels (wino16.inc) in place of the real run: integers of eleven bits and more, on which the fp32
    transforms are exact and the bf16 rounding of the transformed operands is not the identity, against the reference that rounds
    V / U (wgrad: A dY At / Bt X B) to nearest-even and nothing else: the same per-element bound, with S_w from the rounded
    operands.  tests/test_wino_oracle_cpu.py shows per case that truncation, round-half-away and a rounding of x / w / dy ahead of
    the transforms lie outside it.
The switches the library reads once per process (TG_WINO_NO_PIPE, TG_WINO_NO_FAST, TG_WINO_INTERLEAVE) run in one fresh child
process each."""
import time

import numpy as np
import pytest
import torch

from tests import wino_cases as WC
from tests.test_hip_direct_conv import _dev, _weight, child_main as _child_main, dev, run_case, run_child  # noqa: F401

pytestmark = pytest.mark.gpu


def _once(case, d, mode, dev):
    from tg_hip import ops as O
    B, H, W, Cin, Cout, k, s, pad = case.geom
    wino4 = "wino4" in case.mods
    if case.op == "fwd":
        a, sl = WC.fwd_act(case, mode)
        y = O.conv_fwd(_dev(d["x"], dev), _weight(d, dev), _dev(d["bias"], dev), k, s, pad, in_mask=_dev(d["mask"], dev),
                       ratio=_dev(d["ratio"], dev), act=a, slope=sl, wino4=wino4, pool="pool" in case.mods)
        if "pool" in case.mods:
            y, yp = y
            assert np.array_equal(yp.cpu().numpy(), WC.pool2(y.cpu().numpy())), f"{case.id}: the fused pool is not the maximum of y"
        return {"y": y}
    if case.op == "dgrad":
        ga, gs = WC.gate_act(case, mode)
        bits = gate = None
        if "gbits" in case.mods:
            bits = O.relu_gate_pack(_dev(d["gate"], dev))
        else:
            gate = _dev(d["gate"], dev)
        return {"dx": O.conv_dgrad(_dev(d["dy"], dev), _weight(d, dev), (B, H, W, Cin), k, s, pad, in_mask=_dev(d["mask"], dev),
                                   out=_dev(d["base"], dev), gate=gate, gate_act=ga, gate_slope=gs, wino4=wino4, gate_bits=bits)}
    dw, db = O.conv_wgrad(_dev(d["x"], dev), _dev(d["dy"], dev), _weight(d, dev), k, s, pad, want_bias="bias" in case.mods)
    out = {"dw": dw.permute(0, 2, 3, 1).contiguous()}
    if "bias" in case.mods:
        out["db"] = db
    return out


def launch(case, d, mode, dev):
    """The case's op under the process-wide state it asks for (precision, CU reserve, work stealing), restored afterwards."""
    from tg_hip import lib as L
    from tg_hip import ops as O
    lib = L.load()
    try:
        O.set_precision(case.prec)
        if case.ctx == "reserve":
            L.check(lib.tg_set_cu_reserve(128), "tg_set_cu_reserve")
        if case.ctx == "steal":
            L.check(lib.tg_set_work_stealing(2), "tg_set_work_stealing")
        out = _once(case, d, mode, dev)
        if "twice" in case.mods:        # slabs reduced in a fixed order: a repeated launch gives the same bits
            again = _once(case, d, mode, dev)
            for name in out:
                assert torch.equal(out[name], again[name]), f"{case.id} {name}: a repeated launch gave other bits"
        torch.cuda.synchronize()
        return out
    finally:
        O.set_precision("f32")
        L.check(lib.tg_set_cu_reserve(0), "tg_set_cu_reserve")
        L.check(lib.tg_set_work_stealing(0), "tg_set_work_stealing")


@pytest.mark.parametrize("case", WC.HERE, ids=[c.id for c in WC.HERE])
def test_wino_route(dev, case, tmp_path):
    t0 = time.perf_counter()
    run_case(case, dev, tmp_path / "launches.csv", WC, launch)
    print(f"CASE_SECONDS {case.id} {time.perf_counter() - t0:.2f}")


def child_main(env):
    _child_main(env, WC, launch, "WINO_ROUTES_CHILD_OK")


@pytest.mark.parametrize("env", WC.ENVS)
def test_wino_route_behind_switch(dev, env):
    """TG_WINO_NO_PIPE / TG_WINO_NO_FAST / TG_WINO_INTERLEAVE are read once per process: their cases run in a child."""
    run_child(env, "test_hip_wino_routes", WC, "WINO_ROUTES_CHILD_OK")
