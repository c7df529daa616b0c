"""The direct convolution kernels (csrc/igemm.hip: igemm_kernel, igemm_multi_kernel, pgemm_kernel, wgrad_kernel, the split-K
second passes, slab_reduce_kernel; all of csrc/smallconv.hip), one route per case (tests/conv_cases.py).

Every case asserts from the launch records that exactly the expected kernel ran -- (kind, cfg, route) of every launch and its
split count -- and then faces two references that need no measured tolerance (tests/conv_oracle.py):
  - exact: small-integer data, so that every fp32 summation order gives the same bits; torch.equal with the fp64 reference;
  - real: normals with ratio / LeakyReLU / gates / accumulate base; |hip - ref| <= n 2^-24 S |scale| per element.
The routes behind an environment switch that the library reads once per process run in one fresh child process per switch.
The bf16-operand instantiations of the same kernels face the same two runs, through the same run_case, in
tests/test_hip_bf16_direct.py."""
import csv
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests import conv_cases as CC
from tests import conv_oracle as CO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


class Routes:
    """(kind, cfg, route) and splits of the conv launches issued inside the block, in launch order."""

    def __init__(self, path):
        from tg_hip import lib as L
        self.lib, self.path, self.rows, self.splits = L.load(), str(path), [], []

    def _drop(self):
        for kind in (0, 1, 2, 3):
            self.lib.tg_prof_summary(kind, None, None, None, None)

    def __enter__(self):
        self._drop()
        self.lib.tg_prof_enable(1)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.lib.tg_prof_enable(0)
        assert self.lib.tg_prof_dump(self.path.encode()) == 0
        with open(self.path) as f:
            reader = csv.DictReader(f)
            assert reader.fieldnames[-1] == "route", reader.fieldnames
            rows = list(reader)
        self.rows = [(int(r["kind"]), int(r["cfg"]), int(r["route"])) for r in rows]
        self.splits = [int(r["splits"]) for r in rows]
        self._drop()
        return False


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _weight(d, dev):
    """The OIHW parameter whose storage is the kernels' [Cout][k][k][Cin]."""
    return _dev(d["w"], dev).permute(0, 3, 1, 2)


def _bn(d, dev):
    return None if d["bn"] is None else tuple(_dev(t, dev) for t in d["bn"][:4]) + tuple(d["bn"][4:])


def _forward(case, d, mode, dev, bias):
    from tg_hip import ops as O
    B, H, W, Cin, Cout, k, s, pad = case.geom
    a, sl = CC.fwd_act(case, mode)
    x, w = _dev(d["x"], dev), _weight(d, dev)
    if d["bn"] is not None:
        return O.conv_fwd_bnin(x, _bn(d, dev), w, _dev(bias, dev), k, s, pad, act=a, slope=sl)
    return O.conv_fwd(x, w, _dev(bias, dev), k, s, pad, in_mask=_dev(d["mask"], dev), ratio=_dev(d["ratio"], dev), act=a, slope=sl)


def launch(case, d, mode, dev):
    """Runs the case's op on the GPU: {'y' | 'dx' | 'dw', 'db'} -> tensor in the oracle's layout."""
    from tg_hip import ops as O
    B, H, W, Cin, Cout, k, s, pad = case.geom
    if case.op == "fwd":
        return {"y": _forward(case, d, mode, dev, d["bias"])}
    if case.op == "dgrad":
        dy, w = _dev(d["dy"], dev), _weight(d, dev)
        if "map" in case.mods:
            both = torch.cat([_dev(d["pred"], dev), _dev(d["tgt"], dev)]).contiguous()
            sm = O.vgg_sparse_map(both, B, "C", mask=_dev((~d["needed"]).astype(np.float32), dev))
            assert sm is not None and sm.for_bwd
            out = torch.full((B, H, W, Cin), float("nan"), device=dev)
            return {"dx": O.conv_dgrad(dy, w, (B, H, W, Cin), k, s, pad, out=out, sparse=sm.maps[0])}
        return {"dx": O.conv_dgrad(dy, w, (B, H, W, Cin), k, s, pad, in_mask=_dev(d["mask"], dev), out=_dev(d["base"], dev),
                                   gate=_dev(d["gate"], dev), gate_act=O.ACT_RELU if mode == "exact" else O.ACT_LEAKY,
                                   gate_slope=CC.LEAKY_SLOPE)}
    dw, db = O.conv_wgrad(_dev(d["x"], dev), _dev(d["dy"], dev), _weight(d, dev), k, s, pad, in_mask=_dev(d["mask"], dev),
                          want_bias="bias" in case.mods, in_bn=_bn(d, dev))
    out = {"dw": dw.permute(0, 2, 3, 1)}
    if "bias" in case.mods:
        out["db"] = db
    return out


def launch_as_asked(case, d, mode, dev):
    """`launch` under the precision and the per-call switch the case names, both restored afterwards."""
    from tg_hip import ops as O
    try:
        O.set_precision(case.prec)
        if case.setenv:
            os.environ[case.setenv] = "1"
        out = launch(case, d, mode, dev)
        torch.cuda.synchronize()
        return out
    finally:
        O.set_precision("f32")
        if case.setenv:
            os.environ.pop(case.setenv, None)


def run_case(case, dev, csv_path, table=CC, launch_fn=None):
    """The runs of a case (both, unless the case names its own); returns [(output name, err / bound of the real run)].  Raises
    AssertionError on any miss.  `table`: the case module (conv_cases, or wino_cases with `launch_fn` its launcher, which sets
    and restores whatever process-wide state the case asks for around the launch).  Only the launch under test runs at the
    case's precision: the forward a backward case derives its dy from is an fp32 one, whatever the case asks for."""
    from tg_hip import ops as O
    assert O.get_precision() == "f32", "fp32 outside the launch: a case names its precision, and only its launch runs under it"
    launch_fn = launch_fn or launch_as_asked
    figures = []
    for mode in getattr(case, "runs", ("exact", "real")):
        d = table.make_inputs(case, mode)
        if table.needs_forward(case, mode):
            y = _forward(case, d, mode, dev, None)
            d["dy"] = table.backward_dy(case, d, mode, y.cpu().numpy())
        ref = table.reference(case, d, mode)
        with Routes(csv_path) as rt:
            out = launch_fn(case, d, mode, dev)
        assert rt.rows == case.expect, f"{case.id} ({mode}): launches {rt.rows}, expected {case.expect}"
        assert table.splits_ok(case.splits, rt.splits), f"{case.id} ({mode}): splits {rt.splits}, expected {case.splits}"
        slabs = table.slab_cap(case, case.expect)
        for name, r in ref.items():
            got = out[name].detach().cpu()
            assert tuple(got.shape) == r.val.shape, (name, tuple(got.shape), r.val.shape)
            if mode == "exact":
                assert CO.exact_ok(r)
                want = torch.from_numpy(r.val).float()
                assert torch.equal(want.double(), torch.from_numpy(r.val)), "the reference is not an fp32 integer"
                bad = int((got != want).sum()) if got.shape == want.shape else -1
                assert torch.equal(got, want), \
                    f"{case.id} {name}: {bad} of {want.numel()} elements differ from the exact result " \
                    f"(largest difference {float((got.double() - want.double()).abs().max()):.0f})"
            else:
                q, where = CO.worst(got.numpy(), r, slabs)
                print(f"ERR_OVER_BOUND {case.id} {name} routes={sorted(set(case.expect))} {q:.4f}")
                figures.append((name, q))
                assert q <= 1.0, f"{case.id} {name}: error at {q:.3f} of the a-priori bound (flat element {where})"
    return figures


@pytest.mark.parametrize("case", CC.HERE, ids=[c.id for c in CC.HERE])
def test_direct_conv(dev, case, tmp_path):
    t0 = time.perf_counter()
    run_case(case, dev, tmp_path / "launches.csv")
    print(f"CASE_SECONDS {case.id} {time.perf_counter() - t0:.2f}")


def child_main(env, table=CC, launch_fn=None, marker="DIRECT_CONV_CHILD_OK"):
    """Body of the child process of one switch (`env`: NAME or NAME=value): its cases, a verdict line each, and the closing line
    the parent looks for."""
    import tempfile
    assert os.environ.get(env.split("=")[0]), env
    from tg_hip import lib
    lib.load()
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        for case in (c for c in table.CASES if c.env == env):
            t0 = time.perf_counter()
            run_case(case, dev, os.path.join(tmp, "launches.csv"), table, launch_fn)
            print(f"CASE_OK {case.id}")
            print(f"CASE_SECONDS {case.id} {time.perf_counter() - t0:.2f}")
    print(f"{marker} {env}")


def run_child(env, module, table, marker):
    """One fresh child process for the switch `env` (NAME, set to 1, or NAME=value): `module`.child_main(env) runs its cases."""
    name, _, value = env.partition("=")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'terra-gan_amd')!r}]\n" \
           f"from tests.{module} import child_main\nchild_main({env!r})\n"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{name: value or "1"}), cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and f"{marker} {env}" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.count("CASE_OK ") == sum(1 for c in table.CASES if c.env == env)


@pytest.mark.parametrize("env", CC.ENVS)
def test_direct_conv_behind_switch(dev, env):
    """TG_NO_C1MFMA / TG_C1WGRAD / TG_NO_TO1LDS are read once per process: the plain kernels they select run in a child."""
    run_child(env, "test_hip_direct_conv", CC, "DIRECT_CONV_CHILD_OK")
