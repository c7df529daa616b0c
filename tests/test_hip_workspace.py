"""Workspace contract of the C ABI (include/terragan_hip.h: `ws` of tg_*_ws_bytes(...) bytes is enough), on the GPU.

tg_hip.ops hands every kernel one shared scratch buffer that only grows, so an entry point whose query under-reports passes
every other test.  Here `ops.workspace` is replaced by a guarded allocation: a 1 MiB head guard, then a 256-byte aligned region
of exactly what the query reported, then a tail guard of max(reported, 16 MiB).  The guards hold a fixed bit pattern, large
enough that an overrun stays inside the allocation.  Every case runs three times:
  - region poisoned with quiet NaN, then zeroed: the outputs are bit-identical (no read of scratch the call did not write);
  - region enlarged by 64 Mi floats: the outputs are bit-identical (the result does not depend on spare scratch);
and both guards are untouched after each run.  The outputs are held against a float64 CPU reference with the tolerances of
test_hip_ops.close (fp32) and test_hip_bf16 (bf16), and the route each conv took is asserted from the launch records.
"""
import csv
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HEAD = 1 << 18                 # floats: 1 MiB head guard (keeps the region 256-byte aligned)
TAIL_MIN = 1 << 22             # floats: 16 MiB
BIG = 64 << 20                 # floats added to the region for the size-independence run
CANARY = 0x5BADC0DE
POISON = {"nan": 0x7FC00000, "zero": 0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def close(a, b, rtol=1e-4, atol=1e-5):
    """tests/test_hip_ops.py::close, plus: finite wherever the reference is."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert bool(torch.isfinite(a)[torch.isfinite(b)].all()), "non-finite output where the reference is finite"
    err = (a - b).abs().max().item()
    assert err <= atol + rtol * b.abs().max().item(), f"max err {err:.3e} (ref max {b.abs().max().item():.3e})"


def close_bf16(a, b):
    """The bf16 bounds of tests/test_hip_bf16.py::test_wino16_fwd_dgrad."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    e = a - b
    assert float(e.norm() / b.norm()) < 6e-3, float(e.norm() / b.norm())
    assert float(e.abs().max()) < 3e-2 * float(b.abs().max()), (float(e.abs().max()), float(b.abs().max()))


class Guarded:
    """[head guard | region of exactly `nbytes` (rounded up to floats) + extra | tail guard] in one allocation."""

    def __init__(self, nbytes, dev, poison, extra=0):
        self.n = (int(nbytes) + 3) // 4
        self.region_n = self.n + extra
        self.tail = max(self.n, TAIL_MIN)
        self.buf = torch.empty(HEAD + self.region_n + self.tail, dtype=torch.int32, device=dev)
        self.buf[:HEAD].fill_(CANARY)
        self.buf[HEAD + self.region_n:].fill_(CANARY)
        self.buf[HEAD:HEAD + self.region_n].fill_(POISON[poison])
        self.region = self.buf[HEAD:HEAD + self.region_n].view(torch.float32)
        assert self.region.data_ptr() % 256 == 0

    def check(self, what):
        head = int((self.buf[:HEAD] != CANARY).sum())
        tail_bad = (self.buf[HEAD + self.region_n:] != CANARY).nonzero()
        assert head == 0, f"{what}: {head} head-guard words written"
        assert tail_bad.numel() == 0, \
            f"{what}: {tail_bad.numel()} tail-guard words written (reported {self.n} floats, last write at +{int(tail_bad.max()) + 1})"


class WsHarness:
    """Installs the guarded workspace as tg_hip.ops.workspace and runs a case in the three modes."""

    def __init__(self, monkeypatch, dev):
        from tg_hip import ops as O
        self.dev, self.mode, self.live = dev, ("nan", 0), []
        monkeypatch.setattr(O, "workspace", self._workspace)
        monkeypatch.setattr(O, "WPREP_CACHE", False)        # every conv prepares its weights inside the guarded region

    def _workspace(self, nbytes):
        g = Guarded(nbytes, self.dev, *self.mode)
        self.live.append(g)
        return g.region

    def run(self, what, fn):
        """fn() -> tuple of tensors.  Returns the outputs of the NaN-poisoned exact-size run."""
        outs = {}
        for mode in (("nan", 0), ("zero", 0), ("nan", BIG)):
            self.mode, self.live = mode, []
            o = tuple(t.clone() for t in fn())
            torch.cuda.synchronize()
            assert self.live, f"{what}: the op took no workspace"
            for g in self.live:
                g.check(f"{what} {mode}")
            self.live = []
            outs[mode] = o
        ref = outs[("nan", 0)]
        for mode in (("zero", 0), ("nan", BIG)):
            for i, (a, b) in enumerate(zip(ref, outs[mode])):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                    f"{what}: output {i} differs between NaN-poisoned exact scratch and {mode} " \
                    f"({int((a.view(torch.int32) != b.view(torch.int32)).sum())} elements)"
        return ref


class Routes:
    """Launch records (kind, cfg, splits) of the MFMA conv kernels issued inside the block."""

    def __init__(self, tmp_path):
        from tg_hip import lib as L
        self.lib, self.path, self.rows = L.load(), str(tmp_path / "launches.csv"), []

    def __enter__(self):
        for kind in (0, 1, 2, 3):
            self.lib.tg_prof_summary(kind, None, None, None, None)
        self.lib.tg_prof_enable(1)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.lib.tg_prof_enable(0)
        assert self.lib.tg_prof_dump(self.path.encode()) == 0
        self.rows = [(int(r["cfg"]), int(r["splits"])) for r in csv.DictReader(open(self.path))]
        for kind in (0, 1, 2, 3):
            self.lib.tg_prof_summary(kind, None, None, None, None)
        return False


IGEMM = {32, 33, 64, 65, 128, 129, 1064, 1128, 564, 628}      # gathered-row, patch and merged-class kernels (fp32)
WGRAD = {32, 64, 128}                                            # the MFMA wgrad kernel (bm)
SMALL_FWD, SMALL_WGRAD, TO1_MULTI = 2000, 2001, 2004
# id, (B, H, W, Cin, Cout, k, stride, pad), precision, masked, expected cfg of (fwd, dgrad, wgrad) or None, split-K expected in
CONV_CASES = [
    ("wino", (2, 20, 36, 64, 64, 3, 1, 1), "f32", False, ({4064}, {4064}, {4164}), ""),
    ("wino_splitk", (1, 16, 16, 512, 128, 3, 1, 1), "f32", False, ({4064}, {4064}, {4164}), "fd"),
    ("wino_odd", (3, 17, 23, 128, 64, 3, 1, 1), "f32", False, ({4064}, {4064}, {4164}), ""),
    ("wino44", (2, 32, 48, 64, 64, 3, 1, 1), "wino4", False, ({4044}, {4044}, {4164}), ""),
    ("wino16", (2, 32, 48, 64, 64, 3, 1, 1), "bf16", False, ({4016}, {4016}, {4116}), ""),
    ("wino22", (2, 32, 48, 64, 128, 4, 2, 1), "f32", False, ({4022}, {4022}, {4122}), ""),
    ("s2d_5x5", (2, 64, 96, 64, 128, 5, 2, 2), "f32", False, ({4064}, {4064}, {4164}), ""),
    ("igemm_splitk_4x4", (16, 4, 4, 512, 512, 3, 1, 1), "f32", True, (IGEMM, IGEMM, WGRAD), "fd"),
    ("igemm_splitk_8x8", (16, 8, 8, 512, 512, 3, 1, 1), "f32", True, (IGEMM, IGEMM, WGRAD), "fd"),
    ("enc7_s2", (16, 4, 4, 512, 512, 3, 2, 1), "f32", True, (IGEMM, IGEMM, WGRAD), ""),
    ("multiclass_dgrad", (2, 17, 23, 64, 128, 3, 2, 1), "f32", True, (IGEMM, IGEMM, WGRAD), ""),
    ("stride3", (2, 19, 25, 32, 64, 3, 3, 1), "f32", True, (IGEMM, IGEMM, WGRAD), ""),
    ("conv1x1", (3, 20, 12, 32, 64, 1, 1, 0), "f32", True, (IGEMM, IGEMM, WGRAD), ""),
    ("c1_k3", (2, 33, 44, 1, 64, 3, 1, 1), "f32", True, ({SMALL_FWD}, None, {SMALL_WGRAD}), ""),
    ("c1_k4_dconv0", (2, 37, 44, 1, 64, 4, 2, 1), "f32", False, ({SMALL_FWD}, None, {SMALL_WGRAD}), ""),
    ("c1_k7_enc1", (1, 29, 45, 1, 64, 7, 2, 3), "f32", True, ({SMALL_FWD}, None, {SMALL_WGRAD}), ""),
    ("to1_lds_final", (1, 16, 16, 64, 1, 3, 1, 1), "f32", False, ({SMALL_FWD}, None, {SMALL_WGRAD}), ""),
    ("to1_nolds", (2, 3, 20, 64, 1, 3, 1, 1), "f32", False, ({SMALL_FWD}, None, {SMALL_WGRAD}), ""),
    ("to1_multi_dgrad", (2, 18, 24, 1, 64, 4, 2, 1), "f32", False, ({SMALL_FWD}, {TO1_MULTI}, {SMALL_WGRAD}), ""),
    ("to1w_dlast", (2, 9, 13, 512, 1, 4, 1, 1), "f32", False, ({SMALL_FWD}, None, {SMALL_WGRAD}), ""),
    # the train step's own layers at g72x40b3 (tests/golden) and enc1 / D conv0 at B = 1, 488 x 976
    ("g72x40b3_enc1", (3, 72, 40, 1, 64, 7, 2, 3), "f32", True, ({SMALL_FWD}, None, {SMALL_WGRAD}), ""),
    ("g72x40b3_enc2", (3, 36, 20, 64, 128, 5, 2, 2), "f32", True, (None, None, None), ""),
    ("g72x40b3_dec1", (3, 72, 40, 64, 64, 3, 1, 1), "f32", True, (None, None, None), ""),
    ("g72x40b3_final", (3, 72, 40, 64, 1, 3, 1, 1), "f32", False, ({SMALL_FWD}, None, {SMALL_WGRAD}), ""),
    ("g72x40b3_dconv0", (3, 72, 40, 1, 64, 4, 2, 1), "f32", False, ({SMALL_FWD}, None, {SMALL_WGRAD}), ""),
    ("g72x40b3_dconv1", (3, 36, 20, 64, 128, 4, 2, 1), "f32", False, (None, None, None), ""),
    ("g72x40b3_dlast", (3, 4, 2, 512, 1, 4, 1, 1), "f32", False, (None, None, None), ""),
    ("enc1_b1_488x976", (1, 488, 976, 1, 64, 7, 2, 3), "f32", True, ({SMALL_FWD}, None, {SMALL_WGRAD}), ""),
    ("dconv0_b1_488x976", (1, 488, 976, 1, 64, 4, 2, 1), "f32", False, ({SMALL_FWD}, None, {SMALL_WGRAD}), ""),
]


def _set_prec(prec):
    from tg_hip import ops as O
    O.set_precision("bf16" if prec == "bf16" else "f32")


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_workspace_contract(dev, case, monkeypatch, tmp_path):
    from tg_hip import ops as O
    name, (B, H, W, Cin, Cout, k, s, p), prec, masked, expect, splitk = case
    h = WsHarness(monkeypatch, dev)
    wino4 = prec == "wino4"
    _set_prec(prec)
    try:
        g = torch.Generator().manual_seed(sum(case[1]))
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        x = torch.randn(B, H, W, Cin, generator=g)
        w = torch.randn(Cout, Cin, k, k, generator=g) / (k * Cin ** 0.5)
        bias = torch.randn(Cout, generator=g) * 0.1
        dy = torch.randn(B, Ho, Wo, Cout, generator=g)
        m = (torch.rand(B, H, W, generator=g) > 0.3).float() if masked else None
        xd, wd, bd, dyd = x.to(dev), w.contiguous(memory_format=torch.channels_last).to(dev), bias.to(dev), dy.to(dev)
        md = m.to(dev) if masked else None
        xm = x * m[..., None] if masked else x

        routes = {}
        with Routes(tmp_path) as r:
            y, = h.run(f"{name} fwd", lambda: (O.conv_fwd(xd, wd, bd, k, s, p, in_mask=md, wino4=wino4),))
        routes["fwd"] = r.rows
        with Routes(tmp_path) as r:
            dx, = h.run(f"{name} dgrad", lambda: (O.conv_dgrad(dyd, wd, (B, H, W, Cin), k, s, p, in_mask=md, wino4=wino4),))
        routes["dgrad"] = r.rows
        with Routes(tmp_path) as r:
            dw, db = h.run(f"{name} wgrad", lambda: O.conv_wgrad(xd, dyd, wd, k, s, p, in_mask=md))
        routes["wgrad"] = r.rows

        for (op, rows), want in zip(routes.items(), expect):
            cfgs = {c for c, _ in rows}
            if want is not None:
                assert cfgs & want, f"{name} {op}: ran {rows}, expected a cfg in {sorted(want)}"
            if op[0] in splitk:
                assert max(sp for c, sp in rows if c in (want or cfgs)) > 1, f"{name} {op}: no split-K launch in {rows}"

        ref_y = F.conv2d(_nchw(xm).double(), w.double(), bias.double(), s, p).permute(0, 2, 3, 1)
        xr = _nchw(x).double().requires_grad_(True)
        F.conv2d(xr, w.double(), None, s, p).backward(_nchw(dy).double())
        ref_dx = xr.grad.permute(0, 2, 3, 1) * (m[..., None].double() if masked else 1.0)
        ref_dw = torch.nn.grad.conv2d_weight(_nchw(xm).double(), (Cout, Cin, k, k), _nchw(dy).double(), stride=s, padding=p)
        ref_db = dy.double().sum((0, 1, 2))
        if prec == "bf16":
            close_bf16(y, ref_y)
            close_bf16(dx, ref_dx)
            close_bf16(dw.permute(0, 2, 3, 1).contiguous(), ref_dw.permute(0, 2, 3, 1))
            assert torch.allclose(db.cpu().double(), ref_db, atol=1e-3, rtol=1e-5)
        else:
            close(y, ref_y)
            close(dx, ref_dx)
            close(dw.permute(0, 2, 3, 1).contiguous(), ref_dw.permute(0, 2, 3, 1))
            close(db, ref_db)
    finally:
        O.set_precision("f32")


def _wprep_call(h, O, L, lib, g, mode, wv, wprep, xd, dyd, md):
    """tg_conv_fwd_p / tg_conv_dgrad_p with (or without: wprep None) prepared weights, workspace from the harness."""
    if mode == O.WPREP_FWD:
        y = torch.empty(g.B, g.Ho, g.Wo, g.Cout, device=xd.device)
        ws = O.workspace(lib.tg_conv_fwd_ws_bytes(C.byref(g)))
        L.check(lib.tg_conv_fwd_p(C.byref(g), O._p(xd), O._p(md), O._p(wv), O._p(wprep), None, None, 0, 0.0, O._p(y), O._p(ws),
                                  ws.numel() * 4, O._stream()), "tg_conv_fwd_p")
        return (y,)
    dx = torch.empty(g.B, g.H, g.W, g.Cin, device=xd.device)
    ws = O.workspace(lib.tg_conv_dgrad_ws_bytes(C.byref(g)))
    L.check(lib.tg_conv_dgrad_p(C.byref(g), O._p(dyd), O._p(wv), O._p(wprep), O._p(md), None, 0, 0.0, O._p(dx), 0, O._p(ws),
                                ws.numel() * 4, O._stream()), "tg_conv_dgrad_p")
    return (dx,)


WPREP_CASES = [c for c in CONV_CASES if c[0] in ("wino", "wino_splitk", "wino44", "wino16", "wino22", "s2d_5x5", "igemm_splitk_4x4",
                                                 "multiclass_dgrad", "stride3", "conv1x1")]


@pytest.mark.parametrize("case", WPREP_CASES, ids=[c[0] for c in WPREP_CASES])
def test_prepared_weights_contract(dev, case, monkeypatch):
    """tg_conv_wprep writes inside exactly tg_conv_wprep_bytes, and the prepared call equals the unprepared one bit for bit."""
    from tg_hip import lib as L, ops as O
    name, (B, H, W, Cin, Cout, k, s, p), prec, masked, _expect, _sk = case
    lib = L.load()
    h = WsHarness(monkeypatch, dev)
    _set_prec(prec)
    try:
        gen = torch.Generator().manual_seed(sum(case[1]) + 1)
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        xd = torch.randn(B, H, W, Cin, generator=gen).to(dev)
        dyd = torch.randn(B, Ho, Wo, Cout, generator=gen).to(dev)
        wv = (torch.randn(Cout, k, k, Cin, generator=gen) / (k * Cin ** 0.5)).to(dev)
        md = (torch.rand(B, H, W, generator=gen) > 0.3).float().to(dev) if masked else None
        g = L.TgConv(B, H, W, Cin, Ho, Wo, Cout, k, s, p, O._prec(prec == "wino4"))
        prepared = 0
        for mode in (O.WPREP_FWD, O.WPREP_DGRAD):
            nb = lib.tg_conv_wprep_bytes(C.byref(g), mode)
            if nb == 0:
                continue
            prepared += 1
            gw = Guarded(nb, dev, "nan")
            L.check(lib.tg_conv_wprep(C.byref(g), mode, O._p(wv), O._p(gw.region), O._stream()), "tg_conv_wprep")
            torch.cuda.synchronize()
            gw.check(f"{name} wprep mode {mode}")
            raw, = h.run(f"{name} raw {mode}", lambda: _wprep_call(h, O, L, lib, g, mode, wv, None, xd, dyd, md))
            prep, = h.run(f"{name} prepared {mode}", lambda: _wprep_call(h, O, L, lib, g, mode, wv, gw.region, xd, dyd, md))
            assert torch.equal(raw.view(torch.int32), prep.view(torch.int32)), f"{name} mode {mode}: prepared != unprepared"
        assert prepared, f"{name}: no prepared form for either mode"
    finally:
        O.set_precision("f32")


def test_conv_variants_contract(dev, monkeypatch, tmp_path):
    """Gated / gate-bit dgrads, the fused pool, and BatchNorm-on-load at `final`'s geometry."""
    from tg_hip import ops as O
    h = WsHarness(monkeypatch, dev)
    gen = torch.Generator().manual_seed(77)
    B, H, W, Cin, Cout = 2, 32, 48, 64, 64
    x = torch.randn(B, H, W, Cin, generator=gen)
    a = torch.relu(torch.randn(B, H, W, Cin, generator=gen))           # a ReLU output: the gate
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) / (3 * Cin ** 0.5)
    dy = torch.randn(B, H, W, Cout, generator=gen)
    xd, ad, dyd = x.to(dev), a.to(dev), dy.to(dev)
    wd = w.contiguous(memory_format=torch.channels_last).to(dev)
    bias = torch.zeros(Cout, device=dev)
    # pool: y and maxpool2(y) from one call
    y, yp = h.run("fwd_pool", lambda: O.conv_fwd(xd, wd, bias, 3, 1, 1, act=O.ACT_RELU, pool=True))
    ref = F.conv2d(_nchw(x).double(), w.double(), None, 1, 1).clamp_min(0)
    close(y, ref.permute(0, 2, 3, 1))
    close(yp, F.max_pool2d(ref, 2).permute(0, 2, 3, 1))
    # gated dgrad and its gate-bit form
    dxg, = h.run("dgrad_gated", lambda: (O.conv_dgrad(dyd, wd, (B, H, W, Cin), 3, 1, 1, gate=ad),))
    bits = O.relu_gate_pack(ad)
    dxb, = h.run("dgrad_gbits", lambda: (O.conv_dgrad(dyd, wd, (B, H, W, Cin), 3, 1, 1, gate_bits=bits),))
    assert torch.equal(dxg.view(torch.int32), dxb.view(torch.int32))
    xr = _nchw(torch.zeros(B, H, W, Cin)).double().requires_grad_(True)
    F.conv2d(xr, w.double(), None, 1, 1).backward(_nchw(dy).double())
    close(dxg, xr.grad.permute(0, 2, 3, 1) * (a > 0).double())
    # BatchNorm + ReLU on load, 64 -> 1 3x3 (`final` over dec1's output) at g72x40b3 and 16 x 16
    for (b_, h_, w_) in ((3, 72, 40), (1, 16, 16)):
        xb = torch.randn(b_, h_, w_, 64, generator=gen) * 1.5 + 0.3
        mean, rstd = xb.mean((0, 1, 2)), 1.0 / (xb.var((0, 1, 2), unbiased=False) + 1e-5).sqrt()
        gamma, beta = torch.rand(64, generator=gen) + 0.5, torch.randn(64, generator=gen) * 0.3
        w1 = torch.randn(1, 64, 3, 3, generator=gen) * 0.1
        dz = torch.randn(b_, h_, w_, 1, generator=gen)
        assert O.conv_bnin_supported((b_, h_, w_, 64), 1, 3, 1, 1) and O.conv_bnin_supported((b_, h_, w_, 64), 1, 3, 1, 1, wgrad=True)
        bn = tuple(t.to(dev) for t in (mean, rstd, gamma, beta)) + (O.ACT_RELU, 0.0)
        w1d, b1d = w1.contiguous(memory_format=torch.channels_last).to(dev), torch.full((1,), 0.25, device=dev)
        xbd, dzd = xb.to(dev), dz.to(dev)
        yb, = h.run(f"fwd_bnin {b_}x{h_}x{w_}", lambda: (O.conv_fwd_bnin(xbd, bn, w1d, b1d, 3, 1, 1),))
        dwb, dbb = h.run(f"wgrad_bnin {b_}x{h_}x{w_}", lambda: O.conv_wgrad(xbd, dzd, w1d, 3, 1, 1, in_bn=bn))
        act = ((xb.double() - mean.double()) * rstd.double() * gamma.double() + beta.double()).clamp_min(0)
        close(yb, F.conv2d(_nchw(act), w1.double(), torch.full((1,), 0.25, dtype=torch.float64), 1, 1).permute(0, 2, 3, 1))
        rdw = torch.nn.grad.conv2d_weight(_nchw(act), (1, 64, 3, 3), _nchw(dz).double(), stride=1, padding=1)
        close(dwb.permute(0, 2, 3, 1).contiguous(), rdw.permute(0, 2, 3, 1))
        close(dbb, dz.double().sum((0, 1, 2)))


# ---- BatchNorm and reductions -----------------------------------------------------------------------------------------------
BN_CASES = [(2, 3), (2, 64), (37, 3), (1001, 64), (4099, 1024), ((1 << 20) + 3, 3), ((1 << 20) + 5, 64)]


@pytest.mark.parametrize("rows,C", BN_CASES)
def test_bn_workspace_contract(dev, rows, C, monkeypatch):
    from tg_hip import ops as O
    h = WsHarness(monkeypatch, dev)
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(rows, C, generator=g) * 2 + 5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    gy = torch.randn(rows, C, generator=g)
    xd = x.reshape(1, 1, rows, C).contiguous().to(dev)
    gd, bd = gamma.to(dev), beta.to(dev)

    def stats():
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        mean, rstd = O.bn_stats(xd, rm, rv, torch.zeros((), dtype=torch.long, device=dev))
        return mean, rstd, rm, rv

    mean, rstd, rm, rv = h.run(f"bn_stats {rows}x{C}", stats)
    m2, r2, out = h.run(f"bn_fwd {rows}x{C}", lambda: O.bn_fwd(xd, gd, bd, O.ACT_RELU))
    xd64 = x.double()
    mu, var = xd64.mean(0), xd64.var(0, unbiased=False)
    for mm, rr in ((mean, rstd), (m2, r2)):
        close(mm, mu, rtol=1e-5, atol=1e-6)
        close(rr, 1 / (var + 1e-5).sqrt(), rtol=1e-5, atol=1e-6)
    close(rm, 0.1 * mu, rtol=1e-5, atol=1e-6)
    close(rv, 0.9 + 0.1 * xd64.var(0, unbiased=True), rtol=1e-5, atol=1e-6)
    xh = (xd64 - mu) / (var + 1e-5).sqrt()
    yref = (xh * gamma.double() + beta.double()).clamp_min(0)
    close(out.reshape(rows, C), yref)
    gyd = gy.reshape(1, 1, rows, C).contiguous().to(dev)
    dy, dgamma, dbeta, dbias = h.run(f"bn_act_bwd {rows}x{C}", lambda: O.bn_act_bwd(gyd, xd, mean, rstd, gd, bd, O.ACT_RELU,
                                                                                     inplace=False))
    gg = gy.double() * (out.reshape(rows, C).cpu() > 0)           # the ReLU gate the kernel saw (fp32 rounding decides ties)
    n = rows
    rdbeta, rdgamma = gg.sum(0), (gg * xh).sum(0)
    rdy = gamma.double() / (var + 1e-5).sqrt() * (gg - rdbeta / n - xh * rdgamma / n)
    close(dy.reshape(rows, C), rdy, rtol=2e-4, atol=1e-5)
    close(dgamma, rdgamma, rtol=2e-4, atol=1e-4)
    close(dbeta, rdbeta, rtol=2e-4, atol=1e-4)
    close(dbias, rdy.sum(0), rtol=1e-3, atol=2e-3 * math.sqrt(rows))


@pytest.mark.parametrize("rows_g,groups,C", [(7, 2, 4), (37, 3, 64), (4099, 2, 512), ((1 << 20) + 3, 2, 4)])
def test_bn_grouped_workspace_contract(dev, rows_g, groups, C, monkeypatch):
    from tg_hip import ops as O
    h = WsHarness(monkeypatch, dev)
    g = torch.Generator().manual_seed(rows_g * groups + C)
    x = torch.randn(groups * rows_g, C, generator=g) * 2 + 1
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    gy = torch.randn(groups * rows_g, C, generator=g)
    xd, gyd = x.reshape(groups, 1, rows_g, C).contiguous().to(dev), gy.reshape(groups, 1, rows_g, C).contiguous().to(dev)
    gd, bd = gamma.to(dev), beta.to(dev)
    mean, rstd, out = h.run("bn_fwd_grouped", lambda: O.bn_fwd_grouped(xd, groups, gd, bd, O.ACT_LEAKY, 0.2))
    dy, dgamma, dbeta, dbias = h.run("bn_act_bwd_grouped", lambda: O.bn_act_bwd_grouped(gyd.clone(), xd, groups, mean, rstd, gd, bd,
                                                                                          O.ACT_LEAKY, 0.2))
    xg, gyg = x.double().reshape(groups, rows_g, C), gy.double().reshape(groups, rows_g, C)
    mu, var = xg.mean(1, keepdim=True), xg.var(1, unbiased=False, keepdim=True)
    xh = (xg - mu) / (var + 1e-5).sqrt()
    z = xh * gamma.double() + beta.double()
    close(out.reshape(groups, rows_g, C), torch.where(z > 0, z, 0.2 * z))
    gg = gyg * torch.where(out.reshape(groups, rows_g, C).cpu() > 0, 1.0, 0.2)
    rdbeta, rdgamma = gg.sum(1, keepdim=True), (gg * xh).sum(1, keepdim=True)
    rdy = gamma.double() / (var + 1e-5).sqrt() * (gg - rdbeta / rows_g - xh * rdgamma / rows_g)
    close(dy.reshape(groups, rows_g, C), rdy, rtol=2e-4, atol=1e-5)
    close(dgamma, rdgamma.sum((0, 1)), rtol=2e-4, atol=1e-4)
    close(dbeta, rdbeta.sum((0, 1)), rtol=2e-4, atol=1e-4)
    close(dbias, rdy.sum((0, 1)), rtol=1e-3, atol=2e-3 * math.sqrt(groups * rows_g))


@pytest.mark.parametrize("shape", [(4, 64, 64, 64), (3, 72, 40, 64)])
def test_bn_bwd_conv1_workspace_contract(dev, shape, monkeypatch):
    from tg_hip import ops as O
    h = WsHarness(monkeypatch, dev)
    B, H, W, Cc = shape
    g = torch.Generator().manual_seed(sum(shape))
    y = (torch.randn(B, H, W, Cc, generator=g) * 1.5 + 0.3).to(dev)
    gamma, beta = (torch.rand(Cc, generator=g) + 0.5).to(dev), (torch.randn(Cc, generator=g) * 0.3).to(dev)
    ratio = (torch.rand(B, H, W, generator=g) * 2).to(dev)
    w = (torch.randn(1, Cc, 3, 3, generator=g) * 0.2).contiguous(memory_format=torch.channels_last).to(dev)
    dz = torch.randn(B, H, W, 1, generator=g).to(dev)
    assert O.bn_bwd_conv1_supported(tuple(y.shape))
    mean, rstd = O.bn_stats(y)
    dy1, dg1, db1, dbias1 = h.run("bn_act_bwd_conv1", lambda: O.bn_act_bwd_conv1(dz, w, y, mean, rstd, gamma, beta, O.ACT_RELU,
                                                                                  ratio=ratio))
    # fp64 reference and bounds of tests/test_hip_ops.py::test_bn_backward_over_a_recomputed_1channel_dgrad
    yd, m64, r64 = y.double().cpu(), mean.double().cpu(), rstd.double().cpu()
    dad = F.conv_transpose2d(_nchw(dz.double().cpu()), w.double().cpu(), None, 1, 1).permute(0, 2, 3, 1)
    xh = (yd - m64) * r64
    gg = dad * ((xh * gamma.double().cpu() + beta.double().cpu()) > 0)
    n = B * H * W
    dbeta, dgamma = gg.sum((0, 1, 2)), (gg * xh).sum((0, 1, 2))
    dyr = gamma.double().cpu() * r64 * (gg - dbeta / n - xh * dgamma / n) * ratio.double().cpu()[..., None]
    close(dy1, dyr, rtol=1e-4, atol=1e-5 * float(dyr.abs().max()))
    close(dg1, dgamma, rtol=1e-4, atol=1e-5 * float(dgamma.abs().max()))
    close(db1, dbeta, rtol=1e-4, atol=1e-5 * float(dbeta.abs().max()))
    close(dbias1, dyr.sum((0, 1, 2)), rtol=1e-4, atol=2e-5 * float(dyr.abs().sum((0, 1, 2)).max()))


@pytest.mark.parametrize("n", [1, 3, 1001, (1 << 20) + 7, 3 << 20])
def test_reductions_workspace_contract(dev, n, monkeypatch):
    from tg_hip import ops as O
    h = WsHarness(monkeypatch, dev)
    g = torch.Generator().manual_seed(n)
    a, b, z = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g) * 4
    ad, bd, zd = a.to(dev), b.to(dev), z.to(dev)
    l1, da = h.run(f"l1_mean {n}", lambda: O.l1_mean(ad, bd))
    close(l1[0], (a.double() - b.double()).abs().mean(), rtol=1e-5, atol=1e-7)
    close(da, torch.sign(a.double() - b.double()) / n, rtol=1e-4, atol=1e-9)
    for t in (0.0, 1.0):
        lo, dz = h.run(f"bce {n} {t}", lambda: O.bce_logits(zd, t))
        zz = z.double().requires_grad_(True)
        loss = F.binary_cross_entropy_with_logits(zz, torch.full_like(zz, t))
        loss.backward()
        close(lo[0], loss.detach(), rtol=1e-5, atol=1e-7)
        close(dz, zz.grad, rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("shape", [(1, 2, 3), (1, 5, 7), (3, 72, 40), (2, 257, 129), (17, 256, 256)])
def test_pixel_losses_workspace_contract(dev, shape, monkeypatch):
    from oracle import terragan_oracle as Orc
    from tg_hip import ops as O
    h = WsHarness(monkeypatch, dev)
    B, H, W = shape
    g = torch.Generator().manual_seed(B * H * W)
    pred = torch.rand(B, 1, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    tgt = torch.rand(B, 1, H, W, generator=g, dtype=torch.float64)
    m = (torch.rand(B, 1, H, W, generator=g) > 0.4).double()
    tot = (pred - tgt).abs().mean() + 0.1 * Orc.tv_loss(pred * (1 - m)) + 0.5 * Orc.boundary_loss(pred, tgt, m)
    tot.backward()
    pd, td, mdv = (t.detach()[:, 0].float().contiguous().to(dev) for t in (pred, tgt, m))
    out5, dp = h.run(f"pixel_losses {shape}", lambda: O.pixel_losses(pd, td, mdv, 1.0, 0.1, 0.5))
    close(out5[4], tot.detach(), rtol=1e-5, atol=1e-7)
    close(dp, pred.grad[:, 0], rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("imgs,H,W", [(1, 16, 16), (3, 72, 40), (5, 33, 47), (16, 256, 256)])
def test_quality_metrics_workspace_contract(dev, imgs, H, W, monkeypatch):
    from tg_hip import ops as O
    h = WsHarness(monkeypatch, dev)
    g = torch.Generator().manual_seed(imgs * H + W)
    p_, t_ = torch.rand(imgs, 1, H, W, generator=g), torch.rand(imgs, 1, H, W, generator=g)
    m_ = (torch.rand(imgs, 1, H, W, generator=g) > 0.5).float()
    out, = h.run(f"quality_metrics {imgs}x{H}x{W}", lambda: (O.quality_metrics(p_.to(dev), t_.to(dev), m_.to(dev)),))
    p, t = p_.double(), t_.double()
    mse = ((p - t) ** 2).mean()
    mu_p, mu_t = F.avg_pool2d(p, 11, 1, 5), F.avg_pool2d(t, 11, 1, 5)
    s_pp = F.avg_pool2d(p * p, 11, 1, 5) - mu_p ** 2
    s_tt = F.avg_pool2d(t * t, 11, 1, 5) - mu_t ** 2
    s_pt = F.avg_pool2d(p * t, 11, 1, 5) - mu_p * mu_t
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ssim = (((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p ** 2 + mu_t ** 2 + c1) * (s_pp + s_tt + c2))).mean()
    ref = torch.stack([mse, 20 * torch.log10(1 / mse.sqrt()), ssim, (p - t).abs().mean(), mse.sqrt()])
    close(out[:5], ref, rtol=1e-4, atol=1e-6)
