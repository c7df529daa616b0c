"""The wide form of the F(2x2,2x2) kernel (csrc/wino22.inc, wino22w_kernel: 64 tiles x 128 channels per work item) beside the
narrow one (wino22_kernel), both run in this process through TG_WINO22_WIDE, which the library reads at every launch.

Every case asserts, for the forward of a 4x4 / stride-2 / pad-1 convolution or for its four-class input gradient:
  (a) the wide form's output is torch.equal to the narrow form's (same K order, same MFMA chain per point, same output transform);
  (b) small-integer inputs and weights give the exact integer result (every intermediate is an fp32 integer);
  (c) random data stays inside the bound tests/test_hip_wino.py uses for this kernel family, against fp64 conv2d;
  (d) the launch record names the form launch_wino22's rule predicts: wide only with N % 128 == 0, one split and at least
      WINO_PLAN_CUS widened items -- the three fallbacks (N = 64, too few items, a split-K plan) included.
Shapes: the smallest at which the wide form can go wrong -- 8 and 16 input channels (a parity-phase change inside an item), one
and two 128-channel N tiles, one item per image (32x32), 294 items on 256 workgroups (6 x 224x224: some walk two items, the
hand-over included) and an odd-edged 72x72 (Ho = 36 clips tiles at the right and bottom edges)."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests.test_hip_direct_conv import Routes, dev  # noqa: F401

pytestmark = pytest.mark.gpu

PLAN_CUS = 256                          # WINO_PLAN_CUS (csrc/igemm.hip)
FAST, QUEUED, WIDE = 2, 4, 8            # WinoRoute (csrc/igemm_params.h): cfg 4022 = 1 + these + gate


def choose_splits(tiles, max_splits, slots=PLAN_CUS):
    """csrc/igemm.hip: choose_splits."""
    if tiles >= 4 * slots:
        return 1
    best, best_eff = 1, 0.0
    for sp in range(1, max(max_splits, 1) + 1):
        blocks = tiles * sp
        rounds = -(-blocks // slots)
        eff = blocks / (rounds * slots)
        if eff > best_eff + 1e-9:
            best_eff, best = eff, sp
        if blocks >= slots and eff >= 0.92:
            return sp
        if blocks >= 6 * slots:
            break
    return best


def plan(B, Ho, Wo, N, K, ncls):
    """launch_wino22's rule: (narrow items, splits, wide?) for N output channels and a contraction of K."""
    items = B * -(-Ho // 16) * -(-Wo // 16) * (N // 64) * ncls
    nchunks, splits = K // 8, 1
    if nchunks >= 16:
        splits = choose_splits(items, min(nchunks // 8, 16))
    per = -(-nchunks // splits)
    splits = -(-nchunks // per)
    return items, splits, N % 128 == 0 and splits == 1 and items // 2 >= PLAN_CUS


def both_forms(run, csv_path, want_wide, gate=False, queued=False):
    """run() under the default switch and with the wide form off: (default output, narrow output); asserts the records."""
    base = 1 + (QUEUED if queued else 0) + FAST + (1 if gate else 0)
    out = []
    for off in (False, True):
        try:
            if off:
                os.environ["TG_WINO22_WIDE"] = "0"
            with Routes(csv_path) as rt:
                y = run()
        finally:
            os.environ.pop("TG_WINO22_WIDE", None)
        rows = [r for r in rt.rows if r[1] == 4022]
        want = base + (WIDE if want_wide and not off else 0)
        assert rows == [(0, 4022, want)], f"launch records {rt.rows}: expected one 4022 launch on route {want}"
        out.append((y, rt.splits[rt.rows.index(rows[0])]))
    return out[0][0], out[1][0], out[0][1]


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# B, H, W, Cin, Cout: the forward reads Cin (K = 4 Cin) and writes Cout; the dgrad cases mirror them
SHAPES = [(256, 32, 32, 8, 128), (256, 32, 32, 16, 128), (128, 32, 32, 8, 256), (128, 32, 32, 16, 256),
          (6, 224, 224, 8, 128), (6, 224, 224, 16, 128), (6, 224, 224, 8, 256), (6, 224, 224, 16, 256),
          (29, 72, 72, 8, 128)]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_wide_forward(dev, case, tmp_path):
    from tg_hip import ops as O
    B, H, W, Cin, Cout = case
    Ho, Wo = H // 2, W // 2
    items, splits, wide = plan(B, Ho, Wo, Cout, 4 * Cin, 1)
    assert wide and splits == 1 and items // 2 >= PLAN_CUS, "the case is meant to take the wide form"
    csv = tmp_path / "launches.csv"
    g = torch.Generator().manual_seed(sum(case))
    # (b) integers: exact, with a bias
    x, w, bias = ints(g, (B, H, W, Cin), -3, 3), ints(g, (Cout, Cin, 4, 4), -2, 2), ints(g, (Cout,), -4, 4)
    wd = w.contiguous(memory_format=torch.channels_last).to(dev)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), bias.double(), 2, 1).permute(0, 2, 3, 1).contiguous().to(dev)
    yw, yn, _ = both_forms(lambda: O.conv_fwd(x.to(dev), wd, bias.to(dev), 4, 2, 1), csv, True)
    assert torch.equal(yw, yn), "integer data: the wide form differs from the narrow one"
    assert torch.equal(yw.double(), ref), "integer data: not the exact result"
    # (c) random data: plain, then bias + row scale + LeakyReLU; (a) on both
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, 4, 4, generator=g) / (4 * Cin ** 0.5)
    bias = torch.randn(Cout, generator=g) * 0.1
    ratio = torch.rand(B, Ho, Wo, generator=g) * 0.75 + 0.25
    wd = w.contiguous(memory_format=torch.channels_last).to(dev)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), None, 2, 1).permute(0, 2, 3, 1).contiguous().to(dev)
    tol = 2e-6 * max(1.0, ref.abs().max().item()) * (Cin / 16) ** 0.5 + 3e-6
    yw, yn, _ = both_forms(lambda: O.conv_fwd(x.to(dev), wd, None, 4, 2, 1), csv, True)
    assert torch.equal(yw, yn), "the wide form differs from the narrow one"
    err = (yw.double() - ref).abs().max().item()
    print(f"WIDE_FWD {case} plain err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (case, err, tol)
    refe = (ref + bias.double().to(dev)) * ratio[..., None].double().to(dev)
    refe = torch.where(refe > 0, refe, 0.2 * refe)
    yw, yn, _ = both_forms(lambda: O.conv_fwd(x.to(dev), wd, bias.to(dev), 4, 2, 1, ratio=ratio.to(dev), act=O.ACT_LEAKY, slope=0.2),
                           csv, True)
    assert torch.equal(yw, yn), "bias + row scale + LeakyReLU: the wide form differs from the narrow one"
    err = (yw.double() - refe).abs().max().item()
    print(f"WIDE_FWD {case} epilogue err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (case, err, tol)


# the mirror images: B, H, W (of dx), Cout (K of the dgrad), Cin (its output channels); four classes per patch
DGRAD_SHAPES = [(64, 32, 32, 8, 128), (64, 32, 32, 16, 128), (32, 32, 32, 8, 256), (32, 32, 32, 16, 256),
                (6, 224, 224, 8, 128), (6, 224, 224, 16, 128), (6, 224, 224, 8, 256), (6, 224, 224, 16, 256),
                (8, 72, 72, 8, 128)]


@pytest.mark.parametrize("case", DGRAD_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_wide_dgrad(dev, case, tmp_path):
    from tg_hip import ops as O
    B, H, W, Cout, Cin = case
    Ho, Wo = H // 2, W // 2
    items, splits, wide = plan(B, Ho, Wo, Cin, Cout, 4)
    assert wide and splits == 1 and items // 2 >= PLAN_CUS, "the case is meant to take the wide form"
    csv = tmp_path / "launches.csv"
    g = torch.Generator().manual_seed(sum(case) + 1)
    gd = torch.Generator(device=dev).manual_seed(sum(case) + 2)
    shape = (B, H, W, Cin)

    def ref_of(dy, w):          # fp64 on the host (small operands), compared on the device (dx is the large tensor)
        return F.conv_transpose2d(dy.permute(0, 3, 1, 2).double(), w.double(), None, 2, 1).permute(0, 2, 3, 1).contiguous().to(dev)

    # (b) integers: exact, plain and behind a ReLU gate (multipliers 0 / 1)
    dy, w = ints(g, (B, Ho, Wo, Cout), -3, 3), ints(g, (Cout, Cin, 4, 4), -2, 2)
    xact = torch.randn(shape, generator=gd, device=dev)
    wd = w.contiguous(memory_format=torch.channels_last).to(dev)
    ref = ref_of(dy, w)
    yw, yn, _ = both_forms(lambda: O.conv_dgrad(dy.to(dev), wd, shape, 4, 2, 1), csv, True)
    assert torch.equal(yw, yn), "integer data: the wide form differs from the narrow one"
    assert torch.equal(yw.double(), ref), "integer data: not the exact result"
    yw, yn, _ = both_forms(lambda: O.conv_dgrad(dy.to(dev), wd, shape, 4, 2, 1, gate=xact, gate_act=O.ACT_RELU), csv, True, gate=True)
    assert torch.equal(yw, yn), "integer data, gated: the wide form differs from the narrow one"
    assert torch.equal(yw.double(), ref * (xact > 0).double()), "integer data, gated: not the exact result"
    # (c) random data: plain, LeakyReLU gate, mask (row scale) + accumulate; (a) on each
    dy = torch.randn(B, Ho, Wo, Cout, generator=g)
    w = torch.randn(Cout, Cin, 4, 4, generator=g) / (4 * Cout ** 0.5)
    mask = (torch.rand((B, H, W), generator=gd, device=dev) > 0.3).float()
    base = torch.randn(shape, generator=gd, device=dev)
    wd = w.contiguous(memory_format=torch.channels_last).to(dev)
    ref = ref_of(dy, w)
    tol = 2e-6 * max(1.0, ref.abs().max().item()) * (Cout / 16) ** 0.5 + 3e-6
    yw, yn, _ = both_forms(lambda: O.conv_dgrad(dy.to(dev), wd, shape, 4, 2, 1), csv, True)
    assert torch.equal(yw, yn), "the wide form differs from the narrow one"
    err = (yw.double() - ref).abs().max().item()
    print(f"WIDE_DGRAD {case} plain err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (case, err, tol)
    yw, yn, _ = both_forms(lambda: O.conv_dgrad(dy.to(dev), wd, shape, 4, 2, 1, gate=xact, gate_act=O.ACT_LEAKY, gate_slope=0.2), csv, True,
                           gate=True)
    assert torch.equal(yw, yn), "gated: the wide form differs from the narrow one"
    err = (yw.double() - ref * torch.where(xact > 0, 1.0, 0.2).double()).abs().max().item()
    print(f"WIDE_DGRAD {case} gated err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (case, err, tol)
    yw, yn, _ = both_forms(lambda: O.conv_dgrad(dy.to(dev), wd, shape, 4, 2, 1, in_mask=mask, out=base.clone()), csv, True)
    assert torch.equal(yw, yn), "mask + accumulate: the wide form differs from the narrow one"
    err = (yw.double() - (base.double() + ref * mask[..., None].double())).abs().max().item()
    print(f"WIDE_DGRAD {case} mask+acc err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (case, err, tol)


def test_wide_with_a_work_stealing_queue(dev, tmp_path):
    """The queue twins (tg_set_work_stealing): 294 forward items and 1176 gated dgrad items pulled by 256 workgroups."""
    from tg_hip import lib as L
    from tg_hip import ops as O
    lib = L.load()
    B, H, W, Cin, Cout = 6, 224, 224, 8, 128
    g = torch.Generator().manual_seed(7)
    x, w, bias = ints(g, (B, H, W, Cin), -3, 3), ints(g, (Cout, Cin, 4, 4), -2, 2), ints(g, (Cout,), -4, 4)
    wd = w.contiguous(memory_format=torch.channels_last).to(dev)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), bias.double(), 2, 1).permute(0, 2, 3, 1)
    dy, w2 = ints(g, (B, H // 2, W // 2, Cin), -3, 3), ints(g, (Cin, Cout, 4, 4), -2, 2)
    xact = torch.randn(B, H, W, Cout, generator=g)
    wd2 = w2.contiguous(memory_format=torch.channels_last).to(dev)
    refd = F.conv_transpose2d(dy.permute(0, 3, 1, 2).double(), w2.double(), None, 2, 1).permute(0, 2, 3, 1) * (xact > 0).double()
    try:
        L.check(lib.tg_set_work_stealing(2), "tg_set_work_stealing")
        yw, yn, _ = both_forms(lambda: O.conv_fwd(x.to(dev), wd, bias.to(dev), 4, 2, 1), tmp_path / "l.csv", True, queued=True)
        dw, dn, _ = both_forms(lambda: O.conv_dgrad(dy.to(dev), wd2, (B, H, W, Cout), 4, 2, 1, gate=xact.to(dev), gate_act=O.ACT_RELU),
                               tmp_path / "l.csv", True, gate=True, queued=True)
        torch.cuda.synchronize()
    finally:
        L.check(lib.tg_set_work_stealing(0), "tg_set_work_stealing")
    assert torch.equal(yw, yn) and torch.equal(yw.cpu().double(), ref)
    assert torch.equal(dw, dn) and torch.equal(dw.cpu().double(), refd)


# the three fallbacks of the rule, forward: B, H, W, Cin, Cout, why
FALLBACKS = [(6, 224, 224, 8, 64, "N = 64"), (2, 32, 32, 8, 128, "too few items"), (270, 32, 32, 48, 128, "a split-K plan")]


@pytest.mark.parametrize("case", FALLBACKS, ids=lambda c: c[5].replace(" ", "_"))
def test_narrow_where_the_rule_says_so(dev, case, tmp_path):
    from tg_hip import ops as O
    B, H, W, Cin, Cout, why = case
    items, splits, wide = plan(B, H // 2, W // 2, Cout, 4 * Cin, 1)
    assert not wide
    if why == "N = 64":
        assert Cout % 128 and splits == 1 and items >= PLAN_CUS
    elif why == "too few items":
        assert Cout % 128 == 0 and splits == 1 and items // 2 < PLAN_CUS
    else:
        assert Cout % 128 == 0 and splits > 1 and items // 2 >= PLAN_CUS
    g = torch.Generator().manual_seed(sum(case[:5]))
    x, w = ints(g, (B, H, W, Cin), -3, 3), ints(g, (Cout, Cin, 4, 4), -2, 2)
    wd = w.contiguous(memory_format=torch.channels_last).to(dev)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), None, 2, 1).permute(0, 2, 3, 1)
    y, yn, got_splits = both_forms(lambda: O.conv_fwd(x.to(dev), wd, None, 4, 2, 1), tmp_path / "launches.csv", False)
    assert got_splits == splits, (got_splits, splits)
    assert torch.equal(y, yn) and torch.equal(y.cpu().double(), ref), why
