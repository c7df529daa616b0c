"""Activation checkpointing of the perceptual loss's frozen VGG trunk: ReLU gates packed into bits (tg_relu_gate_pack), dgrads
gated by those bits (tg_conv_dgrad_gbits) bit-identical to the fp32-gated ones on every route, vgg_forward(keep="gates") /
vgg_backward bit-identical to keep=True at a small fraction of the retained bytes, and the config-5 train step's peak."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture
def f32_after():
    from tg_hip import ops as O
    yield O
    O.set_precision("f32")


def _np_pack(a, nb):
    """numpy reference of relu_gate_pack: uint32 [nb][H][W][C/32], bit c % 32 of word c / 32 = a > 0."""
    x = a[:nb].cpu().numpy()
    bits = (x > 0).astype(np.uint64).reshape(*x.shape[:-1], x.shape[-1] // 32, 32)
    return (bits << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def _u32(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _specials(a, g):
    """Scatter -0.0, +0.0, NaN, +-inf and +-denormals over a."""
    flat = a.view(-1)
    vals = torch.tensor([-0.0, 0.0, float("nan"), float("inf"), -float("inf"), 1e-40, -1e-40, 1.4e-45, -1.4e-45],
                        dtype=torch.float32)
    idx = torch.randint(0, flat.numel(), (max(9, flat.numel() // 16),), generator=g)
    flat[idx] = vals[torch.arange(idx.numel()) % vals.numel()].to(a.device)
    return a


@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_relu_gate_pack_matches_numpy(dev, C):
    from tg_hip import ops as O
    g = torch.Generator().manual_seed(C)
    for B, H, W, nb in ((3, 5, 7, 2), (1, 9, 3, 1), (4, 17, 33, 4)):
        a = torch.randn(B, H, W, C, generator=g).to(dev)
        a = _specials(a, g)
        bits = O.relu_gate_pack(a, nb)
        assert bits.dtype == torch.uint32 and tuple(bits.shape) == (nb, H, W, C // 32)
        assert np.array_equal(_u32(bits), _np_pack(a, nb))


def _gated_pair(dev, O, B, S, cin, cout, wino4, seed, specials=False):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev)
    w = O.weight_view(w.contiguous(memory_format=torch.channels_last)).permute(0, 3, 1, 2)
    dy = torch.randn(B, S, S, cout, generator=g).to(dev)
    gate = torch.randn(B, S, S, cin, generator=g).clamp_min(0.0).to(dev)      # a ReLU output: about half exact zeros
    if specials:
        gate = _specials(gate, g)
    ref = O.conv_dgrad(dy, w, (B, S, S, cin), 3, 1, 1, gate=gate, gate_act=O.ACT_RELU, wino4=wino4)
    got = O.conv_dgrad(dy, w, (B, S, S, cin), 3, 1, 1, gate_bits=O.relu_gate_pack(gate), wino4=wino4)
    return ref, got


# the four gated dgrads of the trunk: input channels of conv 2 / 7 / 12 / 14 at 1x, 1/2x, 1/4x, 1/4x of the image
TRUNK_GATED = [(64, 1), (128, 2), (256, 4), (256, 4)]


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("wino4", [True, False])
def test_bit_gated_dgrad_equals_fp32_gated(dev, f32_after, prec, wino4):
    O = f32_after
    O.set_precision(prec)
    for size in (64, 256, 512):
        for B in (1, 3):
            for li, (ch, div) in enumerate(TRUNK_GATED):
                ref, got = _gated_pair(dev, O, B, size // div, ch, ch, wino4, 1000 * li + size + B, specials=li == 0)
                assert torch.equal(ref, got), (prec, wino4, size, B, li)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_bit_gated_dgrad_split_k_and_small_routes(dev, f32_after, prec):
    """256 contraction channels over few work items (one 32x32 image): the Winograd planner splits K (gated is off in the kernel,
    the bits go through gate_bits_apply after the split-K epilogue); 8 contraction channels: one K step, the non-pipelined kernel;
    32 channels: the smallest gate word."""
    O = f32_after
    O.set_precision(prec)
    for B, S, cin, cout in ((1, 32, 256, 256), (1, 16, 256, 256), (2, 40, 64, 8), (2, 24, 32, 32), (1, 20, 96, 64)):
        ref, got = _gated_pair(dev, O, B, S, cin, cout, False, S * cin + cout)
        assert torch.equal(ref, got), (prec, B, S, cin, cout)


_NO_WINO_CHILD = r"""
import sys, torch
sys.path[:0] = [{root!r}, {pkg!r}]
from tests.test_hip_vgg_gates import _gated_pair
from tg_hip import ops as O
dev = torch.device("cuda:0")
for prec in ("f32", "bf16"):
    O.set_precision(prec)
    for B, S, ch in ((1, 64, 64), (3, 32, 128), (2, 16, 256), (1, 17, 32)):
        ref, got = _gated_pair(dev, O, B, S, ch, ch, False, S + ch)
        assert torch.equal(ref, got), (prec, B, S, ch)
print("NO_WINO_OK")
"""


def test_bit_gated_dgrad_without_winograd(dev):
    """TG_NO_WINO=1 (read once per process): the implicit-GEMM route runs ungated and gate_bits_apply follows -- in a child."""
    env = dict(os.environ, TG_NO_WINO="1")
    code = _NO_WINO_CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "terra-gan_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "NO_WINO_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _trunk(dev, O, family):
    from oracle import terragan_oracle as Orc
    if family == "standin":
        sd = Orc.init_vgg_standin()
    else:
        from tests.vgg_like import trained_like_state
        sd = trained_like_state()
    V = {k: v.to(dev) for k, v in sd.items()}
    for k in list(V):
        if k.endswith(".weight"):
            V[k] = O.weight_view(V[k].contiguous(memory_format=torch.channels_last)).permute(0, 3, 1, 2)
    V["0.folded"] = O.fold_cin(V["0.weight"])
    return V


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("family", ["standin", "trained_like"])
def test_trunk_backward_from_gates_equals_keep(dev, f32_after, prec, family):
    from oracle import terragan_oracle as Orc
    from tg_hip import engine as E
    O = f32_after
    O.set_precision(prec)
    V = _trunk(dev, O, family)
    for size, B in ((128, 3), (512, 2)):
        real, mask = Orc.synth_batch(B, size, 7 + size)
        noise = torch.rand(real.shape, generator=torch.Generator().manual_seed(8 + size))
        pred = real * mask + (real + 0.3 * (noise - real)) * (1 - mask)
        both = torch.cat([pred, real]).reshape(2 * B, size, size).to(dev).contiguous()
        res = {}
        for keep in (True, "gates"):
            feats, ctx = E.vgg_forward(V, both, keep=keep, nb=B)
            _perc, dfeat = O.l1_mean(feats[:B], feats[B:], 0.1, relu_gate=True)
            res[keep] = (feats.clone(), E.vgg_backward(ctx, dfeat, nb=B, gated=True))
            del ctx
        assert torch.equal(res[True][0], res["gates"][0]), (family, prec, size)
        assert torch.equal(res[True][1], res["gates"][1]), (family, prec, size)


def _ctx_bytes(ctx, codes):
    seen, total = set(), 0
    for st in ctx.steps:
        for name in ("a", "x", "bits") + (("code",) if codes else ()):
            t = getattr(st, name, None)
            if t is None:
                continue
            s = t.untyped_storage()
            if s.data_ptr() not in seen:
                seen.add(s.data_ptr())
                total += s.nbytes()
    return total


def test_gates_context_retains_a_fraction(dev):
    """256^2, B = 4 (forward over 8 images): the "gates" context holds the bits of the pred half (~4.2 MB) where keep=True holds
    ~302 MB of fp32 activations (features[15] included); storage bytes, so a [:nb] view would count its whole buffer."""
    from oracle import terragan_oracle as Orc
    from tg_hip import engine as E
    from tg_hip import ops as O
    V = _trunk(dev, O, "standin")
    B, size = 4, 256
    real, mask = Orc.synth_batch(B, size, 5)
    both = torch.cat([real * mask, real]).reshape(2 * B, size, size).to(dev).contiguous()
    _f1, ck = E.vgg_forward(V, both, keep=True)
    _f2, cg = E.vgg_forward(V, both, keep="gates", nb=B)
    keep_nc, gates_nc = _ctx_bytes(ck, codes=False), _ctx_bytes(cg, codes=False)
    keep_all, gates_all = _ctx_bytes(ck, codes=True), _ctx_bytes(cg, codes=True)
    print(f"\nretained by the VGG context at 256^2 x 8 images: keep=True {keep_nc / 1e6:.1f} MB (+ codes {keep_all / 1e6:.1f}), "
          f"gates {gates_nc / 1e6:.2f} MB (+ codes {gates_all / 1e6:.2f})")
    assert gates_nc * 48 <= keep_nc, (gates_nc, keep_nc)
    assert gates_all * 12 <= keep_all, (gates_all, keep_all)
    assert not any(getattr(st, "a", None) is not None for st in cg.steps)


def _build(dev, seed=0):
    from mvp_gan.src.models import Discriminator, PConvUNet
    from mvp_gan.src.utils.losses import InpaintingLoss
    torch.manual_seed(seed)
    G, D = PConvUNet(), Discriminator()
    crit = InpaintingLoss(0.1, 0.1, device=torch.device("cpu"))
    G, D, crit = G.to(dev), D.to(dev), crit.to(dev)
    return G, D, crit, torch.optim.Adam(G.parameters(), lr=2e-4), torch.optim.Adam(D.parameters(), lr=2e-4)


def test_config5_checkpointing_covers_the_trunk(dev):
    """1024^2, B = 4, two steps: the checkpointed step (generator checkpointing + the trunk kept as bit gates) is bit-identical
    to the plain one and its peak sits at least 3 GiB below the plain step's."""
    from mvp_gan.src.train import train_step
    from oracle import terragan_oracle as Orc
    real, mask = Orc.synth_batch(4, 1024, 3001)
    real, mask = real.to(dev), mask.to(dev)
    res = {}
    for name, ck in (("plain", False), ("ckpt", True)):
        G, D, crit, oG, oD = _build(dev)
        G.activation_checkpointing = ck
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        for _s in range(2):
            out = train_step(G, D, crit, oG, oD, real, mask)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        res[name] = ([p_.detach().clone() for p_ in list(G.parameters()) + list(D.parameters())], out["gen"].clone(),
                     float(out["g_total"]), float(out["d_loss"]), peak)
        del G, D, crit, oG, oD, out
    assert res["plain"][2:4] == res["ckpt"][2:4]
    assert torch.equal(res["plain"][1], res["ckpt"][1])
    for a, b in zip(res["plain"][0], res["ckpt"][0]):
        assert torch.equal(a, b)
    print(f"\nconfig 5 peak HBM over the step: plain {res['plain'][4] / 2**30:.2f} GiB, checkpointed {res['ckpt'][4] / 2**30:.2f} GiB")
    assert res["ckpt"][4] <= res["plain"][4] - (3 << 30), (res["plain"][4], res["ckpt"][4])


def test_human_guided_step_checkpointed_is_exact(dev):
    from mvp_gan.src.models import PConvUNet
    from mvp_gan.src.training.human_guided_trainer import human_guided_step
    from mvp_gan.src.utils.losses import HumanGuidedLoss
    from oracle import terragan_oracle as Orc
    cfg = {"training": {"loss_weights": {"boundary": 0.5},
                        "modes": {"human_guided": {"human_feedback_weight": 0.3, "base_loss_weight": 0.7,
                                                   "learning_rate": 1e-4, "batch_size": 2}}}}
    real, mask = Orc.synth_batch(2, 256, 41)
    _, human = Orc.synth_batch(2, 256, 42)
    human = (1 - human) * 255.0
    res = []
    for ck in (False, True):
        torch.manual_seed(0)
        G = PConvUNet()
        crit = HumanGuidedLoss(cfg, device=torch.device("cpu"))
        G, crit = G.to(dev), crit.to(dev)
        G.activation_checkpointing = ck
        opt = torch.optim.Adam(G.parameters(), lr=1e-4)
        loss, gen = human_guided_step(G, crit, opt, real.to(dev), mask.to(dev), human.to(dev))
        res.append((float(loss), gen.clone(), [p_.detach().clone() for p_ in G.parameters()]))
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1])
    for a, b in zip(res[0][2], res[1][2]):
        assert torch.equal(a, b)
