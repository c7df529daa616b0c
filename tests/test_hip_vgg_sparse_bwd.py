"""The sparse backward of the frozen VGG trunk: tg_conv_dgrad_sparse / tg_maxpool2_bwd_code_sparse produce the dense
launches' bits on every needed pixel and write nothing else, the 1-channel dgrad zeroes what nobody needs, whole trunk backwards
and train steps equal the dense ones bit for bit -- with fractional masks, eager and graphed -- and module autograd stays dense."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_hip_vgg_sparse import _build, _pair, _read_map, _same, _state, _two_steps, _weights, dev  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = ["blobs", "corners", "signed_zero", "empty", "full"]
# (nb, H, W, Cin, Cout) of the conv whose dgrad runs: the layer shapes of test_sparse_launch_equals_dense and the partial-tile
# sizes
SHAPES = [(2, 64, 64, 64, 64), (1, 48, 80, 64, 128), (2, 32, 32, 256, 256), (2, 33, 47, 64, 64), (2, 18, 34, 64, 64)]
# ... and the 256 x 256 blobs case, whose map share shows that tiles are both skipped and computed, and a 128-channel layer
# with enough work items for one K split
CASES = [(k,) + s for s in SHAPES for k in KINDS] + [("blobs", 2, 256, 256, 64, 64), ("blobs", 2, 128, 128, 128, 128)]


def _expect_list_walk(nb, H, W, Cin, Cout):
    """Which launches must honour the tile list: the pipelined kernel in ONE K split -- 64 contraction channels are 8 K steps (no
    split below 16), and the 128-channel case has 2 x 64 x 2 = 256 work items, which fill the chip without a split.  The small
    64 -> 128 and 256 -> 256 shapes split K and fall back to the dense launch."""
    return Cout == 64 or (nb, H, W, Cin, Cout) == (2, 128, 128, 128, 128)


def _dil(d, n=1):
    """bool [nb][H][W] dilated by n pixels: what n 3x3 convs spread a pixel set to."""
    x = d.float().unsqueeze(1)
    for _ in range(n):
        x = F.max_pool2d(x, 3, 1, 1)
    return x[:, 0] > 0


def _tiles_to_pixels(flags, H, W):
    """bool [nb][ty][tx] -> bool [nb][H][W]."""
    return flags.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W]


def _needed_pair(nb, H, W, seed, kind):
    """(pred, target, mask, needed): needed = the patterns differ or mask != 1; the mask opens a few pixels where they agree."""
    p, t = _pair(nb, H, W, seed, kind)
    m = (p.view(torch.int32) == t.view(torch.int32)).float()
    if kind in ("blobs", "corners"):
        m[:, H // 3, W // 2] = 0.5
        m[:, H - 1, 0] = 1.0 - 2.0 ** -24
    needed = (p.view(torch.int32) != t.view(torch.int32)) | (m != 1)
    return p, t, m, needed


def _map(dev, p, t, m, plan="C"):
    from tg_hip import ops as O
    x = torch.cat([p, t]).to(dev).contiguous()
    sm = O.vgg_sparse_map(x, p.shape[0], plan, mask=m.to(dev).contiguous())
    assert sm is not None and sm.for_bwd
    return sm


@pytest.mark.parametrize("gate", ["plain", "gate", "gate_bits"])
@pytest.mark.parametrize("kind,nb,H,W,Cin,Cout", CASES)
def test_sparse_dgrad_equals_dense_on_needed_pixels(dev, kind, gate, nb, H, W, Cin, Cout):
    from tg_hip import ops as O
    p, t, m, needed = _needed_pair(nb, H, W, 11 + H, kind)
    sm = _map(dev, p, t, m)
    flags, cnt, _ = _read_map(sm, 0)
    flags = torch.from_numpy(flags)
    # the map covers one dilation of the needed pixels: exactly the pixels of this dgrad's output somebody reads
    need1 = _dil(needed, 1)
    assert torch.equal(flags, F.max_pool2d(F.pad(need1.float().unsqueeze(1), (0, -W % 16, 0, -H % 16)), 16, 16)[:, 0] > 0)
    share = flags.float().mean().item()
    if (H, W) == (256, 256):
        assert 0.05 < share < 0.95, share               # the case that shows tiles are skipped AND computed
    if kind == "empty":
        assert cnt == 0
    if kind == "full":
        assert share == 1.0
    g = torch.Generator().manual_seed(3 + H + Cin)
    dy = torch.randn(nb, H, W, Cout, generator=g)
    w, _b = _weights(Cout, Cin, 7 + Cout, dev)
    kw = {}
    if gate != "plain":
        a = torch.relu(torch.randn(nb, H, W, Cin, generator=g)).to(dev)
        kw = {"gate": a} if gate == "gate" else {"gate_bits": O.relu_gate_pack(a)}
    shp = (nb, H, W, Cin)
    dense = O.conv_dgrad(dy.to(dev), w, shp, 3, 1, 1, **kw).clone()
    nan = float("nan")
    # (a) clean dy into a NaN-filled output: ONE writer -- tiles outside the map stay NaN (or, where the planner had to fall back
    # to the dense launch, every tile is written and equals it)
    out = torch.full(shp, nan, device=dev)
    O.conv_dgrad(dy.to(dev), w, shp, 3, 1, 1, out=out, sparse=sm.maps[0], **kw)
    torch.cuda.synchronize()
    tile_px = _tiles_to_pixels(flags, H, W).to(dev)
    assert torch.equal(out[tile_px], dense[tile_px])
    outside = out[~tile_px]
    ran_sparse = bool(torch.isnan(outside).all())
    assert ran_sparse or not torch.isnan(outside).any()
    # the planner's decision is the expected one for this shape and gate, and the launch did what the planner says
    planned = O.conv_dgrad_sparse_planned(shp, Cout, sm.maps[0], {"plain": 0, "gate": 1, "gate_bits": 2}[gate])
    assert planned == _expect_list_walk(nb, H, W, Cin, Cout)
    if share < 1.0:                                     # (every tile listed: nothing outside to look at)
        assert ran_sparse == planned
    # (b) dy is valid only where a needed output pixel reads it (two dilations): the needed pixels keep their bits
    dyp = dy.clone()
    dyp[~_dil(needed, 2)] = nan
    out = torch.full(shp, nan, device=dev)
    O.conv_dgrad(dyp.to(dev), w, shp, 3, 1, 1, out=out, sparse=sm.maps[0], **kw)
    torch.cuda.synchronize()
    n1 = need1.to(dev)
    assert torch.equal(out[n1], dense[n1])
    assert bool(torch.isfinite(out[n1]).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nb,H,W", [(2, 64, 64), (1, 48, 80), (2, 33, 47), (2, 18, 34), (2, 256, 256)])
def test_sparse_dgrad_to_one_channel_zeroes_the_rest(dev, kind, nb, H, W):
    """The 64 -> 1 dgrad (the trunk's first conv): dense bits where needed, exactly 0.0 elsewhere, finite everywhere, whatever
    the unneeded part of dy holds.  Sizes with W % 4 != 0 take the generic route + the zeroing pass."""
    from tg_hip import ops as O
    p, t, m, needed = _needed_pair(nb, H, W, 11 + H, kind)
    sm = _map(dev, p, t, m)
    if (H, W) == (256, 256) and kind == "blobs":
        assert 0.05 < torch.from_numpy(_read_map(sm, 0)[0]).float().mean().item() < 0.95
    g = torch.Generator().manual_seed(5 + H)
    dy = torch.randn(nb, H, W, 64, generator=g)
    w, _b = _weights(64, 1, 9, dev)
    shp = (nb, H, W, 1)
    dense = O.conv_dgrad(dy.to(dev), w, shp, 3, 1, 1).clone()
    dyp = dy.clone()
    dyp[~_dil(needed, 1)] = float("nan")
    out = torch.full(shp, float("nan"), device=dev)
    O.conv_dgrad(dyp.to(dev), w, shp, 3, 1, 1, out=out, sparse=sm.maps[0])
    torch.cuda.synchronize()
    n0 = needed.to(dev).unsqueeze(-1)
    assert torch.equal(out[n0], dense[n0])
    assert bool((out[~n0] == 0).all()) and bool(torch.isfinite(out).all())
    if kind == "full":
        assert torch.equal(out, dense)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nb,Ho,Wo,C", [(2, 32, 32, 64), (1, 24, 40, 128), (2, 9, 17, 64), (2, 128, 128, 64)])
def test_sparse_pool_code_backward(dev, kind, nb, Ho, Wo, C):
    from tg_hip import ops as O
    H, W = 2 * Ho, 2 * Wo
    p, t, m, needed = _needed_pair(nb, H, W, 11 + H, kind)
    sm = _map(dev, p, t, m)
    flags, cnt, _ = _read_map(sm, 0)
    flags = torch.from_numpy(flags)
    if (H, W) == (256, 256) and kind == "blobs":
        assert 0.05 < flags.float().mean().item() < 0.95
    g = torch.Generator().manual_seed(17 + Ho)
    dout = torch.randn(nb, Ho, Wo, C, generator=g)
    code = torch.randint(0, 8, (nb, Ho, Wo, C), generator=g, dtype=torch.uint8).to(dev)
    dense = O.maxpool2_bwd_code(dout.to(dev), code).clone()
    tile_px = _tiles_to_pixels(flags, H, W)
    # dout is valid only under the mapped tiles
    doutp = dout.clone()
    doutp[~(F.max_pool2d(tile_px.float().unsqueeze(1), 2, 2)[:, 0] > 0)] = float("nan")
    out = torch.full((nb, H, W, C), float("nan"), device=dev)
    O.maxpool2_bwd_code(doutp.to(dev), code, sparse=sm.maps[0], out=out)
    torch.cuda.synchronize()
    tp = tile_px.to(dev)
    assert torch.equal(out[tp], dense[tp])
    assert bool(torch.isnan(out[~tp]).all())            # one writer, nothing stray
    if kind == "full":
        assert torch.equal(out, dense)


def _crit(dev):
    from mvp_gan.src.utils.losses import InpaintingLoss
    torch.manual_seed(0)
    return InpaintingLoss(0.1, 0.1, device=torch.device("cpu")).to(dev)


@pytest.mark.parametrize("keep", [True, "gates"])
@pytest.mark.parametrize("wino4", [True, False])
def test_trunk_backward_sparse_equals_dense_and_zeroes(dev, monkeypatch, keep, wino4):
    """wino4=True: F(4x4,3x3) from the 128-channel layers up, as on the bench -- the sparse launches start below them.
    wino4=False: every dgrad is local, the whole backward runs on the maps and dfeat itself may be poisoned outside them."""
    from tg_hip import engine as E
    from tg_hip import ops as O
    monkeypatch.setattr(E, "VGG_SPARSE", True)
    monkeypatch.setattr(E, "VGG_SPARSE_BWD", True)
    nb, H, W = 2, 256, 256
    p, t, m, needed = _needed_pair(nb, H, W, 11 + H, "blobs")
    assert 0.05 < needed.float().mean().item() < 0.95
    V = _crit(dev)._vgg_tensors()
    both = torch.cat([p, t]).to(dev).contiguous()
    feats, ctx = E.vgg_forward(V, both, keep=keep, nb=nb, bwd_mask=m.to(dev).contiguous())
    assert ctx.smaps is not None and ctx.smaps.for_bwd
    _val, dfeat = O.l1_mean(feats[:nb], feats[nb:], 1.0, want_grad=True, relu_gate=True)
    dense = E.vgg_backward(ctx, dfeat.clone(), nb=nb, gated=True, wino4=wino4, sparse=False).clone()
    # every buffer the backward allocates starts as NaN
    real_empty = O.empty

    def nan_empty(*shape, like=None, device=None):
        return real_empty(*shape, like=like, device=device).fill_(float("nan"))
    monkeypatch.setattr(O, "empty", nan_empty)
    # every map-steered launch is recorded: did it leave something unwritten, and was it planned to?
    real_dgrad, real_pool = O.conv_dgrad, O.maxpool2_bwd_code
    seen = []

    def rec_dgrad(dy, w, x_shape, *a, **kw):
        out = real_dgrad(dy, w, x_shape, *a, **kw)
        sp = kw.get("sparse")
        if sp is not None and x_shape[3] != 1:
            gate = 1 if kw.get("gate") is not None else (2 if kw.get("gate_bits") is not None else 0)
            seen.append(("dgrad", tuple(x_shape), O.conv_dgrad_sparse_planned(tuple(x_shape), dy.shape[3], sp, gate),
                         bool(torch.isnan(out).any())))
        return out

    def rec_pool(dout, code, sparse=None, out=None):
        r = real_pool(dout, code, sparse=sparse, out=out)
        if sparse is not None:
            seen.append(("pool", tuple(r.shape), True, bool(torch.isnan(r).any())))
        return r
    monkeypatch.setattr(O, "conv_dgrad", rec_dgrad)
    monkeypatch.setattr(O, "maxpool2_bwd_code", rec_pool)
    df = dfeat.clone()
    if not wino4:
        # what the trunk's output gradient is needed at: the needed pixels carried through the trunk's geometry
        d = needed.float().unsqueeze(1)
        for it in E.VGG_TRUNK:
            d = F.max_pool2d(d, 2, 2) if it == "M" else F.max_pool2d(d, 3, 1, 1)
        df[~(d[:, 0] > 0).to(dev)] = float("nan")
    sparse = E.vgg_backward(ctx, df, nb=nb, gated=True, wino4=wino4, sparse=True)
    torch.cuda.synchronize()
    n0 = needed.to(dev)
    assert bool(torch.isfinite(sparse).all())
    assert torch.equal(sparse[n0], dense[n0])
    assert bool((sparse[~n0] == 0).all())
    assert bool((dense[~n0] != 0).any())                # (the dense gradient does live outside the holes: something was skipped)
    # intermediate tiles really stayed unwritten wherever the planner takes the list walk -- a dense fallback followed by the
    # zeroing pass would satisfy everything above.  vgg2's dgrad and pool 1's backward always do; with wino4=False vgg7's dgrad
    # and pool 2's backward as well (vgg5's 64 -> 128 splits K at this batch and runs dense)
    assert all(unwritten for _k, _s, planned, unwritten in seen if planned), seen
    want = {("dgrad", (nb, 256, 256, 64)), ("pool", (nb, 256, 256, 64))}
    if not wino4:
        want |= {("dgrad", (nb, 128, 128, 128)), ("pool", (nb, 128, 128, 128))}
    assert want <= {(k, s_) for k, s_, planned, _u in seen if planned}, seen


def _fractional(mask, seed):
    """A mask with values strictly between 0 and 1 -- 1 - 2^-24 among them -- sprinkled over the known region."""
    g = torch.Generator().manual_seed(seed)
    m = mask.clone()
    r = torch.rand(m.shape, generator=g)
    known = m == 1
    m[known & (r < 0.01)] = 1.0 - 2.0 ** -24
    m[known & (r > 0.99)] = 0.5
    m[(m == 0) & (r < 0.3)] = 0.25
    return m


@pytest.mark.parametrize("ckpt", [False, True])
def test_train_step_fractional_mask_sparse_equals_dense(dev, monkeypatch, ckpt):
    from oracle import terragan_oracle as Orc
    batches = []
    for s in (21, 22):
        real, mask = Orc.synth_batch(4, 128, s)
        mask = _fractional(mask, s)
        assert bool(((mask > 0) & (mask < 1)).any()) and bool((mask == 1.0 - 2.0 ** -24).any())
        batches.append((real.to(dev), mask.to(dev)))
    _same(_two_steps(dev, batches, False, ckpt, monkeypatch), _two_steps(dev, batches, True, ckpt, monkeypatch))


def test_module_autograd_stays_dense(dev, monkeypatch):
    """InpaintingLoss through autograd hands its gradient to arbitrary consumers: it is the dense one everywhere."""
    from oracle import terragan_oracle as Orc
    from tg_hip import engine as E
    crit = _crit(dev)
    real, mask = Orc.synth_batch(2, 128, 31)
    real, mask = real.to(dev), mask.to(dev)
    torch.manual_seed(1)
    pred0 = (real * mask + (1 - mask) * torch.rand_like(real)).detach()
    grads = []
    for on in (False, True):
        monkeypatch.setattr(E, "VGG_SPARSE", on)
        pred = pred0.clone().requires_grad_(True)
        crit(pred, real, mask).backward()
        grads.append(pred.grad.clone())
    torch.cuda.synchronize()
    assert torch.equal(grads[0], grads[1])
    outside = (mask == 1) & (pred0 == real)
    assert bool((grads[1][outside] != 0).any())         # a consumer outside the holes sees the perceptual gradient


def test_graph_replay_sparse_backward_equals_eager(dev, monkeypatch):
    from mvp_gan.src.train import train_step
    from oracle import terragan_oracle as Orc
    from tg_hip import engine as E
    from tg_hip.graph import GraphedTrainStep
    monkeypatch.setattr(E, "VGG_SPARSE", True)
    monkeypatch.setattr(E, "VGG_SPARSE_BWD", True)
    batches = []
    for s in (1000, 1001, 1002, 1003):
        real, mask = Orc.synth_batch(4, 128, s)
        batches.append((real.to(dev), (_fractional(mask, s) if s & 1 else mask).to(dev)))
    G, D, crit, oG, oD = _build(dev)
    eager = [train_step(G, D, crit, oG, oD, r, m)["gen"].clone() for r, m in batches]
    se = _state(G, D, oG, oD)
    G2, D2, crit2, oG2, oD2 = _build(dev)
    step = GraphedTrainStep(G2, D2, crit2, oG2, oD2, warmup=2)
    graphed = [step(r, m)["gen"].clone() for r, m in batches]
    torch.cuda.synchronize()
    assert step.graph is not None and step.replays >= 1
    for a, b in zip(eager, graphed):
        assert torch.equal(a, b)
    for a, b in zip(se, _state(G2, D2, oG2, oD2)):
        assert torch.equal(a, b)
