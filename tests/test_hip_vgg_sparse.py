"""Prediction-half tile maps of the frozen VGG trunk (tg_vgg_sparse_map) and the sparse forward launches that honour them
(tg_conv_fwd_sparse): the maps match a max-pool reference of the difference image, every sparse launch is bit-identical to the
dense one, and so are whole train steps (TG_VGG_SPARSE on / off), eager and graphed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PLAN = "CCMCCMCCC"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def _ref_tiles(pred, target, plan):
    """CPU reference: per conv of `plan`, bool [nb][tiles_y][tiles_x] -- a 16x16 output tile whose receptive field holds a pixel
    whose bit pattern differs between pred and target."""
    d = (pred.view(torch.int32) != target.view(torch.int32)).float().unsqueeze(1)
    out = []
    for op in plan:
        if op == "C":
            d = F.max_pool2d(d, 3, 1, 1)
            H, W = d.shape[2:]
            ty, tx = -(-H // 16), -(-W // 16)
            pad = F.pad(d, (0, 16 * tx - W, 0, 16 * ty - H))
            out.append(F.max_pool2d(pad, 16, 16)[:, 0] > 0)
        else:
            d = F.max_pool2d(d, 2, 2)
    return out


def _read_map(sm, i):
    m = sm.maps[i]
    n = m.nb * m.tiles_y * m.tiles_x
    base = sm.buf.data_ptr()
    raw = sm.buf.cpu().numpy()
    cnt = int(raw[m.count - base:m.count - base + 4].view(np.int32)[0])
    bits = raw[m.bits - base:m.bits - base + 4 * ((n + 31) // 32)].view(np.uint32)
    flags = ((bits[np.arange(n) // 32] >> (np.arange(n) % 32).astype(np.uint32)) & 1).astype(bool)
    lst = raw[m.list - base:m.list - base + 4 * cnt].view(np.int32)
    return flags.reshape(m.nb, m.tiles_y, m.tiles_x), cnt, lst


def _pair(nb, H, W, seed, kind):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(nb, H, W, generator=g)
    p = t.clone()
    if kind == "blobs":
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        for b in range(nb):
            for _ in range(3):
                cy, cx, r = (torch.randint(0, H, (1,), generator=g).item(), torch.randint(0, W, (1,), generator=g).item(),
                             torch.randint(2, max(3, H // 6), (1,), generator=g).item())
                sel = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
                p[b][sel] = torch.rand(int(sel.sum()), generator=g)
    elif kind == "corners":
        for b in range(nb):
            for (y, x) in ((0, 0), (15, 15), (16, 16), (H - 1, W - 1), (0, W - 1), (H // 2, 31)):
                if y < H and x < W:
                    p[b, y, x] += 0.25
    elif kind == "signed_zero":
        t[:, 5, 7] = 0.0
        p[:, 5, 7] = -0.0
    elif kind == "full":
        p = p + 1.0
    return p, t


@pytest.mark.parametrize("kind", ["blobs", "corners", "signed_zero", "empty", "full"])
@pytest.mark.parametrize("nb,H,W", [(3, 64, 48), (1, 72, 40), (2, 256, 256)])
def test_map_matches_reference(dev, kind, nb, H, W):
    from tg_hip import ops as O
    p, t = _pair(nb, H, W, 11 + H, kind)
    x = torch.cat([p, t]).to(dev).contiguous()
    sm = O.vgg_sparse_map(x, nb, PLAN)
    assert sm is not None
    ref = _ref_tiles(p, t, PLAN)
    for i, r in enumerate(ref):
        flags, cnt, lst = _read_map(sm, i)
        assert np.array_equal(flags, r.numpy()), (i, kind)
        want = np.flatnonzero(r.numpy().reshape(-1))
        assert cnt == want.size and np.array_equal(lst, want), (i, kind)
    if kind == "signed_zero":
        assert _read_map(sm, 0)[1] > 0


def _act_pair(nb, H, W, Cin, seed, kind):
    """[pred; target] activations [2 nb][H][W][Cin] that differ exactly where the 1-channel pair of `kind` does, and that pair."""
    p1, t1 = _pair(nb, H, W, seed, kind)
    g = torch.Generator().manual_seed(seed + 1)
    tgt = torch.relu(torch.randn(nb, H, W, Cin, generator=g))
    pred = tgt.clone()
    diff = p1.view(torch.int32) != t1.view(torch.int32)
    pred[diff] = torch.relu(torch.randn(int(diff.sum()), Cin, generator=g)) + 0.5
    return torch.cat([pred, tgt]), torch.cat([p1, t1])


def _weights(Cout, Cin, seed, dev):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5).to(dev)
    b = (0.1 * torch.randn(Cout, generator=g)).to(dev)
    return w, b


@pytest.mark.parametrize("kind", ["blobs", "corners", "signed_zero", "empty", "full"])
@pytest.mark.parametrize("mode", ["plain", "pool", "code"])
@pytest.mark.parametrize("nb,H,W,Cin,Cout", [(2, 64, 64, 64, 64), (1, 48, 80, 64, 128), (2, 32, 32, 256, 256)])
def test_sparse_launch_equals_dense(dev, kind, mode, nb, H, W, Cin, Cout, tmp_path):
    from tests import wino_cases as WC
    from tests.test_hip_direct_conv import Routes
    from tg_hip import ops as O
    rt = Routes(tmp_path / "launches.csv")
    a, x1 = _act_pair(nb, H, W, Cin, 100 + H + Cin, kind)
    a, x1 = a.to(dev).contiguous(), x1.to(dev).contiguous()
    w, b = _weights(Cout, Cin, 7 + Cout, dev)
    sm = O.vgg_sparse_map(x1, nb, "C")
    sp = sm.maps[0]
    if mode == "code" and O.conv_pool_code_supported(tuple(a.shape), Cout):
        yp0, c0 = O.conv_fwd_pool_code(a, w, b)
        yp0, c0 = yp0.clone(), c0.clone()
        with rt:
            yp1, c1 = O.conv_fwd_pool_code(a, w, b, sparse=sp)
        torch.cuda.synchronize()
        assert torch.equal(yp0, yp1) and torch.equal(c0, c1)
    elif mode != "plain":           # (also "code" where the geometry has no pool-code path)
        y0, yp0 = O.conv_fwd(a, w, b, 3, 1, 1, act=O.ACT_RELU, pool=True)
        y0, yp0 = y0.clone(), yp0.clone()
        with rt:
            y1, yp1 = O.conv_fwd(a, w, b, 3, 1, 1, act=O.ACT_RELU, pool=True, sparse=sp)
        torch.cuda.synchronize()
        assert torch.equal(y0, y1) and torch.equal(yp0, yp1)
    else:
        y0 = O.conv_fwd(a, w, b, 3, 1, 1, act=O.ACT_RELU).clone()
        with rt:
            y1 = O.conv_fwd(a, w, b, 3, 1, 1, act=O.ACT_RELU, sparse=sp)
        torch.cuda.synchronize()
        assert torch.equal(y0, y1)
    # ... and where wino_plan's conditions say the map is honoured (the pipelined kernel in one split, with the pool fused where
    # one is asked for), the launch record must name a tile-map instantiation: equal bits alone would also pass a dense launch
    pl = WC.wino_plan(2 * nb, H, W, Cin, Cout, pool=mode != "plain")
    if pl["pipe"] and pl["splits"] == 1 and (mode == "plain" or pl["pool"]):
        assert rt.rows == [(0, 4064, WC.R_MAP if mode == "plain" else WC.R_MAP_POOL)], rt.rows
    else:
        assert len(rt.rows) == 1 and rt.rows[0][:2] == (0, 4064) and rt.rows[0][2] not in WC.MAP_ROUTES, rt.rows


@pytest.mark.parametrize("H,W", [(33, 47), (18, 34)])
def test_sparse_launch_odd_and_small_sizes(dev, H, W):
    """Sizes the pooled kernel cannot take (odd) or tile grids with partial tiles: the result is still the dense one."""
    from tg_hip import ops as O
    nb, Cin, Cout = 2, 64, 64
    a, x1 = _act_pair(nb, H, W, Cin, 5 + H, "blobs")
    a, x1 = a.to(dev).contiguous(), x1.to(dev).contiguous()
    w, b = _weights(Cout, Cin, 3, dev)
    sp = O.vgg_sparse_map(x1, nb, "C").maps[0]
    y0 = O.conv_fwd(a, w, b, 3, 1, 1, act=O.ACT_RELU).clone()
    y1 = O.conv_fwd(a, w, b, 3, 1, 1, act=O.ACT_RELU, sparse=sp)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)


def _build(dev, seed=0):
    from mvp_gan.src.models import Discriminator, PConvUNet
    from mvp_gan.src.utils.losses import InpaintingLoss
    torch.manual_seed(seed)
    G, D = PConvUNet(), Discriminator()
    crit = InpaintingLoss(0.1, 0.1, device=torch.device("cpu"))
    G, D, crit = G.to(dev), D.to(dev), crit.to(dev)
    return G, D, crit, torch.optim.Adam(G.parameters(), lr=2e-4), torch.optim.Adam(D.parameters(), lr=2e-4)


def _state(G, D, oG, oD):
    t = [p_.detach().clone() for p_ in list(G.parameters()) + list(D.parameters())]
    for o in (oG, oD):
        for st in o.state.values():
            t += [st[k].detach().clone() for k in ("exp_avg", "exp_avg_sq")]
    return t


def _two_steps(dev, batches, sparse, ckpt=False, monkeypatch=None):
    from mvp_gan.src.train import train_step
    from tg_hip import engine as E
    monkeypatch.setattr(E, "VGG_SPARSE", sparse)
    G, D, crit, oG, oD = _build(dev)
    G.activation_checkpointing = ckpt
    outs = []
    for real, mask in batches:
        out = train_step(G, D, crit, oG, oD, real, mask)
        outs.append((out["gen"].clone(), float(out["g_total"]), float(out["d_loss"]), float(out["g_loss"])))
    torch.cuda.synchronize()
    return outs, _state(G, D, oG, oD)


def _same(a, b):
    (oa, sa), (ob, sb) = a, b
    for x, y in zip(oa, ob):
        assert torch.equal(x[0], y[0]) and x[1:] == y[1:]
    assert len(sa) == len(sb)
    for x, y in zip(sa, sb):
        assert torch.equal(x, y)


@pytest.mark.parametrize("B,size,seeds,ckpt", [(16, 256, (1000, 1001), False), (16, 256, (1002, 1003), True),
                                               (3, (72, 40), (5, 6), False)])
def test_train_step_sparse_equals_dense(dev, monkeypatch, B, size, seeds, ckpt):
    from oracle import terragan_oracle as Orc
    batches = []
    for s in seeds:
        if isinstance(size, tuple):
            real, mask = Orc.synth_batch(B, max(size), s)
            real, mask = real[..., :size[0], :size[1]].contiguous(), mask[..., :size[0], :size[1]].contiguous()
        else:
            real, mask = Orc.synth_batch(B, size, s)
        batches.append((real.to(dev), mask.to(dev)))
    dense = _two_steps(dev, batches, False, ckpt, monkeypatch)
    sparse = _two_steps(dev, batches, True, ckpt, monkeypatch)
    _same(dense, sparse)


def test_graph_replay_sparse_equals_eager(dev, monkeypatch):
    from mvp_gan.src.train import train_step
    from oracle import terragan_oracle as Orc
    from tg_hip import engine as E
    from tg_hip.graph import GraphedTrainStep
    monkeypatch.setattr(E, "VGG_SPARSE", True)
    batches = []
    for s in (1000, 1001, 1002, 1003):
        real, mask = Orc.synth_batch(4, 128, s)
        batches.append((real.to(dev), mask.to(dev)))
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
