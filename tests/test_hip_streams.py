"""GPU checks of the stream network, the height above the nearest drainage and the flood comparison (csrc/drainage.hip,
mvp_gan/src/flow_routing.py stream_network and hand, mvp_gan/src/evaluate_raster.py flood_errors) against the
numpy oracle of tests/streams_oracle.py.  Classes, links, step counts, orders and the bits of HAND and of the distances are compared
bit for bit, the counters and every number derived from them exactly; nothing has a tolerance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import drainage_oracle as DR
from tests import flow_oracle as FO
from tests import streams_oracle as SO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = (0.25, 0.5, 1.0, 2.0)
_REF = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def _route(name, z, fill=True, mask=None):
    """The oracle's routing of a named scene, computed once and left unchanged."""
    key = (name, fill)
    if key not in _REF:
        r = FO.route(z, mask, None, fill)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _net(name, code, acc, mc):
    """The oracle's network of a named scene in both forms, computed once."""
    key = ("net", name, mc)
    if key not in _REF:
        a, b = SO.network_kahn(code, acc, mc), SO.network_links(code, acc, mc)
        for k in ("cls", "link", "nc", "nd", "order"):
            assert np.array_equal(a[k], b[k]), k
        a["link_rounds"], a["sync_rounds"] = b["link_rounds"], b["order_rounds"]
        _REF[key] = a
    return _REF[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ops_net(dev, code, acc, mc, cellsize=1.0, link_batch=8, order_batch=8, max_rounds=1 << 16):
    """The network through the ops -> dict of numpy planes, the counts, and the rounds."""
    from tg_hip import ops as O
    H, W = code.shape
    d = torch.from_numpy(np.array(code)).to(dev)
    a = torch.from_numpy(np.array(acc, np.int32)).to(dev)
    ws = O.flow_basin_ws(H, W, dev)
    cls, node, c0 = O.stream_class(d, a, mc, ws)
    start = node.cpu().numpy().copy()
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    k = 0
    while k < 32:
        n = min(link_batch, 32 - k)
        O.flow_basin(H, W, k, n, state, ws)
        k += n
        if state.cpu().tolist()[0] == 0:
            break
    link_rounds = state.cpu().tolist()[1]
    top, nc, nd, ln, c1 = O.flow_basin_finish(H, W, link_rounds, ws, cellsize, want_steps=True)
    junctions = torch.nonzero(cls.reshape(-1) == O.STREAM_JUNCTION).reshape(-1).to(torch.int32)
    changed = torch.full((1,), -7, dtype=torch.int32, device=dev)
    rounds, left = 0, 1
    while left and rounds < max_rounds:
        O.stream_order(d, cls, top, junctions, order_batch, node, changed)
        rounds += order_batch
        left = int(changed.item())
    out, c2 = O.stream_order_finish(cls, top, node)
    return {"cls": cls.cpu().numpy(), "link": top.cpu().numpy(), "nc": nc.cpu().numpy(), "nd": nd.cpu().numpy(),
            "order": out.cpu().numpy(), "length": ln.cpu().numpy(), "start": start, "c0": c0.cpu().tolist(), "c1": c1.cpu().tolist(),
            "c2": c2.cpu().tolist(), "link_rounds": link_rounds, "order_rounds": rounds, "nj": junctions.numel(), "left": left}


def _check(dev, name, code, acc, mc, cellsize=1.0, **kw):
    """stream_network and the ops against the oracle: class, order, link, nc, nd and every count -> (oracle, info)."""
    from mvp_gan.src.flow_routing import stream_network
    want = _net(name, code, acc, mc)
    wi = SO.info(want, cellsize)
    order, link, info = stream_network(code, acc, mc, cellsize=cellsize, **kw)
    assert order.dtype == torch.uint8 and link.dtype == torch.int32 and order.is_cuda and link.is_cuda
    assert tuple(order.shape) == tuple(link.shape) == code.shape
    np.testing.assert_array_equal(order.cpu().numpy(), want["order"])
    np.testing.assert_array_equal(link.cpu().numpy(), want["link"])
    assert {k: info[k] for k in wi} == wi, (info, wi)
    ce = kw.get("check_every", 8)
    assert info["converged"] is True and info["link_rounds"] == want["link_rounds"]
    # in place a round sees values of its own, so it is never behind the synchronous iteration; read back every ce rounds
    assert info["order_rounds"] <= -(-want["sync_rounds"] // ce) * ce and (info["order_rounds"] > 0) == (want["junctions"] > 0)
    assert set(info) == set(wi) | {"link_rounds", "order_rounds", "converged"}
    g = _ops_net(dev, code, acc, mc, cellsize)
    for k in ("cls", "link", "nc", "nd", "order"):
        np.testing.assert_array_equal(g[k], want[k], err_msg=k)
    np.testing.assert_array_equal(g["start"], (want["cls"] != 0).astype(np.int32))
    np.testing.assert_array_equal(_bits(g["length"]), _bits(DR.length_m(want["nc"], want["nd"], cellsize)))
    assert g["c0"] == [want["cells"], want["heads"], want["junctions"], want["outlets"]] and g["nj"] == want["junctions"]
    mx, cells, links = SO.order_counts(want)
    assert g["c2"] == [mx] + cells + links and sum(links) == want["heads"] + want["junctions"] and sum(cells) == want["cells"]
    assert g["link_rounds"] == want["link_rounds"] and g["left"] == 0
    return want, info


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def _small():
    return {"1x1": np.full((1, 1), 1000.5, np.float32), "1x300": FO.rounded_pits(1, 300, 1), "300x1": FO.rounded_pits(300, 1, 2),
            "2x2": FO.rounded_pits(2, 2, 3, npits=1)}


@pytest.mark.parametrize("name", list(_small()))
def test_small_shapes(dev, name):
    r = _route(name, _small()[name])
    want, info = _check(dev, name, r["dir"], r["acc"], 1)
    assert info["stream_cells"] == r["dir"].size and info["outlets"] >= 1
    if name == "1x1":
        assert info == {"stream_cells": 1, "heads": 1, "junctions": 0, "outlets": 1, "links": 1, "max_order": 1,
                        "cells_by_order": [1] + [0] * 14, "links_by_order": [1] + [0] * 14, "link_rounds": 0, "order_rounds": 0,
                        "converged": True, "longest_link_m": 0.0}
    if name in ("1x300", "300x1"):
        _check(dev, name, r["dir"], r["acc"], 3)


@pytest.mark.parametrize("mc", (1, 20))
@pytest.mark.parametrize("H", (63, 64, 65, 129))
@pytest.mark.parametrize("W", (127, 128, 130))
def test_tile_shapes(dev, H, W, mc):
    name = f"rounded {H}x{W}"
    r = _route(name, FO.rounded_pits(H, W, 100 * H + W, npits=20))
    want, info = _check(dev, name, r["dir"], r["acc"], mc, cellsize=2.0)
    assert info["junctions"] > (1000 if mc == 1 else 20) and info["max_order"] >= (5 if mc == 1 else 3)
    assert (want["nd"] > 0).any() and (want["nc"] > 0).any() and info["link_rounds"] >= 2


def _voids():
    """67x130 with 5 % voids, half by the mask and half NaN -> (z, mask)."""
    rng = np.random.default_rng(5)
    z = FO.rounded_pits(67, 130, 5, npits=12)
    mask = (rng.random(z.shape) >= 0.025).astype(np.float32)
    z[rng.random(z.shape) < 0.025] = np.nan
    return z, mask


def _voids_route():
    z, mask = _voids()
    return _route("voids 67x130", z, True, mask)


def test_voids(dev):
    r = _voids_route()
    assert 0.03 < (~r["known"]).mean() < 0.07
    for mc in (1, 5):
        want, info = _check(dev, "voids 67x130", r["dir"], r["acc"], mc)
        assert (want["link"][~r["known"]] == -1).all() and (want["order"][~r["known"]] == 0).all()
    # an accumulation plane that does not belong to the grid: streams that end in mid-slope
    acc = np.random.default_rng(6).integers(0, 6, r["acc"].shape).astype(np.int32)
    want, info = _check(dev, "voids 67x130 foreign acc", r["dir"], acc, 3)
    assert info["outlets"] > int(np.isin(r["dir"], (FO.OUT, FO.PIT)).sum())


def _serpentine():
    """The first 8130 cells of the channel of flow_oracle.serpentine as a hand-made grid: every cell flows to the next one along
    the channel, the last one OUT, everything else unknown; the accumulation plane is 1 on the channel.  One head, one link of
    8130 cells: 8129 steps, 13 rounds of the doubling."""
    _, order = FO.serpentine()
    order = np.where(order < 8130, order, -1)
    code = np.zeros(order.shape, np.uint8)
    ys, xs = np.nonzero(order >= 0)
    idx = np.argsort(order[ys, xs])
    ys, xs = ys[idx], xs[idx]
    step = {(0, 1): 1, (1, 0): 3, (0, -1): 5, (-1, 0): 7}
    for i in range(len(ys) - 1):
        code[ys[i], xs[i]] = step[(ys[i + 1] - ys[i], xs[i + 1] - xs[i])]
    code[ys[-1], xs[-1]] = FO.OUT
    return code, (order >= 0).astype(np.int32), (int(ys[0]), int(xs[0]))


def test_serpentine(dev):
    """One link of 8130 cells, 13 rounds of the doubling: a record torn between two iterates or a wrong final plane would show."""
    code, acc, (y0, x0) = _serpentine()
    want, info = _check(dev, "serpentine", code, acc, 1)
    assert (info["stream_cells"], info["heads"], info["junctions"], info["outlets"], info["max_order"]) == (8130, 1, 0, 1, 1)
    assert info["link_rounds"] == 13 and info["order_rounds"] == 0 and info["longest_link_m"] == 8129.0
    assert (want["link"][code != 0] == y0 * 130 + x0).all() and want["nc"].max() == 8129 and not want["nd"].any()


def test_spiral_flat(dev):
    z, channel = FO.spiral_flat()
    r = _route("spiral flat", z, fill=False)
    for mc in (1, 30):
        want, info = _check(dev, "spiral flat", r["dir"], r["acc"], mc, cellsize=0.5)
    assert info["junctions"] > 0 and info["link_rounds"] >= 5


def test_comb(dev):
    code, acc = SO.comb()
    want, info = _check(dev, "comb", code, acc, 1)
    assert want["sync_rounds"] == 132 and info["junctions"] == 132 and info["max_order"] == 3
    assert info["cells_by_order"][:3] == [4 + 129, 2, 260] and info["links_by_order"][:3] == [4 + 129, 2, 130]


def test_empty_and_no_stream(dev):
    code = np.zeros((70, 65), np.uint8)
    want, info = _check(dev, "empty", code, np.zeros((70, 65), np.int32), 1)
    none = {"stream_cells": 0, "heads": 0, "junctions": 0, "outlets": 0, "links": 0, "max_order": 0, "cells_by_order": [0] * 15,
            "links_by_order": [0] * 15, "link_rounds": 0, "order_rounds": 0, "converged": True, "longest_link_m": 0.0}
    assert info == none
    r = _voids_route()
    want, info = _check(dev, "voids 67x130", r["dir"], r["acc"], int(r["acc"].max()) + 1)      # nj = 0: nothing is launched
    assert info == none
    want, info = _check(dev, "voids 67x130", r["dir"], r["acc"], int(r["acc"].max()))
    assert info["stream_cells"] >= 1 and info["junctions"] == 0 and info["max_order"] == 1


# ---- the rounds --------------------------------------------------------------------------------------------------------------
def test_rounds_in_batches(dev):
    code, acc, _ = _serpentine()
    ws = _net("serpentine", code, acc, 1)
    cc, ca = SO.comb()
    wc = _net("comb", cc, ca, 1)
    r = _route("rounded 129x130", FO.rounded_pits(129, 130, 100 * 129 + 130, npits=20))
    wr = _net("rounded 129x130", r["dir"], r["acc"], 1)
    for batch in (1, 5, 32):
        g = _ops_net(dev, code, acc, 1, link_batch=batch)
        assert g["link_rounds"] == 13 and g["order_rounds"] == 8 and g["left"] == 0     # nj = 0: changed is zeroed all the same
        for k in ("cls", "link", "nc", "nd", "order"):
            np.testing.assert_array_equal(g[k], ws[k], err_msg=k)
        for w, (c, a) in ((wc, (cc, ca)), (wr, (r["dir"], r["acc"]))):
            g = _ops_net(dev, c, a, 1, link_batch=batch, order_batch=batch)
            assert g["left"] == 0 and g["order_rounds"] <= -(-w["sync_rounds"] // batch) * batch
            for k in ("cls", "link", "nc", "nd", "order"):
                np.testing.assert_array_equal(g[k], w[k], err_msg=k)


def test_reproducible_and_check_every(dev):
    from mvp_gan.src.flow_routing import stream_network
    cc, ca = SO.comb()
    r = _voids_route()
    for code, acc in ((r["dir"], r["acc"]), (cc, ca)):
        outs = [stream_network(code, acc, 1, cellsize=2.0, check_every=n) for n in (8, 8, 1, 64)]
        for o, l, i in outs[1:]:
            assert torch.equal(o, outs[0][0]) and torch.equal(l, outs[0][1])
            assert {k: v for k, v in i.items() if k != "order_rounds"} == {k: v for k, v in outs[0][2].items() if k != "order_rounds"}
        assert outs[3][2]["order_rounds"] % 64 == 0


def test_stopped_early(dev):
    from mvp_gan.src.flow_routing import stream_network
    code, acc = SO.comb()
    want = _net("comb", code, acc, 1)
    order, link, info = stream_network(code, acc, 1, max_rounds=2, check_every=1)
    got = order.cpu().numpy()
    S = want["order"] > 0
    assert info["converged"] is False and info["order_rounds"] == 2
    assert (got <= want["order"]).all() and (got[S] >= 1).all() and (got[~S] == 0).all() and (got < want["order"]).any()
    np.testing.assert_array_equal(link.cpu().numpy(), want["link"])
    # HAND against the streams of an order refuses lower bounds: they would leave links out of the drainage
    from mvp_gan.src.flow_routing import hand_routed
    d, a = torch.from_numpy(code).to(dev), torch.from_numpy(acc).to(dev)
    w = torch.zeros(code.shape, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match="not converged after 2 rounds"):
        hand_routed(w, d, a, {}, 1.0, 1, min_order=3, check_every=1, max_rounds=2)
    h, _, info, stream = hand_routed(w, d, a, {}, 1.0, 1, min_order=3)
    np.testing.assert_array_equal(stream.cpu().numpy(), (want["order"] >= 3).astype(np.uint8))
    assert info["drained"] == int((code != 0).sum()) and info["network"]["converged"] and info["stream_cells"] == 260


def test_inputs_numpy_and_tensor(dev):
    from mvp_gan.src.flow_routing import flow_routing, stream_network
    zv, mask = _voids()
    r = _voids_route()
    want = _net("voids 67x130", r["dir"], r["acc"], 5)
    direction, acc, _ = flow_routing(zv, mask)
    for d, a in ((np.array(r["dir"]), np.array(r["acc"])), (torch.from_numpy(np.array(r["dir"])).to(dev), np.array(r["acc"])),
                 (direction, acc)):
        order, link, _ = stream_network(d, a, 5)
        np.testing.assert_array_equal(order.cpu().numpy(), want["order"])
        np.testing.assert_array_equal(link.cpu().numpy(), want["link"])
    with pytest.raises(ValueError, match="pass a numpy array or a HIP tensor"):
        stream_network(torch.from_numpy(np.array(r["dir"])), np.array(r["acc"]), 5)
    with pytest.raises(ValueError, match="pass a numpy array or a HIP tensor"):
        stream_network(np.array(r["dir"]), torch.from_numpy(np.array(r["acc"])), 5)
    bad = np.array(r["dir"])
    bad[5, 5] = 254
    with pytest.raises(ValueError, match="254"):
        stream_network(bad, np.array(r["acc"]), 5)


# ---- HAND --------------------------------------------------------------------------------------------------------------------
def _hand_check(dev, name, z, mask=None, cellsize=1.0, min_cells=20, min_order=1, fill=True):
    from mvp_gan.src.flow_routing import hand
    r = _route(name, z, fill, mask)
    want = SO.hand(r["w"], r["dir"], SO.drainage_mask(r["dir"], r["acc"], min_cells, min_order), cellsize)
    outs = []
    for zz, mm in ((z, mask), (torch.from_numpy(np.array(z)).to(dev), None if mask is None else torch.from_numpy(mask).to(dev))):
        h, dist, info = hand(zz, mm, cellsize=cellsize, min_cells=min_cells, min_order=min_order, fill=fill)
        assert h.dtype == dist.dtype == torch.float32 and h.is_cuda and tuple(h.shape) == tuple(dist.shape) == z.shape
        np.testing.assert_array_equal(_bits(h.cpu().numpy()), _bits(want["hand"]))
        np.testing.assert_array_equal(_bits(dist.cpu().numpy()), _bits(want["distance"]))
        got = {k: info[k] for k in ("drained", "undrained", "stream_cells", "max_hand_m", "rounds")}
        assert got == {"drained": want["drained"], "undrained": want["undrained"], "stream_cells": want["stream_cells"],
                       "max_hand_m": want["max_hand"], "rounds": want["rounds"]}
        assert info["known"] == int(r["known"].sum()) and info["pits"] == r["pits"] and info["filled"] is fill
        assert ("network" in info) == (min_order > 1)
        outs.append((h, dist))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    return want, info


@pytest.mark.parametrize("name", list(_small()))
def test_hand_small_shapes(dev, name):
    """The scenes of test_small_shapes: every pixel a drainage pixel (all zeros), and a threshold that leaves slopes above it."""
    z = _small()[name]
    want, info = _hand_check(dev, name, z, min_cells=1)
    assert info["drained"] == info["stream_cells"] == z.size and info["undrained"] == 0 and not want["hand"].any()
    want, info = _hand_check(dev, name, z, cellsize=2.0, min_cells=3)
    assert info["drained"] + info["undrained"] == z.size
    if name in ("1x300", "300x1"):
        assert info["drained"] > 100 and info["undrained"] > 50 and info["max_hand_m"] >= 10.0 and info["rounds"] == 2
    if name == "1x1":
        assert (info["drained"], info["undrained"], info["stream_cells"]) == (0, 1, 0) and np.isnan(want["hand"]).all()


@pytest.mark.parametrize("H", (63, 64, 65, 129))
@pytest.mark.parametrize("W", (127, 128, 130))
def test_hand_tile_shapes(dev, H, W):
    """The scenes of test_tile_shapes."""
    z = FO.rounded_pits(H, W, 100 * H + W, npits=20)
    want, info = _hand_check(dev, f"rounded {H}x{W}", z, cellsize=2.0, min_cells=20)
    assert info["drained"] > 0.5 * H * W and info["undrained"] > 0 and info["max_hand_m"] >= 2.0
    fin = ~np.isnan(want["hand"])
    assert (want["hand"][fin] >= 0).all()
    w2, i2 = _hand_check(dev, f"rounded {H}x{W}", z, cellsize=2.0, min_cells=4, min_order=2)
    w1, i1 = _hand_check(dev, f"rounded {H}x{W}", z, cellsize=2.0, min_cells=4)
    assert 0 < i2["stream_cells"] < i1["stream_cells"] and i2["network"]["max_order"] >= 3 and i2["network"]["converged"]
    _hand_check(dev, f"rounded {H}x{W}", z, min_cells=1)


def test_hand_spiral_flat(dev):
    """The scene of test_spiral_flat, routed as given: the channel floor is one flat, so every drained pixel of it has a hand
    of exactly 0 and a distance that runs along the channel."""
    z, channel = FO.spiral_flat()
    for mc in (30, 3000):
        want, info = _hand_check(dev, "spiral flat", z, cellsize=0.5, min_cells=mc, fill=False)
        fin = ~np.isnan(want["hand"])
        assert (want["hand"][channel & fin] == 0).all() and (channel & fin).sum() > 10000 and info["max_hand_m"] == 100.0
    assert info["undrained"] == 260 and info["rounds"] >= 10 and np.nanmax(np.where(channel, want["distance"], np.nan)) > 400.0
    _hand_check(dev, "spiral flat", z, cellsize=0.5, min_cells=1, fill=False)


def test_hand_voids_pit_and_scenes(dev):
    z, mask = _voids()
    want, info = _hand_check(dev, "voids 67x130", z, mask, cellsize=0.5, min_cells=10)
    assert np.isnan(want["hand"][mask == 0]).all() and info["unknown"] > 100
    _hand_check(dev, "voids 67x130", z, mask, min_cells=1)                              # every known pixel is drainage: all zeros
    # no stream: a threshold above the largest accumulation leaves every known pixel undrained
    r = _voids_route()
    want, info = _hand_check(dev, "voids 67x130", z, mask, min_cells=int(r["acc"].max()) + 1)
    assert (info["drained"], info["stream_cells"], info["max_hand_m"]) == (0, 0, 0.0) and info["undrained"] == info["known"]
    assert np.isnan(want["hand"]).all() and np.isnan(want["distance"]).all()
    pit = np.array([[1003, 1002, 1004], [1001, 990, 1005], [1006, 1002.5, 1007]], np.float32)
    want, info = _hand_check(dev, "3x3 pit", pit, min_cells=9, fill=False)
    assert info["drained"] == 9 and info["max_hand_m"] == 17.0 and want["hand"][1, 1] == 0 and info["pits"] == 1
    want, info = _hand_check(dev, "3x3 pit", pit, min_cells=10, fill=False)
    assert (info["drained"], info["undrained"], info["stream_cells"], info["max_hand_m"]) == (0, 9, 0, 0.0)
    zs, _ = FO.serpentine()
    want, info = _hand_check(dev, "serpentine z", zs, min_cells=4000, fill=False)
    assert info["rounds"] >= 10 and info["drained"] > 4000
    _hand_check(dev, "serpentine z", zs, min_cells=4000)
    nan = np.full((5, 70), np.nan, np.float32)
    want, info = _hand_check(dev, "no known pixel", nan, min_cells=1)
    assert info["drained"] == info["undrained"] == info["stream_cells"] == 0 and np.isnan(want["hand"]).all()


def test_hand_ops(dev):
    """tg_hand on planes given directly: terminals off the drainage, negative and out-of-range basins, no distance plane."""
    from tg_hip import ops as O
    rng = np.random.default_rng(11)
    H, W = 7, 70
    w = rng.normal(1000, 5, (H, W)).astype(np.float32)
    basin = rng.integers(0, H * W, (H, W)).astype(np.int32)
    basin[rng.random((H, W)) < 0.2] = -1
    sm = (rng.random((H, W)) < 0.5).astype(np.uint8)
    ln = rng.random((H, W)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    h, dist, counts = O.hand(t(w), t(basin), t(sm), t(ln))
    ok = basin >= 0
    drained = ok & (sm.ravel()[np.where(ok, basin, 0)] != 0)
    want = np.where(drained, w - w.ravel()[np.where(ok, basin, 0)], np.float32(np.nan)).astype(np.float32)
    np.testing.assert_array_equal(_bits(h.cpu().numpy()), _bits(want))
    np.testing.assert_array_equal(_bits(dist.cpu().numpy()), _bits(np.where(drained, ln, np.float32(np.nan))))
    pos = want[drained & (want > 0)]
    assert counts.cpu().tolist() == [int(drained.sum()), int((ok & ~drained).sum()), int(((sm != 0) & ok).sum()),
                                     int(pos.max().view(np.uint32))]
    h2, none, c2 = O.hand(t(w), t(basin), t(sm))
    assert none is None and torch.equal(h2.view(torch.int32), h.view(torch.int32)) and torch.equal(c2, counts)


# ---- flood_compare -----------------------------------------------------------------------------------------------------------
def _flood(dev, sel, ht, hp, stages):
    from tg_hip import ops as O
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    got = O.flood_compare(t(sel, np.uint8), t(ht, np.float32), t(hp, np.float32), stages).cpu().tolist()
    want = SO.flood_compare(sel, ht, hp, stages)
    assert len(got) == 30 and got[:len(want)] == want and not any(got[len(want):]), (got, want)
    return want


def test_flood_compare_every_counter(dev):
    nan = np.float32(np.nan)
    q = np.float32(1 / 1024)
    sel = np.array([[1, 1, 1, 1, 0, 1, 1, 1]], np.uint8)
    ht = np.array([[0, nan, 1, nan, 5, 2, 2, 0.5]], np.float32)
    hp = np.array([[1, 1, nan, nan, 7, 2 + 0.5 * q, 2 - 1.5 * q, 0.25]], np.float32)
    c = _flood(dev, sel, ht, hp, (0.5,))
    assert c == [4, 2, 2, 1024 + 2 + 256, 1024 - 2 - 256, int(np.float32(1.0).view(np.uint32)), 2, 1, 1]
    c = _flood(dev, sel, ht, hp, (0.25, 0.5, 1, 1.5, 2, 2.0000002, 3, 100))
    assert c[6:12] == [1, 1, 0, 2, 1, 1] and c[-3:] == [4, 4, 4]
    assert _flood(dev, np.zeros((1, 8), np.uint8), ht, hp, (1.0,)) == [0] * 9
    # more than one wave and block, not a multiple of either; every rounding case at random
    rng = np.random.default_rng(3)
    H, W = 9, 301
    ht = (rng.integers(0, 8192, (H, W)) / 1024 + rng.choice([0, 0.5, 0.25, 0.75], (H, W)) / 1024).astype(np.float32)
    hp = (rng.integers(0, 8192, (H, W)) / 1024 + rng.choice([0, 0.5, 0.25, 0.75], (H, W)) / 1024).astype(np.float32)
    ht[rng.random((H, W)) < 0.1] = nan
    hp[rng.random((H, W)) < 0.1] = nan
    sel = (rng.random((H, W)) < 0.8).astype(np.uint8)
    c = _flood(dev, sel, ht, hp, (0.5, 1.0, 2.0, 5.0))
    assert c[0] > 1500 and c[1] > 100 and c[2] > 100 and c[3] > abs(c[4]) > 0 and all(v > 0 for v in c[6:])
    c = _flood(dev, sel, hp, ht, (0.5, 1.0, 2.0, 5.0, 7.5))
    assert c[4] != 0 and len(c) == 6 + 15
    from tg_hip import lib as L
    from tg_hip import ops as O
    with pytest.raises(L.TgError, match="stages"):
        O.flood_compare(torch.zeros(2, 2, dtype=torch.uint8, device=dev), torch.zeros(2, 2, device=dev), torch.zeros(2, 2, device=dev),
                        (1.0, 1.0))


def test_flood_compare_sums_above_32_bits(dev):
    H = W = 300
    sel = np.ones((H, W), np.uint8)
    ht = np.zeros((H, W), np.float32)
    hp = np.full((H, W), 4000.0, np.float32)
    c = _flood(dev, sel, ht, hp, (1.0, 4000.0))
    assert c[3] == c[4] == H * W * 4000 * 1024 > 2 ** 32 and c[6:] == [H * W, 0, 0, H * W, H * W, H * W]
    c = _flood(dev, sel, hp, ht, (1.0,))
    assert c[3] == H * W * 4000 * 1024 and c[4] == -c[3] and c[5] == int(np.float32(4000).view(np.uint32))


# ---- flood_errors ------------------------------------------------------------------------------------------------------------
def _scene_ref():
    if "scene" not in _REF:
        z, pred, holes = DR.scene()
        _REF["scene"] = (z, pred, holes) + SO.flood(z, pred, holes, DR.CELLSIZE, DR.STREAM_CELLS, STAGES)
    return _REF["scene"]


def test_flood_errors_against_the_oracle(dev):
    from mvp_gan.src.evaluate_raster import flood_errors, flood_raw, flood_summary
    from tests.test_streams_cpu import edge_selection
    z, pred, holes, c, rep, sides = _scene_ref()
    kw = dict(cellsize=DR.CELLSIZE, stream_cells=DR.STREAM_CELLS, stages_m=STAGES)
    counts, stages, got_sides = flood_raw(z, pred, holes, **kw)
    assert stages == STAGES and counts[:len(c)] == c and not any(counts[len(c):])
    for g, s in zip(got_sides, sides):
        assert g == {"drained": s["h"]["drained"], "undrained": s["h"]["undrained"], "stream_cells": s["h"]["stream_cells"],
                     "max_hand_m": s["h"]["max_hand"], "rounds": s["h"]["rounds"]}
    d = flood_errors(z, pred, holes, **kw)
    print(json.dumps(d))
    assert d == rep                                                         # every derived number with ==
    assert d["cells"] == 10200 and d["undrained_truth"] == d["undrained_pred"] == 0
    assert d == flood_errors(torch.from_numpy(z).to(dev), torch.from_numpy(pred).to(dev), torch.from_numpy(holes).to(dev), **kw)
    assert "flood: HAND MAE" in flood_summary(d)
    # a selection with undrained pixels on both sides
    sel = edge_selection()
    c2 = SO.flood_compare(sel, sides[0]["h"]["hand"], sides[1]["h"]["hand"], STAGES)
    d2 = flood_errors(z, pred, sel, **kw)
    assert d2 == SO.flood_report(c2, STAGES, DR.STREAM_CELLS) and (d2["cells"], d2["undrained_truth"], d2["undrained_pred"]) == (3462, 1146, 1146)
    # other stages and another threshold
    c3, rep3, _ = SO.flood(z, pred, holes, DR.CELLSIZE, 400, (0.1, 3.0))
    assert flood_errors(z, pred, holes, cellsize=DR.CELLSIZE, stream_cells=400, stages_m=(0.1, 3.0)) == rep3


def test_flood_errors_identity_and_nan(dev):
    from mvp_gan.src.evaluate_raster import flood_errors
    z, pred, holes, c, rep, sides = _scene_ref()
    kw = dict(cellsize=DR.CELLSIZE, stream_cells=DR.STREAM_CELLS, stages_m=STAGES)
    d = flood_errors(z, z.copy(), holes, **kw)
    assert d["hand"] == {"mae_m": 0.0, "bias_m": 0.0, "max_m": 0.0} and d["cells"] == 10200
    for s in d["stages"]:
        assert s["csi"] == s["precision"] == s["recall"] == 1.0 and s["truth_cells"] == s["pred_cells"] == s["both_cells"] > 0
    # a fill that left pixels out: unknown on both sides.  The block lies on a summit, so no path ends at the void's rim
    nanp = pred.copy()
    nanp[92:95, 175:179] = np.nan
    d = flood_errors(z, nanp, holes, **kw)
    assert d == SO.flood(z, nanp, holes, DR.CELLSIZE, DR.STREAM_CELLS, STAGES)[1]
    assert d["cells"] == 10200 - 12 and d["undrained_truth"] == d["undrained_pred"] == 12


def test_evaluate_raster_flood(dev):
    """End to end on the small scene of tests/test_hip_drainage.py: the GAN, the harmonic baseline and the IDW fill, each with its
    flood entry, equal to a direct flood_errors call on that fill; without the option the report is what it was."""
    from mvp_gan.src.evaluate_raster import eval_holes, evaluate_raster, flood_errors, flood_summary
    from mvp_gan.src.fill_voids import fill_voids
    from mvp_gan.src.interpolate import interpolate_voids
    from mvp_gan.src.models import PConvUNet
    from tests.test_hip_terrain_eval import _terrain
    torch.manual_seed(7)
    G = PConvUNet().to(dev)
    H, W, c = 400, 520, 2.0
    z = _terrain(H, W, c, 8)
    kw = dict(cellsize=c, block=160, tile=80, window=128, overlap=16, baseline="laplace", compare=("idw",))
    fk = dict(stream_cells=200, stages_m=(0.5, 1.0, 3.0))
    rep, pred = evaluate_raster(G, z, flood=True, stream_cells=200, flood_stages_m=(0.5, 1.0, 3.0), **kw)
    before = pred.clone()
    plain, pred0 = evaluate_raster(G, z, **kw)                                # the parent's call
    assert torch.equal(pred, pred0)

    def strip(r):
        return {k: (strip(v) if isinstance(v, dict) and k in ("baseline", "compare", "idw") else v) for k, v in r.items()
                if k != "flood"}
    assert "flood" not in plain and "flood" not in plain["baseline"] and "flood" not in plain["compare"]["idw"]
    assert json.dumps(strip(rep)) == json.dumps(plain) and set(rep) - set(plain) == {"flood"}
    zt = torch.from_numpy(z).to(dev)
    hm, keep, _ = eval_holes(zt, None, split="test", block=160, tile=80, cellsize=c)
    assert json.dumps(rep["flood"]) == json.dumps(flood_errors(zt, pred, hm, cellsize=c, **fk))
    bpred, _ = fill_voids(zt, keep, method="laplace")
    assert json.dumps(rep["baseline"]["flood"]) == json.dumps(flood_errors(zt, bpred, hm, cellsize=c, **fk))
    ipred, _ = interpolate_voids(zt, keep, method="idw", cellsize=c)
    assert json.dumps(rep["compare"]["idw"]["flood"]) == json.dumps(flood_errors(zt, ipred, hm, cellsize=c, **fk))
    assert torch.equal(pred, before)                                           # pred is unchanged
    sides = [rep["flood"], rep["baseline"]["flood"], rep["compare"]["idw"]["flood"]]
    for s in sides:
        assert s["stream_cells"] == 200 and [g["stage_m"] for g in s["stages"]] == [0.5, 1.0, 3.0] and s["cells"] > 0
        assert "flood:" in flood_summary(s)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------
def test_cli(dev, tmp_path):
    from mvp_gan.src.asc import read_asc
    from tests.test_hip_terrain_eval import _write_asc
    z, _ = _voids()
    z[np.isnan(z)] = -9999.0
    dem, dout, aout, oout, lout, hout, hdout = (str(tmp_path / n) for n in ("dem.asc", "d.asc", "a.asc", "o.asc", "l.asc", "h.asc",
                                                                             "hd.asc"))
    _write_asc(dem, z, 0.5, -9999)
    zr, _ = read_asc(dem)
    r = FO.route(zr, None, -9999.0, True)
    net = SO.network_kahn(r["dir"], r["acc"], 5)
    inf = SO.info(net, 0.5)
    want = SO.hand(r["w"], r["dir"], SO.drainage_mask(r["dir"], r["acc"], 5, 2), 0.5)
    p = subprocess.run([sys.executable, "-m", "mvp_gan.src.flow_routing", "--dem", dem, "--dir-out", dout, "--acc-out", aout,
                        "--min-cells", "5", "--order-out", oout, "--links-out", lout, "--hand-out", hout, "--hand-distance-out",
                        hdout, "--min-order", "2"],
                       cwd=os.path.join(ROOT, "terra-gan_amd"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert f"{inf['stream_cells']} stream cells in {inf['links']} links ({inf['heads']} heads, {inf['junctions']} junctions, " \
           f"{inf['outlets']} outlets), largest Strahler order {inf['max_order']}, longest link {inf['longest_link_m']:.9g} m" in p.stdout
    assert f"{want['drained']} cells drain to {want['stream_cells']} drainage cells (order >= 2), {want['undrained']} do not; " \
           f"largest height above drainage {want['max_hand']:.9g} m" in p.stdout
    got, hdr = read_asc(oout)
    np.testing.assert_array_equal(got, net["order"].astype(np.float32))
    assert "NODATA_value" not in dict(hdr) and dict(hdr)["cellsize"] == "0.5"
    got, _ = read_asc(lout)
    np.testing.assert_array_equal(got, net["link"].astype(np.float32))
    for path, plane in ((hout, want["hand"]), (hdout, want["distance"])):
        got, hdr = read_asc(path)
        assert dict(hdr)["NODATA_value"] == "-9999"
        np.testing.assert_array_equal(_bits(got), _bits(np.where(np.isnan(plane), np.float32(-9999), plane)))   # full precision
    assert np.isnan(want["hand"]).sum() > 100 and len(np.unique(want["hand"])) > 5
