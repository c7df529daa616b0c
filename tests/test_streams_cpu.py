"""CPU checks of the stream network, the height above the nearest drainage and the flood comparison (csrc/drainage.hip,
mvp_gan/src/flow_routing.py stream_network and hand, mvp_gan/src/evaluate_raster.py flood_errors): the two
forms of class, link and order in tests/streams_oracle.py against each other and against hand-made grids, the comb that makes the
order travel, the properties of HAND, the flood counters and the report assembly on hand-made numbers, the conditions the GPU scene
must meet, host-side rejection by the five C entry points, the ops and the Python API, and the CLI parsers, all without a GPU.
Every comparison is exact."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

from tests import drainage_oracle as DR
from tests import flow_oracle as FO
from tests import streams_oracle as SO
from tests.test_flow_cpu import _rasters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tg_stream_class", "tg_stream_order", "tg_stream_order_finish", "tg_hand", "tg_flood_compare")
KEYS = ("cls", "link", "nc", "nd", "order")
PITS = ((63, 127, 1), (64, 128, 2), (65, 130, 3), (129, 130, 4), (129, 127, 5))        # H, W, seed
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def contract():
    """The oracle implements what include/terragan_hip.h states."""
    txt = " ".join(open(os.path.join(ROOT, "include", "terragan_hip.h")).read().replace("* ", "").split())
    for name in NAMES:
        assert name + "(" in txt, name
    for name, v in (("TG_STREAM_HEAD", SO.HEAD), ("TG_STREAM_INTERIOR", SO.INTERIOR), ("TG_STREAM_JUNCTION", SO.JUNCTION),
                    ("TG_STREAM_ORDER_BINS", SO.NBINS), ("TG_FLOOD_MAX_STAGES", 8)):
        assert f"#define {name} {v} " in txt, name
    assert "#define TG_FLOOD_COUNTS (6 + 3 TG_FLOOD_MAX_STAGES)" in txt
    assert "max(m1, m2 + 1)" in txt and "rint((double)|hp - ht| 1024)" in txt
    return txt


def _both(code, acc, min_cells):
    a, b = SO.network_kahn(code, acc, min_cells), SO.network_links(code, acc, min_cells)
    for k in KEYS + ("cells", "heads", "junctions", "outlets"):
        assert np.array_equal(a[k], b[k]), k
    S = (code != 0) & (acc >= min_cells)
    assert a["cells"] == int(S.sum()) and ((a["cls"] != 0) == S).all() and ((a["order"] > 0) == S).all()
    assert ((a["link"] >= 0) == S).all()
    top = a["link"][S]
    assert np.isin(a["cls"].ravel()[top], (SO.HEAD, SO.JUNCTION)).all()                 # a link starts at a head or a junction
    assert (a["order"][S] == a["order"].ravel()[top]).all()                             # the order is constant along a link
    lk = np.isin(a["cls"], (SO.HEAD, SO.JUNCTION))
    assert (a["link"][lk] == np.flatnonzero(lk.ravel())).all() and not a["nc"][lk].any() and not a["nd"][lk].any()
    return a, b


def _pits(H, W, seed):
    key = ("pits", H, W, seed)
    if key not in _REF:
        _REF[key] = FO.route(FO.rounded_pits(H, W, seed))
    return _REF[key]


# ---- class, link, order ----------------------------------------------------------------------------------------------------
def test_two_forms_agree_on_random_rasters():
    n = junctions = 0
    for z in _rasters():
        r = FO.route(z)
        for mc in (1, 4, 20):
            a, _ = _both(r["dir"], r["acc"], mc)
            n += 1
            junctions += a["junctions"]
            if mc == 1:
                assert a["cells"] == int(r["known"].sum()) and a["outlets"] == int(np.isin(r["dir"], (FO.OUT, FO.PIT)).sum())
    assert n == 123 and junctions > 1000


@pytest.mark.parametrize("H,W,seed", PITS)
def test_two_forms_agree_on_rounded_pits(H, W, seed):
    r = _pits(H, W, seed)
    for mc in (1, 4, 20):
        a, b = _both(r["dir"], r["acc"], mc)
        if mc == 1:
            assert a["order"].max() >= 5 and a["junctions"] > 2000, (a["order"].max(), a["junctions"])
            assert b["order_rounds"] > 8
    # an accumulation that does not belong to the grid: the definitions hold for any pair
    rng = np.random.default_rng(seed)
    acc = rng.integers(0, 6, r["acc"].shape).astype(np.int32)
    a, _ = _both(r["dir"], acc, 3)
    assert a["outlets"] > int(np.isin(r["dir"], (FO.OUT, FO.PIT)).sum())              # streams that end in mid-slope


def _order_of(rows, at, min_cells=1):
    code = SO.grid(rows)
    acc, _ = FO.accumulate_kahn(code)
    a, _ = _both(code, acc, min_cells)
    return a["order"][at], a


def test_hand_made_grids():
    # a Y: two heads meet, 1 + 1 -> 2
    o, a = _order_of(["2.4", ".3.", ".o."], (1, 1))
    assert o == 2 and a["order"].tolist() == [[1, 0, 1], [0, 2, 0], [0, 2, 0]] and a["cls"].tolist() == [[1, 0, 1], [0, 3, 0], [0, 2, 0]]
    assert a["link"].tolist() == [[0, -1, 2], [-1, 4, -1], [-1, 4, -1]] and a["nc"][2, 1] == 1 and (a["heads"], a["junctions"]) == (2, 1)
    assert a["outlets"] == 1
    # three heads into one pixel -> 2
    o, a = _order_of(["234", ".o."], (1, 1))
    assert o == 2 and a["cls"][1, 1] == SO.JUNCTION
    # (2, 1, 1) -> 2: a Y whose stem meets two more heads
    rows = ["2.4..",
            ".3...",
            ".3...",
            "1o5.."]
    o, a = _order_of(rows, (3, 1))
    assert a["order"][2, 1] == 2 and o == 2
    # (2, 2, 1) -> 3: two Ys and a head
    rows = ["2.4.2.4",
            ".3...3.",
            ".2.3.4.",                                                              # (2, 3): a head N of the meeting pixel
            "..1o5..",
            "......."]
    code = SO.grid(rows)
    acc, _ = FO.accumulate_kahn(code)
    a, _ = _both(code, acc, 1)
    assert a["order"][3, 2] == 2 and a["order"][3, 4] == 2 and a["order"][2, 3] == 1 and a["order"][3, 3] == 3
    assert SO.order_counts(a)[0] == 3
    # min_cells cuts the heads off: the Y's stem alone is a head of its own
    o, a = _order_of(["2.4", ".3.", ".o."], (1, 1), min_cells=3)
    assert o == 1 and a["cells"] == 2 and a["heads"] == 1 and a["link"][2, 1] == 4 and a["nc"][2, 1] == 1
    # diagonal steps are counted apart
    code = SO.grid(["2...", ".2..", "..2.", "...o"])
    acc, _ = FO.accumulate_kahn(code)
    a, _ = _both(code, acc, 1)
    assert a["nd"][3, 3] == 3 and a["nc"][3, 3] == 0 and a["link"][3, 3] == 0
    assert SO.info(a, 2.0)["longest_link_m"] == float(np.float32(2.0 * 3 * DR.SQRT2))


def test_comb_makes_the_order_travel():
    code, acc = SO.comb()
    a, b = _both(code, acc, 1)
    assert a["junctions"] == 132 and a["heads"] == 4 + 129 and a["outlets"] == 1
    assert (a["order"][2, 4:] == 3).all() and a["order"][1, 3] == a["order"][3, 3] == 2 and (a["order"][1, 6:-1:2] == 1).all()
    assert b["order_rounds"] == 132 > 64
    # stopped early every value is a lower bound, at least 1 on the streams
    part = SO.network_links(code, acc, 1, max_rounds=2)
    S = a["order"] > 0
    assert (part["order"] <= a["order"]).all() and (part["order"][S] >= 1).all() and (part["order"] < a["order"]).any()


# ---- HAND ------------------------------------------------------------------------------------------------------------------
def test_hand_properties():
    for H, W, seed in PITS[:3]:
        r = _pits(H, W, seed)
        for mc, mo in ((20, 1), (4, 1), (4, 2)):
            stream = SO.drainage_mask(r["dir"], r["acc"], mc, mo)
            h = SO.hand(r["w"], r["dir"], stream, 2.0)
            hh, known = h["hand"], r["dir"] != 0
            fin = ~np.isnan(hh)
            assert (hh[fin] >= 0).all() and (hh[stream != 0] == 0).all() and fin[stream != 0].all()
            assert h["drained"] == int(fin.sum()) and h["drained"] + h["undrained"] == int(known.sum())
            assert (np.isnan(h["distance"]) == ~fin).all() and (h["distance"][stream != 0] == 0).all()
            # undrained exactly where the path ends off the drainage
            T = DR.watersheds(r["dir"])["T"]
            ends_on = known & (stream.ravel()[np.where(known, T, 0)] != 0)
            reaches = known & (DR.watersheds(r["dir"], stream)["T"] != T)
            assert (fin == (ends_on | reaches | (stream != 0))).all()
            assert h["stream_cells"] == int(stream.sum())
        # min_order = 2 takes the order-1 links out of the drainage
        net = SO.network_kahn(r["dir"], r["acc"], 4)
        s1, s2 = SO.drainage_mask(r["dir"], r["acc"], 4, 1), SO.drainage_mask(r["dir"], r["acc"], 4, 2)
        assert ((s1 != 0) & (s2 == 0) == (net["order"] == 1)).all() and 0 < s2.sum() < s1.sum()
        h1, h2 = SO.hand(r["w"], r["dir"], s1)["hand"], SO.hand(r["w"], r["dir"], s2)["hand"]
        both = ~np.isnan(h1) & ~np.isnan(h2)
        assert (h2[both] >= h1[both]).all() and (h2[both] > h1[both]).any() and np.isnan(h2).sum() >= np.isnan(h1).sum()
    # a pit that is no stream: nothing drains
    pit = np.array([[1003, 1002, 1004], [1001, 990, 1005], [1006, 1002.5, 1007]], np.float32)
    r = FO.route(pit, fill=False)
    h = SO.hand(r["w"], r["dir"], SO.drainage_mask(r["dir"], r["acc"], 10))
    assert np.isnan(h["hand"]).all() and (h["drained"], h["undrained"], h["stream_cells"]) == (0, 9, 0)
    h = SO.hand(r["w"], r["dir"], SO.drainage_mask(r["dir"], r["acc"], 9))
    assert h["hand"][1, 1] == 0 and h["hand"][0, 0] == np.float32(13) and h["drained"] == 9 and h["max_hand"] == 17.0


# ---- the flood counters ----------------------------------------------------------------------------------------------------
def test_flood_counters_by_hand():
    nan = np.float32(np.nan)
    q = np.float32(1 / 1024)
    sel = np.array([[1, 1, 1, 1, 0, 1, 1, 1]], np.uint8)
    ht = np.array([[0, nan, 1, nan, 5, 2, 2, 0.5]], np.float32)
    hp = np.array([[1, 1, nan, nan, 7, 2 + 0.5 * q, 2 - 1.5 * q, 0.25]], np.float32)
    c = SO.flood_compare(sel, ht, hp, (0.5,))
    # cells: columns 0, 5, 6, 7; the ties round to even: 0.5 -> 0, 1.5 -> 2
    assert c[:3] == [4, 2, 2]
    assert c[3] == 1024 + 0 + 2 + 256 and c[4] == 1024 + 0 - 2 - 256
    assert c[5] == int(np.float32(1.0).view(np.uint32))
    assert c[6:] == [2, 1, 1]                                                       # a stage equal to a hand value is wet (<=)
    c8 = SO.flood_compare(sel, ht, hp, (0.25, 0.5, 1, 1.5, 2, 2.0000002, 3, 100))
    assert len(c8) == 30 and c8[:6] == c[:6]
    assert [c8[6 + 3 * i:9 + 3 * i] for i in range(8)] == [[1, 1, 0], [2, 1, 1], [2, 2, 2], [2, 2, 2], [4, 3, 3], [4, 3, 3], [4, 4, 4],
                                                          [4, 4, 4]]
    assert SO.flood_compare(np.zeros((1, 8), np.uint8), ht, hp, (1.0,)) == [0] * 9
    rep = SO.flood_report(SO.flood_compare(np.zeros((1, 8), np.uint8), ht, hp, (1.0,)), (1.0,), 7)
    assert rep["hand"] == {"mae_m": None, "bias_m": None, "max_m": None} and rep["stages"][0]["csi"] is None


def test_assemble_flood():
    from mvp_gan.src.evaluate_raster import assemble_flood, flood_summary
    bits = int(np.float32(9.75).view(np.uint32))
    c = [200, 3, 4, 200 * 1024 + 512, -100 * 1024, bits, 50, 40, 30, 120, 100, 90] + [0] * 18
    d = assemble_flood(c, (0.5, 2.0), stream_cells=100)
    assert d == {"cells": 200, "stream_cells": 100, "undrained_truth": 3, "undrained_pred": 4,
                 "hand": {"mae_m": 200.5 / 200, "bias_m": -0.5, "max_m": 9.75},
                 "stages": [{"stage_m": 0.5, "truth_cells": 50, "pred_cells": 40, "both_cells": 30, "csi": 0.5, "precision": 0.75,
                             "recall": 0.6},
                            {"stage_m": 2.0, "truth_cells": 120, "pred_cells": 100, "both_cells": 90, "csi": 90 / 130,
                             "precision": 0.9, "recall": 0.75}]}
    assert d == SO.flood_report(c, (0.5, 2.0), 100)
    line = flood_summary(d)
    assert "HAND MAE 1.002 m" in line and "0.5 m 0.500" in line and "2 m 0.692" in line and "over 200 px" in line
    # zero denominators
    z = assemble_flood([0] * 30, (1.0,), stream_cells=5)
    assert z["hand"] == {"mae_m": None, "bias_m": None, "max_m": None}
    assert z["stages"] == [{"stage_m": 1.0, "truth_cells": 0, "pred_cells": 0, "both_cells": 0, "csi": None, "precision": None,
                            "recall": None}]
    assert "n/a" in flood_summary(z)
    z = assemble_flood([5, 0, 0, 0, 0, 0, 0, 3, 0], (1.0,), stream_cells=5)
    assert z["stages"][0]["csi"] == 0.0 and z["stages"][0]["recall"] is None and z["hand"]["mae_m"] == 0.0
    with pytest.raises(ValueError, match="counters"):
        assemble_flood([0] * 8, (1.0,), stream_cells=5)


# ---- the scene of the GPU tests ------------------------------------------------------------------------------------------------
STAGES = (0.25, 0.5, 1.0, 2.0)


def scene_ref():
    if "scene" not in _REF:
        z, pred, holes = DR.scene()
        _REF["scene"] = (z, pred, holes) + SO.flood(z, pred, holes, DR.CELLSIZE, DR.STREAM_CELLS, STAGES)
    return _REF["scene"]


def edge_selection():
    """A selection that takes in raster-edge rows, where paths leave the raster before they meet a stream."""
    sel = np.zeros((192, 192), np.uint8)
    sel[:12, :] = 1
    sel[-12:, :] = 1
    return sel


def test_scene_conditions():
    z, pred, holes, c, rep, sides = scene_ref()
    assert c[:3] == [10200, 0, 0] and int(holes.sum()) == 10200                       # every hole pixel drained on both sides
    # every extent, the truth's and the fill's at every stage, wets at least 500 pixels (their overlap at the lowest stage is
    # smaller: that is what a CSI of 0.12 says)
    assert len(c) == 6 + 12 and min(min(c[6 + 3 * i], c[7 + 3 * i]) for i in range(4)) >= 500 and min(c[8::3]) > 0
    for s in rep["stages"]:
        assert 0.05 < s["csi"] < 0.95, s
    assert rep["hand"]["mae_m"] > 0.1 and rep["hand"]["max_m"] > 1.0
    # the second selection: undrained pixels on both sides
    t, p = sides[0]["h"], sides[1]["h"]
    assert t["undrained"] == 1979 and t["drained"] + t["undrained"] == 36864
    sel = edge_selection()
    c2 = SO.flood_compare(sel, t["hand"], p["hand"], STAGES)
    assert int(sel.sum()) == 24 * 192 and c2[:3] == [3462, 1146, 1146] and c2[1] >= 100 and c2[2] >= 100
    assert (c2[1], c2[2]) == (int((np.isnan(t["hand"]) & (sel != 0)).sum()), int((np.isnan(p["hand"]) & (sel != 0)).sum()))


# ---- rejections and plumbing -----------------------------------------------------------------------------------------------
def _lib():
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    return L, L.load()


def test_c_entry_points_reject_without_gpu():
    L, lib = _lib()
    f = [C.c_void_p(0x1000 * (i + 1)) for i in range(16)]
    big = 1 << 40
    stages = lambda *v: L.TgFloodStages((C.c_float * 8)(*v))

    def err(rc, msg):
        assert rc == -1 and msg in lib.tg_last_error(), (rc, lib.tg_last_error())

    cls_ = lambda H, W, mc=1, d=f[0], acc=f[1], cl=f[2], o=f[3], cnt=f[4], ws=f[5], nb=big: \
        lib.tg_stream_class(d, acc, H, W, mc, cl, o, cnt, ws, nb, None)
    ordr = lambda H, W, nj=1, n=1, d=f[0], cl=f[2], top=f[6], j=f[7], o=f[3], ch=f[8]: \
        lib.tg_stream_order(d, cl, top, j, nj, H, W, n, o, ch, None)
    fin = lambda H, W, cl=f[2], top=f[6], o=f[3], out=f[9], cnt=f[4]: lib.tg_stream_order_finish(cl, top, o, H, W, out, cnt, None)
    hand = lambda H, W, w=f[0], b=f[1], s=f[2], ln=None, h=f[3], dist=None, cnt=f[4]: lib.tg_hand(w, b, s, ln, H, W, h, dist, cnt, None)
    fld = lambda H, W, st=stages(0.5, 1.0), k=2, sel=f[0], ht=f[1], hp=f[2], cnt=f[4]: lib.tg_flood_compare(sel, ht, hp, H, W, st, k, cnt, None)
    for H, W in ((0, 5), (5, 0), (-1, 5), (5, -1), (1 << 16, 1 << 15), (1 << 30, 2)):
        for call in (cls_, ordr, fin, hand, fld):
            err(call(H, W), b"must be non-empty with H*W < 2^31")
    for kw in ({"d": None}, {"acc": None}, {"cl": None}, {"o": None}, {"cnt": None}, {"ws": None}):
        err(cls_(8, 8, **kw), b"null pointer")
    for kw in ({"d": None}, {"cl": None}, {"top": None}, {"o": None}, {"ch": None}):
        err(ordr(8, 8, **kw), b"null pointer")
    err(ordr(8, 8, j=None), b"null junction list")
    for kw in ({"cl": None}, {"top": None}, {"o": None}, {"out": None}, {"cnt": None}):
        err(fin(8, 8, **kw), b"null pointer")
    for kw in ({"w": None}, {"b": None}, {"s": None}, {"h": None}, {"cnt": None}):
        err(hand(8, 8, **kw), b"null pointer")
    for kw in ({"ln": f[5]}, {"dist": f[5]}):
        err(hand(8, 8, **kw), b"go together")
    for kw in ({"sel": None}, {"ht": None}, {"hp": None}, {"cnt": None}):
        err(fld(8, 8, **kw), b"null pointer")
    for mc in (0, -1, -(1 << 31)):
        err(cls_(8, 8, mc=mc), b"min_cells")
    for nj in (-1, 65):
        err(ordr(8, 8, nj=nj), b"nj")
    for n in (0, -1, (1 << 20) + 1):
        err(ordr(8, 8, n=n), b"n = ")
    for k in (0, -1, 9):
        err(fld(8, 8, k=k), b"stages must lie in [1, 8]")
    for st in (stages(0.0, 1.0), stages(-1.0, 1.0), stages(math.nan, 1.0), stages(0.5, math.inf)):
        err(fld(8, 8, st=st), b"finite and > 0")
    for st in (stages(1.0, 1.0), stages(1.0, 0.5)):
        err(fld(8, 8, st=st), b"strictly increasing")
    for H, W in ((8, 8), (129, 4097), (32767, 32767)):
        err(cls_(H, W, nb=lib.tg_flow_basin_ws_bytes(H, W) - 1), b"workspace")
    err(cls_(8, 8, ws=C.c_void_p(0x1008)), b"aligned")


def test_signatures_and_constants():
    from tg_hip import lib as L
    from tg_hip import ops as O
    P, I, SZ, I32 = C.c_void_p, C.c_int, C.c_size_t, C.c_int32
    assert L.SIGNATURES["tg_stream_class"] == (I, [P, P, I, I, I32, P, P, P, P, SZ, P])
    assert L.SIGNATURES["tg_stream_order"] == (I, [P, P, P, P, I, I, I, I, P, P, P])
    assert L.SIGNATURES["tg_stream_order_finish"] == (I, [P, P, P, I, I, P, P, P])
    assert L.SIGNATURES["tg_hand"] == (I, [P, P, P, P, I, I, P, P, P, P])
    assert L.SIGNATURES["tg_flood_compare"] == (I, [P, P, P, I, I, L.TgFloodStages, I, P, P])
    assert C.sizeof(L.TgFloodStages) == 32
    assert (L.TG_STREAM_ORDER_COUNTS, L.TG_FLOOD_COUNTS, L.TG_FLOOD_MAX_STAGES) == (31, 30, 8)
    assert (O.STREAM_HEAD, O.STREAM_INTERIOR, O.STREAM_JUNCTION) == (SO.HEAD, SO.INTERIOR, SO.JUNCTION)
    assert O.FLOOD_NAMES == SO.FLOOD_NAMES and O.STREAM_ORDER_BINS == SO.NBINS


def test_ops_reject_before_any_launch():
    import torch
    from tg_hip import lib as L
    from tg_hip import ops as O
    d = torch.zeros(4, 4, dtype=torch.uint8)
    i32 = torch.zeros(4, 4, dtype=torch.int32)
    f32 = torch.zeros(4, 4, dtype=torch.float32)
    ws = torch.zeros(4096, dtype=torch.uint8)
    ch = torch.zeros(1, dtype=torch.int32)
    for call in (lambda: O.stream_class(d, i32, 1, ws), lambda: O.stream_order(d, d, i32, ch, 1, i32, ch),
                 lambda: O.stream_order_finish(d, i32, i32), lambda: O.hand(f32, i32, d), lambda: O.flood_compare(d, f32, f32, (1.0,)),
                 lambda: O.stream_class(np.zeros((4, 4), np.uint8), i32, 1, ws)):
        with pytest.raises(L.TgError):
            call()
    for bad in ((), (1,) * 9, (0.0,), (-1.0, 1.0), (math.nan,), (math.inf,), (1e39,), (1.0, 1.0), (2.0, 1.0), (1.0, 1.0 + 1e-9),
                "ab", None, (True,)):
        with pytest.raises(L.TgError, match="stages"):
            O.flood_stages(bad)
    st, k = O.flood_stages((0.25, 0.5, 1, 2))
    assert k == 4 and list(st.s) == [0.25, 0.5, 1.0, 2.0, 0.0, 0.0, 0.0, 0.0]
    assert O.flood_stages(range(1, 9))[1] == 8


def test_python_rejects_bad_arguments():
    import torch
    from mvp_gan.src import evaluate_raster as ER
    from mvp_gan.src import flow_routing as FR
    d = np.ones((8, 8), np.uint8)
    a = np.ones((8, 8), np.int32)
    with pytest.raises(ValueError, match="H, W"):
        FR.stream_network(np.zeros((2, 3, 4), np.uint8), a, 1)
    with pytest.raises(ValueError, match="2\\^31"):
        FR.stream_network(np.broadcast_to(np.uint8(0), (1 << 16, 1 << 15)), a, 1)
    for bad in (d.astype(np.int32), torch.ones(8, 8, dtype=torch.int64), [[1, 2], [3, 4]]):
        with pytest.raises(ValueError, match="uint8"):
            FR.stream_network(bad, a, 1)
    with pytest.raises(ValueError, match="accumulation"):
        FR.stream_network(d, np.ones((8, 9), np.int32), 1)
    for bad in (a.astype(np.int64), a.astype(np.float32), torch.ones(8, 8, dtype=torch.int64)):
        with pytest.raises(ValueError, match="int32"):
            FR.stream_network(d, bad, 1)
    for n in (0, -1, 1.5, "3", None, True, 2 ** 31):
        with pytest.raises(ValueError, match="min_cells"):
            FR.stream_network(d, a, n)
        with pytest.raises(ValueError, match="min_cells"):
            FR.hand(np.zeros((8, 8), np.float32), min_cells=n)
    for c in (0.0, -1.0, math.nan, math.inf, None, "x"):
        with pytest.raises(ValueError, match="cellsize"):
            FR.stream_network(d, a, 1, cellsize=c)
    for n in (0, -1, 1.5, None, True, (1 << 20) + 1):
        with pytest.raises(ValueError, match="check_every"):
            FR.stream_network(d, a, 1, check_every=n)
        with pytest.raises(ValueError, match="max_rounds"):
            FR.stream_network(d, a, 1, max_rounds=n)
    for k in (0, -1, 1.5, None, True, 256):
        with pytest.raises(ValueError, match="min_order"):
            FR.hand(np.zeros((8, 8), np.float32), min_order=k)
    with pytest.raises(ValueError, match="fill"):
        FR.hand(np.zeros((8, 8), np.float32), fill=1)
    with pytest.raises(ValueError, match="H, W"):
        FR.hand(np.zeros((8,), np.float32))
    sig = inspect.signature(FR.stream_network).parameters
    assert list(sig)[:3] == ["direction", "accumulation", "min_cells"]
    assert [(k, sig[k].default, sig[k].kind) for k in list(sig)[3:]] == \
        [(k, v, inspect.Parameter.KEYWORD_ONLY) for k, v in (("cellsize", 1.0), ("max_rounds", 65536), ("check_every", 8))]
    sig = inspect.signature(FR.hand).parameters
    assert [(k, sig[k].default) for k in list(sig)[2:8]] == [("nodata", None), ("cellsize", 1.0), ("min_cells", 1000), ("min_order", 1),
                                                            ("fill", True), ("max_sweeps", 4096)]
    assert list(inspect.signature(FR.hand_from_routing).parameters)[:4] == ["w", "direction", "stream", "cellsize"]
    assert inspect.signature(FR.route_known).parameters["return_surface"].default is False
    # flood_errors and evaluate_raster
    z = np.zeros((8, 8), np.float32)
    with pytest.raises(ValueError, match="shape"):
        ER.flood_errors(z, np.zeros((8, 9), np.float32), z, cellsize=1.0)
    with pytest.raises(ValueError, match="cellsize"):
        ER.flood_errors(z, z, z, cellsize=0.0)
    for n in (0, 1.5, None, True, 2 ** 31):
        with pytest.raises(ValueError, match="stream_cells"):
            ER.flood_errors(z, z, z, cellsize=1.0, stream_cells=n)
    for bad in ((), (1,) * 9, (0.0,), (-1.0, 1.0), (math.nan,), (math.inf,), (1.0, 1.0), (2.0, 1.0), (1.0, 1.0 + 1e-9), None, 3.0):
        with pytest.raises(ValueError, match="flood stages"):
            ER.flood_errors(z, z, z, cellsize=1.0, stages_m=bad)
        with pytest.raises(ValueError, match="flood stages"):
            ER.evaluate_raster(None, z, cellsize=1.0, flood=True, flood_stages_m=bad)
    assert ER.check_flood_stages((0.1, 1, 2)) == (float(np.float32(0.1)), 1.0, 2.0)
    sig = inspect.signature(ER.flood_errors).parameters
    assert [(k, sig[k].default) for k in list(sig)[3:]] == [("cellsize", inspect.Parameter.empty), ("mask", None), ("nodata", None),
                                                            ("stream_cells", 1000), ("stages_m", (0.5, 1.0, 2.0, 5.0))]
    for fn in (ER.evaluate_raster, ER.baseline_report, ER.compare_report):
        sig = inspect.signature(fn).parameters
        assert (sig["flood"].default, sig["flood_stages_m"].default) == (False, (0.5, 1.0, 2.0, 5.0))


def test_no_cpu_path(monkeypatch):
    import torch
    from mvp_gan.src.evaluate_raster import flood_errors
    from mvp_gan.src.flow_routing import hand, stream_network
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        stream_network(np.ones((8, 8), np.uint8), np.ones((8, 8), np.int32), 1)
    z = np.zeros((8, 8), np.float32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hand(z)
    with pytest.raises(RuntimeError, match="no HIP device|no CPU path"):
        flood_errors(z, z, z, cellsize=1.0)


def test_compare_report_assembly_threads_flood():
    from mvp_gan.src.evaluate_raster import assemble_compare
    raw = {"idw": {"height": 1}, "nearest": {"height": 2}}
    infos = {"idw": {"a": 1}, "nearest": {"a": 2}}
    cmp = assemble_compare(raw, infos)
    assert all("flood" not in cmp[k] and set(cmp[k]) == {"height", "method", "fill"} for k in cmp)
    a, b = {"cells": 1}, {"cells": 2}
    cmp = assemble_compare(raw, infos, None, None, {"idw": a, "nearest": b})
    assert cmp["idw"]["flood"] is a and cmp["nearest"]["flood"] is b and "drainage" not in cmp["idw"] and "flood" not in raw["idw"]


def test_cli_parsers():
    from mvp_gan.src.evaluate_raster import build_parser as eval_parser
    from mvp_gan.src.evaluate_raster import main as eval_main
    from mvp_gan.src.flow_routing import parse_args
    base = ["--dem", "in.asc", "--dir-out", "d.asc", "--acc-out", "a.asc"]
    a = parse_args(base)
    assert (a.order_out, a.links_out, a.hand_out, a.hand_distance_out, a.min_order, a.min_cells) == (None, None, None, None, 1, None)
    a = parse_args(base + ["--order-out", "o.asc", "--links-out", "l.asc", "--min-cells", "50"])
    assert (a.order_out, a.links_out, a.hand_out, a.min_cells) == ("o.asc", "l.asc", None, 50)
    a = parse_args(base + ["--hand-out", "h.asc", "--hand-distance-out", "hd.asc", "--min-order", "2", "--min-cells", "50",
                           "--streams-out", "s.asc"])
    assert (a.hand_out, a.hand_distance_out, a.min_order, a.streams_out) == ("h.asc", "hd.asc", 2, "s.asc")
    for bad in (base + ["--order-out", "o.asc"], base + ["--links-out", "l.asc"], base + ["--hand-out", "h.asc"],
                base + ["--min-cells", "5"], base + ["--hand-distance-out", "hd.asc", "--order-out", "o.asc", "--min-cells", "5"],
                base + ["--min-order", "2", "--order-out", "o.asc", "--min-cells", "5"],
                base + ["--hand-out", "h.asc", "--min-cells", "5", "--min-order", "0"],
                base + ["--hand-out", "h.asc", "--min-cells", "0"], base + ["--hand-out", "h.asc", "--min-cells", "5", "--min-order", "x"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
    ebase = ["--dem", "in.asc", "--checkpoint", "g.pth"]
    a = eval_parser().parse_args(ebase)
    assert a.flood is False and a.flood_stages == [0.5, 1.0, 2.0, 5.0]
    a = eval_parser().parse_args(ebase + ["--flood", "--flood-stages", "0.25", "1", "--stream-cells", "250"])
    assert (a.flood, a.flood_stages, a.stream_cells) == (True, [0.25, 1.0], 250)
    for bad in (ebase + ["--flood", "yes"], ebase + ["--flood-stages"], ebase + ["--flood-stages", "x"]):
        with pytest.raises(SystemExit):
            eval_parser().parse_args(bad)
    for bad in (["--flood-stages", "2", "1"], ["--flood-stages", "0"], ["--flood-stages"] + ["1"] * 9):
        with pytest.raises(SystemExit):
            eval_main(ebase + ["--flood"] + bad)
