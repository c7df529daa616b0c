"""CPU oracle of the stream classes, links and Strahler orders, the height above the nearest drainage and the flood comparison
(csrc/drainage.hip, mvp_gan/src/flow_routing.py stream_network and hand, mvp_gan/src/evaluate_raster.py flood_errors, DESIGN.md
section 8x), numpy only.

For a direction grid of tests/flow_oracle.py (without UNDECIDED), an accumulation plane and min_cells: a stream pixel has a
direction and accumulation >= min_cells; a stream donor of p is a stream pixel with a code 1..8 whose receiver is p.  Class, link
and order come in two independent forms: along Kahn's topological order of the stream pixels, and the link-top form of the GPU (the
`up` pointer doubling, then a synchronous iteration over the junctions).  HAND goes through tests/drainage_oracle.py's watersheds
with the drainage mask as pour points."""
from collections import deque

import numpy as np

from tests import depfill_oracle as DO
from tests import drainage_oracle as DR
from tests import flow_oracle as FO

HEAD, INTERIOR, JUNCTION = 1, 2, 3
NBINS = 15
FLOOD_NAMES = ("cells", "undrained_t", "undrained_p", "abs_q10", "bias_q10", "abs_max_bits")


def receivers(code):
    """-> next int64 [H * W]: the receiver's linear index for the codes 1..8 when it lies inside the raster, else -1."""
    H, W = code.shape
    y, x = np.mgrid[0:H, 0:W]
    nxt = np.full((H, W), -1, np.int64)
    for c in range(1, 9):
        yy, xx = y + FO.DY[c - 1], x + FO.DX[c - 1]
        sel = (code == c) & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        nxt[sel] = yy[sel] * W + xx[sel]
    return nxt.ravel()


def _graph(code, acc, min_cells):
    """-> (S bool [n], nxt, don bool [n]: stream pixels with a receiver, sd int64 [n], cls uint8 [n], terminal bool [n])."""
    nxt = receivers(code)
    S = ((code != 0) & (acc >= min_cells)).ravel()
    don = S & (nxt >= 0)
    sd = np.bincount(nxt[don], minlength=S.size)
    cls = np.where(S, np.where(sd == 0, HEAD, np.where(sd == 1, INTERIOR, JUNCTION)), 0).astype(np.uint8)
    to_stream = np.zeros(S.size, bool)
    to_stream[don] = S[nxt[don]]
    return S, nxt, don, sd, cls, S & ~to_stream


def _strahler(m1, m2):
    return max(m1, m2 + 1)


def network_kahn(code, acc, min_cells):
    """Class, link, steps and order along Kahn's order of the stream pixels: a pixel is taken once all its stream donors are done.
    -> dict(cls uint8, link int64 (-1 off the streams), nc, nd int64, order int64 [H][W], cells, heads, junctions, outlets)"""
    S, nxt, don, sd, cls, term = _graph(code, acc, min_cells)
    n = S.size
    c = code.ravel().astype(np.int64)
    indeg = np.where(S, sd, 0).astype(np.int64)
    m1, m2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    link = np.full(n, -1, np.int64)
    nc, nd = np.zeros(n, np.int64), np.zeros(n, np.int64)
    order = np.zeros(n, np.int64)
    q = deque(np.nonzero(cls == HEAD)[0].tolist())
    seen = 0
    while q:
        p = q.popleft()
        seen += 1
        if cls[p] == HEAD:
            order[p], link[p] = 1, p
        elif cls[p] == JUNCTION:
            order[p], link[p], nc[p], nd[p] = _strahler(m1[p], m2[p]), p, 0, 0
        else:
            order[p] = m1[p]                                        # link, nc, nd were set by the one donor
        r = nxt[p]
        if r >= 0 and S[r]:
            o = order[p]
            if o > m1[r]:
                m1[r], m2[r] = o, m1[r]
            elif o > m2[r]:
                m2[r] = o
            if cls[r] == INTERIOR:
                card = c[p] % 2 == 1
                link[r], nc[r], nd[r] = link[p], nc[p] + int(card), nd[p] + int(not card)
            indeg[r] -= 1
            if indeg[r] == 0:
                q.append(int(r))
    assert seen == int(S.sum()), "the stream pixels have a cycle"
    s = code.shape
    return {"cls": cls.reshape(s), "link": link.reshape(s), "nc": nc.reshape(s), "nd": nd.reshape(s), "order": order.reshape(s),
            "cells": int(S.sum()), "heads": int((cls == HEAD).sum()), "junctions": int((cls == JUNCTION).sum()),
            "outlets": int(term.sum())}


def link_doubling(code, acc, min_cells):
    """The `up` doubling of the GPU: records (next, last, nc, nd) with the start (up, p, c, d), (c, d) from the donor's code.
    -> (top, nc, nd int64 [n], rounds)"""
    S, nxt, don, sd, cls, _ = _graph(code, acc, min_cells)
    n = S.size
    c = code.ravel().astype(np.int64)
    up = np.full(n, -1, np.int64)
    into = don & (cls[np.where(nxt >= 0, nxt, 0)] == INTERIOR)
    up[nxt[into]] = np.nonzero(into)[0]
    last = np.where(S, np.arange(n, dtype=np.int64), -1)
    card = (up >= 0) & (c[np.where(up >= 0, up, 0)] % 2 == 1)
    nc, nd = card.astype(np.int64), ((up >= 0) & ~card).astype(np.int64)
    rounds = 0
    while (up >= 0).any():
        live = up >= 0
        qq = up[live]
        last2, nc2, nd2, up2 = last.copy(), nc.copy(), nd.copy(), up.copy()
        last2[live], nc2[live], nd2[live], up2[live] = last[qq], nc[live] + nc[qq], nd[live] + nd[qq], up[qq]
        last, nc, nd, up, rounds = last2, nc2, nd2, up2, rounds + 1
        assert rounds <= 32
    return last, nc, nd, rounds


def order_step(node, top, dq, dj):
    """One synchronous round: every junction from the plane before the round.  dq: the stream donors of junctions, dj their
    receivers."""
    vals = node[top[dq]]
    m1 = np.zeros(node.size, np.int64)
    np.maximum.at(m1, dj, vals)
    ism = vals == m1[dj]
    cnt = np.bincount(dj[ism], minlength=node.size)
    m2 = np.zeros(node.size, np.int64)
    np.maximum.at(m2, dj[~ism], vals[~ism])
    m2 = np.where(cnt >= 2, m1, m2)
    new = node.copy()
    js = np.unique(dj)
    new[js] = np.maximum(node[js], np.maximum(m1[js], m2[js] + 1))
    return new


def network_links(code, acc, min_cells, max_rounds=None):
    """The link-top form: classes from the donor counts, top by the doubling, then the synchronous iteration over the junctions
    until a round changes nothing.  -> dict as network_kahn plus link_rounds and order_rounds (the last one, which changes
    nothing, included); with max_rounds the plane after that many rounds."""
    S, nxt, don, sd, cls, term = _graph(code, acc, min_cells)
    top, nc, nd, link_rounds = link_doubling(code, acc, min_cells)
    jd = don & (cls[np.where(nxt >= 0, nxt, 0)] == JUNCTION)
    dq, dj = np.nonzero(jd)[0], nxt[jd]
    node = S.astype(np.int64)
    rounds = 0
    while dq.size and (max_rounds is None or rounds < max_rounds):
        new = order_step(node, top, dq, dj)
        rounds += 1
        if np.array_equal(new, node):
            break
        node = new
    order = np.where(S, node[np.where(S, top, 0)], 0)
    s = code.shape
    return {"cls": cls.reshape(s), "link": top.reshape(s), "nc": nc.reshape(s), "nd": nd.reshape(s), "order": order.reshape(s),
            "cells": int(S.sum()), "heads": int((cls == HEAD).sum()), "junctions": int((cls == JUNCTION).sum()),
            "outlets": int(term.sum()), "link_rounds": link_rounds, "order_rounds": rounds}


def order_counts(net):
    """-> (the largest order, cells per order 1..15, links per order 1..15), higher orders in the last bin."""
    o = np.minimum(net["order"], NBINS).ravel()
    lk = np.isin(net["cls"].ravel(), (HEAD, JUNCTION))
    cells = [int((o == i).sum()) for i in range(1, NBINS + 1)]
    links = [int(((o == i) & lk).sum()) for i in range(1, NBINS + 1)]
    return int(net["order"].max()) if net["order"].size else 0, cells, links


def info(net, cellsize=1.0):
    """stream_network's info from a network dict, without the round counts."""
    mx, cells, links = order_counts(net)
    ln = DR.length_m(net["nc"], net["nd"], cellsize)
    return {"stream_cells": net["cells"], "heads": net["heads"], "junctions": net["junctions"], "outlets": net["outlets"],
            "links": net["heads"] + net["junctions"], "max_order": mx, "cells_by_order": cells, "links_by_order": links,
            "longest_link_m": float(ln.max()) if ln.size else 0.0}


# ---- HAND ---------------------------------------------------------------------------------------------------------------------
def hand(w, code, stream, cellsize=1.0):
    """-> dict(hand, distance float32 [H][W], drained, undrained, stream_cells, max_hand, rounds)."""
    w = np.asarray(w, np.float32)
    stream = np.asarray(stream) != 0
    ws = DR.watersheds(code, stream, cellsize)
    T = ws["T"]
    ok = T >= 0
    drained = ok & stream.ravel()[np.where(ok, T, 0)]
    with np.errstate(invalid="ignore"):
        h = np.where(drained, w - w.ravel()[np.where(ok, T, 0)], np.float32(np.nan)).astype(np.float32)
    h[np.isnan(h)] = np.float32(np.nan)
    dist = np.where(drained, ws["length"], np.float32(np.nan)).astype(np.float32)
    pos = h[drained & (h > 0)]
    return {"hand": h, "distance": dist, "drained": int(drained.sum()), "undrained": int((ok & ~drained).sum()),
            "stream_cells": int((stream & ok).sum()), "max_hand": float(pos.max()) if pos.size else 0.0, "rounds": ws["rounds"]}


def drainage_mask(code, acc, min_cells, min_order=1):
    S = (code != 0) & (acc >= min_cells)
    if min_order > 1:
        S = network_kahn(code, acc, min_cells)["order"] >= min_order
    return S.astype(np.uint8)


# ---- flood comparison ---------------------------------------------------------------------------------------------------------
def flood_compare(sel, ht, hp, stages):
    """The counters of tg_flood_compare with plain numpy -> a list of 6 + 3 * len(stages) Python ints."""
    ht, hp = np.asarray(ht, np.float32), np.asarray(hp, np.float32)
    s = np.asarray(sel) != 0
    nt, np_ = np.isnan(ht), np.isnan(hp)
    ok = s & ~nt & ~np_
    a, b = ht[ok], hp[ok]
    d = (b - a).astype(np.float32)
    ad = np.abs(d)
    q = lambda v: sum(int(x) for x in np.rint(v.astype(np.float64) * 1024.0).tolist())
    out = [int(ok.sum()), int((s & nt).sum()), int((s & np_).sum()), q(ad), q(d),
           int(ad.max().view(np.uint32)) if ad.size else 0]
    for st in stages:
        st = np.float32(st)
        wt, wp = a <= st, b <= st
        out += [int(wt.sum()), int(wp.sum()), int((wt & wp).sum())]
    return out


def flood_report(c, stages, stream_cells):
    """assemble_flood's arithmetic, written out once more."""
    cells = c[0]
    ratio = lambda a, b: a / b if b else None
    rep = {"cells": cells, "stream_cells": stream_cells, "undrained_truth": c[1], "undrained_pred": c[2],
           "hand": {"mae_m": ratio(c[3] / 1024, cells), "bias_m": ratio(c[4] / 1024, cells),
                    "max_m": float(np.array([c[5]], np.uint32).view(np.float32)[0]) if cells else None},
           "stages": []}
    for i, s in enumerate(stages):
        t, p, b = c[6 + 3 * i:9 + 3 * i]
        rep["stages"].append({"stage_m": float(np.float32(s)), "truth_cells": t, "pred_cells": p, "both_cells": b,
                              "csi": ratio(b, t + p - b), "precision": ratio(b, p), "recall": ratio(b, t)})
    return rep


def flood(z, pred, holes, cellsize, stream_cells, stages):
    """flood_errors with the oracles -> (counters, report, the two sides: the routing dict plus "hand")."""
    z, pred = np.asarray(z, np.float32), np.asarray(pred, np.float32)
    known = DO.known_map(z) & DO.known_map(pred)
    sides = []
    for s in (z, pred):
        r = FO.route(np.where(known, s, np.float32(np.nan)), fill=True)
        r["h"] = hand(r["w"], r["dir"], drainage_mask(r["dir"], r["acc"], stream_cells), cellsize)
        sides.append(r)
    c = flood_compare(holes, sides[0]["h"]["hand"], sides[1]["h"]["hand"], stages)
    return c, flood_report(c, stages, stream_cells), sides


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def grid(rows):
    """A direction grid from rows of characters: '.' unknown, 1..8 the codes, 'o' OUT, 'p' PIT."""
    m = {".": 0, "o": FO.OUT, "p": FO.PIT}
    return np.array([[m[ch] if ch in m else int(ch) for ch in row] for row in rows], np.uint8)


def comb(width=264):
    """5 x width: the stem is row 2, columns 4 .. width - 1, flowing E to an OUT in the last column; it starts at (2, 4) as the
    confluence of two order-2 streams, (1, 3) and (3, 3), each fed by two heads in column 2; heads at (1, c), c = 6, 8, ..,
    width - 2, flow S into it.  The stem is of order 3 throughout, and an order-1 side stream never raises it: the 3 has to
    travel junction by junction.  -> (code, acc)"""
    code = np.zeros((5, width), np.uint8)
    code[2, 4:width - 1] = 1
    code[2, width - 1] = FO.OUT
    code[1, 3], code[3, 3] = 2, 8                                   # SE and NE into (2, 4)
    code[0, 2], code[1, 2] = 2, 1                                   # SE and E into (1, 3)
    code[3, 2], code[4, 2] = 1, 8                                   # E and NE into (3, 3)
    code[1, 6:width - 1:2] = 3                                      # S into the stem
    acc, _ = FO.accumulate_kahn(code)
    return code, acc
