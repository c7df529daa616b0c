"""CPU oracle of the flow routing (csrc/flow.hip, mvp_gan/src/flow_routing.py), numpy only.

Codes: 0 unknown; 1..8 the receiver E, SE, S, SW, W, NW, N, NE; OUT = 9; PIT = 255; UNDECIDED = 254 between the slope step and
the flat directions.  Equal candidates are taken in the order E, S, W, N, SE, SW, NW, NE.  The slope step is done in float32
(one subtract, for a diagonal one multiply by float32(0x1.6a09e6p-1)).  D has two independent forms, a multi-source
breadth-first search and the synchronous relaxation; the accumulation has two, Kahn's topological order and the doubling
recurrence.  Known pixels and outlets are tests/depfill_oracle.py's (connectivity 8)."""
from collections import deque

import numpy as np

from tests import depfill_oracle as DO

OUT, PIT, UNDECIDED, FAR = 9, 255, 254, 0x7fffffff
DY = (0, 1, 1, 1, 0, -1, -1, -1)                       # code - 1 -> offset
DX = (1, 1, 0, -1, -1, -1, 0, 1)
PREF = (1, 3, 5, 7, 2, 4, 6, 8)                        # codes in the order of preference
DIAG = np.float32(float.fromhex("0x1.6a09e6p-1"))


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside."""
    H, W = a.shape
    pad = np.full((H + 2, W + 2), fill, a.dtype)
    pad[1:-1, 1:-1] = a
    return pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def slope_step(w, known):
    """-> (dir uint8 with UNDECIDED, D int32: 0 decided, FAR undecided, -1 unknown)."""
    w = np.asarray(w, np.float32)
    H, W = w.shape
    best = np.zeros((H, W), np.float32)
    code = np.zeros((H, W), np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in PREF:
            dy, dx = DY[c - 1], DX[c - 1]
            s = (w - _shift(w, dy, dx, np.float32(0))).astype(np.float32)
            if c % 2 == 0:
                s = (s * DIAG).astype(np.float32)
            ok = known & _shift(known, dy, dx, False) & (s > best)       # strict: the first of equals keeps its place
            best = np.where(ok, s, best)
            code = np.where(ok, np.uint8(c), code)
    out = DO.outlets(known, 8)
    code = np.where(known & (code == 0), np.where(out, np.uint8(OUT), np.uint8(UNDECIDED)), code).astype(np.uint8)
    code[~known] = 0
    D = np.where(code == UNDECIDED, FAR, 0).astype(np.int32)
    D[~known] = -1
    return code, D


def flat_distance_bfs(w, D0):
    """D by a multi-source breadth-first search from the decided pixels through equal heights."""
    w = np.asarray(w, np.float32)
    H, W = w.shape
    D = D0.copy()
    und = D0 == FAR
    seed = np.zeros((H, W), bool)                                  # decided pixels next to an undecided one of their height
    for dy, dx in zip(DY, DX):
        seed |= (D0 == 0) & _shift(und, dy, dx, False) & (_shift(w, dy, dx, np.float32(0)) == w)
    q = deque((int(y), int(x)) for y, x in zip(*np.nonzero(seed)))
    while q:
        y, x = q.popleft()
        for dy, dx in zip(DY, DX):
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W and D[yy, xx] == FAR and w[yy, xx] == w[y, x]:
                D[yy, xx] = D[y, x] + 1
                q.append((yy, xx))
    return D


def flat_relax_step(w, D):
    w = np.asarray(w, np.float32)
    big = np.int64(FAR)
    cur = np.where(D < 0, big, D.astype(np.int64))
    m = np.full(D.shape, big, np.int64)
    hs = np.where(D < 0, np.float32(np.nan), w)
    with np.errstate(invalid="ignore"):
        for dy, dx in zip(DY, DX):
            eq = _shift(hs, dy, dx, np.float32(np.nan)) == hs
            m = np.minimum(m, np.where(eq, _shift(cur, dy, dx, big), big))
    new = np.minimum(cur, np.where(m < big, m + 1, big))
    return np.where(D < 0, -1, new).astype(np.int32)


def flat_distance_relax(w, D0, max_steps=None):
    """D by the synchronous relaxation D <- min(D, 1 + min over the equal-height neighbours D) -> (D, steps taken)."""
    D, steps = D0.copy(), 0
    while max_steps is None or steps < max_steps:
        nd = flat_relax_step(w, D)
        steps += 1
        if np.array_equal(nd, D):
            break
        D = nd
    return D, steps


def flat_dirs(w, code, D, exact=True):
    """The undecided pixels' codes from D.  exact: the neighbour of equal height with D(p) - 1 (the definition); otherwise the
    one with the smallest D below D(p), which is what a stopped iteration leaves (the same thing at the fixed point)."""
    w = np.asarray(w, np.float32)
    out = code.copy()
    und = code == UNDECIDED
    fin = und & (D > 0) & (D < FAR)
    best = np.where(fin, D, 0).astype(np.int64)
    pick = np.full(code.shape, PIT, np.uint8)
    hs = np.where(D < 0, np.float32(np.nan), w)
    with np.errstate(invalid="ignore"):
        for c in PREF:
            dy, dx = DY[c - 1], DX[c - 1]
            dn = _shift(D.astype(np.int64), dy, dx, np.int64(-1))
            eq = _shift(hs, dy, dx, np.float32(np.nan)) == hs
            if exact:
                ok = fin & eq & (dn == D.astype(np.int64) - 1) & (pick == PIT)
            else:
                ok = fin & eq & (dn >= 0) & (dn < best)
                best = np.where(ok, dn, best)
            pick = np.where(ok, np.uint8(c), pick)
    out[und] = pick[und]
    return out


def receivers(code):
    """-> next int64 [H * W]: the receiver's linear index, -1 for OUT, PIT and unknown."""
    H, W = code.shape
    y, x = np.mgrid[0:H, 0:W]
    nxt = np.full((H, W), -1, np.int64)
    for c in range(1, 9):
        sel = code == c
        nxt[sel] = (y[sel] + DY[c - 1]) * W + x[sel] + DX[c - 1]
    return nxt.ravel()


def accumulate_kahn(code):
    """-> (A int32 [H][W], the longest flow path in steps)."""
    nxt = receivers(code)
    n = nxt.size
    acc = (code.ravel() != 0).astype(np.int64)
    length = np.zeros(n, np.int64)                                 # steps of the longest path that ends here
    indeg = np.bincount(nxt[nxt >= 0], minlength=n)
    q = deque(np.nonzero((indeg == 0) & (code.ravel() != 0))[0].tolist())
    seen = 0
    while q:
        p = q.popleft()
        seen += 1
        r = nxt[p]
        if r >= 0:
            acc[r] += acc[p]
            length[r] = max(length[r], length[p] + 1)
            indeg[r] -= 1
            if indeg[r] == 0:
                q.append(int(r))
    assert seen == int((code != 0).sum()), "the direction grid has a cycle"
    return acc.reshape(code.shape).astype(np.int32), int(length.max()) if n else 0


def accumulate_doubling(code):
    """The recurrence of the GPU -> (A int32 [H][W], rounds)."""
    nxt = receivers(code)
    S = (code.ravel() != 0).astype(np.int64)
    rounds = 0
    while (nxt >= 0).any():
        live = nxt >= 0
        S2 = S.copy()
        np.add.at(S2, nxt[live], S[live])
        n2 = np.full_like(nxt, -1)
        n2[live] = nxt[nxt[live]]
        S, nxt, rounds = S2, n2, rounds + 1
        assert rounds <= 32
    return S.reshape(code.shape).astype(np.int32), rounds


def route(z, mask=None, nodata=None, fill=True):
    """The whole chain -> dict(known, w, dir, D, acc, flat_cells, pits, outlets, longest, rounds)."""
    z = np.asarray(z, np.float32)
    known = DO.known_map(z, mask, nodata)
    if fill:
        w = DO.finish(z, DO.priority_flood(z, known, 8), known)[0]
    else:
        w = z
    code0, D0 = slope_step(w, known)
    D = flat_distance_bfs(w, D0)
    code = flat_dirs(w, code0, D)
    acc, longest = accumulate_kahn(code)
    rounds = 0
    while (1 << rounds) <= longest:
        rounds += 1
    und = code0 == UNDECIDED
    return {"known": known, "w": w, "dir": code, "D": D, "acc": acc, "flat_cells": int((und & (code != PIT)).sum()),
            "pits": int((code == PIT).sum()), "outlets": int(DO.outlets(known, 8).sum()), "longest": longest, "rounds": rounds}


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def rounded_pits(H, W, seed, npits=20, base=1000.0):
    """Integer-rounded relief near `base` with dug pits: plateaus and ties."""
    return np.rint(DO.pits_scene(H, W, seed, npits=npits, base=base, relief=2.0)).astype(np.float32)


def spiral_flat(n=130, pitch=3):
    """The spiral of depfill_oracle.spiral_scene with a constant channel floor (1000 m) between the wall (1100 m) and the border
    ring (1050 m), and the ring's cells next to the channel's outer end, (1 .. pitch - 1, 0), dug to 990 m: the only way out.  D
    runs the whole channel from there, across every tile seam.  The lanes are two pixels wide (pitch 3): at depfill's pitch of 4
    the channel is 3971 steps long, and the tests want more than 4096.  -> (z, channel)"""
    z, channel = DO.spiral_scene(n, pitch)
    z = z.copy()
    z[channel] = 1000.0
    z[pitch, 0] = 1050.0
    z[1:pitch, 0] = 990.0
    return z, channel


def serpentine(n=130):
    """A one-pixel channel between walls (1300 m): along the odd rows, joined at alternating ends, strictly descending by 2 cm a
    cell from 1200 m to its mouth on the raster's edge.  -> (z, order int [n][n]: the cell's place along the channel, -1 off it)"""
    z = np.full((n, n), 1300.0, np.float32)
    order = np.full((n, n), -1, np.int64)
    k = 0
    rows = list(range(1, n - 1, 2))
    for i, r in enumerate(rows):
        cols = range(1, n - 1) if i % 2 == 0 else range(n - 2, 0, -1)
        for c in cols:
            order[r, c] = k
            k += 1
        if i + 1 < len(rows):
            order[r + 1, cols[-1]] = k                             # the link down to the next row
            k += 1
    last = rows[-1]
    end = n - 1 if (len(rows) - 1) % 2 == 0 else 0                 # the mouth: on through the edge column
    order[last, end] = k
    on = order >= 0
    z[on] = (1200.0 - 0.02 * order[on]).astype(np.float32)
    return z, order


def lake_scene(n=130):
    """Ground that falls to the east, a dyke (1010 m) around a flat lake (1000 m) that lies across the seam between two tiles, and
    one notch in the dyke at (64, 64), the corner pixel of a tile where four tiles meet, itself at 1000 m: the lake's only way
    out, to the lower ground east of it.  -> (z, lake bool)"""
    y, x = np.mgrid[0:n, 0:n]
    z = (1001.0 - 0.03 * x + 0.001 * y).astype(np.float32)
    z[29:102, 19:65] = 1010.0
    lake = np.zeros((n, n), bool)
    lake[30:101, 20:64] = True
    z[lake] = 1000.0
    z[64, 64] = 1000.0
    return z, lake
