"""GPU checks of the void-fill solvers stage by stage (csrc/voidfill.hip): tg_vfill_setup, tg_vfill_cycle,
tg_vfill_pcg_start / _iter and tg_vfill_bih_start / _iter are called one at a time through tg_hip.ops, the workspaces are read
at the offsets of vfill_layout, vfill_pcg_layout and vfill_bih_layout, and every level's right-hand side, down-pass and up-pass
field, every vector, scalar and per-tile partial of the conjugate gradients is compared with the numpy mirrors
(tests/vfill_pcg_mirror.py, tests/vfill_bih_mirror.py) by tests/vfill_trace.compare: within K x max(max |fp32 mirror - fp64
mirror|, eps32 x scale) of the fp64 mirror, the fp32 mirror rounding as the compiled kernels do (fma=True: the compiler contracts
five products and sums that the source writes apart).  The scalars are also checked against the state's own vectors and scalars
(the dot products to the order of an fp64 sum, alpha and beta bit for bit), and a scalar on which the two mirrors disagree
beyond 2^-10 of its size, rounding of a cancelling sum, is held to that check alone (vfill_trace.GATE).  Every compared step is a single step; the converged result, which hides
a wrong restriction, prolongation, coarsest solve, halo, partial or beta, is the business of the three test_hip_fill_voids*.py."""
import numpy as np
import pytest
import torch

from tests import vfill_bih_mirror as B
from tests import vfill_pcg_mirror as M
from tests import vfill_trace as T

pytestmark = pytest.mark.gpu
CYCLES = 3
PCG_ITERS = 3
BIH_ITERS = 2
BIH_DOT_TOL = 2.0 ** -30           # A p = D(D(p)) cancels: its fp64 rounding is a larger share of p.Ap than in the Laplace solvers


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


_CASES = {}


def _case(name):
    """(z, known) and the fp32 set-up of a case, built once and left unchanged."""
    if name not in _CASES:
        z, k = T.case(name)
        v, c, _ = M._start(z, k, np.float32)
        for a in (z, k, v):
            a.setflags(write=False)
        _CASES[name] = (z, k, v, c, M.Plan(k, np.float32))
    return _CASES[name]


_REFS = {}


def _ref(key, make):
    """A mirror's trace, computed once per case and solver and shared by the two runs."""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


class Ws:
    """A workspace copied to the host, read by byte offset."""

    def __init__(self, t):
        self.b = t.cpu().numpy()

    def arr(self, off, dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.b[off:off + n].view(dtype).reshape(shape).copy()


def _setup(dev, name):
    from mvp_gan.src.fill_voids import vfill_layout
    from tg_hip import ops as O
    z, k, v, c, plan = _case(name)
    H, W = z.shape
    ws = O.vfill_ws(H, W, dev)
    O.vfill_setup(torch.from_numpy(z.copy()).to(dev), torch.from_numpy(k.astype(np.float32)).to(dev), None, ws)
    lay, nbytes = vfill_layout(H, W)
    assert nbytes == ws.numel() and len(lay) == plan.L
    return ws, lay


def _check_setup(w, lay, name):
    """c, v = z - c and the flags of every level bit for bit; per level the active-tile count and the set of listed tiles; the
    coarse levels' fields and right-hand sides 0."""
    z, k, v, c, plan = _case(name)
    from mvp_gan.src.fill_voids import VFILL_HDR
    hdr = w.arr(0, VFILL_HDR, ())
    _same(np.float32(hdr["c"]).reshape(1), np.float32(c).reshape(1), "c")
    assert int(hdr["known"]) == int(k.sum())
    L = plan.L
    for l, (lv, pl) in enumerate(zip(lay, plan.lv)):
        h, wd = lv["H"], lv["W"]
        assert (h, wd) == (pl["H"], pl["W"])
        fl = w.arr(lv["flags"], np.uint8, (h, wd))
        assert np.isin(fl, (0, 2)).all(), f"setup/L{l}/flags"
        T.exact(f"setup/L{l}/fix", fl == 2, pl["fix"])
        for key in ("u0", "u1"):
            _same(w.arr(lv[key], np.float32, (h, wd)), v if l == 0 else np.zeros((h, wd), np.float32), f"setup/L{l}/{key}")
        if l:
            _same(w.arr(lv["f"], np.float32, (h, wd)), np.zeros((h, wd), np.float32), f"setup/L{l}/f")
        act = T.tiles_with_unknown(pl["fix"])
        n = int(hdr["ntiles"][l])
        if l == L - 1:
            assert n == 0, f"setup/L{l}: the coarsest level keeps no tile list"
            continue
        assert lv["tiles"] == act.size and n == int(act.sum()), (f"setup/L{l}/ntiles", n, int(act.sum()))
        listed = w.arr(lv["list"], np.int32, (lv["tiles"],))[:n]
        assert len(set(listed.tolist())) == n and set(listed.tolist()) == set(np.flatnonzero(act.ravel()).tolist()), \
            f"setup/L{l}/tiles"
    assert (hdr["ntiles"][L:] == 0).all()


def _read_cycle(w, lay):
    """The trace of the last plain cycle as the workspace holds it: per level f, u1 (down) and u0 (up)."""
    L = len(lay)
    tr = {"f": [None] * L, "down": [None] * L, "up": [None] * L, "u1": [None] * L}
    for l, lv in enumerate(lay):
        sh = (lv["H"], lv["W"])
        if l:
            tr["f"][l] = w.arr(lv["f"], np.float32, sh)
        tr["u1"][l] = w.arr(lv["u1"], np.float32, sh)
        if l < L - 1:
            tr["down"][l] = tr["u1"][l]
        tr["up"][l] = w.arr(lv["u0"], np.float32, sh)
    return tr


def run_mg(dev, name, K=None, log=None):
    """Setup and CYCLES plain cycles; -> the arrays read, for the bitwise comparison of two runs."""
    from tg_hip import ops as O
    z, k, v, c, plan = _case(name)
    H, W = z.shape
    L = plan.L
    ws, lay = _setup(dev, name)
    w = Ws(ws)
    _check_setup(w, lay, name)
    read = {"flags": [w.arr(lv["flags"], np.uint8, (lv["H"], lv["W"])) for lv in lay]}
    ch = torch.zeros(1, dtype=torch.int32, device=dev)
    u_in = v
    for cyc in range(1, CYCLES + 1):
        O.vfill_cycle(H, W, ws, ch)
        w = Ws(ws)
        got = _read_cycle(w, lay)
        r64, r32 = _ref((name, "mg"), lambda: T.cycle_refs(k, v)) if cyc == 1 else T.cycle_refs(k, u_in)
        T.compare_cycle(f"{name}/mg/cycle{cyc}", got, r64, r32, K=K, log=log)
        assert got["f"][0] is None and lay[0]["f"] is None            # level 0 of the plain cycle has no right-hand side
        if L == 1:
            assert got["down"][0] is None
            _same(got["u1"][0], v, "one level: u1 is never written")   # the coarsest kernel works on u0 alone
        else:
            _same(got["u1"][L - 1], np.zeros_like(got["u1"][L - 1]), "the coarsest level has no down pass")
        # the change word: exactly the largest |u0 - u_in| over the unknowns in fp32, and within the bound of the mirrors'
        change = ch.cpu().numpy().view(np.float32)[0]
        d = np.abs(got["up"][0] - u_in)[~k].max()
        _same(np.float32(change).reshape(1), np.float32(d).reshape(1), f"{name}/mg/cycle{cyc}/change")
        c64, c32 = (float(np.abs(r["up"][0] - np.asarray(u_in, r["up"][0].dtype))[~k].max()) for r in (r64, r32))
        T.compare(f"{name}/mg/cycle{cyc}/L0/change", float(change), c64, c32, scale=float(np.abs(r64["up"][0]).max()),
                  K=T.K_FIELD if K is None else K, log=log)
        # cells of tiles without an unknown keep their setup value; fixed cells keep it everywhere
        for l, pl in enumerate(plan.lv):
            quiet = ~T.cell_tile_mask(T.tiles_with_unknown(pl["fix"]), pl["H"], pl["W"]) if l < L - 1 else pl["fix"]
            quiet = quiet | pl["fix"]
            keep = v if l == 0 else np.zeros((pl["H"], pl["W"]), np.float32)
            for key in ("u1", "up") + (("f",) if l else ()):
                ref = keep if key != "f" else np.zeros_like(keep)
                _same(got[key][l][quiet], ref[quiet], f"{name}/mg/cycle{cyc}/L{l}/{key}: cells without an unknown")
        read[f"cycle{cyc}"] = [a for key in ("f", "u1", "up") for a in got[key] if a is not None] + [np.float32(change).reshape(1)]
        u_in = got["up"][0]
        u_in.setflags(write=False)
    return read


def _scalars(w, off):
    from mvp_gan.src.fill_voids import VFILL_PCG_SCAL
    s = w.arr(off, VFILL_PCG_SCAL, ())
    return {k: s[k].item() for k in VFILL_PCG_SCAL.names}


def _partials(name, prefix, got_parts, states, k_idx, ap, K, log, gated, tol):
    """The per-tile partials of p.Ap, r'.z and r'.z' (by tile id): slots of tiles without an unknown exactly 0; each slot the fp64
    block sum of the GPU's own vectors and the scalar the sum of its slots (within tol x sum |terms|: the order of an fp64 sum);
    and against the block sums of the mirrors, unless the scalar has no reference (vfill_trace.GATE).  states: (got, s64, s32)
    lists; ap: p -> A p."""
    z, k = _case(name)[:2]
    act = T.tiles_with_unknown(k)
    f = np.float64
    terms = []
    for st in states:
        s = st[k_idx]
        zo = st[k_idx - 1]["z"] if k_idx else np.zeros_like(s["z"])
        terms.append([s["p"].astype(f) * ap(s["p"]).astype(f), s["r"].astype(f) * zo.astype(f),
                      s["r"].astype(f) * s["z"].astype(f)])
    for j, key in enumerate(("pap", "rz_old", "rz_new")):
        what = f"{prefix}/part_{key}"
        g = got_parts[j].reshape(act.shape)
        assert (g[~act].view(np.uint64) == 0).all(), f"{what}: a slot of a tile without an unknown is not 0"
        own, mag = T.tile_sums(terms[0][j]), T.tile_sums(np.abs(terms[0][j]))
        bad = np.abs(g - own) > tol * mag
        assert not bad.any(), f"{what}: tile {np.argwhere(bad)[0].tolist()} is not the block sum of the GPU's own vectors"
        total = float(states[0][k_idx][key])
        assert abs(total - float(g.sum())) <= tol * float(mag.sum()), f"{prefix}/{key}: not the sum of its partials"
        if f"{prefix}/{key}" not in gated:
            T.compare(what, g, T.tile_sums(terms[1][j]), T.tile_sums(terms[2][j]), K=T.K_SCALAR if K is None else K, log=log)


def run_pcg(dev, name, K=None, log=None):
    from mvp_gan.src.fill_voids import vfill_pcg_layout
    from tg_hip import ops as O
    z, k, v, c, plan = _case(name)
    H, W = z.shape
    ws, lay = _setup(dev, name)
    pws = O.vfill_pcg_ws(H, W, dev)
    q, nbytes = vfill_pcg_layout(H, W)
    assert nbytes == pws.numel()
    s64, s32 = _ref((name, "pcg"), lambda: T.pcg_refs(z, k, PCG_ITERS))
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    got, parts, read = [], [], {}
    for it in range(PCG_ITERS + 1):
        if it == 0:
            O.vfill_pcg_start(H, W, ws, pws)
        else:
            O.vfill_pcg_iter(H, W, ws, pws, st)
        w, pw = Ws(ws), Ws(pws)
        s = _scalars(pw, 0)
        assert s["restarts"] == 0 and s["_pad"] == 0
        for key in ("r", "z"):
            s[key] = pw.arr(q[key], np.float32, (H, W))
        s["p"] = pw.arr(q["p1" if s["parity"] else "p0"], np.float32, (H, W))
        s["x"] = w.arr(lay[0]["u0"], np.float32, (H, W))
        _same(s["x"], w.arr(lay[0]["u1"], np.float32, (H, W)), "x' is copied back from u1")
        got.append(s)
        parts.append([pw.arr(o, np.float64, (q["tiles"],)) for o in q["part"]])
        read[it] = [s["x"], s["r"], s["z"], s["p"]] + parts[-1] + [np.array([s[n] for n in ("rho", "pap", "rz_old", "rz_new")]),
                                                                    np.array([s["alpha"], s["beta"]], np.float32)]
    gated = []
    T.compare_states(f"{name}/pcg", got, s64, s32, lambda p: T.neg_lap(p, k), K_field=K, K_scalar=K, log=log, gated=gated)
    assert sorted(q.split("/", 1)[1] for q in gated) == sorted(T.PCG_GATED[name]), gated
    for it in range(PCG_ITERS + 1):
        step = "start" if it == 0 else f"iter{it}"
        _partials(name, f"{name}/pcg/{step}", parts[it], (got, s64, s32), it, lambda p: T.neg_lap(p, k), K, log, gated, T.DOT_TOL)
        for key in ("r", "z", "p"):
            assert not got[it][key][k].any(), f"{name}/pcg/{step}/{key}: not 0 at a known pixel"
        _same(got[it]["x"][k], v[k], f"{name}/pcg/{step}/x: a known pixel moved")
    assert int(st[1].item()) == 0
    return read


def run_bih(dev, name, inner, K=None, log=None):
    from mvp_gan.src.fill_voids import vfill_bih_layout
    from tg_hip import ops as O
    z, k, v, c, plan = _case(name)
    H, W = z.shape
    ws, lay = _setup(dev, name)
    bws = O.vfill_bih_ws(H, W, dev)
    q, nbytes = vfill_bih_layout(H, W)
    assert nbytes == bws.numel()
    s64, s32 = _ref((name, "bih", inner), lambda: T.bih_refs(z, k, BIH_ITERS, inner))
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    got, parts, read = [], [], {}
    for it in range(BIH_ITERS + 1):
        if it == 0:
            O.vfill_bih_start(H, W, ws, bws, inner)
        else:
            O.vfill_bih_iter(H, W, ws, bws, inner, st)
        w, bw = Ws(ws), Ws(bws)
        s = _scalars(bw, q["sc_out"])
        si = _scalars(bw, q["sc_in"])
        assert s["restarts"] == 0 and si["restarts"] == 0 and s["_pad"] == 0 and si["_pad"] == 0
        if inner == 1:
            assert all(v_ == 0 for v_ in si.values()), "inner = 1 is one bare cycle: the inner block is never written"
        s["x"] = bw.arr(q["xa"], np.float64, (H, W))
        _same(s["x"], bw.arr(q["xb"], np.float64, (H, W)), "x' is copied back from xb")
        _same(w.arr(lay[0]["u0"], np.float32, (H, W)), s["x"].astype(np.float32), "level 0's u0 is x rounded to fp32")
        s["r"] = bw.arr(q["r"], np.float64, (H, W))
        _same(bw.arr(q["rf"], np.float32, (H, W)), s["r"].astype(np.float32), "rf is r rounded to fp32")
        s["z"] = bw.arr(q["z"], np.float32, (H, W))
        s["p"] = bw.arr(q["p1" if s["parity"] else "p0"], np.float32, (H, W))
        got.append(s)
        parts.append([bw.arr(o, np.float64, (q["tiles"],)) for o in q["part"][:3]])
        read[it] = [s["x"], s["r"], s["z"], s["p"]] + parts[-1] + [np.array([s[n] for n in ("rho", "pap", "rz_old", "rz_new")]),
                                                                    np.array([s["alpha"], s["beta"]], np.float32)]
    tag = f"{name}/bih{inner}"
    gated = []
    T.compare_states(tag, got, s64, s32, lambda p: B.apply_A(p, k), K_field=K, K_scalar=K, log=log, gated=gated,
                     dot_tol=BIH_DOT_TOL)
    assert all(q.split("/")[2] != "start" for q in gated), gated
    for it in range(BIH_ITERS + 1):
        step = "start" if it == 0 else f"iter{it}"
        _partials(name, f"{tag}/{step}", parts[it], (got, s64, s32), it, lambda p: B.apply_A(p, k), K, log, gated, BIH_DOT_TOL)
        _same(got[it]["x"][k], v[k].astype(np.float64), f"{tag}/{step}/x: a known pixel moved")
    assert int(st[1].item()) == 0
    return read


def _twice(run, *args):
    """Two runs read bitwise-equal values at every compared offset."""
    a, b = run(*args), run(*args)
    assert a.keys() == b.keys()
    for key in a:
        assert len(a[key]) == len(b[key])
        for x, y in zip(a[key], b[key]):
            _same(x, y, f"run-to-run, {key}")


@pytest.mark.parametrize("name", T.CASES)
def test_plain_cycle_stages(dev, name):
    _twice(run_mg, dev, name)


@pytest.mark.parametrize("name", T.CASES)
def test_pcg_stages(dev, name):
    _twice(run_pcg, dev, name)


@pytest.mark.parametrize("inner", [1, 3])
@pytest.mark.parametrize("name", T.CASES)
def test_bih_stages(dev, name, inner):
    _twice(run_bih, dev, name, inner)


def test_big_case_reaches_the_second_trip():
    """3 x 131500: more level-0 tiles than the grid limit, every one of them active, and unknowns in the tiles with an id >= 2048,
    so the comparisons above cover what the tile loop's second trip wrote."""
    z, k = _case("3x131500")[:2]
    act = T.tiles_with_unknown(k)
    assert act.size == 2055 > 2048 and act.all() and (~k[:, 2048 * 64:]).sum() > 100
    lv = M.levels(*z.shape)
    assert [h for h, _ in lv[:3]] == [3, 2, 1] and lv[-1] == (1, 9)
