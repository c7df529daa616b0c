"""CPU checks of the biharmonic void fill (fill_voids(method="biharmonic"), csrc/voidfill.hip): the dense
fp64 oracle (tests/vfill_bih_oracle.py) against scipy's sparse solve and against the closed form it must reproduce and the
harmonic fill must miss; the numpy mirror of the solver (tests/vfill_bih_mirror.py) in fp64 against the oracle, and with the
kernels' storage types within 2e-5 x range on the scenes of section 8q, with the iteration counts the GPU tests budget from; the
third workspace's query against its host mirror; host-side rejection by the three new C entry points; Python validation, the
CLI flags, BASELINES and the new symbols.  All without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import vfill_bih_mirror as BM
from tests import vfill_bih_oracle as BO
from tests import vfill_oracle as VO
from tests import vfill_pcg_mirror as M
from tests.test_hip_fill_voids_bih import MIRROR_ITERATIONS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2e-5                        # max |u - u*| / range, the bound of the GPU tests
# The tight solve stops when the largest step is 1e-10 x range; while the steps contract by 0.999 or better per iteration the
# remaining error is at most 1000 steps: 1e-7 x range, 200 times inside BOUND.
TIGHT_TOL, TIGHT_ERR = 1e-10, 1e-7


def _range(z, k):
    return float(z[k].max()) - float(z[k].min())


# ---- the oracle -----------------------------------------------------------------------------------------------------
def _sparse_normal_solve(z, known):
    sp = pytest.importorskip("scipy.sparse")
    spl = pytest.importorskip("scipy.sparse.linalg")
    H, W = known.shape
    n = H * W
    idx = np.arange(n).reshape(H, W)
    rows, cols, vals = [], [], []
    for a, b in ((idx[1:, :], idx[:-1, :]), (idx[:, 1:], idx[:, :-1])):
        a, b = a.ravel(), b.ravel()
        rows += [a, b, a, b]
        cols += [b, a, a, b]
        vals += [np.ones(a.size), np.ones(a.size), -np.ones(a.size), -np.ones(a.size)]
    L = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    u, kk = np.flatnonzero(~known.ravel()), np.flatnonzero(known.ravel())
    B, Bk = L[:, u], L[:, kk]
    out = np.asarray(z, np.float64).copy().ravel()
    out[u] = spl.spsolve((B.T @ B).tocsc(), -(B.T @ (Bk @ out[kk])))
    return out.reshape(H, W)


@pytest.mark.parametrize("seed", range(4))
def test_oracle_against_scipy(seed):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(1, 30)), int(rng.integers(2, 40))
    z = BM.terrain(H, W, seed)
    known = rng.random((H, W)) < (0.05, 0.3, 0.7, 0.9)[seed]
    known[rng.integers(H), rng.integers(W)] = True
    if known.all():
        known[0, 0] = False
    ref = _sparse_normal_solve(z, known)
    out = BO.solve(z, known)
    assert np.array_equal(out[known], z[known].astype(np.float64))
    assert np.abs(out - ref).max() <= 1e-9 * max(_range(z, known), 1.0)
    assert np.abs(BO.energy_gradient(out, known)).max() <= 1e-9 * max(_range(z, known), 1.0)


@pytest.mark.parametrize("H,W,void", [(37, 53, "disc"), (40, 60, (5, 30, 10, 50)), (64, 64, (2, 62, 20, 40))])
def test_oracle_reproduces_the_cubic_the_harmonic_oracle_misses(H, W, void):
    f = BO.bih_poly_raster(H, W)
    known = ~VO.disc(H, W, 18, 26, 9) if void == "disc" else M.box_known(H, W, [void])
    ys, xs = np.nonzero(~known)
    assert ys.min() >= 2 and xs.min() >= 2 and ys.max() < H - 2 and xs.max() < W - 2
    rng = _range(f, known)
    assert np.abs(M.diff_sum(M.diff_sum(f))[2:-2, 2:-2]).max() <= 1e-10 * rng
    assert np.abs(BO.solve(f, known) - f).max() <= 1e-9 * rng
    miss = np.abs(VO.solve(f, known) - f).max()
    print("harmonic miss / range", miss / rng)
    assert miss > 1e-2 * rng


def test_apply_A_is_the_oracles_matrix():
    z = BM.terrain(9, 11, 1).astype(np.float64)
    known = np.random.default_rng(1).random((9, 11)) < 0.5
    x = np.where(known, 0.0, z)
    a = BM.apply_A(x, known)
    # symmetric and positive: x.Ax = |D(x)|^2 over S
    y = np.where(known, 0.0, np.random.default_rng(2).normal(size=z.shape))
    assert abs((y * a).sum() - (x * BM.apply_A(y, known)).sum()) <= 1e-9 * abs((y * a).sum())
    assert abs((x * a).sum() - (M.diff_sum(x) ** 2).sum()) <= 1e-9 * (x * a).sum()
    assert np.array_equal(a[known], np.zeros(int(known.sum())))


# ---- the mirror -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["37x53 disc, cubic", "96x80 left half"])
def test_fp64_mirror_against_the_oracle(name):
    z, k = BM.case(name)
    rng = _range(z, k)
    ref, info = BM.solve64(z, k, tol=TIGHT_TOL * rng)
    print(name, info["cycles"])
    assert info["converged"] and info["restarts"] == 0
    assert np.array_equal(ref[k], z[k].astype(np.float64))
    assert np.abs(ref - BO.solve(z, k)).max() <= TIGHT_ERR * rng


# the mirror's own outer iterations with the kernels' storage types, inner = 3 (DESIGN.md section 8q lists them next to the GPU's)
ITERATIONS = {
    "37x53 disc, cubic": 13,
    "128x160 void [30:93, 61:130]": 26,
    "300x300 void [64:192, 128:256]": 42,
    "96x80 left half": 29,
    "257x129 1% known": 74,
}


@pytest.mark.parametrize("name", list(ITERATIONS))
def test_mirror_with_the_kernels_storage_types(name):
    z, k = BM.case(name)
    rng = _range(z, k)
    ref, tight = BM.solve64(z, k, tol=TIGHT_TOL * rng)         # accepted above against the oracle
    assert tight["converged"]
    out, info = BM.solve(z, k)
    err = np.abs(out.astype(np.float64) - ref).max()
    print(name, info["cycles"], info["vcycles"], "err / range", err / rng, info["history"])
    assert info["converged"] and info["restarts"] == 0
    assert np.array_equal(out[k], z[k])
    assert err <= BOUND * rng
    assert info["cycles"] == ITERATIONS[name]
    # the mirror stops at the step that meets the rule; the GPU has launched that iteration's preconditioner by then and
    # reports 6 more
    assert info["vcycles"] == 6 * info["cycles"]


@pytest.mark.parametrize("name", [n for n in BM.SMALL_SCENES if n in MIRROR_ITERATIONS])
def test_mirror_counts_of_the_gpu_scenes(name):
    z, m, nd = BM.small_scene(name)
    k = VO.known_mask(z, m, nd)
    zz = np.where(k, z, 0)
    out, info = BM.solve(zz, k)
    assert info["converged"] and info["restarts"] == 0 and info["cycles"] == MIRROR_ITERATIONS[name], info
    # one known pixel: the range is 0 and the fill is that value exactly, which the dense solve only rounds to
    ref = np.full(z.shape, float(z[3, 4])) if name == "12x9 one known" else BO.solve(zz, k)
    assert np.abs(out.astype(np.float64) - ref).max() <= BOUND * _range(zz, k)


@pytest.mark.parametrize("name", [n for n in MIRROR_ITERATIONS if n.endswith("cubic")])
def test_mirror_counts_of_the_cubic_scenes(name):
    z, k = BM.case(name)
    out, info = BM.solve(z, k)
    assert info["converged"] and info["restarts"] == 0 and info["cycles"] == MIRROR_ITERATIONS[name], info
    H, W = z.shape
    assert np.abs(out.astype(np.float64) - BO.bih_poly_raster(H, W)).max() <= BOUND * _range(z, k)


def test_mirror_bare_cycle_does_not_converge_on_the_aligned_void():
    z, k = BM.case("300x300 void [64:192, 128:256]")
    out, info = BM.solve(z, k, inner=1, max_cycles=100)
    assert not info["converged"] and info["cycles"] == 100 and np.isfinite(out).all()


def test_mirror_guards():
    z, m, nd = BM.small_scene("12x9 one known")
    k = m != 0
    out, info = BM.solve(z, k)
    assert info["converged"] and info["change"] == 0.0 and np.array_equal(out, np.full(z.shape, z[3, 4]))
    out, info = BM.solve(z, np.ones(z.shape, bool))
    assert info["cycles"] == 0 and info["vcycles"] == 0 and info["converged"] and np.array_equal(out, z)


# ---- the third workspace --------------------------------------------------------------------------------------------
def _lib():
    from tg_hip import lib as L
    return L, L.load()


SIZES = [(1, 1), (1, 2), (2, 1), (16, 16), (17, 16), (32, 64), (33, 65), (37, 53), (257, 129), (1500, 2100), (4096, 4096),
         (8192, 8192), (8193, 8191), (1, 300000), (300000, 1)]
F64, F32 = ("xa", "xb", "r"), ("rf", "t", "z", "p0", "p1", "e0", "e1", "ri", "zi", "q0", "q1", "d")


@pytest.mark.parametrize("H,W", SIZES)
def test_bih_ws_query_matches_the_mirror_layout(H, W):
    from mvp_gan.src.fill_voids import vfill_bih_layout, vfill_layout, vfill_pcg_layout
    _, lib = _lib()
    lay, total = vfill_bih_layout(H, W)
    assert lib.tg_vfill_bih_ws_bytes(H, W) == total
    assert lay["tiles"] == vfill_layout(H, W)[0][0]["tiles"]
    n = H * W
    spans = [(lay["sc_out"], 256), (lay["sc_in"], 256)] + [(lay[key], 8 * n) for key in F64] + \
        [(lay[key], 4 * n) for key in F32] + [(o, 8 * lay["tiles"]) for o in lay["part"]]
    assert len(lay["part"]) == 6
    spans.sort()
    for (a, na), (b, _) in zip(spans, spans[1:]):
        assert a + na <= b
    assert spans[-1][0] + spans[-1][1] <= total
    assert all(o % 256 == 0 for o, _ in spans)
    # the two existing workspaces keep their layouts
    assert lib.tg_vfill_ws_bytes(H, W) == vfill_layout(H, W)[1]
    assert lib.tg_vfill_pcg_ws_bytes(H, W) == vfill_pcg_layout(H, W)[1]


def test_bih_ws_query_rejects_bad_shapes():
    _, lib = _lib()
    for H, W in ((0, 5), (5, 0), (-1, 3), (1 << 16, 1 << 15)):
        assert lib.tg_vfill_ws_bytes(H, W) == 0
        assert lib.tg_vfill_bih_ws_bytes(H, W) == 0


def test_c_entry_points_reject_without_gpu():
    L, lib = _lib()
    f = [C.c_void_p(0x1000 * (i + 1)) for i in range(4)]
    ws, bws = C.c_void_p(0x100000), C.c_void_p(0x200000)       # 256-byte aligned, never dereferenced

    def err(rc, msg, code=(-1, -3)):
        assert rc in code and msg in lib.tg_last_error(), (rc, lib.tg_last_error())

    nb, nbb = lib.tg_vfill_ws_bytes(8, 8), lib.tg_vfill_bih_ws_bytes(8, 8)
    start = lambda H, W, w, b, p, pb, inner=3: lib.tg_vfill_bih_start(H, W, w, b, p, pb, inner, None)
    it = lambda H, W, w, b, p, pb, inner=3, ch=f[0], rs=f[1]: lib.tg_vfill_bih_iter(H, W, w, b, p, pb, inner, ch, rs, None)
    for H, W in ((0, 5), (5, 0), (-1, 5), (1 << 16, 1 << 15)):
        err(start(H, W, ws, 1 << 30, bws, 1 << 30), b"H*W < 2^31")
        err(it(H, W, ws, 1 << 30, bws, 1 << 30), b"H*W < 2^31")
    for call in (start, it):
        err(call(8, 8, None, nb, bws, nbb), b"null pointer")
        err(call(8, 8, ws, nb, None, nbb), b"null pointer")
        err(call(8, 8, C.c_void_p(0x100004), nb, bws, nbb), b"aligned")
        err(call(8, 8, ws, nb, C.c_void_p(0x200010), nbb), b"aligned")
        for b in (nb - 1, 0):
            err(call(8, 8, ws, b, bws, nbb), b"workspace", (-3,))
        for b in (nbb - 1, 0):
            err(call(8, 8, ws, nb, bws, b), b"biharmonic workspace", (-3,))
        # workspaces sized for a smaller raster are short for a larger one
        err(call(300, 200, ws, lib.tg_vfill_ws_bytes(300, 200), bws, lib.tg_vfill_bih_ws_bytes(150, 100)),
            b"biharmonic workspace", (-3,))
        err(call(300, 200, ws, lib.tg_vfill_ws_bytes(150, 100), bws, lib.tg_vfill_bih_ws_bytes(300, 200)), b"workspace", (-3,))
        for inner in (0, -1, 9, 1 << 20):
            err(call(8, 8, ws, nb, bws, nbb, inner), b"inner")
    err(it(8, 8, ws, nb, bws, nbb, ch=None), b"null pointer")
    err(it(8, 8, ws, nb, bws, nbb, rs=None), b"null pointer")


# ---- Python API -----------------------------------------------------------------------------------------------------
def test_methods_and_defaults():
    from mvp_gan.src import fill_voids as FV
    assert FV.METHODS == ("laplace", "biharmonic")
    sig = inspect.signature(FV.fill_voids).parameters
    assert sig["method"].default == "laplace" and sig["max_cycles"].default is None and sig["inner"].default == 3
    assert sig["solver"].default == "mg"
    assert FV.resolve_max_cycles(None, "laplace") == 50 and FV.resolve_max_cycles(None, "biharmonic") == 200
    assert FV.resolve_max_cycles(7, "laplace") == 7 and FV.resolve_max_cycles(7, "biharmonic") == 7
    z = np.zeros((8, 8), np.float32)
    for method in FV.METHODS:
        assert FV.check_args(z, None, method, None, None, None, None) == (8, 8, None)


@pytest.mark.parametrize("kw,match", [
    (dict(method="thinplate"), "method"),
    (dict(method="Biharmonic"), "method"),
    (dict(method=None), "method"),
    (dict(method=["biharmonic"]), "method"),
    (dict(method="biharmonic", inner=0), "inner"),
    (dict(method="biharmonic", inner=9), "inner"),
    (dict(method="biharmonic", inner=-1), "inner"),
    (dict(method="biharmonic", inner=2.0), "inner"),
    (dict(method="biharmonic", inner=True), "inner"),
    (dict(method="biharmonic", inner=None), "inner"),
    (dict(method="laplace", inner=0), "inner"),
    (dict(method="biharmonic", max_cycles=0), "max_cycles"),
    (dict(method="biharmonic", max_cycles=2.5), "max_cycles"),
    (dict(method="biharmonic", solver="cg"), "solver"),
    (dict(method="biharmonic", tol=-1.0), "tol"),
])
def test_python_rejects_before_any_launch(kw, match):
    from mvp_gan.src.fill_voids import fill_voids
    with pytest.raises(ValueError, match=f"fill_voids: {match}"):
        fill_voids(np.zeros((64, 64), np.float32), **kw)


def test_laplace_info_keys_are_unchanged(monkeypatch):
    # the argument path of fill_voids with the device calls stubbed: which keys each method and solver reports
    import torch
    from mvp_gan.src import fill_voids as FV
    from tg_hip import ops as O
    calls = []

    class Stats:
        def cpu(self):
            return self

        def tolist(self):
            return [60, 4, 0, int(np.float32(1.0).view(np.int32))]

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(FV.R, "to_f32", lambda a, *args, **kw: a)
    monkeypatch.setattr(torch, "zeros", lambda *a, **kw: [np.int32(0), np.int32(0)])
    monkeypatch.setattr(torch, "empty", lambda *a, **kw: np.zeros(1, np.int32))
    for name in ("vfill_ws", "vfill_pcg_ws", "vfill_bih_ws", "vfill_pcg_start", "vfill_bih_start", "vfill_cycle", "vfill_pcg_iter",
                 "vfill_bih_iter", "vfill_finish"):
        monkeypatch.setattr(O, name, (lambda n: lambda *a, **kw: calls.append((n, a[4:5] if "bih" in n else ())))(name))
    monkeypatch.setattr(O, "vfill_setup", lambda *a, **kw: Stats())
    z = np.zeros((8, 8), np.float32)
    base = ["unknown", "unfilled", "cycles", "change", "tol", "converged", "levels"]
    _, info = FV.fill_voids(z)
    assert list(info) == base and info["cycles"] == 1 and [c[0] for c in calls] == ["vfill_ws", "vfill_cycle", "vfill_finish"]
    _, info = FV.fill_voids(z, method="laplace", solver="pcg", inner=5)
    assert list(info) == base + ["solver", "restarts"]
    calls.clear()
    _, info = FV.fill_voids(z, method="biharmonic", solver="pcg", inner=2)
    assert list(info) == base + ["method", "inner", "restarts", "vcycles"]
    assert info["method"] == "biharmonic" and info["inner"] == 2 and info["cycles"] == 1 and info["vcycles"] == 8
    assert [c[0] for c in calls] == ["vfill_ws", "vfill_bih_ws", "vfill_bih_start", "vfill_bih_iter", "vfill_finish"]
    assert calls[2][1] == (2,) and calls[3][1] == (2,)


# ---- CLI flags and baselines ----------------------------------------------------------------------------------------
def test_cli_parses_method_and_inner():
    from mvp_gan.src import fill_voids as FV
    base = ["--dem", "a.asc", "--out", "o.asc"]
    d = FV.build_parser().parse_args(base)
    assert (d.method, d.inner, d.max_cycles, d.solver) == ("laplace", 3, 50, "mg")
    a = FV.build_parser().parse_args(base + ["--method", "biharmonic", "--inner", "5", "--max-cycles", "50"])
    assert (a.method, a.inner, a.max_cycles) == ("biharmonic", 5, 50)
    assert isinstance(d.max_cycles, FV._Unset) and not isinstance(a.max_cycles, FV._Unset)
    with pytest.raises(SystemExit):
        FV.build_parser().parse_args(base + ["--method", "idw"])
    for extra in (["--method", "biharmonic"], ["--method", "laplace", "--inner", "2"]):
        with pytest.raises(FileNotFoundError):                 # the flags parse; the raster is read next
            FV.main(["--dem", "/nonexistent/in.asc", "--out", "o.asc"] + extra)


def test_cli_default_budget_follows_the_method(monkeypatch, tmp_path):
    from mvp_gan.src import fill_voids as FV
    from mvp_gan.src.asc import write_asc
    src = str(tmp_path / "in.asc")
    write_asc(src, np.zeros((4, 5), np.float32), [("ncols", "5"), ("nrows", "4"), ("xllcorner", "0"), ("yllcorner", "0"),
                                                  ("cellsize", "1"), ("NODATA_value", "-9999")])
    seen = []

    class Out:
        def cpu(self):
            return self

        def numpy(self):
            return np.zeros((4, 5), np.float32)

    def fake(dem, mask, **kw):
        seen.append(kw)
        return Out(), {"unknown": 0, "unfilled": 0, "cycles": 0, "change": 0.0, "tol": 0.0, "converged": True, "vcycles": 0}

    monkeypatch.setattr(FV, "fill_voids", fake)
    base = ["--dem", src, "--out", str(tmp_path / "o.asc")]
    FV.main(base)
    FV.main(base + ["--method", "biharmonic"])
    FV.main(base + ["--method", "biharmonic", "--max-cycles", "50", "--inner", "4"])
    assert [(k["method"], k["max_cycles"], k["inner"]) for k in seen] == \
        [("laplace", None, 3), ("biharmonic", None, 3), ("biharmonic", 50, 4)]


def test_baselines():
    from mvp_gan.src import evaluate_raster as ER
    assert ER.BASELINES == ("laplace", "biharmonic")
    assert inspect.signature(ER.baseline_report).parameters["method"].default == "laplace"
    z = np.zeros((64, 64), np.float32)
    with pytest.raises(ValueError, match="baseline"):
        ER.evaluate_raster(None, z, cellsize=1.0, baseline="thinplate")
    with pytest.raises(ValueError, match="fallback"):
        ER.evaluate_raster(None, z, cellsize=1.0, fallback="biharmonic")      # out of scope: the fallback stays harmonic
    for b in ER.BASELINES:
        with pytest.raises(FileNotFoundError):
            ER.main(["--dem", "/nonexistent/in.asc", "--checkpoint", "ck.pth", "--baseline", b])
    with pytest.raises(SystemExit):
        ER.main(["--dem", "/nonexistent/in.asc", "--checkpoint", "ck.pth", "--baseline", "idw"])


def test_bench_tool_knows_the_method():
    src = open(os.path.join(ROOT, "tools", "fill_voids_bench.py")).read()
    assert '"--method"' in src and "vfill_bih_iter" in src and "ms_per_vcycle" in src


# ---- symbols --------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    L, lib = _lib()
    from tg_hip import ops as O
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "terragan_hip.h")).read(), flags=re.S)
    I, P, SZ = C.c_int, C.c_void_p, C.c_size_t
    want = {"tg_vfill_bih_ws_bytes": (SZ, [I, I]),
            "tg_vfill_bih_start": (I, [I, I, P, SZ, P, SZ, I, P]),
            "tg_vfill_bih_iter": (I, [I, I, P, SZ, P, SZ, I, P, P, P])}
    for name, sig in want.items():
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert decl, f"{name} not declared"
        assert len(decl.group(1).split(",")) == len(sig[1])
        assert L.SIGNATURES[name] == sig
        fn = getattr(lib, name)
        assert fn.argtypes == sig[1] and fn.restype == sig[0]
    assert re.search(r"TG_VFILL_BIH_MAX_INNER\s*=\s*8", txt)
    for name in ("vfill_bih_ws", "vfill_bih_start", "vfill_bih_iter"):
        assert callable(getattr(O, name))
