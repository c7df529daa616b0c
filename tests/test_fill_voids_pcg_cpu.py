"""CPU checks of the conjugate-gradient solver of the harmonic void fill (fill_voids(solver="pcg"), csrc/voidfill.hip,
DESIGN.md section 8n): the numpy mirror of the V-cycle and of the PCG loop (tests/vfill_pcg_mirror.py, fp32 values, fp64 dots)
against a tight fp64 solve on the cases of section 8n up to 768 x 768, with the iteration counts it gives; the second
workspace's query against its host mirror; host-side rejection by the two new C entry points; `solver` validation in the four
Python functions; the CLI flag; the new symbols.  All without a GPU."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from tests import vfill_oracle as VO
from tests import vfill_pcg_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2e-5                        # max |u - u*| / range, the bound of tests/test_hip_fill_voids.py


def _terrain(H, W, seed, noise=0.3):
    rng = np.random.default_rng(seed)
    f = VO.harmonic_field(H, W, (120, 4, -3, 2, 1, 0.2), W / 2, H / 2, max(H, W) / 2)
    return (f + 6 * np.sin(np.arange(W) / 17.0)[None, :] * np.cos(np.arange(H) / 23.0)[:, None]
            + rng.normal(0, noise, (H, W))).astype(np.float32)


def _case(name):
    if name in M.ALIGNED:
        H, W, boxes = M.ALIGNED[name]
        return M.field(H, W).astype(np.float32), M.box_known(H, W, boxes)
    if name == "37x53 disc":
        return _terrain(37, 53, 2), ~VO.disc(37, 53, 18, 26, 9)
    if name == "257x129 1% known":
        return _terrain(257, 129, 3), np.random.default_rng(3).random((257, 129)) < 0.01
    if name == "257x129 edges and a corner":
        k = np.ones((257, 129), bool)
        k[:40, :30] = False
        k[200:, 100:] = False
        k[100:140, :12] = False
        return _terrain(257, 129, 3), k
    assert name == "1x300 runs"
    n = 300
    k = np.ones(n, bool)
    k[: n // 20] = False
    k[n // 3: n // 3 + n // 4] = False
    k[n - 7:] = False
    k[n // 2 + 50::97] = False
    return _terrain(1, n, 1), k.reshape(1, n)


# the mirror's own iteration counts (DESIGN.md section 8n lists them next to the GPU's)
PCG_ITERATIONS = {
    "37x53 disc": 7,
    "257x129 1% known": 10,
    "257x129 edges and a corner": 9,
    "1x300 runs": 14,
    "300x300 void [64:192, 128:256]": 9,
    "512x512 void [128:384, 128:384]": 9,
    "512x512 left half": 9,
    "768x768 missing tiles": 10,
}


@pytest.mark.parametrize("name", list(PCG_ITERATIONS))
def test_mirror_pcg_against_fp64_solve(name):
    z, k = _case(name)
    rng = float(z[k].max()) - float(z[k].min())
    # the tight solve: the same loop in fp64 run to stagnation, accepted by the oracle's residual; on the small cases it is
    # also the oracle's dense solve
    ref, _ = M.solve_pcg(z, k, tol=0.0, max_cycles=30, dt=np.float64)
    assert np.abs(VO.residual(ref, k)).max() <= 1e-12 * rng
    assert np.array_equal(ref[k], z[k].astype(np.float64))
    if (~k).sum() <= VO.MAX_COMPONENT and name != "257x129 1% known":
        assert np.abs(VO.solve(z, k) - ref).max() <= 1e-9 * rng
    out, info = M.solve_pcg(z, k)
    print(name, info["cycles"], info["history"])
    assert info["converged"] and info["restarts"] == 0
    assert np.array_equal(out[k], z[k])
    assert np.abs(out.astype(np.float64) - ref).max() <= BOUND * rng
    assert info["cycles"] == PCG_ITERATIONS[name]
    # the plain cycle of the same mirror needs at least as many: it has not converged one cycle earlier
    _, mg = M.solve_mg(z, k, max_cycles=info["cycles"] - 1)
    assert not mg["converged"], mg


def test_mirror_plain_cycle_stalls_on_aligned_voids():
    # the premise of the solver: on the 300 x 300 aligned void the change of the plain cycle contracts by 0.75 or worse
    z, k = _case("300x300 void [64:192, 128:256]")
    _, mg = M.solve_mg(z, k, max_cycles=16)
    h = mg["history"]
    assert not mg["converged"] and h[-1] / h[-2] > 0.7


@pytest.mark.parametrize("side", ["left", "right"])
def test_border_field_is_the_exact_fill_of_voids_on_the_border(side):
    H, W = 40, 56
    f = M.border_field(H, W, side, (50, 3, -0.2, 0.01))
    k = np.ones((H, W), bool)
    if side == "left":
        k[:, :20] = False                                  # touches the left, top and bottom edges
    else:
        k[:13, 30:] = False                                # the top right corner
        k[20:30, 10:25] = False
    assert np.abs(VO.residual(f, k)).max() <= 1e-10 * np.abs(f).max()
    np.testing.assert_allclose(VO.solve(f, k, max_component=10 ** 4), f, rtol=0, atol=1e-9 * np.abs(f).max())


def test_mirror_guards():
    z = _terrain(12, 9, 4)
    k = np.zeros(z.shape, bool)
    k[3, 4] = True
    out, info = M.solve_pcg(z, k)                          # one known pixel: range 0, rho = 0
    assert info["converged"] and info["change"] == 0.0 and np.array_equal(out, np.full(z.shape, z[3, 4]))
    out, info = M.solve_pcg(z, np.ones(z.shape, bool))
    assert info["cycles"] == 0 and info["converged"] and np.array_equal(out, z)


# ---- the second workspace -------------------------------------------------------------------------------------------
def _lib():
    from tg_hip import lib as L
    return L, L.load()


SIZES = [(1, 1), (1, 2), (2, 1), (16, 16), (17, 16), (33, 65), (64, 64), (65, 64), (37, 53), (257, 129), (1500, 2100),
         (4096, 4096), (4097, 4095), (8192, 8192), (8193, 8191), (1, 300000), (300000, 1)]


@pytest.mark.parametrize("H,W", SIZES)
def test_pcg_ws_query_matches_the_mirror_layout(H, W):
    from mvp_gan.src.fill_voids import vfill_layout, vfill_pcg_layout
    _, lib = _lib()
    lay, total = vfill_pcg_layout(H, W)
    assert lib.tg_vfill_pcg_ws_bytes(H, W) == total
    assert lay["tiles"] == vfill_layout(H, W)[0][0]["tiles"]
    n = H * W
    spans = [(0, 256)] + [(lay[key], 4 * n) for key in ("r", "z", "p0", "p1", "d")] + [(o, 8 * lay["tiles"]) for o in lay["part"]]
    assert len(lay["part"]) == 3
    spans.sort()
    for (a, na), (b, _) in zip(spans, spans[1:]):
        assert a + na <= b
    assert spans[-1][0] + spans[-1][1] <= total
    assert all(o % 256 == 0 for o, _ in spans)
    # the first workspace is untouched by the new solver
    assert lib.tg_vfill_ws_bytes(H, W) >= vfill_layout(H, W)[1]


def test_pcg_ws_query_rejects_bad_shapes():
    _, lib = _lib()
    for H, W in ((0, 5), (5, 0), (-1, 3), (1 << 16, 1 << 15)):
        assert lib.tg_vfill_ws_bytes(H, W) == 0
        assert lib.tg_vfill_pcg_ws_bytes(H, W) == 0


def test_c_entry_points_reject_without_gpu():
    L, lib = _lib()
    f = [C.c_void_p(0x1000 * (i + 1)) for i in range(4)]
    ws, pws = C.c_void_p(0x100000), C.c_void_p(0x200000)       # 256-byte aligned, never dereferenced

    def err(rc, msg, code=(-1, -3)):
        assert rc in code and msg in lib.tg_last_error(), (rc, lib.tg_last_error())

    nb, npb = lib.tg_vfill_ws_bytes(8, 8), lib.tg_vfill_pcg_ws_bytes(8, 8)
    start = lambda H, W, w, b, p, pb: lib.tg_vfill_pcg_start(H, W, w, b, p, pb, None)
    it = lambda H, W, w, b, p, pb, ch=f[0], rs=f[1]: lib.tg_vfill_pcg_iter(H, W, w, b, p, pb, ch, rs, None)
    for H, W in ((0, 5), (5, 0), (-1, 5), (1 << 16, 1 << 15)):
        err(start(H, W, ws, 1 << 30, pws, 1 << 30), b"H*W < 2^31")
        err(it(H, W, ws, 1 << 30, pws, 1 << 30), b"H*W < 2^31")
    for call in (start, it):
        err(call(8, 8, None, nb, pws, npb), b"null pointer")
        err(call(8, 8, ws, nb, None, npb), b"null pointer")
        err(call(8, 8, C.c_void_p(0x100004), nb, pws, npb), b"aligned")
        err(call(8, 8, ws, nb, C.c_void_p(0x200010), npb), b"aligned")
        for b in (nb - 1, 0):
            err(call(8, 8, ws, b, pws, npb), b"workspace", (-3,))
        for b in (npb - 1, 0):
            err(call(8, 8, ws, nb, pws, b), b"pcg workspace", (-3,))
        # workspaces sized for a smaller raster are short for a larger one
        err(call(300, 200, ws, lib.tg_vfill_ws_bytes(300, 200), pws, lib.tg_vfill_pcg_ws_bytes(150, 100)), b"pcg workspace", (-3,))
        err(call(300, 200, ws, lib.tg_vfill_ws_bytes(150, 100), pws, lib.tg_vfill_pcg_ws_bytes(300, 200)), b"workspace", (-3,))
    err(it(8, 8, ws, nb, pws, npb, ch=None), b"null pointer")
    err(it(8, 8, ws, nb, pws, npb, rs=None), b"null pointer")


# ---- Python API -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["cg", None, "", "PCG", 1])
def test_python_rejects_unknown_solvers(solver):
    from mvp_gan.src.evaluate_raster import evaluate_raster
    from mvp_gan.src.fill_voids import SOLVERS, fill_voids
    from mvp_gan.src.inpaint_raster import inpaint_raster
    from mvp_gan.src.seam_correct import correct_seams
    assert SOLVERS == ("mg", "pcg")
    z = np.zeros((64, 64), np.float32)
    with pytest.raises(ValueError, match="fill_voids: solver"):
        fill_voids(z, solver=solver)
    with pytest.raises(ValueError, match="correct_seams: solver"):
        correct_seams(z, z, solver=solver)
    with pytest.raises(ValueError, match="inpaint_raster: solver"):
        inpaint_raster(None, z, solver=solver)
    with pytest.raises(ValueError, match="evaluate_raster: solver"):
        evaluate_raster(None, z, cellsize=1.0, solver=solver)


def test_default_solver_is_mg():
    import inspect
    from mvp_gan.src.evaluate_raster import baseline_report, evaluate_raster
    from mvp_gan.src.fill_voids import fill_voids
    from mvp_gan.src.inpaint_raster import inpaint_raster
    from mvp_gan.src.seam_correct import correct_seams
    for fn in (fill_voids, correct_seams, inpaint_raster, evaluate_raster, baseline_report):
        assert inspect.signature(fn).parameters["solver"].default == "mg", fn


# ---- CLI flags ------------------------------------------------------------------------------------------------------
def test_fill_voids_and_seam_cli_parse_the_solver():
    from mvp_gan.src.fill_voids import build_parser
    from mvp_gan.src.seam_correct import build_parser as seam_parser
    assert build_parser().parse_args(["--dem", "a.asc", "--out", "o.asc"]).solver == "mg"
    assert build_parser().parse_args(["--dem", "a.asc", "--out", "o.asc", "--solver", "pcg"]).solver == "pcg"
    base = ["--dem", "a.asc", "--filled", "f.asc", "--out", "o.asc"]
    assert seam_parser().parse_args(base).solver == "mg"
    assert seam_parser().parse_args(base + ["--solver", "pcg"]).solver == "pcg"
    for p, b in ((build_parser(), ["--dem", "a.asc", "--out", "o.asc"]), (seam_parser(), base)):
        with pytest.raises(SystemExit):
            p.parse_args(b + ["--solver", "cg"])


@pytest.mark.parametrize("module,base", [
    ("fill_voids", ["--dem", "/nonexistent/in.asc", "--out", "o.asc"]),
    ("seam_correct", ["--dem", "/nonexistent/in.asc", "--filled", "f.asc", "--out", "o.asc"]),
    ("inpaint_raster", ["--dem", "/nonexistent/in.asc", "--checkpoint", "ck.pth", "--out", "o.asc", "--fallback", "laplace"]),
    ("evaluate_raster", ["--dem", "/nonexistent/in.asc", "--checkpoint", "ck.pth", "--baseline", "laplace"]),
])
def test_solver_flag_parses_in_the_four_clis(module, base):
    mod = importlib.import_module(f"mvp_gan.src.{module}")
    with pytest.raises(SystemExit):
        mod.main(base + ["--solver", "cg"])
    for s in ("mg", "pcg"):
        with pytest.raises(FileNotFoundError):                 # the flag parses; the raster is read next
            mod.main(base + ["--solver", s])


def test_bench_tool_knows_the_solver_and_the_missing_tile_scene():
    import importlib.util
    spec = importlib.util.spec_from_file_location("fill_voids_bench", os.path.join(ROOT, "tools", "fill_voids_bench.py"))
    fb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fb)                            # puts tools/ on sys.path for raster_bench
    z, keep = fb.scene(512, 512, "tiles")
    assert z.shape == keep.shape == (512, 512)
    assert abs((keep == 0).mean() - 6 / 64) < 1e-9
    holes = np.argwhere(keep == 0)
    assert (holes.min(0) % 64 == 0).all() and keep[64:128, 64:192].sum() == 0


# ---- symbols --------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    L, lib = _lib()
    from tg_hip import ops as O
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "terragan_hip.h")).read(), flags=re.S)
    I, P, SZ = C.c_int, C.c_void_p, C.c_size_t
    want = {"tg_vfill_pcg_ws_bytes": (SZ, [I, I]),
            "tg_vfill_pcg_start": (I, [I, I, P, SZ, P, SZ, P]),
            "tg_vfill_pcg_iter": (I, [I, I, P, SZ, P, SZ, P, P, P])}
    for name, sig in want.items():
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert decl, f"{name} not declared"
        assert len(decl.group(1).split(",")) == len(sig[1])
        assert L.SIGNATURES[name] == sig
        fn = getattr(lib, name)
        assert fn.argtypes == sig[1] and fn.restype == sig[0]
    for name in ("vfill_pcg_ws", "vfill_pcg_start", "vfill_pcg_iter"):
        assert callable(getattr(O, name))
