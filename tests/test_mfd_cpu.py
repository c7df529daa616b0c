"""CPU checks of the multiple-flow-direction accumulation, the slope and the wetness index (csrc/mfd.hip,
mvp_gan/src/flow_routing.py): the two forms of the accumulation in tests/mfd_oracle.py against each other
bit for bit, the conditions the definition promises (an acyclic graph, mass conservation, A >= 1), hand-made cases with known
answers, the slope of a plane, host-side rejection and the CLI parser, all without a GPU."""
import os

import numpy as np
import pytest

from tests import flow_oracle as FO
from tests import mfd_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tg_mfd_ws_bytes", "tg_mfd_setup", "tg_mfd_sweep", "tg_mfd_finish", "tg_terrain_slope", "tg_wetness", "tg_wetness_compare")
MASS_RTOL = 1e-12                                       # the prototype stayed below 5e-14 with float64 fractions


@pytest.fixture(scope="module", autouse=True)
def contract():
    """The oracle implements what include/terragan_hip.h states."""
    txt = " ".join(open(os.path.join(ROOT, "include", "terragan_hip.h")).read().replace("* ", "").split())
    for name in NAMES:
        assert name + "(" in txt, name
    assert "valid iff d_j > 0 (a NaN never is)" in txt
    assert "S = the fp64 sum of the valid t_j in the order j = 0..7" in txt
    assert "A(p) = A(p) + f A(n_k): one fp64 multiply, one fp64 add, nothing fused" in txt
    assert "#define TG_MFD_MAX_EXPONENT 8 " in txt
    return txt


@pytest.mark.parametrize("name", list(MO.scenes()))
def test_two_forms_agree_and_conditions(name):
    """Kahn's order and the level-synchronous relaxation give the same float64 bits; Kahn visits every known pixel (mfd asserts
    it), mass is conserved to 1e-12 relative, A >= 1 on known pixels and 0 elsewhere."""
    for e in MO.EXPONENTS:
        z, nodata, fill, r, m = MO.scene_ref(name, e)
        known = r["known"]
        A2, rounds = MO.accumulate_relax(m["F"], known)
        assert np.array_equal(m["A"].view(np.uint64), A2.view(np.uint64)), (name, e)
        assert rounds == m["longest"] + 1
        n = int(known.sum())
        assert sum(m["counts"].values()) == n
        assert abs(m["mass_out"] - n) <= MASS_RTOL * n, (name, e, m["mass_out"], n)
        assert (m["A"][known] >= 1).all() and (m["A"][~known] == 0).all()
        print(name, e, m["counts"], "longest", m["longest"], "d8", r["longest"], "mass err", abs(m["mass_out"] - n) / n)


def test_scene_conditions():
    """What the GPU tests rely on: path lengths past the inner-round cap, the single pixels of the flats, the void."""
    _, _, _, r, m = MO.scene_ref("serpentine", 1)
    assert m["longest"] > 8000
    _, _, _, r, m = MO.scene_ref("spiral", 1)
    assert m["longest"] > 5000
    z, lake = FO.lake_scene()
    _, _, _, r, m = MO.scene_ref("lake", 1)
    assert (m["cls"][lake] == MO.SINGLE).all() and m["cls"][64, 64] == MO.DISPERSIVE     # the notch drops to the east
    _, _, _, r, m = MO.scene_ref("void", 1)
    assert int((~r["known"]).sum()) == 401 and not r["known"][0, 33]
    _, _, _, r, m = MO.scene_ref("unfilled", 1)
    pits = r["dir"] == FO.PIT
    assert pits.sum() > 0 and (m["cls"][pits] == MO.SINK).all()
    assert not m["F"][:, pits].any()                                     # a pit gives nothing, and what it holds leaves
    assert abs(m["mass_out"] - r["known"].sum()) <= MASS_RTOL * r["known"].sum()
    assert m["mass_out"] > m["A"][r["dir"] == FO.OUT].sum()


def test_plane():
    """z = -x: the sum of A down column x is H (x + 1) for every x."""
    H, W = 37, 53
    z = np.repeat(-np.arange(W, dtype=np.float32)[None, :], H, 0) + np.float32(1000)
    for e in MO.EXPONENTS:
        r, m = MO.route_mfd(z, fill=False, e=e)
        col = m["A"].sum(0)
        want = H * (np.arange(W) + 1.0)
        assert (np.abs(col - want) <= MASS_RTOL * want).all(), e


def test_ridge_and_valley():
    H, W = 21, 33
    y, x = np.mgrid[0:H, 0:W]
    ridge = (1000 - np.abs(x - 16)).astype(np.float32)                   # a one-pixel ridge along column 16
    for e in MO.EXPONENTS:
        r, m = MO.route_mfd(ridge, fill=False, e=e)
        assert (m["A"][:, 16] == 1.0).all()
    # a V-shaped valley whose floor falls to the south.  In two dimensions the sides spread over three rows of the floor, so the
    # floor holds the D8 count only where everything has arrived, at the mouth; along the floor A grows downstream.
    valley = (1000 + np.abs(x - 16) - 0.01 * y).astype(np.float32)
    for e in MO.EXPONENTS:
        r, m = MO.route_mfd(valley, fill=False, e=e)
        floor = m["A"][:, 16]
        assert r["acc"][-1, 16] == H * W and abs(floor[-1] - H * W) <= MASS_RTOL * H * W, e
        assert (np.diff(floor) > 0).all()
    # a valley one pixel wide (a single row): every pixel has one lower neighbour, so A is the D8 count everywhere, exactly
    row = (1000 + np.abs(np.arange(33) - 16)).astype(np.float32)[None, :]
    for e in MO.EXPONENTS:
        r, m = MO.route_mfd(row, fill=False, e=e)
        assert np.array_equal(m["A"], r["acc"].astype(np.float64)) and m["A"][0, 16] == 33, e


def test_fractions():
    """At exponent 1 a diagonal drop weighs exactly half a cardinal drop of the same size; cdiag is Quinn's."""
    assert MO.cdiag(1) == 0.5 and MO.cdiag(3) == 0.25
    z = np.full((3, 3), 10.0, np.float32)
    z[1, 2] = 8.0                                                        # E of the centre
    z[2, 2] = 8.0                                                        # SE of the centre
    r = FO.route(z, fill=False)
    F, S, cls = MO.fractions(r["w"], r["known"], r["dir"], 1)
    assert F[0][1, 1] == 2 * F[1][1, 1] and F[0][1, 1] + F[1][1, 1] == 1.0 and cls[1, 1] == MO.DISPERSIVE
    assert F[0][1, 1] == 2.0 / 3.0 and S[1, 1] == 3.0
    F8, _, _ = MO.fractions(r["w"], r["known"], r["dir"], 8)
    assert F8[1][1, 1] / F8[0][1, 1] == 2.0 ** -4.5
    for bad in (0, 9, 1.0, True, None):
        with pytest.raises(ValueError):
            MO.fractions(r["w"], r["known"], r["dir"], bad)


def test_slope_of_a_plane():
    H, W = 20, 24
    y, x = np.mgrid[0:H, 0:W]
    known = np.ones((H, W), bool)
    for p, q, c in ((0.25, -0.5, 1.0), (0.125, 0.375, 2.0), (1.0, 0.0, 0.5), (0.3, 0.7, 30.0)):
        z = (p * x + q * y).astype(np.float32)
        s = MO.slope(z, known, c)
        assert s.dtype == np.float32
        want = np.hypot(p, q) / c
        inner = s[1:-1, 1:-1]
        exact = float(p).is_integer() or (p * 8).is_integer()
        tol = 4 * np.finfo(np.float32).eps * want if exact else 2e-5 * want     # z itself is rounded for p = 0.3
        assert (np.abs(inner - want) <= tol).all(), (p, q, c)
    known[5, 5] = False
    s = MO.slope(z, known, 1.0)
    assert np.isnan(s[5, 5]) and np.isfinite(s[known]).all()


def test_twi_and_stats_oracle():
    acc = np.array([[1, 4], [16, 0]], np.float32)
    slp = np.array([[0.5, 1e-6], [np.nan, 1]], np.float32)
    known = np.array([[1, 1], [1, 0]], bool)
    t = MO.twi_ref(acc, slp, known, 2.0, 1e-3)
    assert t[0, 0] == np.log(4.0) and np.isnan(t[1, 1])
    assert t[0, 1] == np.log(8.0 / float(np.float32(1e-3))) == t[0, 1] and t[1, 0] == np.log(32.0 / float(np.float32(1e-3)))
    a = np.array([[1, 2], [np.nan, 4]], np.float32)
    b = np.array([[1.5, 1], [3, np.inf]], np.float32)
    assert MO.wetness_stats(np.ones((2, 2)), a, b) == (2, -0.5, 1.5, 1.25, np.float32(1))


# ---- host side ---------------------------------------------------------------------------------------------------------------
def test_python_rejects_bad_arguments():
    from mvp_gan.src.flow_routing import mfd_accumulation, terrain_slope, wetness_index
    z = np.zeros((4, 4), np.float32)
    for bad in (0, 9, 1.5, 2.0, True, "1", np.float64(2.0), np.bool_(True), np.int64(9)):
        with pytest.raises(ValueError, match="exponent"):
            mfd_accumulation(z, exponent=bad)
        with pytest.raises(ValueError, match="exponent"):
            wetness_index(z, exponent=bad)
    for bad in (0, -1e-3, float("nan"), float("inf"), 1e-60, None):
        with pytest.raises(ValueError, match="min_slope"):
            wetness_index(z, min_slope=bad)
    # numpy's integers and reals are numbers: check_* hand back plain Python values
    from mvp_gan.src.flow_routing import check_exponent, check_min_slope
    from tg_hip import ops as O
    for good in (4, np.int64(4), np.int32(4), np.uint8(4)):
        assert check_exponent(good) == 4 and type(check_exponent(good)) is int and O.mfd_cdiag(good) == 2.0 ** -2.5
    for good, want in ((0.01, 0.01), (np.float64(0.01), 0.01), (np.float32(0.01), float(np.float32(0.01))), (1, 1.0), (np.int64(2), 2.0)):
        assert check_min_slope(good) == want and type(check_min_slope(good)) is float
    with pytest.raises(ValueError, match="cellsize"):
        terrain_slope(z, cellsize=0)
    with pytest.raises(ValueError):
        mfd_accumulation(np.zeros((4,), np.float32))


def test_c_entry_points_reject_without_gpu():
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    lib = L.load()
    assert lib.tg_mfd_ws_bytes(0, 5) == 0 and lib.tg_mfd_ws_bytes(1 << 16, 1 << 15) == 0
    n = lib.tg_mfd_ws_bytes(130, 70)
    assert n >= 256 + 130 * 70 * 9 + 6 and lib.tg_mfd_ws_bytes(131, 70) > n
    # the layout exactly: 256 control bytes, the open plane and two mark planes of a byte per 64x64 tile, the donor bytes, S, and
    # 2048 partials of 4 doubles; each of the first five rounded up to 256 bytes
    up = lambda v: -(-v // 256) * 256
    for H, W in [(1, 1), (1, 2049), (2049, 1), (63, 65), (64, 64), (65, 63), (130, 70), (257, 1101), (1501, 2099), (4097, 513),
                 (8191, 8193), (32767, 3), (3, 32767), (32767, 32767), (46340, 46340), (1, (1 << 31) - 1)]:
        tiles = -(-H // 64) * -(-W // 64)
        assert lib.tg_mfd_ws_bytes(H, W) == 256 + 3 * up(tiles) + up(H * W) + up(8 * H * W) + 65536, (H, W)
    one, two = C.c_void_p(8), C.c_void_p(16)                             # non-null, never dereferenced: every call is refused
    for e in (0, 9):
        assert lib.tg_mfd_setup(one, one, one, 4, 4, e, 0.5, two, one, one, n, None) == -1
        assert b"exponent" in lib.tg_last_error()
        assert lib.tg_mfd_sweep(one, 4, 4, e, 0.5, 1, two, one, one, n, None) == -1
    assert lib.tg_mfd_setup(one, one, one, 4, 4, 1, 0.0, two, one, one, n, None) == -1 and b"cdiag" in lib.tg_last_error()
    need = lib.tg_mfd_ws_bytes(4, 4)
    assert lib.tg_mfd_setup(one, one, one, 4, 4, 1, 0.5, two, one, one, need - 1, None) == -1 and b"workspace" in lib.tg_last_error()
    assert lib.tg_mfd_sweep(one, 4, 4, 1, 0.5, 1, two, one, one, need - 1, None) == -1 and b"workspace" in lib.tg_last_error()
    assert lib.tg_mfd_sweep(one, 4, 4, 1, 0.5, 0, two, one, one, need, None) == -1
    assert lib.tg_mfd_finish(one, one, 4, 4, one, one, one, need - 1, None) == -1 and b"workspace" in lib.tg_last_error()
    assert lib.tg_wetness_compare(one, one, one, 4, 4, one, one, one, need - 1, None) == -1
    assert lib.tg_mfd_setup(None, one, one, 4, 4, 1, 0.5, two, one, one, need, None) == -1 and b"null" in lib.tg_last_error()
    assert lib.tg_terrain_slope(one, one, 4, 4, 0.0, one, None) == -1
    assert lib.tg_wetness(one, one, one, 4, 4, 1.0, 0.0, one, None) == -1 and b"min_slope" in lib.tg_last_error()
    assert lib.tg_wetness(one, one, one, 0, 4, 1.0, 1e-3, one, None) == -1


def test_wetness_row_assembly():
    """The pure halves of the wetness row: the dict from the kernel's numbers, and its place in assemble_compare."""
    import inspect
    from mvp_gan.src import evaluate_raster as ER
    bits = int(np.array([1.5], np.float32).view(np.uint32)[0])
    d = ER.assemble_wetness([4, bits], [-2.0, 3.0, 9.0])
    assert d == {"cells": 4, "bias": -0.5, "mae": 0.75, "rmse": 1.5, "max": 1.5}
    assert ER.assemble_wetness([0, 0], [0.0, 0.0, 0.0]) == {"cells": 0, "bias": None, "mae": None, "rmse": None, "max": None}
    assert "n/a" in ER.wetness_summary(ER.assemble_wetness([0, 0], [0.0, 0.0, 0.0])) and "MAE 0.75" in ER.wetness_summary(d)
    raw = {"idw": {"height": 1}, "nearest": {"height": 2}}
    infos = {"idw": {"a": 1}, "nearest": {"a": 2}}
    cmp = ER.assemble_compare(raw, infos)
    assert all("wetness" not in cmp[k] and set(cmp[k]) == {"height", "method", "fill"} for k in cmp)
    a, b = {"cells": 1}, {"cells": 2}
    cmp = ER.assemble_compare(raw, infos, None, None, None, {"idw": a, "nearest": b})
    assert cmp["idw"]["wetness"] is a and cmp["nearest"]["wetness"] is b and "flood" not in cmp["idw"] and "wetness" not in raw["idw"]
    cmp = ER.assemble_compare(raw, infos, wetness={"idw": a, "nearest": b}, flood={"idw": b, "nearest": a})
    assert cmp["idw"]["wetness"] is a and cmp["idw"]["flood"] is b
    sig = inspect.signature(ER.wetness_errors).parameters
    assert [(k, sig[k].default) for k in list(sig)[3:]] == [("cellsize", inspect.Parameter.empty), ("mask", None), ("nodata", None),
                                                            ("exponent", 1), ("min_slope", 1e-3)]
    for fn in (ER.evaluate_raster, ER.baseline_report, ER.compare_report):
        sig = inspect.signature(fn).parameters
        assert (sig["wetness"].default, sig["wetness_exponent"].default, sig["wetness_min_slope"].default) == (False, 1, 1e-3)


def test_cli_parser():
    from mvp_gan.src.flow_routing import MIN_SLOPE, parse_args
    base = ["--dem", "in.asc", "--dir-out", "d.asc", "--acc-out", "a.asc"]
    a = parse_args(base)
    assert a.mfd_acc_out is None and a.slope_out is None and a.twi_out is None and a.exponent == 1 and a.min_slope == MIN_SLOPE
    a = parse_args(base + ["--mfd-acc-out", "m.asc", "--exponent", "4", "--slope-out", "s.asc", "--twi-out", "t.asc",
                           "--min-slope", "0.01"])
    assert (a.mfd_acc_out, a.exponent, a.slope_out, a.twi_out, a.min_slope) == ("m.asc", 4, "s.asc", "t.asc", 0.01)
    for bad in (["--exponent", "4"], ["--mfd-acc-out", "m.asc", "--exponent", "9"], ["--mfd-acc-out", "m.asc", "--exponent", "0"],
                ["--min-slope", "0.01"], ["--twi-out", "t.asc", "--min-slope", "0"], ["--mfd-acc-out", "m.asc", "--exponent", "1.5"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    from mvp_gan.src.evaluate_raster import build_parser
    a = build_parser().parse_args(["--dem", "x.asc", "--pred", "p.asc", "--holes", "h.png", "--wetness", "--exponent", "4",
                                   "--min-slope", "0.01"])
    assert a.wetness and a.exponent == 4 and a.min_slope == 0.01
    a = build_parser().parse_args(["--dem", "x.asc", "--pred", "p.asc", "--holes", "h.png"])
    assert not a.wetness and a.exponent == 1
