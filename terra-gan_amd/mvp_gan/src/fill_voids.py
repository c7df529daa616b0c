"""Fill the voids of a DSM by harmonic (Laplace) interpolation on the GPU (csrc/voidfill.hip).

The plain interpolation every DEM void-fill tool offers (MATLAB's regionfill solves the same equation): a baseline to score the
GAN against, and a fill for the voids no inpainting window reaches.

  - known K: mask != 0 (if given), finite, and != nodata (if given; a NaN nodata is ignored), the rule of inpaint_raster; with
    `objects` (an object_mask.ObjectSpec, which needs `cellsize`) the object_mask keep mask replaces `mask`;
  - every other pixel p is unknown and satisfies sum_{q in N4(p)} (u_q - u_p) = 0 over its 4-neighbours inside the raster
    (a natural, Neumann, border), with u = z on K; when K is not empty the solution is unique;
  - known pixels come back bit for bit; when K is empty every pixel is NaN and info["unfilled"] = H * W;
  - V-cycles run until the largest change of one cycle over the unknowns is at most `tol` (default 1e-6 x the range of z
    over K), at most `max_cycles`; running out is not an error: info["converged"] is then False;
  - solver="pcg" runs flexible conjugate gradients with the same V-cycle as the preconditioner: one
    iteration is one cycle, and `tol`, `max_cycles`, info["cycles"] and info["change"] (the largest step of an iteration)
    keep their meaning.  It is the solver for large and for tile-aligned voids (a missing tile of a mosaic), on which the
    plain cycle converges slowly or not at all; info gains "solver" and "restarts".  The default "mg" is unchanged.

  - method="biharmonic" fills with the curvature-minimising (thin-plate, minimum-curvature) surface instead (DESIGN.md
    section 8q): the unknowns minimise the sum of (sum_q (u_q - u_p))^2 over themselves and their 4-neighbours, so the fill
    meets the terrain in height and slope and carries ridges and valleys across a void; off the raster border it reproduces
    every cubic.  Conjugate gradients on the normal equations (the state in fp64), preconditioned by two approximate Laplace
    solves of `inner` V-cycles each: `max_cycles` (default 200) and info["cycles"] count outer iterations, info["vcycles"]
    the V-cycles (2 x inner per iteration and for the start); `solver` is validated and unused.

Two calls on the same inputs return bitwise-equal rasters and equal info.

CLI: python -m mvp_gan.src.fill_voids --dem in.asc [--mask m.png|m.asc] [--nodata v] [--remove-objects [spec flags]]
         [--tol t] [--max-cycles n] [--solver mg|pcg] [--method laplace|biharmonic] [--inner k] --out out.asc
"""
import argparse
import math

import numpy as np
import torch

from . import raster_args as R

METHODS = ("laplace", "biharmonic")
MAX_CYCLES = {"laplace": 50, "biharmonic": 200}    # what max_cycles=None resolves to
INNER = 3                      # V-cycles of one approximate Laplace solve of the biharmonic preconditioner
MAX_INNER = 8
SOLVERS = ("mg", "pcg")
CMAX = 16                      # coarsest level: longer side at most this
TILE_Y, TILE_X = 32, 64        # tiles of the level passes
ALIGN = 256
MAX_LEVELS = 32


# ---- host-side mirror of the level plan and workspace layout (tg_vfill_ws_bytes, tg_vfill_levels) ---------------------
def vfill_levels(H, W):
    """[(H_l, W_l)]: halve with ceil until the longer side is at most CMAX."""
    H, W = int(H), int(W)
    out = [(H, W)]
    while max(out[-1]) > CMAX:
        h, w = out[-1]
        out.append(((h + 1) // 2, (w + 1) // 2))
    return out


def _al(n):
    return -(-n // ALIGN) * ALIGN


def vfill_layout(H, W):
    """-> (levels [dict: H, W, tiles, flags, list, u0, u1, f byte offsets], total bytes) of the workspace."""
    off = ALIGN                                         # header: tile counters, statistics, offset
    out = []
    for l, (h, w) in enumerate(vfill_levels(H, W)):
        n = h * w
        tiles = -(-h // TILE_Y) * -(-w // TILE_X)
        lv = {"H": h, "W": w, "tiles": tiles}
        lv["flags"] = off
        off += _al(n)
        lv["list"] = off
        off += _al(4 * tiles)
        lv["u0"] = off
        off += _al(4 * n)
        lv["u1"] = off
        off += _al(4 * n)
        lv["f"] = None
        if l:
            lv["f"] = off
            off += _al(4 * n)
        out.append(lv)
    return out, off


def vfill_pcg_layout(H, W):
    """-> (dict: r, z, p0, p1, d, part (3 offsets: p.Ap, r'.z, r'.z' by tile id) byte offsets, total bytes) of the second
    workspace of the pcg solver (tg_vfill_pcg_ws_bytes); the scalars sit in the first ALIGN bytes."""
    n = int(H) * int(W)
    tiles = -(-int(H) // TILE_Y) * -(-int(W) // TILE_X)
    off = ALIGN
    out = {"tiles": tiles}
    for k in ("r", "z", "p0", "p1", "d"):
        out[k] = off
        off += _al(4 * n)
    out["part"] = []
    for _ in range(3):
        out["part"].append(off)
        off += _al(8 * tiles)
    return out, off


# the header of the workspace (VfHdr of csrc/voidfill.hip, pinned there by static_asserts): its first bytes
VFILL_HDR = np.dtype([("lo_key", "<u4"), ("hi_key", "<u4"), ("known", "<u8"), ("c", "<f4"), ("_pad", "<i4"),
                      ("ntiles", "<i4", (MAX_LEVELS,))])

# the scalar block of the conjugate gradients (VfPcgScal of csrc/voidfill.hip, pinned there by static_asserts): the first bytes
# of the pcg workspace, and the blocks at sc_out (outer loop) and sc_in (inner solve) of the biharmonic workspace
VFILL_PCG_SCAL = np.dtype([("rho", "<f8"), ("pap", "<f8"), ("rz_old", "<f8"), ("rz_new", "<f8"), ("alpha", "<f4"), ("beta", "<f4"),
                           ("restarts", "<u4"), ("restart", "<u4"), ("parity", "<u4"), ("_pad", "<u4")])


def vfill_bih_layout(H, W):
    """-> (dict: sc_out, sc_in (scalars), xa, xb, r (fp64), rf, t, z, p0, p1 (fp32, outer loop), e0, e1, ri, zi, q0, q1, d (fp32,
    inner solve), part (6 offsets: the outer p.Ap, r'.z, r'.z' by tile id, then the inner solve's) byte offsets, total bytes)
    of the workspace of the biharmonic fill (tg_vfill_bih_ws_bytes)."""
    n = int(H) * int(W)
    tiles = -(-int(H) // TILE_Y) * -(-int(W) // TILE_X)
    out = {"tiles": tiles, "sc_out": 0, "sc_in": ALIGN}
    off = 2 * ALIGN
    for k in ("xa", "xb", "r"):
        out[k] = off
        off += _al(8 * n)
    for k in ("rf", "t", "z", "p0", "p1", "e0", "e1", "ri", "zi", "q0", "q1", "d"):
        out[k] = off
        off += _al(4 * n)
    out["part"] = []
    for _ in range(6):
        out["part"].append(off)
        off += _al(8 * tiles)
    return out, off


def check_solver(solver, who="fill_voids"):
    if not isinstance(solver, str) or solver not in SOLVERS:
        raise ValueError(f"{who}: solver {solver!r} must be one of {SOLVERS}")
    return solver


def check_inner(inner, who="fill_voids"):
    if isinstance(inner, bool) or not isinstance(inner, (int, np.integer)) or not 1 <= inner <= MAX_INNER:
        raise ValueError(f"{who}: inner {inner!r} must be an integer in 1..{MAX_INNER}")
    return int(inner)


def resolve_max_cycles(max_cycles, method):
    """max_cycles=None: 50 V-cycles for "laplace", 200 outer iterations for "biharmonic"."""
    return MAX_CYCLES[method] if max_cycles is None else max_cycles


# ---- validation -----------------------------------------------------------------------------------------------------
def check_args(dem, mask, method, tol, max_cycles, objects, cellsize, who="fill_voids"):
    """Host-side rejection before any launch; -> (H, W, cellsize or None)."""
    shape = R.raster_shape(dem, mask, who)
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError(f"{who}: method {method!r} must be one of {METHODS}")
    max_cycles = resolve_max_cycles(max_cycles, method)
    if tol is not None:
        try:
            t = float(tol)
        except (TypeError, ValueError):
            t = math.nan
        if not math.isfinite(t) or t < 0:
            raise ValueError(f"{who}: tol {tol!r} must be finite and >= 0")
    if isinstance(max_cycles, bool) or not isinstance(max_cycles, (int, np.integer)) or max_cycles < 1:
        raise ValueError(f"{who}: max_cycles {max_cycles!r} must be an integer >= 1")
    c = None
    if objects is not None:
        try:
            c = R.cellsize(cellsize, who)
        except ValueError:
            raise ValueError(f"{who}: objects need a cellsize, finite and > 0, got {cellsize!r}") from None
        objects.check()
    return shape[0], shape[1], c


# ---- the fill -------------------------------------------------------------------------------------------------------
@torch.no_grad()
def fill_voids(dem, mask=None, *, nodata=None, method="laplace", tol=None, max_cycles=None, objects=None, cellsize=None,
               solver="mg", inner=INNER):
    """dem: float32 [H][W] in metres (numpy or HIP tensor); mask: same shape, nonzero = known (optional).
    method: "laplace" (harmonic) or "biharmonic" (thin-plate; `inner` V-cycles per approximate Laplace solve).
    solver: "mg" (V-cycles) or "pcg" (conjugate gradients around the V-cycle; one iteration counts as one cycle).
    max_cycles: None = 50 for "laplace", 200 (outer iterations) for "biharmonic".
    Returns (raster float32 HIP tensor [H][W], info dict: unknown, unfilled, cycles, change, tol, converged, levels, with
    objects the object_mask info under "objects", with solver="pcg" also solver and restarts, and with method="biharmonic"
    method, inner, restarts and vcycles)."""
    from tg_hip import ops as O
    H, W, c = check_args(dem, mask, method, tol, max_cycles, objects, cellsize)
    check_solver(solver)
    inner = check_inner(inner)
    max_cycles = resolve_max_cycles(max_cycles, method)
    bih = method == "biharmonic"
    z, m, nodata, device = R.upload(dem, mask, nodata, "fill_voids")
    oinfo = None
    if objects is not None:
        from .object_mask import object_mask
        _, m, oinfo = object_mask(z, m, nodata=nodata, cellsize=c, spec=objects)
    ws = O.vfill_ws(H, W, device)
    st = O.vfill_setup(z, m, nodata, ws).cpu().tolist()        # the one sync before the cycles
    known, unknown = int(st[0]), int(st[1])
    rng = R.bits_f32(st[3]) - R.bits_f32(st[2]) if known else 0.0
    t = 1e-6 * rng if tol is None else float(tol)
    cycles, change, converged, restarts, vcycles = 0, 0.0, known > 0, 0, 0
    if known and unknown and bih:
        converged = False
        bws = O.vfill_bih_ws(H, W, device)
        O.vfill_bih_start(H, W, ws, bws, inner)
        vcycles = 2 * inner
        st = torch.zeros(2, dtype=torch.int32, device=device)  # change bits, restarts
        while cycles < max_cycles:
            O.vfill_bih_iter(H, W, ws, bws, inner, st)
            cycles += 1
            vcycles += 2 * inner
            change = R.bits_f32(st[0].item())                    # one read per outer iteration
            if change <= t:
                converged = True
                break
        restarts = int(st[1].item())
    elif known and unknown and solver == "pcg":
        converged = False
        pws = O.vfill_pcg_ws(H, W, device)
        O.vfill_pcg_start(H, W, ws, pws)
        st = torch.zeros(2, dtype=torch.int32, device=device)  # change bits, restarts
        while cycles < max_cycles:
            O.vfill_pcg_iter(H, W, ws, pws, st)
            cycles += 1
            change = R.bits_f32(st[0].item())                    # one read per iteration
            if change <= t:
                converged = True
                break
        restarts = int(st[1].item())
    elif known and unknown:
        converged = False
        ch = torch.empty(1, dtype=torch.int32, device=device)
        while cycles < max_cycles:
            O.vfill_cycle(H, W, ws, ch)
            cycles += 1
            change = R.bits_f32(ch.item())                       # one read per cycle
            if change <= t:
                converged = True
                break
    out = O.vfill_finish(z, ws)
    info = {"unknown": unknown, "unfilled": 0 if known else H * W, "cycles": cycles, "change": change, "tol": t,
            "converged": converged, "levels": len(vfill_levels(H, W))}
    if solver == "pcg" and not bih:
        info["solver"] = solver
        info["restarts"] = restarts
    if bih:
        info.update(method=method, inner=inner, restarts=restarts, vcycles=vcycles)
    if oinfo is not None:
        info["objects"] = oinfo
    return out, info


# ---- CLI ------------------------------------------------------------------------------------------------------------
class _Unset(int):
    """The --max-cycles default: 50 as ever, told apart from a given 50 so that --method decides what it resolves to."""


def build_parser():
    from .object_mask import add_spec_args
    ap = argparse.ArgumentParser(description="Fill the voids of an ESRI ASCII grid DSM by harmonic (Laplace) interpolation.")
    ap.add_argument("--dem", required=True, help="input .asc raster (NODATA_value cells are voids)")
    ap.add_argument("--mask", help="optional mask (.png or .asc) of the raster's size: nonzero = known, 0 = void")
    ap.add_argument("--nodata", type=float, help="nodata value (default: the .asc header's NODATA_value)")
    ap.add_argument("--remove-objects", action="store_true",
                    help="find above-ground objects (cellsize from the header) and fill them too: bare earth")
    add_spec_args(ap)
    ap.add_argument("--tol", type=float, help="stop when a cycle changes no void pixel by more (default 1e-6 x range)")
    ap.add_argument("--max-cycles", type=int, default=_Unset(MAX_CYCLES["laplace"]),
                    help="default 50 V-cycles (laplace) or 200 outer iterations (biharmonic)")
    ap.add_argument("--method", choices=METHODS, default="laplace",
                    help="laplace: harmonic fill; biharmonic: minimum-curvature (thin-plate) fill")
    ap.add_argument("--inner", type=int, default=INNER,
                    help="biharmonic: V-cycles per approximate Laplace solve of the preconditioner (1..8)")
    ap.add_argument("--solver", choices=SOLVERS, default="mg",
                    help="mg: V-cycles; pcg: conjugate gradients around the V-cycle, for large or tile-aligned voids")
    ap.add_argument("--out", required=True, help="output .asc raster")
    return ap


def main(argv=None):
    from .asc import read_inputs, with_nodata, write_asc
    from .object_mask import spec_from_args
    ap = build_parser()
    a = ap.parse_args(argv)
    dem, header, mask, nodata, cellsize = read_inputs(a)
    objects = spec_from_args(a) if a.remove_objects else None
    max_cycles = None if isinstance(a.max_cycles, _Unset) else a.max_cycles
    out, info = fill_voids(dem, mask, nodata=nodata, tol=a.tol, max_cycles=max_cycles, objects=objects,
                           cellsize=cellsize, solver=a.solver, method=a.method, inner=a.inner)
    write_asc(a.out, out.cpu().numpy(), with_nodata(header) if info["unfilled"] else header)
    print(f"{a.out}: {info['unknown']} void pixels, {info['cycles']} cycles, converged {info['converged']}, "
          + (f"method {a.method}, {info['vcycles']} V-cycles" if a.method == "biharmonic" else f"solver {a.solver}"))
    if not info["converged"]:
        print(f"warning: not converged: last change {info['change']:.3g} > tol {info['tol']:.3g} after {info['cycles']} "
              "cycles" if info["unknown"] and info["unfilled"] == 0 else "warning: nothing is known: every pixel is NaN")
    return info


if __name__ == "__main__":
    main()
