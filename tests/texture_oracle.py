"""numpy restatement of the second-difference spectrum (csrc/texture.hip): the semantics of
include/terragan_hip.h's tg_texture_compare, written with shifted slices and nothing from mvp_gan.

Octave j has the lag h = 2^j px; class 0 (axial) the unit steps (dy, dx) = (0, 1), (1, 0), class 1 (diagonal) (1, 1), (1, -1);
scale s = 2 j + class.  A triple (centre x, step u) counts when sel[x] and known[x] are nonzero and both arms x - hu, x + hu lie
inside the raster and are known.  Per triple in float64 from the float32 values: d = (s(x - hu) + s(x + hu)) - 2 s(x)."""
import numpy as np

OCTAVES, SCALES, NSUM = 5, 10, 3
STEPS = (((0, 1), (1, 0)), ((1, 1), (1, -1)))        # [class] -> unit steps (dy, dx)


def _views(a, dy, dx):
    """(centre, minus arm, plus arm) views of a for the offset (dy, dx), dy >= 0: the centres whose two arms lie inside; None when
    no centre has."""
    H, W = a.shape
    ax = abs(dx)
    if H - 2 * dy <= 0 or W - 2 * ax <= 0:
        return None
    c = a[dy:H - dy, ax:W - ax]
    minus = a[0:H - 2 * dy, ax - dx:W - ax - dx]
    plus = a[2 * dy:H, ax + dx:W - ax + dx]
    return c, minus, plus


def spectrum(z, p, sel, known, octaves=OCTAVES):
    """-> (counts int64 [SCALES], sums float64 [SCALES][NSUM]: of d_z d_z, d_p d_p, d_z d_p, abs_sums float64 [SCALES][NSUM]: the
    sums of the absolute values of the same terms).  Entries of octaves past `octaves` are zero."""
    assert 1 <= octaves <= OCTAVES
    z = np.asarray(z, np.float32)
    p = np.asarray(p, np.float32)
    assert z.ndim == 2 and p.shape == z.shape
    sel = np.asarray(sel) != 0
    known = np.asarray(known) != 0
    counts = np.zeros(SCALES, np.int64)
    sums = np.zeros((SCALES, NSUM), np.float64)
    abs_sums = np.zeros((SCALES, NSUM), np.float64)
    z64, p64 = z.astype(np.float64), p.astype(np.float64)
    for j in range(octaves):
        h = 1 << j
        for cls in range(2):
            s = 2 * j + cls
            for uy, ux in STEPS[cls]:
                dy, dx = h * uy, h * ux
                vk = _views(known, dy, dx)
                if vk is None:
                    continue
                ok = _views(sel, dy, dx)[0] & vk[0] & vk[1] & vk[2]
                zc, zm, zp = _views(z64, dy, dx)
                pc, pm, pp = _views(p64, dy, dx)
                with np.errstate(invalid="ignore", over="ignore"):
                    dz = ((zm + zp) - 2.0 * zc)[ok]
                    dp = ((pm + pp) - 2.0 * pc)[ok]
                    terms = (dz * dz, dp * dp, dz * dp)
                counts[s] += int(ok.sum())
                for q, t in enumerate(terms):
                    sums[s, q] += t.sum()
                    abs_sums[s, q] += np.abs(t).sum()
    return counts, sums, abs_sums
