"""The premise of the sparse trunk backward, checked in float32 on the CPU with the pieces and the summation order of
the kernels (csrc/wino.inc, csrc/wino44.inc):
  F(2x2,3x3)  an output pixel is a function of its own 3x3 input window ONLY -- whatever the rest of the 4x4 patch holds, NaN
              included, the pixel keeps its bits.  Tiles next to unwritten memory therefore keep exact values on every pixel
              whose window is valid, and wino_pipe_kernel may run on a tile list.
  F(4x4,3x3)  every output of a tile is a sum over all six patch rows and columns whose out-of-window terms cancel only in exact
              arithmetic: the same experiment gives NaN.  wino44_kernel cannot be made tile-sparse bit for bit."""
import numpy as np

f32 = np.float32


# ---- F(2x2,3x3) in the kernel's order ------------------------------------------------------------------------------------------
def _g2(g):
    """U = G g Gt, G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1] (wino_weights_kernel: rows first, then columns)."""
    def t(v0, v1, v2):
        return [v0, f32(0.5) * (v0 + v1 + v2), f32(0.5) * (v0 - v1 + v2), v2]
    rows = [t(g[0][j], g[1][j], g[2][j]) for j in range(3)]          # rows[j][a]
    return [[t(rows[0][a], rows[1][a], rows[2][a])[b] for b in range(4)] for a in range(4)]


def _v2(d):
    """V = Bt d B as wino_pipe_kernel's thread forms it: row a = d[r0] + d[r1] * s1, then t0-t2, t1+t2, t2-t1, t1-t3."""
    V = []
    for a in range(4):
        r0 = 0 if a == 0 else (2 if a == 2 else 1)
        r1 = 3 if a == 3 else (1 if a == 2 else 2)
        s1 = f32(1.0) if a == 1 else f32(-1.0)
        t = [d[r0][j] + d[r1][j] * s1 for j in range(4)]
        V.append([t[0] - t[2], t[1] + t[2], t[2] - t[1], t[1] - t[3]])
    return V


def _y2(patches, weights):
    """patches [C][4][4], weights [C][3][3] -> the 2x2 outputs: 16 accumulators over the channels (the MFMA K loop, in order),
    row sums s[a][j], and the two halves' exchange: row 0 = (s0 + s1) + s2, row 1 = (-s2 - s3) + s1."""
    acc = [[f32(0.0)] * 4 for _ in range(4)]
    for d, g in zip(patches, weights):
        V, U = _v2(d), _g2(g)
        for a in range(4):
            for b in range(4):
                acc[a][b] = acc[a][b] + V[a][b] * U[a][b]
    s = [[acc[a][0] + acc[a][1] + acc[a][2], acc[a][1] - acc[a][2] - acc[a][3]] for a in range(4)]
    return [[(s[0][j] + s[1][j]) + s[2][j] for j in range(2)], [(-s[2][j] - s[3][j]) + s[1][j] for j in range(2)]]


def _rand(rng, *shape):
    return rng.standard_normal(shape).astype(f32)


def test_f22_output_pixel_sees_only_its_window():
    rng = np.random.default_rng(0)
    with np.errstate(invalid="ignore"):
        for _ in range(10):
            C = 5
            d, g = _rand(rng, C, 4, 4), _rand(rng, C, 3, 3)
            ref = _y2(d, g)
            direct = [[sum(float(np.sum(d[c, i:i + 3, j:j + 3].astype(np.float64) * g[c])) for c in range(C)) for j in range(2)]
                      for i in range(2)]
            for i in range(2):
                for j in range(2):
                    assert abs(float(ref[i][j]) - direct[i][j]) < 1e-4          # (the model computes the convolution)
                    poisoned = np.full_like(d, np.nan)
                    poisoned[:, i:i + 3, j:j + 3] = d[:, i:i + 3, j:j + 3]
                    y = _y2(poisoned, g)[i][j]
                    assert np.isfinite(y)
                    assert np.float32(y).tobytes() == np.float32(ref[i][j]).tobytes(), (i, j)
                    # ... and garbage of any finite kind outside the window changes nothing either
                    junk = (_rand(rng, C, 4, 4) * f32(1e30)).astype(f32)
                    junk[:, i:i + 3, j:j + 3] = d[:, i:i + 3, j:j + 3]
                    assert np.float32(_y2(junk, g)[i][j]).tobytes() == np.float32(ref[i][j]).tobytes(), (i, j)


# ---- F(4x4,3x3): wino44.inc's matrices -----------------------------------------------------------------------------------------
BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                [0, 4, 0, -5, 0, 1]], dtype=f32)
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
               [0, 0, 1]], dtype=f32)
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=f32)


def _mm(A, B):
    """Matrix product that skips structural zeros of the constant matrix A / B (the kernels never multiply by them)."""
    out = np.zeros((A.shape[0], B.shape[1]), dtype=f32)
    for i in range(A.shape[0]):
        for j in range(B.shape[1]):
            s = f32(0.0)
            for k in range(A.shape[1]):
                s = s + A[i, k] * B[k, j]
            out[i, j] = s
    return out


def _mm_const_left(Cm, X):
    out = np.zeros((Cm.shape[0], X.shape[1]), dtype=f32)
    for i in range(Cm.shape[0]):
        for j in range(X.shape[1]):
            s = f32(0.0)
            for k in range(Cm.shape[1]):
                if Cm[i, k] != 0:
                    s = s + Cm[i, k] * X[k, j]
            out[i, j] = s
    return out


def _y4(d, g):
    V = _mm_const_left(BT4, _mm_const_left(BT4, d).T).T
    U = _mm(_mm(G4, g), G4.T)
    return _mm_const_left(AT4, _mm_const_left(AT4, (U * V)).T).T


def test_f44_output_pixel_needs_the_whole_patch():
    rng = np.random.default_rng(1)
    d, g = _rand(rng, 6, 6), _rand(rng, 3, 3)
    with np.errstate(invalid="ignore"):
        ref = _y4(d, g)
        direct = np.array([[np.sum(d[i:i + 3, j:j + 3].astype(np.float64) * g) for j in range(4)] for i in range(4)])
        assert np.allclose(ref, direct, atol=1e-4)
        for i in range(4):
            for j in range(4):
                poisoned = np.full_like(d, np.nan)
                poisoned[i:i + 3, j:j + 3] = d[i:i + 3, j:j + 3]
                assert np.isnan(_y4(poisoned, g)[i, j]), (i, j)
        # finite garbage outside the window: the out-of-window terms cancel only in exact arithmetic, the bits move
        moved = 0
        for i in range(4):
            for j in range(4):
                junk = (_rand(rng, 6, 6) * f32(1e3)).astype(f32)
                junk[i:i + 3, j:j + 3] = d[i:i + 3, j:j + 3]
                moved += np.float32(_y4(junk, g)[i, j]).tobytes() != np.float32(ref[i, j]).tobytes()
        assert moved > 0
