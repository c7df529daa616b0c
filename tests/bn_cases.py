"""Case tables, input builders and the dispatch mirror of the BatchNorm family of csrc/pointwise.hip, shared by
tests/test_hip_batchnorm.py (GPU) and tests/test_bn_oracle_cpu.py (CPU: the mirror against the library's host-side queries, the
coverage the tables claim, the exactness conditions of the inputs).

The mirror restates the host-side geometry of pointwise.hip in Python for the default environment: the TG_* switches of these
kernels are read once per process (`static`), the tests set none of them and select paths by shape alone.  Pointwise kernels
write no launch records, so which kernel a shape reaches is known from this mirror only."""
import numpy as np

from tests.pointwise_oracle import ACT_LEAKY, ACT_NONE, ACT_RELU

ACTS = (ACT_NONE, ACT_RELU, ACT_LEAKY)
ACT_NAME = {ACT_NONE: "none", ACT_RELU: "relu", ACT_LEAKY: "leaky"}
SLOPE = 0.25                              # exact inputs: a power of two keeps the leaky branch dyadic
REAL_SLOPE = 0.2                          # real inputs: the network's own slope
EPS32 = float(np.float32(1e-5))           # what the kernels see of eps / momentum: the C ABI takes them as float
MOM32 = float(np.float32(0.1))
SENTINEL = -12345.5


def cdiv(a, b):
    return -(-a // b)


def align_up(n, a):
    return cdiv(n, a) * a


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------
BN_SMALL_ROWS = 2048                      # pointwise.hip:808
FR_COLS, FR_LANES = 16, 16                # pointwise.hip:159 (final_reduce: 16 partial-row lanes, 4 partial rows per unrolled trip)


def small_ok(rows, C):
    """bn_small_ok (pointwise.hip:809)."""
    return rows <= BN_SMALL_ROWS and C % 16 == 0 and C >= 64


SMALL_ENTRIES = ("bn_fwd", "bn_act_bwd")  # tg_bn_fwd (pointwise.hip:897), tg_bn_act_bwd (:1287); tg_bn_stats / tg_bn_act_fwd and the
#                                           grouped and conv1 calls never take the one-launch form


def path(rows, C, entry):
    """Which first-stage / apply kernels `entry` runs at [rows][C]: 'small' (bn_fwd_small_kernel / bn_bwd_small_kernel), 'quad'
    (colreduce4_kernel, bn_act_fwd4 / bn_bwd_apply4) or 'scalar' (colreduce_kernel, bn_act_fwd1 / bn_bwd_apply1)."""
    if entry in SMALL_ENTRIES and small_ok(rows, C):
        return "small"
    return "quad" if C % 4 == 0 else "scalar"


def col_geom(rows, C):
    """col_geom (pointwise.hip:35) -> dict cpp, rlanes, npass, grid, rows_per_block."""
    cpp = min(C, 256)
    rlanes = 256 // cpp
    want = min(max(cdiv(rows, rlanes * 16), 1), 1024)
    rpb = cdiv(rows, want)
    return dict(cpp=cpp, rlanes=rlanes, npass=cdiv(C, cpp), grid=cdiv(rows, rpb), rows_per_block=rpb, capped=cdiv(rows, rlanes * 16) > 1024)


def col_geom4(rows, C, cap=512, per=8):
    """col_geom4 (pointwise.hip:142) -> dict qpp, rlanes, grid, rows_per_block."""
    qpp = min(C // 4, 256)
    rlanes = 256 // qpp
    want = min(max(cdiv(rows, rlanes * per), 1), cap)
    rpb = cdiv(rows, want)
    return dict(qpp=qpp, rlanes=rlanes, grid=cdiv(rows, rpb), rows_per_block=rpb, capped=cdiv(rows, rlanes * per) > cap)


def row_geom(rows, C):
    """row_geom (pointwise.hip:770): the apply grid of the quad kernels -> dict qpp, rlanes, grid (x, y)."""
    nquads = C // 4
    qpp = min(nquads, 256)
    rlanes = 256 // qpp
    gx = min(max(cdiv(rows, rlanes * 4), 1), 2048)
    return dict(qpp=qpp, rlanes=rlanes, grid=(gx, cdiv(nquads, qpp)), capped=cdiv(rows, rlanes * 4) > 2048)


def first_stage(rows, C):
    """Geometry of the statistics / backward first stage of tg_bn_stats / tg_bn_act_bwd off the small path."""
    if C % 4 == 0:
        g = col_geom4(rows, C)
        g["idle"] = g["qpp"] * g["rlanes"] < 256
    else:
        g = col_geom(rows, C)
        g["idle"] = g["cpp"] * g["rlanes"] < 256
    return g


def conv1_geom(rows, C):
    """tg_bn_act_bwd_conv1 (pointwise.hip:1248-1275): first stage = col_geom4 with up to 2048 blocks, `share` = lane-group sharing
    of the nine taps (qpp 16 / 32 / 64), apply = contiguous row ranges, up to 2048 blocks."""
    g = col_geom4(rows, C, cap=2048)
    g["share"] = g["qpp"] in (16, 32, 64)
    want = min(max(cdiv(rows, g["rlanes"] * 32), 1), 2048)
    g["apply_grid"] = cdiv(rows, cdiv(rows, want))
    g["apply_capped"] = cdiv(rows, g["rlanes"] * 32) > 2048
    return g


def bn_ws_bytes(rows, C):
    """tg_bn_ws_bytes (pointwise.hip:680)."""
    if rows <= 0 or C <= 0:
        return 0
    grid = col_geom(rows, C)["grid"]
    if C % 4 == 0:
        grid = max(grid, col_geom4(rows, C)["grid"])
    return align_up(grid * 5 * C, 64) * 4


def bn_grouped_ws_bytes(rows_g, groups, C):
    """tg_bn_grouped_ws_bytes (pointwise.hip:2481)."""
    if rows_g <= 0 or groups <= 0 or C <= 0 or C % 4:
        return 0
    return (align_up(groups * col_geom4(rows_g, C)["grid"] * 5 * C, 64) + align_up(groups * 2 * C, 64)) * 4


def bn_conv1_ws_bytes(rows, C):
    """tg_bn_conv1_ws_bytes (pointwise.hip:1231)."""
    return max(bn_ws_bytes(rows, C), align_up(4096 * 5 * C, 64) * 4)


def conv1_supported(rows, C):
    """tg_bn_bwd_conv1_supported (pointwise.hip:1235)."""
    return C % 4 == 0 and 4 <= C <= 1024 and rows > 0 and not small_ok(rows, C)


# ---- case tables --------------------------------------------------------------------------------------------------------------
# (rows, C): the smallest shapes that reach each path and geometry
SCALAR = [(2, 1), (50, 1), (1024, 3), (77, 6), (300, 255), (40, 258), (9, 1023), (16500, 257)]
QUAD = [(2, 4), (700, 4), (683, 12), (1000, 40), (100, 72), (3000, 48), (2049, 64), (4096, 64), (4100, 1024)]
SMALL = [(2, 64), (63, 64), (64, 80), (65, 128), (2048, 64), (300, 1024)]       # through bn_fwd / bn_act_bwd
# rows <= 2048 with C % 16 == 0: the quad kernels through bn_stats / bn_act_fwd (idle threads at C = 192, 75 first-stage blocks at
# C = 1024), the one-launch kernels through bn_fwd / bn_act_bwd -- as the SMALL shapes are, which lack these two geometries
MIXED = [(333, 192), (600, 1024)]
APPLY_CAP = [(8200, 1024)]                                                       # bn_act_fwd / bn_act_bwd only
STAT_CASES = SCALAR + QUAD + SMALL + MIXED
FWD_BWD_CASES = STAT_CASES + APPLY_CAP

CONV1_NON_SHARE = [(2, 9, 5, 4), (3, 7, 11, 16), (4, 1, 37, 8), (4, 37, 1, 8), (2, 6, 7, 72), (1, 41, 51, 512), (1, 41, 51, 1024)]
CONV1_SHARE = [(2, 33, 35, 64), (2, 33, 32, 128), (1, 46, 45, 256)]              # qpp 16 / 32 / 64
CONV1_CAP = [(1, 129, 128, 1024)]
CONV1_CASES = CONV1_NON_SHARE + CONV1_SHARE + CONV1_CAP

GROUPED = [(2, 4, 8), (683, 12, 3), (2100, 64, 2), (4100, 1024, 2)]              # (rows_g, C, groups)
ORDERS = [[0, 1, 0], [2, 0, 1, 1], [3, 1, 0, 2, 2, 0, 3, 1]]

# real inputs (part B): rows from the tables, at most 4100 so that the worst-case bound of the variance stays a small fraction of
# the variance (test_bn_oracle_cpu.py asserts B_var / (var + eps) <= 0.05 for every one of them)
REAL_KINDS = ("far", "neg", "outlier", "const", "plain")
REAL_CASES = [("scalar", 50, 1, 1), ("scalar", 1024, 3, 1), ("scalar", 300, 255, 1), ("scalar", 40, 258, 1),
              ("scalar", 9, 1023, 1),
              ("quad", 2, 4, 1), ("quad", 700, 4, 1), ("quad", 683, 12, 1), ("quad", 1000, 40, 1), ("quad", 2049, 64, 1),
              ("quad", 600, 1024, 1),
              ("small", 2, 64, 1), ("small", 63, 64, 1), ("small", 333, 192, 1), ("small", 65, 128, 1), ("small", 2048, 64, 1),
              ("small", 300, 1024, 1),
              ("grouped", 683, 12, 3), ("grouped", 2100, 64, 2)]


def case_id(c):
    return "x".join(str(v) for v in c)


def opts(i):
    """Optional arguments of table entry i: activation, ratio / dbias / in-place / running statistics given or absent, in patterns of
    different periods so that every path's entries meet each value (test_bn_oracle_cpu.py checks that they do)."""
    return dict(act=ACTS[i % 3], ratio=i % 2 == 0, dbias=(i // 2) % 2 == 0, inplace=(i + i // 3) % 2 == 1, running=(i + i // 2) % 2 == 0)


def case_opts(table, case):
    return opts(table.index(case))


# ---- exact inputs (part A): every sum the kernels form is a sum of dyadic numbers below 2^24 units -----------------------------
def _seed(*shape):
    s = 7
    for v in shape:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


def _choice(rng, vals, size):
    return np.asarray(vals, dtype=np.float32)[rng.integers(0, len(vals), size)]


def exact_params(rng, C):
    """Free dyadic per-channel statistics and parameters: mean integer in [-50, 50], rstd in {0.5, 1, 2}, gamma in +-{0.5, 1, 2},
    beta in 0.25 * {-8..8}."""
    return dict(mean=rng.integers(-50, 51, C).astype(np.float32), rstd=_choice(rng, (0.5, 1.0, 2.0), C),
                gamma=_choice(rng, (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0), C), beta=(0.25 * rng.integers(-8, 9, C)).astype(np.float32))


def exact_inputs(rows, C, k=3):
    """y = mean + integer in [-k, k], dout integer in [-4, 4], ratio in {0.5, 1, 2} per row, all fp32.  With these xh, z, g, g xh,
    ratio g, ratio xh and all their partial sums are dyadic; z == 0 is frequent (the gate is z > 0)."""
    rng = np.random.default_rng(_seed(rows, C, k))
    p = exact_params(rng, C)
    p["y"] = (p["mean"] + rng.integers(-k, k + 1, (rows, C))).astype(np.float32)
    p["dout"] = rng.integers(-4, 5, (rows, C)).astype(np.float32)
    p["ratio"] = _choice(rng, (0.5, 1.0, 2.0), rows)
    return p


def exact_conv1_inputs(B, H, W, C):
    """exact_inputs with k = 2 and the incoming gradient given as dz, w in {-1, 0, 1} (dout = their 3x3 dgrad: integers in [-9, 9])."""
    rng = np.random.default_rng(_seed(B, H, W, C))
    rows = B * H * W
    p = exact_params(rng, C)
    p["y"] = (p["mean"] + rng.integers(-2, 3, (rows, C))).astype(np.float32)
    p["dz"] = rng.integers(-1, 2, (B, H, W)).astype(np.float32)
    p["w"] = rng.integers(-1, 2, (3, 3, C)).astype(np.float32)
    p["ratio"] = _choice(rng, (0.5, 1.0, 2.0), rows)
    return p


def exact_grouped_inputs(rows_g, C, groups):
    """exact_inputs for `groups` stacked passes: gamma / beta shared, mean / rstd [groups][C] free per pass, y / dout
    [groups * rows_g][C]; no ratio (the grouped backward takes none)."""
    rng = np.random.default_rng(_seed(rows_g, C, groups, 5))
    p = exact_params(rng, C)
    per = [exact_params(rng, C) for _ in range(groups)]
    p["mean"], p["rstd"] = np.stack([q["mean"] for q in per]), np.stack([q["rstd"] for q in per])
    p["y"] = np.concatenate([(p["mean"][g] + rng.integers(-3, 4, (rows_g, C))).astype(np.float32) for g in range(groups)])
    p["dout"] = rng.integers(-4, 5, (groups * rows_g, C)).astype(np.float32)
    return p


def dyadic_stat_inputs(rows, C, seed=0):
    """Every channel holds m +- a with equal counts in shuffled order (rows even), m integer in [-50, 50], a in {0.5, 1, 2, 4}.  With
    eps = 0.0 the shifted sums are exact, mean == m and rstd == 1 / a exactly on every path, so xh = +-1 and the whole
    forward -> backward chain is exact.  -> exact_inputs' dict with y, m, a in place of y, mean, rstd."""
    assert rows % 2 == 0
    rng = np.random.default_rng(_seed(rows, C, 99, seed))
    p = exact_params(rng, C)
    del p["mean"], p["rstd"]
    p["m"] = rng.integers(-50, 51, C).astype(np.float32)
    p["a"] = _choice(rng, (0.5, 1.0, 2.0, 4.0), C)
    sign = np.ones((rows, C), dtype=np.float32)
    sign[rows // 2:] = -1.0
    sign = rng.permuted(sign, axis=0)
    p["y"] = (p["m"] + sign * p["a"]).astype(np.float32)
    p["dout"] = rng.integers(-4, 5, (rows, C)).astype(np.float32)
    p["ratio"] = _choice(rng, (0.5, 1.0, 2.0), rows)
    return p


# units of the seven sums on exact inputs: sum d, sum d^2 (statistics, d = y - y[0]); q0..q4 (backward)
STAT_UNITS = (1.0, 1.0)
BWD_UNITS = (0.25, 0.125, 0.125, 0.25, 0.5)


def stat_terms(y):
    d = np.asarray(y, dtype=np.float64)
    d = d - d[0]
    return [d, d * d]


def bwd_terms(dout, y, mean, rstd, gamma, beta, act, slope, ratio):
    """The five per-row terms of the backward sums, in float64 (exact on exact inputs)."""
    y, dout = np.asarray(y, np.float64), np.asarray(dout, np.float64)
    xh = (y - np.asarray(mean, np.float64)) * np.asarray(rstd, np.float64)
    z = xh * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    ga = np.ones_like(z) if act == ACT_NONE else np.where(z > 0, 1.0, 0.0 if act == ACT_RELU else slope)
    g = dout * ga
    rr = (np.ones(y.shape[0]) if ratio is None else np.asarray(ratio, np.float64))[:, None]
    return [g, g * xh, rr * g, rr * xh, np.broadcast_to(rr, y.shape)]


# ---- real inputs (part B) -------------------------------------------------------------------------------------------------------
def real_inputs(kind, rows, C, groups=1):
    """y [groups * rows][C] fp32, gamma, beta:
    far 1000 + 0.01 N(0,1); neg -300 + 0.5 N; outlier = far with row 0 (of every group) 8 std above the mean; const = 5 + 2 N with
    one constant channel; plain 5 + 2 N."""
    rng = np.random.default_rng(_seed(rows, C, groups, REAL_KINDS.index(kind)))
    n = rng.standard_normal((groups * rows, C))
    if kind in ("far", "outlier"):
        y = 1000.0 + 0.01 * n
        if kind == "outlier":
            y[::rows] = 1000.0 + 0.08
    elif kind == "neg":
        y = -300.0 + 0.5 * n
    else:
        y = 5.0 + 2.0 * n
        if kind == "const":
            y[:, C // 2] = 7.3
    return dict(y=y.astype(np.float32), gamma=(rng.random(C) + 0.5).astype(np.float32), beta=rng.standard_normal(C).astype(np.float32),
                const_channel=C // 2 if kind == "const" else None)


def stat_bounds(y, eps):
    """The derived bounds of part B for one [n][C] pass, from float64: d = y - y[0], md = mean(d), u = 2^-24.
    -> dict mean (|mean - ref| <= (n + 2) u mean|d| + u |ref|), b_var = 2 (n + 8) u (mean(d^2) + md^2) (the worst-case error, in any
    summation order, of sum d^2 / n - (sum d / n)^2), rstd_rel = b_var / (var + eps) + 2 u, and the references ref_mean, var, rstd."""
    u = 2.0 ** -24
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    d = y - y[0]
    md = d.mean(0)
    ref_mean = y.mean(0)
    var = ((y - ref_mean) ** 2).mean(0)
    b_var = 2.0 * (n + 8) * u * ((d * d).mean(0) + md * md)
    return dict(n=n, ref_mean=ref_mean, var=var, rstd=1.0 / np.sqrt(var + eps), mean_sum=(n + 2) * u * np.abs(d).mean(0),
                mean=(n + 2) * u * np.abs(d).mean(0) + u * np.abs(ref_mean), b_var=b_var, rstd_rel=b_var / (var + eps) + 2 * u)
