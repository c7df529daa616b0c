"""numpy mirror of csrc/simulate.hip, operation for operation: the uint32 phase, the float32 cosine
polynomial, the float64 sum over the waves in index order, the 32-bit mix, the Irwin-Hall nugget term, the combine and the ensemble
statistics.  field() reproduces tg_sim_field to the last bit.  Kriging comes from tests/kriging_oracle.py: weights() solves every
void pixel's bordered system once, so that any number of fields can be kriged over the same samples in float64."""
import numpy as np

from tests import kriging_oracle as K

F32, F64, U32 = np.float32, np.float64, np.uint32
# (float)((-1)^j (pi / 2)^(2 j) / (2 j)!), j = 0 .. 7: the literals of sim_cos
COEF = tuple(F32(float.fromhex(h)) for h in ("0x1p+0", "-0x1.3bd3ccp+0", "0x1.03c1f0p-2", "-0x1.55d3c8p-6", "0x1.e1f506p-11",
                                             "-0x1.a6d1f2p-16", "0x1.f9d38ap-22", "-0x1.b6e250p-28"))
GOLD = U32(0x9e3779b9)


def mix(v):
    v = np.asarray(v, U32).copy()
    v ^= v >> U32(16)
    v *= U32(0x7feb352d)
    v ^= v >> U32(15)
    v *= U32(0x846ca68b)
    v ^= v >> U32(16)
    return v


def cos_reduced(q, m):
    """The polynomial on quadrant q (0 .. 3) and the 24-bit fraction m of the quarter turn -> float32."""
    q, m = np.asarray(q, U32), np.asarray(m, U32)
    mm = np.where(q & U32(1), U32(0x1000000) - m, m)
    t = mm.astype(F32) * F32(2.0 ** -24)
    s = t * t
    c = np.full(s.shape, COEF[7], F32)
    for j in range(6, -1, -1):
        c = c * s
        c = c + COEF[j]
    return np.where((q + U32(1)) & U32(2), -c, c)


def cos_phase(p):
    """cos(2 pi p / 2^32) as the kernel takes it, p uint32."""
    p = np.asarray(p, U32)
    return cos_reduced(p >> U32(30), (p >> U32(6)) & U32(0xffffff))


def nugget_term(H, W, origin, seed, realisation):
    """g float64 [H][W]: (the sum of the twelve 16-bit lanes of six hash words - 393210) * 2^-16."""
    y0, x0 = origin
    Y = (np.arange(H, dtype=np.uint64) + np.uint64(y0)).astype(U32)[:, None]
    X = (np.arange(W, dtype=np.uint64) + np.uint64(x0)).astype(U32)[None, :]
    with np.errstate(over="ignore"):
        row = mix(mix(mix(np.array([seed], U32) + GOLD) ^ U32(realisation)) ^ Y)
        key = mix(row ^ X)
        total = np.zeros((H, W), np.int64)
        for j in range(1, 7):
            h = mix(key + U32(j) * GOLD)
            total += (h & U32(0xffff)).astype(np.int64) + (h >> U32(16)).astype(np.int64)
    return (total - 393210).astype(F64) * F64(2.0 ** -16)


def field(H, W, table, origin=(0, 0), nugget_amp=0.0, seed=0, realisation=0):
    """u float32 [H][W], bit for bit tg_sim_field's.  table: a structured array with fx, fy, phase, amp."""
    y0, x0 = origin
    Y = (np.arange(H, dtype=np.uint64) + np.uint64(y0)).astype(U32)[:, None]
    X = (np.arange(W, dtype=np.uint64) + np.uint64(x0)).astype(U32)[None, :]
    acc = np.zeros((H, W), F64)
    with np.errstate(over="ignore"):
        for w in table:
            fx, fy = U32(int(w["fx"]) & 0xffffffff), U32(int(w["fy"]) & 0xffffffff)
            p = fx * X + (fy * Y + U32(w["phase"]))
            acc = acc + F64(F32(w["amp"])) * cos_phase(p).astype(F64)
    if F32(nugget_amp) != 0:
        acc = acc + F64(F32(nugget_amp)) * nugget_term(H, W, origin, seed, realisation)
    return acc.astype(F32)


def combine(z, known, zk, u, uk, s1=None, s2=None):
    """-> out float32; s1, s2 (float64, in place) take d and d * d on the unknown pixels."""
    z, zk, u, uk = (np.asarray(a, F32) for a in (z, zk, u, uk))
    kn = np.asarray(known) != 0
    d = u.astype(F64) - uk.astype(F64)
    out = np.where(kn, z, (zk.astype(F64) + d).astype(F32))
    if s1 is not None:
        s1[~kn] = s1[~kn] + d[~kn]
        s2[~kn] = s2[~kn] + d[~kn] * d[~kn]
    return out


def stats(zk, s1, s2, n):
    """-> (mean float32, sd float32, sd float64 before its rounding)."""
    zk = np.asarray(zk, F32)
    with np.errstate(invalid="ignore"):
        mean = (zk.astype(F64) + s1 / F64(n)).astype(F32)
        v = (s2 - (s1 * s1) / F64(n)) / F64(n - 1)
        sd = np.sqrt(np.where(v > 0, v, 0.0))
    sd = np.where(np.isnan(zk), np.nan, sd)
    return mean, sd.astype(F32), sd


# ---- kriging any field over one set of samples ------------------------------------------------------------------------------
def weights(known, hits, vg, cellsize):
    """The ordinary-kriging weights of every void pixel with a ray sample, once: -> dict ys, xs int [P]; sy, sx int [P][8] (the
    sample pixels, the pixel itself where a ray has none); w float64 [P][8] (0 there); var float64 [P] (the kriging variance)."""
    kn = np.asarray(known) != 0
    hits = np.asarray(hits).astype(np.int64)
    have = (hits > 0) & ~kn[None]
    pattern = (have * (1 << np.arange(8))[:, None, None]).sum(0)
    dirs = np.array(K.DIRS, np.int64)
    out = {k: [] for k in ("ys", "xs", "sy", "sx", "w", "var")}
    for pat in np.unique(pattern[~kn]):
        if pat == 0:
            continue
        ys, xs = np.nonzero((pattern == pat) & ~kn)
        rays = [j for j in range(8) if pat >> j & 1]
        k = hits[rays][:, ys, xs].T
        off = k[:, :, None] * dirs[rays][None, :, :]
        s = K.bordered(off, np.zeros(k.shape), vg, cellsize)
        sy, sx = np.repeat(ys[:, None], 8, 1), np.repeat(xs[:, None], 8, 1)
        w = np.zeros((len(ys), 8))
        sy[:, rays], sx[:, rays], w[:, rays] = ys[:, None] + off[:, :, 0], xs[:, None] + off[:, :, 1], s["w"]
        for name, v in (("ys", ys), ("xs", xs), ("sy", sy), ("sx", sx), ("w", w), ("var", np.maximum(s["var"], 0.0))):
            out[name].append(v)
    return {k: np.concatenate(v) for k, v in out.items()}


def krige_with(wt, f):
    """The float64 kriging of the field f at the pixels of weights() -> [P]."""
    return (wt["w"] * np.asarray(f, F64)[wt["sy"], wt["sx"]]).sum(1)
