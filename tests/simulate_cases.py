"""The measurements behind tests/golden/simulate_stats.json, shared by tests/test_simulate_cpu.py (which repeats them and compares)
and by `python -m tests.simulate_cases` (which writes the file).  Nothing here touches the GPU or the kernel: every figure is a
property of the numpy mirror (tests/simulate_oracle.py) and of spectral_waves."""
import json
import os

import numpy as np

from mvp_gan.src import simulate as S
from mvp_gan.src.kriging import Variogram
from tests import kriging_oracle as K
from tests import simulate_oracle as SO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simulate_stats.json")
ROTATIONS = 8                                              # seeds whose rotation the wave-table test tries
MODELS = {"power-0.5": ("power", 0.0, 0.05, 0.5), "power-1.0": ("power", 0.0, 0.05, 1.0), "power-1.5": ("power", 0.0, 0.05, 1.5),
          "power-1.9": ("power", 0.0, 0.05, 1.9), "exponential-8": ("exponential", 0.0, 4.0, 8.0),
          "exponential-40": ("exponential", 0.0, 4.0, 40.0)}
WAVES = (64, 256, 512)
FIELD_SIDE, FIELD_SEEDS, FIELD_WAVES = 256, 16, 64
SPREAD = {"side": 96, "known": 0.2, "realisations": 64, "seeds": 4, "waves": 64}
SPREAD_VG = Variogram("power", 0.0, 0.05, 1.0)


def cosine_max_error(chunk=1 << 22):
    """The largest |polynomial - cos| over all 4 * 2^24 reduced arguments, cos in float64 at the same (truncated) angle."""
    worst = 0.0
    for q in range(4):
        for lo in range(0, 1 << 24, chunk):
            m = np.arange(lo, lo + chunk, dtype=np.uint32)
            got = SO.cos_reduced(np.uint32(q), m).astype(np.float64)
            want = np.cos((2.0 * np.pi / 2.0 ** 26) * (q * float(1 << 24) + m.astype(np.float64)))
            worst = max(worst, float(np.abs(got - want).max()))
    return worst


def class_lags():
    """The 64 lags of the statistics: L = 1 .. 32 px, axial and diagonal; a class pools its two directions as
    empirical_variogram does.  -> (vectors int64 [128][2], metres per pixel of lag [64])."""
    v = S.lag_vectors(32)
    return v, np.array([L * (np.sqrt(2.0) if k else 1.0) for L in range(1, 33) for k in (0, 1)])


def table_error(spec, waves, seed, cellsize=1.0):
    """max over the 64 lags of |gamma_N - gamma| / gamma."""
    vg = Variogram(*spec)
    v, h = class_lags()
    g = S.realised_variogram(S.spectral_waves(vg, cellsize, waves, seed), vg.nugget, v).reshape(32, 2, 2).mean(2).ravel()
    want = vg.gamma(cellsize * h)
    return float(np.abs(g / want - 1.0).max())


def table_errors():
    return {f"{name}/{w}": max(table_error(spec, w, s) for s in range(ROTATIONS)) for name, spec in MODELS.items() for w in WAVES}


def field_error():
    """The empirical variogram (oracle slicing, lags 1 .. 32 px in octaves) of the mirror's field, averaged over the seeds, against
    the closed form averaged in the same way: max over the 12 scales of |ratio - 1|."""
    vg = SPREAD_VG
    known = np.ones((FIELD_SIDE, FIELD_SIDE), np.uint8)
    emp, want = np.zeros(2 * K.OCTAVES), np.zeros(2 * K.OCTAVES)
    vec = np.array([v for j in range(K.OCTAVES) for v in ((0, 1 << j), (1 << j, 0), (1 << j, 1 << j), (1 << j, -(1 << j)))])
    for seed in range(FIELD_SEEDS):
        tab = S.with_phases(S.spectral_waves(vg, 1.0, FIELD_WAVES, seed), seed, 0)
        pairs, sums = K.variogram(SO.field(FIELD_SIDE, FIELD_SIDE, tab), known)
        emp += sums / (2.0 * pairs)
        want += S.realised_variogram(tab, 0.0, vec).reshape(-1, 2).mean(1)
    return float(np.abs(emp / want - 1.0).max())


def spread_scene():
    n = SPREAD["side"]
    known = (np.random.Generator(np.random.PCG64(5)).random((n, n)) < SPREAD["known"]).astype(np.uint8)
    return known, SO.weights(known, K.ray_hits(known), SPREAD_VG, 1.0)


def spread_ratios():
    """Per seed: the mean over the void pixels of mean_r d^2 / sigma^2_krige, d = u - krige(u) in float64 on the mirror's u."""
    known, wt = spread_scene()
    n, out = SPREAD["side"], []
    for seed in range(SPREAD["seeds"]):
        tab = S.spectral_waves(SPREAD_VG, 1.0, SPREAD["waves"], seed)
        d2 = np.zeros(len(wt["ys"]))
        for r in range(SPREAD["realisations"]):
            u = SO.field(n, n, S.with_phases(tab, seed, r)).astype(np.float64)
            d = u[wt["ys"], wt["xs"]] - SO.krige_with(wt, u)
            d2 += d * d
        out.append(float((d2 / SPREAD["realisations"] / wt["var"]).mean()))
    return out


def measure():
    r = spread_ratios()
    return {"cosine_max_abs_error": cosine_max_error(), "table_rel_error": table_errors(), "field_rel_error": field_error(),
            "spread_ratio_mean": float(np.mean(r)), "spread_ratio_spread": float(np.max(r) - np.min(r)), "spread_ratios": r}


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(measure(), f, indent=1)
        f.write("\n")
    print(open(GOLDEN).read())
