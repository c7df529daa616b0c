"""Case table of the direct convolution kernels (csrc/igemm.hip: igemm / igemm_multi / pgemm / wgrad and the split-K second
passes; csrc/smallconv.hip), shared by tests/test_hip_direct_conv.py (GPU: the launch records must show exactly the expected
kernel, then the exact-integer and the a-priori-bound checks of tests/conv_oracle.py) and tests/test_conv_oracle_cpu.py (CPU: the
oracle against float64 autograd, the exactness condition, fp32 PyTorch inside the bound, and `predict` = the expectation).
B16_CASES: the same for the bf16-operand instantiations of these kernels and wgrad_bf16_kernel (tests/test_hip_bf16_direct.py).

`predict` restates the host-side planners of the two files (pick_bn, choose_splits, plan_splits, try_pgemm, try_igemm_multi,
wgrad_plan, the smallconv_* and Winograd admission predicates) in Python, for the default environment (no TG_* switch) and a
workspace of the size the queries report.  The table's expectations are literals; the restatement only has to agree with them,
and the GPU has the last word."""
import math
from types import SimpleNamespace as NS

import numpy as np

from tests import conv_oracle as CO

# SmallRoute (csrc/igemm_params.h)
SR_C1MFMA, SR_C1CONV, SR_TO1CONVW, SR_TO1_LDS, SR_TO1_LDS_BNIN, SR_TO1_LDS_MAP, SR_TO1CONV64 = 100, 110, 200, 300, 301, 302, 400
SR_MULTI22_LDS, SR_MULTI22 = 500, 501
SR_C1WGRAD_MFMA, SR_C1WGRAD_MFMA_BIAS, SR_C1WGRAD, SR_TO1WGRADW, SR_TO1WGRAD_LDS, SR_TO1WGRAD_LDS_BNIN, SR_TO1WGRAD64 = \
    600, 610, 620, 700, 800, 801, 900
SMALL_FWD, SMALL_WGRAD, TO1_MULTI = 2000, 2001, 2004
T1_TH, T1_TW, C1_T = 4, 16, 16


def cdiv(a, b):
    return -(-a // b)


# ---- the planners, restated ---------------------------------------------------------------------------------------------------
def choose_splits(tiles, max_splits, slots):
    max_splits = max(max_splits, 1)
    if tiles >= 4 * slots:
        return 1
    best, best_eff = 1, 0.0
    for sp in range(1, max_splits + 1):
        blocks = tiles * sp
        rounds = cdiv(blocks, slots)
        eff = blocks / (rounds * slots)
        if eff > best_eff + 1e-9:
            best_eff, best = eff, sp
        if blocks >= slots and eff >= 0.92:
            return sp
        if blocks >= 6 * slots:
            break
    return best


def pick_bn(N):
    return 128 if N >= 128 and N % 128 == 0 else (64 if N > 32 else 32)


def _finish(p):
    p.M = p.B * p.OH * p.OW
    p.Ktot = p.TH * p.TW * p.C
    p.nchunks = cdiv(p.C, 32)
    p.T = cdiv(p.Ktot, 32) if p.C % 4 else p.TH * p.TW * p.nchunks
    return p


def fwd_params(g):
    B, H, W, Cin, Cout, k, s, pad = g
    Ho, Wo = CO.out_size(H, k, s, pad), CO.out_size(W, k, s, pad)
    return _finish(NS(B=B, IH=H, IW=W, C=Cin, OH=Ho, OW=Wo, N=Cout, DH=Ho, DW=Wo, ds=1, TH=k, TW=k, ss=s, tstep=1, sy0=-pad, sx0=-pad,
                      kstep=1, masked=False))


def dgrad_classes(g):
    B, H, W, Cin, Cout, k, st, pad = g
    Ho, Wo = CO.out_size(H, k, st, pad), CO.out_size(W, k, st, pad)
    out = []
    for py in range(st):
        for px in range(st):
            OH, OW = (H - py + st - 1) // st, (W - px + st - 1) // st
            if OH <= 0 or OW <= 0:
                continue
            ky0, kx0 = (py + pad) % st, (px + pad) % st
            TH = (k - ky0 + st - 1) // st if ky0 < k else 0
            TW = (k - kx0 + st - 1) // st if kx0 < k else 0
            out.append(_finish(NS(B=B, IH=Ho, IW=Wo, C=Cout, OH=OH, OW=OW, N=Cin, DH=H, DW=W, ds=st, TH=TH, TW=TW, ss=1, tstep=-1,
                                  sy0=(py + pad - ky0) // st, sx0=(px + pad - kx0) // st, kstep=st, masked=False)))
    return out


def to1w_ok(p):
    return p.N == 1 and p.C in (256, 512) and (p.TH, p.TW) in ((4, 4), (3, 3))


def to1_cfg_ok(th, tw):
    return (th, tw) in ((3, 3), (2, 2), (4, 4), (1, 1), (2, 1), (1, 2))


def smallconv_fwd_applies(p):
    taps = p.TH * p.TW
    if p.C == 1 and p.N >= 64 and p.N % 64 == 0 and 1 <= taps <= 64:
        return True
    if p.N == 1 and p.C == 64 and p.OW % 4 == 0 and to1_cfg_ok(p.TH, p.TW):
        return True
    return to1w_ok(p)


def to1_fwd_lds_ok(p, env=None):
    return env != "TG_NO_TO1LDS" and p.TH == 3 and p.TW == 3 and p.ss == 1 and p.tstep in (1, -1) and p.OH >= T1_TH and p.OW >= T1_TW


def smallconv_fwd_route(p, bnin=False, env=None, sparse=False):
    if p.C == 1:
        k743 = p.TH == p.TW and p.TH in (7, 4, 3)
        return (SR_C1CONV if env == "TG_NO_C1MFMA" else SR_C1MFMA) + p.TH if k743 else SR_C1CONV
    if to1w_ok(p):
        return SR_TO1CONVW + 10 * p.TH + p.C // 256
    if to1_fwd_lds_ok(p, env):
        if sparse and p.C == 64 and p.ds == 1 and (p.DH, p.DW) == (p.OH, p.OW):
            return SR_TO1_LDS_MAP
        return SR_TO1_LDS_BNIN if bnin else SR_TO1_LDS
    assert to1_cfg_ok(p.TH, p.TW)
    return SR_TO1CONV64 + 10 * p.TH + p.TW


def to1_multi_applies(cls):
    return len(cls) == 4 and all(p.N == 1 and p.C == 64 and p.TH == 2 and p.TW == 2 and p.OW % 4 == 0 and p.M == cls[0].M and
                                 p.OH == cls[0].OH and p.OW == cls[0].OW for p in cls)


def to1_multi_route(cls, env=None):
    ys = [p.sy0 + t * p.tstep for p in cls for t in range(2)]
    xs = [p.sx0 + t * p.tstep for p in cls for t in range(2)]
    ok = env != "TG_NO_TO1LDS" and cls[0].OH >= T1_TH and cls[0].OW >= T1_TW and all(p.ss == 1 and not p.masked for p in cls)
    return SR_MULTI22_LDS if ok and max(ys) - min(ys) <= 2 and max(xs) - min(xs) <= 2 else SR_MULTI22


def plan_splits(p):
    bn = pick_bn(p.N)
    tiles = cdiv(p.M, 128) * cdiv(p.N, bn)
    splits = choose_splits(tiles, min(p.T // 4, 64), 512) if p.T >= 8 else 1
    sps = cdiv(p.T if p.T > 0 else 1, splits)
    return cdiv(p.T, sps) if p.T > 0 else 1


def pgemm_class_ok(p):
    if p.ss != 1 or p.C % 32 or not (1 <= p.TH <= 4 and 1 <= p.TW <= 4) or p.OW < 16 or p.OH < 8:
        return False
    n64 = not (p.N >= 128 and p.N % 128 == 0)
    return not (n64 and (p.N < 48 or p.OH < 16))


def try_pgemm(cls):
    """(cfg, splits) of the patch kernel's launch, or None."""
    if not all(pgemm_class_ok(p) for p in cls):
        return None
    p = cls[0]
    n64 = not (p.N >= 128 and p.N % 128 == 0)
    th, tw, bn = (16 if n64 else 8), 16, (64 if n64 else 128)
    work = sum(cdiv(c.OW, tw) * cdiv(c.OH, th) * c.B * cdiv(p.N, bn) for c in cls)
    nchunks, splits = p.C // 32, 1
    if len(cls) == 1:
        if nchunks >= 4:
            splits = choose_splits(work, min(nchunks // 2, 32), 512)
    elif work < 512:
        return None
    return 1000 + bn, cdiv(nchunks, cdiv(nchunks, splits))


def try_igemm_multi(cls):
    """(cfg, per-class split counts) of the merged gathered-row launch, or None."""
    bn = pick_bn(cls[0].N)
    if not 2 <= len(cls) <= 4 or bn not in (64, 128):
        return None
    if any(p.M <= 0 or p.N != cls[0].N or p.C % 4 or smallconv_fwd_applies(p) or p.T <= 0 for p in cls):
        return None
    tl = [cdiv(p.M, 128) * cdiv(p.N, bn) for p in cls]
    tmax = max(p.T for p in cls)
    sp = [1] * len(cls)
    if tmax >= 8:
        sp = [choose_splits(sum(tl), min(tmax // 4, 64), 512)] * len(cls)
        best = 1e300
        for L in range(tmax, 3, -1):
            cand = [min(cdiv(p.T, L), max(1, min(p.T // 4, 64))) for p in cls]
            blocks = sum(t * s for t, s in zip(tl, cand))
            longest = max(cdiv(p.T, s) for p, s in zip(cls, cand))
            cost = float(cdiv(blocks, 512)) * (longest + 4.0) + 0.002 * float(blocks)
            if cost < best * 0.995:
                best, sp = cost, cand
    return 500 + bn, tuple(cdiv(p.T, cdiv(p.T, s)) for p, s in zip(cls, sp))


# The record of an MFMA launch: in bf16 mode (tg_hip.ops.set_precision("bf16")) the gathered-row kernel at BN 64 / 128 with the
# vector gather, the patch kernel and the merged gathered-row launch run their BF16 = true instantiations, kind 3 with a cfg of
# their own each; BN 32 and the scalar gather (Cin % 4 != 0) have no bf16 twin and keep the fp32 record.
B16_CFG = {64: 3064, 128: 3128, 1064: 3264, 1128: 3328, 564: 3564, 628: 3628}


def mfma_record(cfg, bf16=False):
    return (3, B16_CFG[cfg], 0) if bf16 and cfg in B16_CFG else (0, cfg, 0)


def launch_igemm(p, bnin=False, env=None, sparse=False, bf16=False):
    """(kind, cfg, route), splits of launch_igemm after plan_splits."""
    if smallconv_fwd_applies(p):
        return (2, SMALL_FWD, smallconv_fwd_route(p, bnin, env, sparse)), 1
    assert not bnin
    pg = try_pgemm([p])
    if pg:
        return mfma_record(pg[0], bf16), pg[1]
    return mfma_record(pick_bn(p.N) + (1 if p.C % 4 else 0), bf16), plan_splits(p)


def wino_geom_ok(p, bf16=False):
    return p.TH == 3 and p.TW == 3 and p.ss == 1 and p.C % (16 if bf16 else 8) == 0 and p.N % 64 == 0 and p.OH >= 16 and p.OW >= 16


def _halved(g):
    B, H, W, Cin, Cout, k, s, pad = g
    return H % 2 == 0 and W % 2 == 0 and CO.out_size(H, k, s, pad) == H // 2 and CO.out_size(W, k, s, pad) == W // 2


def s2d_ok(g):
    B, H, W, Cin, Cout, k, s, pad = g
    return (k, s, pad) == (5, 2, 2) and _halved(g) and Cin % 16 == 0 and Cout % 64 == 0 and H // 2 >= 32 and W // 2 >= 32


def wino22_ok(g, c8, c64):
    B, H, W, Cin, Cout, k, s, pad = g
    return (k, s, pad) == (4, 2, 1) and _halved(g) and c8 % 8 == 0 and c64 % 64 == 0 and H // 2 >= 16 and W // 2 >= 16


def wgrad_plan(g):
    """(bm, splits) of wgrad_kernel and of wgrad_bf16_kernel."""
    B, H, W, Cin, Cout, k, s, pad = g
    Ho, Wo = CO.out_size(H, k, s, pad), CO.out_size(W, k, s, pad)
    bm = 32 if Cout % 4 or Cout < 32 else (128 if Cout >= 128 and Cin % 4 == 0 else 64)
    tiles = cdiv(Cout, bm) * cdiv(k * k * Cin, 128)
    T = cdiv(B * Ho * Wo, 32)
    sp = choose_splits(tiles, min(cdiv(T, 4), 512), 256 * (2 if bm == 128 else 3))
    return bm, cdiv(T, cdiv(T, sp))


def smallconv_wgrad_route(g, want_db, bnin, env=None):
    """SmallRoute of the weight gradient, or None where smallconv_wgrad_applies is false."""
    B, H, W, Cin, Cout, k, s, pad = g
    Ho, Wo = CO.out_size(H, k, s, pad), CO.out_size(W, k, s, pad)
    to1w = Cout == 1 and Cin % 256 == 0 and Cin <= 1024 and k in (3, 4) and s == 1
    if Cin == 1 and Cout >= 64 and Cout % 64 == 0 and k in (3, 4, 7):
        return (SR_C1WGRAD if env == "TG_C1WGRAD" else SR_C1WGRAD_MFMA_BIAS if want_db else SR_C1WGRAD_MFMA) + k
    if not (to1w or (Cout == 1 and Cin == 64 and Wo % 4 == 0 and k in (3, 4))):
        return None
    if to1w:
        return SR_TO1WGRADW + k
    if env != "TG_NO_TO1LDS" and Cin == 64 and k == 3 and s == 1 and pad == 1 and Ho >= T1_TH and Wo >= T1_TW:
        return SR_TO1WGRAD_LDS_BNIN if bnin else SR_TO1WGRAD_LDS
    return SR_TO1WGRAD64 + k


def wgrad_slabs(g, route):
    """Partial slabs the weight-gradient launch reduces (smallconv_wgrad_blocks; wgrad_plan's splits for the MFMA kernel)."""
    B, H, W, Cin, Cout, k, s, pad = g
    Ho, Wo = CO.out_size(H, k, s, pad), CO.out_size(W, k, s, pad)
    if route == 0:
        return wgrad_plan(g)[1]
    if Cin == 1:
        return min(cdiv(Wo, C1_T) * cdiv(Ho, C1_T) * B, 512)
    if route in (SR_TO1WGRADW + 3, SR_TO1WGRADW + 4):
        return B * cdiv(Ho, 4)
    if route in (SR_TO1WGRAD_LDS, SR_TO1WGRAD_LDS_BNIN):
        return min(cdiv(Wo, T1_TW) * cdiv(Ho, T1_TH) * B, 768)
    quads = B * Ho * Wo // 4
    qpb = cdiv(quads, max(1, min(cdiv(quads, 64), 1024)))
    return cdiv(quads, qpb) if qpb > 0 else 1


def wgrad_bf16_ok(g, bm, setenv=None):
    """bf16 mode: wgrad_bf16_kernel takes the launch wgrad_kernel would get (conv_wgrad_impl; the switch is read per call)."""
    B, H, W, Cin, Cout, k, s, pad = g
    return Cin % 4 == 0 and Cout % 4 == 0 and CO.out_size(W, k, s, pad) % 32 == 0 and bm >= 64 and setenv != "TG_NO_BF16_WGRAD"


def predict(case):
    """[(kind, cfg, route), ...] in launch order, and the recorded split counts [splits, ...] (igemm_multi: per class, as one tuple)."""
    g, op, mods = case.geom, case.op, case.mods
    B, H, W, Cin, Cout, k, s, pad = g
    masked, bnin, env, bf16 = "mask" in mods, "bnin" in mods, case.env, case.prec == "bf16"
    if op == "fwd":
        p = fwd_params(g)
        assert not s2d_ok(g) and (bf16 or not wino22_ok(g, Cin, Cout)) and not wino_geom_ok(p, bf16), "a Winograd route takes this forward"
        r, sp = launch_igemm(p, bnin, env, bf16=bf16)
        return [r], [sp]
    if op == "dgrad":
        assert not (s2d_ok(g) and "gate" not in mods) and (bf16 or not wino22_ok(g, Cout, Cin)), "a Winograd route takes this dgrad"
        p1 = NS(TH=k, TW=k, ss=s, C=Cout, N=Cin, OH=H, OW=W)
        assert not wino_geom_ok(p1, bf16), "a Winograd route takes this dgrad"
        cls = dgrad_classes(g)
        if s * s <= 4:
            if to1_multi_applies(cls):
                return [(2, TO1_MULTI, to1_multi_route(cls, env))], [1]
            if len(cls) > 1 and not smallconv_fwd_applies(cls[0]):
                pg = try_pgemm(cls)
                if pg:
                    return [mfma_record(pg[0], bf16)], [pg[1]]
                mu = try_igemm_multi(cls)
                if mu:
                    return [mfma_record(mu[0], bf16)], [mu[1]]
        rs = [launch_igemm(p, False, env, "map" in mods, bf16) for p in cls]
        return [r for r, _ in rs], [sp for _, sp in rs]
    assert op == "wgrad"
    route = smallconv_wgrad_route(g, "bias" in mods, bnin, env)
    if route is not None:
        return [(2, SMALL_WGRAD, route)], [1]
    Ho, Wo = CO.out_size(H, k, s, pad), CO.out_size(W, k, s, pad)
    assert not s2d_ok(g), "a Winograd route takes this wgrad"
    s1_64 = (k, s) == (3, 1) and Cin % 64 == 0 and Cout % 64 == 0 and Ho >= 16
    if bf16:        # wino16_wgrad_ok: Wo >= 32; the fp32 F(3x3,2x2) kernel up to 256 input channels; F(2x2,2x2) never
        assert masked or not (s1_64 and (Wo >= 32 or (Wo >= 16 and Cin <= 256))), "Winograd wgrad"
    else:
        assert masked or not (s1_64 and Wo >= 16), "Winograd wgrad"
        assert masked or not (wino22_ok(g, 64, 64) and Cin % 64 == 0 and Cout % 64 == 0), "Winograd F(2x2,2x2) wgrad"
    bm, sp = wgrad_plan(g)
    return [(3, 3700 + bm, 0) if bf16 and wgrad_bf16_ok(g, bm, case.setenv) else (1, bm, 0)], [sp]


# ---- split-count classes ----------------------------------------------------------------------------------------------------------
SPLITS = {
    "1": lambda s: s == 1,
    "2-7": lambda s: 2 <= s <= 7,
    "8": lambda s: s == 8,
    "9-15": lambda s: 9 <= s <= 15,
    "17+odd8": lambda s: s >= 17 and s % 8 != 0,
    ">1": lambda s: s > 1,
    ">=1": lambda s: s >= 1,
}


def splits_ok(cls, recorded):
    """`recorded`: one entry per launch.  `cls`: a class of SPLITS that every launch must fall in, or the per-class split counts
    of an igemm_multi launch as a tuple (its record carries the largest; predict() restates all of them)."""
    if isinstance(cls, tuple):
        return [max(r) if isinstance(r, tuple) else r for r in recorded] == [max(cls)]
    return all(SPLITS[cls](max(s) if isinstance(s, tuple) else s) for s in recorded)


def slab_cap(case, pred):
    """The most partial sums the case's route can add to an element (the `slabs` of conv_oracle.bound): 64 for plan_splits and
    try_igemm_multi, 32 for try_pgemm (igemm.hip: splitk_room_floats), the persistent grids' caps for the small-channel weight
    gradients and min(ceil(T / 4), 512) for wgrad_plan; 1 (the accumulator itself) where the route has no second pass."""
    kind, cfg, route = pred[0]
    if case.op != "wgrad":
        return 1 if kind == 2 else (32 if cfg in (1064, 1128, B16_CFG[1064], B16_CFG[1128]) else 64)
    if kind in (1, 3):
        return 512
    if route in (SR_TO1WGRADW + 3, SR_TO1WGRADW + 4):
        B, H, W, Cin, Cout, k, s, pad = case.geom
        return B * cdiv(CO.out_size(H, k, s, pad), 4)
    return {SR_TO1WGRAD_LDS: 768, SR_TO1WGRAD_LDS_BNIN: 768, SR_TO1WGRAD64 + 3: 1024, SR_TO1WGRAD64 + 4: 1024}.get(route, 512)


# ---- the table --------------------------------------------------------------------------------------------------------------------
class Case:
    """prec: 'f32' | 'bf16' (tg_hip.ops.set_precision around the launch under test);  env: a switch the library reads once per
    process (the case runs in a child);  setenv: a switch it reads per call, set around the launch."""

    def __init__(self, id, geom, op, mods, expect, splits="1", env=None, prec="f32", setenv=None):
        self.id, self.geom, self.op, self.mods, self.splits, self.env = id, geom, op, frozenset(mods.split()), splits, env
        self.expect = [expect] if isinstance(expect[0], int) else list(expect)
        self.prec, self.setenv = prec, setenv

    @property
    def rounds(self):
        """The case runs on a bf16 direct kernel: its reference is the convolution of the operands rounded to bf16."""
        return self.prec == "bf16" and all(kind == 3 for kind, _, _ in self.expect)

    def __repr__(self):
        return self.id


def I(cfg):
    return (0, cfg, 0)


def F(route):
    return (2, SMALL_FWD, route)


def Wg(bm):
    return (1, bm, 0)


def Ws(route):
    return (2, SMALL_WGRAD, route)


# modifiers: mask (input mask; forward: + ratio in the real run), bias, relu | leaky (forward activation; a backward run's dy
# then comes through the activation's backward from the kernel's own forward output), gate (dgrad: fused activation backward from
# a float gate source), acc (dgrad: accumulate into out=), bnin (BatchNorm-on-load)
CASES = []


def case(*a, **k):
    CASES.append(Case(*a, **k))


# ---- gathered-row kernel (igemm_kernel): cfg = BN (+ 1 for the scalar gather, Cin % 4 != 0) ---------------------------------------
case("ig33_c3_s2", (2, 9, 11, 3, 24, 3, 2, 1), "fwd", "mask bias leaky", I(33))
case("ig32_s2_split2", (2, 9, 11, 8, 24, 3, 2, 1), "fwd", "bias", I(32), "2-7")
case("ig65_c6_5x5", (3, 13, 15, 6, 96, 5, 1, 2), "fwd", "mask", I(65))
case("ig65_n34_ragged", (2, 13, 15, 3, 34, 3, 2, 1), "fwd", "bias relu", I(65))
case("ig64_s2_split2", (3, 13, 15, 16, 96, 3, 2, 1), "fwd", "mask bias leaky", I(64), "2-7")
case("ig129_c3_s2", (2, 13, 15, 3, 128, 3, 2, 1), "fwd", "bias", I(129))
case("ig128_1x1_ragged_m", (2, 13, 15, 16, 128, 1, 1, 0), "fwd", "mask bias leaky", I(128))
case("ig32_dgrad_5x5_split5", (1, 9, 11, 16, 24, 5, 1, 2), "dgrad", "mask gate", I(32), "2-7")
# split-K on tiny grids: the second pass's groups of eight slabs + a tail of up to seven, and its scalar branch (N % 4 != 0)
case("splitk_6", (1, 4, 4, 96, 128, 3, 1, 1), "fwd", "bias", I(128), "2-7")
case("splitk_8", (2, 8, 8, 64, 128, 4, 2, 1), "fwd", "mask bias leaky", I(128), "8")
case("splitk_9", (1, 4, 4, 128, 128, 3, 1, 1), "fwd", "", I(128), "9-15")
case("splitk_11", (1, 4, 4, 192, 128, 3, 1, 1), "fwd", "bias relu", I(128), "9-15")
case("splitk_18", (2, 8, 8, 256, 64, 3, 1, 1), "fwd", "mask", I(64), "17+odd8")
case("splitk_36", (1, 8, 8, 512, 128, 3, 2, 1), "fwd", "mask bias leaky", I(128), "17+odd8")
case("splitk_9_n34_scalar", (1, 4, 4, 128, 34, 3, 1, 1), "fwd", "mask bias leaky", I(64), "9-15")
case("splitk_18_n34_scalar", (1, 5, 5, 256, 34, 3, 2, 1), "fwd", "bias", I(64), "17+odd8")
case("splitk_dgrad_acc", (1, 4, 4, 128, 256, 3, 1, 1), "dgrad", "mask acc", I(128), "17+odd8")
# ---- patch kernel (pgemm_kernel): cfg = 1000 + BN ---------------------------------------------------------------------------------
case("pg64_whole_3x3", (1, 16, 16, 32, 96, 3, 1, 1), "fwd", "mask bias leaky", I(1064))
case("pg64_over_4x4", (1, 18, 19, 32, 48, 4, 1, 1), "fwd", "bias", I(1064))
case("pg128_whole_1x1", (1, 8, 16, 32, 128, 1, 1, 0), "fwd", "mask", I(1128))
case("pg128_over_2x2", (1, 18, 19, 32, 128, 2, 1, 0), "fwd", "bias relu", I(1128))
case("pg128_over_4x4", (2, 18, 19, 64, 128, 4, 1, 1), "fwd", "mask bias leaky", I(1128))
case("pg64_splitk2", (1, 16, 16, 128, 96, 1, 1, 0), "fwd", "mask bias leaky", I(1064), "2-7")
case("pg128_splitk4", (1, 8, 16, 256, 128, 2, 1, 1), "fwd", "bias", I(1128), "2-7")
case("pg64_n50_scalar_store", (1, 18, 19, 32, 50, 3, 1, 1), "fwd", "mask bias leaky", I(1064))          # N % 4 != 0: no wide stores
case("pg64_n50_splitk2_scalar", (1, 16, 16, 128, 50, 1, 1, 0), "fwd", "bias", I(1064), "2-7")
case("pg128_dgrad_2x2_gate", (1, 17, 18, 128, 32, 2, 1, 0), "dgrad", "mask gate", I(1128))
case("pg64_dgrad_1x1_acc", (1, 16, 16, 64, 64, 1, 1, 0), "dgrad", "acc", I(1064))
case("pg128_merged4_dgrad", (16, 64, 64, 128, 32, 3, 2, 1), "dgrad", "mask", I(1128))
# ---- the parity classes of a stride-2 dgrad in one gathered-row launch (igemm_multi_kernel): cfg = 500 + BN ------------------------
case("multi128_small_grid", (1, 32, 32, 128, 32, 3, 2, 1), "dgrad", "mask", I(628), (1, 1, 1, 1))
case("multi128_per_class", (1, 9, 9, 128, 128, 3, 2, 1), "dgrad", "mask gate", I(628), (1, 2, 2, 4))
case("multi128_per_class_8", (2, 8, 8, 128, 256, 3, 2, 1), "dgrad", "acc", I(628), (2, 4, 4, 8))
case("multi64_per_class", (1, 7, 9, 96, 128, 3, 2, 1), "dgrad", "mask", I(564), (1, 2, 2, 4))
case("multi64_per_class_8", (2, 8, 8, 64, 256, 3, 2, 1), "dgrad", "gate", I(564), (2, 4, 4, 8))
# ... and class by class where the merged launches do not apply: stride 3 (nine classes), N <= 32
case("classes_stride3", (2, 10, 13, 64, 32, 3, 3, 1), "dgrad", "mask", [I(64)] * 9)
case("classes_n24", (2, 9, 11, 24, 64, 3, 2, 1), "dgrad", "mask acc", [I(32)] * 4, ">=1")
case("classes_n24_scalar", (2, 9, 11, 24, 6, 3, 2, 1), "dgrad", "gate", [I(33)] * 4)
# ---- 1 -> N channels (forward of enc1 / D conv0 / VGG conv1_1; dgrad of `final` and D's last conv) ----------------------------------
case("c1mfma7", (2, 19, 21, 1, 64, 7, 2, 3), "fwd", "mask bias leaky", F(SR_C1MFMA + 7))
case("c1mfma4", (2, 19, 21, 1, 128, 4, 2, 1), "fwd", "bias leaky", F(SR_C1MFMA + 4))
case("c1mfma3", (2, 33, 21, 1, 64, 3, 1, 1), "fwd", "mask bias relu", F(SR_C1MFMA + 3))
case("c1mfma3_dgrad_final", (2, 9, 12, 64, 1, 3, 1, 1), "dgrad", "gate", F(SR_C1MFMA + 3))
case("c1mfma4_dgrad_dlast", (2, 6, 7, 128, 1, 4, 1, 1), "dgrad", "acc", F(SR_C1MFMA + 4))
case("c1conv0_5x5", (2, 19, 21, 1, 64, 5, 1, 2), "fwd", "mask bias leaky", F(SR_C1CONV))
case("c1conv0_dgrad_classes", (2, 10, 13, 64, 1, 3, 2, 1), "dgrad", "gate", [F(SR_C1CONV)] * 4)
# ---- C -> 1 channel ------------------------------------------------------------------------------------------------------------------
case("to1convw_256_3", (2, 6, 7, 256, 1, 3, 1, 1), "fwd", "bias", F(SR_TO1CONVW + 31))
case("to1convw_256_4", (2, 6, 7, 256, 1, 4, 1, 1), "fwd", "mask bias leaky", F(SR_TO1CONVW + 41))
case("to1convw_512_3", (2, 6, 7, 512, 1, 3, 1, 1), "fwd", "mask bias", F(SR_TO1CONVW + 32))
case("to1convw_512_4", (3, 4, 2, 512, 1, 4, 1, 1), "fwd", "bias", F(SR_TO1CONVW + 42))
case("to1convw_grid_cap", (1, 112, 111, 256, 1, 3, 1, 1), "fwd", "bias", F(SR_TO1CONVW + 31))        # 12432 outputs: 1036 > 1024 blocks
case("to1_lds_ragged", (2, 17, 20, 64, 1, 3, 1, 1), "fwd", "mask bias leaky", F(SR_TO1_LDS))
case("to1_lds_whole", (1, 8, 32, 64, 1, 3, 1, 1), "fwd", "bias", F(SR_TO1_LDS))
case("to1_lds_bnin_ragged", (2, 17, 20, 64, 1, 3, 1, 1), "fwd", "bias bnin", F(SR_TO1_LDS_BNIN))
case("to1_lds_bnin_whole", (1, 8, 32, 64, 1, 3, 1, 1), "fwd", "bias bnin", F(SR_TO1_LDS_BNIN))
case("to1_lds_map_ragged", (2, 17, 20, 1, 64, 3, 1, 1), "dgrad", "map", F(SR_TO1_LDS_MAP))
case("to1_lds_map_whole", (1, 32, 32, 1, 64, 3, 1, 1), "dgrad", "map", F(SR_TO1_LDS_MAP))
case("to1_lds_dgrad_c1_k3", (2, 17, 20, 1, 64, 3, 1, 1), "dgrad", "mask acc", F(SR_TO1_LDS))
case("to1conv64_33_h3", (2, 3, 20, 64, 1, 3, 1, 1), "fwd", "mask bias leaky", F(SR_TO1CONV64 + 33))
case("to1conv64_44", (2, 7, 9, 64, 1, 4, 1, 1), "fwd", "bias", F(SR_TO1CONV64 + 44))
case("to1conv64_classes_3x3_s2", (2, 14, 16, 1, 64, 3, 2, 1), "dgrad", "mask",
     [F(SR_TO1CONV64 + 11), F(SR_TO1CONV64 + 12), F(SR_TO1CONV64 + 21), F(SR_TO1CONV64 + 22)])
case("multi22_lds", (2, 18, 32, 1, 64, 4, 2, 1), "dgrad", "", (2, TO1_MULTI, SR_MULTI22_LDS))
case("multi22_lds_acc", (1, 8, 40, 1, 64, 4, 2, 1), "dgrad", "acc", (2, TO1_MULTI, SR_MULTI22_LDS))
case("multi22_below_tile", (2, 6, 8, 1, 64, 4, 2, 1), "dgrad", "", (2, TO1_MULTI, SR_MULTI22))
case("multi22_masked", (2, 18, 32, 1, 64, 4, 2, 1), "dgrad", "mask", (2, TO1_MULTI, SR_MULTI22_LDS))
# ---- weight gradients: wgrad_kernel, cfg = BM -------------------------------------------------------------------------------------------
case("wg32_c3", (2, 9, 11, 3, 24, 3, 2, 1), "wgrad", "mask bias", Wg(32))
case("wg32_rowseg_split2", (1, 8, 32, 8, 24, 3, 1, 1), "wgrad", "bias", Wg(32), ">1")
case("wg32_c3_reduce_n162", (2, 33, 35, 3, 6, 3, 1, 1), "wgrad", "mask leaky", Wg(32), ">1")
case("wg64_c6", (2, 13, 15, 6, 96, 3, 2, 1), "wgrad", "mask", Wg(64))
case("wg64_c16", (2, 13, 15, 16, 96, 3, 2, 1), "wgrad", "bias", Wg(64))
case("wg64_c3_cout128", (2, 13, 15, 3, 128, 3, 2, 1), "wgrad", "", Wg(64))
case("wg64_rowseg_split2", (2, 8, 64, 16, 96, 3, 2, 1), "wgrad", "mask leaky", Wg(64), ">1")
case("wg64_masked_3x3_split8", (2, 16, 32, 64, 64, 3, 1, 1), "wgrad", "mask bias", Wg(64), ">1")
case("wg128_c16", (2, 13, 15, 16, 128, 3, 2, 1), "wgrad", "mask bias", Wg(128))
case("wg128_rowseg_split2", (1, 8, 32, 16, 128, 1, 1, 0), "wgrad", "", Wg(128), ">1")
case("wg64_c6_split8", (2, 21, 23, 6, 96, 3, 1, 1), "wgrad", "mask bias", Wg(64), ">1")
case("wg128_split5", (2, 33, 35, 16, 128, 3, 2, 1), "wgrad", "mask", Wg(128), ">1")
case("wg128_rowseg_split1", (1, 4, 32, 16, 128, 3, 1, 1), "wgrad", "bias", Wg(128))
case("wg64_rowseg_split1", (1, 2, 32, 64, 96, 3, 1, 1), "wgrad", "mask", Wg(64))
case("wg32_rowseg_split1", (1, 2, 32, 8, 24, 3, 1, 1), "wgrad", "", Wg(32))
# ---- weight gradients of the 1-channel-side layers ----------------------------------------------------------------------------------------
case("c1wgrad_mfma7_bias", (2, 19, 21, 1, 64, 7, 2, 3), "wgrad", "mask bias", Ws(SR_C1WGRAD_MFMA_BIAS + 7))
case("c1wgrad_mfma4_bias", (2, 19, 21, 1, 128, 4, 2, 1), "wgrad", "bias leaky", Ws(SR_C1WGRAD_MFMA_BIAS + 4))
case("c1wgrad_mfma3_bias", (2, 33, 21, 1, 64, 3, 1, 1), "wgrad", "mask bias", Ws(SR_C1WGRAD_MFMA_BIAS + 3))
case("c1wgrad_mfma7", (2, 19, 21, 1, 64, 7, 2, 3), "wgrad", "", Ws(SR_C1WGRAD_MFMA + 7))
case("c1wgrad_mfma4", (2, 19, 21, 1, 64, 4, 2, 1), "wgrad", "mask", Ws(SR_C1WGRAD_MFMA + 4))
case("c1wgrad_mfma3", (2, 33, 21, 1, 64, 3, 1, 1), "wgrad", "", Ws(SR_C1WGRAD_MFMA + 3))
case("c1wgrad_mfma3_513_tiles", (3, 130, 290, 1, 64, 3, 1, 1), "wgrad", "mask bias", Ws(SR_C1WGRAD_MFMA_BIAS + 3))
case("to1wgradw3_256", (2, 6, 7, 256, 1, 3, 1, 1), "wgrad", "bias", Ws(SR_TO1WGRADW + 3))
case("to1wgradw4_512", (2, 6, 7, 512, 1, 4, 1, 1), "wgrad", "mask", Ws(SR_TO1WGRADW + 4))
case("to1wgradw3_768", (2, 6, 7, 768, 1, 3, 1, 1), "wgrad", "mask bias", Ws(SR_TO1WGRADW + 3))
case("to1wgradw4_1024", (3, 4, 2, 1024, 1, 4, 1, 1), "wgrad", "", Ws(SR_TO1WGRADW + 4))
case("to1wgrad_lds", (2, 17, 20, 64, 1, 3, 1, 1), "wgrad", "mask bias", Ws(SR_TO1WGRAD_LDS))
case("to1wgrad_lds_770_tiles", (2, 220, 112, 64, 1, 3, 1, 1), "wgrad", "mask", Ws(SR_TO1WGRAD_LDS))
case("to1wgrad_lds_bnin", (2, 17, 20, 64, 1, 3, 1, 1), "wgrad", "bias bnin", Ws(SR_TO1WGRAD_LDS_BNIN))
case("to1wgrad_lds_bnin_whole", (1, 8, 32, 64, 1, 3, 1, 1), "wgrad", "bnin", Ws(SR_TO1WGRAD_LDS_BNIN))
case("to1wgrad64_3_h3", (2, 3, 20, 64, 1, 3, 1, 1), "wgrad", "mask bias", Ws(SR_TO1WGRAD64 + 3))
case("to1wgrad64_4", (2, 7, 9, 64, 1, 4, 1, 1), "wgrad", "", Ws(SR_TO1WGRAD64 + 4))
case("to1wgrad64_4_1036_blocks", (2, 365, 365, 64, 1, 4, 1, 1), "wgrad", "", Ws(SR_TO1WGRAD64 + 4))
# ---- routes behind a switch that is read once per process: one fresh child process per switch ----------------------------------------------
case("c1conv7", (2, 19, 21, 1, 64, 7, 2, 3), "fwd", "mask bias leaky", F(SR_C1CONV + 7), env="TG_NO_C1MFMA")
case("c1conv4", (2, 19, 21, 1, 128, 4, 2, 1), "fwd", "bias", F(SR_C1CONV + 4), env="TG_NO_C1MFMA")
case("c1conv3", (2, 33, 21, 1, 64, 3, 1, 1), "fwd", "mask bias relu", F(SR_C1CONV + 3), env="TG_NO_C1MFMA")
case("c1conv3_dgrad", (2, 9, 12, 64, 1, 3, 1, 1), "dgrad", "gate", F(SR_C1CONV + 3), env="TG_NO_C1MFMA")
case("c1wgrad7", (2, 19, 21, 1, 64, 7, 2, 3), "wgrad", "mask bias", Ws(SR_C1WGRAD + 7), env="TG_C1WGRAD")
case("c1wgrad4", (2, 19, 21, 1, 128, 4, 2, 1), "wgrad", "bias", Ws(SR_C1WGRAD + 4), env="TG_C1WGRAD")
case("c1wgrad3", (2, 33, 21, 1, 64, 3, 1, 1), "wgrad", "mask", Ws(SR_C1WGRAD + 3), env="TG_C1WGRAD")
case("c1wgrad3_513_tiles", (3, 130, 290, 1, 64, 3, 1, 1), "wgrad", "bias", Ws(SR_C1WGRAD + 3), env="TG_C1WGRAD")
case("to1conv64_33_nolds", (2, 17, 20, 64, 1, 3, 1, 1), "fwd", "mask bias leaky", F(SR_TO1CONV64 + 33), env="TG_NO_TO1LDS")
case("multi22_nolds", (2, 18, 32, 1, 64, 4, 2, 1), "dgrad", "acc", (2, TO1_MULTI, SR_MULTI22), env="TG_NO_TO1LDS")
case("to1wgrad64_3_nolds", (2, 17, 20, 64, 1, 3, 1, 1), "wgrad", "mask bias", Ws(SR_TO1WGRAD64 + 3), env="TG_NO_TO1LDS")

ENVS = ("TG_NO_C1MFMA", "TG_C1WGRAD", "TG_NO_TO1LDS")
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
HERE = [c for c in CASES if c.env is None]

# ---- the same kernels' BF16 = true instantiations, and wgrad_bf16_kernel (tests/test_hip_bf16_direct.py) ------------------------------
# Every case runs in bf16 mode.  The kernels round the two MFMA operands to bf16 (RNE) when they stage them into LDS and nothing
# else, so a case on a bf16 kernel (Case.rounds) faces the oracle on the ROUNDED operands with the unchanged fp32 bound; the
# integers of the exact run are bf16 numbers.  Records: gathered-row 3000 + BN, patch 3200 + BN, merged 3500 + BN, wgrad 3700 + BM.
B16_CASES = []


def Bf(cfg):
    return (3, cfg, 0)


def b16(id, src, expect, splits=None, **k):
    """A bf16-mode case: `src` = (geometry, op, modifiers), or the id of the fp32 case whose geometry, op, modifiers (and split
    class, unless given: the bf16 launchers share the fp32 planners) it takes."""
    if isinstance(src, str):
        c = BY_ID[src]
        src, splits = (c.geom, c.op, " ".join(sorted(c.mods))), c.splits if splits is None else splits
    B16_CASES.append(Case(id, src[0], src[1], src[2], expect, splits or "1", prec="bf16", **k))


# gathered-row kernel (igemm_kernel<.., BF16>): 3000 + BN
b16("b16_ig64_s2_split2", "ig64_s2_split2", Bf(3064))
b16("b16_ig64_n34_ragged", ((2, 13, 15, 8, 34, 3, 2, 1), "fwd", "bias relu"), Bf(3064), "2-7")         # ragged N, scalar stores
b16("b16_ig128_1x1_ragged_m", "ig128_1x1_ragged_m", Bf(3128))
# Cin % 8 != 0: one 32-wide chunk is mostly zero padding, and half of an 8-wide bf16 LDS read is padding
b16("b16_ig64_c12", ((2, 9, 11, 12, 64, 3, 2, 1), "fwd", "mask bias"), Bf(3064), "2-7")
b16("b16_ig64_c20", ((2, 9, 11, 20, 64, 3, 1, 1), "fwd", "bias"), Bf(3064), "2-7")
b16("b16_ig128_c36_tail", ((2, 9, 11, 36, 128, 3, 2, 1), "fwd", "mask"), Bf(3128), "2-7")               # a full chunk + a 4-channel tail
b16("b16_ig64_d4x4s2", ((2, 32, 32, 64, 64, 4, 2, 1), "fwd", "bias leaky"), Bf(3064), "8")              # F(2x2,2x2) in fp32 mode
b16("b16_splitk_9", "splitk_9", Bf(3128))
b16("b16_splitk_11", "splitk_11", Bf(3128))
b16("b16_splitk_18_n34_scalar", "splitk_18_n34_scalar", Bf(3064))
b16("b16_splitk_36", "splitk_36", Bf(3128))
b16("b16_splitk_dgrad_acc", "splitk_dgrad_acc", Bf(3128))
b16("b16_classes_stride3", ((2, 10, 13, 64, 64, 3, 3, 1), "dgrad", "mask"), [Bf(3064)] * 9)
# patch kernel (pgemm_kernel<.., BF16>): 3200 + BN
for _id in ("pg64_whole_3x3", "pg64_over_4x4", "pg64_splitk2", "pg64_n50_scalar_store", "pg64_n50_splitk2_scalar", "pg64_dgrad_1x1_acc"):
    b16("b16_" + _id, _id, Bf(3264))
for _id in ("pg128_whole_1x1", "pg128_over_2x2", "pg128_over_4x4", "pg128_splitk4", "pg128_dgrad_2x2_gate", "pg128_merged4_dgrad"):
    b16("b16_" + _id, _id, Bf(3328))
# the four 2x2-tap classes of a discriminator layer, merged: 4 x 128 work items, the least the merged patch launch takes
b16("b16_pg128_merged4_d4x4s2", ((16, 64, 64, 128, 64, 4, 2, 1), "dgrad", "mask"), Bf(3328))
# merged gathered-row launch (igemm_multi_kernel<.., true>): 3500 + BN
for _id in ("multi128_small_grid", "multi128_per_class", "multi128_per_class_8"):
    b16("b16_" + _id, _id, Bf(3628))
for _id in ("multi64_per_class", "multi64_per_class_8"):
    b16("b16_" + _id, _id, Bf(3564))
# weight gradient (wgrad_bf16_kernel): 3700 + BM
b16("b16_wg128_rowseg_split2", "wg128_rowseg_split2", Bf(3828))
b16("b16_wg64_rowseg_split2", "wg64_rowseg_split2", Bf(3764))
b16("b16_wg64_masked_3x3_split8", "wg64_masked_3x3_split8", Bf(3764))
b16("b16_wg128_rowseg_split1", "wg128_rowseg_split1", Bf(3828))
b16("b16_wg64_rowseg_split1", "wg64_rowseg_split1", Bf(3764))
b16("b16_wg64_36_rows_k72", ((1, 4, 32, 8, 36, 3, 1, 1), "wgrad", "mask bias"), Bf(3764))              # 36 of 64 rows, Ktot 72 < 128
b16("b16_wg128_ragged_bm_k180", ((2, 4, 32, 20, 160, 3, 1, 1), "wgrad", "bias"), Bf(3828), ">=1")      # 160 = 128 + 32, Ktot 180 = 128 + 52
b16("b16_wg64_5x5_s2", ((1, 9, 64, 16, 96, 5, 2, 2), "wgrad", "mask"), Bf(3764), ">=1")                # Wo = 32
b16("b16_wg128_image_edges", ((3, 2, 32, 16, 128, 3, 1, 1), "wgrad", ""), Bf(3828), ">=1")             # image boundaries inside the K walk
# precision must not leak: these stay on the fp32 kernels in bf16 mode -- the fp32 record, the UNROUNDED reference
for _id in ("ig33_c3_s2", "ig65_c6_5x5", "ig32_dgrad_5x5_split5", "classes_n24", "wg32_c3", "wg64_c6", "c1mfma7", "to1_lds_ragged",
            "to1convw_256_3", "multi22_lds", "c1wgrad_mfma3_bias", "to1wgrad_lds"):
    b16("b16_keeps_" + _id, _id, BY_ID[_id].expect)
b16("b16_keeps_wg64_wo8", ((2, 13, 16, 16, 96, 3, 2, 1), "wgrad", "mask bias"), Wg(64))                 # Wo = 8, no multiple of 32
b16("b16_keeps_wg64_behind_switch", "wg64_rowseg_split2", Wg(64), setenv="TG_NO_BF16_WGRAD")
B16_BY_ID = {c.id: c for c in B16_CASES}
assert len(B16_BY_ID) == len(B16_CASES) and not set(B16_BY_ID) & set(BY_ID)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
LEAKY_SLOPE = float(np.float32(0.2))           # the C ABI takes slopes as float: the fp32 value nearest 0.2, on every side


def fwd_act(case, mode):
    """(act, slope) of the case's forward: the exact run has no LeakyReLU (a slope of 0.2 leaves the integers)."""
    if "relu" in case.mods or ("leaky" in case.mods and mode == "exact"):
        return CO.ACT_RELU, 0.0
    return (CO.ACT_LEAKY, LEAKY_SLOPE) if "leaky" in case.mods else (CO.ACT_NONE, 0.0)


def make_inputs(case, mode):
    """fp32 arrays of the case in `mode`: 'exact' = integers of {-3 ... 3}, 0/1 mask, no ratio, identity BatchNorm; 'real' = normals,
    the partial convolution's ratio k^2 / sum(mask) where the case is masked, positive rstd and gamma."""
    B, H, W, Cin, Cout, k, s, pad = case.geom
    Ho, Wo = CO.out_size(H, k, s, pad), CO.out_size(W, k, s, pad)
    rng = np.random.default_rng(sum(case.geom) * 7 + len(case.id) + (0 if mode == "exact" else 1))
    if mode == "exact":
        draw = lambda *shape: rng.integers(-3, 4, size=shape).astype(np.float32)
    else:
        draw = lambda *shape: rng.standard_normal(size=shape, dtype=np.float32)
    d = {"x": draw(B, H, W, Cin), "w": draw(Cout, k, k, Cin), "dy": draw(B, Ho, Wo, Cout)}
    if mode == "real":
        d["w"] *= np.float32(1.0 / (k * math.sqrt(Cin)))
    d["bias"] = draw(Cout) if "bias" in case.mods else None
    d["mask"] = (rng.random((B, H, W)) > 0.3).astype(np.float32) if "mask" in case.mods else None
    d["ratio"] = None
    if d["mask"] is not None and mode == "real":
        ssum = CO.conv_fwd(d["mask"][..., None], np.ones((1, k, k, 1)), k, s, pad).val[..., 0]
        d["ratio"] = np.where(ssum > 0, (k * k) / np.maximum(ssum, 1.0), 0.0).astype(np.float32)
    d["gate"] = draw(B, H, W, Cin) if "gate" in case.mods else None
    d["base"] = draw(B, H, W, Cin) if "acc" in case.mods else None
    d["bn"] = None
    if "bnin" in case.mods:
        if mode == "exact":
            d["bn"] = (np.zeros(Cin, np.float32), np.ones(Cin, np.float32), np.ones(Cin, np.float32), np.zeros(Cin, np.float32),
                       CO.ACT_RELU, 0.0)
        else:
            d["bn"] = (draw(Cin) * np.float32(0.3), np.float32(0.5) + rng.random(Cin, dtype=np.float32),
                       np.float32(0.5) + rng.random(Cin, dtype=np.float32), draw(Cin) * np.float32(0.3), CO.ACT_LEAKY, LEAKY_SLOPE)
    if "map" in case.mods:
        # tg_conv_dgrad_sparse: prediction and target agree except on a block; dx is wanted where they differ or mask != 1
        pred = draw(B, H, W)
        tgt = pred.copy()
        tgt[:, 2:H // 2, 3:W // 2] += np.float32(1.0)
        d["pred"], d["tgt"] = pred, tgt
        d["needed"] = pred != tgt
    return d


OPERANDS = {"fwd": ("x", "w"), "dgrad": ("dy", "w"), "wgrad": ("x", "dy")}


def round_operands(case, d, rnd=CO.bf16_rne):
    """The arrays with the two MFMA operands of the case's op passed through `rnd` and `dy_bias` = the dy as drawn: the bias
    gradient is the fp32 column sum of the unrounded dy.  (The 0/1 mask multiply that precedes the rounding in the kernels
    commutes with it.)"""
    assert d["bn"] is None, "no bf16 kernel applies BatchNorm on load"
    out = dict(d, dy_bias=d["dy"])
    for name in OPERANDS[case.op]:
        out[name] = rnd(d[name])
    return out


def reference(case, d, mode):
    """The oracle's results for the arrays of make_inputs (and, for a backward run behind an activation, the dy the test derived
    from the kernel's own forward output): {'y' | 'dx' | 'dw', 'db'} -> conv_oracle.Res.  A case on a bf16 kernel (Case.rounds):
    for those arrays with the MFMA operands rounded to bf16."""
    B, H, W, Cin, Cout, k, s, pad = case.geom
    a, sl = fwd_act(case, mode)
    if case.rounds and "dy_bias" not in d:
        d = round_operands(case, d)
    if case.op == "fwd":
        return {"y": CO.conv_fwd(d["x"], d["w"], k, s, pad, d["mask"], d["bias"], d["ratio"], a, sl, d["bn"])}
    if case.op == "dgrad":
        r = CO.conv_dgrad(d["dy"], d["w"], (B, H, W, Cin), k, s, pad, d["mask"], d["gate"],
                          CO.ACT_RELU if mode == "exact" else CO.ACT_LEAKY, LEAKY_SLOPE, d["base"])
        if "map" in case.mods:
            keep = d["needed"][..., None].astype(np.float64)
            r = r._replace(val=r.val * keep, S=r.S * keep)
        return {"dx": r}
    rw, rb = CO.conv_wgrad(d["x"], d["dy"], k, s, pad, d["mask"], d["bn"], d.get("dy_bias"))
    return {"dw": rw, "db": rb} if "bias" in case.mods else {"dw": rw}


def needs_forward(case, mode):
    """A backward case behind an activation: its dy comes through the activation's backward from a forward output."""
    return case.op != "fwd" and fwd_act(case, mode)[0] != CO.ACT_NONE


def forward_args(case, d, mode):
    """conv_oracle.conv_fwd arguments of the forward a backward case hangs on."""
    B, H, W, Cin, Cout, k, s, pad = case.geom
    a, sl = fwd_act(case, mode)
    return dict(x=d["x"], w=d["w"], k=k, s=s, p=pad, mask=d["mask"], bias=None, ratio=d["ratio"], act_kind=a, slope=sl, in_bn=d["bn"])


def backward_dy(case, d, mode, y):
    """dz = gy * act'(y) * ratio in fp32, gy = the drawn dy and y = the forward output THE CODE UNDER TEST produced: an output
    within rounding of zero may have the other sign in fp64, and one flipped gate moves a gradient by a whole term.  That is
    the activation's discontinuity, not an error of the (linear) dgrad / wgrad kernels, which get this dz as their input."""
    a, sl = fwd_act(case, mode)
    dz = d["dy"] * np.where(np.asarray(y, np.float32) > 0, np.float32(1.0), np.float32(sl if a == CO.ACT_LEAKY else 0.0))
    if d["ratio"] is not None:
        dz = dz * d["ratio"][..., None]
    return dz.astype(np.float32)
