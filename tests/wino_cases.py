"""Case table of the Winograd kernels (csrc/wino.inc: wino_kernel / wino_pipe_kernel / wino_wgrad_kernel; wino16.inc: their bf16
twins; wino22.inc: wino22_kernel / wino22_wgrad_kernel; wino44.inc: wino44_kernel), one kernel instantiation per case, shared by
tests/test_hip_wino_routes.py (GPU: the launch records must show exactly the expected (kind, cfg, route) and split count, then
the exact-integer run and, where the case has one, the a-priori-bound run of tests/conv_oracle.py) and
tests/test_wino_oracle_cpu.py (CPU: the oracle against float64 autograd, the exactness and sensitivity conditions, an fp32
emulation of each algorithm inside the bound, and `predict` = the expectation).

Runs: 'exact' (integers of {-3 ... 3}: bit equality), 'real' (normals: the a-priori bound of any fp32 evaluation) and, for the
cases on a kernel of wino16.inc, 'rounded': integers of eleven bits (twelve: GRID_WIDE), on which the fp32 transforms are exact and the bf16 rounding of
the transformed operands is NOT the identity, against the reference that rounds them to nearest-even as the kernel must -- the
same fp32 bound then holds per element, and truncation, round-half-away or a rounding ahead of the transforms miss it by far.

`predict` restates the host-side planners (wino_geom_ok, wino_plan, launch_wino22, wino44_ok, wino_wgrad_plan and its twins,
s2d_ok, choose_splits, choose_splits_k) in Python on top of tests/conv_cases.py, for a workspace of the size the queries report.
The table's expectations are literals; the restatement only has to agree with them, and the GPU has the last word.

Routes (WinoRoute, csrc/igemm_params.h) = 1 + the index into the launcher's kernel table."""
import math

import numpy as np

from tests import conv_cases as CC
from tests import conv_oracle as CO
from tests.conv_cases import cdiv, choose_splits, s2d_ok

PLAN_CUS = 256
# launch_wino's table (cfg 4064; the first eight also cfg 4016)
R_PLAIN, R_GATE, R_FAST, R_FAST_GATE, R_PIPE, R_PIPE_GATE, R_POOL, R_GBITS = range(1, 9)
R_QUEUED = 8                                    # + the static walk's route
R_MAP, R_MAP_POOL, R_LIST, R_LIST_GATE, R_LIST_GBITS = 17, 18, 19, 20, 21
MAP_ROUTES = (R_MAP, R_MAP_POOL, R_LIST, R_LIST_GATE, R_LIST_GBITS)
# launch_wino22's (cfg 4022): 1 + (queue ? 4 : 0) + (fast ? 2 : 0) + gate;  launch_wino44's (cfg 4044): plain, gate, bit gate
W22_FAST, W22_QUEUED = 2, 4
R44_PLAIN, R44_GATE, R44_GBITS = 1, 2, 3


def choose_splits_k(tiles, max_splits, slots, ksteps, slab_steps=0.0):
    max_splits = max(max_splits, 1)
    best, best_cost = 1, 1e300
    for sp in range(1, max_splits + 1):
        blocks = tiles * sp
        rounds = cdiv(blocks, slots)
        cost = float(rounds) * (float(cdiv(ksteps, sp)) + 4.0) + slab_steps * float(blocks)
        if cost < best_cost * 0.995:
            best_cost, best = cost, sp
    return best


def splitk_room(out):
    return min(out * 64, 64 << 20)


def wino_plan(B, OH, OW, C, N, bf16=False, amask=False, gate=False, gbits=False, pool=False, acc=False, env=None):
    """dict(splits, fast, pipe, gated, pool, gbits, ki, last) of an F(2x2,3x3) launch on the plain dst grid (static walk)."""
    kc = 16 if bf16 else 8
    total = cdiv(OW, 16) * cdiv(OH, 16) * B * (N // 64)
    M = B * OH * OW
    nchunks, splits = C // kc, 1
    if nchunks >= 16:
        smax = min(nchunks // 8, 16)
        while smax > 1 and smax * M * N > splitk_room(M * N):
            smax -= 1
        splits = choose_splits(total, smax, PLAN_CUS)
    cps = cdiv(nchunks, splits)
    splits = cdiv(nchunks, cps)
    one, last = splits == 1, nchunks - (splits - 1) * cps
    fast = env != "TG_WINO_NO_FAST" and not amask
    gated = gate and one
    pipe = fast and env != "TG_WINO_NO_PIPE" and last >= 2 and cps >= 2
    pool = pool and pipe and not gated and one and OH % 2 == 0 and OW % 2 == 0 and not acc
    gbits = gbits and pipe and one
    ki = 7 if gbits else 6 if pool else 4 + gated if pipe else (2 if fast else 0) + gated
    return dict(splits=splits, fast=fast, pipe=pipe, gated=gated, pool=pool, gbits=gbits, ki=ki, last=last, items=total)


def wino_geom_ok(OH, OW, C, N, bf16):
    return C % (16 if bf16 else 8) == 0 and N % 64 == 0 and OH >= 16 and OW >= 16


def wino44_ok(OH, OW, C, N, wino4, bf16, amask, rowscale):
    return wino4 and not bf16 and C % 8 == 0 and N % 64 == 0 and OH >= 16 and OW >= 32 and not amask and not rowscale


def launch_s1(B, OH, OW, C, N, case, amask, rowscale, gate, gbits, pool, acc):
    """(record, splits) of launch_wino_s1: F(4x4,3x3) where the call asks for it and the launch allows, else F(2x2,3x3)."""
    bf16, queued = case.prec == "bf16", case.ctx == "steal"
    assert wino_geom_ok(OH, OW, C, N, bf16), "not a stride-1 3x3 Winograd launch"
    if wino44_ok(OH, OW, C, N, "wino4" in case.mods, bf16, amask, rowscale):
        return (0, 4044, R44_GBITS if gbits else R44_GATE if gate else R44_PLAIN), 1
    pl = wino_plan(B, OH, OW, C, N, bf16, amask, gate, gbits, pool, acc, case.envname)
    if bf16:
        return (3, 4016, 1 + pl["ki"]), pl["splits"]
    return (0, 4064, 1 + pl["ki"] + (R_QUEUED if queued else 0)), pl["splits"]


def launch_w22(g, dgrad, case, amask, gate):
    B, H, W, Cin, Cout, k, s, pad = g
    Ho, Wo = H // 2, W // 2
    C, N, ncls = (Cout, Cin, 4) if dgrad else (4 * Cin, Cout, 1)
    M = B * Ho * Wo
    total = cdiv(Wo, 16) * cdiv(Ho, 16) * B * (N // 64) * ncls
    nchunks, splits = C // 8, 1
    if nchunks >= 16:
        smax = min(nchunks // 8, 16)
        while smax > 1 and smax * M * N * ncls > splitk_room(M * N * ncls):
            smax -= 1
        splits = choose_splits(total, smax, PLAN_CUS)
    splits = cdiv(nchunks, cdiv(nchunks, splits))
    fast = case.envname != "TG_WINO_NO_FAST" and not amask
    ki = (W22_QUEUED if case.ctx == "steal" else 0) + (W22_FAST if fast else 0) + (1 if gate and splits == 1 else 0)
    return (0, 4022, 1 + ki), splits


def wgrad_plan(B, Ho, Wo, Cin, Cout, strip_w=16, min_strips=8, ctiles=1):
    nstrips = B * cdiv(Ho, 2) * cdiv(Wo, strip_w)
    tiles = (Cout // 64) * (Cin // 64) * ctiles
    sp = choose_splits_k(tiles, max(min(nstrips // min_strips, 512), 1), PLAN_CUS, nstrips, 0.03)
    return cdiv(nstrips, cdiv(nstrips, sp))


def wino_wgrad_ok(g, bf16):
    B, H, W, Cin, Cout, k, s, pad = g
    Ho, Wo = CO.out_size(H, k, s, pad), CO.out_size(W, k, s, pad)
    return not (bf16 and Cin > 256) and (k, s) == (3, 1) and Cin % 64 == 0 and Cout % 64 == 0 and Ho >= 16 and Wo >= 16


def wino16_wgrad_ok(g, bf16):
    B, H, W, Cin, Cout, k, s, pad = g
    Ho, Wo = CO.out_size(H, k, s, pad), CO.out_size(W, k, s, pad)
    return bf16 and (k, s) == (3, 1) and Cin % 64 == 0 and Cout % 64 == 0 and Ho >= 16 and Wo >= 32


def wino22_wgrad_ok(g, bf16):
    B, H, W, Cin, Cout, k, s, pad = g
    return not bf16 and CC.wino22_ok(g, 64, 64) and Cin % 64 == 0 and Cout % 64 == 0


def s2d_geom(g):
    B, H, W, Cin, Cout, k, s, pad = g
    return (B, H // 2, W // 2, 4 * Cin, Cout, 3, 1, 1)


def predict(case):
    """[(kind, cfg, route), ...] in launch order and the recorded split counts, of a case that runs on a Winograd kernel."""
    g, op, mods = case.geom, case.op, case.mods
    bf16 = case.prec == "bf16"
    masked, gate, gbits, acc, pool = (m in mods for m in ("mask", "gate", "gbits", "acc", "pool"))
    rep = 2 if "twice" in mods else 1
    if op == "wgrad":
        assert not masked, "a masked weight gradient runs on wgrad_kernel"
        g2 = s2d_geom(g) if s2d_ok(g) else g
        B, H, W, Cin, Cout, k, s, pad = g2
        Ho, Wo = CO.out_size(H, k, s, pad), CO.out_size(W, k, s, pad)
        if wino16_wgrad_ok(g2, bf16):
            r, sp = (3, 4116, 1), wgrad_plan(B, Ho, Wo, Cin, Cout, 32, 4)
        elif wino_wgrad_ok(g2, bf16):
            r, sp = (1, 4164, 1), wgrad_plan(B, Ho, Wo, Cin, Cout)
        else:
            assert wino22_wgrad_ok(g, bf16), "not a Winograd weight gradient"
            r, sp = (1, 4122, 1), wgrad_plan(B, Ho, Wo, Cin, Cout, ctiles=4)
        return [r] * rep, [sp] * rep
    dgrad = op == "dgrad"
    if s2d_ok(g) and not (dgrad and (gate or gbits)):
        B, H, W, Cin, Cout, k, s, pad = s2d_geom(g)         # the mask rides in the space-to-depth / depth-to-space pass
        r, sp = launch_s1(B, H, W, Cout, Cin, case, False, False, False, False, False, False) if dgrad else \
            launch_s1(B, H, W, Cin, Cout, case, False, False, False, False, False, False)
        return [r], [sp]
    B, H, W, Cin, Cout, k, s, pad = g
    if not bf16 and (CC.wino22_ok(g, Cout, Cin) if dgrad else CC.wino22_ok(g, Cin, Cout)):
        r, sp = launch_w22(g, dgrad, case, masked and not dgrad, gate)
        return [r], [sp]
    assert (k, s) == (3, 1), "not a Winograd launch"
    if dgrad:           # the mask of a dgrad is the epilogue's row scale, not a source mask
        r, sp = launch_s1(B, H, W, Cout, Cin, case, False, masked, gate, gbits, False, acc)
    else:
        Ho, Wo = CO.out_size(H, k, s, pad), CO.out_size(W, k, s, pad)
        r, sp = launch_s1(B, Ho, Wo, Cin, Cout, case, masked, masked, False, False, pool, False)
    return [r], [sp]


def algorithm(case):
    """The matrices the case's route uses (conv_oracle.WINO)."""
    if case.expect[0][1] == 4044:
        return "F43"
    return "F22" if case.expect[0][1] in (4022, 4122) else "F23"


def slab_cap(case, pred):
    return CO.WINO_SLABS_WGRAD if case.op == "wgrad" else CO.WINO_SLABS_CONV


def splits_ok(expected, recorded):
    return list(recorded) == ([expected] * len(recorded) if isinstance(expected, int) else list(expected))


# ---- the table ------------------------------------------------------------------------------------------------------------------------
class Case(CC.Case):
    """prec: 'f32' | 'bf16' (tg_hip.ops.set_precision for the launch);  runs: the references the case faces;  ctx: 'reserve' =
    tg_set_cu_reserve(128), 'steal' = tg_set_work_stealing(2) around the launch;  env: 'NAME' or 'NAME=value', a switch the library
    reads once per process;  grid: (sigma, largest magnitude) of the rounded run's integers, where GRID is too narrow for the case."""

    def __init__(self, id, geom, op, mods, expect, splits=1, env=None, prec="f32", runs=None, ctx=None, grid=None):
        CC.Case.__init__(self, id, geom, op, mods, expect, splits, env)
        self.grid = grid or GRID
        if "twice" in self.mods:
            self.expect = self.expect * 2
        self.prec, self.ctx = prec, ctx
        self.envname = env.split("=")[0] if env else None
        self.alg = algorithm(self)
        # F(4x4,3x3) rounds its coefficients (1/6, 1/24): no exact run.  bf16 operands: no usable a-priori bound against the
        # unrounded convolution (2^-8 S_w is a third of the result's rms); a case on a bf16 Winograd kernel (Case.rounds) faces the
        # reference that rounds the transformed operands as the kernel does instead, on data for which that rounding is determined.
        self.runs = runs or (("real",) if self.alg == "F43" else ("exact", "rounded") if self.rounds else
                             ("exact",) if prec == "bf16" else ("exact", "real"))

    @property
    def rounds(self):
        """The case runs on a kernel of wino16.inc: V / U (wgrad: A dY At / Bt X B) are rounded to bf16."""
        return self.prec == "bf16" and all(r[:2] in ((3, 4016), (3, 4116)) for r in self.expect)


CASES = []
# The rounded run's integers: clip(rint(sigma N(0,1)), +-max).  GRID_WIDE: where structural zeros (the taps a 5x5 filter lacks of the
# 6x6 it is regrouped into; the padding tiles of a ragged strip) thin out the share of operand elements that bf16 rounding changes.
GRID, GRID_WIDE = (400.0, 2047.0), (800.0, 4095.0)


def case(*a, **k):
    CASES.append(Case(*a, **k))


def W(route):
    return (0, 4064, route)


def W16(route):
    return (3, 4016, route)


def W22(route):
    return (0, 4022, route)


def W44(route):
    return (0, 4044, route)


WG, WG16, WG22 = (1, 4164, 1), (3, 4116, 1), (1, 4122, 1)
Q = R_QUEUED

# modifiers as in conv_cases, and: pool (forward: the fused 2x2 max-pool, tg_conv_fwd_pool), gbits (dgrad: ReLU gate of one bit per
# element, relu_gate_pack), wino4 (the call asks for F(4x4,3x3)), twice (the launch is repeated: bit-equal results)
# ---- wino_kernel, static walk: source mask = no buffer descriptors (non-fast); fast with ONE K step of 8 channels ----------------------
case("wk_masked_fwd", (1, 16, 16, 8, 64, 3, 1, 1), "fwd", "mask bias leaky", W(R_PLAIN))
case("wk_masked_fwd_ragged_2n", (2, 17, 19, 24, 128, 3, 1, 1), "fwd", "mask bias relu", W(R_PLAIN))
case("wk_fast_1k", (1, 16, 16, 8, 64, 3, 1, 1), "fwd", "bias relu", W(R_FAST))
case("wk_fast_ragged", (2, 17, 19, 8, 64, 3, 1, 1), "fwd", "bias leaky", W(R_FAST))
case("wk_fast_2p5_x_1p5_tiles", (1, 40, 24, 8, 64, 3, 1, 1), "fwd", "", W(R_FAST))
case("wk_fast_pad0", (1, 19, 21, 8, 64, 3, 1, 0), "fwd", "bias leaky", W(R_FAST))
case("wk_fast_pad2", (1, 15, 17, 8, 64, 3, 1, 2), "fwd", "bias", W(R_FAST))
case("wk_fast_2n", (1, 17, 19, 8, 128, 3, 1, 1), "fwd", "bias leaky", W(R_FAST))
case("wk_fast_gate_dgrad", (2, 17, 19, 64, 8, 3, 1, 1), "dgrad", "mask gate", W(R_FAST_GATE))
case("wk_fast_acc_dgrad", (1, 17, 19, 64, 8, 3, 1, 1), "dgrad", "mask acc", W(R_FAST))
case("wk_fast_dgrad_pad0", (1, 19, 21, 64, 8, 3, 1, 0), "dgrad", "gate", W(R_FAST_GATE))
# ---- wino_pipe_kernel: two K steps and more -------------------------------------------------------------------------------------------
case("wp_2k_one_item", (1, 16, 16, 16, 64, 3, 1, 1), "fwd", "bias leaky", W(R_PIPE))
case("wp_3k_ragged_2n", (2, 17, 19, 24, 128, 3, 1, 1), "fwd", "bias relu", W(R_PIPE))
case("wp_gate_dgrad", (2, 17, 19, 64, 16, 3, 1, 1), "dgrad", "mask gate", W(R_PIPE_GATE))
case("wp_acc_dgrad", (1, 17, 19, 64, 24, 3, 1, 1), "dgrad", "acc", W(R_PIPE))
case("wp_132_items_on_128", (1, 176, 192, 16, 64, 3, 1, 1), "fwd", "bias leaky", W(R_PIPE), ctx="reserve")
case("wp_gate_132_items_on_128", (1, 176, 192, 64, 16, 3, 1, 1), "dgrad", "gate", W(R_PIPE_GATE), ctx="reserve")
case("wp_270_items", (3, 144, 160, 16, 64, 3, 1, 1), "fwd", "bias", W(R_PIPE))
case("wp_pool", (1, 16, 32, 16, 64, 3, 1, 1), "fwd", "bias relu pool", W(R_POOL))
case("wp_pool_half_tile", (2, 24, 40, 16, 64, 3, 1, 1), "fwd", "bias relu pool", W(R_POOL))
case("wp_gbits", (2, 17, 19, 64, 16, 3, 1, 1), "dgrad", "gbits", W(R_GBITS))
case("wp_gbits_132_items_on_128", (1, 176, 192, 64, 16, 3, 1, 1), "dgrad", "gbits", W(R_GBITS), ctx="reserve")
# ---- split-K: slabs + igemm_splitk_epilogue --------------------------------------------------------------------------------------------
case("wk_split2_masked", (1, 16, 16, 128, 64, 3, 1, 1), "fwd", "mask bias leaky", W(R_PLAIN), 2)
case("wp_split2", (1, 17, 19, 128, 64, 3, 1, 1), "fwd", "bias relu", W(R_PIPE), 2)
case("wp_split2_uneven_17", (1, 16, 16, 136, 64, 3, 1, 1), "fwd", "bias leaky", W(R_PIPE), 2)
# 73 chunks in 9 splits of 9: the last split holds ONE chunk, which the pipeline cannot run -- wino_kernel fast at nine K steps
case("wk_fast_split9_last_single", (1, 16, 16, 584, 64, 3, 1, 1), "fwd", "bias leaky", W(R_FAST), 9)
case("wp_split16_cap", (1, 16, 16, 1024, 64, 3, 1, 1), "fwd", "bias", W(R_PIPE), 16)
case("wp_split2_gate_in_epilogue", (1, 17, 19, 64, 128, 3, 1, 1), "dgrad", "mask gate", W(R_PIPE), 2)
case("wp_split2_acc", (1, 16, 16, 64, 128, 3, 1, 1), "dgrad", "acc", W(R_PIPE), 2)
# ---- the same kernels pulling their items from the work-stealing queues ----------------------------------------------------------------
case("q_wk_masked", (2, 17, 19, 8, 64, 3, 1, 1), "fwd", "mask bias leaky", W(Q + R_PLAIN), ctx="steal")
case("q_wk_fast", (2, 17, 19, 8, 64, 3, 1, 1), "fwd", "bias", W(Q + R_FAST), ctx="steal")
case("q_wk_fast_gate", (2, 17, 19, 64, 8, 3, 1, 1), "dgrad", "mask gate", W(Q + R_FAST_GATE), ctx="steal")
case("q_wp_270_items", (3, 144, 160, 16, 64, 3, 1, 1), "fwd", "bias leaky", W(Q + R_PIPE), ctx="steal")
case("q_wp_gate", (2, 17, 19, 64, 16, 3, 1, 1), "dgrad", "gate", W(Q + R_PIPE_GATE), ctx="steal")
case("q_wp_pool", (2, 24, 40, 16, 64, 3, 1, 1), "fwd", "bias relu pool", W(Q + R_POOL), ctx="steal")
case("q_wp_gbits", (2, 17, 19, 64, 16, 3, 1, 1), "dgrad", "gbits", W(Q + R_GBITS), ctx="steal")
case("q_wp_split2", (1, 17, 19, 128, 64, 3, 1, 1), "fwd", "bias", W(Q + R_PIPE), 2, ctx="steal")
# ---- 5x5 stride 2 as 3x3 over the space-to-depth input ---------------------------------------------------------------------------------
case("s2d_fwd", (1, 64, 64, 16, 64, 5, 2, 2), "fwd", "mask bias leaky", W(R_PIPE))
case("s2d_dgrad", (1, 64, 64, 16, 64, 5, 2, 2), "dgrad", "mask acc", W(R_PIPE))
case("s2d_wgrad", (1, 64, 64, 16, 64, 5, 2, 2), "wgrad", "bias", WG, 4)
# ---- bf16 operands (wino16_kernel / wino16_pipe_kernel: K steps of 16 channels), exact and rounded run -----------------------------------
case("w16_masked", (2, 17, 19, 16, 64, 3, 1, 1), "fwd", "mask bias relu", W16(R_PLAIN), prec="bf16")
case("w16_fast_1k", (2, 17, 19, 16, 128, 3, 1, 1), "fwd", "bias relu", W16(R_FAST), prec="bf16")
case("w16_fast_gate", (2, 17, 19, 64, 16, 3, 1, 1), "dgrad", "mask gate", W16(R_FAST_GATE), prec="bf16")
case("w16_pipe_2k", (2, 17, 19, 32, 64, 3, 1, 1), "fwd", "bias", W16(R_PIPE), prec="bf16")
case("w16_pipe_132_items_on_128", (1, 176, 192, 32, 64, 3, 1, 1), "fwd", "bias relu", W16(R_PIPE), prec="bf16", ctx="reserve")
case("w16_pipe_gate", (2, 17, 19, 64, 48, 3, 1, 1), "dgrad", "mask gate", W16(R_PIPE_GATE), prec="bf16")
case("w16_pipe_acc", (1, 17, 19, 64, 32, 3, 1, 0), "dgrad", "acc", W16(R_PIPE), prec="bf16")
case("w16_pool", (2, 24, 40, 32, 64, 3, 1, 1), "fwd", "bias relu pool", W16(R_POOL), prec="bf16")
case("w16_gbits", (2, 17, 19, 64, 32, 3, 1, 1), "dgrad", "gbits", W16(R_GBITS), prec="bf16")
case("w16_split2", (1, 17, 19, 256, 64, 3, 1, 1), "fwd", "bias relu", W16(R_PIPE), 2, prec="bf16")
case("w16_split2_masked", (1, 16, 16, 256, 64, 3, 1, 1), "fwd", "mask bias", W16(R_PLAIN), 2, prec="bf16")
case("w16_s2d_fwd", (1, 64, 64, 16, 64, 5, 2, 2), "fwd", "mask bias relu", W16(R_PIPE), prec="bf16", grid=GRID_WIDE)
case("w16_wgrad", (1, 16, 32, 64, 64, 3, 1, 1), "wgrad", "bias", WG16, 2, prec="bf16")
case("w16_wgrad_ragged_split", (2, 17, 35, 64, 128, 3, 1, 1), "wgrad", "twice", WG16, 9, prec="bf16", grid=GRID_WIDE)
case("w16_keeps_fp32_wgrad", (1, 16, 16, 64, 64, 3, 1, 1), "wgrad", "bias", WG, prec="bf16")
# wino16_wgrad_kernel without padding, above the 256 input channels where the fp32 kernel stops, and behind the space-to-depth
# regrouping; the bf16 dgrad behind it
case("w16_wgrad_pad0", (2, 20, 36, 64, 64, 3, 1, 0), "wgrad", "", WG16, 9, prec="bf16")
case("w16_wgrad_c320", (1, 16, 32, 320, 64, 3, 1, 1), "wgrad", "", WG16, 2, prec="bf16")
case("w16_s2d_wgrad", (1, 64, 64, 16, 64, 5, 2, 2), "wgrad", "bias", WG16, 4, prec="bf16")
case("w16_s2d_dgrad", (1, 64, 64, 16, 64, 5, 2, 2), "dgrad", "mask acc", W16(R_PIPE), prec="bf16", grid=GRID_WIDE)
# ---- wino22_kernel: 4x4 stride 2, forward over the shifted space-to-depth view, dgrad = four classes in one launch --------------------------
case("w22_masked_fwd", (1, 32, 32, 8, 64, 4, 2, 1), "fwd", "mask bias leaky", W22(1))
case("w22_fast_fwd", (2, 36, 44, 8, 128, 4, 2, 1), "fwd", "bias leaky", W22(1 + W22_FAST))
case("w22_dgrad", (1, 32, 32, 64, 8, 4, 2, 1), "dgrad", "mask", W22(1 + W22_FAST))
case("w22_dgrad_acc", (2, 36, 44, 64, 16, 4, 2, 1), "dgrad", "acc", W22(1 + W22_FAST))
case("w22_dgrad_gate", (2, 36, 44, 128, 8, 4, 2, 1), "dgrad", "mask gate", W22(2 + W22_FAST))
case("w22_fwd_split2", (1, 32, 32, 32, 64, 4, 2, 1), "fwd", "bias leaky", W22(1 + W22_FAST), 2)
case("w22_fwd_split2_masked", (1, 36, 44, 32, 64, 4, 2, 1), "fwd", "mask bias", W22(1), 2)
case("w22_dgrad_split2", (1, 36, 44, 64, 128, 4, 2, 1), "dgrad", "mask acc", W22(1 + W22_FAST), 2)
case("w22_dgrad_split2_gate", (1, 32, 32, 64, 128, 4, 2, 1), "dgrad", "gate", W22(1 + W22_FAST), 2)
case("q_w22_masked_fwd", (1, 36, 44, 8, 64, 4, 2, 1), "fwd", "mask bias leaky", W22(1 + W22_QUEUED), ctx="steal")
case("q_w22_fast_fwd", (1, 32, 32, 8, 64, 4, 2, 1), "fwd", "bias", W22(1 + W22_QUEUED + W22_FAST), ctx="steal")
case("q_w22_dgrad_gate", (2, 36, 44, 64, 8, 4, 2, 1), "dgrad", "gate", W22(2 + W22_QUEUED + W22_FAST), ctx="steal")
# ---- wino44_kernel (the call asks for F(4x4,3x3)): the a-priori-bound run, Cin <= 64 ------------------------------------------------------------
case("w44_one_block", (1, 16, 32, 8, 64, 3, 1, 1), "fwd", "bias relu wino4", W44(R44_PLAIN))
case("w44_ragged_2n", (2, 19, 37, 16, 128, 3, 1, 1), "fwd", "bias leaky wino4", W44(R44_PLAIN))
case("w44_pad0_c64", (1, 21, 39, 64, 64, 3, 1, 0), "fwd", "bias wino4", W44(R44_PLAIN))
case("w44_dgrad_acc", (1, 19, 37, 64, 8, 3, 1, 1), "dgrad", "acc wino4", W44(R44_PLAIN))
case("w44_dgrad_gate", (2, 19, 37, 64, 16, 3, 1, 1), "dgrad", "gate wino4", W44(R44_GATE))
case("w44_dgrad_gbits", (2, 19, 37, 64, 16, 3, 1, 1), "dgrad", "gbits wino4", W44(R44_GBITS))
case("w44_132_items_on_128", (1, 176, 192, 8, 128, 3, 1, 1), "fwd", "bias relu wino4", W44(R44_PLAIN), ctx="reserve")
case("w44_gate_132_items_on_128", (1, 176, 192, 128, 8, 3, 1, 1), "dgrad", "gate wino4", W44(R44_GATE), ctx="reserve")
# ---- weight gradients: wino_wgrad_kernel F(3x3,2x2), wino22_wgrad_kernel F(2x2,2x2); slabs reduced in fixed order ------------------------------
case("wg_one_split", (1, 16, 16, 64, 64, 3, 1, 1), "wgrad", "bias", WG)
case("wg_ragged_strips", (1, 17, 19, 64, 64, 3, 1, 1), "wgrad", "twice", WG, 2)
case("wg_8_splits", (2, 32, 32, 64, 64, 3, 1, 1), "wgrad", "bias twice", WG, 8)
case("wg_tiles_2x2_pad0", (1, 19, 21, 128, 128, 3, 1, 0), "wgrad", "bias", WG, 2)
case("wg_pad2", (1, 15, 17, 64, 128, 3, 1, 2), "wgrad", "", WG, 2)
case("wg22_one_split", (1, 32, 32, 64, 64, 4, 2, 1), "wgrad", "bias", WG22)
case("wg22_ragged_strips", (1, 36, 44, 64, 64, 4, 2, 1), "wgrad", "twice", WG22, 2)
case("wg22_8_splits_tiles_2x2", (2, 64, 64, 128, 128, 4, 2, 1), "wgrad", "bias twice", WG22, 8)
# ---- behind a switch that is read once per process: one fresh child process per switch -----------------------------------------------------------
case("nopipe_fast_4k", (2, 17, 19, 32, 64, 3, 1, 1), "fwd", "bias leaky", W(R_FAST), env="TG_WINO_NO_PIPE")
case("nopipe_fast_gate_8k", (2, 17, 19, 64, 64, 3, 1, 1), "dgrad", "mask gate", W(R_FAST_GATE), env="TG_WINO_NO_PIPE")
case("nopipe_fast_split2", (1, 17, 19, 128, 64, 3, 1, 1), "fwd", "bias", W(R_FAST), 2, env="TG_WINO_NO_PIPE")
case("nopipe_fast_132_items_on_128", (1, 176, 192, 16, 64, 3, 1, 1), "fwd", "bias", W(R_FAST), env="TG_WINO_NO_PIPE", ctx="reserve")
case("nopipe_q_fast", (2, 17, 19, 32, 64, 3, 1, 1), "fwd", "bias", W(Q + R_FAST), env="TG_WINO_NO_PIPE", ctx="steal")
case("nopipe_w16_fast_2k", (2, 17, 19, 32, 64, 3, 1, 1), "fwd", "bias relu", W16(R_FAST), env="TG_WINO_NO_PIPE", prec="bf16")
case("nopipe_w16_fast_gate", (2, 17, 19, 64, 48, 3, 1, 1), "dgrad", "gate", W16(R_FAST_GATE), env="TG_WINO_NO_PIPE", prec="bf16")
case("nofast_plain_3k", (2, 17, 19, 24, 64, 3, 1, 1), "fwd", "bias leaky", W(R_PLAIN), env="TG_WINO_NO_FAST")
case("nofast_gate_dgrad", (2, 17, 19, 64, 16, 3, 1, 1), "dgrad", "mask gate", W(R_GATE), env="TG_WINO_NO_FAST")
case("nofast_q_gate_dgrad", (2, 17, 19, 64, 16, 3, 1, 1), "dgrad", "gate", W(Q + R_GATE), env="TG_WINO_NO_FAST", ctx="steal")
case("nofast_w16_gate_dgrad", (2, 17, 19, 64, 32, 3, 1, 1), "dgrad", "mask gate", W16(R_GATE), env="TG_WINO_NO_FAST", prec="bf16")
case("nofast_w22_dgrad", (2, 36, 44, 64, 8, 4, 2, 1), "dgrad", "mask", W22(1), env="TG_WINO_NO_FAST")
case("nofast_w22_dgrad_gate", (2, 36, 44, 64, 8, 4, 2, 1), "dgrad", "gate", W22(2), env="TG_WINO_NO_FAST")
case("nofast_q_w22_dgrad_gate", (1, 32, 32, 64, 8, 4, 2, 1), "dgrad", "gate", W22(2 + W22_QUEUED), env="TG_WINO_NO_FAST", ctx="steal")
for _v in ("0", "1"):           # the contiguous (0) and the interleaved (1, the default below 6 MB of U) walk over the items
    case(f"interleave{_v}_wp_132_on_128", (1, 176, 192, 16, 64, 3, 1, 1), "fwd", "bias", W(R_PIPE), env=f"TG_WINO_INTERLEAVE={_v}",
         ctx="reserve")
    case(f"interleave{_v}_wk_masked", (2, 40, 24, 8, 128, 3, 1, 1), "fwd", "mask bias leaky", W(R_PLAIN), env=f"TG_WINO_INTERLEAVE={_v}")
    case(f"interleave{_v}_w22_dgrad", (2, 36, 44, 64, 8, 4, 2, 1), "dgrad", "gate", W22(2 + W22_FAST), env=f"TG_WINO_INTERLEAVE={_v}")
    case(f"interleave{_v}_w44", (2, 19, 37, 16, 128, 3, 1, 1), "fwd", "bias wino4", W44(R44_PLAIN), env=f"TG_WINO_INTERLEAVE={_v}")

ENVS = ("TG_WINO_NO_PIPE", "TG_WINO_NO_FAST", "TG_WINO_INTERLEAVE=0", "TG_WINO_INTERLEAVE=1")
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
HERE = [c for c in CASES if c.env is None]
assert {c.env for c in CASES if c.env} == set(ENVS)


# ---- inputs and references ---------------------------------------------------------------------------------------------------------------
def fwd_act(case, mode):
    return CC.fwd_act(case, mode)


def gate_act(case, mode):
    """(kind, slope) of a dgrad's gate: bit gates are ReLU gates; float gates are LeakyReLU's in the real run."""
    if "gbits" in case.mods or mode == "exact":
        return CO.ACT_RELU, 0.0
    return CO.ACT_LEAKY, CC.LEAKY_SLOPE


def grid_draw(rng, grid, *shape):
    """Integers clip(rint(sigma N(0,1)), +-max) as fp32 (GRID: eleven bits), so that the transformed operands (sums of up to four
    of them, quarters of sums of up to nine) are exact in fp32 and mostly NOT bf16 numbers."""
    sigma, top = grid
    return np.clip(np.rint(sigma * rng.standard_normal(size=shape)), -top, top).astype(np.float32)


def make_inputs(case, mode):
    """conv_cases.make_inputs, and the mode 'rounded' of the cases on a bf16 Winograd kernel: x, w and dy on the grid of
    grid_draw; mask, ratio, gate and activation as in the real run; bias and base as in the real run times the power of two
    nearest the rms of the result (sigma^2 sqrt(products per element))."""
    if mode == "rounded":
        B, H, W, Cin, Cout, k, s, pad = case.geom
        d = CC.make_inputs(case, "real")
        rng = np.random.default_rng(sum(case.geom) * 11 + len(case.id) + 2)
        for name in ("x", "w", "dy"):
            d[name] = grid_draw(rng, case.grid, *d[name].shape)
        mag = np.float32(2.0 ** round(math.log2(case.grid[0] ** 2 * math.sqrt(k * k * (Cout if case.op == "dgrad" else Cin)))))
        for name in ("bias", "base"):
            if d[name] is not None:
                d[name] = d[name] * mag
    else:
        d = CC.make_inputs(case, mode)
    if "gbits" in case.mods:
        B, H, W, Cin = case.geom[:4]
        rng = np.random.default_rng(len(case.id) + sum(case.geom))
        d["gate"] = rng.integers(-3, 4, size=(B, H, W, Cin)).astype(np.float32)
    return d


def needs_forward(case, mode):
    assert case.op == "fwd" or not ({"relu", "leaky"} & case.mods), "backward cases take their gate as a drawn tensor"
    return False


def reference(case, d, mode):
    """{'y' (, 'yp') | 'dx' | 'dw' (, 'db')} -> conv_oracle.WRes / Res.  'yp' = the 2x2 max-pool of y: judged against the pooled
    reference in the exact run, against the pool of the kernel's own y in the real and the rounded run (a maximum does not round).
    The rounded run: conv_oracle's evaluation with the transformed operands rounded to bf16."""
    B, H, W, Cin, Cout, k, s, pad = case.geom
    a, sl = fwd_act(case, mode)
    if mode == "rounded":
        assert case.rounds and case.alg == "F23", case.id
        if case.op == "fwd":
            return {"y": CO.wino_fwd_rounded(d["x"], d["w"], k, s, pad, case.alg, d["mask"], d["bias"], d["ratio"], a, sl)}
        if case.op == "dgrad":
            ga, gs = gate_act(case, mode)
            return {"dx": CO.wino_dgrad_rounded(d["dy"], d["w"], (B, H, W, Cin), k, s, pad, case.alg, d["mask"], d["gate"], ga, gs,
                                                d["base"])}
        rw, rb = CO.wino_wgrad_rounded(d["x"], d["dy"], k, s, pad, case.alg)
        return {"dw": rw, "db": rb} if "bias" in case.mods else {"dw": rw}
    if case.op == "fwd":
        return {"y": CO.wino_fwd(d["x"], d["w"], k, s, pad, case.alg, d["mask"], d["bias"], d["ratio"], a, sl)}
    if case.op == "dgrad":
        ga, gs = gate_act(case, mode)
        return {"dx": CO.wino_dgrad(d["dy"], d["w"], (B, H, W, Cin), k, s, pad, case.alg, d["mask"], d["gate"], ga, gs, d["base"])}
    rw, rb = CO.wino_wgrad(d["x"], d["dy"], k, s, pad, case.alg)
    return {"dw": rw, "db": rb} if "bias" in case.mods else {"dw": rw}


def pool2(y):
    B, H, W, C = y.shape
    return y.reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


def sensitivity(case, ref):
    """max over the outputs of max bound / rms(reference): the a-priori bound is worth asserting only far below the signal."""
    slabs = slab_cap(case, case.expect)
    return max(float(CO.bound(r, slabs).max()) / math.sqrt(float(np.mean(r.val ** 2))) for r in ref.values())


SENSITIVITY_CAP = 0.05
