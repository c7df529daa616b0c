#!/usr/bin/env python3
"""Randomised check of the DIRECT convolution kernels (implicit-GEMM forward / dgrad incl. the merged parity classes of strided
dgrads, the weight-gradient kernel, the 1-channel-side kernels) against the fp64 oracle of tests/conv_oracle.py: random kernel
sizes / strides / channel counts / ragged spatial sizes, with the partial-conv mask and ratio.  Run with TG_NO_WINO=1
TG_NO_WINO22=1 TG_NO_S2D=1 to send the stride-1 3x3 / 4x4 stride-2 / 5x5 stride-2 layers through them too (the a-priori bound
below does not hold for a Winograd transform: without the switches those ops are skipped).  Every result is judged per
element by the oracle's a-priori bound n 2^-24 S |scale|; --exact draws small integers instead (0/1 mask, no ratio, ReLU) and
asks for bit equality.  Prints the worst error / bound with the launch records (kind, cfg, route) of the op that produced it;
exits non-zero above 1.
    python tools/direct_fuzz.py [--cases 80] [--seed 0] [--exact]"""
import argparse
import csv
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "terra-gan_amd")]
import numpy as np
import torch
from tests import conv_oracle as CO
from tg_hip import lib as L
from tg_hip import ops as O

SLOPE = float(np.float32(0.2))
SLABS = 1024              # at least the partial sums of any direct route (tests/conv_cases.py: slab_cap)


class Routes:
    def __init__(self, path):
        self.lib, self.path, self.rows = L.load(), path, []

    def __enter__(self):
        for kind in (0, 1, 2, 3):
            self.lib.tg_prof_summary(kind, None, None, None, None)
        self.lib.tg_prof_enable(1)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.lib.tg_prof_enable(0)
        self.lib.tg_prof_dump(self.path.encode())
        self.rows = [(int(r["kind"]), int(r["cfg"]), int(r["route"]), int(r["splits"])) for r in csv.DictReader(open(self.path))]
        for kind in (0, 1, 2, 3):
            self.lib.tg_prof_summary(kind, None, None, None, None)
        return False


def judge(got, ref, exact):
    """err / bound of one result (exact: 0 where every bit agrees, inf otherwise)."""
    got = got.detach().cpu().numpy()
    if exact:
        assert CO.exact_ok(ref)
        return 0.0 if np.array_equal(got.astype(np.float64), ref.val) else float("inf")
    return CO.worst(got, ref, SLABS)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=80)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--exact", action="store_true", help="small-integer data, bit equality with the fp64 reference")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    ri = lambda lo, hi: int(rng.integers(lo, hi + 1))
    if args.exact:
        draw = lambda *shape: rng.integers(-3, 4, size=shape).astype(np.float32)
    else:
        draw = lambda *shape: rng.standard_normal(size=shape, dtype=np.float32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    act, slope = (O.ACT_RELU, 0.0) if args.exact else (O.ACT_LEAKY, SLOPE)
    worst, worst_case = 0.0, None
    csv_path = os.path.join(tempfile.mkdtemp(), "launches.csv")
    for case in range(args.cases):
        k, s = [(3, 1), (3, 2), (4, 2), (5, 2), (1, 1), (7, 2)][ri(0, 5)]
        p = {3: 1, 4: 1, 5: 2, 1: 0, 7: 3}[k]
        kind = ri(0, 9)
        if kind == 0:
            Cin, Cout = 1, 64 * ri(1, 2)                # 1-channel source
        elif kind == 1:
            Cin, Cout = 64, 1                           # 1-channel destination
            if k not in (3, 4):
                k, s, p = 3, 1, 1
        else:
            Cin, Cout = 4 * ri(1, 96), 4 * ri(1, 96)
            if ri(0, 5) == 0:
                Cin = ri(1, 9)                          # scalar-gather path
        B = ri(1, 4)
        H, W = ri(max(k, 6), 40), ri(max(k, 6), 48)
        if Cout == 1:
            W = 4 * ((W + 3) // 4)
        Ho, Wo = CO.out_size(H, k, s, p), CO.out_size(W, k, s, p)
        x, w, b, gy = draw(B, H, W, Cin), draw(Cout, k, k, Cin), draw(Cout), draw(B, Ho, Wo, Cout)
        if not args.exact:
            w *= np.float32(1.0 / (k * Cin ** 0.5))
        m = (rng.random((B, H, W)) > 0.3).astype(np.float32)
        ratio = None
        if not args.exact:
            ssum = CO.conv_fwd(m[..., None], np.ones((1, k, k, 1)), k, s, p).val[..., 0]
            ratio = np.where(ssum > 0, (k * k) / np.maximum(ssum, 1.0), 0.0).astype(np.float32)
        xd, md, wd = to(x), to(m), to(w).permute(0, 3, 1, 2)
        rd = to(ratio) if ratio is not None else None
        res = {}
        with Routes(csv_path) as rt:
            y = O.conv_fwd(xd, wd, to(b), k, s, p, in_mask=md, ratio=rd, act=act, slope=slope)
        res["fwd"] = (judge(y, CO.conv_fwd(x, w, k, s, p, m, b, ratio, act, slope), args.exact), rt.rows)
        # the activation's gate is taken from the kernels' OWN forward output: an output within fp32 rounding of zero may have the
        # other sign in fp64, and one flipped gate moves every gradient by a whole term -- that is the activation's discontinuity,
        # not an error of the (linear) dgrad / wgrad kernels under test, which get this dz as their input
        dz = gy * np.where(y.cpu().numpy() > 0, np.float32(1.0), np.float32(slope))
        if ratio is not None:
            dz = dz * ratio[..., None]
        dz = dz.astype(np.float32)
        with Routes(csv_path) as rt:
            dx = O.conv_dgrad(to(dz), wd, (B, H, W, Cin), k, s, p, in_mask=md)
        res["dgrad"] = (judge(dx, CO.conv_dgrad(dz, w, (B, H, W, Cin), k, s, p, m), args.exact), rt.rows)
        with Routes(csv_path) as rt:
            dw, db = O.conv_wgrad(xd, to(dz), wd, k, s, p, in_mask=md)
        rw, rb = CO.conv_wgrad(x, dz, k, s, p, m)
        res["wgrad"] = (judge(dw.permute(0, 2, 3, 1), rw, args.exact), rt.rows)
        res["bias"] = (judge(db, rb, args.exact), rt.rows)
        # a launch with a tag from 4000 up is a Winograd kernel (tests/test_hip_wino.py): its transforms are outside the bound
        res = {n: v for n, v in res.items() if all(cfg < 4000 for _kind, cfg, _route, _splits in v[1])}
        if not res:
            continue
        name = max(res, key=lambda n: res[n][0])
        if res[name][0] > worst or worst_case is None:
            worst, worst_case = res[name][0], ((B, H, W, Cin, Cout, k, s, p), name, res[name][1], {n: v[0] for n, v in res.items()})
    what = "bit equality (0 = every bit agrees)" if args.exact else "error / a-priori bound"
    assert worst_case is not None, "every op of every case ran on a Winograd kernel"
    print(f"{args.cases} cases, worst {what} = {worst:.4f}  at {worst_case[0]} in {worst_case[1]}, "
          f"launches (kind, cfg, route, splits) {worst_case[2]}; all ops of that case: {worst_case[3]}")
    sys.exit(0 if worst <= 1.0 else 1)


if __name__ == "__main__":
    main()
