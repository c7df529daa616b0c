#!/usr/bin/env python3
"""Forward time of the VGG trunk on a [pred; target] batch, dense (TG_VGG_SPARSE=0 behaviour) against sparse, on the bench's
masks (pred = target outside the holes) and on the worst case (every pixel differs: every tile active), plus the map launch
alone (tg_vgg_sparse_map).  Also checks that every sparse forward equals the dense one bit for bit.  DESIGN §8g.

    python tools/vgg_sparse_timing.py [--size 256] [--batch 16] [--iters 30]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "terra-gan_amd")):
    sys.path.insert(0, _p)
os.environ.setdefault("TERRAGAN_ALLOW_STANDIN_VGG", "1")

import torch  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    from mvp_gan.src.utils.losses import InpaintingLoss
    from tg_hip import engine as E
    from tg_hip import ops as O
    from tg_hip.engine import VGG_TRUNK
    from tg_hip.synth import synth_batch
    dev = torch.device("cuda:0")
    crit = InpaintingLoss(0.1, 0.1, device=torch.device("cpu")).to(dev)
    V = crit._vgg_tensors()
    B = a.batch
    real, mask = synth_batch(B, a.size, 1000)
    real, mask = real.to(dev)[:, 0], mask.to(dev)[:, 0]
    tgt = real * mask
    noise = torch.rand(B, a.size, a.size, generator=torch.Generator().manual_seed(1)).to(dev)
    cases = {"bench masks": torch.where(mask > 0, tgt, noise), "all holes": noise + 1.0}
    plan = "".join("M" if it == "M" else "C" for it in VGG_TRUNK)
    for name, pred in cases.items():
        both = torch.cat([pred, tgt]).contiguous()
        res = {}
        for sparse in (False, True):
            E.VGG_SPARSE = sparse
            res[sparse] = timed(lambda: E.vgg_forward(V, both, keep=False, nb=B), a.iters)
        E.VGG_SPARSE = False
        f0, _ = E.vgg_forward(V, both, keep=False, nb=B)
        E.VGG_SPARSE = True
        f1, _ = E.vgg_forward(V, both, keep=False, nb=B)
        torch.cuda.synchronize()
        assert torch.equal(f0, f1), name
        tmap = timed(lambda: O.vgg_sparse_map(both, B, plan), a.iters)
        print(f"{name:12s}: trunk forward dense {res[False]:.3f} ms, sparse {res[True]:.3f} ms "
              f"({res[False] - res[True]:+.3f} ms), map launch {tmap * 1e3:.1f} us, bitwise equal")


if __name__ == "__main__":
    main()
