#!/usr/bin/env python3
"""Backward time of the VGG trunk (input gradient of the prediction half), dense against sparse (vgg_backward(sparse=True)), on
the bench's masks (pred = target outside the holes) and on the worst case ("all holes": every pixel needed, every tile listed --
what the sparse launches cost when they skip nothing), fp32 activations and --checkpoint style bit gates.  Also checks that the
sparse result equals the dense one bit for bit on the needed pixels and is 0.0 elsewhere.  DESIGN §8k.

    python tools/vgg_sparse_bwd_timing.py [--size 256] [--batch 16] [--iters 30]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "terra-gan_amd")):
    sys.path.insert(0, _p)
os.environ.setdefault("TERRAGAN_ALLOW_STANDIN_VGG", "1")

import torch  # noqa: E402

from vgg_sparse_timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    from mvp_gan.src.utils.losses import InpaintingLoss
    from tg_hip import engine as E
    from tg_hip import ops as O
    from tg_hip.synth import synth_batch
    dev = torch.device("cuda:0")
    crit = InpaintingLoss(0.1, 0.1, device=torch.device("cpu")).to(dev)
    V = crit._vgg_tensors()
    B = a.batch
    real, mask = synth_batch(B, a.size, 1000)
    real, mask = real.to(dev)[:, 0].contiguous(), mask.to(dev)[:, 0].contiguous()
    tgt = real * mask
    noise = torch.rand(B, a.size, a.size, generator=torch.Generator().manual_seed(1)).to(dev)
    cases = {"bench masks": (torch.where(mask > 0, tgt, noise), mask), "all holes": (noise + 1.0, torch.zeros_like(mask))}
    E.VGG_SPARSE = E.VGG_SPARSE_BWD = True
    for name, (pred, m) in cases.items():
        both = torch.cat([pred, tgt]).contiguous()
        needed = (pred.view(torch.int32) != tgt.view(torch.int32)) | (m != 1)
        for keep in (True, "gates"):
            feats, ctx = E.vgg_forward(V, both, keep=keep, nb=B, bwd_mask=m)
            _v, dfeat = O.l1_mean(feats[:B], feats[B:], 1.0, want_grad=True, relu_gate=True)
            # dense twice, around the sparse run: the spread of the dense figure is what "costs nothing at full coverage" is held to
            res = [timed(lambda sp=sp: E.vgg_backward(ctx, dfeat, nb=B, gated=True, sparse=sp), a.iters) for sp in (False, True, False)]
            d0 = E.vgg_backward(ctx, dfeat, nb=B, gated=True, sparse=False).clone()
            d1 = E.vgg_backward(ctx, dfeat, nb=B, gated=True, sparse=True)
            torch.cuda.synchronize()
            assert torch.equal(d0[needed], d1[needed]) and bool((d1[~needed] == 0).all()), (name, keep)
            print(f"{name:12s} keep={str(keep):5s}: needed pixels {needed.float().mean().item():.3f}, trunk backward dense "
                  f"{res[0]:.3f} / {res[2]:.3f} ms, sparse {res[1]:.3f} ms ({min(res[0], res[2]) - res[1]:+.3f} ms), "
                  f"equal on needed / 0 elsewhere")


if __name__ == "__main__":
    main()
