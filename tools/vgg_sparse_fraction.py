#!/usr/bin/env python3
"""Share of the prediction half's 16x16 output tiles of each VGG-trunk conv that can differ from the target half on the bench's
synthetic masks: a tile can differ iff a hole pixel (mask == 0) lies in its receptive field -- one 3x3 dilation per
conv, a 2x2 max per pool.  CPU only; the same recipe as tg_vgg_sparse_map, from the masks instead of the data.

    python tools/vgg_sparse_fraction.py [--size 256] [--batch 16] [--seeds 1000,1001,1002,1003]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "terra-gan_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tg_hip.engine import VGG_TRUNK  # noqa: E402
from tg_hip.synth import synth_batch  # noqa: E402


def fractions(mask):
    """mask [B][1][H][W] (1 = valid) -> {layer: share of its prediction tiles that can differ}"""
    d = (mask < 1).float()
    out = {}
    for item in VGG_TRUNK:
        if item == "M":
            d = F.max_pool2d(d, 2, 2)
            continue
        d = F.max_pool2d(d, 3, 1, 1)
        H, W = d.shape[2:]
        ty, tx = -(-H // 16), -(-W // 16)
        t = F.max_pool2d(F.pad(d, (0, 16 * tx - W, 0, 16 * ty - H)), 16, 16)
        out[f"vgg{item}"] = float(t.mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seeds", default="1000,1001,1002,1003")
    a = ap.parse_args()
    rows = []
    for s in (int(v) for v in a.seeds.split(",")):
        _real, mask = synth_batch(a.batch, a.size, s)
        fr = fractions(mask)
        rows.append(fr)
        print(f"seed {s}: " + "  ".join(f"{k} {v:.3f}" for k, v in fr.items()) + f"   hole share {float((mask < 1).float().mean()):.3f}")
    print("mean    : " + "  ".join(f"{k} {sum(r[k] for r in rows) / len(rows):.3f}" for k in rows[0]))


if __name__ == "__main__":
    main()
