#!/usr/bin/env python3
"""Watershed and drainage-comparison throughput (mvp_gan/src/flow_routing.py watersheds, mvp_gan/src/evaluate_raster.py
drainage_errors, csrc/drainage.hip) on the 8192^2 scenes of tools/flow_routing_bench.py.  Prints one JSON
line per scene: ms per watersheds call by device events (host syncs included), its rounds, ms per round of tg_flow_basin alone
(all rounds enqueued at once, no read-back between them) and the GB/s that follow from the bytes a round moves (32 B per pixel
and 16 B more per pixel whose pointer is live, the live counts read from the workspace); in the same run tg_flow_accum's ms per
round on the same direction grid, for scale; and ms per drainage_errors call with each part's share (two routings, two
watersheds, two distance transforms, the comparison), each part between its own pair of events.  The truth of a scene with voids
is the terrain before the voids were cut and the fill is interpolate_voids'; for "basins" the truth is the terrain with the
basins and the fill the terrain without them, compared where they differ.

    python tools/drainage_bench.py [--size 8192] [--scenes 0.3 0.02 tiles basins] [--reps 3] [--warmup 1] [--stream-cells 1000]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "terra-gan_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

RECORD_BYTES = 16                                   # (next, last, nc, nd)
LIVE_WORD = 8                                       # int32 index of live[0] in the workspace's control block
PARTS = ("routings", "watersheds", "edts", "compare")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--scenes", nargs="+", default=["0.3", "0.02", "tiles", "basins"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--stream-cells", type=int, default=1000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("drainage_bench: needs an MI355X (no CPU timing)")
    from fill_depressions_bench import BASINS, basins
    from fill_voids_bench import scene
    from mvp_gan.src.evaluate_raster import drainage_errors
    from mvp_gan.src.flow_routing import flow_routing, route_known, streams, watersheds
    from mvp_gan.src.interpolate import interpolate_voids
    from tg_hip import ops as O
    H = W = a.size
    dev = torch.device("cuda:0")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(a.warmup):
            out = fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps, out

    for name in a.scenes:
        if name == "basins":
            z, keep = scene(H, W, "0.0")
            pred = torch.from_numpy(z).to(dev)
            truth = torch.from_numpy(basins(z, BASINS, 1)).to(dev)
            holes = (truth != pred).to(torch.uint8)
        else:
            z, keep = scene(H, W, name)
            truth = torch.from_numpy(z).to(dev)
            kt = torch.from_numpy(keep).to(dev)
            pred, finfo = interpolate_voids(truth, kt)
            assert finfo["unfilled"] == 0
            holes = (kt == 0).to(torch.uint8)
        direction, acc, rinfo = flow_routing(pred)
        ms_ws, (_, _, winfo) = timed(lambda: watersheds(direction))
        rounds = winfo["rounds"]
        # the rounds alone, enqueued at once; then the accumulation's rounds on the same grid
        ws = O.flow_basin_ws(H, W, dev)
        state = torch.empty(2, dtype=torch.int32, device=dev)
        ms_b = ms_a = 0.0
        for rep in range(a.warmup + a.reps):
            O.flow_basin_init(direction, None, ws)
            torch.cuda.synchronize()
            e0.record()
            O.flow_basin(H, W, 0, rounds, state, ws)
            e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                ms_b += e0.elapsed_time(e1) / a.reps
        live = ws[4 * LIVE_WORD:4 * (LIVE_WORD + rounds)].view(torch.int32).cpu().tolist()
        assert state.cpu().tolist() == [0, rounds]
        round_bytes = sum(2 * RECORD_BYTES * H * W + RECORD_BYTES * n for n in live)
        del ws
        fws = O.flow_ws(H, W, dev)
        for rep in range(a.warmup + a.reps):
            O.flow_accum_init(direction, fws)
            torch.cuda.synchronize()
            e0.record()
            O.flow_accum(H, W, 0, rinfo["acc_rounds"], state, fws)
            e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                ms_a += e0.elapsed_time(e1) / a.reps
        del fws
        ms_de, d = timed(lambda: drainage_errors(truth, pred, holes, cellsize=1.0, stream_cells=a.stream_cells))
        # the parts of drainage_errors, one chain per repetition
        known = torch.ones(H, W, dtype=torch.uint8, device=dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(PARTS) + 1)]
        tot = dict.fromkeys(PARTS, 0.0)
        for rep in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            ev[0].record()
            routed = [route_known(s, known, 1.0) for s in (truth, pred)]
            ev[1].record()
            basin = [watersheds(r[0])[0] for r in routed]
            ev[2].record()
            d2 = [O.edt(streams(r[1], a.stream_cells))[0] for r in routed]
            ev[3].record()
            O.flow_compare(holes, routed[0][0], routed[1][0], basin[0], basin[1], routed[0][1], routed[1][1], d2[0], d2[1],
                           a.stream_cells, 9)
            ev[4].record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                for i, s in enumerate(PARTS):
                    tot[s] += ev[i].elapsed_time(ev[i + 1]) / a.reps
            del routed, basin, d2
        whole = sum(tot.values())
        print(json.dumps({"what": "drainage", "H": H, "W": W, "scene": name, "watersheds_ms_per_call": round(ms_ws, 3),
                          "rounds": rounds, "basins": winfo["basins"], "longest_steps": winfo["longest_steps"],
                          "basin_rounds_ms": round(ms_b, 3), "basin_ms_per_round": round(ms_b / max(rounds, 1), 3),
                          "basin_round_bytes": round_bytes, "basin_GB_per_s": round(round_bytes / (ms_b * 1e6), 1),
                          "live_share_mean": round(sum(live) / (max(rounds, 1) * H * W), 4),
                          "accum_rounds": rinfo["acc_rounds"], "accum_ms_per_round": round(ms_a / max(rinfo["acc_rounds"], 1), 3),
                          "drainage_errors_ms_per_call": round(ms_de, 3), **{"ms_" + s: round(tot[s], 3) for s in PARTS},
                          **{"share_" + s: round(tot[s] / whole, 3) for s in PARTS},
                          "cells": d["cells"], "dir_equal": d["direction"]["equal"], "same_outlet": d["outlet"]["same"],
                          "precision": d["streams"]["precision"], "recall": d["streams"]["recall"],
                          "stream_cells": a.stream_cells, "reps": a.reps, "warmup": a.warmup}), flush=True)


if __name__ == "__main__":
    main()
