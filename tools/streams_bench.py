#!/usr/bin/env python3
"""Stream-network, HAND and flood-comparison throughput (mvp_gan/src/flow_routing.py stream_network and hand,
mvp_gan/src/evaluate_raster.py flood_errors, csrc/drainage.hip) on the 8192^2 scenes of
tools/drainage_bench.py.  Prints one JSON line per scene and stream threshold: ms per stream_network call by device events (host
syncs included) and per part, each part between its own pair of events (the class pass, the link rounds with their count, the
order rounds with their count and the junctions they run over, the finish); ms per hand call (the whole chain from the heights:
depression fill, routing, the drainage mask, HAND) and per hand_from_routing call on the routed surface (the doubling to the
drainage, the finish, tg_hand); ms per flood_errors call with each part's share (two routings, two HANDs, the comparison); and ms
per watersheds call in the same run, for scale.  The truth of a scene with voids is the terrain before the voids were cut and the
fill is interpolate_voids'; for "basins" the truth is the terrain with the basins and the fill the terrain without them, compared
where they differ.

    python tools/streams_bench.py [--size 8192] [--scenes 0.3 0.02 tiles basins] [--reps 3] [--warmup 1] [--min-cells 1000 1]
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

NET_PARTS = ("class", "link_rounds", "order_rounds", "finish")
FLOOD_PARTS = ("routings", "hands", "compare")
STAGES = (0.5, 1.0, 2.0, 5.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--scenes", nargs="+", default=["0.3", "0.02", "tiles", "basins"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--min-cells", type=int, nargs="+", default=[1000, 1])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("streams_bench: needs an MI355X (no CPU timing)")
    from fill_depressions_bench import BASINS, basins
    from fill_voids_bench import scene
    from mvp_gan.src.evaluate_raster import flood_errors
    from mvp_gan.src.flow_routing import (basin_rounds, hand, hand_from_routing, order_rounds, route_known, stream_network, streams,
                                          watersheds)
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
        known = torch.ones(H, W, dtype=torch.uint8, device=dev)
        direction, acc, rinfo, w = route_known(pred, known, 1.0, return_surface=True)
        ms_ws, (_, _, winfo) = timed(lambda: watersheds(direction))
        for mc in a.min_cells:
            ms_net, (_, _, ninfo) = timed(lambda: stream_network(direction, acc, mc))
            # the parts of stream_network, one chain per repetition
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(NET_PARTS) + 1)]
            tot = dict.fromkeys(NET_PARTS, 0.0)
            for rep in range(a.warmup + a.reps):
                ws = O.flow_basin_ws(H, W, dev)
                torch.cuda.synchronize()
                ev[0].record()
                cls, node, _ = O.stream_class(direction, acc, mc, ws)
                ev[1].record()
                lr = basin_rounds(H, W, ws)
                top, _, _, _, _ = O.flow_basin_finish(H, W, lr, ws, 1.0)
                ev[2].record()
                orr, conv = order_rounds(direction, cls, top, node)
                ev[3].record()
                O.stream_order_finish(cls, top, node)
                ev[4].record()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    for i, s in enumerate(NET_PARTS):
                        tot[s] += ev[i].elapsed_time(ev[i + 1]) / a.reps
                del ws, cls, node, top
            smask = streams(acc, mc)
            ms_hfr, (_, _, hinfo) = timed(lambda: hand_from_routing(w, direction, smask, 1.0))
            ms_hand, (_, _, hi) = timed(lambda: hand(pred, min_cells=mc))
            assert hi["drained"] == hinfo["drained"] and hi["max_hand_m"] == hinfo["max_hand_m"]
            ms_fe, d = timed(lambda: flood_errors(truth, pred, holes, cellsize=1.0, stream_cells=mc, stages_m=STAGES))
            fev = [torch.cuda.Event(enable_timing=True) for _ in range(len(FLOOD_PARTS) + 1)]
            ftot = dict.fromkeys(FLOOD_PARTS, 0.0)
            for rep in range(a.warmup + a.reps):
                torch.cuda.synchronize()
                fev[0].record()
                routed = [route_known(s, known, 1.0, return_surface=True) for s in (truth, pred)]
                fev[1].record()
                hands = [hand_from_routing(r[3], r[0], streams(r[1], mc), 1.0)[0] for r in routed]
                fev[2].record()
                O.flood_compare(holes, hands[0], hands[1], STAGES)
                fev[3].record()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    for i, s in enumerate(FLOOD_PARTS):
                        ftot[s] += fev[i].elapsed_time(fev[i + 1]) / a.reps
                del routed, hands
            whole = sum(ftot.values())
            print(json.dumps({"what": "streams", "H": H, "W": W, "scene": name, "min_cells": mc,
                              "stream_network_ms_per_call": round(ms_net, 3), **{"ms_" + s: round(tot[s], 3) for s in NET_PARTS},
                              "link_rounds": ninfo["link_rounds"], "order_rounds": ninfo["order_rounds"],
                              "order_ms_per_round": round(tot["order_rounds"] / max(ninfo["order_rounds"], 1), 4),
                              "stream_cells": ninfo["stream_cells"], "junctions": ninfo["junctions"], "links": ninfo["links"],
                              "max_order": ninfo["max_order"], "longest_link_m": ninfo["longest_link_m"],
                              "hand_ms_per_call": round(ms_hand, 3), "hand_from_routing_ms_per_call": round(ms_hfr, 3),
                              "hand_rounds": hinfo["rounds"], "drained": hinfo["drained"], "undrained": hinfo["undrained"],
                              "max_hand_m": hinfo["max_hand_m"],
                              "flood_errors_ms_per_call": round(ms_fe, 3), **{"flood_ms_" + s: round(ftot[s], 3) for s in FLOOD_PARTS},
                              **{"flood_share_" + s: round(ftot[s] / whole, 3) for s in FLOOD_PARTS},
                              "flood_cells": d["cells"], "hand_mae_m": d["hand"]["mae_m"],
                              "csi": [s["csi"] for s in d["stages"]],
                              "watersheds_ms_per_call": round(ms_ws, 3), "watersheds_rounds": winfo["rounds"],
                              "reps": a.reps, "warmup": a.warmup}), flush=True)


if __name__ == "__main__":
    main()
