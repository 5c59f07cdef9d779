#!/usr/bin/env python3
"""metrics.cvo_metrics against the torch route it replaces, eval_cvo.calc_occ_mask + cal_epe.

Same process, smooth flow pairs at CVO's batch (10 x 512 x 512 by default): 3 warm-up calls, then the median wall time of
20 calls, one synchronisation before and one after each timed call.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from accflow_amd import eval_cvo, metrics, ops  # noqa: E402


def wall_us(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e6 * (time.perf_counter() - t0))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(10, 512, 512), metavar=("B", "H", "W"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    B, H, W = a.shape
    g = torch.Generator().manual_seed(5)

    def enlarge(t):
        return F.interpolate(t, size=(H, W), mode="bilinear", align_corners=True).cuda()
    fflow = enlarge(6 * torch.randn(B, 2, 3, 4, generator=g))
    bflow = -ops.backwarp(fflow, -fflow) + enlarge(0.3 * torch.randn(B, 2, 5, 7, generator=g))
    pred = bflow + enlarge(2.5 * torch.randn(B, 2, 6, 9, generator=g))

    def old():
        occ, _ = eval_cvo.calc_occ_mask(bflow, fflow)
        return eval_cvo.cal_epe(pred, bflow, occ)

    def new():
        m = metrics.cvo_metrics(pred, bflow, fflow)
        return m.epe, m.epe_occ, m.epe_vis
    o, n = old(), new()
    res = {"B": B, "H": H, "W": W, "occluded_share": round(float(ops.fb_occlusion(bflow, fflow, want=("bw",))[0].mean()), 3),
           "torch_route_us": round(wall_us(old, a.warmup, a.reps), 1), "cvo_metrics_us": round(wall_us(new, a.warmup, a.reps), 1),
           "max_abs_difference": [float((x.double() - y).abs().max()) for x, y in zip(o, n)]}
    res["ratio"] = round(res["torch_route_us"] / res["cvo_metrics_us"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
