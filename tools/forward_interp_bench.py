#!/usr/bin/env python3
"""forward_interpolate: the kernel against the host route it replaces (DESIGN.md "forward_interpolate and the video warm start").

1. Per shape (B, h, w), flows of sigma = 3 px: the kernel alone in HIP-event time (10 warm-up launches, median of 100), and
   the host route on the same box - `.cpu()`, two scipy nearest-neighbour interpolations per item (what
   griddata(method="nearest") does), `.cuda()` - wall clock around a synchronise (median of --host-reps); skipped with a note where scipy is not installed.
2. RAFT.estimate_video on 4 frames of 480x1024: ms per pair, cold at 12 iterations (one batched call) against warm-started
   at (12, 8) (--skip-video leaves it out).
One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from accflow_amd import ops  # noqa: E402

SHAPES = [(1, 60, 128), (11, 60, 128), (1, 90, 160), (6, 90, 160)]


def kernel_us(flow, warmup=10, reps=100):
    out = torch.empty_like(flow)
    for _ in range(warmup):
        ops.forward_interpolate(flow, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ops.forward_interpolate(flow, out=out)
        e.record()
        e.synchronize()
        times.append(1e3 * s.elapsed_time(e))
    return statistics.median(times)


def host_route(flow, nearest):
    """The route the kernel replaces, as a video loop pays for it: the flows copied to the host, per item two nearest-neighbour
    interpolators over the kept, moved cells (scipy's NearestNDInterpolator - what griddata(method="nearest") builds - one for
    each flow component, each with its own k-d tree), evaluated at every cell, and the result copied back."""
    moves = flow.detach().cpu().double().flatten(2).transpose(1, 2)              # (B, P, 2): (dx, dy) per cell, float64
    h, w = flow.shape[-2:]
    rows, cols = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    cells = torch.stack([cols, rows], dim=-1).reshape(-1, 2)                     # (P, 2): (x, y) of every cell
    frame = torch.tensor([w, h], dtype=torch.float64)
    filled = []
    for move in moves:
        landed = cells + move
        keep = ((landed > 0) & (landed < frame)).all(dim=1)                      # strictly inside the frame
        points, values = landed[keep].numpy(), move[keep].numpy()
        filled.append(np.stack([nearest(points, values[:, c])(cells.numpy()) for c in (0, 1)]).reshape(2, h, w))
    return torch.from_numpy(np.stack(filled)).float().cuda()


def host_ms(flow, nearest, reps):
    host_route(flow, nearest)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route(flow, nearest)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def video(iters_cold=12, iters_warm=(12, 8), reps=5):
    from accflow_amd.data.synthetic import make_sequence, make_state_dict, normalize
    from accflow_amd.networks import build_flow_estimator
    m = build_flow_estimator("raft")
    m.load_state_dict(make_state_dict(m), strict=True)
    m = m.cuda().eval()
    frames = [normalize(f).cuda() for f in make_sequence(7, 4, 480, 1024)]
    n_pairs = len(frames) - 1
    res = {"size": "4x480x1024", "model": "RAFT", "pairs": n_pairs}
    for key, kw in (("cold_%d_ms_per_pair" % iters_cold, dict(iters=iters_cold, warm_start=False)),
                    ("warm_%d_%d_ms_per_pair" % iters_warm, dict(iters=iters_warm, warm_start=True))):
        m.estimate_video(frames, **kw)
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.estimate_video(frames, **kw)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0) / n_pairs)
        res[key] = round(statistics.median(times), 3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--skip-video", action="store_true")
    a = ap.parse_args()
    try:
        from scipy.interpolate import NearestNDInterpolator as nearest
    except ImportError:
        nearest = None
    g = torch.Generator(device="cuda").manual_seed(0)
    for B, h, w in SHAPES:
        flow = 3.0 * torch.randn(B, 2, h, w, device="cuda", generator=g)
        res = {"B": B, "h": h, "w": w, "kernel_us": round(kernel_us(flow), 1)}
        if nearest is not None:
            res["host_route_ms"] = round(host_ms(flow, nearest, a.host_reps), 2)
            same = torch.equal(host_route(flow, nearest), ops.forward_interpolate(flow))
            res["equal_to_host_route"] = bool(same)      # (information: scipy's tree may break a near tie the other way)
        else:
            res["host_route_ms"] = None
            res["note"] = "scipy not installed: host route not measured"
        print(json.dumps(res), flush=True)
    if not a.skip_video:
        video()


if __name__ == "__main__":
    main()
