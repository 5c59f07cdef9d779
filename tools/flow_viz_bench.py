#!/usr/bin/env python3
"""viz.flow_to_image (two HIP launches, csrc/flow_viz.hip) against the two routes it replaces:
  torch   the colour coding restated with torch operators on the device, same process;
  numpy   the colour coding restated with numpy on the host, including the device-to-host copy of the flow.

Smooth flows at 10 x 512 x 512 (CVO's batch) and 1 x 480 x 1024.  The device routes are timed with HIP events around one
call (3 warm-up calls, median of 20); the host route with the wall clock around copy + colouring (median of 5).  One JSON line
per shape."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from accflow_amd import viz  # noqa: E402


def wheel():
    rows = []
    for n, full, ramp, rising in ((15, 0, 1, 1), (6, 1, 0, 0), (4, 1, 2, 1), (11, 2, 1, 0), (13, 2, 0, 1), (6, 0, 2, 0)):
        for k in range(n):
            row = [0.0, 0.0, 0.0]
            row[full] = 255.0
            row[ramp] = float(255 * k // n if rising else 255 - 255 * k // n)
            rows.append(row)
    return rows


def torch_route(flow, table):
    """(B,2,H,W) -> (B,H,W,3) uint8 with torch operators, per-sample scale."""
    u, v = flow[:, 0], flow[:, 1]
    scale = torch.sqrt(u * u + v * v).flatten(1).amax(1).view(-1, 1, 1) + 1e-5
    u, v = u / scale, v / scale
    rad = torch.sqrt(u * u + v * v).unsqueeze(-1)
    fk = (torch.atan2(-v, -u) / math.pi + 1) / 2 * 54
    k0 = fk.floor().clamp_(0, 54).long()
    k1 = (k0 + 1) % 55
    f = (fk - k0).unsqueeze(-1)
    c0, c1 = table[k0], table[k1]
    col = c0 + f * (c1 - c0)
    col = torch.where(rad <= 1, 1 - rad * (1 - col), 0.75 * col)
    return (255 * col).floor().to(torch.uint8)


def numpy_route(flow_dev, table):
    """the same on the host, one image at a time as the reference does it; the copy is part of it."""
    out = []
    for f in flow_dev.cpu().numpy():
        u, v = f[0], f[1]
        scale = np.sqrt(u * u + v * v).max() + np.float32(1e-5)
        u, v = u / scale, v / scale
        rad = np.sqrt(u * u + v * v)[..., None]
        fk = (np.arctan2(-v, -u) / np.pi + 1) / 2 * 54
        k0 = np.minimum(np.floor(fk), 54).astype(np.int32)
        k1 = (k0 + 1) % 55
        fr = (fk - k0)[..., None]
        c0, c1 = table[k0], table[k1]
        col = c0 + fr * (c1 - c0)
        col = np.where(rad <= 1, 1 - rad * (1 - col), 0.75 * col)
        out.append(np.floor(255 * col).astype(np.uint8))
    return np.stack(out)


def event_us(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(1e3 * a.elapsed_time(b))
    return statistics.median(times)


def wall_us(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append(1e6 * (time.perf_counter() - t0))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, default="10x512x512,1x480x1024")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    t_dev = torch.tensor(wheel(), device="cuda") / 255
    t_host = np.array(wheel(), dtype=np.float32) / np.float32(255)
    for spec in a.shapes.split(","):
        B, H, W = (int(x) for x in spec.split("x"))
        g = torch.Generator().manual_seed(5)
        flow = F.interpolate(8 * torch.randn(B, 2, 3, 4, generator=g), size=(H, W), mode="bilinear", align_corners=True).cuda()
        hip, tor, host = viz.flow_to_image(flow), torch_route(flow, t_dev), numpy_route(flow, t_host)
        res = {"B": B, "H": H, "W": W,
               "hip_us": round(event_us(lambda: viz.flow_to_image(flow), a.warmup, a.reps), 1),
               "torch_us": round(event_us(lambda: torch_route(flow, t_dev), a.warmup, a.reps), 1),
               "numpy_with_copy_us": round(wall_us(lambda: numpy_route(flow, t_host), 5), 1),
               "components_differing_from_torch": int((hip != tor).sum()),
               "components_differing_from_numpy": int((hip.cpu().numpy() != host).sum()), "components": hip.numel()}
        res["torch_over_hip"] = round(res["torch_us"] / res["hip_us"], 2)
        res["numpy_over_hip"] = round(res["numpy_with_copy_us"] / res["hip_us"], 1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
