#!/usr/bin/env python3
"""Resampling inside the two boundary launches (csrc/frame_io.hip) against the torch chains it replaces:
  ingest   FrameScaler.ingest on packed uint8 frames, bilinear and area, against
           F.pad(2 * (F.interpolate(u8.permute(0, 3, 1, 2).float(), size, mode) / 255) - 1, pad, mode="replicate")
           (without a pad F.pad is left out, as a caller would);
  export   FrameScaler.export ("f32" and "u16") of the padded working-size flow against
           ops.flow_export(F.interpolate(unpad(flow), source size, bilinear) * (W / w, H / h), coding).

2160 x 3840 -> 540 x 960 and 872 x 2048 -> 436 x 1024 (padded to 544 x 960 and 440 x 1024), one frame and --batch frames.  Both
routes of a case run in one process, alternating: --rounds rounds of (--reps calls of one, --reps of the other), each call timed
with HIP events after 3 warm-up calls; the figure is the median over all of a route's calls, and `spread` the ratio of its
largest to its smallest per-round median.  `bytes` is what the single launch has to move - the source bytes it needs, read
once (area: the whole frame; bilinear: four taps per output pixel, so a quarter of the frame at a 4x reduction, although
whole cache lines come with them), plus the output written - and `hip_gbs` that over the time.  `max_abs_diff_to_torch` is measured on the timed tensors (torch's float coordinates: DESIGN.md 4.10).
One JSON line per case."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from accflow_amd import ops  # noqa: E402
from accflow_amd.frames import FrameScaler  # noqa: E402


def torch_ingest(u8, size, pad, mode):
    x = u8.permute(0, 3, 1, 2).float()
    x = F.interpolate(x, size=size, mode="bilinear", align_corners=False) if mode == "bilinear" else F.interpolate(x, size=size, mode="area")
    x = 2 * (x / 255.0) - 1
    return F.pad(x, pad, mode="replicate") if any(pad) else x


def torch_export(flow, scaler, coding):
    h, w = scaler.size
    up = F.interpolate(scaler.padder.unpad(flow), size=(scaler.ht, scaler.wd), mode="bilinear", align_corners=False)
    up = up * torch.tensor([scaler.wd / w, scaler.ht / h], device=flow.device).view(1, 2, 1, 1)
    return ops.flow_export(up, coding=coding)


def event_us(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(1e3 * a.elapsed_time(b))
    return times


def alternate(fns, warmup, reps, rounds):
    """{name: (median over all calls, largest / smallest per-round median)} of the routes in fns, run turn by turn."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    calls, per_round = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t = event_us(fn, reps)
            calls[k] += t
            per_round[k].append(statistics.median(t))
    return {k: (statistics.median(calls[k]), max(per_round[k]) / min(per_round[k])) for k in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, default="2160x3840:540x960,872x2048:436x1024", help="HxW:hxw,...")
    ap.add_argument("--batch", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_resize_bench: no GPU - nothing is measured without one")
    for spec in a.shapes.split(","):
        (H, W), (h, w) = (tuple(int(v) for v in part.split("x")) for part in spec.split(":"))
        for N in sorted({1, a.batch}):
            g = torch.Generator().manual_seed(5)
            u8 = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).cuda()
            for mode in ("bilinear", "area"):
                scaler = FrameScaler((H, W), size=(h, w), interp=mode)
                pad = tuple(scaler.padder._pad)
                x = scaler.ingest(u8)
                diff = float((x - torch_ingest(u8, (h, w), pad, mode)).abs().max())
                t = alternate({"hip": lambda: scaler.ingest(u8), "torch": lambda: torch_ingest(u8, (h, w), pad, mode)},
                              a.warmup, a.reps, a.rounds)
                src_bytes = 3 * H * W if mode == "area" else min(3 * H * W, 12 * h * w)      # (bilinear: four taps a pixel at most)
                res = {"what": "ingest " + mode, "N": N, "from": [H, W], "to": [h, w], "pad": pad,
                       "bytes": N * src_bytes + x.numel() * 4, "hip_us": round(t["hip"][0], 1), "torch_us": round(t["torch"][0], 1),
                       "torch_over_hip": round(t["torch"][0] / t["hip"][0], 2), "spread_hip": round(t["hip"][1], 3),
                       "spread_torch": round(t["torch"][1], 3), "max_abs_diff_to_torch": diff}
                res["hip_gbs"] = round(res["bytes"] / (t["hip"][0] * 1e-6) / 1e9, 1)
                print(json.dumps(res), flush=True)
            scaler = FrameScaler((H, W), size=(h, w))
            Hp, Wp = scaler.padder.ht + scaler.padder._pad[2] + scaler.padder._pad[3], scaler.padder.wd + scaler.padder._pad[0] + scaler.padder._pad[1]
            flow = (10 * torch.randn(N, 2, Hp, Wp, generator=g)).cuda()
            for coding in ("f32", "u16"):
                got, ref = scaler.export(flow, coding=coding), torch_export(flow, scaler, coding)
                diff = (float((got - ref).abs().max()) if coding == "f32"
                        else int(np.abs(got.cpu().numpy().astype(np.int64) - ref.cpu().numpy().astype(np.int64)).max()))
                t = alternate({"hip": lambda: scaler.export(flow, coding=coding), "torch": lambda: torch_export(flow, scaler, coding)},
                              a.warmup, a.reps, a.rounds)
                res = {"what": "export " + coding, "N": N, "from": [h, w], "to": [H, W],
                       "bytes": N * (8 * h * w + (8 if coding == "f32" else 6) * H * W), "hip_us": round(t["hip"][0], 1),
                       "torch_us": round(t["torch"][0], 1), "torch_over_hip": round(t["torch"][0] / t["hip"][0], 2),
                       "spread_hip": round(t["hip"][1], 3), "spread_torch": round(t["torch"][1], 3), "max_abs_diff_to_torch": diff}
                res["hip_gbs"] = round(res["bytes"] / (t["hip"][0] * 1e-6) / 1e9, 1)
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
