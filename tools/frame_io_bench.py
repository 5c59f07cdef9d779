#!/usr/bin/env python3
"""The frame / flow-file boundary (csrc/frame_io.hip, one launch each) against the torch routes it replaces:
  ingest   FramePadder.ingest on packed uint8 frames against
           F.pad(2 * (u8.float() / 255) - 1 -> permute(0, 3, 1, 2).contiguous(), pad, mode="replicate")
           (six launches; without a pad F.pad is left out, as a caller would: five);
  export   FramePadder.export against permute(0, 2, 3, 1).contiguous() of the unpadded view ("f32") and against that plus
           the KITTI coding with torch operators on the device ("u16"); the coding with numpy on the host, including the
           device-to-host copy of the flow, is timed with the wall clock beside it.

One frame and seven frames at 480 x 1024 (no pad) and 436 x 1024 (sintel pad: 2 + 2 rows).  The device routes are timed with
HIP events around one call (3 warm-up calls, median of 20).  `bytes` is what the single launch has to move, read + written;
`hbm_fraction` that over the time over --hbm-gbs (default 8000: the MI355X's 8 TB/s).  One JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from accflow_amd.frames import FramePadder  # noqa: E402


def torch_ingest(u8, pad):
    x = 2 * (u8.float() / 255.0) - 1
    x = x.permute(0, 3, 1, 2).contiguous()
    return F.pad(x, pad, mode="replicate") if any(pad) else x


def torch_u16(flow_unpadded, scale):
    f = flow_unpadded.permute(0, 2, 3, 1).contiguous()
    fin = torch.isfinite(f)
    code = torch.where(fin, (scale * f + 32768.0).clamp(0, 65535).trunc(), torch.zeros_like(f)).to(torch.int32)
    return torch.cat([code, fin.all(dim=-1, keepdim=True).to(torch.int32)], dim=-1).to(torch.int16)     # (the bits of uint16)


def numpy_u16(flow_unpadded, scale):
    f = np.ascontiguousarray(flow_unpadded.cpu().numpy().transpose(0, 2, 3, 1))
    code = np.trunc(np.clip(np.float32(scale) * f + np.float32(32768), 0, 65535)).astype(np.uint16)
    return np.concatenate([code, np.ones(code.shape[:3] + (1,), np.uint16)], axis=-1)


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
    ap.add_argument("--shapes", type=str, default="1x480x1024,7x480x1024,1x436x1024,7x436x1024")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    a = ap.parse_args()

    def frac(nbytes, us):
        return round(nbytes / (us * 1e-6) / (a.hbm_gbs * 1e9), 4)

    for spec in a.shapes.split(","):
        N, H, W = (int(x) for x in spec.split("x"))
        g = torch.Generator().manual_seed(5)
        u8 = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).cuda()
        padder = FramePadder((H, W), "sintel")
        pad = tuple(padder._pad)
        Hp, Wp = H + pad[2] + pad[3], W + pad[0] + pad[1]
        x = padder.ingest(u8)
        assert torch.equal(x.cpu(), torch_ingest(u8.cpu(), pad)), "ingest differs from the torch route on the CPU"
        # (on the device torch divides by a scalar as a multiplication by its reciprocal: that route is not bit-equal to the CPU's)
        off = int((x != torch_ingest(u8, pad)).sum())
        nbytes = N * (3 * H * W + 12 * Hp * Wp)
        res = {"what": "ingest", "N": N, "H": H, "W": W, "pad": pad, "bytes": nbytes,
               "hip_us": round(event_us(lambda: padder.ingest(u8), a.warmup, a.reps), 1),
               "torch_us": round(event_us(lambda: torch_ingest(u8, pad), a.warmup, a.reps), 1),
               "elements_differing_from_torch_on_device": off, "elements": x.numel()}
        res["torch_over_hip"] = round(res["torch_us"] / res["hip_us"], 2)
        res["hbm_fraction"] = frac(nbytes, res["hip_us"])
        print(json.dumps(res), flush=True)

        flow = (40 * torch.randn(N, 2, Hp, Wp, generator=g)).cuda()
        un = padder.unpad(flow)
        assert torch.equal(padder.export(flow), un.permute(0, 2, 3, 1).contiguous())
        nbytes = N * 16 * H * W
        res = {"what": "export f32", "N": N, "H": H, "W": W, "bytes": nbytes,
               "hip_us": round(event_us(lambda: padder.export(flow), a.warmup, a.reps), 1),
               "torch_us": round(event_us(lambda: un.permute(0, 2, 3, 1).contiguous(), a.warmup, a.reps), 1)}
        res["torch_over_hip"] = round(res["torch_us"] / res["hip_us"], 2)
        res["hbm_fraction"] = frac(nbytes, res["hip_us"])
        print(json.dumps(res), flush=True)

        got = padder.export(flow, coding="u16").cpu().numpy()
        assert np.array_equal(got, numpy_u16(un, 64.0)), "export differs from numpy's float32 coding"
        off = int((got != torch_u16(un, 64.0).cpu().numpy().view(np.uint16)).sum())
        nbytes = N * 14 * H * W
        res = {"what": "export u16", "N": N, "H": H, "W": W, "bytes": nbytes,
               "hip_us": round(event_us(lambda: padder.export(flow, coding="u16"), a.warmup, a.reps), 1),
               "torch_us": round(event_us(lambda: torch_u16(un, 64.0), a.warmup, a.reps), 1),
               "numpy_with_copy_us": round(wall_us(lambda: numpy_u16(un, 64.0), 5), 1),
               "samples_differing_from_torch_on_device": off, "samples": int(got.size)}
        res["torch_over_hip"] = round(res["torch_us"] / res["hip_us"], 2)
        res["numpy_over_hip"] = round(res["numpy_with_copy_us"] / res["hip_us"], 1)
        res["hbm_fraction"] = frac(nbytes, res["hip_us"])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
