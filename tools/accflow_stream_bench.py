#!/usr/bin/env python3
"""AccFlow.forward against AccFlowStream at 480x1024.

1. 31 frames: forward() on all of them, and the stream at chunk 1, 2, 5 and 10 - ms per frame (wall clock over the whole
   sequence, one synchronisation at its end) and peak allocated memory above what the frames themselves take;
2. the stream alone at chunk 5 on 301 frames (the 31 synthetic frames played forth and back: timing and memory do not depend
   on the content).
One JSON line per configuration.  Every configuration runs once unmeasured first (weight packs, code objects, and the
allocator's pool: the measured run reuses its blocks, as a long video does from the second push on)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from accflow_amd.networks.AccFlow_ import AccFlow, AccFlowStream  # noqa: E402

H, W = 480, 1024


def ping_pong(frames, n):
    period = 2 * (len(frames) - 1)
    for t in range(n):
        k = t % period
        yield frames[k if k < len(frames) else period - k]


def measure(fn, n_frames, warm=True):
    """fn() consumes its frames and returns (number of flows, whether all were finite)."""
    if warm:
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    n_out, finite = fn()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    return {"frames": n_frames, "outputs": n_out, "finite": bool(finite), "ms_per_frame": round(ms / n_frames, 2),
            "peak_allocated_GB": round((torch.cuda.max_memory_allocated() - base) / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=31)
    ap.add_argument("--long", type=int, default=301, help="frames of the stream-only run (0: skip it)")
    ap.add_argument("--chunks", type=int, nargs="*", default=[1, 2, 5, 10])
    a = ap.parse_args()
    from accflow_amd.data.synthetic import make_sequence, make_state_dict, normalize
    from accflow_amd.networks import build_flow_estimator
    model = AccFlow(build_flow_estimator("acc|raft"))
    model.load_state_dict(make_state_dict(model), strict=True)
    model = model.cuda().eval()
    frames = [normalize(f).cuda() for f in make_sequence(7, a.frames, H, W)]

    def forward():
        outs = model(images=frames)
        return len(outs), all(bool(torch.isfinite(o).all()) for o in outs)

    def stream(source, chunk):
        def fn():
            n, finite = 0, torch.ones((), dtype=torch.bool, device="cuda")
            for _, flow in model.accumulate_video(source(), chunk=chunk):      # (each flow is dropped as a consumer would)
                n, finite = n + 1, finite & torch.isfinite(flow).all()
            return n, bool(finite)
        return fn

    size = "%dx%dx%d" % (a.frames, H, W)
    print(json.dumps({"size": size, "route": "forward()", **measure(forward, a.frames)}), flush=True)
    for chunk in a.chunks:
        print(json.dumps({"size": size, "route": "stream", "chunk": chunk,
                          **measure(stream(lambda: iter(frames), chunk), a.frames)}), flush=True)
    if a.long:
        print(json.dumps({"size": "%dx%dx%d" % (a.long, H, W), "route": "stream", "chunk": 5,
                          **measure(stream(lambda: ping_pong(frames, a.long), 5), a.long, warm=False)}), flush=True)


if __name__ == "__main__":
    main()
