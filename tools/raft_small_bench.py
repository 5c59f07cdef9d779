#!/usr/bin/env python3
"""RAFT-small against full RAFT on AccFlow's estimator workload (DESIGN.md "RAFT-small").

1. estimate_pairs over the 11 pairs of a 7-frame 480x1024 sequence (AccFlow.pair_schedule), 12 iterations, default conv mode:
   RAFT(small_args()) and RAFT(default_args()) on the same box, one after the other, each after --warmup calls; wall clock
   around a synchronise, ms per sequence = the mean over --steps calls (the timing of tools/train_bench.py).
2. The per-kernel split of ONE RAFT-small refinement iteration at B = 11, 60x128 on one stream: HIP events around every timed
   launch (accflow_amd/profiler.py), mean over --reps iterations.  flow_from_coords (one small launch) carries no timer.

    python tools/raft_small_bench.py [--steps 10] [--warmup 3] [--out profiles/raft_small_bench.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def build(args):
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks.raft.raft import RAFT
    m = RAFT(args)
    m.load_state_dict(make_state_dict(m), strict=True)
    return m.cuda().eval()


def sequence_ms(model, frames, pairs, steps, warmup):
    for _ in range(warmup):
        model.estimate_pairs(frames, pairs, iters=12)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.estimate_pairs(frames, pairs, iters=12)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def iteration_split(model, frames, pairs, reps):
    """One refinement iteration of the small model on the workspace of all 11 pairs, one stream."""
    from accflow_amd import ops, profiler
    from accflow_amd.networks.raft.corr import CorrBlock
    feats = model.encode_pairs(frames, pairs)
    fmap1 = torch.cat([feats["fmap"][i] for i, _ in pairs], dim=0)
    fmap2 = torch.cat([feats["fmap"][j] for _, j in pairs], dim=0)
    cnet = torch.cat([feats["cnet"][i] for i, _ in pairs], dim=0)
    B, _, h, w = cnet.shape
    with ops.guard_scope(torch.zeros(1, dtype=torch.int32, device="cuda")):
        corr_fn = CorrBlock(fmap1, fmap2, radius=model.args.corr_radius)
        ws = model._workspace(B, h, w, cnet.device)
        model._prepack()
        model._prepare_context(ws, cnet)
        coords1 = ops.coords_grid(B, h, w, cnet.device)
        for _ in range(3):
            model._iteration(ws, corr_fn, coords1, last=False)
        out = torch.empty((B, 2, 8 * h, 8 * w), dtype=torch.float32, device="cuda")
        tm = profiler.KernelTimer(["conv2d", "corr_lookup", "upflow8"])
        profiler.ACTIVE = tm
        try:
            for _ in range(reps):
                model._iteration(ws, corr_fn, coords1, last=False)
            ops.flow_from_coords(coords1, dst0=ws.flow)
            ops.upflow8(ws.flow, out=out)
        finally:
            profiler.ACTIVE = None
        torch.cuda.synchronize()
    rows = []
    for name in ("corr_lookup", "conv2d", "upflow8"):
        per = reps if name != "upflow8" else 1
        for detail, d in tm.by_detail(name).items():
            rows.append({"op": name, "detail": detail, "launches_per_iteration": d["launches"] / per,
                         "us_per_iteration": round(1e3 * d["total_ms"] / per, 1)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from accflow_amd import ops
    from accflow_amd.data.synthetic import make_sequence, normalize
    from accflow_amd.networks.AccFlow_ import AccFlow
    from accflow_amd.networks.raft.raft import default_args, small_args
    assert torch.cuda.is_available(), "raft_small_bench needs the GPU"
    frames = [normalize(f).cuda() for f in make_sequence(1000, 7, 480, 1024)]
    pairs = AccFlow.pair_schedule(7)
    assert len(pairs) == 11
    res = {"workload": "estimate_pairs, 11 pairs of 7x480x1024, 12 iterations", "conv_mode": ops.conv_mode_name(),
           "steps": a.steps, "warmup": a.warmup}
    with torch.no_grad():
        small = build(small_args())
        res["raft_small_ms_per_sequence"] = round(sequence_ms(small, frames, pairs, a.steps, a.warmup), 2)
        full = build(default_args())
        res["raft_ms_per_sequence"] = round(sequence_ms(full, frames, pairs, a.steps, a.warmup), 2)
        del full
        # (once more, after the other model: the spread of the same measurement on this box)
        res["raft_small_ms_per_sequence_again"] = round(sequence_ms(small, frames, pairs, a.steps, 1), 2)
        res["guard_trips"] = ops.guard_report()
        res["small_iteration_split"] = iteration_split(small, frames, pairs, a.reps)
    res["small_iteration_us"] = round(sum(r["us_per_iteration"] for r in res["small_iteration_split"] if r["op"] != "upflow8"), 1)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
