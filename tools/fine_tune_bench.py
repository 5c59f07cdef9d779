"""Time of one fine-tuning step of RAFT's update block (accflow_amd/train_raft.py) on the reference's configuration
(configs/RAFT.yml: batch_per_gpu 6, 256 x 256 crops; 12 iterations, AdamW, clip 1.0), synthetic data, one GPU.  There is no earlier
path to compare with: the time is reported, not gated.

    python tools/fine_tune_bench.py [--batch 6] [--size 256] [--iters 12] [--steps 5] [--warmup 2] [--out profiles/fine_tune_bench.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from accflow_amd import ops, train, train_raft
    from accflow_amd.data.synthetic import gt_flow, make_sequence, make_state_dict, normalize
    from accflow_amd.networks import build_flow_estimator
    model = build_flow_estimator("raft")
    model.load_state_dict(make_state_dict(model), strict=True)
    model = train_raft.freeze_encoders(model.cuda())
    fr = [normalize(f).cuda() for f in make_sequence(11, 2, a.size, a.size, batch=a.batch)]
    gt = torch.as_tensor(gt_flow(0, 1, a.size, a.size)).float().cuda()[None].repeat(a.batch, 1, 1, 1).contiguous()
    params = train_raft.trainable_parameters(model)
    opt = torch.optim.AdamW(params, lr=1.2e-4, weight_decay=1e-5, eps=1e-8)
    losses = []

    def step():
        losses.append(train_raft.train_step(model, opt, fr[0], fr[1], gt, iters=a.iters)[0])
    for _ in range(a.warmup):
        step()
    ms = _timed(step, a.steps)
    # the parts: the frozen encoders alone, and forward + backward of the loop on given features
    with torch.no_grad():
        fmap1, fmap2 = model.fnet([fr[0], fr[1]])
        cnet = model.cnet(fr[0])
        ms_enc = _timed(lambda: (model.fnet([fr[0], fr[1]]), model.cnet(fr[0])), a.steps)
        model(fr[0], fr[1], iters=a.iters)
        ms_inf = _timed(lambda: model(fr[0], fr[1], iters=a.iters), a.steps)

    def loop():
        for p in params:
            p.grad = None
        train_raft.forward_backward(model, fmap1, fmap2, cnet, gt, iters=a.iters)
    ms_loop = _timed(loop, a.steps)
    res = {"workload": "fine-tune step RAFT update block, %dx%d batch %d, %d iterations (configs/RAFT.yml)" % (a.size, a.size, a.batch,
                                                                                                              a.iters),
           "ms_per_step": round(ms, 2), "pairs_per_s": round(a.batch / ms * 1e3, 2),
           "ms_forward_backward_on_features": round(ms_loop, 2), "ms_frozen_encoders": round(ms_enc, 2),
           "ms_inference_forward_same_batch": round(ms_inf, 2), "trainable_elements": sum(p.numel() for p in params),
           "losses": [round(x, 4) for x in losses], "steps": a.steps, "warmup": a.warmup, "conv_mode_train": train.TRAIN_CONV_MODE,
           "guard_trips": ops.guard_report(), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
