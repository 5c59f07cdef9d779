"""Gradient fixture of the update block's fine-tuning step, made by running the REFERENCE (mulns/AccFlow at /root/reference,
read-only) with its own autograd on the CPU in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_raft_ft_golden.py

What it does (imports as in make_golden.py):
  * builds the reference RAFT with the build's deterministic weights, fp32 (mixed_precision = False), .eval() - cnet's
    BatchNorm on its running statistics - with fnet / cnet frozen (accflow_amd/fine_tune.py lists both as deliberate);
  * one seeded 128 x 160 pair, 3 refinement iterations.  The reference's RAFT.forward returns the last prediction only, so the
    per-iteration predictions - what loss.sequence_loss_raft iterates over - are recorded by wrapping `upsample_flow`;
  * loss = loss.sequence_loss_raft(predictions, gt, gamma) with a seeded ground truth, loss.backward();
  * stores the loss and for every update_block parameter: L2 norm and sum of its gradient (float64) and a strided sample of
    <= 2048 gradient values.  No feature maps: tests/test_fine_tune_host.py re-derives them from the same seeded frames.
The fixture holds tensors only; the GPU box never needs /root/reference."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
from make_golden import import_reference, make_state_dict, npy, pair  # noqa: E402

MAX_SAMPLE = 2048
H, W, SEED, GT_SEED, ITERS, GAMMA = 128, 160, 1000, 4321, 3, 0.85


def flow_gt(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return 3.0 * torch.randn(1, 2, H, W, generator=g)


def main():
    torch.set_num_threads(8)
    build, _ = import_reference()
    from loss import sequence_loss_raft
    model = build("raft")
    model.load_state_dict(make_state_dict(model), strict=True)
    model.eval()
    model.args.mixed_precision = False
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith("update_block.")
    i1, i2 = pair(SEED, H, W)
    gt = flow_gt(H, W, GT_SEED)
    preds = []
    orig = model.upsample_flow

    def record(flow, mask):
        up = orig(flow, mask)
        preds.append(up)
        return up
    model.upsample_flow = record
    last = model(i1, i2, iters=ITERS)
    model.upsample_flow = orig
    assert len(preds) == ITERS and preds[-1] is last
    loss, metrics = sequence_loss_raft(preds, gt, GAMMA)
    loss.backward()
    g = {"H": H, "W": W, "seed": SEED, "gt_seed": GT_SEED, "iters": ITERS, "gamma": np.float64(GAMMA),
         "loss": np.float64(loss.item()), "epe": np.float64(metrics["epe"]), "last": npy(last[:, :, ::4, ::4])}
    names = []
    for name, p in model.named_parameters():
        if not name.startswith("update_block."):
            assert p.grad is None, name
            continue
        assert p.grad is not None, name
        gr = p.grad.detach().double().reshape(-1)
        step = max(1, -(-gr.numel() // MAX_SAMPLE))
        names.append(name)
        g["l2/" + name] = np.float64(gr.norm().item())
        g["sum/" + name] = np.float64(gr.sum().item())
        g["step/" + name] = np.int64(step)
        g["val/" + name] = gr[::step].float().numpy()
        assert g["val/" + name].size <= MAX_SAMPLE
    g["names"] = np.array(names)
    out = os.path.join(HERE, "raft_ft_grad.npz")
    np.savez_compressed(out, **g)
    print("loss", loss.item(), "params", len(names), "bytes", os.path.getsize(out))


if __name__ == "__main__":
    main()
