#!/usr/bin/env python3
"""Fine-tuning front end for the pair estimator, with the reference's fine_tune.py semantics on the HIP path (SURVEY section 2
rows 11-12): adapts RAFT to CVO's long intervals.  Stage 1: the update block (accflow_amd/train_raft.py).

    python -m accflow_amd.fine_tune -c configs/RAFT.yml [--steps N] [--resume auto|STEP] [--out DIR] [--valid-batches N] [--synthetic]

Reads the reference's YAML options unchanged (configs/RAFT.yml: exp_name, epochs, lr, wdecay, epsilon, batch_per_gpu, clip,
add_noise, log_freq, valid_freq, image_size, flow_pretrained ...; new keys `gamma` (0.85), `iters` (12) and `valid_iters` (20))
and mirrors fine_tune.py:113-326: per step an interval in 1..6 and a direction are drawn and pick the pair and its label
(:209-222; select_pair below), the noise field (:225-229), sequence_loss_raft with gamma over 12 iterations (loss.py:4-25),
clipping, AdamW and the one-cycle schedule; validation of (imgs[-1], imgs[0]) against bflows[-1] at `valid_iters` on the
inference path with best-EPE checkpoint rotation (:262-318); the estimator's whole state_dict saved under the `module.` prefix
of the reference's nn.DataParallel checkpoints.  The optimizer, the schedule, save_ckpt, rotate_ckpts, add_noise, the gradient
all-reduce, one process per GPU and the refusal to overwrite are train_acc's.

Differences, all deliberate:
  * only `update_block.*` is trainable: fnet and cnet are frozen and stay in eval(), so cnet's BatchNorm uses its running
    statistics (fine_tune.py:163's model.train() trains everything and runs BatchNorm on batch statistics - that needs the
    backward of the correlation lookup and of the normalisations: stage 2, not built);
  * there is no GradScaler and no autocast: forward in f16x3 under its range guard (a tripped step redone in bf16x6), backward in
    bf16x6 - fp32-equivalent arithmetic (train_raft.forward_backward);
  * one prediction per iteration: the reference's own call `sequence_loss_raft(model(...), ...)` (fine_tune.py:232-233) is
    inconsistent with its RAFT.forward, which returns the last prediction only (raft.py:146).  One prediction per
    iteration is upstream RAFT's training mode and what sequence_loss_raft iterates over (loss.py:10-13);
  * as train_acc: existing checkpoint directories are never archived or overwritten, a run ends at the step count the schedule
    was built for, best_epe / best_step travel in the `.state` file, and without the CVO training LMDB or the
    `flow_pretrained` checkpoint the run STOPS unless --synthetic (or ACCFLOW_SYNTHETIC=1).  The synthetic sequences carry no
    delta flows (data.dataset.SyntheticCVO refuses those keys): the adjacent labels are synthetic.gt_flow(0, 1) / gt_flow(1, 0).
"""
import argparse
import logging
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from accflow_amd import train_acc  # noqa: E402

DEFAULTS = dict(train_acc.DEFAULTS, gamma=0.85, iters=12, valid_iters=20)


def parse_options(path):
    import yaml
    with open(path) as f:
        opt = yaml.safe_load(f) or {}
    for k, v in DEFAULTS.items():
        opt.setdefault(k, v)
    if "exp_name" not in opt:
        raise ValueError("%s: no exp_name" % path)
    if str(opt["loss_type"]).upper() != "L1":
        raise NotImplementedError("loss_type %r: fine_tune.py only implements the L1 sequence loss" % opt["loss_type"])
    return argparse.Namespace(**opt)


def draw_interval():
    """fine_tune.py:209-210: an interval in 1..6 (numpy's generator) and a direction (python's), like the reference."""
    return int(np.random.randint(1, 7)), random.choice([-1, 1])


def select_pair(imgs, labels, interval, direction):
    """fine_tune.py:211-222 -> ((image1, image2), label).  labels: the batch dict's flow lists."""
    if not 1 <= interval <= 6 or direction not in (-1, 1):
        raise ValueError("select_pair: interval in 1..6, direction +-1")
    if interval * direction == 1:            # local forward flow
        return (imgs[0], imgs[1]), labels["delta_fflows"][0]
    if interval * direction == -1:           # local backward flow
        return (imgs[1], imgs[0]), labels["delta_bflows"][0]
    if direction == 1:                       # cross-frame forward flow
        return (imgs[0], imgs[interval]), labels["fflows"][interval - 2]
    return (imgs[interval], imgs[0]), labels["bflows"][interval - 2]


def synthetic_delta_labels(like):
    """The adjacent labels of the synthetic sequences (every sample moves alike): gt_flow(0, 1) and gt_flow(1, 0)."""
    from accflow_amd.data.synthetic import gt_flow
    N, _, H, W = like.shape

    def rep(i, j):
        return torch.as_tensor(gt_flow(i, j, H, W)).float().to(like.device)[None].repeat(N, 1, 1, 1).contiguous()
    return {"delta_fflows": [rep(0, 1)], "delta_bflows": [rep(1, 0)]}


def validate(model, loader, dev, limit, iters):
    """fine_tune.py:262-284 on this rank: (imgs[-1], imgs[0]) against bflows[-1] on the inference path."""
    from accflow_amd import metrics
    from accflow_amd.eval_cvo import preprocess
    total, n = None, 0
    with torch.no_grad():
        for i, batch in enumerate(loader):
            if limit is not None and i >= limit:
                break
            d = preprocess(batch, dev)
            out = model(d["imgs"][-1], d["imgs"][0], iters=iters)
            m = metrics.flow_metrics(out, d["bflows"][-1])
            row = torch.stack([m.epe.mean(), m.px1.mean(), m.px3.mean(), m.px5.mean()])
            total = row if total is None else total + row
            n += 1
    if not n:
        raise RuntimeError("validate: the validation loader yielded no batch")
    return {"val_" + k: v for k, v in zip(("epe", "1px", "3px", "5px"), (total / n).cpu().tolist())}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", "-c", type=str, required=True)
    ap.add_argument("--steps", type=int, default=None, help="stop after this many optimizer steps (smoke runs)")
    ap.add_argument("--resume", type=str, default=None, help="'auto' (latest) or a saved step number (fine_tune.py:169-176)")
    ap.add_argument("--out", type=str, default=".", help="root of logs/<exp_name> and checkpoints/<exp_name>")
    ap.add_argument("--valid-batches", type=int, default=None, help="cap on validation batches per validation")
    ap.add_argument("--synthetic", action="store_true",
                    help="smoke run: synthetic sequences / synthetic estimator weights where the real ones are missing")
    a = ap.parse_args(argv)
    args = parse_options(a.config)
    synthetic_ok = a.synthetic or os.environ.get("ACCFLOW_SYNTHETIC", "0") == "1"
    import torch.distributed as dist
    from accflow_amd import train_raft
    from accflow_amd.data.dataset import fetch_train_dataloader, fetch_valid_dataloader, find_cvo_lmdb
    from accflow_amd.eval_cvo import _strip_module, preprocess
    from accflow_amd.networks import build_flow_estimator
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    log_dir, ckpt_dir = os.path.join(a.out, "logs", args.exp_name), os.path.join(a.out, "checkpoints", args.exp_name)
    # (as train_acc: every go / no-go decision is taken by EVERY rank before the process group exists)
    if a.resume is None and os.path.isdir(ckpt_dir) and os.listdir(ckpt_dir):
        raise SystemExit("%s holds checkpoints: pass --resume auto or another --out" % ckpt_dir)
    have_lmdb = find_cvo_lmdb(True) is not None
    if not synthetic_ok:
        missing = [what for what, ok in (("the CVO training LMDB (ACCFLOW_CVO_LMDB / data/datasets/CVO_full/cvo_train.lmdb)", have_lmdb),
                                         ("flow_pretrained %r" % args.flow_pretrained,
                                          bool(args.flow_pretrained) and os.path.isfile(args.flow_pretrained))) if not ok]
        if missing:
            raise SystemExit("fine_tune: %s not found - a real run needs them; pass --synthetic (or ACCFLOW_SYNTHETIC=1) for a "
                             "smoke run on synthetic sequences / synthetic estimator weights" % " and ".join(missing))
    model = build_flow_estimator(args.exp_name)
    train_raft.check_model(model)               # (RAFT-small / GMA: stage 2 - refused before anything is created)
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(dev)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
    if rank == 0:
        os.makedirs(log_dir, exist_ok=True)
        os.makedirs(ckpt_dir, exist_ok=True)
    if world > 1:
        dist.barrier()
    logging.basicConfig(level=logging.INFO if rank == 0 else logging.WARNING, format="%(asctime)s %(message)s",
                        handlers=[logging.StreamHandler()] + ([logging.FileHandler(os.path.join(log_dir, "base_%s.log" % args.exp_name))]
                                                              if rank == 0 else []))
    log = logging.getLogger("base")

    # ---- data (fine_tune.py:131-154); the synthetic sequences have no delta keys ----
    crop = args.image_size[0] if isinstance(args.image_size, (list, tuple)) else args.image_size
    keys = ["fflows", "bflows", "delta_fflows", "delta_bflows"] if have_lmdb else ["fflows", "bflows"]
    loader, dst = fetch_train_dataloader(keys=keys, batch=args.batch_per_gpu, crop_size=crop, split="clean+final", workers=0,
                                         rank=rank, world=world, seed=1234)
    vloader, _ = fetch_valid_dataloader(keys=["bflows"], split="clean", batch=args.batch_per_gpu)
    per_epoch = max(1, len(loader))
    num_steps = per_epoch * args.epochs
    log.info("Train on %d samples with batch %d x %d ranks, %d iters/epoch, %d iters in total", len(dst), args.batch_per_gpu,
             world, per_epoch, num_steps)

    # ---- model & optimizer (:156-168) ----
    synthetic_used = not have_lmdb
    if args.flow_pretrained and os.path.isfile(args.flow_pretrained):
        model.load_state_dict(_strip_module(torch.load(args.flow_pretrained, map_location="cpu")))
    else:
        from accflow_amd.data.synthetic import make_state_dict
        log.warning("SMOKE RUN: flow_pretrained %r not found, the estimator gets the build's deterministic synthetic weights",
                    args.flow_pretrained)
        model.load_state_dict(make_state_dict(model), strict=True)
        synthetic_used = True
    model = train_raft.freeze_encoders(model.to(dev))
    params = train_raft.trainable_parameters(model)
    log.info("model: %s  trainable %d (update_block), frozen %d parameters", args.exp_name, sum(p.numel() for p in params),
             sum(p.numel() for p in model.parameters() if not p.requires_grad))
    optimizer, scheduler = train_acc.fetch_optimizer(args, params, num_steps)
    step, best_epe, best_step = 0, 1e10, 0
    if a.resume is not None:
        stem = "latest" if a.resume.lower() == "auto" else "%06d" % int(a.resume)
        model.load_state_dict(_strip_module(torch.load(os.path.join(ckpt_dir, stem + ".pth"), map_location="cpu")), strict=True)
        state = torch.load(os.path.join(ckpt_dir, stem + ".state"), map_location="cpu")
        optimizer.load_state_dict(state["optimizer"])
        scheduler.load_state_dict(state["scheduler"])
        step = state["iter"]
        best_epe, best_step = state.get("best_epe", 1e10), state.get("best_step", step)
        log.info("resumed %s at iter %d", stem, step)
    elif world > 1:                           # every rank starts from rank 0's weights
        for p in model.state_dict().values():
            dist.broadcast(p, 0)

    losses, epes, t_last = [], [], time.time()
    done = step >= num_steps
    for epoch in range(step // per_epoch, args.epochs):
        if done:
            break
        skip = step - epoch * per_epoch if epoch == step // per_epoch else 0
        loader.sampler.set_epoch(epoch, skip=skip * args.batch_per_gpu)
        for batch in loader:
            step += 1
            d = preprocess(batch, dev)
            imgs = d["imgs"]
            if "delta_fflows" not in d:
                d.update(synthetic_delta_labels(imgs[0]))
            interval, direction = draw_interval()
            pair, label = select_pair(imgs, d, interval, direction)
            if args.add_noise:
                pair = train_acc.add_noise(list(pair))
            loss, ups = train_raft.train_step(model, optimizer, pair[0], pair[1], label, iters=args.iters, gamma=args.gamma,
                                              clip=args.clip, scheduler=scheduler)
            losses.append(loss)
            epes.append(train_acc.sequence_loss_metrics(ups, [label])["epe"])
            if step % args.log_freq == 0 or step < 25:
                dt = (time.time() - t_last) / len(losses)
                log.info("<epoch:%2d, iter:%6d, t:%.2fs, eta:%.2fh, loss:%.3f, epe:%.3f>", epoch, step, dt,
                         dt * (num_steps - step) / 3600, sum(losses) / len(losses), sum(epes) / len(epes))
                losses, epes, t_last = [], [], time.time()
            last = (a.steps is not None and step >= a.steps) or step >= num_steps
            if step % args.valid_freq == 0 or last:
                if rank == 0:
                    vm = validate(model, vloader, dev, a.valid_batches, args.valid_iters)
                    new_best = vm["val_epe"] <= best_epe
                    if new_best:
                        best_epe, best_step = vm["val_epe"], step
                    extra = {"best_epe": best_epe, "best_step": best_step, "synthetic": bool(synthetic_used)}
                    train_acc.save_ckpt(step, scheduler, optimizer, model, ckpt_dir, True, extra)
                    if new_best:
                        train_acc.save_ckpt(step, scheduler, optimizer, model, ckpt_dir, False, extra)
                        train_acc.rotate_ckpts(ckpt_dir)
                    log.info("Validation EPE: %.3f, current best EPE: %.3f(step: %s)", vm["val_epe"], best_epe, best_step)
                if world > 1:
                    dist.barrier()
            if last:
                done = True
                break
        if done:
            break
    if rank == 0:
        torch.save({"module." + k: v.detach().cpu() for k, v in model.state_dict().items()}, os.path.join(ckpt_dir, "final.pth"))
        log.info("Finish training")
    if world > 1:
        dist.destroy_process_group()
    return step


if __name__ == "__main__":
    main()
