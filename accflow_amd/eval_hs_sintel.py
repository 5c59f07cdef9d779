#!/usr/bin/env python3
"""High-Speed Sintel evaluation: python -m accflow_amd.eval_hs_sintel --root DIR [--interv 6] [--acc acc|direct]
                                                                      [--ofe raft|gma] [--acc_ckpt F] [--ofe_ckpt F]

Every sample of data.dataset.High_Speed_Sintel holds two original Sintel frames, the high-speed frames rendered between
them, the ground-truth flow from the first original frame to the second and its occlusion mask.  Every interv-th high-speed
frame is taken (both ends included), resampled to the ground truth's size in ingest's launch (frames.FrameScaler - the
reference's loader does this with cv2.resize on the host) and handed to the model in REVERSED order: the model returns
F(last of its list -> first of its list), the ground truth runs from the first frame to the last.  The last returned flow is
scored with metrics.flow_metrics: EPE over all, occluded and visible pixels per sample, and their means.

Without checkpoints the deterministic synthetic weights are used (announced on stderr): the numbers then test the
pipeline, they are not results.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from accflow_amd import frames as _frames, metrics  # noqa: E402


def predict(model, hs_u8, size, acc="acc", device="cuda"):
    """hs_u8: the chosen high-speed frames in file order, a list of uint8 (H0,W0,3) tensors -> the predicted flow from the
    first to the last of them, (1,2,h,w) at size = (h, w)."""
    if len(hs_u8) < (3 if acc == "acc" else 2):
        raise ValueError("eval_hs_sintel: %d frame(s) chosen, %s needs at least %d" % (len(hs_u8), acc, 3 if acc == "acc" else 2))
    u8 = torch.stack(list(hs_u8)[::-1]).to(device)
    scaler = _frames.FrameScaler(u8.shape[1:3], size=tuple(int(v) for v in size))
    x = scaler.ingest(u8)
    imgs = [x[k:k + 1] for k in range(x.shape[0])]
    with torch.no_grad():
        flow = model(imgs)[-1] if acc == "acc" else model(imgs[-1], imgs[0])
    return scaler.padder.unpad(flow).contiguous()


def run(root, interv=6, acc="acc", ofe="raft", acc_ckpt=None, ofe_ckpt=None, blacklist=(), model=None, device="cuda",
        keep_flows=False, verbose=True):
    """Returns {"samples": [{"name", "epe_all", "epe_occ", "epe_vis"} per sample], "mean": {"epe_all", "epe_occ", "epe_vis"}}
    (floats; plain means over the samples, NaN where a sample has no occluded pixel, as in eval_cvo); keep_flows: every
    sample's entry also holds its prediction under "flow"."""
    from accflow_amd.data.dataset import High_Speed_Sintel
    if acc not in ("acc", "direct"):
        raise ValueError("eval_hs_sintel: acc is 'acc' or 'direct', got %r" % (acc,))
    device = torch.device(device)
    dataset = High_Speed_Sintel(root, interv, list(blacklist))
    if len(dataset) == 0:
        raise ValueError("eval_hs_sintel: no sample under %s" % root)
    if model is None:
        from accflow_amd.eval_cvo import build_model
        if not (acc_ckpt if acc == "acc" else ofe_ckpt):
            print("eval_hs_sintel: no checkpoint given - running on the deterministic synthetic weights", file=sys.stderr)
        model = build_model(acc, ofe, acc_ckpt, ofe_ckpt, device)
    samples = []
    for index in range(len(dataset)):
        s = dataset[index]
        gt, occ = s["gt_flow"][None].to(device), s["occ_mask"][None].to(device)
        pred = predict(model, s["hs_sintel_u8"], gt.shape[2:], acc=acc, device=device)
        m = metrics.flow_metrics(pred, gt.contiguous(), occ.contiguous())
        entry = {"name": os.path.basename(dataset.sample_list[index]), "epe_all": float(m.epe[0]), "epe_occ": float(m.epe_occ[0]),
                 "epe_vis": float(m.epe_vis[0])}
        if verbose:
            print("%s  all:%.4f occ:%.4f vis:%.4f" % (entry["name"], entry["epe_all"], entry["epe_occ"], entry["epe_vis"]))
        if keep_flows:
            entry["flow"] = pred
        samples.append(entry)
    mean = {k: float(torch.tensor([e[k] for e in samples], dtype=torch.float64).mean()) for k in ("epe_all", "epe_occ", "epe_vis")}
    if verbose:
        print("Finish".center(50, "="))
        print("AVG EPE %s|%s over %d sample(s), interv %d: " % (acc, ofe, len(samples), interv))
        print("all:%.4f occ:%.4f vis:%.4f" % (mean["epe_all"], mean["epe_occ"], mean["epe_vis"]))
    return {"samples": samples, "mean": mean}


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", required=True, metavar="DIR", help="the folder of sample folders")
    ap.add_argument("--interv", type=int, default=6)
    ap.add_argument("--acc", "-acc", choices=["acc", "direct"], default="acc")
    ap.add_argument("--ofe", "-ofe", choices=["raft", "gma"], default="raft")
    ap.add_argument("--acc_ckpt", default=None)
    ap.add_argument("--ofe_ckpt", default=None)
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(dev)
    run(a.root, interv=a.interv, acc=a.acc, ofe=a.ofe, acc_ckpt=a.acc_ckpt, ofe_ckpt=a.ofe_ckpt, device=dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
