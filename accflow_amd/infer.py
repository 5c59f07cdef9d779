#!/usr/bin/env python3
"""Long-range flow of a folder of frames: python -m accflow_amd.infer --frames DIR|GLOB --out DIR [--flo] [--kitti] [--png]

The frames (PNG or binary PPM, all of one size, in sorted order) are decoded into one pinned buffer, sent to the device with
one copy and turned into the estimators' input with one launch (frames.FramePadder.ingest).  They are then pushed frame by
frame through AccFlowStream (--acc acc; constant memory whatever the length) or, with --acc direct, the estimator runs on
(frame i, frame 0) for every i.  For each i >= 2 the flow F(i -> 0) is written as
    flow_<i>_to_0.flo        --flo    Middlebury .flo, float32
    flow_<i>_to_0_kitti.png  --kitti  16-bit PNG, KITTI's coding: 64 f + 32768, third channel 1 = valid
    flow_<i>_to_0.png        --png    the Middlebury colour coding
from ops.flow_export and viz.flow_to_image; nothing but the file's bytes is formed on the host.

The colour PNGs of a run share a scale so that their colours are comparable: picture i is drawn at the largest |flow| of the
PADDED flows 2..i - what has been seen so far, not the whole sequence's maximum, which a stream cannot know.  A flow that
grows along the sequence therefore keeps its colours from its frame on; earlier pictures are not redrawn.

--size WxH | --scale S | --max-side N run the network at a working size (frames.FrameScaler: footage larger than the network
should see - its displacements beyond the lookup's reach, its cost growing with the pixel count); the frames are resampled
inside the ingest launch (--interp bilinear|area).  With --flows-at source (the default) every file is at the frames' own
size again - the flow resampled and its vectors rescaled inside the export launch, the colour PNG drawn from that flow and
scaled by its maxima - with --flows-at working at the working size.

Without checkpoints the deterministic synthetic weights are used (announced on stderr): the files are then good for timing
and for testing the pipeline, not for looking at.
"""
import argparse
import glob
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from accflow_amd import frames as _frames, ops, viz  # noqa: E402

EXTENSIONS = (".png", ".ppm")
KITTI_SCALE = 64.0


def frame_paths(spec):
    """DIR: its .png / .ppm files; anything else: a glob pattern.  Sorted by name."""
    if os.path.isdir(spec):
        paths = [os.path.join(spec, n) for n in os.listdir(spec) if n.lower().endswith(EXTENSIONS)]
    else:
        paths = glob.glob(spec)
    return sorted(paths)


def parse_size(text):
    """'WxH' -> (H, W)."""
    try:
        w, h = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError("expected WxH, e.g. 1024x436, got %r" % text)
    if w < 1 or h < 1:
        raise argparse.ArgumentTypeError("expected a positive WxH, got %r" % text)
    return h, w


def run(frames, out=None, acc="acc", ofe="raft", acc_ckpt=None, ofe_ckpt=None, iters=None, pad="sintel", flo=False, kitti=False,
        png=False, bgr=False, model=None, device="cuda", size=None, scale=None, max_side=None, interp="bilinear",
        flows_at="source"):
    """frames: a directory, a glob pattern or a list of paths.  Returns [F(i -> 0) for i = 2 .. n-1], each (1,2,H,W) float32
    on the device at the frames' own size (a view of the padded flow).  out: the directory the files go to (needed with flo,
    kitti or png).  model: a built model to use instead of eval_cvo.build_model(acc, ofe, acc_ckpt, ofe_ckpt, device).
    size = (h, w) / scale / max_side (at most one; frames.working_size): the network runs at that working size - the frames
    are resampled in ingest's launch (interp: "bilinear" or "area") - and, with flows_at="source", the returned flows and
    every file are at the frames' own size again, resampled and rescaled in export's launch; flows_at="working" leaves
    them at the working size."""
    from accflow_amd.networks.AccFlow_ import AccFlowStream
    paths = frame_paths(frames) if isinstance(frames, str) else list(frames)
    if len(paths) < 3:
        raise ValueError("infer: %d frame(s) found, an accumulated flow needs at least 3" % len(paths))
    if (flo or kitti or png) and out is None:
        raise ValueError("infer: an output directory is needed to write files")
    if acc not in ("acc", "direct") or pad not in ("sintel", "kitti"):
        raise ValueError("infer: acc is 'acc' or 'direct' and pad 'sintel' or 'kitti', got %r and %r" % (acc, pad))
    if flows_at not in ("source", "working"):
        raise ValueError("infer: flows_at is 'source' or 'working', got %r" % (flows_at,))
    device = torch.device(device)
    if model is None:
        from accflow_amd.eval_cvo import build_model
        if not (acc_ckpt if acc == "acc" else ofe_ckpt):
            print("infer: no checkpoint given - running on the deterministic synthetic weights", file=sys.stderr)
        model = build_model(acc, ofe, acc_ckpt, ofe_ckpt, device)
    if out is not None:
        os.makedirs(out, exist_ok=True)
    u8 = _frames.load_frames(paths, device)
    scaler = _frames.FrameScaler(u8.shape[1:3], size=size, scale=scale, max_side=max_side, pad=pad, interp=interp)
    padder = scaler.padder
    # (the model's padded working-size flow goes out through the scaler, at the source size, or through the padder alone)
    to_source = scaler.resizes and flows_at == "source"
    back = scaler if to_source else padder
    x = scaler.ingest(u8, layout="hwc", bgr=bgr)
    kw = {} if iters is None else {"iters": iters}
    stream = AccFlowStream(model, **kw) if acc == "acc" else None
    flows, seen = [], None
    with torch.no_grad():
        for i in range(len(paths)):
            if stream is not None:
                got = stream.push(x[i:i + 1])
            else:
                got = [model(x[i:i + 1], x[0:1], **kw)] if i >= 2 else []
            for flow in got:
                flow = flow.contiguous()
                flows.append(scaler.flow(flow) if to_source else padder.unpad(flow))
                stem = os.path.join(out, "flow_%d_to_0" % i) if out is not None else None
                if flo:
                    _frames.write_flo(stem + ".flo", back.export(flow, coding="f32")[0])
                if kitti:
                    _frames.write_png16(stem + "_kitti.png", back.export(flow, coding="u16", scale=KITTI_SCALE, big_endian=True)[0])
                if png and to_source:                                   # drawn from the resized flow, scaled by its own maximum
                    full = flows[-1]
                    rad = ops.flow_maxrad(full)
                    seen = rad if seen is None else torch.maximum(seen, rad)
                    viz.write_png(stem + ".png", viz.flow_to_image(full, max_rad=seen)[0])
                elif png:
                    rad = ops.flow_maxrad(flow)
                    seen = rad if seen is None else torch.maximum(seen, rad)
                    y0, x0, H, W = padder.crop
                    viz.write_png(stem + ".png", viz.flow_to_image(flow, max_rad=seen)[0, y0:y0 + H, x0:x0 + W])
    return flows


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", required=True, metavar="DIR|GLOB")
    ap.add_argument("--out", required=True, metavar="DIR")
    ap.add_argument("--acc", "-acc", choices=["acc", "direct"], default="acc")
    ap.add_argument("--ofe", "-ofe", choices=["raft", "gma"], default="raft")
    ap.add_argument("--acc_ckpt", default=None)
    ap.add_argument("--ofe_ckpt", default=None)
    ap.add_argument("--iters", type=int, default=None, help="the estimator's refinement iterations (default: the model's)")
    ap.add_argument("--pad", choices=["sintel", "kitti"], default="sintel")
    ap.add_argument("--flo", action="store_true", help="write Middlebury .flo files")
    ap.add_argument("--kitti", action="store_true", help="write 16-bit KITTI flow PNGs")
    ap.add_argument("--png", action="store_true", help="write colour-coded PNGs")
    ap.add_argument("--bgr", action="store_true", help="hand the model BGR channel order (weights trained on BGR-decoded frames)")
    sz = ap.add_mutually_exclusive_group()
    sz.add_argument("--size", type=parse_size, default=None, metavar="WxH", help="run the network at this working size")
    sz.add_argument("--scale", type=float, default=None, metavar="S", help="working size = the frames' size times S")
    sz.add_argument("--max-side", type=int, default=None, metavar="N", help="shrink frames whose longer side exceeds N to N")
    ap.add_argument("--interp", choices=["bilinear", "area"], default="bilinear", help="how the frames are resampled")
    ap.add_argument("--flows-at", choices=["source", "working"], default="source",
                    help="the size of the written flows: the frames' own (resampled back, vectors rescaled) or the working size")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if not (a.flo or a.kitti or a.png):
        a.flo = True
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(dev)
    flows = run(a.frames, a.out, acc=a.acc, ofe=a.ofe, acc_ckpt=a.acc_ckpt, ofe_ckpt=a.ofe_ckpt, iters=a.iters, pad=a.pad,
                flo=a.flo, kitti=a.kitti, png=a.png, bgr=a.bgr, device=dev, size=a.size, scale=a.scale, max_side=a.max_side,
                interp=a.interp, flows_at=a.flows_at)
    print("infer: %d flow(s) of %d x %d written to %s" % (len(flows), flows[0].shape[2], flows[0].shape[3], a.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
