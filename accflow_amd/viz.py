"""Showing a flow: the Middlebury colour coding on the device, and a PNG writer for what it paints.

The reference colours a flow with numpy on the host (utils/flow_viz.py: one device-to-host copy of the flow, then a dozen
full-frame temporaries).  Here it is two HIP launches (ops.flow_maxrad, ops.flow_to_rgb: csrc/flow_viz.hip): the first
leaves each sample's scale in device memory, the second reads it there, so nothing in `flow_to_image` waits for the device
and the picture stays where a video encoder or the next kernel can take it.  `write_png` is the only step that needs the
bytes on the host.
"""
import struct
import zlib

import torch

from . import ops
from .networks._packs import require_cuda

__all__ = ["flow_to_image", "write_png", "save_flow"]


def flow_to_image(flow, max_rad=None, clip_flow=None, convert_to_bgr=False, layout="hwc"):
    """flow (B,2,H,W) or (2,H,W) on the device -> uint8 (B,H,W,3) / (H,W,3) on the device (layout "chw": (B,3,H,W) / (3,H,W)).

    max_rad   None: every sample is scaled by its own largest |flow|, as the reference's flow_to_image does;
              "batch": one scale for the whole batch - the colours of a sequence's frames are then comparable;
              a float or a (B,) float32 device tensor: that scale (one launch) - flows beyond it are drawn at 3/4 brightness.
    clip_flow the reference's np.clip(flow, 0, clip_flow) before anything else (negative components become 0).
    Pixels with a non-finite component or one beyond 1e9 are black and do not count for the scale."""
    if not isinstance(flow, torch.Tensor) or flow.dim() not in (3, 4):
        raise RuntimeError("flow_to_image: flow must be a (B,2,H,W) or (2,H,W) tensor, got %s" % (
            tuple(flow.shape) if isinstance(flow, torch.Tensor) else type(flow),))
    require_cuda(flow)
    single = flow.dim() == 3
    if single:
        flow = flow[None]
    B = flow.shape[0]
    if max_rad is None or (isinstance(max_rad, str) and max_rad == "batch"):
        scale = ops.flow_maxrad(flow, clip=clip_flow, shared=max_rad is not None)
    elif isinstance(max_rad, torch.Tensor):
        require_cuda(max_rad)
        scale = max_rad.to(torch.float32).reshape(-1).contiguous()
    elif isinstance(max_rad, (int, float)):
        scale = torch.full((B,), float(max_rad), dtype=torch.float32, device=flow.device)
    else:
        raise RuntimeError("flow_to_image: max_rad must be None, 'batch', a number or a (B,) device tensor, got %r" % (max_rad,))
    img = ops.flow_to_rgb(flow, scale, clip=clip_flow, bgr=convert_to_bgr, layout=layout)
    return img[0] if single else img


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, img, level=6):
    """uint8 (H,W,3) - a tensor on any device or anything with the buffer of one - as an 8-bit RGB PNG: one IDAT chunk, every
    scanline with filter 0.  Standard library only."""
    if isinstance(img, torch.Tensor):
        if img.dtype != torch.uint8:
            raise ValueError("write_png: expected uint8, got %s" % img.dtype)
        img = img.detach().cpu().contiguous().numpy()
    view = memoryview(img)
    if view.format != "B" or view.ndim != 3 or view.shape[2] != 3 or view.shape[0] < 1 or view.shape[1] < 1:
        raise ValueError("write_png: expected a uint8 (H,W,3) image, got format %r shape %s" % (view.format, view.shape))
    if not view.c_contiguous:
        raise ValueError("write_png: the image must be C-contiguous")
    H, W = view.shape[:2]
    raw, row = view.tobytes(), 3 * W
    lines = b"".join(b"\x00" + raw[y * row:(y + 1) * row] for y in range(H))
    png = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
           + _chunk(b"IDAT", zlib.compress(lines, level)) + _chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)


def save_flow(flow, path):
    """The reference's save_flow (train_acc.py:90-93): sample 0 of an (N,2,H,W) batch, coloured at its own scale, as a PNG."""
    write_png(path, flow_to_image(flow[:1])[0])
