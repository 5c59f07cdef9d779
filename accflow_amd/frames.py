"""The boundary between files and the device: 8-bit frames in, flow files out.

A video is 8-bit interleaved frames of any size; the estimators take float32 (N,3,H,W) in [-1, 1] with H and W multiples of
8.  `FramePadder.ingest` is that step as ONE launch (ops.frames_from_u8: conversion, normalisation, channel order, planar
layout and replicate padding), where torch operators take six launches and five full-frame temporaries; its `export` is
`unpad` plus the coding of a flow file as one launch (ops.flow_export).  Both kernels: csrc/frame_io.hip.
`FrameScaler` puts a size policy on top - run at a working size, get the flow at the source size: its `ingest` resamples
the frames inside that one launch (ops.frames_from_u8(size=)), its `export` resamples and rescales the flow inside the other
(ops.flow_resize).

The file formats here are the host half - standard library and numpy only, like viz.write_png: a PNG / PPM reader
(`read_image`), Middlebury .flo (`write_flo`, `read_flo`: the reference's frame_utils.writeFlow / readFlow) and 16-bit RGB PNG
(`write_png16`: the container of frame_utils.writeFlowKITTI and of CVO's flows).  The decoder is written to be correct, not
fast: a video pipeline hands its decoder's buffers to `ingest` directly.
"""
import numbers
import struct
import zlib
from fractions import Fraction

import numpy as np
import torch

from . import ops
from .viz import _chunk

__all__ = ["FramePadder", "FrameScaler", "working_size", "read_image", "load_frames", "write_flo", "read_flo", "write_png16"]

FLO_TAG = 202021.25


class FramePadder:
    """InputPadder's arithmetic (networks/raft/utils/utils.py) on 8-bit frames: pads to multiples of 8, centred for mode
    "sintel", height at the bottom and width centred for "kitti" (any other mode name, as in InputPadder)."""

    def __init__(self, dims, mode="sintel"):
        self.ht, self.wd = int(dims[-2]), int(dims[-1])
        pad_ht = (((self.ht // 8) + 1) * 8 - self.ht) % 8
        pad_wd = (((self.wd // 8) + 1) * 8 - self.wd) % 8
        if mode == "sintel":
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, pad_ht // 2, pad_ht - pad_ht // 2]
        else:
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, 0, pad_ht]

    @property
    def crop(self):
        """(y0, x0, H, W) of the frame inside the padded frame."""
        return (self._pad[2], self._pad[0], self.ht, self.wd)

    def ingest(self, u8, layout="hwc", bgr=False, normalize=True, out=None):
        """uint8 (N,H,W,3) or (H,W,3) (layout "chw": (N,3,H,W) or (3,H,W)) on the device -> float32 (N,3,Hp,Wp), padded."""
        if isinstance(u8, torch.Tensor) and u8.dim() == 3:
            u8 = u8[None]
        if isinstance(u8, torch.Tensor) and u8.dim() == 4 and layout in ("hwc", "chw"):
            hw = tuple(u8.shape[1:3]) if layout == "hwc" else tuple(u8.shape[2:4])
            if hw != (self.ht, self.wd):
                raise RuntimeError("FramePadder.ingest: frames are %d x %d, the padder was made for %d x %d" % (hw + (self.ht, self.wd)))
        return ops.frames_from_u8(u8, layout=layout, bgr=bgr, pad=tuple(self._pad), normalize=normalize, out=out)

    def unpad(self, x):
        """A view of the frame's part of a padded (..., Hp, Wp) tensor."""
        y0, x0, H, W = self.crop
        return x[..., y0:y0 + H, x0:x0 + W]

    def export(self, flow, coding="f32", scale=64.0, big_endian=False, out=None):
        """A padded flow (N,2,Hp,Wp) -> the file payload of its unpadded part (ops.flow_export)."""
        return ops.flow_export(flow, crop=self.crop, coding=coding, scale=scale, big_endian=big_endian, out=out)


def working_size(dims, size=None, scale=None, max_side=None):
    """The (h, w) the network should see for source frames of dims[-2:], in integer arithmetic:
    size = (h, w): as given;  scale = s: floor(side * s + 0.5) per side, at least 8 (s is taken as the exact rational a float
    is);  max_side = m: unchanged where the longer side is <= m, otherwise the longer side becomes m and the other
    floor(other * m / longer + 0.5), at least 1;  none of them: the source size.  More than one of them raises."""
    ht, wd = int(dims[-2]), int(dims[-1])
    if ht < 1 or wd < 1:
        raise RuntimeError("FrameScaler: frames of %d x %d" % (ht, wd))
    if sum(a is not None for a in (size, scale, max_side)) > 1:
        raise RuntimeError("FrameScaler: give at most one of size, scale and max_side")
    if size is not None:
        return ops._size2(size, "FrameScaler")
    if scale is not None:
        try:
            s = Fraction(scale)
        except (TypeError, ValueError, OverflowError):
            s = Fraction(0)
        if s <= 0:
            raise RuntimeError("FrameScaler: scale must be a positive finite number, got %r" % (scale,))
        return tuple(max(8, int((2 * side * s + 1) // 2)) for side in (ht, wd))
    if max_side is not None:
        if isinstance(max_side, bool) or not isinstance(max_side, numbers.Integral) or max_side < 1:
            raise RuntimeError("FrameScaler: max_side must be a positive integer, got %r" % (max_side,))
        m, longer = int(max_side), max(ht, wd)
        if longer <= m:
            return ht, wd
        other = max(1, (2 * min(ht, wd) * m + longer) // (2 * longer))
        return (m, other) if ht >= wd else (other, m)
    return ht, wd


class FrameScaler:
    """Run at a working size, get the flow at the source size: frames of dims[-2:] are resampled to `.size` inside ingest's
    launch and the flow is resampled back - its vectors scaled with it - inside export's.  size / scale / max_side:
    working_size's policy (at most one).  `.padder` is the FramePadder of the working size; pad: its mode.  interp:
    "bilinear" or "area", for the frames (a flow is always resampled bilinearly).  With no size argument - or one that
    leaves the size as it is - every method is the FramePadder's."""

    def __init__(self, dims, size=None, scale=None, max_side=None, pad="sintel", interp="bilinear"):
        if interp not in ("bilinear", "area"):
            raise RuntimeError("FrameScaler: interp must be 'bilinear' or 'area', got %r" % (interp,))
        self.ht, self.wd = int(dims[-2]), int(dims[-1])
        self.size = working_size(dims, size, scale, max_side)
        self.interp = interp
        self.padder = FramePadder(self.size, mode=pad)
        self.resizes = self.size != (self.ht, self.wd)

    def ingest(self, u8, layout="hwc", bgr=False, normalize=True, out=None):
        """uint8 frames at the source size -> float32 (N,3,Hp,Wp) at the padded working size, one launch."""
        if not self.resizes:
            return self.padder.ingest(u8, layout=layout, bgr=bgr, normalize=normalize, out=out)
        if isinstance(u8, torch.Tensor) and u8.dim() == 3:
            u8 = u8[None]
        if isinstance(u8, torch.Tensor) and u8.dim() == 4 and layout in ("hwc", "chw"):
            hw = tuple(u8.shape[1:3]) if layout == "hwc" else tuple(u8.shape[2:4])
            if hw != (self.ht, self.wd):
                raise RuntimeError("FrameScaler.ingest: frames are %d x %d, the scaler was made for %d x %d" % (hw + (self.ht, self.wd)))
        return ops.frames_from_u8(u8, layout=layout, bgr=bgr, pad=tuple(self.padder._pad), normalize=normalize, out=out,
                                  size=self.size, interp=self.interp)

    def _window(self, flow, who):
        """(flow, crop): a padded working flow with the frame's window, or an unpadded one (made dense) with none."""
        h, w = self.size
        pl, pr, pt, pb = self.padder._pad
        if isinstance(flow, torch.Tensor) and flow.dim() == 4:
            if tuple(flow.shape[2:]) == (h + pt + pb, w + pl + pr):
                return flow, self.padder.crop
            if tuple(flow.shape[2:]) == (h, w):
                return flow.contiguous(), None
        raise RuntimeError("FrameScaler.%s: expected a (N,2,%d,%d) flow of the working size or its padded form, got %s" % (
            who, h, w, tuple(flow.shape) if isinstance(flow, torch.Tensor) else type(flow)))

    def flow(self, flow):
        """A working-size flow - padded (N,2,Hp,Wp) as the model returns it, or unpadded (N,2,h,w) - as (N,2,H,W) at the
        SOURCE size.  Without a resize: the padder's unpad (a view)."""
        flow, crop = self._window(flow, "flow")
        if not self.resizes:
            return flow if crop is None else self.padder.unpad(flow)
        return ops.flow_resize(flow, (self.ht, self.wd), crop=crop, coding="nchw")

    def export(self, flow, coding="f32", scale=64.0, big_endian=False, out=None):
        """A working-size flow (as in `flow`) -> the file payload at the SOURCE size, one launch."""
        if not self.resizes:
            return self.padder.export(flow, coding=coding, scale=scale, big_endian=big_endian, out=out)
        if coding not in ("f32", "u16"):
            raise RuntimeError("FrameScaler.export: coding must be 'f32' or 'u16', got %r" % (coding,))
        flow, crop = self._window(flow, "export")
        return ops.flow_resize(flow, (self.ht, self.wd), crop=crop, coding=coding, scale=scale, big_endian=big_endian, out=out)


# ------------------------------------------------------------------------------------------------
# images


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def _read_png(data, path):
    pos, ihdr, idat = 8, None, []
    while pos + 8 <= len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise ValueError("read_image: %s: truncated %s chunk" % (path, tag.decode("latin-1")))
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError("read_image: %s: bad checksum in the %s chunk" % (path, tag.decode("latin-1")))
        pos += 12 + n
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
    if ihdr is None or not idat:
        raise ValueError("read_image: %s: no IHDR or no IDAT chunk" % path)
    W, H, depth, ctype, comp, filt, interlace = ihdr
    if interlace != 0:
        raise ValueError("read_image: %s: interlaced PNGs are not supported" % path)
    if depth != 8:
        raise ValueError("read_image: %s: bit depth %d is not supported (8 only)" % (path, depth))
    if ctype not in (0, 2, 6):
        raise ValueError("read_image: %s: colour type %d is not supported (gray, RGB and RGBA only)" % (path, ctype))
    if comp != 0 or filt != 0 or W < 1 or H < 1:
        raise ValueError("read_image: %s: malformed header" % path)
    bpp = {0: 1, 2: 3, 6: 4}[ctype]
    row = W * bpp
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != H * (row + 1):
        raise ValueError("read_image: %s: %d bytes of pixel data, expected %d" % (path, len(raw), H * (row + 1)))
    img = np.zeros((H, row), dtype=np.uint8)
    prev = np.zeros(row, dtype=np.uint8)
    for y in range(H):
        ft = raw[y * (row + 1)]
        line = np.frombuffer(raw, dtype=np.uint8, count=row, offset=y * (row + 1) + 1)
        if ft == 0:
            cur = line.copy()
        elif ft == 2:
            cur = line + prev                                   # (uint8 arithmetic wraps mod 256, as the format defines it)
        elif ft == 1:                                           # Sub: a running sum along the row, channel by channel
            cur = (np.cumsum(line.reshape(W, bpp), axis=0, dtype=np.uint32) & 255).astype(np.uint8).reshape(row)
        elif ft in (3, 4):
            cur = np.zeros(row, dtype=np.uint8)
            li, pv = line.tolist(), prev.tolist()
            c = [0] * row
            for i in range(row):
                a = c[i - bpp] if i >= bpp else 0
                if ft == 3:
                    pred = (a + pv[i]) >> 1
                else:
                    pred = _paeth(a, pv[i], pv[i - bpp] if i >= bpp else 0)
                c[i] = (li[i] + pred) & 255
            cur[:] = c
        else:
            raise ValueError("read_image: %s: unknown scanline filter %d in row %d" % (path, ft, y))
        img[y] = cur
        prev = cur
    img = img.reshape(H, W, bpp)
    if ctype == 0:
        return np.repeat(img, 3, axis=2)
    return np.ascontiguousarray(img[:, :, :3])


def _read_ppm(data, path):
    pos, fields = 2, []
    while len(fields) < 3:                                       # width, height, maxval: separated by whitespace, '#' starts a comment
        while pos < len(data) and (data[pos:pos + 1].isspace() or data[pos:pos + 1] == b"#"):
            if data[pos:pos + 1] == b"#":
                while pos < len(data) and data[pos:pos + 1] not in (b"\n", b"\r"):
                    pos += 1
            else:
                pos += 1
        start = pos
        while pos < len(data) and data[pos:pos + 1].isdigit():
            pos += 1
        if start == pos:
            raise ValueError("read_image: %s: malformed PPM header" % path)
        fields.append(int(data[start:pos]))
    if not data[pos:pos + 1].isspace():
        raise ValueError("read_image: %s: malformed PPM header" % path)
    pos += 1                                                     # exactly one whitespace byte ends the header
    W, H, maxval = fields
    if maxval != 255:
        raise ValueError("read_image: %s: PPM maxval %d is not supported (255 only)" % (path, maxval))
    if W < 1 or H < 1 or len(data) - pos < 3 * W * H:
        raise ValueError("read_image: %s: %d bytes of pixel data, expected %d" % (path, len(data) - pos, 3 * W * H))
    return np.frombuffer(data, dtype=np.uint8, count=3 * W * H, offset=pos).reshape(H, W, 3).copy()


def read_image(path):
    """An image file -> uint8 (H,W,3) RGB ndarray.  PNG: non-interlaced, bit depth 8, gray / RGB / RGBA (alpha dropped, gray
    replicated), every scanline filter; binary PPM (P6, maxval 255).  Anything else raises ValueError with the reason."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] == b"\x89PNG\r\n\x1a\n":
        return _read_png(data, path)
    if data[:2] == b"P6":
        return _read_ppm(data, path)
    raise ValueError("read_image: %s is neither a PNG nor a binary PPM (P6); JPEG and other formats are not supported" % path)


def load_frames(paths, device="cuda"):
    """The frames of `paths` as ONE uint8 (N,H,W,3) tensor on `device`: decoded into one pinned host buffer and sent with one
    host-to-device copy.  Frames of differing size raise."""
    paths = list(paths)
    if not paths:
        raise ValueError("load_frames: no frames")
    device = torch.device(device)
    buf = None
    for k, p in enumerate(paths):
        img = read_image(p)
        if buf is None:
            buf = torch.empty((len(paths),) + img.shape, dtype=torch.uint8, pin_memory=device.type == "cuda")
        if tuple(img.shape) != tuple(buf.shape[1:]):
            raise ValueError("load_frames: %s is %d x %d, %s is %d x %d" % (p, img.shape[0], img.shape[1], paths[0],
                                                                            buf.shape[1], buf.shape[2]))
        buf[k].copy_(torch.from_numpy(img))
    return buf.to(device, non_blocking=True)


# ------------------------------------------------------------------------------------------------
# flow files


def _host_array(x, dtype, who):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous()
        x = (x.view(torch.int16) if x.dtype == torch.uint16 else x).numpy()
    x = np.asarray(x)
    if x.dtype == np.int16 and dtype == np.uint16:
        x = x.view(np.uint16)
    if x.dtype != dtype:
        raise ValueError("%s: expected %s, got %s" % (who, np.dtype(dtype).name, x.dtype))
    return x


def write_flo(path, hw2):
    """float32 (H,W,2) = (u, v) per pixel - ops.flow_export's "f32" payload of one sample, a tensor on any device or an
    ndarray - as a Middlebury .flo file: the tag 202021.25, int32 width, int32 height, the payload, all little-endian."""
    a = _host_array(hw2, np.float32, "write_flo")
    if a.ndim != 3 or a.shape[2] != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_flo: expected a float32 (H,W,2) array, got shape %s" % (a.shape,))
    with open(path, "wb") as f:
        f.write(struct.pack("<fii", FLO_TAG, a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a).astype("<f4", copy=False).tobytes())


def read_flo(path):
    """A Middlebury .flo file -> float32 (H,W,2) ndarray."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or struct.unpack("<f", data[:4])[0] != FLO_TAG:
        raise ValueError("read_flo: %s does not start with the .flo tag 202021.25" % path)
    W, H = struct.unpack("<ii", data[4:12])
    if W < 1 or H < 1 or len(data) - 12 != 8 * W * H:
        raise ValueError("read_flo: %s: %d x %d needs %d payload bytes, the file has %d" % (path, H, W, 8 * W * H, len(data) - 12))
    return np.frombuffer(data, dtype="<f4", offset=12).reshape(H, W, 2).astype(np.float32)


def write_png16(path, hw3_be, level=6):
    """(H,W,3) 16-bit samples ALREADY in big-endian byte order - ops.flow_export(coding="u16", big_endian=True) of one sample
    - as a 16-bit RGB PNG: the buffer's rows are the scanlines as they stand, each with filter 0."""
    a = _host_array(hw3_be, np.uint16, "write_png16")
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png16: expected a 16-bit (H,W,3) array, got shape %s" % (a.shape,))
    H, W = a.shape[:2]
    raw, row = np.ascontiguousarray(a).tobytes(), 6 * W
    lines = b"".join(b"\x00" + raw[y * row:(y + 1) * row] for y in range(H))
    png = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 16, 2, 0, 0, 0))
           + _chunk(b"IDAT", zlib.compress(lines, level)) + _chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)
