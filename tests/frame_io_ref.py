"""What the frame_io tests share: a PNG encoder with a chosen scanline filter and a PNG decoder for depth 8 and 16, both
written from the PNG specification for the tests alone (the product's decoder, accflow_amd.frames.read_image, is what they
check), the ingest cases and the CPU references.  Nothing here touches the library."""
import struct
import zlib

import numpy as np
import torch
import torch.nn.functional as F

FILTERS = {"None": 0, "Sub": 1, "Up": 2, "Average": 3, "Paeth": 4}
COLOUR = {1: 0, 3: 2, 4: 6}        # channels -> PNG colour type

# (N, H, W) of the ingest cases: no pad; replicate from one pixel; pads 3 and 3 (sintel 1/2, kitti bottom); width pad 0 left
# 1 right and W % 4 != 0; the interior fast path with a 7-row pad
INGEST_SHAPES = ((1, 8, 8), (1, 1, 1), (2, 13, 21), (1, 16, 31), (3, 9, 40))


def _predict(f, a, b, c):
    if f == 0:
        return 0
    if f == 1:
        return a
    if f == 2:
        return b
    if f == 3:
        return (a + b) // 2
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)


def encode_png(img, filt, interlace=0, depth=8, idat_split=None):
    """img: (H,W,C) uint8 (depth 8) or uint16 (depth 16), C in 1, 3, 4; filt: one filter type for every row or a list with one
    per row.  interlace is written into the header only (the tests need a file that SAYS it is interlaced)."""
    H, W, C = img.shape
    rows = img.astype(">u2").view(np.uint8).reshape(H, -1) if depth == 16 else img.reshape(H, -1)
    bpp = C * depth // 8
    filts = [filt] * H if isinstance(filt, int) else list(filt)
    lines = b""
    for y in range(H):
        cur = rows[y].astype(np.int64).tolist()
        up = rows[y - 1].astype(np.int64).tolist() if y else [0] * len(cur)
        out = []
        for i, x in enumerate(cur):
            a = cur[i - bpp] if i >= bpp else 0
            c = up[i - bpp] if i >= bpp else 0
            out.append((x - _predict(filts[y], a, up[i], c)) & 255)
        lines += bytes([filts[y]]) + bytes(out)
    z = zlib.compress(lines, 6)
    parts = [z] if not idat_split else [z[:idat_split], z[idat_split:]]
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, COLOUR[C], 0, 0, interlace))
            + b"".join(chunk(b"IDAT", p) for p in parts) + chunk(b"IEND", b""))


def decode_png(data):
    """Non-interlaced, depth 8 or 16, gray / RGB / RGBA -> ((H,W,C) uint8 or uint16 in native order, the rows' filter types)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        pos += 12 + n
    assert pos == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert depth in (8, 16) and colour in (0, 2, 6) and (comp, filt, lace) == (0, 0, 0)
    C = {0: 1, 2: 3, 6: 4}[colour]
    bpp = C * depth // 8
    row = W * bpp
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    assert len(raw) == H * (row + 1)
    out, filters = np.zeros((H, row), dtype=np.uint8), []
    for y in range(H):
        f, line = raw[y * (row + 1)], raw[y * (row + 1) + 1:(y + 1) * (row + 1)]
        filters.append(f)
        up = out[y - 1].tolist() if y else [0] * row
        cur = [0] * row
        for i in range(row):
            a = cur[i - bpp] if i >= bpp else 0
            c = up[i - bpp] if i >= bpp else 0
            cur[i] = (line[i] + _predict(f, a, up[i], c)) & 255
        out[y] = cur
    if depth == 16:
        return out.view(">u2").astype(np.uint16).reshape(H, W, C), filters
    return out.reshape(H, W, C), filters


def ingest_bytes(N, H, W, seed):
    """uint8 (N,H,W,3): every sample starts with the bytes 0..255 in order (as far as it is long), then seeded random bytes."""
    g = np.random.default_rng(seed)
    x = g.integers(0, 256, (N, H * W * 3), dtype=np.uint8)
    k = min(256, H * W * 3)
    x[:, :k] = np.arange(k, dtype=np.uint8)
    return torch.from_numpy(x.reshape(N, H, W, 3))


def all_codes_frame():
    """(1,8,32,3): each channel holds all 256 codes, in three different orders."""
    a = np.arange(256, dtype=np.uint8)
    return torch.from_numpy(np.stack([a, a[::-1], np.roll(a, 77)], axis=-1).reshape(1, 8, 32, 3).copy())


def ingest_reference(hwc, pad, bgr=False, normalize=True):
    """The CPU reference: F.pad(2 * (x.float() / 255.0) - 1, pad, mode="replicate") on (N,3,H,W); hwc: uint8 (N,H,W,3)."""
    x = hwc.permute(0, 3, 1, 2)
    if bgr:
        x = x.flip(1)
    x = x.float()
    if normalize:
        x = 2 * (x / 255.0) - 1
    return F.pad(x, list(pad), mode="replicate")


def u16_reference(flow, crop, scale, big_endian):
    """numpy in float32: (N,2,Hp,Wp) ndarray -> uint16 (N,H,W,3), the samples in native or swapped byte order."""
    y0, x0, H, W = crop
    f = np.ascontiguousarray(flow[:, :, y0:y0 + H, x0:x0 + W].transpose(0, 2, 3, 1))
    fin = np.isfinite(f)
    with np.errstate(invalid="ignore", over="ignore"):                 # (64 * 3e38 is inf in float32 too, and clips to 65535)
        code = np.trunc(np.clip(np.float32(scale) * np.where(fin, f, np.float32(0)) + np.float32(32768), 0, 65535))
    assert code.dtype == np.float32
    code = np.where(fin, code, 0).astype(np.uint16)
    out = np.concatenate([code, fin.all(axis=-1, keepdims=True).astype(np.uint16)], axis=-1)
    return out.byteswap() if big_endian else out
