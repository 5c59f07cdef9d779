"""The Middlebury colour coding restated in float64 from its definition, the comparison rule of the flow_viz tests, and the
input recipes they share with tests/golden/make_flow_viz_golden.py, and a PNG decoder.  Nothing here touches the library.

Definition.  wheel: 55 entries, segments RY 15, YG 6, GC 4, CB 11, BM 13, MR 6, ramps floor(255 k / n).  For (u, v) = flow /
(s + 1e-5):  rad = |(u, v)|, fk = (atan2(-v, -u) / pi + 1) / 2 * 54, k0 = floor(fk), k1 = (k0 + 1) mod 55, f = fk - k0,
col = c0 + f (c1 - c0) with c = wheel / 255, then col = 1 - rad (1 - col) where rad <= 1 and 0.75 col elsewhere; the byte is
floor(255 col).  The divisor s + 1e-5 is the float32 sum (what the kernel and numpy's float32 both form); everything after it
is float64 here.

Rule (derived, not measured).  x = 255 col in float64.  Where x is an integer the byte must be x (the saturated channel, white,
black).  Where 0 < |x - round(x)| <= TAU = 5e-3 the byte may be round(x) or round(x) - 1.  Everywhere else it must be floor(x).
TAU is five times a bound of 1e-3: atan2f within a few ulp of pi puts the angle a off by ~5e-7, fk by ~1.4e-5 (plus float32
fk's own 2e-6), the steepest wheel step is 64/255 per index, so col is off by ~4e-6 and x by ~1e-3.  A pixel whose float64
rad lies within 2^-22 of 1 may take either brightness branch.  Both escapes are capped by the callers BEFORE an output is
looked at: at most 1.5 % of a case's components in the TAU band, at most one rad-1 pixel per image."""
import struct
import zlib

import numpy as np

TAU = 5e-3
RAD_BAND = 2.0 ** -22
MAX_BAND_SHARE = 0.015
UNKNOWN = 1e9


def make_wheel():
    segs = ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True), (6, 0, 2, False))
    rows = []
    for n, full, ramp, rising in segs:
        for k in range(n):
            row = [0, 0, 0]
            row[full] = 255
            row[ramp] = (255 * k) // n if rising else 255 - (255 * k) // n
            rows.append(row)
    wheel = np.array(rows, dtype=np.float64)
    assert wheel.shape == (55, 3)
    return wheel


WHEEL = make_wheel()


def clip32(flow, clip):
    """np.clip(flow, 0, clip) in float32, the reference's clip_flow (None: the flow itself)."""
    flow = np.asarray(flow, dtype=np.float32)
    return flow if clip is None else np.clip(flow, np.float32(0), np.float32(clip))


def unknown(flow):
    """(H,W) mask of a (2,H,W) flow: a component that is NaN, infinite or beyond 1e9."""
    with np.errstate(invalid="ignore"):
        return ~(np.abs(flow) <= UNKNOWN).all(axis=0)


def max_radius32(flow, clip=None):
    """max sqrt(u*u + v*v) over the valid pixels of a (2,H,W) flow, every operation in float32; 0 without a valid pixel."""
    flow = clip32(flow, clip)
    ok = ~unknown(flow)
    if not ok.any():
        return np.float32(0)
    u, v = flow[0][ok], flow[1][ok]
    return np.max(np.sqrt(np.square(u) + np.square(v)))


def colours64(flow, scale, clip=None):
    """flow (2,H,W) float32, scale: the float32 s -> (x_in, x_out, rad, unknown): x = 255 col (H,W,3) float64 by the rad <= 1
    formula and by the 0.75 formula, rad (H,W) float64, the unknown mask (x is 0 there)."""
    flow = clip32(flow, clip)
    bad = unknown(flow)
    d = np.float64(np.float32(scale) + np.float32(1e-5))
    with np.errstate(all="ignore"):
        u, v = flow[0].astype(np.float64) / d, flow[1].astype(np.float64) / d
        rad = np.sqrt(u * u + v * v)
        fk = (np.arctan2(-v, -u) / np.pi + 1.0) / 2.0 * 54.0
    fk, rad = np.where(bad, 0.0, fk), np.where(bad, 0.0, rad)
    k0 = np.minimum(np.floor(fk), 54).astype(np.int64)
    k1 = (k0 + 1) % 55
    f = (fk - k0)[..., None]
    c0, c1 = WHEEL[k0] / 255.0, WHEEL[k1] / 255.0
    col = c0 + f * (c1 - c0)
    x_in = 255.0 * (1.0 - rad[..., None] * (1.0 - col))
    x_out = 255.0 * (0.75 * col)
    x_in[bad] = 0.0
    x_out[bad] = 0.0
    return x_in, x_out, rad, bad


def _allowed(x):
    """(lo, hi, band): the bytes lo..hi are accepted for x; band marks the components inside the TAU band."""
    r = np.round(x)
    dist = np.abs(x - r)
    band = (dist > 0) & (dist <= TAU)
    fl = np.floor(x)
    lo = np.clip(np.where(band, r - 1, fl), 0, 255)
    hi = np.clip(np.where(band, r, fl), 0, 255)
    # (0 < x <= TAU leaves the byte 0 alone - the zero channel of the pixel that sets the scale, x = 255 * 1e-5 / (s + 1e-5),
    # is always there: no choice, so it does not count as a band component)
    return lo, hi, band & (lo != hi)


def expectation(flow, scale, clip=None):
    """What the rule accepts for one image: dict with lo / hi (H,W,3) for the pixel's own branch, lo2 / hi2 for the other
    branch where rad is within RAD_BAND of 1 (elsewhere equal to lo / hi), band (H,W,3), near_one (H,W), x (H,W,3)."""
    x_in, x_out, rad, bad = colours64(flow, scale, clip)
    inside = rad <= 1.0
    x = np.where(inside[..., None], x_in, x_out)
    other = np.where(inside[..., None], x_out, x_in)
    near_one = (np.abs(rad - 1.0) < RAD_BAND) & ~bad
    lo, hi, band = _allowed(x)
    lo2, hi2, band2 = _allowed(other)
    sel = near_one[..., None]
    return {"lo": lo, "hi": hi, "lo2": np.where(sel, lo2, lo), "hi2": np.where(sel, hi2, hi), "band": band,
            "near_one": near_one, "x": x, "unknown": bad}


def check_image(img, flow, scale, clip=None, bgr=False, exact=False, caps=True, what=""):
    """Assert the rule for img (H,W,3) uint8 against flow (2,H,W) at the float32 scale.  exact: the case must have no
    component in the TAU band and no rad-1 pixel (tiny shapes), so the comparison is with floor(x) alone.  caps=False is for
    hand-made inputs of a few pixels (a share of them means nothing); generated cases keep the caps.  Returns
    (components in the band, rad-1 pixels, worst |x - round(x)| among components that differ from floor(x))."""
    e = expectation(flow, scale, clip)
    n_band, n_one = int(e["band"].sum()), int(e["near_one"].sum())
    # the caps come first: they are properties of the input, not of the output under test
    if caps or exact:
        assert n_band <= (0 if exact else MAX_BAND_SHARE * e["band"].size), (what, "components in the tau band", n_band, e["band"].size)
        assert n_one <= (0 if exact else 1), (what, "pixels with |rad - 1| < 2^-22", n_one)
    got = np.asarray(img)
    assert got.dtype == np.uint8 and got.shape == e["x"].shape, (what, got.dtype, got.shape)
    got = got[..., ::-1] if bgr else got
    g = got.astype(np.float64)
    ok = ((g >= e["lo"]) & (g <= e["hi"])) | ((g >= e["lo2"]) & (g <= e["hi2"]))
    if not ok.all():
        y, xx, c = [int(t[0]) for t in np.nonzero(~ok)]
        raise AssertionError("%s: %d components outside the rule; first at (%d,%d) channel %d: got %d, 255 col = %.6f, flow (%r, %r), "
                             "scale %r" % (what, int((~ok).sum()), y, xx, c, got[y, xx, c], e["x"][y, xx, c], float(flow[0, y, xx]),
                                           float(flow[1, y, xx]), float(scale)))
    differ = (g != np.floor(e["x"])) & ~e["near_one"][..., None]
    worst = float(np.abs(e["x"] - np.round(e["x"]))[differ].max()) if differ.any() else 0.0
    return n_band, n_one, worst


# ---- input recipes (torch on the CPU: the same bits wherever they are drawn) ----

def off_the_seam(flow):
    """Keep a non-zero |v| at least 1e-3 |u|, so that only exact signed zeros sit on the colour seam (u > 0, v = +-0)."""
    import torch
    u, v = flow[..., 0:1, :, :], flow[..., 1:2, :, :]
    small = (v != 0) & (v.abs() < 1e-3 * u.abs())
    v = torch.where(small, torch.copysign(2e-3 * u.abs(), v), v)
    return torch.cat([u, v], dim=-3).contiguous()


def smooth_flow(B, H, W, seed):
    """interpolate(8 randn(B, 2, 3, 4)) to (H, W)."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    t = 8 * torch.randn(B, 2, 3, 4, generator=g)
    return off_the_seam(F.interpolate(t, size=(H, W), mode="bilinear", align_corners=True))


def noise_flow(B, H, W, seed):
    """5 randn."""
    import torch
    g = torch.Generator().manual_seed(seed)
    return off_the_seam(5 * torch.randn(B, 2, H, W, generator=g))


# ---- a PNG decoder for what viz.write_png writes (and for any other 8-bit RGB, non-interlaced file) ----

def decode_png(data):
    """8-bit RGB, non-interlaced: chunks with their CRCs, one inflate over all IDAT chunks, all five scanline filters."""
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
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    row = 3 * W
    assert len(raw) == H * (row + 1)
    out = np.zeros((H, row), dtype=np.uint8)
    filters = []
    for y in range(H):
        f, line = raw[y * (row + 1)], np.frombuffer(raw, np.uint8, row, y * (row + 1) + 1).astype(np.int64)
        filters.append(f)
        up = out[y - 1].astype(np.int64) if y else np.zeros(row, np.int64)
        cur = np.zeros(row, np.int64)
        for i in range(row):
            a = cur[i - 3] if i >= 3 else 0
            b, c = up[i], (up[i - 3] if i >= 3 else 0)
            if f == 0:
                pred = 0
            elif f == 1:
                pred = a
            elif f == 2:
                pred = b
            elif f == 3:
                pred = (a + b) // 2
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            cur[i] = (line[i] + pred) & 255
        out[y] = cur
    return out.reshape(H, W, 3), filters
