"""What the frame_resize tests share: the resampling geometry restated with Python integers, the CPU references and the
shapes.  Nothing here touches the library.

Yardsticks: bilinear - torch's F.interpolate(align_corners=False) in float64 (its float32 route is up to 6e-4 levels away from
float64 because of its float coordinates, so it is no yardstick); area - the integer windows of F.interpolate(mode="area")
with float32(sum) / float32(count), which is bit-defined."""
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

# (N, H, W) -> (h, w): a non-integer reduction with N > 1; an enlargement (negative numerators, clamped borders); w % 4 != 0;
# one pixel; an enlargement by non-integer factors
BILINEAR_CASES = (((2, 13, 19), (8, 12)), ((1, 7, 5), (16, 24)), ((1, 21, 37), (10, 18)), ((1, 1, 1), (8, 8)), ((1, 5, 6), (17, 23)))
AREA_CASES = (((2, 13, 19), (8, 12)), ((1, 20, 30), (4, 7)), ((1, 16, 32), (8, 16)))
PADS = ((0, 0, 0, 0), (1, 2, 3, 4))


def taps(n_in, n_out):
    """Per output index: (a, b, f) - the clamped taps and the weight of b as an exact Fraction (half-pixel centres)."""
    out = []
    for x in range(n_out):
        num, den = (2 * x + 1) * n_in - n_out, 2 * n_out
        i0 = num // den                                     # (Python's // is the floor division)
        out.append((min(max(i0, 0), n_in - 1), min(max(i0 + 1, 0), n_in - 1), Fraction(num - i0 * den, den)))
    return out


def bilinear_f64(x, size):
    """(N,C,H,W) of any dtype -> float64 (N,C,h,w)."""
    return F.interpolate(x.double(), size=tuple(size), mode="bilinear", align_corners=False)


def levels(hwc, bgr=False):
    """uint8 (N,H,W,3) -> (N,3,H,W) uint8 in the channel order the model is handed."""
    x = hwc.permute(0, 3, 1, 2)
    return x.flip(1) if bgr else x


def area_windows(n_in, n_out):
    return [(y * n_in // n_out, -((-(y + 1) * n_in) // n_out)) for y in range(n_out)]


def area_reference(hwc, size, bgr=False, normalize=True):
    """float32 (N,3,h,w): integer window sums, float32(sum) / float32(count), then torch's 2 * (x / 255.0) - 1 in float32."""
    x = levels(hwc, bgr).numpy().astype(np.int64)
    h, w = size
    rows, cols = area_windows(x.shape[2], h), area_windows(x.shape[3], w)
    out = np.zeros(x.shape[:2] + (h, w), dtype=np.float32)
    for y, (r0, r1) in enumerate(rows):
        for xx, (c0, c1) in enumerate(cols):
            s = x[:, :, r0:r1, c0:c1].sum(axis=(2, 3))
            out[:, :, y, xx] = s.astype(np.float32) / np.float32((r1 - r0) * (c1 - c0))
    t = torch.from_numpy(out)
    return 2 * (t / 255.0) - 1 if normalize else t


def tap_bound(win, size):
    """For a float (N,C,Hc,Wc) window and an output size: per output pixel the largest |tap| among its four taps (N,C,h,w), in
    float64 - what the relative error bound of a resized flow is stated in."""
    a = win.double().abs()
    ty, tx = taps(a.shape[2], size[0]), taps(a.shape[3], size[1])
    ya, yb = torch.tensor([t[0] for t in ty]), torch.tensor([t[1] for t in ty])
    xa, xb = torch.tensor([t[0] for t in tx]), torch.tensor([t[1] for t in tx])
    m = torch.maximum(a[:, :, ya], a[:, :, yb])
    return torch.maximum(m[:, :, :, xa], m[:, :, :, xb])


def touched(n_in, n_out, src):
    """The output indices whose non-zero-weight taps include source index `src`."""
    return [i for i, (a, b, f) in enumerate(taps(n_in, n_out)) if a == src or (b == src and f != 0)]
