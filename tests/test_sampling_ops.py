"""The gather-type kernels (csrc/sampling.hip: backwarp / compose_flow, getOcc, convex upsampling, downflow8, the deformable
columns) and the element-wise / S16-producing half of csrc/misc.hip (blend, flow_from_coords, the instance-norm apply passes,
the indexed tanh / relu split) against float64 references written HERE, on every branch the host code takes by size, on
batch-strided operands, and on both sides of the S16 range guard.

References.  A sample position is formed in float32 exactly as the kernel forms it (x + u; for downflow8 the float32 scale
times the index) and clamped to +-1e6 as make_taps does; everything after that is float64.  So the only difference
between kernel and reference is the rounding of the interpolation itself, and every bound below is a COUNT OF ROUNDINGS
times eps = 2^-24 times the magnitude the rounding happens at - none is taken from what the kernels give.  MARGIN = 2
covers associations other than the one counted (the compiler may contract to FMAs, which only removes roundings).

    bilinear (backwarp, compose, getOcc, downflow8), K_BILINEAR = 8: ax = sx - floor(sx) is exact; 1 - ax, 1 - ay: one
      rounding each; their product: one (a weight carries <= 3); weight * value: one (<= 4 on a term); three additions at
      partial sums <= max|plane| (the weights sum to <= 1): 3; that is 7, + 1 for second-order terms.
    error map: + 1 for I1 - warp at a magnitude <= max|I1| + max|I2|.
    binary map: the thresholded mean of C terms, each <= M = max|I1| + max|I2| and each carrying (K_BILINEAR + 1) eps M;
      C - 1 additions and the division by C at a mean of ~1: the bit may differ from err64 <= 1 only where
      |err64 - 1| <= (C + K_OCC * M) eps, K_OCC = 9 (the issue's (C + k) 2^-24 with the image magnitude written out).
    convex upsampling: m - max rounds once at a magnitude <= s (the spread of the 9 logits): a relative s eps on exp(),
      whose own error is <= 1 ulp = 2 eps; the same again for the denominator, + 8 additions + 1 division: (13 + 2 s) on a
      weight; weight * 8 flow: 1; 8 additions at partial sums <= 8 max|flow|: (K_UP + C_UP s) eps 8 max|flow| with K_UP = 22,
      C_UP = 2.
    deformable columns, K_COL = 12: uh = 1 - lh, uw = 1 - lw: one each; uh * uw * v: two more (4 on a term); 3 additions;
      the modulation: 1, and 4 for the sigmoid when the kernel applies it.
    S16 (hi + lo of 16 x): hi has 11 bits, the remainder is exact in fp32 and lo keeps 11 bits of it: 2^-22 |x|, plus fp16's
      subnormal spacing 2^-25 / 16 = 2^-29 where lo underflows.
"""
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import accflow_oracle as O

gpu = pytest.mark.gpu
T = torch.from_numpy
EPS = 2.0 ** -24
MARGIN = 2.0
K_BILINEAR, K_OCC, K_UP, C_UP, K_COL = 8, 9, 22, 2, 12
# A deformable convolution whose weights pick ONE column per (output, tap) with weight 1 (perm_weight): 9 non-zero terms.
# Per term: the column (K_COL) + its S16 split (2^-22 = 4 eps) + the weight's split (4) + the dropped lo * lo product (4);
# up to 27 non-zero fp16 products are added in fp32 at partial sums <= 9 max|column|, through up to 4 split-K partial sums
# (another 4): 31; the pre-split output: 4.
K_DCONV = K_COL + 4 + 4 + 4 + 31 + 4
S16_REL, S16_ABS = 2.0 ** -22, 2.0 ** -29
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def dev(t):
    return t.cuda()


def grid32(H, W):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return xs, ys


# ------------------------------------------------------------------------------------------------
# float64 references


def clamp_like_make_taps(s):
    """fminf(fmaxf(s, -1e6), 1e6): IEEE fmaxf drops a NaN operand, so NaN becomes -1e6 (a sample far outside: 0)."""
    return torch.nan_to_num(s, nan=-1.0e6, posinf=1.0e6, neginf=-1.0e6).clamp(-1.0e6, 1.0e6)


def gather0(planes, yy, xx):
    """planes (B, C, H, W), integer yy / xx (B, h, w) -> planes[b, c, yy, xx], 0 where the index leaves the plane."""
    B, C, H, W = planes.shape
    ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(B, 1, -1).expand(B, C, -1)
    v = planes.reshape(B, C, H * W).gather(2, idx).reshape(B, C, *yy.shape[1:])
    return torch.where(ok[:, None], v, torch.zeros_like(v))


def bilinear64(planes, sx, sy):
    """Zero-padded bilinear samples of float64 planes (B, C, H, W) at positions (B, h, w) (any float type, taken as given)."""
    sx, sy = sx.double(), sy.double()
    x0, y0 = torch.floor(sx), torch.floor(sy)
    ax, ay = sx - x0, sy - y0
    x0, y0 = x0.long(), y0.long()
    out = ((1 - ax) * (1 - ay))[:, None] * gather0(planes, y0, x0)
    out = out + (ax * (1 - ay))[:, None] * gather0(planes, y0, x0 + 1)
    out = out + ((1 - ax) * ay)[:, None] * gather0(planes, y0 + 1, x0)
    return out + (ax * ay)[:, None] * gather0(planes, y0 + 1, x0 + 1)


def warp64(img, flow):
    """backwarp: img sampled at (x + u, y + v), positions in float32 as backwarp_kernel forms them."""
    xs, ys = grid32(*img.shape[2:])
    sx, sy = clamp_like_make_taps(xs[None] + flow[:, 0].float()), clamp_like_make_taps(ys[None] + flow[:, 1].float())
    return bilinear64(img.double(), sx, sy)


def compose64(step, acc):
    return step.double() + warp64(acc, step)


def err_map64(flow, i1, i2):
    return (i1.double() - warp64(i2, flow)).abs()


def occ_err64(flow, i1, i2):
    return err_map64(flow, i1, i2).mean(dim=1, keepdim=True)


def convex_upsample64(flow, mask):
    N, _, H, W = flow.shape
    w = torch.softmax(mask.double().reshape(N, 9, 64, H, W), dim=1)
    f = F.pad(8.0 * flow.double(), (1, 1, 1, 1))
    out = torch.zeros(N, 2, 64, H, W, dtype=torch.float64)
    for k in range(9):
        out += w[:, k][:, None] * f[:, :, k // 3:k // 3 + H, k % 3:k % 3 + W][:, :, None]
    return out.reshape(N, 2, 8, 8, H, W).permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * H, 8 * W)


def downflow8_64(flow, pos=torch.float32):
    """Bilinear resize to (H/8, W/8) with aligned corners, / 8.  pos = float32, as the compiled downflow8_kernel forms the
    position: the scale is a float32 quotient, the source index is the integer part of the float32 product scale * index, and
    the fraction `sy - (float)y0` is contracted with that product into one fma (hipcc's default, -ffp-contract=fast): the
    EXACT product minus the index, rounded once.  A product rounded first (the fp32 oracle; a build without contraction) moves
    the sample by up to half an ulp of the position - 3e-5 px at 1 000 px, hundreds of times the interpolation's own rounding
    on a noise field: measured 2026-10-16, 29x / 57x the bound at 480 x 1024 / 720 x 1280 against that form, 0.07x / 0.15x
    against this one.  pos = float64: everything in float64 (the form F.interpolate evaluates)."""
    N, C, H, W = flow.shape
    h, w = H // 8, W // 8

    def axis(n_out, n_in):
        if n_out == 1:
            return torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.float64)
        scale = torch.tensor(n_in - 1, dtype=pos) / torch.tensor(n_out - 1, dtype=pos)
        exact = scale.double() * torch.arange(n_out, dtype=torch.float64)     # (24 x 11 bits: exact in float64)
        i0 = exact.to(pos).long()
        return i0, (exact - i0).to(pos).double()
    (y0, ly), (x0, lx) = axis(h, H), axis(w, W)
    y1, x1 = torch.where(y0 < H - 1, y0 + 1, y0), torch.where(x0 < W - 1, x0 + 1, x0)
    ly, lx = ly[:, None], lx[None, :]
    f = flow.double()
    top = (1 - lx) * f[:, :, y0][:, :, :, x0] + lx * f[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * f[:, :, y1][:, :, :, x0] + lx * f[:, :, y1][:, :, :, x1]
    return ((1 - ly) * top + ly * bot) / 8


def deform_tap64(x, offset, mask, t, KH=3, KW=3, pad=1):
    """Tap t of the deformed im2col columns, (B, C, H, W) float64.  torchvision's boundary rule as written above
    deform_columns_kernel: the sample is 0 when h <= -1, h >= H, w <= -1 or w >= W, corners outside contribute 0."""
    B, C, H, W = x.shape
    xs, ys = grid32(H, W)
    h = (ys + float(t // KW - pad))[None] + offset[:, 2 * t].float()
    w = (xs + float(t % KW - pad))[None] + offset[:, 2 * t + 1].float()
    inside = (h > -1) & (h < H) & (w > -1) & (w < W)
    v = bilinear64(x.double(), torch.where(inside, w, torch.zeros_like(w)), torch.where(inside, h, torch.zeros_like(h)))
    return torch.where(inside[:, None], v, torch.zeros_like(v)) * mask[:, t].double()[:, None]


def deform_columns64(x, offset, mask):
    """(B, 9 * C, H, W), column tap * C + c."""
    return torch.cat([deform_tap64(x, offset, mask, t) for t in range(9)], dim=1)


def deform_conv64(x, offset, mask, weight, bias=None):
    out = 0
    for t in range(9):
        out = out + torch.einsum("oc,bchw->bohw", weight[:, :, t // 3, t % 3].double(), deform_tap64(x, offset, mask, t))
    return out if bias is None else out + bias.double().view(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------------
# the host's size arithmetic, restated; test_host_thresholds_are_the_ones_restated_here pins it to the sources

WARP_CCHUNK = 16
OCC_SMALL_BELOW = 1 << 17
SPLIT_ITEMS_PER_LAUNCH = 64


def warp_chunks(C):
    return -(-C // WARP_CCHUNK)


def occ_branch(B, H, W):
    return "binary4" if B * H * W < OCC_SMALL_BELOW else "per-pixel"


def deform_chunks(C, B, H, W):
    n = B * 9 * H * W
    return (8 if C >= 64 else 1) if n < (1 << 18) else (2 if n < (1 << 20) else 1)


def deform_presplit(C):
    return C % 8 == 0 and (9 * C) % 32 == 0


def test_host_thresholds_are_the_ones_restated_here():
    """The branch every GPU case asserts comes from the functions above; they are the host code's only while these lines
    stand in the sources, so a changed threshold fails here instead of moving the coverage silently."""
    src = open(os.path.join(ROOT, "accflow_amd", "csrc", "sampling.hip")).read()
    assert "constexpr int WARP_CCHUNK = 16;" in src
    assert src.count("if (binary && np < (1 << 17))") == 2                     # accflow_get_occ_f32 and _s16
    assert src.count("const int chunks = n < (1 << 18) ? (C >= 64 ? 8 : 1) : (n < (1 << 20) ? 2 : 1);") == 2
    assert src.count("const int cper = (C + 3) / 4") == 3                       # the three binary kernels
    assert len(re.findall(r"cdiv\(C, WARP_CCHUNK\)", src)) == 2 and "cdiv(C, 8)" in src
    assert "const float sy_scale = H8 > 1 ?" in src and "const float sx_scale = W8 > 1 ?" in src
    misc = open(os.path.join(ROOT, "accflow_amd", "csrc", "misc.hip")).read()
    assert "struct split_idx { int v[64]; };" in misc and "for (int b0 = 0; b0 < B; b0 += 64)" in misc
    py = open(os.path.join(ROOT, "accflow_amd", "ops.py")).read()
    assert "if USE_DEFORM_S16_COLUMNS and C % 8 == 0 and (pk.KH * pk.KW * C) % 32 == 0:" in py


# ------------------------------------------------------------------------------------------------
# seeded inputs (shared by the CPU condition checks and the GPU cases)

FLOW_KINDS = ("smooth", "noise", "int", "border", "wild")


def make_flow(kind, B, H, W, seed):
    g = gen(seed)
    xs, ys = grid32(H, W)
    if kind == "smooth":
        f = torch.stack([3 * torch.sin(xs / 9 + 0.3) + ys / 20, 2 * torch.cos(ys / 7) - xs / 30])[None]
        return (f * torch.linspace(1.0, 1.7, B).view(B, 1, 1, 1)).contiguous()
    if kind == "noise":
        return torch.randn(B, 2, H, W, generator=g) * 4
    if kind == "int":
        return torch.randint(-3, 4, (B, 2, H, W), generator=g).float()
    if kind == "border":       # every source lands exactly on -1, 0, the last column / row, or one past it
        tx = torch.tensor([-1.0, 0.0, W - 1.0, float(W)])[((xs + ys) % 4).long()]
        ty = torch.tensor([-1.0, 0.0, H - 1.0, float(H)])[((xs // 4 + ys) % 4).long()]
        return torch.stack([tx - xs, ty - ys])[None].repeat(B, 1, 1, 1)
    assert kind == "wild"      # what the clamp in make_taps is for
    f = torch.randn(B, 2, H, W, generator=g) * 4
    v = f.view(-1)
    for j, bad in enumerate((1.0e9, -1.0e9, float("inf"), float("-inf"), float("nan"))):
        v[j::7] = bad if v.numel() < 40 else v[j::7]
        v[3 * j + 1::41] = bad
    return f


WARP_CASES = [
    # C, B, H, W, flow, channel chunks
    (1, 2, 1, 1, "wild", 1),
    (2, 2, 1, 19, "border", 1),
    (15, 2, 20, 28, "noise", 1),
    (16, 2, 37, 53, "int", 1),
    (17, 2, 20, 28, "border", 2),
    (37, 2, 20, 28, "wild", 3),
    (128, 1, 60, 128, "smooth", 8),
    (16, 20, 60, 128, "noise", 1),
    (17, 1, 90, 160, "wild", 2),
    (2, 20, 90, 160, "smooth", 1),
    (3, 1, 480, 1024, "noise", 1),
]
COMPOSE_CASES = [
    # B, H, W, flow
    (2, 1, 1, "wild"), (2, 1, 19, "border"), (2, 20, 28, "noise"), (2, 37, 53, "int"), (1, 60, 128, "smooth"),
    (20, 60, 128, "wild"), (1, 90, 160, "border"), (20, 90, 160, "noise"), (1, 480, 1024, "smooth"),
]


def test_warp_cases_cover_the_table():
    assert {c[0] for c in WARP_CASES} >= {1, 2, 15, 16, 17, 37, 128}
    for shapes in ({c[2:4] for c in WARP_CASES}, {c[1:3] for c in COMPOSE_CASES}):
        assert shapes >= {(1, 1), (1, 19), (20, 28), (37, 53), (60, 128), (90, 160), (480, 1024)}
    for cases, b, hw in ((WARP_CASES, 1, slice(2, 4)), (COMPOSE_CASES, 0, slice(1, 3))):
        assert {(c[b], c[hw]) for c in cases} >= {(1, (60, 128)), (20, (60, 128)), (1, (90, 160)), (20, (90, 160))}
    assert {c[4] for c in WARP_CASES} == set(FLOW_KINDS) == {c[3] for c in COMPOSE_CASES}
    assert all(warp_chunks(c[0]) == c[5] for c in WARP_CASES)


OCC_CASES = [
    # C, B, H, W, branch of the binary form
    (1, 2, 20, 28, "binary4"), (2, 2, 20, 28, "binary4"), (3, 1, 37, 53, "binary4"), (5, 2, 20, 28, "binary4"),
    (24, 1, 60, 128, "binary4"), (37, 2, 20, 28, "binary4"), (128, 1, 60, 128, "binary4"),
    (1, 20, 60, 128, "per-pixel"), (2, 20, 60, 128, "per-pixel"), (3, 20, 60, 128, "per-pixel"),
    (5, 20, 60, 128, "per-pixel"), (24, 20, 60, 128, "per-pixel"), (37, 20, 60, 128, "per-pixel"),
]
OCC_BATCH_CASE = (128, 20, 60, 128, (0, 19))     # one item alone (binary4) against the same item inside the batch (per-pixel)


@functools.lru_cache(maxsize=2)
def occ_inputs(C, B, H, W, items=None):
    """flow, I1, I2 with the images scaled so that the threshold of 1 sits at the median of the float64 error (both classes
    present); items: the float64 error is evaluated for these batch items only (the C = 128 batch of 20)."""
    g = gen(4000 + 16 * C + B)
    i1, i2 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    flow = torch.randn(B, 2, H, W, generator=g) * 3
    sel = list(range(B)) if items is None else list(items)
    s = 1.0 / float(occ_err64(flow[sel], i1[sel], i2[sel]).median())
    return flow, i1 * s, i2 * s


def occ_band(C, i1, i2):
    return MARGIN * (C + K_OCC * (float(i1.abs().max()) + float(i2.abs().max()))) * EPS


@pytest.mark.parametrize("case", OCC_CASES + [OCC_BATCH_CASE])
def test_occlusion_inputs_meet_the_conditions(case):
    """From the float64 reference alone: at most 0.1 % of a case's pixels lie where the fp32 sum may legitimately give the
    other bit, and each class holds at least 20 %."""
    C, B, H, W, last = case
    items = last if isinstance(last, tuple) else None
    flow, i1, i2 = occ_inputs(C, B, H, W, items)
    sel = list(range(B)) if items is None else list(items)
    e = occ_err64(flow[sel], i1[sel], i2[sel])
    assert float(((e - 1.0).abs() <= occ_band(C, i1, i2)).double().mean()) <= 1e-3
    assert 0.2 <= float((e <= 1.0).double().mean()) <= 0.8
    if items is None:
        assert occ_branch(B, H, W) == last
    else:
        assert occ_branch(B, H, W) == "per-pixel" and occ_branch(1, H, W) == "binary4"


def test_occ_cases_cover_the_table():
    for br in ("binary4", "per-pixel"):
        cs = {c[0] for c in OCC_CASES if c[4] == br}
        assert cs >= {1, 2, 3, 5, 24, 37} and any(c < 4 for c in cs) and any(c % 4 for c in cs if c > 4)
    assert 128 in {c[0] for c in OCC_CASES} and OCC_BATCH_CASE[0] == 128


def straddle_inputs(C, B, H, W):
    """Zero flow, I2 = 0 and I1 = 1 + k 2^-23 with small integers k: every |I1 - warp(I2)| is I1 exactly, the float64 mean
    sits within a few 2^-23 of the threshold everywhere, and the bit depends on how the fp32 sum is associated."""
    k = torch.randint(-6, 7, (B, C, H, W), generator=gen(8000 + C))
    return torch.zeros(B, 2, H, W), 1.0 + k.float() * 2.0 ** -23, torch.zeros(B, C, H, W)


def quarter_sum_bits32(i1, pairs=True):
    """The binary kernels' sum restated in fp32: four quarter sums over cper = ceil(C / 4) channels each, in channel order,
    added as (q0 + q1) + (q2 + q3); pairs=False: ((q0 + q1) + q2) + q3, another association of the same terms."""
    C = i1.shape[1]
    cper = (C + 3) // 4
    q = []
    for kq in range(4):
        acc = torch.zeros_like(i1[:, 0])
        for c in range(kq * cper, min(C, (kq + 1) * cper)):
            acc = acc + i1[:, c]
        q.append(acc)
    tot = (q[0] + q[1]) + (q[2] + q[3]) if pairs else ((q[0] + q[1]) + q[2]) + q[3]
    return (tot / float(C) <= 1.0).float()[:, None]


STRADDLE_CASES = [(4, 20, 60, 128), (13, 20, 60, 128), (24, 20, 60, 128)]


@pytest.mark.parametrize("case", STRADDLE_CASES)
def test_straddling_inputs_tell_the_associations_apart(case):
    _, i1, _ = straddle_inputs(*case)
    a, b = quarter_sum_bits32(i1[:2]), quarter_sum_bits32(i1[:2], pairs=False)
    assert float((a != b).float().mean()) >= 0.02 and 0.2 <= float(a.mean()) <= 0.8
    assert float((i1.double().mean(1) - 1.0).abs().max()) <= 6 * 2.0 ** -23


UPSAMPLE_CASES = [
    # B, H8, W8, logits
    (2, 1, 1, "scale1"), (2, 1, 19, "scale20"), (2, 11, 19, "scale80"), (1, 11, 19, "ties"), (1, 11, 19, "onehot"),
    (1, 60, 128, "scale1"), (1, 90, 160, "scale20"),
]


def upsample_inputs(B, H, W, kind):
    g = gen(5000 + H * W + len(kind))
    flow = torch.randn(B, 2, H, W, generator=g) * 3
    if kind.startswith("scale"):
        mask = torch.randn(B, 576, H, W, generator=g) * float(kind[5:])
    elif kind == "ties":       # equal logits in groups: all nine (zeros) in the first row, subsets elsewhere
        mask = torch.randint(0, 2, (B, 576, H, W), generator=g).float() * 3.0
        mask[:, :, 0] = 0.0
    else:                      # one tap 200 above the rest: its weight is 1 to fp32
        mask = torch.randn(B, 576, H, W, generator=g)
        k = torch.randint(0, 9, (B, 1, 64, H, W), generator=g)
        mask = (mask.view(B, 9, 64, H, W) + 200.0 * (torch.arange(9).view(1, 9, 1, 1, 1) == k)).view(B, 576, H, W)
    return flow, mask.contiguous()


def upsample_bound(flow, mask):
    m = mask.view(mask.shape[0], 9, 64, *mask.shape[2:])
    spread = float((m.amax(1) - m.amin(1)).max())
    return MARGIN * (K_UP + C_UP * spread) * EPS * 8 * float(flow.abs().max())


DOWNFLOW_CASES = [(8, 8), (8, 64), (64, 8), (16, 24), (480, 1024), (720, 1280)]


def downflow_inputs(H, W, kind):
    if kind == "noise":
        return torch.randn(2, 2, H, W, generator=gen(6000 + H + W)) * 5
    xs, ys = grid32(H, W)
    f = torch.stack([3 * torch.sin(xs / 90) + ys / 200, 2 * torch.cos(ys / 70) - xs / 300])[None]
    return torch.cat([f, 1.5 * f.flip(1)], 0).contiguous()


DEFORM_CASES = [
    # kernel, C, B, H, W, chunks
    ("s16", 128, 1, 60, 128, 8), ("s16", 128, 4, 60, 128, 2), ("s16", 32, 16, 60, 128, 1), ("s16", 32, 2, 14, 22, 1),
    ("s16", 96, 2, 14, 22, 8), ("s16", 160, 1, 13, 17, 8),
    ("f32", 128, 1, 60, 128, 8), ("f32", 128, 4, 60, 128, 2), ("f32", 8, 16, 60, 128, 1), ("f32", 8, 2, 14, 22, 1),
    ("f32", 100, 2, 14, 22, 8),
]


def test_deform_cases_cover_the_table():
    for kern in ("s16", "f32"):
        cs = [c for c in DEFORM_CASES if c[0] == kern]
        assert all(deform_chunks(*c[1:5]) == c[5] for c in cs)
        # chunks = 8, 1 (few channels), 2, 1 (many samples): the four branches of the host's expression
        assert {(c[5], c[2] * 9 * c[3] * c[4] < (1 << 18)) for c in cs} == {(8, True), (1, True), (2, False), (1, False)}
    assert {c[1] for c in DEFORM_CASES if c[0] == "s16"} == {32, 96, 128, 160}
    assert all(deform_presplit(c[1]) for c in DEFORM_CASES if c[0] == "s16")
    assert {c[1] for c in DEFORM_CASES if c[0] == "f32"} == {8, 100, 128}
    assert not deform_presplit(8) and not deform_presplit(100)
    # 12 and 20 octets over 8 chunks: oper = 2 / 3 -> chunks 6, 7 empty / chunk 6 ragged (2 of 3), chunk 7 empty
    assert [min(12, (k + 1) * 2) - min(12, k * 2) for k in range(8)] == [2, 2, 2, 2, 2, 2, 0, 0]
    assert [max(0, min(20, (k + 1) * 3) - k * 3) for k in range(8)] == [3, 3, 3, 3, 3, 3, 2, 0]
    # 100 channels over 8 chunks: cper = 13 -> the last chunk holds 9
    assert min(100, 8 * 13) - 7 * 13 == 9


def deform_inputs(C, B, H, W):
    """Offsets: noise, and on a regular pattern of (pixel, tap) the sample lands exactly on -1, 0, H - 1, H (w: W), just inside
    either border, and far outside."""
    g = gen(7000 + C + B)
    x = torch.randn(B, C, H, W, generator=g)
    off = torch.randn(B, 18, H, W, generator=g) * 2.5
    logit = torch.randn(B, 9, H, W, generator=g) * 2
    xs, ys = grid32(H, W)
    for t in range(9):
        base_h, base_w = ys + float(t // 3 - 1), xs + float(t % 3 - 1)
        th = torch.tensor([-1.0, 0.0, H - 1.0, float(H), -1.0 + 2.0 ** -12, H - 2.0 ** -12, 1.0e4, -1.0e9])
        tw = torch.tensor([-1.0, 0.0, W - 1.0, float(W), -1.0 + 2.0 ** -12, W - 2.0 ** -12, -1.0e4, 1.0e9])
        ph, pw = ((xs + 2 * ys + t) % 16).long(), ((3 * xs + ys + 5 * t) % 16).long()
        off[:, 2 * t] = torch.where(ph < 8, th[ph % 8] - base_h, off[:, 2 * t])
        off[:, 2 * t + 1] = torch.where(pw < 8, tw[pw % 8] - base_w, off[:, 2 * t + 1])
    return x, off, logit


def perm_weight(C):
    """(C, C, 3, 3) with w[o, (o + 7 t) % C, t] = 1: output o is the sum of nine columns, one per tap, and every column
    of the 9 C is read by exactly one output - a wrong, missing or misplaced column shows at full size."""
    w = torch.zeros(C, C, 9)
    o = torch.arange(C)
    for t in range(9):
        w[o, (o + 7 * t) % C, t] = 1.0
    return w.view(C, C, 3, 3)


def test_deform_inputs_visit_every_boundary_branch():
    x, off, _ = deform_inputs(32, 2, 14, 22)
    xs, ys = grid32(14, 22)
    hs = torch.stack([ys + float(t // 3 - 1) + off[:, 2 * t] for t in range(9)], 1)
    ws = torch.stack([xs + float(t % 3 - 1) + off[:, 2 * t + 1] for t in range(9)], 1)
    for p, n in ((hs, 14), (ws, 22)):
        for v in (-1.0, 0.0, n - 1.0, float(n), -1.0 + 2.0 ** -12, n - 2.0 ** -12):
            assert int((p == v).sum()) > 20, v
        assert int((p.abs() > 5000).sum()) > 20


# ------------------------------------------------------------------------------------------------
# CPU: the references against torch's float64 operators, the fp32 oracle and the golden fixtures


def test_references_agree_with_torch_in_float64():
    g = gen(1)
    B, C, H, W = 2, 5, 13, 17
    img = torch.randn(B, C, H, W, generator=g)
    flow = torch.randint(-640, 640, (B, 2, H, W), generator=g).float() / 64        # x + u is exact in float32
    xs, ys = grid32(H, W)
    gx = 2 * (xs[None].double() + flow[:, 0].double()) / (W - 1) - 1
    gy = 2 * (ys[None].double() + flow[:, 1].double()) / (H - 1) - 1
    want = F.grid_sample(img.double(), torch.stack([gx, gy], -1), mode="bilinear", padding_mode="zeros", align_corners=True)
    assert float((warp64(img, flow) - want).abs().max()) <= 1e-12
    assert float((compose64(flow, img[:, :2]) - (flow.double() + want[:, :2])).abs().max()) <= 1e-12
    big = torch.randn(2, 2, 64, 96, generator=g)
    want = F.interpolate(big.double(), size=(8, 12), mode="bilinear", align_corners=True) / 8
    assert float((downflow8_64(big, pos=torch.float64) - want).abs().max()) <= 1e-12
    for hw in ((8, 64), (64, 8), (8, 8)):
        big = torch.randn(1, 2, *hw, generator=g)
        want = F.interpolate(big.double(), size=(hw[0] // 8, hw[1] // 8), mode="bilinear", align_corners=True) / 8
        assert float((downflow8_64(big, pos=torch.float64) - want).abs().max()) <= 1e-12
    x = torch.randn(B, C, H, W, generator=g)
    zero, one = torch.zeros(B, 18, H, W), torch.ones(B, 9, H, W)
    want = F.unfold(x.double(), 3, padding=1).view(B, C, 9, H, W).transpose(1, 2).reshape(B, 9 * C, H, W)
    assert torch.equal(deform_columns64(x, zero, one), want)
    w, b = torch.randn(7, C, 3, 3, generator=g), torch.randn(7, generator=g)
    want = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    assert float((deform_conv64(x, zero, one, w, b) - want).abs().max()) <= 1e-12
    fl, mk = torch.randn(B, 2, 6, 7, generator=g), torch.randn(B, 576, 6, 7, generator=g) * 3
    nb = F.unfold(8 * fl.double(), 3, padding=1).view(B, 2, 9, 1, 6, 7)
    want = (torch.softmax(mk.double().view(B, 1, 9, 64, 6, 7), 2) * nb).sum(2)
    want = want.view(B, 2, 8, 8, 6, 7).permute(0, 1, 4, 2, 5, 3).reshape(B, 2, 48, 56)
    assert float((convex_upsample64(fl, mk) - want).abs().max()) <= 1e-12


def test_references_agree_with_the_fp32_oracle():
    """The oracle evaluates the same positions in fp32: the two differ by fp32 rounding, within the bounds counted above."""
    g = gen(2)
    B, C, H, W = 2, 9, 20, 28
    img, img2 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    for kind in ("noise", "border", "smooth", "int"):
        flow = make_flow(kind, B, H, W, 3)
        tol = K_BILINEAR * EPS * float(img.abs().max())
        assert float((O.backwarp(img, flow) - warp64(img, flow)).abs().max()) <= tol
        acc = img[:, :2].contiguous()
        assert float((O.compose_flow(flow, acc) - compose64(flow, acc)).abs().max()) <= tol + EPS * float(flow.abs().max() + 5)
        tol_e = (K_BILINEAR + 1) * EPS * float(img.abs().max() + img2.abs().max())
        assert float((O.get_occ(flow, img, img2, binary=False) - err_map64(flow, img, img2)).abs().max()) <= tol_e
        assert float((O.get_occ_error(flow, img, img2) - occ_err64(flow, img, img2)).abs().max()) <= tol_e + C * EPS * 2
    for kind in ("scale1", "scale20", "ties", "onehot"):
        fl, mk = upsample_inputs(2, 6, 7, kind)
        assert float((O.convex_upsample(fl, mk) - convex_upsample64(fl, mk)).abs().max()) <= upsample_bound(fl, mk)
    for hw in ((16, 24), (8, 64), (64, 8), (8, 8), (480, 1024)):
        for kind in ("noise", "smooth"):
            big = downflow_inputs(*hw, kind)
            # (the oracle rounds scale * index before it takes the fraction: half an ulp of a position <= max(H, W), times a
            # slope of at most 2 max|plane| per pixel)
            tol = (K_BILINEAR + 2 * max(hw)) * EPS * float(big.abs().max()) / 8
            assert float((O.downflow8(big) - downflow8_64(big)).abs().max()) <= tol
    x, off, logit = deform_inputs(8, 2, 14, 22)
    w, b = torch.randn(6, 8, 3, 3, generator=g) * 0.2, torch.randn(6, generator=g)
    m = torch.sigmoid(logit)
    tol = (K_COL + 72) * EPS * float(x.abs().max()) * float(w.abs().sum(dim=(1, 2, 3)).max())
    assert float((O.deform_conv2d(x, off, m, w, b) - deform_conv64(x, off, m, w, b)).abs().max()) <= tol


def test_references_agree_with_the_golden_fixtures(golden):
    """The reference implementation's own outputs, at the tolerances tests/test_oracle_golden.py holds the oracle to."""
    h = golden("harness")
    assert float((warp64(T(h["img"]), T(h["fflow"])) - T(h["warped"])).abs().max()) <= 1e-5
    assert float((downflow8_64(T(h["big"])) - T(h["down"])).abs().max()) <= 1e-5
    k = golden("deform_conv_kat")
    for tag in "ab":
        a = {n: T(k[tag + "_" + n]) for n in ("x", "offset", "mask", "weight", "bias", "out")}
        out = deform_conv64(a["x"], a["offset"], a["mask"], a["weight"], a["bias"])
        assert bool(((out - a["out"]).abs() <= 5e-6 + 1e-5 * a["out"].abs()).all())


# ------------------------------------------------------------------------------------------------
# GPU


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as o
    assert torch.cuda.is_available()
    return o


@pytest.fixture(scope="module")
def ops16(ops):
    if ops.conv_mode_name() != "f16x3":
        pytest.skip("S16 tensors belong to the f16x3 mode")
    return ops


@pytest.fixture
def launches(ops, monkeypatch):
    """Names of the library entry points called, in order (the route an op took)."""
    from accflow_amd import _lib
    lib, seen = _lib.load(), []
    for name in ("accflow_deform_columns_s16", "accflow_deform_columns_f32", "accflow_activation_f32"):
        def spy(*a, _f=getattr(lib, name), _n=name):
            seen.append(_n)
            return _f(*a)
        monkeypatch.setattr(lib, name, spy)
    return seen


def within(tag, got, ref, bound):
    """|got - ref| <= bound where ref is finite, the same inf / NaN elsewhere; prints the largest error-to-bound ratio."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), tag + ": NaN pattern"
    assert torch.equal(got[~fin & ~torch.isnan(ref)], ref[~fin & ~torch.isnan(ref)]), tag + ": infinities"
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    r = float(((got - ref).abs()[fin] / bound[fin]).max()) if bool(fin.any()) else 0.0
    print("RATIO %s %.3f" % (tag, r))
    assert r <= 1.0, "%s: error / bound = %.3f" % (tag, r)


def plane_max(t):
    return t.double().abs().amax(dim=(2, 3), keepdim=True)


SENT = -777.25


def in_view(t):
    """t as channels [3, 3 + C) of a NaN-filled CUDA buffer: a batch-strided operand; a read outside the slice poisons the result."""
    B, C, H, W = t.shape
    buf = torch.full((B, C + 5, H, W), float("nan"), device="cuda")
    buf[:, 3:3 + C] = t.cuda()
    return buf[:, 3:3 + C]


def out_view(B, C, H, W):
    buf = torch.full((B, C + 5, H, W), SENT, device="cuda")
    return buf[:, 3:3 + C], buf


def untouched(buf, C):
    return bool((buf[:, :3] == SENT).all()) and bool((buf[:, 3 + C:] == SENT).all())


SENT16 = 0x7B5A7B5A


def out16_view(ops, B, C, H, W):
    """An S16 (B, C, H, W) that is octets [1, 1 + O) of items [1, 1 + B) of a sentinel-filled buffer."""
    O_ = (C + 7) // 8
    big = torch.full((B + 2, O_ + 2, 2, H, W, 4), SENT16, dtype=torch.int32, device="cuda")
    return ops.S16(big[1:1 + B, 1:1 + O_], C), big


def untouched16(big, B, O_):
    keep = torch.ones(big.shape[:2], dtype=torch.bool, device=big.device)
    keep[1:1 + B, 1:1 + O_] = False
    return bool((big[keep] == SENT16).all())


@gpu
@pytest.mark.parametrize("case", WARP_CASES)
def test_backwarp_vs_float64(ops, case):
    C, B, H, W, kind, chunks = case
    assert warp_chunks(C) == chunks
    img = torch.randn(B, C, H, W, generator=gen(100 + C))
    flow = make_flow(kind, B, H, W, 200 + C)
    # recorded 2026-10-16, f16x3 mode: largest ratio 0.140
    within("backwarp C%d B%d %dx%d %s" % (C, B, H, W, kind), ops.backwarp(dev(img), dev(flow)), warp64(img, flow),
           MARGIN * K_BILINEAR * EPS * plane_max(img))


@gpu
@pytest.mark.parametrize("case", COMPOSE_CASES)
def test_compose_flow_vs_float64(ops, case):
    """out = step + warp(acc, step): one more rounding, at a magnitude <= |step| + max|acc|.  A NaN / infinite step gives a
    zero sample (the clamp) and leaves the NaN / infinity of `step + 0` in its own channel."""
    B, H, W, kind = case
    step = make_flow(kind, B, H, W, 300 + H)
    acc = torch.randn(B, 2, H, W, generator=gen(301 + H)) * 5
    ref = compose64(step, acc)
    bound = MARGIN * EPS * (K_BILINEAR * plane_max(acc) + torch.nan_to_num(step.double().abs(), nan=0.0, posinf=0.0) + plane_max(acc))
    # recorded 2026-10-16, f16x3 mode: largest ratio 0.164
    within("compose B%d %dx%d %s" % (B, H, W, kind), ops.compose_flow(dev(step), dev(acc)), ref, bound)


def check_bits(tag, bits, err, band):
    bits = bits.detach().cpu()
    assert set(bits.unique().tolist()) <= {0.0, 1.0}, tag
    flips = (bits == 1.0) != (err <= 1.0)
    r = float(((err - 1.0).abs()[flips] / band).max()) if bool(flips.any()) else 0.0
    print("RATIO %s %.3f (%d of %d bits differ)" % (tag, r, int(flips.sum()), flips.numel()))
    assert r <= 1.0, "%s: a bit differs at |err64 - 1| = %.3f of the summation bound" % (tag, r)


@gpu
@pytest.mark.parametrize("case", OCC_CASES)
def test_get_occ_vs_float64(ops16, case):
    """Error map and binary map, as fp32 and pre-split, on the branch the case's size selects.  The binary bits equal
    err64 <= 1 outside the summation band, and the fp32 and S16 forms carry the same bits."""
    ops = ops16
    C, B, H, W, branch = case
    assert occ_branch(B, H, W) == branch
    flow, i1, i2 = occ_inputs(C, B, H, W)
    tag = "C%d B%d %dx%d" % (C, B, H, W)
    emap = err_map64(flow, i1, i2)
    err = emap.mean(dim=1, keepdim=True)
    ops.guard_tripped()
    d = [dev(flow), dev(i1), dev(i2)]
    bound = MARGIN * EPS * (K_BILINEAR * plane_max(i2) + plane_max(i1) + plane_max(i2))
    # recorded 2026-10-16, f16x3 mode: largest ratio 0.136
    within("emap f32 " + tag, ops.get_occ(*d, binary=False), emap, bound)
    e16 = ops.get_occ(*d, binary=False, out16=ops.S16.empty(B, C, H, W, "cuda"))
    # recorded 2026-10-16, f16x3 mode: largest ratio 0.147
    within("emap s16 " + tag, e16.to_float(), emap, bound + S16_REL * emap + S16_ABS)
    b32 = ops.get_occ(*d, binary=True)
    b16 = ops.get_occ(*d, binary=True, out16=ops.S16.empty(B, 1, H, W, "cuda"))
    assert torch.equal(b16.to_float(), b32)
    # recorded 2026-10-16, f16x3 mode: largest ratio 0.005 (at most 1 bit of a case differs)
    check_bits("occ bits %s (%s)" % (tag, branch), b32, err, occ_band(C, i1, i2))
    assert not ops.guard_tripped()


@gpu
def test_get_occ_item_alone_and_inside_a_batch(ops16):
    """The fusion chain runs one sequence at batch 1 (binary4 kernel) and the folded chain / a CVO batch above 2^17 pixels
    (per-pixel kernels): an item gets the same occlusion bits either way, in both output forms."""
    ops = ops16
    C, B, H, W, items = OCC_BATCH_CASE
    assert occ_branch(B, H, W) == "per-pixel" and occ_branch(1, H, W) == "binary4"
    flow, i1, i2 = occ_inputs(C, B, H, W, items)
    d = [dev(flow), dev(i1), dev(i2)]
    b32 = ops.get_occ(*d, binary=True)
    b16 = ops.get_occ(*d, binary=True, out16=ops.S16.empty(B, 1, H, W, "cuda")).to_float()
    assert torch.equal(b16, b32)
    for k in items:
        one = [t[k:k + 1] for t in d]
        a32 = ops.get_occ(*one, binary=True)
        a16 = ops.get_occ(*one, binary=True, out16=ops.S16.empty(1, 1, H, W, "cuda")).to_float()
        assert torch.equal(a32, b32[k:k + 1]) and torch.equal(a16, b32[k:k + 1])
        err = occ_err64(flow[k:k + 1], i1[k:k + 1], i2[k:k + 1])
        # recorded 2026-10-16, f16x3 mode: largest ratio 0.000 (no bit differs)
        check_bits("occ bits C128 item %d of 20" % k, b32[k:k + 1], err, occ_band(C, i1, i2))


@gpu
@pytest.mark.parametrize("case", STRADDLE_CASES)
def test_get_occ_association_at_the_threshold(ops16, case):
    """Every pixel within a few ulp of the threshold (straddle_inputs): all four binary launches - fp32 and S16 output, the
    batch on the per-pixel kernels and two of its items alone on the binary4 kernel - give exactly the bits of the documented
    association, which another order of the same additions does not (regression case of the hand mutation check: the
    seeded random cases flip a bit under such a change about once in a million pixels)."""
    ops = ops16
    C, B, H, W = case
    assert occ_branch(B, H, W) == "per-pixel" and occ_branch(1, H, W) == "binary4"
    flow, i1, i2 = straddle_inputs(C, B, H, W)
    want = quarter_sum_bits32(i1)
    d = [dev(flow), dev(i1), dev(i2)]
    assert torch.equal(ops.get_occ(*d, binary=True).cpu(), want)
    assert torch.equal(ops.get_occ(*d, binary=True, out16=ops.S16.empty(B, 1, H, W, "cuda")).to_float().cpu(), want)
    for k in (0, B - 1):
        one = [t[k:k + 1] for t in d]
        assert torch.equal(ops.get_occ(*one, binary=True).cpu(), want[k:k + 1])
        assert torch.equal(ops.get_occ(*one, binary=True, out16=ops.S16.empty(1, 1, H, W, "cuda")).to_float().cpu(), want[k:k + 1])


@gpu
@pytest.mark.parametrize("case", UPSAMPLE_CASES)
def test_convex_upsample_vs_float64(ops, case):
    B, H, W, kind = case
    flow, mask = upsample_inputs(B, H, W, kind)
    # recorded 2026-10-16, f16x3 mode: largest ratio 0.034
    within("convex_upsample B%d %dx%d %s" % (B, H, W, kind), ops.convex_upsample(dev(flow), dev(mask)),
           convex_upsample64(flow, mask), upsample_bound(flow, mask))


@gpu
@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("hw", DOWNFLOW_CASES)
def test_downflow8_vs_float64(ops, hw, kind):
    H, W = hw
    assert (H // 8 == 1, W // 8 == 1) == {(8, 8): (True, True), (8, 64): (True, False), (64, 8): (False, True)}.get(hw, (False, False))
    big = downflow_inputs(H, W, kind)
    # recorded 2026-10-16, f16x3 mode: largest ratio 0.154
    within("downflow8 %dx%d %s" % (H, W, kind), ops.downflow8(dev(big)), downflow8_64(big),
           MARGIN * K_BILINEAR * EPS * plane_max(big) / 8)


@gpu
@pytest.mark.parametrize("case", DEFORM_CASES)
def test_deform_columns_vs_float64(ops16, launches, case):
    """The columns through the convolution behind them, with weights that read every column exactly once (perm_weight):
    ops.deform_conv2d_s16 with the modulation as logits and as values, and ops.conv2d(offset=, dmask=)."""
    ops = ops16
    kern, C, B, H, W, chunks = case
    assert deform_chunks(C, B, H, W) == chunks and (deform_presplit(C) or kern == "f32")
    x, off, logit = deform_inputs(C, B, H, W)
    m = torch.sigmoid(logit)
    pk = ops.PackedConv(dev(perm_weight(C)), None, stride=1, padding=1, tap_major=True)
    assert pk.zcols is not None
    ref = deform_conv64(x, off, m.double(), perm_weight(C))
    bound = MARGIN * K_DCONV * EPS * 9 * float(x.abs().max())
    tag = "%s C%d B%d %dx%d chunks %d" % (kern, C, B, H, W, chunks)
    ops.guard_tripped()
    route = "accflow_deform_columns_" + kern
    if kern == "s16" or not deform_presplit(C):                # (the fp32 columns of C = 128 are ops.conv2d's alone)
        om = dev(torch.cat([off, logit], 1))                   # (the channel slices AccPlus passes)
        o16 = ops.deform_conv2d_s16(pk, dev(x), om[:, :18], om[:, 18:], ops.S16.empty(B, C, H, W, "cuda"), mask_is_logit=True)
        assert [n for n in launches if n.startswith("accflow_deform")] == [route]
        assert ("accflow_activation_f32" in launches) == (kern == "f32")       # the sigmoid pass of the fp32 route
        # recorded 2026-10-16, f16x3 mode: largest ratio 0.004
        within("deform logits " + tag, o16.to_float(), ref, bound)
        del launches[:]
        o16 = ops.deform_conv2d_s16(pk, dev(x), dev(off), dev(m), ops.S16.empty(B, C, H, W, "cuda"))
        assert launches == [route]
        # recorded 2026-10-16, f16x3 mode: largest ratio 0.004
        within("deform mask " + tag, o16.to_float(), ref, bound)
    if kern == "f32":
        del launches[:]
        out = ops.conv2d(pk, dev(x), offset=dev(off), dmask=dev(m))
        assert launches == ["accflow_deform_columns_f32"]
        # recorded 2026-10-16, f16x3 mode: largest ratio 0.004
        within("deform conv2d " + tag, out, ref, bound)
    assert not ops.guard_tripped()


@gpu
@pytest.mark.parametrize("n_out", [7, 64, 70])
def test_split_tanh_relu_indexed(ops, n_out):
    """Output item b = tanh / relu halves of source item idx[b]; 64 items per launch, looped: bit-equal to split_tanh_relu on
    the gathered tensor, with `net` and `inp` as channel slices of one sentinel-filled buffer."""
    assert (n_out > SPLIT_ITEMS_PER_LAUNCH) == (n_out == 70)
    g = gen(900 + n_out)
    n_src, hd, cd, H, W = 9, 24, 40, 6, 10
    src = dev(torch.randn(n_src, hd + cd, H, W, generator=g) * 2)
    idx = [(5 * b * b + 3) % n_src for b in range(n_out)]                   # repeated, out of order
    assert len(set(idx)) < n_out and idx != sorted(idx)
    buf = torch.full((n_out, hd + cd + 11, H, W), SENT, device="cuda")
    net, inp = buf[:, 2:2 + hd], buf[:, 5 + hd:5 + hd + cd]
    ops.split_tanh_relu_indexed(src, idx, net, inp, hd, cd)
    want_net, want_inp = torch.empty(n_out, hd, H, W, device="cuda"), torch.empty(n_out, cd, H, W, device="cuda")
    ops.split_tanh_relu(src[idx].contiguous(), want_net, want_inp, hd, cd)
    assert torch.equal(net, want_net) and torch.equal(inp, want_inp)
    assert torch.equal(inp, torch.relu(src[idx][:, hd:]))
    for sl in (buf[:, :2], buf[:, 2 + hd:5 + hd], buf[:, 5 + hd + cd:]):
        assert bool((sl == SENT).all())
    for bad in (n_src, -1):
        with pytest.raises(RuntimeError):
            ops.split_tanh_relu_indexed(src, idx[:-1] + [bad], net, inp, hd, cd)


# ------------------------------------------------------------------------------------------------
# operand layouts: slices of sentinel-filled buffers give the bits of the contiguous run and write nothing outside


def _layout_backwarp(ops):
    B, C, H, W = 3, 21, 20, 28
    img, flow = torch.randn(B, C, H, W, generator=gen(11)), make_flow("noise", B, H, W, 12)
    want = ops.backwarp(dev(img), dev(flow))
    out, buf = out_view(B, C, H, W)                                           # out= as a channel slice
    ops.backwarp(in_view(img), in_view(flow), out=out)
    assert torch.equal(out, want) and untouched(buf, C)
    big = torch.full((B + 2, C, H, W), SENT, device="cuda")                   # out= as a batch slice
    ops.backwarp(in_view(img), in_view(flow), out=big[1:1 + B])
    assert torch.equal(big[1:1 + B], want) and bool((big[0] == SENT).all()) and bool((big[B + 1] == SENT).all())


def _layout_compose(ops):
    B, H, W = 3, 20, 28
    step, acc = make_flow("noise", B, H, W, 13), torch.randn(B, 2, H, W, generator=gen(14)) * 4
    assert torch.equal(ops.compose_flow(in_view(step), in_view(acc)), ops.compose_flow(dev(step), dev(acc)))


def _layout_get_occ(ops):
    C, B, H, W = 37, 2, 20, 28
    flow, i1, i2 = occ_inputs(C, B, H, W)
    for binary in (False, True):
        Co = 1 if binary else C
        want = ops.get_occ(dev(flow), dev(i1), dev(i2), binary=binary)
        out, buf = out_view(B, Co, H, W)
        ops.get_occ(in_view(flow), in_view(i1), in_view(i2), binary=binary, out=out)
        assert torch.equal(out, want) and untouched(buf, Co)
        want16 = ops.get_occ(dev(flow), dev(i1), dev(i2), binary=binary, out16=ops.S16.empty(B, Co, H, W, "cuda"))
        o16, big = out16_view(ops, B, Co, H, W)
        ops.get_occ(in_view(flow), in_view(i1), in_view(i2), binary=binary, out16=o16)
        assert torch.equal(o16.data, want16.data) and untouched16(big, B, (Co + 7) // 8)


def _layout_get_occ_large(ops):
    C, B, H, W = 5, 20, 60, 128                                               # the per-pixel binary kernels
    flow, i1, i2 = occ_inputs(C, B, H, W)
    want = ops.get_occ(dev(flow), dev(i1), dev(i2), binary=True)
    out, buf = out_view(B, 1, H, W)
    ops.get_occ(in_view(flow), in_view(i1), in_view(i2), binary=True, out=out)
    assert torch.equal(out, want) and untouched(buf, 1)
    o16, big = out16_view(ops, B, 1, H, W)
    ops.get_occ(in_view(flow), in_view(i1), in_view(i2), binary=True, out16=o16)
    assert torch.equal(o16.to_float(), want) and untouched16(big, B, 1)


def _layout_convex_upsample(ops):
    B, H, W = 2, 11, 19
    flow, mask = upsample_inputs(B, H, W, "scale20")
    want = ops.convex_upsample(dev(flow), dev(mask))
    big = torch.full((B + 2, 2, 8 * H, 8 * W), SENT, device="cuda")
    ops.convex_upsample(in_view(flow), in_view(mask), out=big[1:1 + B])
    assert torch.equal(big[1:1 + B], want) and bool((big[0] == SENT).all()) and bool((big[B + 1] == SENT).all())


def _layout_deform(ops):
    for C in (32, 8):                                                         # pre-split and fp32 columns
        B, H, W = 2, 14, 22
        x, off, logit = deform_inputs(C, B, H, W)
        pk = ops.PackedConv(dev(perm_weight(C)), None, stride=1, padding=1, tap_major=True)
        want = ops.deform_conv2d_s16(pk, dev(x), dev(off), dev(logit), ops.S16.empty(B, C, H, W, "cuda"), mask_is_logit=True)
        got = ops.deform_conv2d_s16(pk, in_view(x), in_view(off), in_view(logit), ops.S16.empty(B, C, H, W, "cuda"),
                                    mask_is_logit=True)
        assert torch.equal(got.data, want.data)


def _layout_flow_from_coords(ops):
    B, H, W = 2, 9, 13
    coords = dev(O.coords_grid(B, H, W) + torch.randn(B, 2, H, W, generator=gen(15)) * 6)
    s0, m0 = ops.S16.empty(B, 16, H, W, "cuda"), ops.S16.empty(B, 128, H, W, "cuda", zero=True)
    d0 = torch.empty(B, 2, H, W, device="cuda")
    ops.flow_from_coords_s16(coords, d0, None, s0, m0, 126)
    stack, sbig = out16_view(ops, B, 16, H, W)
    mbig = torch.full((B + 1, 17, 2, H, W, 4), SENT16, dtype=torch.int32, device="cuda")
    motion = ops.S16(mbig[1:, 1:], 128)
    o0, b0 = out_view(B, 2, H, W)
    o1, b1 = out_view(B, 2, H, W)
    ops.flow_from_coords_s16(coords, o0, o1, stack, motion, 126)
    assert torch.equal(o0, d0) and torch.equal(o1, d0) and untouched(b0, 2) and untouched(b1, 2)
    assert torch.equal(stack.data, s0.data) and untouched16(sbig, B, 2)
    assert torch.equal(motion.data[:, 15, :, :, :, 3], m0.data[:, 15, :, :, :, 3])        # channels 126, 127: word 3 of octet 15
    mbig[1:, 16, :, :, :, 3] = SENT16
    assert bool((mbig == SENT16).all())                                                   # and nothing else was written
    flow = (coords.cpu().double() - O.coords_grid(B, H, W).double())
    mag = coords.cpu().abs().double() + O.coords_grid(B, H, W).double()         # (one rounding of coords - grid)
    # recorded 2026-10-16, f16x3 mode: largest ratios 0.000 (flow), 0.389 (motion word), 0.176 (stack)
    within("flow_from_coords_s16 flow", d0, flow, EPS * mag + S16_ABS)
    within("flow_from_coords_s16 motion", m0.to_float()[:, 126:128], flow, (EPS + S16_REL) * mag + S16_ABS)
    rows = F.pad(flow, (0, 0, 3, 3))
    want = torch.cat([rows[:, c:c + 1, ky:ky + H] for c in range(2) for ky in range(7)] + [torch.zeros(B, 2, H, W).double()], 1)
    within("flow_from_coords_s16 stack", s0.to_float(), want, (EPS + S16_REL) * float(mag.max()) + S16_ABS)


def _layout_blend_and_norm(ops):
    B, C, H, W = 2, 21, 9, 13
    g = gen(16)
    f1, f2, m = torch.randn(B, C, H, W, generator=g) * 3, torch.randn(B, C, H, W, generator=g), torch.rand(B, 1, H, W, generator=g)
    want = ops.blend(dev(f1), dev(f2), dev(m), out16=ops.S16.empty(B, C, H, W, "cuda"))
    o16, big = out16_view(ops, B, C, H, W)
    ops.blend(dev(f1), dev(f2), dev(m), out16=o16)
    assert torch.equal(o16.data, want.data) and untouched16(big, B, 3)
    x, res = torch.randn(B, C, H, W, generator=g) * 2 + 1, torch.randn(B, C, H, W, generator=g)
    st = host_stats(ops, x)
    want = ops.S16.empty(B, C, H, W, "cuda")
    ops.instance_norm(dev(x), 2, res=dev(res), stats=st, out16=want, fp32_out=False)
    o16, big = out16_view(ops, B, C, H, W)
    ops.instance_norm(dev(x), 2, res=dev(res), stats=st, out16=o16, fp32_out=False)
    assert torch.equal(o16.data, want.data) and untouched16(big, B, 3)


LAYOUTS = {"backwarp": _layout_backwarp, "compose_flow": _layout_compose, "get_occ": _layout_get_occ,
           "get_occ_large": _layout_get_occ_large, "convex_upsample": _layout_convex_upsample, "deform_columns": _layout_deform,
           "flow_from_coords_s16": _layout_flow_from_coords, "blend_and_instance_norm_s16": _layout_blend_and_norm}


@gpu
@pytest.mark.parametrize("op", sorted(LAYOUTS))
def test_operand_layouts(ops16, op):
    ops16.guard_tripped()
    LAYOUTS[op](ops16)
    assert not ops16.guard_tripped()


# ------------------------------------------------------------------------------------------------
# the range guard of every S16 producer: |x| * 2^4 >= 65520 must OR the flag (the documented fallback signal; nothing faults)

CLEAR, TRIP = 4094.0, 4096.0


def host_stats(ops, x):
    """ops.ConvStats of x (B, C, H, W) as a convolution's epilogue leaves them: {sum, M2, n} records, here two per plane."""
    B, C, H, W = x.shape
    xd = x.double().reshape(B, C, H * W)
    recs = []
    for p in (xd[..., :H * W // 2], xd[..., H * W // 2:]):
        recs.append(torch.stack([p.sum(-1), (p - p.mean(-1, keepdim=True)).pow(2).sum(-1), torch.full((B, C), float(p.shape[-1]),
                                                                                                    dtype=torch.float64)], -1))
    return ops.ConvStats(torch.stack(recs, 2).float().cuda().contiguous(), 2)


def expect_guard(ops, fn, tripped, what):
    ops.guard_tripped()                     # (clear whatever an earlier test left)
    out = fn()
    assert ops.guard_tripped() == tripped, what
    assert not ops.guard_tripped(), what + ": reported once, then reset"
    return out


def s16_close(tag, got16, want32):
    """The de-split tensor equals the fp32 form to the format's precision."""
    want = want32.detach().cpu().double()
    within(tag, got16.to_float(), want, S16_REL * want.abs() + S16_ABS)


@gpu
def test_guard_get_occ_error_map(ops16):
    """The value is reached through |I1 - warp(I2)| with both images inside the range."""
    ops = ops16
    C, B, H, W = 13, 2, 9, 12
    g = gen(21)
    i1, i2, flow = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g), torch.zeros(B, 2, H, W)

    def run(v):
        a, b = i1.clone(), i2.clone()
        a[1, 9, 4, 5], b[1, 9, 4, 5] = v / 2, -v / 2                   # zero flow: the sample is the pixel itself
        return a, b, lambda: ops.get_occ(dev(flow), dev(a), dev(b), binary=False, out16=ops.S16.empty(B, C, H, W, "cuda"))
    a, b, fn = run(0.0)
    # recorded 2026-10-16, f16x3 mode: largest ratio 0.497
    s16_close("guard emap tame", expect_guard(ops, fn, False, "tame"), ops.get_occ(dev(flow), dev(a), dev(b), binary=False))
    a, b, fn = run(CLEAR)
    e = expect_guard(ops, fn, False, "4094")
    assert float(e.to_float()[1, 9, 4, 5]) == CLEAR
    expect_guard(ops, run(TRIP)[2], True, "4096")
    expect_guard(ops, lambda: ops.get_occ(dev(flow), dev(i1 * 0.5), dev(i2 * 0.5), binary=True, out16=ops.S16.empty(B, 1, H, W, "cuda")),
                 False, "binary map")


@gpu
def test_guard_blend(ops16):
    ops = ops16
    B, C, H, W = 2, 13, 9, 12
    g = gen(22)
    f1, f2, m = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g), torch.rand(B, 1, H, W, generator=g)

    def run(v):
        a, b, mm = f1.clone(), f2.clone(), m.clone()
        a[0, 12, 8, 11], b[0, 12, 8, 11], mm[0, 0, 8, 11] = v, v, 0.5       # 0.5 v + 0.5 v: exact
        return a, b, mm, lambda: ops.blend(dev(a), dev(b), dev(mm), out16=ops.S16.empty(B, C, H, W, "cuda"))
    a, b, mm, fn = run(1.0)
    # recorded 2026-10-16, f16x3 mode: largest ratio 0.678
    s16_close("guard blend tame", expect_guard(ops, fn, False, "tame"), ops.blend(dev(a), dev(b), dev(mm)))
    assert float(expect_guard(ops, run(CLEAR)[3], False, "4094").to_float()[0, 12, 8, 11]) == CLEAR
    expect_guard(ops, run(TRIP)[3], True, "4096")


@gpu
@pytest.mark.parametrize("logit", [True, False])
def test_guard_deform_columns(ops16, launches, monkeypatch, logit):
    """The 1x1 convolution behind the columns has a guard of its own (its pre-split output), and an out-of-range column
    reaches it as an infinity: the convolution is taken out here, so that only the columns kernel can raise the flag - and
    the columns themselves are compared with float64."""
    ops = ops16
    B, C, H, W = 2, 32, 9, 12
    x, off, lg = deform_inputs(C, B, H, W)
    off[0] = 0.0                                                           # item 0: the centre tap samples the pixel itself
    msk = lg if logit else torch.sigmoid(lg)
    msk[0] = 40.0 if logit else 1.0                                        # sigmoid(40) = 1 in fp32
    pk = ops.PackedConv(dev(perm_weight(C)), None, stride=1, padding=1, tap_major=True)
    kept = []
    monkeypatch.setattr(ops, "conv2d", lambda zpk, cols, out16=None, fp32_out=True: kept.append(cols) or out16)

    def run(v):
        a = x.clone()
        a[0, 31, 8, 11] = v
        return a, lambda: ops.deform_conv2d_s16(pk, dev(a), dev(off), dev(msk), ops.S16.empty(B, C, H, W, "cuda"), mask_is_logit=logit)
    a, fn = run(1.0)
    expect_guard(ops, fn, False, "tame")
    m64 = torch.sigmoid(msk.double()) if logit else msk.double()
    want = deform_columns64(a, off, m64)
    # recorded 2026-10-16, f16x3 mode: largest ratio 0.060
    within("deform columns s16 logit=%d" % logit, kept[-1].to_float(), want,
           MARGIN * K_COL * EPS * float(a.abs().max()) + S16_REL * want.abs() + S16_ABS)
    expect_guard(ops, run(CLEAR)[1], False, "4094")
    assert float(kept[-1].to_float()[0, 4 * C + 31, 8, 11]) == CLEAR       # (tap 4 = the centre)
    expect_guard(ops, run(TRIP)[1], True, "4096")
    assert set(launches) == {"accflow_deform_columns_s16"}


@gpu
def test_guard_flow_from_coords(ops16):
    """Through a coordinate: the flow word of the motion features and the row-shifted stack both hold coords - grid."""
    ops = ops16
    B, H, W = 2, 9, 12
    base = O.coords_grid(B, H, W) + torch.randn(B, 2, H, W, generator=gen(24))

    def run(v, with_motion):
        c = base.clone()
        c[1, 1, 8, 11] = 8.0 + v                                           # y = 8: flow_y = v exactly
        motion = ops.S16.empty(B, 128, H, W, "cuda", zero=True) if with_motion else None
        stack = ops.S16.empty(B, 16, H, W, "cuda")
        return stack, motion, lambda: ops.flow_from_coords_s16(dev(c), None, None, stack, motion, 126)
    for with_motion in (True, False):
        expect_guard(ops, run(0.0, with_motion)[2], False, "tame")
        stack, motion, fn = run(CLEAR, with_motion)
        expect_guard(ops, fn, False, "4094")
        assert float(stack.to_float()[1, 10, 8, 11]) == CLEAR               # channel 7 + 3: flow_y, unshifted
        assert motion is None or float(motion.to_float()[1, 127, 8, 11]) == CLEAR
        expect_guard(ops, run(TRIP, with_motion)[2], True, "4096")


@gpu
def test_guard_instance_norm(ops16):
    """A normalised value alone is bounded by sqrt(H * W) (one spike in a plane of zeros gives sqrt(H * W - 1)), far below
    4095 at any size the encoders see: modes 0 and 1 and the projected form (two normalised values) have a clear side only.
    Mode 2 reaches the range through its residual: a large fp32 one, or a pre-split one near the top of the format plus a
    normalised spike."""
    ops = ops16
    B, C, H, W = 2, 13, 16, 24
    g = gen(25)
    x = torch.randn(B, C, H, W, generator=g) * 2 + 0.5
    x[1, 12, 15, 23] = 60.0                                                 # a spike: its normalised value is large
    n64 = F.instance_norm(x.double(), eps=1e-5)
    assert float(n64[1, 12, 15, 23]) > 6.5 and float(n64[0, 0].min()) < -0.5
    neg = divmod(int(n64[0, 0].argmin()), W)                                # relu(norm) = 0 here: the result is the residual
    st = host_stats(ops, x)
    res = torch.rand(B, C, H, W, generator=g)

    def run(mode, r=None, fp32_out=False):
        o16 = ops.S16.empty(B, C, H, W, "cuda")
        o32 = ops.instance_norm(dev(x), mode, res=r, stats=st, out16=o16, fp32_out=fp32_out)
        return o16, o32
    for mode in (0, 1, 2):
        r = dev(res) if mode == 2 else None
        o16, o32 = expect_guard(ops, lambda: run(mode, r, True), False, "tame mode %d" % mode)
        # recorded 2026-10-16, f16x3 mode: largest ratio 0.904 (mode 0), 0.793, 0.497
        s16_close("guard instance norm mode %d" % mode, o16, o32)
        want = {0: n64, 1: torch.relu(n64), 2: torch.relu(res.double() + torch.relu(n64))}[mode]
        assert float((o32.cpu().double() - want).abs().max()) <= 2e-5           # (tests/test_hip_parity.py's tolerance)

    def with_res(v, where):
        r = res.clone()
        r[where] = v
        return r
    o16, _ = expect_guard(ops, lambda: run(2, dev(with_res(CLEAR, (0, 0) + neg))), False, "fp32 residual 4094")
    assert float(o16.to_float()[(0, 0) + neg]) == CLEAR
    expect_guard(ops, lambda: run(2, dev(with_res(5000.0, (0, 3, 2, 2)))), True, "fp32 residual 5000")
    # the pre-split residual
    r16 = expect_guard(ops, lambda: ops.to_s16(dev(res)), False, "to_s16")
    o16, o32 = expect_guard(ops, lambda: run(2, r16, True), False, "S16 residual, tame")
    # recorded 2026-10-16, f16x3 mode: largest ratio 0.497
    s16_close("guard instance norm s16res", o16, o32)
    r16 = ops.to_s16(dev(with_res(CLEAR, (0, 0) + neg)))
    o16, _ = expect_guard(ops, lambda: run(2, r16), False, "S16 residual 4094")
    assert float(o16.to_float()[(0, 0) + neg]) == CLEAR
    r16 = ops.to_s16(dev(with_res(4090.0, (1, 12, 15, 23))))                # 4090 + a normalised value above 6.5
    expect_guard(ops, lambda: run(2, r16), True, "S16 residual 4090 + spike")
    # the projected closing pass: relu(norm(proj) + relu(norm(x)))
    proj = torch.randn(B, C + 11, H, W, generator=g) * 3 - 1
    pst = host_stats(ops, proj)
    pd = dev(proj)
    o16 = expect_guard(ops, lambda: ops.instance_norm_proj(dev(x), st, pd[:, 8:8 + C], pst, 8, ops.S16.empty(B, C, H, W, "cuda")),
                       False, "projection")
    want = torch.relu(F.instance_norm(proj[:, 8:8 + C].double(), eps=1e-5) + torch.relu(n64))
    assert float((o16.to_float().cpu().double() - want).abs().max()) <= 2e-5 + S16_REL * float(want.max())
