"""Every route of the CorrBlock lookup from a stored pyramid (csrc/corr_lookup.hip, corr_lookup_disp_kernel in
csrc/corr_disp.hip, csrc/corr_lookup_conv.hip) against a float64 reference written HERE, element by element.

Routes (pinned to the sources by test_route_table_is_the_one_in_the_sources):
         entry point                       kernel                             layout      output
    L1   accflow_corr_lookup_f32           corr_lookup_kernel<4>              row-major   fp32, 4 x 81 channels
    L2   accflow_corr_lookup_r3_f32        corr_lookup_kernel<3>              row-major   fp32, 4 x 49 channels
    L3   accflow_corr_lookup_disp_f32      corr_lookup_disp_kernel<1, false>  displaced   fp32, 4 x 81 channels
    L4   accflow_corr_lookup_disp_s16      corr_lookup_disp_kernel<1, true>   displaced   pre-split S16, 4 x 88 channels
    L5   accflow_corr_lookup_convc1_s16    corr_lookup_convc1_ws_kernel<3>    displaced   act(convc1(lookup)), taps never stored
The two on-the-fly routes (accflow_corr_lookup_alt_*) compute the correlation itself; tests/test_alt_corr.py owns them.

Reference.  The pyramid is DATA: each level an independent random tensor (B P, 1, H8 >> l, W8 >> l), the displaced form
DispPyramid.from_rowmajor of the same tensors - nothing here depends on the volume kernels.  The level coordinate is formed
as the kernels form it: fp32 coords x fp32(2^-l) (exact; no subnormal coordinate is used), then
fminf(fmaxf(., -1e6), 1e6) (a NaN becomes -1e6).  From there on everything is float64: floor, the two fractions, the four
weights, zero outside the plane.  Channel l T^2 + i T + j, i along x, j along y, T = 2 R + 1.
test_reference_is_the_oracle_lookup pins it to oracle.accflow_oracle.corr_lookup in float64 for both radii.

Gate, per element, none of it taken from what a kernel returns:
    |got - ref64| <= MARGIN K_LOOKUP 2^-24 m,       MARGIN = 2 (tests/test_sampling_ops.py), K_LOOKUP = 8
    m = the largest |value| of the four cells the tap blends, cells outside the plane counting as 0 - so a tap wholly
        outside the plane must be exactly 0.
K_LOOKUP counts the roundings of the kernels' chain fma(a11, w11, fma(a10, w10, fma(a01, w01, a00 * w00))), each as an
ABSOLUTE error in units of eps m (eps = 2^-24); the weights cannot be counted relatively, 1 - ax loses all its bits where
ax rounds to 1:
    ax = cx - floor(cx) is NOT always exact: it is inexact only when the difference is larger than |cx| (cx in (-1, 0) and
      the result >= 1/2; for cx in (-2^-25, 0) it rounds to 1.0), one rounding of a number <= 1: eps / 2.  Then ax >= 1/2
      and 1 - ax is exact (Sterbenz).  Where ax is exact, 1 - ax rounds once at <= 1: eps / 2.  Either way ax and 1 - ax
      each carry <= eps / 2; across the four weights that is (eps / 2) ((1 - ay) + (1 - ay) + ay + ay) = eps; the same for
      ay: 2 so far.
    the four products w = (.)(.) round once each, relative: eps (w00 + w01 + w10 + w11) = eps: 3.
    a00 * w00 rounds once and each of the three fmas once, at partial sums <= m (the weights sum to <= 1): 7.
    + 1 for the second-order terms: 8.
So the gate is 16 eps m: 20 times tighter than the 2e-5 on N(0, 1) data of the older tests, and relative per element.
    S16 output (L4): + S16_REL |x| + S16_ABS = 2^-22 |x| + 2^-29 (tests/test_sampling_ops.py).
    L5, one-hot weights: the L4 gate for the fp32 destination (the taps are split before the product; the weight 1 and its
      power-of-two row scale split exactly, every other product is zero, the accumulation adds only hi + lo), one more S16
      term for the pre-split destination.
test_fp32_evaluation_holds_the_gate shows that torch's fp32 evaluation of the same formula on the CPU stays inside the gate
on every case of the module.

Shapes (B, H8, W8): Sa (2, 8, 8): P = 64, one wave, half a 128-pixel block, level 3 is 1 x 1, every window straddles every
border;  Sb (1, 9, 11): P = 99, second wave with 35 live lanes, levels 4 x 5, 2 x 2, 1 x 1, x1 >> l == Wl and
y1 >> l == Hl occur at levels 1 - 3 (the displaced layout's wrap m += Wl taken by every cell);  Sc (1, 17, 23): P = 391,
4 blocks of 128, the last with 7 pixels, odd height, odd widths at levels 0 - 2 (17, 8, 4, 2 x 23, 11, 5, 2);  Sd (2, 12, 88): level 3 is 1 x 11: load_row's 16-byte
path (Wl >= 10 at radius 4, >= 8 at radius 3) is reachable in x at every level, B = 2 through a wide frame.
Coordinates: the grid plus a smooth flow (bilinear from a 3 x 4 control grid at +-3 px), noise at sigma = 4, or zero; on
top of that PLACED coordinates c = 2^l u per level, with xs = floor(u) - R:
    A window wholly inside;  B straddling the low border, C the high border, BC both (plane narrower than 2 R + 1);
    Dl only the last window column / row inside (xs + 2 R + 1 == 0), Df only the first (xs == Wl - 1);
    El / Eh just outside (xs + 2 R + 2 == 0, xs == Wl): every tap exactly 0;
    F0 / Fn integer u = 0 and Wl - 1, Fh half-integer u;  G u = -2^-26: fp32 ax rounds to 1;
    H +-1e5, +-1e9, +-inf, NaN in x alone, in y alone and in both.
test_placed_coordinates_reach_every_class asserts from the reference's integer origins that every class realisable at a
level is hit at that level, for both radii and both axes, with the other axis's window on the plane, in a ragged shape
(Sb or Sc) and in Sd.  Placed pixels sit in the last, partly filled wave of Sb and Sc.
Values: unit (randn), everywhere; spread (randn 2^U(-10, 8) per cell, all |x| 16 < 65520 - asserted) on every route at Sb
and Sd.

Further checks of every GPU case: L3 == L1 bit for bit; L4 == the S16 split of L3 bit for bit (hi = fp16(16 v),
lo = fp16(16 v - hi), channel l 88 + j 9 + i, the 7 tail channels of each level zero); L2's channel (l, i, j) == L1's
(l, i + 1, j + 1) bit for bit; every destination is a channel slice of a wider sentinel-filled tensor (with B = 2 the
batch stride differs from the channel count) whose other channels stay unchanged bit for bit; the padding lanes p >= P of
the displaced pyramid hold NaN and every result is finite; the range guard is quiet after every L4 and L5 call.

Teeth (test_gate_has_teeth, CPU): seven mutations of the float64 reference at the module's own inputs - i / j swapped,
origin off by one in x, trunc for floor, border clamp for zero padding, ax + 2^-18, the clamp dropped, one level's plane
taken from the neighbouring pixel.  Largest error / gate per mutation, measured on the CPU: see the test's docstring.
The order of level scale and clamp cannot be told apart by ANY input at these shapes (whatever the clamp touches lies
>= 1e6 / 8 cells outside every plane at either order; 1e5 is clamped at neither): the test asserts that instead.

Not covered: the on-the-fly routes (above), invalid arguments (tests/test_host_logic.py), shapes beyond (12, 88).

Measured on the MI355X, 2026-10-20, every case passing (each under a tenth of a second after the first) - largest
error / gate per route, unit / spread:
    L1 0.201 / 0.159   L2 0.175 / 0.157   L3 0.201 / 0.159 (the bits of L1)   L4 0.740 / 0.960
    L5 fp32 0.439 / 0.923   L5 S16 0.284 / 0.470;  L5's fp32 result equals the decode of L4's taps exactly in all 8 cases.
(The fp32 routes sit at 3.2 eps m of the 16; torch's float32 evaluation on the CPU reaches the same 0.201.  The S16 figures
near 1 are the spread class's smallest values, where lo is an fp16 subnormal and S16_ABS = 2^-29, half its spacing over 16,
is the whole gate and the whole error.)  Every bit-for-bit identity held in every case: nothing was found to fix.
Nobody had measured these ratios before the module was written; no gate, margin, shape or input was chosen from them.
"""
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import accflow_oracle as O
from test_sampling_ops import MARGIN, EPS, S16_REL, S16_ABS, clamp_like_make_taps, gen, dev

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_LOOKUP = 8
ASHIFT = 4                      # ACCFLOW_F16_ASHIFT
ASC = float(1 << ASHIFT)
F16_GUARD = 65520.0
S16_LEVEL_CHANNELS = 88
LOOKUP_FUSED_K = 336
SHAPES = {"Sa": (2, 8, 8), "Sb": (1, 9, 11), "Sc": (1, 17, 23), "Sd": (2, 12, 88)}      # name -> (B, H8, W8)
KINDS = ("smooth", "noise", "zero")
SENT = -777.25
SENT16 = 0x5A5A5A5A
PAD_LO, PAD_HI = 5, 7           # sentinel channels below / above an fp32 destination
HUGE = (1.0e5, -1.0e5, 1.0e9, -1.0e9, float("inf"), float("-inf"), float("nan"))
ROUTES = {
    "L1": ("accflow_corr_lookup_f32", "corr_lookup_kernel<4>"),
    "L2": ("accflow_corr_lookup_r3_f32", "corr_lookup_kernel<3>"),
    "L3": ("accflow_corr_lookup_disp_f32", "corr_lookup_disp_kernel<1, false>"),
    "L4": ("accflow_corr_lookup_disp_s16", "corr_lookup_disp_kernel<1, true>"),
    "L5": ("accflow_corr_lookup_convc1_s16", "corr_lookup_convc1_ws_kernel<3>"),
}

CASES = [(s, k, "unit") for s in SHAPES for k in KINDS] + [(s, k, "spread") for s in ("Sb", "Sd") for k in KINDS]
# L5: shape, coordinates, values, first tap, activation ("none" once and "relu" once per shape and value class; t0 = 0 and
# 68 together read all 324 taps, tap 80 of each level through the 16-deep tail step)
FUSED_CASES = [(s, k, c, t0, act) for s, c in (("Sb", "unit"), ("Sc", "unit"), ("Sb", "spread"), ("Sd", "spread"))
               for k, t0, act in (("smooth", 0, "none"), ("noise", 68, "relu"))]


def case_id(c):
    return "-".join(map(str, c))


def _seed(*key):
    s = 29
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % 1000003
    return s


# ------------------------------------------------------------------------------------------------
# routes pinned to the sources


def _function_body(text, head):
    i = text.index(head)
    return text[i:text.index("\n}\n", i)]


def test_route_table_is_the_one_in_the_sources():
    """The entry -> kernel table, R = 4 or 3, the 88-channel S16 stride, LOOKUP_FUSED_K = 336, ACCFLOW_F16_ASHIFT = 4 and
    the one blend chain stand in the sources as this module restates them."""
    def src(*p):
        return open(os.path.join(ROOT, *p)).read()
    csrc = ("accflow_amd", "csrc")
    look, disp, conv = src(*csrc, "corr_lookup.hip"), src(*csrc, "corr_disp.hip"), src(*csrc, "corr_lookup_conv.hip")
    py = src("accflow_amd", "ops.py")
    assert "#define ACCFLOW_F16_ASHIFT %d\n" % ASHIFT in src("include", "accflow_hip.h")
    launched = {}
    # L1, L2: one templated launcher, instantiated at 4 and 3
    for row, R in (("L1", 4), ("L2", 3)):
        body = _function_body(look, 'extern "C" int %s(' % ROUTES[row][0])
        assert re.findall(r"return launch_lookup<(\d)>\(", body) == [str(R)]
        launched[row] = "corr_lookup_kernel<%d>" % R
    launcher = _function_body(look, "int launch_lookup(")
    assert re.findall(r"hipLaunchKernelGGL\(([a-z_0-9]+<[A-Z]>),", launcher) == ["corr_lookup_kernel<R>"]
    assert 'static_assert(R == 4 || R == 3, "load_row moves rows of 10 or 8 floats");' in look
    assert "constexpr int WIN = 2 * R + 2, T = 2 * R + 1;" in look
    assert "if (xs >= 0 && xs + WIN <= Wl) {" in look
    assert "hipLaunchKernelGGL(corr_lookup_kernel<R>, dim3(cdiv(np, 64)), dim3(256)," in look
    # L3, L4: the two instantiations of the displaced kernel (OUT16 defaults to false)
    assert "template <int PF, bool OUT16 = false>" in disp and "constexpr int R = 4, WIN = 2 * R + 2;" in disp
    for row in ("L3", "L4"):
        body = _function_body(disp, 'extern "C" int %s(' % ROUTES[row][0])
        k = re.findall(r"hipLaunchKernelGGL\(\(?(corr_lookup_disp_kernel<[^>]*>)\)?, dim3\(cdiv\(\(long long\)H8 \* W8, 64\), B, 4\), dim3\(64\)", body)
        assert len(k) == 1 and body.count("hipLaunchKernelGGL(") == 1
        launched[row] = {"corr_lookup_disp_kernel<1>": "corr_lookup_disp_kernel<1, false>"}.get(k[0], k[0])
    assert disp.count("o16[(long long)((lvl * 11 + oct) * 2 + ") == 2 and 11 * 8 == S16_LEVEL_CHANNELS
    assert "const int n = j * 9 + i;" in disp and "o[(long long)(i * 9 + j) * P] = blend4(" in disp
    assert "if (m < 0) m += Wl;" in disp and "if (m < 0) m += Hl;" in disp
    # L5: the product build launches the PF = 3 instantiation
    body = _function_body(conv, 'extern "C" int %s(' % ROUTES["L5"][0])
    k = re.findall(r"hipLaunchKernelGGL\(\((corr_lookup_convc1_ws_kernel<[^>]*>)\), grid, block, 0, st, a\);", body)
    assert k == ["corr_lookup_convc1_ws_kernel<3, true>", "corr_lookup_convc1_ws_kernel<3>"]     # (the first: tools builds only)
    assert body.index("#ifdef ACCFLOW_LC1_PROF") < body.index(k[0]) < body.index("#endif") < body.rindex(k[1])
    launched["L5"] = k[1]
    assert launched == {r: v[1] for r, v in ROUTES.items()}
    assert "constexpr int NSUPER = 10, NSTEP = 21;" in conv and "return 16 * NSTEP;" in conv and 16 * 21 == LOOKUP_FUSED_K
    assert "constexpr int R = 4, WIN = 2 * R + 2;" in conv and "constexpr int n = j * 9 + i;" in conv
    # the one blend chain and the one coordinate chain, in all three files
    chain = "__builtin_fmaf(a11, w11, __builtin_fmaf(a10, w10, __builtin_fmaf(a01, w01, a00 * w00)))"
    assert chain in disp and chain in conv
    assert "__builtin_fmaf(r1[i + 1], w11, __builtin_fmaf(r1[i], w10, __builtin_fmaf(r0[i + 1], w01, r0[i] * w00)))" in look
    for text in (look, disp, conv):
        assert len(re.findall(r"c[xy] = fminf\(fmaxf\(c[xy], -1\.0e6f\), 1\.0e6f\);", text)) == 2
        assert "const float inv = 1.0f / (float)(1 << lvl);" in text
        assert "const float ax = cx - fx0, ay = cy - fy0;" in text
        assert "const int xs = (int)fx0 - R, ys = (int)fy0 - R;" in text
        assert "const float w00 = (1.0f - ax) * (1.0f - ay), w01 = ax * (1.0f - ay), w10 = (1.0f - ax) * ay, w11 = ax * ay;" in text
    # ops.py: which entry each wrapper calls, the S16 stride and the fused reduction length
    assert "LOOKUP_S16_CHANNELS = 4 * %d " % S16_LEVEL_CHANNELS in py and "LOOKUP_FUSED_K = %d " % LOOKUP_FUSED_K in py
    assert 'return _corr_lookup_alt(pyramid, coords, out, "accflow_corr_lookup_disp_f32")' in py
    rowmajor = py[py.index("def _corr_lookup_rowmajor("):py.index("def convex_upsample(")]
    assert re.findall(r"_launch\(lib\.(accflow_corr_lookup[a-z0-9_]*),", rowmajor) == ["accflow_corr_lookup_r3_f32", "accflow_corr_lookup_f32"]
    assert rowmajor.index("if radius == 3:") < rowmajor.index("lib.accflow_corr_lookup_r3_f32") < rowmajor.index("lib.accflow_corr_lookup_f32,")
    assert "return _launch(lib.accflow_corr_lookup_disp_s16, args," in py
    assert "return _launch(lib.accflow_corr_lookup_convc1_s16, args," in py


# ------------------------------------------------------------------------------------------------
# seeded inputs


@functools.lru_cache(maxsize=None)
def make_pyramid(shape, cls):
    """4 levels (B P, 1, Hl, Wl) float32 of independent random data."""
    B, H8, W8 = SHAPES[shape]
    g = gen(_seed("pyramid", shape, cls))
    lv = []
    for l in range(4):
        t = torch.randn(B * H8 * W8, 1, H8 >> l, W8 >> l, generator=g)
        if cls == "spread":
            t = t * torch.exp2(torch.rand(t.shape, generator=g) * 18.0 - 10.0)
        else:
            assert cls == "unit"
        lv.append(t.contiguous())
    return tuple(lv)


FRAC = 0.3125


def axis_radius_values(n, R):
    """u along an axis of n cells for the classes that depend on the radius (xs = floor(u) - R)."""
    WIN = 2 * R + 2
    u = []
    if n >= WIN:
        u += [R + FRAC, n - R - 2 + 0.6875]                  # A: xs = 0 and xs = n - WIN
    if n >= WIN - 1:
        u += [R - 1 + FRAC, n - R - 1 + FRAC]                # B: xs = -1;  C: xs = n - WIN + 1
    else:
        u += [R - 1 + FRAC]                                  # BC: xs = -1 and xs + WIN > n
    u += [-R - 1 + FRAC, n - 1 + R + 0.6875]                 # Dl: xs = -(2R + 1);  Df: xs = n - 1
    return u, [-R - 2 + 0.6875, n + R + FRAC]                # El: xs = -(2R + 2);  Eh: xs = n


def axis_common_values(n):
    return [0.0, float(n - 1), float(n // 2), 0.5, n // 2 + 0.5, n - 1 + 0.5, -2.0 ** -26]      # F0, Fn, F, Fh x 3, G


@functools.lru_cache(maxsize=None)
def placements(shape):
    """-> (huge, placed): lists of level-0 (cx, cy), every number exact in float32.  huge: class H; placed: the classes A - G
    of every level.  Every class but E keeps its window on the plane, so one pixel carries a class of x AND a class of y
    (k-th with k-th: the corners low / low, high / high, ...; at radius 4 also k-th with (k + 5)-th); E stands against a
    window on the plane in the other axis (radius 4) or against E (radius 3)."""
    B, H8, W8 = SHAPES[shape]
    placed = []
    for l in range(4):
        Hl, Wl, s = H8 >> l, W8 >> l, float(1 << l)
        midx, midy = Wl // 2 + 0.4375, Hl // 2 + 0.4375
        for R in (4, 3):
            (X, EX), (Y, EY) = axis_radius_values(Wl, R), axis_radius_values(Hl, R)
            if R == 4:
                X, Y = X + axis_common_values(Wl), Y + axis_common_values(Hl)
            n = max(len(X), len(Y))
            placed += [(s * X[k % len(X)], s * Y[k % len(Y)]) for k in range(n)]
            if R == 4:
                placed += [(s * X[k % len(X)], s * Y[(k + 5) % len(Y)]) for k in range(n)]
                placed += [(s * u, s * midy) for u in EX] + [(s * midx, s * u) for u in EY]
            else:
                placed += [(s * EX[0], s * EY[0]), (s * EX[1], s * EY[1])]
    placed = list(dict.fromkeys(placed))
    midx, midy = W8 // 2 + 0.4375, H8 // 2 + 0.4375
    huge = [(v, midy) for v in HUGE] + [(midx, v) for v in HUGE] + [(v, v) for v in HUGE]
    return huge, placed


def placed_budget(shape):
    B, H8, W8 = SHAPES[shape]
    return min(len(placements(shape)[1]), (4 * H8 * W8) // 5 - 3 * len(HUGE))


@functools.lru_cache(maxsize=None)
def make_coords(shape, kind):
    """-> (coords (B, 2, H8, W8) float32, placed mask (B, P)).  Item b of kind k takes class H and `budget` placements
    starting at (k B + b) budget of the list (so the small shapes walk through it over their cases); even items fill the END
    of the frame (the last, partly filled wave), odd items the start."""
    B, H8, W8 = SHAPES[shape]
    P = H8 * W8
    g = gen(_seed("coords", shape, kind))
    ys, xs = torch.meshgrid(torch.arange(H8, dtype=torch.float32), torch.arange(W8, dtype=torch.float32), indexing="ij")
    if kind == "smooth":
        ctrl = (torch.rand(B, 2, 3, 4, generator=g) * 2 - 1) * 3
        flow = F.interpolate(ctrl, size=(H8, W8), mode="bilinear", align_corners=True)
    elif kind == "noise":
        flow = torch.randn(B, 2, H8, W8, generator=g) * 4
    else:
        assert kind == "zero"
        flow = torch.zeros(B, 2, H8, W8)
    coords = (torch.stack([xs, ys])[None] + flow).reshape(B, 2, P).contiguous()
    huge, placed = placements(shape)
    n = placed_budget(shape)
    mask = torch.zeros(B, P, dtype=torch.bool)
    for b in range(B):
        start = (KINDS.index(kind) * B + b) * n
        pts = huge + [placed[(start + t) % len(placed)] for t in range(n)]
        assert len(pts) <= P
        for t, (cx, cy) in enumerate(pts):
            p = P - 1 - t if b % 2 == 0 else t
            coords[b, 0, p], coords[b, 1, p] = cx, cy
            mask[b, p] = True
    return coords.view(B, 2, H8, W8), mask


# ------------------------------------------------------------------------------------------------
# the reference (float64), the same formula in float32, and its mutations

MUTATIONS = ("ij swapped", "origin + 1 in x", "trunc for floor", "border clamp", "ax + 2^-18", "no clamp", "neighbour's plane")


def level_coord32(c, l, scale_after_clamp=False, clamp=True):
    """float32 level-0 coordinates -> the float32 level coordinate as the kernels form it."""
    inv = torch.tensor(1.0 / (1 << l), dtype=torch.float32)
    assert c.dtype == torch.float32
    if scale_after_clamp:
        return clamp_like_make_taps(c) * inv
    return clamp_like_make_taps(c * inv) if clamp else c * inv


def lookup(pyr, coords, R, dtype=torch.float64, mut=None):
    """-> (out (B, 4 T^2, H8, W8) in dtype, m (same shape, float64): the largest |cell| of the four a tap blends,
    origins: per level (xs, ys, ax, ay, cx32, cy32) over the B P pixels)."""
    B, _, H8, W8 = coords.shape
    P, T, WIN = H8 * W8, 2 * R + 1, 2 * R + 2
    M = B * P
    q = torch.arange(WIN)
    outs, ms, origins = [], [], []
    for l, lvl in enumerate(pyr):
        Hl, Wl = H8 >> l, W8 >> l
        assert tuple(lvl.shape) == (M, 1, Hl, Wl)
        plane = lvl.reshape(M, Hl * Wl)
        if mut == "neighbour's plane" and l == 1:
            plane = torch.roll(plane, 1, dims=0)
        kw = {"scale_after_clamp": mut == "scale after clamp", "clamp": mut != "no clamp"}
        cx32, cy32 = level_coord32(coords[:, 0].reshape(M), l, **kw), level_coord32(coords[:, 1].reshape(M), l, **kw)
        cx, cy = cx32.to(dtype), cy32.to(dtype)
        fx, fy = (torch.trunc(cx), torch.trunc(cy)) if mut == "trunc for floor" else (torch.floor(cx), torch.floor(cy))
        ax, ay = cx - fx, cy - fy
        if mut == "ax + 2^-18":
            ax = ax + 2.0 ** -18
        xs, ys = torch.nan_to_num(fx).long() - R, torch.nan_to_num(fy).long() - R
        if mut == "origin + 1 in x":
            xs = xs + 1
        xx, yy = xs[:, None] + q, ys[:, None] + q                                   # (M, WIN)
        okx, oky = (xx >= 0) & (xx < Wl), (yy >= 0) & (yy < Hl)
        if mut == "border clamp":
            okx, oky = torch.ones_like(okx), torch.ones_like(oky)
        idx = (yy.clamp(0, Hl - 1)[:, :, None] * Wl + xx.clamp(0, Wl - 1)[:, None, :]).reshape(M, WIN * WIN)
        ok = (oky[:, :, None] & okx[:, None, :])
        win = plane.gather(1, idx).reshape(M, WIN, WIN)                             # [pixel][row r][column q], float32
        win = torch.where(ok, win, torch.zeros_like(win))
        a = win.to(dtype)
        a00, a01, a10, a11 = a[:, :T, :T], a[:, :T, 1:], a[:, 1:, :T], a[:, 1:, 1:]  # [pixel][j][i]
        w00, w01, w10, w11 = ((1 - ax) * (1 - ay)), (ax * (1 - ay)), ((1 - ax) * ay), (ax * ay)
        e = (lambda w: w[:, None, None])
        v = ((a00 * e(w00) + a01 * e(w01)) + a10 * e(w10)) + a11 * e(w11)            # the kernels' association
        wa = win.abs().double()
        m = torch.maximum(torch.maximum(wa[:, :T, :T], wa[:, :T, 1:]), torch.maximum(wa[:, 1:, :T], wa[:, 1:, 1:]))
        if mut != "ij swapped":
            v = v.transpose(1, 2)                                                    # [pixel][i][j]
        m = m.transpose(1, 2)
        outs.append(v.reshape(B, P, T * T).transpose(1, 2))
        ms.append(m.reshape(B, P, T * T).transpose(1, 2))
        origins.append((xs, ys, ax.double(), ay.double(), cx32, cy32))
    return (torch.cat(outs, dim=1).reshape(B, 4 * T * T, H8, W8).contiguous(),
            torch.cat(ms, dim=1).reshape(B, 4 * T * T, H8, W8).contiguous(), origins)


def gate_of(m):
    return MARGIN * K_LOOKUP * EPS * m


def s16_term(ref):
    return S16_REL * ref.abs() + S16_ABS


@functools.lru_cache(maxsize=3)
def model(case):
    """The reference and the gate of a case, for both radii."""
    shape, kind, cls = case
    pyr, (coords, _) = make_pyramid(shape, cls), make_coords(shape, kind)
    out = {}
    for R in (4, 3):
        ref, m, org = lookup(pyr, coords, R)
        assert bool(torch.isfinite(ref).all())
        out[R] = {"ref": ref, "m": m, "gate": gate_of(m), "origins": org}
    return out


def worst(err, gate):
    """-> (largest err / gate over the elements with gate > 0, number of elements with err > gate)."""
    pos = gate > 0
    r = float((err[pos] / gate[pos]).max()) if bool(pos.any()) else 0.0
    return r, int((err > gate).sum())


# ------------------------------------------------------------------------------------------------
# CPU: the reference, the inputs, the gate


def test_reference_is_the_oracle_lookup():
    """lookup() in float64 == oracle.accflow_oracle.corr_lookup in float64 on the same float32 data, both radii, to 1e-12
    of the values (of m, the largest cell a tap blends; a tap wholly outside is 0 in both).  Finite in-range coordinates
    only: the oracle has no clamp."""
    for shape in ("Sb", "Sd"):
        for kind in ("smooth", "noise"):
            B, H8, W8 = SHAPES[shape]
            pyr = make_pyramid(shape, "unit")
            coords, _ = make_coords(shape, kind)
            coords = torch.where(torch.isfinite(coords) & (coords.abs() < 1.0e4), coords, torch.full_like(coords, -2.75))
            for R in (4, 3):
                ref, m, _ = lookup(pyr, coords, R)
                want = O.corr_lookup([p.double() for p in pyr], coords.double(), radius=R)
                assert want.shape == ref.shape == (B, 4 * (2 * R + 1) ** 2, H8, W8)
                assert bool(((ref - want).abs() <= 1e-12 * m).all()), (shape, kind, R, float((ref - want).abs().max()))
                assert float(m.max()) > 1 and bool((m == 0).any())


def test_shapes_reach_the_branches_they_are_named_for():
    P = {s: SHAPES[s][1] * SHAPES[s][2] for s in SHAPES}
    assert P["Sa"] == 64 and SHAPES["Sa"][0] == 2 and (8 >> 3, 8 >> 3) == (1, 1)
    assert P["Sb"] == 99 and P["Sb"] - 64 == 35 and [(9 >> l, 11 >> l) for l in (1, 2, 3)] == [(4, 5), (2, 2), (1, 1)]
    for l in (1, 2, 3):       # the last column / row of Sb: every displaced index of that pixel takes the wrap
        assert (11 - 1) >> l == 11 >> l and (9 - 1) >> l == 9 >> l
    assert P["Sc"] == 391 and -(-391 // 128) == 4 and 391 % 128 == 7 and 17 % 2 and all((23 >> l) % 2 for l in range(3))
    assert SHAPES["Sd"] == (2, 12, 88) and (12 >> 3, 88 >> 3) == (1, 11) and 88 >> 3 >= 10
    assert all(P[s] % 128 for s in SHAPES)                   # every displaced pyramid has padding lanes
    for s in ("Sc", "Sd"):                                   # these two hold every placement in every case
        assert placed_budget(s) == len(placements(s)[1]), (s, len(placements(s)[1]))
    for s, lo in (("Sb", 64), ("Sc", 384)):                  # placed pixels in the last, partly filled wave
        for k in KINDS:
            assert bool(make_coords(s, k)[1][0, lo:].all())
    for s in ("Sa", "Sd"):                                   # the two items of a batch hold different data
        n = P[s] * (SHAPES[s][1] * SHAPES[s][2])
        for cls in ("unit",):
            l0 = make_pyramid(s, cls)[0].reshape(2, -1)
            assert l0.shape[1] == n and not torch.equal(l0[0], l0[1])
        for k in KINDS:
            c = make_coords(s, k)[0]
            assert not torch.equal(torch.nan_to_num(c[0]), torch.nan_to_num(c[1]))
    assert sorted({c[0] for c in CASES}) == sorted(SHAPES) and len(CASES) == len(set(CASES)) == 18
    assert {c[:2] for c in CASES if c[2] == "spread"} == {(s, k) for s in ("Sb", "Sd") for k in KINDS}
    assert {(c[0], c[2]) for c in FUSED_CASES} == {("Sb", "unit"), ("Sc", "unit"), ("Sb", "spread"), ("Sd", "spread")}
    for s, cls in {(c[0], c[2]) for c in FUSED_CASES}:
        assert {c[3:] for c in FUSED_CASES if (c[0], c[2]) == (s, cls)} == {(0, "none"), (68, "relu")}
    assert 0 + 256 >= 68 and 68 + 256 == 324


def test_coordinates_are_normal_and_values_below_the_guard():
    for s in SHAPES:
        for k in KINDS:
            c = make_coords(s, k)[0]
            fin = c[torch.isfinite(c)]
            tiny = fin[(fin != 0) & (fin.abs() < 1.0)]
            assert float(tiny.abs().min()) * 2.0 ** -3 >= 2.0 ** -126            # no subnormal at any level
    for s, cls in sorted({(c[0], c[2]) for c in CASES}):
        mx = max(float(t.abs().max()) for t in make_pyramid(s, cls))
        assert mx * ASC < F16_GUARD, (s, cls, mx)
    sp = make_pyramid("Sd", "spread")[0].abs()
    assert float(sp.max()) > 2.0 ** 7 and float(sp.median()) < 2.0 ** -1 and float(sp.min()) < 2.0 ** -12


def axis_classes(xs, n, R, ax, c32):
    """Class name -> bool tensor over the pixels, from the reference's integer window origin along one axis."""
    WIN = 2 * R + 2
    fl = xs + R
    return {
        "A": (xs >= 0) & (xs + WIN <= n),
        "B": (xs < 0) & (xs + WIN > 0) & (xs + WIN <= n),
        "C": (xs >= 0) & (xs < n) & (xs + WIN > n),
        "BC": (xs < 0) & (xs + WIN > n),
        "Dl": xs + WIN - 1 == 0,
        "Df": xs == n - 1,
        "El": xs + WIN == 0,
        "Eh": xs == n,
        "F0": (ax == 0) & (fl == 0),
        "Fn": (ax == 0) & (fl == n - 1),
        "Fh": ax == 0.5,
        "G": (c32 < 0) & (c32 > -2.0 ** -25),
    }


def realisable(n, R):
    WIN = 2 * R + 2
    r = {"Dl", "Df", "El", "Eh", "F0", "Fn", "Fh", "G"}
    if n >= WIN:
        r.add("A")
    if n >= WIN - 1:
        r |= {"B", "C"}
    else:
        r.add("BC")
    return r


def test_placed_coordinates_reach_every_class():
    """A condition on the inputs: per level, axis and radius, every realisable class occurs - with the other axis's window
    on the plane, so that the class shows in a non-zero tap (El / Eh: all taps are zero, no such condition) - in a ragged
    shape (Sb or Sc) and in Sd; class H (x alone, y alone, both; seven values) occurs in EVERY case; class G really rounds
    ax to 1 in float32; the fast row path of load_row is taken in x at every level of Sd, at both radii."""
    hit = {}
    for case in CASES:
        shape, kind, cls = case
        if cls != "unit":
            continue                                          # (the coordinates do not depend on the value class)
        B, H8, W8 = SHAPES[shape]
        coords, _ = make_coords(shape, kind)
        cx0, cy0 = coords[:, 0].reshape(-1), coords[:, 1].reshape(-1)
        for v in HUGE:
            same = (lambda t: torch.isnan(t) if v != v else t == v)
            okx, oky = torch.isfinite(cx0) & (cx0.abs() < 1e4), torch.isfinite(cy0) & (cy0.abs() < 1e4)
            assert bool((same(cx0) & oky).any()) and bool((same(cy0) & okx).any()) and bool((same(cx0) & same(cy0)).any()), (case, v)
        for R in (4, 3):
            WIN = 2 * R + 2
            org = model(case)[R]["origins"]
            for l in range(4):
                Hl, Wl = H8 >> l, W8 >> l
                xs, ys, ax, ay, cx32, cy32 = org[l]
                on_x, on_y = (xs + WIN > 0) & (xs < Wl), (ys + WIN > 0) & (ys < Hl)
                for axis, cl, other in (("x", axis_classes(xs, Wl, R, ax, cx32), on_y), ("y", axis_classes(ys, Hl, R, ay, cy32), on_x)):
                    for name, where in cl.items():
                        if bool((where if name in ("El", "Eh") else where & other).any()):
                            hit.setdefault(("ragged" if shape in ("Sb", "Sc") else shape, R, l, axis), set()).add(name)
                g = axis_classes(xs, Wl, R, ax, cx32)["G"]
                assert bool(((cx32[g] - torch.floor(cx32[g])) == 1.0).all()) and bool((ax[g] < 1.0).all())
    for group in ("ragged", "Sd"):
        H8, W8 = (12, 88) if group == "Sd" else (None, None)
        for R in (4, 3):
            for l in range(4):
                for axis in ("x", "y"):
                    if group == "Sd":
                        need = realisable((W8 if axis == "x" else H8) >> l, R)
                    else:       # what Sb or Sc can realise
                        need = set().union(*(realisable((SHAPES[s][2] if axis == "x" else SHAPES[s][1]) >> l, R) for s in ("Sb", "Sc")))
                    got = hit.get((group, R, l, axis), set())
                    assert need <= got, (group, R, l, axis, sorted(need - got))
    for R in (4, 3):
        for l in range(4):
            assert "A" in hit[("Sd", R, l, "x")]             # load_row's 16-byte path
    assert "A" not in realisable(11 >> 1, 3) and "BC" in realisable(8 >> 1, 4)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fp32_evaluation_holds_the_gate(case):
    """torch's float32 evaluation of the same formula on the CPU (separately rounded products and sums: more roundings than
    the kernels' fma chain) stays inside the gate on every element, both radii; a tap wholly outside is exactly 0."""
    shape, kind, cls = case
    pyr, (coords, _) = make_pyramid(shape, cls), make_coords(shape, kind)
    for R in (4, 3):
        md = model(case)[R]
        got, _, _ = lookup(pyr, coords, R, dtype=torch.float32)
        assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        err = (got.double() - md["ref"]).abs()
        r, bad = worst(err, md["gate"])
        print("FP32 %s R = %d: %.3f of the gate (%.2f eps m)" % (case_id(case), R, r, r * MARGIN * K_LOOKUP))
        assert bad == 0, (case, R, r)
        assert bool((md["m"] == 0).any()) and bool((got[md["m"] == 0] == 0).all())


def test_gate_has_teeth():
    """Each mutation of the float64 reference, evaluated at the module's own inputs (all 18 cases, radius 4), leaves the
    gate somewhere.  Largest error / gate over the elements with a non-zero gate, measured on the CPU: ij swapped 2.6e12,
    origin + 1 in x 1.6e13, trunc for floor 1.2e11, border clamp 1.1e6, neighbour's plane 1.1e12 (the spread class: a large
    cell where the reference blends small ones); no clamp: NaN (inf - inf) where the reference is 0; the smallest excess
    is the perturbed fraction's, ax + 2^-18: 8.0 = 2^-18 |a01 - a00| against 2^-20 m at a01 = -a00.
    Scale after clamp: identical to the reference at every element (asserted) - whatever the clamp touches lies at least
    1e6 / 8 cells outside every plane at either order, and +-1e5 is clamped at neither."""
    ratios = {}
    for case in CASES:
        shape, kind, cls = case
        pyr, (coords, _) = make_pyramid(shape, cls), make_coords(shape, kind)
        md = model(case)[4]
        for mut in MUTATIONS:
            got, _, _ = lookup(pyr, coords, 4, mut=mut)
            if mut == "no clamp":
                r = float("inf") if bool((~torch.isfinite(got) & torch.isfinite(md["ref"])).any()) else 0.0
            else:
                r, _ = worst((got - md["ref"]).abs(), md["gate"])
            ratios[mut] = max(ratios.get(mut, 0.0), r)
        same, _, _ = lookup(pyr, coords, 4, mut="scale after clamp")
        assert torch.equal(same, md["ref"]), case
    print("TEETH " + ", ".join("%s %.3g" % kv for kv in ratios.items()))
    for mut, r in ratios.items():
        assert r > 1.0, (mut, ratios)


# ------------------------------------------------------------------------------------------------
# GPU


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as o
    assert torch.cuda.is_available()
    return o


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def sentinel_dest(B, C, H8, W8):
    """A channel slice of a wider sentinel-filled fp32 tensor -> (wide, the slice)."""
    wide = torch.full((B, PAD_LO + C + PAD_HI, H8, W8), SENT, device="cuda")
    return wide, wide[:, PAD_LO:PAD_LO + C]


def assert_sentinels(tag, wide, C):
    s = bits(torch.tensor([SENT]))[0].item()
    assert bool((bits(wide[:, :PAD_LO]) == s).all()) and bool((bits(wide[:, PAD_LO + C:]) == s).all()), tag + ": wrote outside its channels"


def sentinel_dest16(ops, B, C, H8, W8):
    """The same for a pre-split destination: one sentinel octet on each side."""
    assert C % 8 == 0
    wide = torch.full((B, C // 8 + 2, 2, H8, W8, 4), SENT16, dtype=torch.int32, device="cuda")
    return wide, ops.S16(wide, C + 16).channels(8, 8 + C)


def assert_sentinels16(tag, wide):
    assert bool((wide[:, 0] == SENT16).all()) and bool((wide[:, -1] == SENT16).all()), tag + ": wrote outside its octets"


def s16_halves(s16):
    """ops.S16 -> (hi, lo) float16 CPU tensors (B, 8 O, H, W)."""
    d = s16.data.contiguous().cpu()
    B, Oc, _, H, W, _ = d.shape
    h = d.view(torch.float16).view(B, Oc, 2, H, W, 8)
    return tuple(h[:, :, t].permute(0, 1, 4, 2, 3).reshape(B, Oc * 8, H, W) for t in (0, 1))


def s16_order(v):
    """(B, 324, H, W) in the reference's channel order l 81 + i 9 + j -> (B, 352, H, W) in L4's l 88 + j 9 + i, tails zero."""
    B, _, H, W = v.shape
    out = torch.zeros(B, 4, S16_LEVEL_CHANNELS, H, W, dtype=v.dtype)
    out[:, :, :81] = v.reshape(B, 4, 9, 9, H, W).transpose(2, 3).reshape(B, 4, 81, H, W)
    return out.reshape(B, 4 * S16_LEVEL_CHANNELS, H, W)


def ref_order(v):
    """The inverse of s16_order, tails dropped."""
    B, _, H, W = v.shape
    return v.reshape(B, 4, S16_LEVEL_CHANNELS, H, W)[:, :, :81].reshape(B, 4, 9, 9, H, W).transpose(2, 3).reshape(B, 324, H, W)


def device_inputs(ops, shape, kind, cls):
    B, H8, W8 = SHAPES[shape]
    P = H8 * W8
    pyr = [dev(p) for p in make_pyramid(shape, cls)]
    coords = dev(make_coords(shape, kind)[0])
    dp = ops.DispPyramid.from_rowmajor(pyr, B, H8, W8)
    assert ops.corr_disp_supported(H8, W8) and P % 128
    for l, t in enumerate(dp.levels):                        # the padding lanes are inputs: no finite result may depend on them
        assert tuple(t.shape) == (B, -(-P // 128), H8 >> l, W8 >> l, 128)
        t[:, -1, :, :, P % 128:] = float("nan")
    back = dp.to_rowmajor()
    assert all(torch.equal(a, b) for a, b in zip(back, pyr))
    return pyr, coords, dp


def within(tag, got, ref, gate):
    assert got.shape == ref.shape, (tag, got.shape)
    assert bool(torch.isfinite(got).all()), tag + ": not finite"
    r, bad = worst((got.double() - ref).abs(), gate)
    print("RATIO %s: %.3f" % (tag, r))
    assert bad == 0, "%s: %d elements outside the gate, worst error / gate = %.3f" % (tag, bad, r)


@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_lookup_route_vs_float64(ops, case):
    shape, kind, cls = case
    B, H8, W8 = SHAPES[shape]
    tag = case_id(case)
    md = model(case)
    pyr, coords, dp = device_inputs(ops, shape, kind, cls)
    ops.guard_tripped()
    # L1, L3 (radius 4, fp32) and L2 (radius 3)
    w1, o1 = sentinel_dest(B, 324, H8, W8)
    assert ops.corr_lookup(pyr, coords, out=o1) is o1
    assert_sentinels("L1 " + tag, w1, 324)
    w3, o3 = sentinel_dest(B, 324, H8, W8)
    ops.corr_lookup(dp, coords, out=o3)
    assert_sentinels("L3 " + tag, w3, 324)
    w2, o2 = sentinel_dest(B, 196, H8, W8)
    ops.corr_lookup(pyr, coords, out=o2, radius=3)
    assert_sentinels("L2 " + tag, w2, 196)
    # L4
    w4, o4 = sentinel_dest16(ops, B, 4 * S16_LEVEL_CHANNELS, H8, W8)
    ops.corr_lookup_s16(dp, coords, o4)
    assert not ops.guard_tripped(), "L4 %s: range guard" % tag
    assert_sentinels16("L4 " + tag, w4)
    v1, v2, v3 = o1.cpu(), o2.cpu(), o3.cpu()
    hi4, lo4 = s16_halves(o4)
    within("L1 " + tag, v1, md[4]["ref"], md[4]["gate"])
    within("L3 " + tag, v3, md[4]["ref"], md[4]["gate"])
    within("L2 " + tag, v2, md[3]["ref"], md[3]["gate"])
    dec4 = ref_order((hi4.double() + lo4.double()) / ASC)
    within("L4 " + tag, dec4, md[4]["ref"], md[4]["gate"] + s16_term(md[4]["ref"]))
    # the promised identities, bit for bit
    assert same_bits(v3, v1), "%s: L3 differs from L1 in %d elements" % (tag, int((bits(v3) != bits(v1)).sum()))
    sub = v1.reshape(B, 4, 9, 9, H8, W8)[:, :, 1:8, 1:8].reshape(B, 196, H8, W8)
    assert same_bits(v2, sub), "%s: L2 differs from L1's inner taps in %d elements" % (tag, int((bits(v2) != bits(sub)).sum()))
    x = s16_order(v3) * ASC
    hi = x.half()
    lo = (x - hi.float()).half()
    assert same_bits(hi4, hi), "%s: L4 hi is not fp16(16 L3) in %d elements" % (tag, int((bits(hi4) != bits(hi)).sum()))
    assert same_bits(lo4, lo), "%s: L4 lo is not fp16(16 L3 - hi) in %d elements" % (tag, int((bits(lo4) != bits(lo)).sum()))
    tails = torch.cat([bits(t).reshape(B, 4, S16_LEVEL_CHANNELS, H8, W8)[:, :, 81:] for t in (hi4, lo4)])
    assert bool((tails == 0).all()), tag + ": L4 tail channels"
    zero = md[4]["m"] == 0
    assert bool(zero.any()) and bool((v1[zero] == 0).all()) and bool((v3[zero] == 0).all()) and bool((dec4[zero] == 0).all())


@gpu
@pytest.mark.parametrize("case", FUSED_CASES, ids=case_id)
def test_fused_lookup_picks_one_tap(ops, case):
    """L5 through a one-hot convc1 weight: w[c, t0 + c] = 1, zero bias: output channel c is tap t0 + c of the reference (its
    positive part under ACT_RELU), fp32 and pre-split destination in one call.  Whether the fp32 result equals the decode
    of L4's taps exactly is printed, not gated (2026-10-20: it does, in every case)."""
    shape, kind, cls, t0, act = case
    B, H8, W8 = SHAPES[shape]
    tag = case_id(case)
    md = model((shape, kind, cls))[4]
    pyr, coords, dp = device_inputs(ops, shape, kind, cls)
    wgt = torch.zeros(256, 324, 1, 1)
    wgt[torch.arange(256), t0 + torch.arange(256)] = 1.0
    ref, gate = md["ref"][:, t0:t0 + 256], md["gate"][:, t0:t0 + 256]
    if act == "relu":
        ref = ref.clamp(min=0)                               # (1-Lipschitz: the gate of the tap holds for its positive part)
    ops.guard_tripped()
    with ops.conv_mode("f16x3"):
        fused = ops.lookup_fused_weight(dev(wgt))
        assert tuple(fused.shape) == (256, LOOKUP_FUSED_K, 1, 1) and float(fused.sum()) == 256.0
        pk = ops.PackedConv(fused, torch.zeros(256, device="cuda"))
        w32, o32 = sentinel_dest(B, 256, H8, W8)
        w16, o16 = sentinel_dest16(ops, B, 256, H8, W8)
        ops.corr_lookup_convc1(dp, coords, pk, out16=o16, out=o32, act=ops.ACT_RELU if act == "relu" else ops.ACT_NONE)
        assert not ops.guard_tripped(), "L5 %s: range guard" % tag
        l16 = ops.S16.empty(B, 4 * S16_LEVEL_CHANNELS, H8, W8, coords.device, zero=True)
        ops.corr_lookup_s16(dp, coords, l16)
    assert_sentinels("L5 fp32 " + tag, w32, 256)
    assert_sentinels16("L5 S16 " + tag, w16)
    got32 = o32.cpu()
    hi, lo = s16_halves(o16)
    got16 = (hi.double() + lo.double()) / ASC
    within("L5 fp32 " + tag, got32, ref, gate + s16_term(ref))
    within("L5 S16 " + tag, got16, ref, gate + 2 * s16_term(ref))
    h4, l4 = s16_halves(l16)
    taps = ref_order((h4.double() + l4.double()) / ASC)[:, t0:t0 + 256]
    if act == "relu":
        taps = taps.clamp(min=0)
    print("EXACT %s: L5 fp32 == decode of L4: %s" % (tag, bool((got32.double() == taps).all())))
    zero = md["m"][:, t0:t0 + 256] == 0
    assert bool(zero.any()) and bool((got32[zero] == 0).all()) and bool((got16[zero] == 0).all())
