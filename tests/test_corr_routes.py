"""Every route of the all-pairs correlation volume and its 4-level pyramid (csrc/corr_volume.hip, corr_disp_gemm_kernel /
corr_disp_ring_kernel / accflow_launch_corr_disp_direct in csrc/corr_gemm.hip, corr_disp_store2 in csrc/conv_common.h,
the pooling kernels of csrc/corr_volume.hip and csrc/corr_disp.hip) against a float64 reference written HERE:
level 0 = f1^T f2 / sqrt(C), levels 1..3 = 2x2 means with floor sizes, pool of pool - plain torch on the CPU.

Routes (restated by corr_route below as a function of (entry, mode, C, H8, W8); pinned to the sources by
test_route_table_is_the_one_in_the_sources):
         entry                                    level 0                                          levels 1..3
    V1   ops.corr_volume, f32                     gemm_atb_f32_kernel                              corr_pool_kernel
    V2/3 ops.corr_volume, bf16x6 / bf16x3         1x1 convolution through accflow_conv2d_f32       corr_pool_kernel
         (an f16x3 request runs bf16x6)           over accflow_pack_kmajor
    V4   ops.corr_volume_disp, C % 16 != 0 or     accflow_launch_corr_disp_bf16s                   corr_disp_pool_kernel from level 0
         odd W8 (f16x3 -> bf16x6)
    V5/6 ops.corr_volume_disp, direct,            corr_disp_gemm_kernel<3, false> / <2, false>     level 1 in corr_disp_store2, then
         bf16x6 / bf16x3                                                                           corr_disp_pool_kernel from level 1
    V7   ops.corr_volume_disp, direct, f16x3      corr_disp_ring_kernel                            as V5
    V8   ops.corr_pack +                          the kernels of V5 - V7, acc_scale carrying       as V5
         ops.corr_volume_disp_packed, 3 modes     1 / sqrt(C)
Switch-only, not run here: corr_disp_gemm_kernel<2, true> (ACCFLOW_CORR_GEMM=regs, read once per process).

Designed operand arithmetic (what E_split evaluates in float64 with exact sums; cs = fp32(1.0f / sqrtf(C))):
    f32 (V1)            the reference itself: E_split = 0.
    bf16x6              three bf16 terms per operand (round to nearest, residual in fp32), the six products t_a + t_b <= 2.
    bf16x3              two terms, the products 00, 01, 10.
      placement of cs   per pair (V2 - V6): the query map is fp32(x cs) BEFORE the split; packed (V8): both maps are split as
                        they are and the accumulator is multiplied by cs.
    f16x3, per pair     (V7) query map fp32(x fp32(2^4 cs)), target map x 2^4, both split as fp16 hi + lo with
                        lo = fp16(a - hi), subnormals kept; products hi.hi + lo.hi + hi.lo; the sum times 2^-8.
    f16x3, packed       (V8) both maps x 2^4; the sum times fp32(cs / 256).

Gate, per case and per level, on every element (displaced results read through DispPyramid.to_rowmajor()):
    max |got - ref64| <= MARGIN (E32 + E_split),   MARGIN = 4 (tests/test_gma_routes.py)
    E32      max |.| error, against float64, of the SAME pyramid evaluated by torch in float32 on the CPU;
    E_split  max |.| error, against float64, of the float64 pyramid of the designed level 0 above.
No gate is a constant and none is taken from what the kernels return.

Further checks of every GPU case:
    pooling is exact   for l = 1..3 the stored level l equals (((a + b) + c) + d) * 0.25 evaluated in float32 on the CPU from the
                       route's OWN stored level l - 1 (floor sizes), bit for bit: the reference's pool of pool, and the order
                       all three pooling implementations document (corr_pool_kernel, corr_disp_pool_kernel, the level 1 that
                       corr_disp_store2 emits from registers - which scales each accumulator before it sums, so that the
                       identity holds for an accumulator scale that is no power of two: V8 at C = 48, 96, 128);
    nothing else is    displaced entries: the C-ABI called on level buffers pre-filled with a sentinel, with a sentinel band of
    written            1024 floats on each side of every buffer: bands unchanged, lanes p >= P of the last 128-pixel block
                       unchanged, everything else equal to the ops call bit for bit;
    shapes and batch   of all levels; with B = 2 (and the 4 pairs of V8) the items use different features;
    guard              quiet after every f16x3 call (all inputs satisfy |x| 2^4 < 65520: asserted on the CPU).

Shapes: Ga 8 x 8, B = 2 (P = 64: half a 128-pixel block, 7 of 8 XCD slots return at once, level 3 is 1 x 1);  Gb 9 x 66,
B = 2 (P = 594: 5 query blocks; odd height: the last target tile has one live row and no level-1 cell; two 64-column target
tiles, the second with 2 live columns);  Gc 24 x 46, B = 1 (P = 1104: 9 query blocks, percol = 2 and 7 empty slots,
P % 128 = 80, one target tile narrower than 64);  Gd 17 x 23, B = 1 (odd width: V1 - V4 only; P % 4 = 3: gemm_atb's scalar
loads).  Depths of the direct routes: C = 16, 48, 96, 128, 256 = 2, 4, 6, 8, 16 steps (nstep % 3 = 2, 1, 0, 2, 1; the ring
kernel with fewer steps than slots; zero-filled reduction rows, Kpad > C, at 16 and 48 - 96 is three whole 32-row slabs);
of the others: C = 20, 40 (Kpad = 32, 64) and 256.
Input classes: unit (randn, everywhere), small (randn 2^-6), spread (per-channel factors logspace(-6, 3, C, base = 2)); the
last two on V7 and V8-f16x3 and on one bf16x6 and one bf16x3 direct case, all at (128, Gb).

Not covered: ACCFLOW_CORR_GEMM=regs (above), shapes beyond (24, 46), invalid arguments (tests/test_host_logic.py owns them).

Measured on the MI355X, 2026-10-19, every case passing (each under half a second) - largest error / gate per route, over all
levels and classes:
    V1 0.49   V2 0.33   V3 0.25   V4 0.39   V5 0.38   V6 0.25   V7 0.22   V8 0.47 (bf16x6), 0.24 (bf16x3), 0.41 (f16x3)
    small / spread at (128, Gb): V5 0.21 / 0.19, V6 0.24 / 0.25, V7 0.20 / 0.17, V8-f16x3 0.15 / 0.16
(The bf16x3 rows sit at 1 / MARGIN: E_split is their whole error.  The subnormal-lo regime of the per-pair fp16 split shows
in V7's E_split of the small class - 9.0e-10 against 3.7e-10 on the packed route - and stays inside its gate.)
With corr_disp_store2 as it was before this module (sums first, one scale), the eleven V8 cases at C = 48 and 128 fail the
exact-pooling check at level 1 and the three at C = 256 pass; every float64 gate holds either way.
Nobody had measured these ratios before the module was written; no gate, margin, shape or input was chosen from them.  The
teeth figures quoted at the teeth test are from the CPU.
"""
import functools
import math
import os
import re

import pytest
import torch

from test_gma_routes import MARGIN, TEETH, split_f16, split_bf16, f32, gen, dev

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASHIFT = 4                      # ACCFLOW_F16_ASHIFT (pinned by test_route_table_is_the_one_in_the_sources)
ASC = float(1 << ASHIFT)
F16_GUARD = 65520.0
MODE = {"f32": 0, "bf16x3": 2, "bf16x6": 3, "f16x3": 4}
GRIDS = {"Ga": (2, 8, 8), "Gb": (2, 9, 66), "Gc": (1, 24, 46), "Gd": (1, 17, 23)}     # name -> (B, H8, W8)
PACK_FRAMES = 3
PACK_PAIRS = ((1, 0), (2, 0), (0, 2), (1, 1))      # (query frame, target frame): a reversed pair and a frame with itself
SENT = -777.25
BAND = 1024
SWITCH_ONLY = "corr_disp_gemm_kernel<2, true>"


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------
# the host's dispatch, restated; test_route_table_is_the_one_in_the_sources pins it


def kpad(C):
    return cdiv(C, 32) * 32


def corr_route(entry, mode, C, H8, W8):
    """-> (row, arithmetic, placement of 1 / sqrt(C), level-0 kernel, where levels 1..3 come from).
    entry: "volume" = ops.corr_volume, "disp" = ops.corr_volume_disp, "packed" = ops.corr_pack + corr_volume_disp_packed."""
    if entry == "volume":
        if mode == "f32":
            return "V1", "f32", None, "gemm_atb_f32_kernel", "corr_pool_kernel"
        arith = "bf16x6" if mode == "f16x3" else mode
        return ("V2" if arith == "bf16x6" else "V3"), arith, "query", "accflow_conv2d_f32", "corr_pool_kernel"
    assert mode in ("bf16x6", "bf16x3", "f16x3")
    direct = C >= 16 and C % 16 == 0 and W8 % 2 == 0
    if entry == "packed":
        assert direct, "ops.corr_pack refuses these"
    elif not direct:
        return "V4", ("bf16x6" if mode == "f16x3" else mode), "query", "accflow_launch_corr_disp_bf16s", "corr_disp_pool_kernel"
    kernel = {"bf16x6": "corr_disp_gemm_kernel<3, false>", "bf16x3": "corr_disp_gemm_kernel<2, false>", "f16x3": "corr_disp_ring_kernel"}[mode]
    if entry == "packed":
        return "V8", mode, "acc", kernel, "corr_disp_store2"
    return {"bf16x6": "V5", "bf16x3": "V6", "f16x3": "V7"}[mode], mode, "query", kernel, "corr_disp_store2"


def direct_geometry(C, H8, W8):
    """The launch of accflow_launch_corr_disp_direct and what its kernels derive from it."""
    P = H8 * W8
    npb = cdiv(P, 128)
    percol = cdiv(npb, 8)
    nstep = kpad(C) // 16
    return {"npb": npb, "percol": percol, "empty_slots": 8 * percol - npb, "nstep": nstep, "kfill": kpad(C) > C,
            "tiles_x": cdiv(W8, 64), "last_tile_cols": W8 - 64 * (cdiv(W8, 64) - 1), "odd_height": H8 % 2 == 1,
            "tail_lanes": P % 128}


def _function_body(text, head):
    """The source text of the function whose definition starts with `head`, up to the closing brace in column 0."""
    i = text.index(head)
    return text[i:text.index("\n}\n", i)]


def test_route_table_is_the_one_in_the_sources():
    """Every launch line of accflow_launch_corr_disp_direct and every branch of accflow_corr_level0_bf16s and corr_volume_impl
    has a row of the table above or is the named switch-only entry; the conditions corr_route restates stand in the sources."""
    def src(*p):
        return open(os.path.join(ROOT, *p)).read()
    csrc = ("accflow_amd", "csrc")
    assert "#define ACCFLOW_F16_ASHIFT %d\n" % ASHIFT in src("include", "accflow_hip.h")
    assert "return (K + 31) / 32 * 32;" in src(*csrc, "conv_plan.cpp")
    direct, vol, disp = src(*csrc, "corr_gemm.hip"), src(*csrc, "corr_volume.hip"), src(*csrc, "corr_disp.hip")
    common, bf16s = src(*csrc, "conv_common.h"), src(*csrc, "conv2d_bf16s.hip")
    rows = {r: corr_route(*a)[3] for r, a in (("V5", ("disp", "bf16x6", 128, 8, 8)), ("V6", ("disp", "bf16x3", 128, 8, 8)),
                                              ("V7", ("disp", "f16x3", 128, 8, 8)))}
    # accflow_launch_corr_disp_direct: four launch lines = V7, the switch-only kernel, V6, V5 (V8 launches the same three)
    launch = _function_body(direct, "int accflow_launch_corr_disp_direct(const accflow_conv_desc& d, hipStream_t st) {")
    kernels = re.findall(r"hipLaunchKernelGGL\(\(?([a-z_0-9]+(?:<[^>]*>)?)\)?, grid, dim3\(256\), 0, st, d\);", launch)
    assert launch.count("hipLaunchKernelGGL(") == len(kernels) == 4
    assert sorted(kernels) == sorted(list(rows.values()) + [SWITCH_ONLY])
    assert 'static const bool ringk = [] { const char* e = getenv("ACCFLOW_CORR_GEMM"); return !(e && e[0] == \'r\'); }();' in launch
    assert "if (d.mode == ACCFLOW_CONV_F16X3 && d.wpatch16 && ringk) {" in launch
    assert "else if (d.mode == ACCFLOW_CONV_BF16X3) hipLaunchKernelGGL((corr_disp_gemm_kernel<2, false>)" in launch
    assert "const int nqt = cdiv(d.OH, 2) * cdiv(d.OW, 64);" in launch and "dim3 grid(8 * ((npb + 7) / 8) * nqt);" in launch
    assert direct.count("const int npb = (P + 127) >> 7, percol = (npb + 7) >> 3;") == 2
    assert direct.count("const int nstep = d.Kpad / 16;") == 2
    assert "constexpr int PD = NT == 2 ? 2 : 1;" in direct and "for (int step = 0; step < nstep; step += 3) {" in direct
    assert "constexpr int CRING_SLOTS = 3;" in direct
    assert "constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};" in direct      # bf16: t_a + t_b <= 2 / the last three
    assert "constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};" in direct                         # ring: lo.hi, hi.lo, hi.hi
    assert direct.count("corr_disp_store2(d, acc,") == 2
    # accflow_corr_level0_bf16s: three ways out = direct (V5 - V7), displaced 1x1 convolution (V4), row-major convolution (V2, V3)
    lvl0 = _function_body(vol, "int accflow_corr_level0_bf16s(")
    assert "const bool direct = disp && C >= 16 && C % 16 == 0 && W8 % 2 == 0 && lvl1;" in lvl0
    assert "const bool f16 = direct && mode == ACCFLOW_CONV_F16X3;" in lvl0
    assert "if (mode == ACCFLOW_CONV_F16X3 && !f16) mode = ACCFLOW_CONV_BF16X6;" in lvl0
    assert "const float cscale = 1.0f / sqrtf((float)C);" in lvl0
    assert "const float fs = f16 ? ldexpf(1.0f, ACCFLOW_F16_ASHIFT) : 1.0f;" in lvl0
    assert "wsplit, cscale * fs, f16 ? 1 : 0, guard, st);" in lvl0 and "bsplit, fs, f16 ? 1 : 0, guard, st);" in lvl0
    assert "if (f16) { d.wpatch16 = wsplit; d.guard = guard; d.acc_scale = 1.0f / (fs * fs); }" in lvl0
    outs = [lvl0.count(s) for s in ("= accflow_launch_corr_disp_direct(d, st);", "= accflow_launch_corr_disp_bf16s(d, st);",
                                    "= accflow_conv2d_f32(&d, st);")]
    assert outs == [1, 1, 1] and lvl0.count("const int rc = ") == 3
    assert lvl0.index("if (direct) {") < lvl0.index("if (disp) {") < lvl0.index("accflow_conv2d_f32(&d, st)")
    assert "if (d.mode == ACCFLOW_CONV_BF16X6) hipLaunchKernelGGL((conv2d_bf16s_kernel<2, 2, 3, 16, true>)" in bf16s
    assert "else hipLaunchKernelGGL((conv2d_bf16s_kernel<2, 2, 2, 32, true>)" in bf16s
    # corr_volume_impl: two level-0 branches (V2 / V3, V1) and one pooling launch
    impl = _function_body(vol, "static int corr_volume_impl(")
    assert "if (mode == ACCFLOW_CONV_F16X3) mode = ACCFLOW_CONV_BF16X6;" in impl
    assert "if (ws && mode != ACCFLOW_CONV_F32) {" in impl
    assert impl.count("rc = ") == 2 and impl.count("rc = accflow_corr_level0_bf16s(") == 1 and impl.count("rc = accflow_gemm_atb_f32(") == 1
    assert impl.count("hipLaunchKernelGGL(") == 1 and "hipLaunchKernelGGL(corr_pool_kernel," in impl
    assert "const bool vecA = (M & 3) == 0, vecB = (N & 3) == 0;" in vol
    # the displaced entry pools from level 1 when the GEMM emitted it; the packed entry (V8) always does
    dentry = _function_body(vol, 'extern "C" int accflow_corr_volume_disp_f32(')
    assert "return accflow_corr_disp_pool_from(lvl0, lvl1, lvl2, lvl3, B, H8, W8, lvl1_done ? 1 : 0, as_stream(stream));" in dentry
    packed = _function_body(vol, 'extern "C" int accflow_corr_volume_disp_packed_f32(')
    assert "d.acc_scale = (1.0f / sqrtf((float)C)) / (fs * fs);" in packed
    assert packed.count("accflow_launch_corr_disp_direct(d, st);") == 1
    assert "return accflow_corr_disp_pool_from(lvl0, lvl1, lvl2, lvl3, B, H8, W8, 1, st);" in packed
    assert "C < 16 || (C % 16) || (W8 & 1) ||" in packed and "C < 16 || (C % 16) || (W8 & 1) ||" in _function_body(vol, 'extern "C" int accflow_corr_pack_f32(')
    # the three pooling implementations and the order they document
    assert "const float v = (((a + b) + c) + d) * 0.25f;" in vol
    assert "= (((a + b) + c) + d) * 0.25f;" in disp
    assert "for (int l = first; l < 3; ++l) {" in disp
    store2 = common[common.index("__device__ __forceinline__ void corr_disp_store2("):]
    assert "const float osc = d.acc_scale != 0.0f ? d.acc_scale : 1.0f;" in store2
    assert "const float v = T[lane * DISP_PITCH + pl] * osc;" in store2
    assert "S0[k * DISP_PITCH + pl] = a + b;" in store2 and "const float v = ((S0[k * DISP_PITCH + pl] + a) + b) * 0.25f;" in store2
    assert store2.count("* osc") == 3       # the level-0 value and the two taps of a half, each scaled before any sum


# ------------------------------------------------------------------------------------------------
# the case table

CASES = []      # (row, entry, mode, C, grid, class)


def _case(row, entry, mode, C, grid, cls="unit"):
    CASES.append((row, entry, mode, C, grid, cls))


for _C, _g in ((20, "Gd"), (48, "Ga"), (128, "Gb"), (256, "Gc")):
    _case("V1", "volume", "f32", _C, _g)
for _row, _mode in (("V2", "bf16x6"), ("V3", "bf16x3")):
    for _C, _g in ((20, "Gd"), (96, "Gb"), (256, "Gc")):
        _case(_row, "volume", _mode, _C, _g)
_case("V2", "volume", "f16x3", 96, "Gb")                       # must return the bf16x6 bits
for _mode in ("bf16x6", "bf16x3", "f16x3"):
    for _C, _g in ((40, "Gb"), (256, "Gd"), (20, "Ga")):
        _case("V4", "disp", _mode, _C, _g)
DIRECT_DEPTHS = (16, 48, 96, 128, 256)
for _row, _mode in (("V5", "bf16x6"), ("V6", "bf16x3"), ("V7", "f16x3")):
    for _C in DIRECT_DEPTHS:
        _case(_row, "disp", _mode, _C, "Gb")
    _case(_row, "disp", _mode, 128, "Ga")
    _case(_row, "disp", _mode, 128, "Gc")
for _mode in ("bf16x6", "bf16x3", "f16x3"):
    for _C, _g in ((48, "Gb"), (128, "Gb"), (128, "Gc"), (256, "Ga")):
        _case("V8", "packed", _mode, _C, _g)
for _cls in ("small", "spread"):
    _case("V7", "disp", "f16x3", 128, "Gb", _cls)
    _case("V8", "packed", "f16x3", 128, "Gb", _cls)
    _case("V5", "disp", "bf16x6", 128, "Gb", _cls)
    _case("V6", "disp", "bf16x3", 128, "Gb", _cls)


def case_id(c):
    return "-".join(map(str, c))


# ------------------------------------------------------------------------------------------------
# seeded inputs, the reference and the float64 evaluations of the designed arithmetic (CPU)


def _seed(*key):
    s = 23
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % 1000003
    return s


def make_maps(cls, n, C, h, w):
    """n feature maps (n, C, h, w) float32 of an input class."""
    x = torch.randn(n, C, h, w, generator=gen(_seed("fmaps", cls, n, C, h, w)))
    if cls == "small":
        x = x * 2.0 ** -6
    elif cls == "spread":
        x = x * torch.logspace(-6, 3, C, base=2)[None, :, None, None]
    else:
        assert cls == "unit"
    return x.contiguous()


def case_inputs(case):
    """-> (f1, f2, frames): the query and target maps (B, C, h, w) of the B pairs; frames (F, C, h, w) for the packed entry."""
    row, entry, mode, C, grid, cls = case
    B, h, w = GRIDS[grid]
    if entry == "packed":
        fm = make_maps(cls, PACK_FRAMES, C, h, w)
        return fm[[p[0] for p in PACK_PAIRS]].contiguous(), fm[[p[1] for p in PACK_PAIRS]].contiguous(), fm
    x = make_maps(cls, 2 * B, C, h, w)
    return x[:B].contiguous(), x[B:].contiguous(), None


def dots(a, b):
    """sum_c a[b][c][i] b[b][c][j]"""
    return torch.einsum("bci,bcj->bij", a, b)


def pyramid(l0):
    """[level 0..3] of a (B, P, h, w) level 0 in ITS dtype: (((a + b) + c) + d) * 0.25 over the 2x2 cells, floor sizes, pool of
    pool - the reference (float64), the E32 yardstick (float32) and the exact-pooling check (float32, one level at a time)."""
    out = [l0]
    for _ in range(3):
        out.append(pool(out[-1]))
    return out


def pool(x):
    h2, w2 = x.shape[-2] // 2, x.shape[-1] // 2
    x = x[..., :2 * h2, :2 * w2]
    a, b, c, d = x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]
    return (((a + b) + c) + d) * 0.25


def level0_ref64(f1, f2):
    B, C, h, w = f1.shape
    return (dots(f1.reshape(B, C, -1).double(), f2.reshape(B, C, -1).double()) / math.sqrt(C)).view(B, h * w, h, w)


def level0_f32(f1, f2):
    """The reference formula (corr = f1^T f2, corr / sqrt(dim)) by torch in float32 on the CPU."""
    B, C, h, w = f1.shape
    corr = torch.matmul(f1.reshape(B, C, -1).transpose(1, 2), f2.reshape(B, C, -1))
    return (corr / torch.sqrt(torch.tensor(float(C)))).view(B, h * w, h, w)


def cscale32(C):
    """1.0f / sqrtf((float)C)"""
    return torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(C), dtype=torch.float32))


def level0_design(arith, place, f1, f2, fault=None):
    """Float64 level 0 (B, P, h, w) of a route's designed operand arithmetic, exact sums.  fault (the teeth tests): "no lo.hi",
    "no second term", "no third term", "no last step" (the last 16 channels never accumulated)."""
    B, C, h, w = f1.shape
    q, t = f1.reshape(B, C, -1), f2.reshape(B, C, -1)
    if fault == "no last step":
        q = q.clone()
        q[:, C - 16:] = 0.0
    cs = cscale32(C)
    if arith == "f32":
        s = dots(q.double(), t.double()) / math.sqrt(C)
    elif arith == "f16x3":
        if place == "query":
            qh, ql = split_f16(q * (cs * ASC))
            osc = 1.0 / (ASC * ASC)
        else:
            qh, ql = split_f16(q * ASC)
            osc = float(cs / (ASC * ASC))
        th, tl = split_f16(t * ASC)
        s = dots(qh, th + tl)
        if fault != "no lo.hi":
            s = s + dots(ql, th)
        s = s * osc
    else:
        n = 3 if arith == "bf16x6" else 2
        qt, tt = split_bf16(q * cs if place == "query" else q, n), split_bf16(t, n)
        keep = n - 1                                   # products with t_a + t_b <= keep
        if fault == "no second term":
            keep = 0
        elif fault == "no third term":
            keep = min(keep, 1)
        s = 0.0
        for a in range(keep + 1):
            s = s + dots(qt[a], sum(tt[1:keep - a + 1], tt[0]))
        if place == "acc":
            s = s * float(cs)
    return s.view(B, h * w, h, w)


def wrap_one_off(l0):
    """A displaced column index dx = (x2 - x1) mod W8 whose wrap (x2 < x1) lands one cell off: those cells of the row-major
    view hold their left neighbour's value."""
    B, P, h, w = l0.shape
    x1 = torch.arange(P) % w
    wrapped = torch.arange(w)[None, :] < x1[:, None]                       # (P, w)
    return torch.where(wrapped[None, :, None, :], torch.roll(l0, 1, dims=3), l0)


def errs(pyr, ref):
    return [float((a.double() - b).abs().max()) for a, b in zip(pyr, ref)]


@functools.lru_cache(maxsize=2)
def model(case):
    """Reference pyramid, E32, E_split and gate per level of a case."""
    row, entry, mode, C, grid, cls = case
    B, h, w = GRIDS[grid]
    _, arith, place, _, _ = corr_route(entry, mode, C, h, w)
    f1, f2, _ = case_inputs(case)
    ref = pyramid(level0_ref64(f1, f2))
    e32 = errs(pyramid(level0_f32(f1, f2)), ref)
    esplit = [0.0] * 4 if arith == "f32" else errs(pyramid(level0_design(arith, place, f1, f2)), ref)
    gate = [MARGIN * (a + b) for a, b in zip(e32, esplit)]
    return {"ref": ref, "e32": e32, "esplit": esplit, "gate": gate, "arith": arith, "place": place}


# ------------------------------------------------------------------------------------------------
# CPU: coverage, input conditions, teeth, the level-1 order


def test_cases_cover_the_route_table_and_its_edges():
    for c in CASES:
        row, entry, mode, C, grid, cls = c
        B, h, w = GRIDS[grid]
        assert corr_route(entry, mode, C, h, w)[0] == row, c
    assert len(CASES) == len(set(CASES)) == 61
    by = {r: [c for c in CASES if c[0] == r] for r in ("V1", "V2", "V3", "V4", "V5", "V6", "V7", "V8")}
    assert all(by.values())
    assert {c[3:5] for c in by["V1"]} == {(20, "Gd"), (48, "Ga"), (128, "Gb"), (256, "Gc")}
    for r in ("V2", "V3"):
        assert {c[3:5] for c in by[r]} == {(20, "Gd"), (96, "Gb"), (256, "Gc")}
    assert [c for c in by["V2"] if c[2] == "f16x3"] == [("V2", "volume", "f16x3", 96, "Gb", "unit")]
    assert {(c[2],) + c[3:5] for c in by["V4"]} == {(m, C, g) for m in ("bf16x6", "bf16x3", "f16x3") for C, g in ((40, "Gb"), (256, "Gd"), (20, "Ga"))}
    assert {corr_route(*c[1:4], *GRIDS[c[4]][1:])[1] for c in by["V4"]} == {"bf16x6", "bf16x3"}
    for r in ("V5", "V6", "V7"):
        assert {c[3:5] for c in by[r]} == {(C, "Gb") for C in DIRECT_DEPTHS} | {(128, "Ga"), (128, "Gc")}
        assert {c[5] for c in by[r] if c[3:5] == (128, "Gb")} == {"unit", "small", "spread"}
    assert {(c[2],) + c[3:5] for c in by["V8"]} == {(m, C, g) for m in ("bf16x6", "bf16x3", "f16x3")
                                                    for C, g in ((48, "Gb"), (128, "Gb"), (128, "Gc"), (256, "Ga"))}
    assert {c[5] for c in by["V8"] if c[2:5] == ("f16x3", 128, "Gb")} == {"unit", "small", "spread"}
    assert all(c[5] == "unit" for c in CASES if c[3:5] != (128, "Gb"))
    # the edges of the shapes and depths
    geo = {g: direct_geometry(128, *GRIDS[g][1:]) for g in ("Ga", "Gb", "Gc")}
    assert geo["Ga"]["npb"] == 1 and geo["Ga"]["empty_slots"] == 7 and geo["Ga"]["tail_lanes"] == 64 and GRIDS["Ga"][1] >> 3 == 1
    assert geo["Gb"]["npb"] == 5 and geo["Gb"]["odd_height"] and geo["Gb"]["tiles_x"] == 2 and geo["Gb"]["last_tile_cols"] == 2
    assert geo["Gc"]["npb"] == 9 and geo["Gc"]["percol"] == 2 and geo["Gc"]["empty_slots"] == 7 and geo["Gc"]["tail_lanes"] == 80
    assert geo["Gc"]["tiles_x"] == 1 and geo["Gc"]["last_tile_cols"] < 64
    assert GRIDS["Gd"][2] % 2 == 1 and (GRIDS["Gd"][1] * GRIDS["Gd"][2]) % 4 == 3
    steps = [direct_geometry(C, 9, 66)["nstep"] for C in DIRECT_DEPTHS]
    assert steps == [2, 4, 6, 8, 16] and [s % 3 for s in steps] == [2, 1, 0, 2, 1] and steps[0] < 3 <= steps[1]
    assert [direct_geometry(C, 9, 66)["kfill"] for C in DIRECT_DEPTHS] == [True, True, False, False, False]   # (96 = 3 x 32)
    assert {p for p in PACK_PAIRS if p[0] == p[1]} and {p for p in PACK_PAIRS if p[::-1] in PACK_PAIRS and p[0] != p[1]}
    assert max(max(p) for p in PACK_PAIRS) == PACK_FRAMES - 1
    # the scales that are no power of two: where the level-1 emission has to scale before it sums
    assert [C for C in (48, 128, 256) if math.log(C, 4) % 1] == [48, 128]


@pytest.mark.parametrize("cls", ["unit", "small", "spread"])
def test_inputs_stay_below_the_fp16_guard(cls):
    """|x| 2^4 < 65520 for every map of every case (the per-pair query map carries 2^4 / sqrt(C) <= 2^4 / 4)."""
    seen = 0
    for c in CASES:
        if c[5] != cls:
            continue
        f1, f2, fm = case_inputs(c)
        for x in (f1, f2):
            assert float(x.abs().max()) * ASC < F16_GUARD / 64, c       # (far below: a factor 64 to spare)
        seen += 1
    assert seen
    x = make_maps(cls, 2, 128, 9, 66)
    rms = float(x.double().pow(2).mean().sqrt())
    if cls == "small":
        assert abs(rms * 64 - 1) < 0.05
    elif cls == "spread":
        per_c = x.double().pow(2).mean(dim=(0, 2, 3)).sqrt()
        assert float(per_c[0]) < 2.0 ** -5 and float(per_c[-1]) > 2.0 ** 2.5


TEETH_CASES = [c for c in CASES if c[3:5] == (128, "Gb") and c[5] in ("unit", "spread") and c[0] in ("V5", "V6", "V7", "V8")
               and (c[0] != "V8" or c[2] == "f16x3")]
FAULTS = {"f16x3": ("no lo.hi", "no last step", "wrap"), "bf16x3": ("no second term", "no last step", "wrap"),
          "bf16x6": ("no second term", "no last step", "wrap")}


@pytest.mark.parametrize("case", TEETH_CASES, ids=case_id)
def test_gate_has_teeth(case):
    """Each fault, applied to the float64 evaluation of the designed arithmetic, lands >= TEETH = 8 gates from the reference
    at level 0 (and is printed for every level): the dropped lo.hi product of the fp16 split, the dropped second bf16 term
    (bf16x3 and bf16x6), the last 16-deep step never accumulated, one displaced column wrap one cell off.
    The third bf16 term of bf16x6 cannot reach 8 gates: two bf16 terms hold an operand to 2^-18, the gate of a 128-term fp32
    sum is MARGIN E32 ~ 2^-19 of the result - as tests/test_gma_routes.py found for its bf16x6 routes; it is held to
    exceeding the gate at all, and the dropped second term is the bf16x6 fault.  Measured on the CPU at (128, Gb), unit /
    spread, level 0: no lo.hi 107 / 204 (per pair), 45 / 296 (packed); no second term 122 / 90 (bf16x3), 1.4e3 / 4.9e3 (bf16x6);
    no last step 1.8e4 (bf16x3) to 1.4e6; wrap 4.2e4 (bf16x3) to 2.3e6; no third term (bf16x6) 2.7 / 13.5."""
    row, entry, mode, C, grid, cls = case
    m = model(case)
    f1, f2, _ = case_inputs(case)
    ratios = {}
    faults = FAULTS[m["arith"]] + (("no third term",) if m["arith"] == "bf16x6" else ())
    for fault in faults:
        l0 = level0_design(m["arith"], m["place"], f1, f2, None if fault == "wrap" else fault)
        if fault == "wrap":
            l0 = wrap_one_off(l0)
        e = errs(pyramid(l0), m["ref"])
        ratios[fault] = [a / g for a, g in zip(e, m["gate"])]
    print("TEETH %s %s" % (case_id(case), {k: ["%.3g" % r for r in v] for k, v in ratios.items()}))
    for fault, r in ratios.items():
        assert r[0] >= (1.0 if fault == "no third term" else TEETH), (fault, ratios, m["e32"], m["esplit"])


def test_level1_from_unscaled_sums_is_not_the_pool_of_the_scaled_level0():
    """Why the pooling check exists.  Level 0 stores fp32(s osc) for an fp32 accumulator s.  A level 1 computed as
    ((((s_a + s_b) + s_c) + s_d) osc) / 4 - sums first, one scale - equals the pool of the STORED level 0 only when osc is a
    power of two (then the scale commutes with every rounding).  The per-frame packs put 1 / sqrt(C) into osc: a power of two
    only for C a power of four.  In float32 on the CPU, 9 x 66: at C = 48, 96, 128 tens of thousands of level-1 values
    differ; at C = 16 and 256 none.  Scaling each accumulator before the sums (what corr_disp_store2 does) is the pool of the
    stored values by construction."""
    h, w = 9, 66
    for C in DIRECT_DEPTHS:
        fm = make_maps("unit", 2, C, h, w)
        acc = dots(fm[:1].reshape(1, C, -1).double(), fm[1:].reshape(1, C, -1).double()).float().view(1, h * w, h, w)
        osc = cscale32(C) / (ASC * ASC)
        stored = acc * osc
        a, b, c, d = (acc[..., i:8:2, j:66:2] for i in (0, 1) for j in (0, 1))
        sums_first = ((((a + b) + c) + d) * osc) * 0.25
        scaled_first = (((a * osc + b * osc) + c * osc) + d * osc) * 0.25
        assert torch.equal(scaled_first, pool(stored))
        ndiff = int((sums_first != pool(stored)).sum())
        print("LEVEL1 C = %d: %d of %d differ" % (C, ndiff, sums_first.numel()))
        if C in (16, 256):
            assert ndiff == 0
        else:
            assert ndiff > sums_first.numel() // 10


# ------------------------------------------------------------------------------------------------
# GPU


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as o
    assert torch.cuda.is_available()          # (every case names its mode: nothing here depends on the process default)
    return o


def level_shapes(h, w):
    return [(h >> l, w >> l) for l in range(4)]


def run_entry(ops, case, f1, f2, fm, mode=None):
    """-> (levels as the reference lays them out: 4 tensors (B, P, hl, wl) on the device, the DispPyramid or None)."""
    row, entry, _, C, grid, cls = case
    mode = mode or case[2]
    B, _, h, w = f1.shape
    P = h * w
    if entry == "volume":
        lv = ops.corr_volume(f1, f2, mode=MODE[mode])
        for l, (hl, wl) in enumerate(level_shapes(h, w)):
            assert tuple(lv[l].shape) == (B * P, 1, hl, wl), (l, lv[l].shape)
        return [t.view(B, P, *t.shape[2:]) for t in lv], None
    if entry == "disp":
        dp = ops.corr_volume_disp(f1, f2, mode=MODE[mode])
    else:
        packs = ops.corr_pack(fm, mode=MODE[mode])
        dp = ops.corr_volume_disp_packed(packs, [p[0] for p in PACK_PAIRS], [p[1] for p in PACK_PAIRS])
    for l, (hl, wl) in enumerate(level_shapes(h, w)):
        assert tuple(dp.levels[l].shape) == (B, cdiv(P, 128), hl, wl, 128), (l, dp.levels[l].shape)
    return [t.view(B, P, *t.shape[2:]) for t in dp.to_rowmajor()], dp


def sentinel_call(ops, case, f1, f2, fm, dp):
    """The C-ABI of the displaced entry on sentinel-filled level buffers between sentinel bands: nothing but the lanes p < P
    of the destination is written, and those hold the bits of the ops call."""
    from accflow_amd import _lib
    lib = _lib.load()
    row, entry, mode, C, grid, cls = case
    B, _, h, w = f1.shape
    P, PB = h * w, cdiv(h * w, 128)
    n = [B * PB * hl * wl * 128 for hl, wl in level_shapes(h, w)]
    for l in range(4):
        assert n[l] == B * lib.accflow_corr_disp_level_elems(h, w, l)
    bufs = [torch.full((BAND + k + BAND,), SENT, device="cuda") for k in n]
    lv = [b[BAND:BAND + k] for b, k in zip(bufs, n)]
    guard = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = ops._stream()
    if entry == "disp":
        ws = torch.empty(lib.accflow_corr_volume_ws_bytes(C, h, w), dtype=torch.uint8, device="cuda")
        rc = lib.accflow_corr_volume_disp_f32(ops._p(f1), ops._p(f2), ops._p(lv[0]), ops._p(lv[1]), ops._p(lv[2]), ops._p(lv[3]),
                                              ops._p(ws), MODE[mode], ops._p(guard), B, C, h, w, st)
    else:
        import ctypes
        packs = ops.corr_pack(fm, mode=MODE[mode])
        a1 = (ctypes.c_int * B)(*[p[0] for p in PACK_PAIRS])
        a2 = (ctypes.c_int * B)(*[p[1] for p in PACK_PAIRS])
        rc = lib.accflow_corr_volume_disp_packed_f32(ops._p(packs.data), packs.F, a1, a2, ops._p(lv[0]), ops._p(lv[1]), ops._p(lv[2]),
                                                     ops._p(lv[3]), MODE[mode], ops._p(guard), B, C, h, w, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(guard.item()) == 0, "range guard"
    for l, (hl, wl) in enumerate(level_shapes(h, w)):
        assert bool((bufs[l][:BAND] == SENT).all()) and bool((bufs[l][BAND + n[l]:] == SENT).all()), "level %d: wrote outside its buffer" % l
        t = lv[l].view(B, PB, hl, wl, 128)
        if P % 128:
            assert bool((t[:, -1, :, :, P % 128:] == SENT).all()), "level %d: wrote the padding lanes p >= P" % l
        assert torch.equal(dp._unblocked(t, hl, wl), dp._unblocked(dp.levels[l], hl, wl)), "level %d: differs from the ops call" % l


@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_corr_route_vs_float64(ops, case):
    row, entry, mode, C, grid, cls = case
    B, h, w = GRIDS[grid]
    m = model(case)
    assert corr_route(entry, mode, C, h, w)[0] == row
    f1, f2, fm = case_inputs(case)
    assert f1.shape == f2.shape == (len(PACK_PAIRS) if entry == "packed" else B, C, h, w)
    assert f1.shape[0] == 1 or not torch.equal(f1[0], f1[1])        # (a wrong batch stride shows)
    d1, d2, dfm = dev(f1), dev(f2), (dev(fm) if fm is not None else None)
    tag = case_id(case)
    ops.guard_tripped()
    got, dp = run_entry(ops, case, d1, d2, dfm)
    if mode == "f16x3":
        assert not ops.guard_tripped(), tag + ": range guard"
    if mode != m["arith"]:                                # an f16x3 request that the route runs as bf16x6: the very bits
        again, _ = run_entry(ops, case, d1, d2, dfm, mode=m["arith"])
        for l in range(4):
            assert torch.equal(got[l], again[l]), "%s: level %d is not the %s result" % (tag, l, m["arith"])
    got = [t.cpu() for t in got]
    worst = 0.0
    for l in range(4):
        assert got[l].shape == m["ref"][l].shape, (tag, l, got[l].shape)
        assert not bool(torch.isnan(got[l]).any()), "%s level %d: NaN" % (tag, l)
        e = float((got[l].double() - m["ref"][l]).abs().max())
        print("RATIO %s %s level %d: %.3f  (error %.3g, E32 %.3g, E_split %.3g)" % (row, tag, l, e / m["gate"][l], e, m["e32"][l], m["esplit"][l]))
        worst = max(worst, e / m["gate"][l])
    for l in range(1, 4):
        assert torch.equal(got[l], pool(got[l - 1])), "%s: level %d is not the 2x2 mean of the stored level %d" % (tag, l, l - 1)
    assert worst <= 1.0, "%s: error / gate = %.3f" % (tag, worst)
    if dp is not None:
        sentinel_call(ops, case, d1, d2, dfm, dp)
        assert not ops.guard_tripped(), tag + ": range guard"
