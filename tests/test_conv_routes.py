"""Every default-reachable instantiation of the convolution kernels, each pinned to the route the plan gives it and compared
element by element with float64.

The dispatch is a pure host function (accflow_amd/csrc/conv_plan.cpp); accflow_conv_plan_query returns, for a descriptor, the
plan accflow_conv2d_f32 would launch.  ROWS below is the route table: one row per instantiation (more where a route has edges
of its own), each with the real `ops` call, the plan it must get and a gate.

  CPU (no GPU needed)
    test_row_plans_as_stated      the row's descriptor, filled with dummy pointers by plan_descriptor() - which restates
                                  PackedConv's pack rules and the workspace rule of the four forms of ops._conv_desc - plans
                                  to the row's key;
    test_table_is_complete        the launch lines of the direct kernel, the `case` labels of the im2col and fp32-MFMA
                                  launchers and the multi-source launch lines, counted in the sources: each has a row or is a
                                  named switch-only entry (SWITCH_ONLY);
    test_gate_has_teeth           one wrong tap moves the float64 reference by more than TEETH x the row's gate.
  GPU
    test_route_vs_float64         runs the call with accflow_conv2d_f32 traced (the wrapper asks accflow_conv_plan_query with
                                  the SAME descriptor before it forwards), asserts the traced key - so a drift between
                                  plan_descriptor() and ops.py shows as well -, that the range guard stayed quiet, that nothing
                                  outside the destination's channels changed, and every element against float64.

Inputs follow tests/test_hip_parity.py::test_conv2d_split_bf16 so that its gates transfer: x ~ N(0, 1), w ~ N(0, 2 / K),
b ~ 0.1 N.  References: F.conv2d in float64 plus the epilogue in float64; an S16 source's value is what the tensor holds,
(hi + lo) / 2^4.  Gates (the ones the suite already holds these kernels to):
    fp32 2e-5 + 1e-4 |ref|     bf16x3 2e-3     bf16x6 3e-5     f16x3 1e-4     normalise-on-load (f16x3, bf16x6) 5e-5 + 1e-5 |ref|
    GRU z and r*h 1e-5, h 2e-5     TAPGEMM 2e-6 max |ref| + 1e-6     an S16 destination: through to_float(), + 2^-22 |a| + 2^-29
Normalise-on-load in bf16x3 has no gate in the project: it is computed at run time as MARGIN x (error of a float32 CPU run
+ error of a float64 evaluation of the two-term split: 2 bf16 terms per operand, products 00, 01, 10), MARGIN = 4 and
split_bf16 from tests/test_gma_routes.py.

Out of scope: forms reached only through a routing switch, because the switches are read once per process -
ACCFLOW_DIRECT_W4=0 (the 2 x 2 wave layout of the 128-channel direct kernel: SWITCH_ONLY), ACCFLOW_S16M=1,
ACCFLOW_DIRECT_KT=0, ACCFLOW_DIRECT_KT9=0 (other routes to instantiations tabled here) and ACCFLOW_WGRAD_* (backward).

Measured on the MI355X, 2026-10-19, every row passing and every traced key the row's - largest error / gate per row (an S16
copy, against gate + storage term, reads the same to three digits):
    im2col 64x128 16->64 3x3 s2 bf16x3 0.021;  im2col 64x128 stats bf16x3 0.021
    im2col 128x64 16->96 3x3 s2 bf16x3 0.021;  im2col 128x64 16->128 1x1 s2 bf16x3 0.033
    im2col 64x64 16->64 3x3 s2 bf16x3 0.018;  im2col 128x128 16->96 3x3 s2 bf16x3 0.021
    im2col 64x128 16->64 3x3 s2 bf16x6 0.123;  im2col 64x128 stats bf16x6 0.123
    im2col 128x64 16->96 3x3 s2 bf16x6 0.117;  im2col 128x64 16->128 1x1 s2 bf16x6 0.030
    im2col 64x64 16->64 3x3 s2 bf16x6 0.108;  im2col 128x128 16->96 3x3 s2 bf16x6 0.113
    im2col 64x128 16->64 3x3 s2 f16x3 0.024;  im2col 64x128 stats f16x3 0.024;  im2col 128x64 16->96 3x3 s2 f16x3 0.026
    im2col 128x64 16->128 1x1 s2 f16x3 0.017;  im2col 64x64 16->64 3x3 s2 f16x3 0.020
    im2col 128x128 16->96 3x3 s2 f16x3 0.028;  im2col 64x128 ragged 0.027;  im2col 128x64 ragged 0.026
    tail 32->192 3x3 bf16x3 0.017;  tail 32->320 3x3 bf16x3 0.018;  tail 32->192 3x3 bf16x6 0.166
    tail 32->320 3x3 bf16x6 0.155;  tail 32->192 3x3 f16x3 0.034;  tail 32->320 3x3 f16x3 0.038
    tail 32->192 res_relu 0.034;  tail 32->320 accum bf16x6 0.184;  no tail 32->192 gru_q 0.066;  no tail 64->200 0.053
    tail S16 256->192 3x3 res_relu out16 0.059;  tail S16 64->320 1x1 0.017;  tail S16 64->160 1x5 0.027
    norm f16 generic 40->96 3x3 0.032;  norm f16 generic 64->128 1x5 0.029;  norm f16 tap9 64->96 3x3 0.035
    norm f16 64->64 3x3 0.034;  norm bf16x6 40->96 3x3 0.029;  norm bf16x6 64->64 3x3 0.042
    norm bf16x3 40->96 3x3 0.236;  norm bf16x3 64->64 3x3 0.233;  norm + split-K 128->128 3x3 0.025
    S16 generic 128->64 1x5 split-K 0.015;  S16 generic 128->64 1x5 0.040;  S16 generic 128->64 1x1 split-K 0.009
    S16 generic 128->64 1x1 0.018;  S16 generic 16->128 1x7 0.014;  S16 tap5 128->128 1x5 0.046
    S16 tap5 64+64->128 5x1 split-K out16 0.015;  S16 tap9 128->64 3x3 0.089;  S16 tap9 128->128 3x3 out16 0.075
    tapgemm generic 128->128 1x5 0.157;  tapgemm tap9 128->128 3x3 0.178;  gru_zr 32+16->64 1x5 0.024
    gru_zr 48->96 1x5 0.026;  gru_q 32+16->32 5x1 0.033;  gru_q 48->128 5x1 bf16x6 0.050;  res_relu 48->128 3x3 0.025
    accum 48->64 3x3 0.030;  gru_zr 128+16->64 1x5 split-K 0.023;  gru_zr 144->96 1x5 split-K 0.026
    gru_q 128+16->32 5x1 split-K 0.039;  gru_q 144->128 5x1 bf16x6 split-K 0.049;  res_relu 144->128 3x3 split-K 0.018
    accum 144->64 3x3 split-K 0.024;  direct 40->64 3x3 bf16x3 0.014;  direct 40->96 3x3 bf16x3 0.014
    direct 40->64 3x3 bf16x6 0.134;  direct 40->96 3x3 bf16x6 0.110;  direct 40->64 3x3 f16x3 0.029
    direct 40->96 3x3 f16x3 0.026;  f32 32ch x 256px 0.069;  f32 32ch x 128px 0.044;  f32 64ch x 128px 0.070
    f32 64ch x 64px 0.055;  f32 96ch x 128px 0.081;  f32 128ch x 128px 0.084;  f32 128ch x 64px 0.088
    stem 3->64 7x7 s2 0.018;  small 8->2 3x3 0.013;  small 40->3 3x3 s2 0.031;  small-patch 96->3 1x5 0.034
    small-patch 64->1 3x3 0.034;  multi lay 0 tap9 0.045;  multi lay 0 generic 0.030;  multi lay 1 tap9 0.028
    multi lay 1 generic 0.021;  multi lay 2 tap9 0.031;  multi lay 2 generic 0.026;  multi lay 3 tap9 0.041
    multi lay 3 generic 0.027
Normalise-on-load in bf16x3, computed at run time: 40->96 gate 8.655e-05 = 4 x (E32 1.415e-06 + E_split 2.022e-05), measured
error 2.04e-05 (0.236 of the gate); 64->64 gate 8.089e-05 = 4 x (9.669e-07 + 1.925e-05), measured 1.88e-05 (0.233).
No gate, margin, shape or input was chosen from these figures.
"""
import ctypes
import os
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

import test_gma_routes as R

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accflow_amd", "csrc")
TEETH, MARGIN = R.TEETH, R.MARGIN
S16_REL, S16_ABS = 2.0 ** -22, 2.0 ** -29
SENT = -777.25
SENT16 = 0x7B7B7B7B

SMALL, SMALL_PATCH, STEM, DIRECT, S16M, IM2COL, F32 = range(7)        # conv_family (conv_plan.h)
GENERIC, TAP5, TAP9 = 0, 1, 2                                          # conv_loop
MODE = {"f32": 0, "bf16x3": 2, "bf16x6": 3, "f16x3": 4}
PLAN = ("family", "tc", "tp", "wc", "wp", "lay", "loop", "tapgemm", "norm", "w4", "mode", "slots", "ch0", "Z", "Zhead", "Ztail")
KSPLIT_MAX_PIXELS = 4 * 7680                                           # ops.KSPLIT_MAX_PIXELS (asserted on the GPU)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------
# the route table


class Row:
    """One call.  kind: conv (ops.conv2d), tapgemm (ops.conv2d_tapgemm), multi (ops.conv2d_multi with a forced layout).
    key = (family, (tc, tp, wc, wp, lay), loop, tapgemm, norm, w4, mode, Z > 1, ch0)."""

    def __init__(self, name, cins, cout, k, shape, key, mode="f16x3", stride=1, epi="store", bias=True, s16=False, out16=False,
                 stats=False, norm=False, pre=False, nokws=False, kind="conv", lay=None, slots=None, share=None, tail=None):
        self.name, self.cins, self.cout, self.k, self.shape, self.key = name, tuple(cins), cout, tuple(k), tuple(shape), key
        self.mode, self.stride, self.epi, self.bias, self.s16, self.out16 = mode, stride, epi, bias, s16, out16
        self.stats, self.norm, self.pre, self.nokws, self.kind, self.lay, self.slots = stats, norm, pre, nokws, kind, lay, slots
        self.share = share or name          # rows of one `share` run on the same inputs and the same reference
        self.tail = tail                    # tail cut: (ch0, Z of the head, Z of the tail)
        self.cin = sum(self.cins)
        self.pad = (self.k[0] // 2, self.k[1] // 2)
        B, H, W = self.shape
        self.OH = (H + 2 * self.pad[0] - self.k[0]) // stride + 1
        self.OW = (W + 2 * self.pad[1] - self.k[1]) // stride + 1
        self.n_out = cout // 2 if epi == "gru_zr" else cout

    def __repr__(self):
        return self.name


def direct(tc, mode="f16x3", loop=GENERIC, norm=0, z=False, ch0=0, tapgemm=0):
    return (DIRECT, (tc, 0, 0, 0, 0), loop, tapgemm, norm, int(tc == 2), MODE[mode], z, ch0)


def im2col(tc, tp, mode):
    return (IM2COL, (tc, tp, 0, 0, 0), GENERIC, 0, 0, 0, MODE[mode], False, 0)


def f32tile(wc, wp, tc, tp):
    return (F32, (tc, tp, wc, wp, 0), GENERIC, 0, 0, 0, MODE["f32"], False, 0)


def s16m(lay, loop):
    return (S16M, (0, 0, 0, 0, lay), loop, 0, 0, 0, MODE["f16x3"], False, 0)


def plain(fam, mode):
    return (fam, (0, 0, 0, 0, 0), GENERIC, 0, 0, 0, MODE[mode], False, 0)


SPLIT_MODES = ("bf16x3", "bf16x6", "f16x3")
S = (2, 13, 37)         # ragged both ways: 4 x 2 tiles of 4 x 32 pixels per item, the last of each row 5 wide, the last row 1 high
E = (2, 10, 18)
T3, T2 = (3, 60, 128), (2, 60, 128)      # 360 128-channel workgroups: the tail cut is taken with a workspace on offer
ROWS = []


def add(*a, **kw):
    ROWS.append(Row(*a, **kw))


# ---- the im2col tiles (stride 2: not the direct kernel's), three modes each; statistics where the tile grid allows them
for m in SPLIT_MODES:
    add("im2col 64x128 16->64 3x3 s2 %s" % m, (16,), 64, (3, 3), (2, 256, 384), im2col(1, 2, m), mode=m, stride=2, share="i12")
    add("im2col 64x128 stats %s" % m, (16,), 64, (3, 3), (2, 256, 384), im2col(1, 2, m), mode=m, stride=2, share="i12", stats=True,
        slots=384)
    add("im2col 128x64 16->96 3x3 s2 %s" % m, (16,), 96, (3, 3), (1, 256, 384), im2col(2, 1, m), mode=m, stride=2, share="i21")
    add("im2col 128x64 16->128 1x1 s2 %s" % m, (16,), 128, (1, 1), (1, 256, 384), im2col(2, 1, m), mode=m, stride=2, share="i21p")
    add("im2col 64x64 16->64 3x3 s2 %s" % m, (16,), 64, (3, 3), (2, 26, 74), im2col(1, 1, m), mode=m, stride=2, share="i11")
    add("im2col 128x128 16->96 3x3 s2 %s" % m, (16,), 96, (3, 3), (2, 256, 384), im2col(2, 2, m), mode=m, stride=2, share="i22")
# 49 794 output pixels = 390 tiles, the last one partial, tiles straddling the two items: no statistics (0 slots)
add("im2col 64x128 ragged", (16,), 64, (3, 3), (2, 258, 386), im2col(1, 2, "f16x3"), stride=2, stats=True, slots=0)
add("im2col 128x64 ragged", (16,), 96, (3, 3), (1, 258, 386), im2col(2, 1, "f16x3"), stride=2)

# ---- the tail cut (Cout = 128 m + 1..64: the head on the 128-channel kernel, the tail on the 64-channel one), fp32 sources
for m in SPLIT_MODES:
    add("tail 32->192 3x3 %s" % m, (32,), 192, (3, 3), T3, direct(2, m, ch0=128), mode=m, share="t192", tail=(128, 1, 1))
    add("tail 32->320 3x3 %s" % m, (32,), 320, (3, 3), T2, direct(2, m, ch0=256), mode=m, share="t320", tail=(256, 1, 1))
add("tail 32->192 res_relu", (32,), 192, (3, 3), T3, direct(2, ch0=128), epi="res_relu", tail=(128, 1, 1))
add("tail 32->320 accum bf16x6", (32,), 320, (3, 3), T2, direct(2, "bf16x6", ch0=256), mode="bf16x6", epi="accum", tail=(256, 1, 1))
# ... declined: an epilogue that is not pointwise, a 72-channel remainder
add("no tail 32->192 gru_q", (32,), 192, (3, 3), T3, direct(2), epi="gru_q", pre=True)
add("no tail 64->200", (64,), 200, (3, 3), T3, direct(2))
# ... S16 sources (never diverted whatever the grid), no workspace
add("tail S16 256->192 3x3 res_relu out16", (256,), 192, (3, 3), (1, 12, 64), direct(2, loop=TAP9, ch0=128), s16=True, out16=True,
    epi="res_relu", nokws=True, tail=(128, 1, 1))
add("tail S16 64->320 1x1", (64,), 320, (1, 1), (1, 13, 37), direct(2, ch0=256), s16=True, nokws=True, tail=(256, 1, 1))
add("tail S16 64->160 1x5", (64,), 160, (1, 5), (1, 13, 37), direct(2, loop=TAP5, ch0=128), s16=True, nokws=True, tail=(128, 1, 1))

# ---- normalise-on-load
add("norm f16 generic 40->96 3x3", (40,), 96, (3, 3), S, direct(2, norm=1), norm=True, stats=True, slots=8)
add("norm f16 generic 64->128 1x5", (64,), 128, (1, 5), S, direct(2, norm=1), norm=True, stats=True, slots=8)
add("norm f16 tap9 64->96 3x3", (64,), 96, (3, 3), S, direct(2, norm=1, loop=TAP9), norm=True, stats=True, slots=8)
add("norm f16 64->64 3x3", (64,), 64, (3, 3), S, direct(1, norm=1), norm=True, stats=True, slots=16)
add("norm bf16x6 40->96 3x3", (40,), 96, (3, 3), S, direct(2, "bf16x6", norm=1), mode="bf16x6", norm=True, stats=True, slots=8)
add("norm bf16x6 64->64 3x3", (64,), 64, (3, 3), S, direct(1, "bf16x6", norm=1), mode="bf16x6", norm=True, stats=True, slots=16)
add("norm bf16x3 40->96 3x3", (40,), 96, (3, 3), S, direct(2, "bf16x3", norm=1), mode="bf16x3", norm=True, stats=True, slots=8)
add("norm bf16x3 64->64 3x3", (64,), 64, (3, 3), S, direct(1, "bf16x3", norm=1), mode="bf16x3", norm=True, stats=True, slots=16)
add("norm + split-K 128->128 3x3", (128,), 128, (3, 3), S, direct(2, norm=1, loop=TAP9, z=True), norm=True)

# ---- S16 sources
for k in ((1, 5), (1, 1)):
    add("S16 generic 128->64 %dx%d split-K" % k, (128,), 64, k, S, direct(1, z=True), s16=True, share="s64 %dx%d" % k)
    add("S16 generic 128->64 %dx%d" % k, (128,), 64, k, S, direct(1), s16=True, nokws=True, share="s64 %dx%d" % k)
add("S16 generic 16->128 1x7", (16,), 128, (1, 7), S, direct(2), s16=True, nokws=True)
add("S16 tap5 128->128 1x5", (128,), 128, (1, 5), S, direct(2, loop=TAP5), s16=True, nokws=True)
add("S16 tap5 64+64->128 5x1 split-K out16", (64, 64), 128, (5, 1), S, direct(2, loop=TAP5, z=True), s16=True, out16=True)
add("S16 tap9 128->64 3x3", (128,), 64, (3, 3), S, direct(1, loop=TAP9), s16=True, nokws=True)
add("S16 tap9 128->128 3x3 out16", (128,), 128, (3, 3), S, direct(2, loop=TAP9), s16=True, out16=True, nokws=True)
add("tapgemm generic 128->128 1x5", (128,), 128, (1, 5), (1, 20, 64), direct(2, tapgemm=1), s16=True, nokws=True, kind="tapgemm")
add("tapgemm tap9 128->128 3x3", (128,), 128, (3, 3), (1, 20, 64), direct(2, tapgemm=1, loop=TAP9), s16=True, nokws=True, kind="tapgemm")

# ---- the direct kernel's epilogues inside the kernel (a workspace is on offer; <= 48 input channels = 3 chunks: one part) ...
add("gru_zr 32+16->64 1x5", (32, 16), 64, (1, 5), E, direct(1), epi="gru_zr", pre=True)
add("gru_zr 48->96 1x5", (48,), 96, (1, 5), E, direct(2), epi="gru_zr")      # the z | r boundary inside a 32-row tile
add("gru_q 32+16->32 5x1", (32, 16), 32, (5, 1), E, direct(1), epi="gru_q", pre=True)
add("gru_q 48->128 5x1 bf16x6", (48,), 128, (5, 1), E, direct(2, "bf16x6"), mode="bf16x6", epi="gru_q", pre=True)
add("res_relu 48->128 3x3", (48,), 128, (3, 3), E, direct(2), epi="res_relu")
add("accum 48->64 3x3", (48,), 64, (3, 3), E, direct(1), epi="accum")
# ... and the same through the split-K reduce kernel (>= 128 input channels: four parts)
add("gru_zr 128+16->64 1x5 split-K", (128, 16), 64, (1, 5), E, direct(1, z=True), epi="gru_zr", pre=True)
add("gru_zr 144->96 1x5 split-K", (144,), 96, (1, 5), E, direct(2, z=True), epi="gru_zr")
add("gru_q 128+16->32 5x1 split-K", (128, 16), 32, (5, 1), E, direct(1, z=True), epi="gru_q", pre=True)
add("gru_q 144->128 5x1 bf16x6 split-K", (144,), 128, (5, 1), E, direct(2, "bf16x6", z=True), mode="bf16x6", epi="gru_q", pre=True)
add("res_relu 144->128 3x3 split-K", (144,), 128, (3, 3), E, direct(2, z=True), epi="res_relu")
add("accum 144->64 3x3 split-K", (144,), 64, (3, 3), E, direct(1, z=True), epi="accum")

# ---- what the other test files reach already, each at one small shape, so that this table is the whole list
for m in SPLIT_MODES:
    add("direct 40->64 3x3 %s" % m, (40,), 64, (3, 3), S, direct(1, m), mode=m, share="d64")
    add("direct 40->96 3x3 %s" % m, (40,), 96, (3, 3), S, direct(2, m), mode=m, share="d96")
add("f32 32ch x 256px", (20,), 8, (3, 3), (1, 256, 384), f32tile(1, 4, 1, 2), mode="f32")
add("f32 32ch x 128px", (20,), 27, (3, 3), S, f32tile(1, 4, 1, 1), mode="f32")
add("f32 64ch x 128px", (20,), 48, (3, 3), (1, 192, 256), f32tile(2, 2, 1, 2), mode="f32")
add("f32 64ch x 64px", (20,), 130, (3, 3), S, f32tile(2, 2, 1, 1), mode="f32")
add("f32 96ch x 128px", (20,), 192, (3, 3), (1, 128, 192), f32tile(1, 4, 3, 1), mode="f32")
add("f32 128ch x 128px", (20,), 130, (3, 3), (1, 128, 192), f32tile(2, 2, 2, 2), mode="f32")
add("f32 128ch x 64px", (20,), 130, (3, 3), (1, 96, 128), f32tile(2, 2, 2, 1), mode="f32")
add("stem 3->64 7x7 s2", (3,), 64, (7, 7), (2, 26, 74), plain(STEM, "f16x3"), stride=2)
add("small 8->2 3x3", (8,), 2, (3, 3), S, plain(SMALL, "f32"), mode="f32")
add("small 40->3 3x3 s2", (40,), 3, (3, 3), S, plain(SMALL, "f32"), mode="f32", stride=2)
add("small-patch 96->3 1x5", (96,), 3, (1, 5), S, plain(SMALL_PATCH, "f32"), mode="f32")
add("small-patch 64->1 3x3", (64,), 1, (3, 3), S, plain(SMALL_PATCH, "f32"), mode="f32")
for lay, cout in ((0, 128), (1, 64), (2, 64), (3, 96)):
    add("multi lay %d tap9" % lay, (32, 32), cout, (3, 3), S, s16m(lay, TAP9), s16=True, nokws=True, kind="multi", lay=lay)
    add("multi lay %d generic" % lay, (32, 32), cout, (1, 5), S, s16m(lay, GENERIC), s16=True, nokws=True, kind="multi", lay=lay)

BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)


# ------------------------------------------------------------------------------------------------
# which instantiation a row's key stands for (launch_conv_direct, s16m_launch and the two `switch` launchers, restated;
# test_table_is_complete pins the lists to the sources)

_S16 = "true, true, false, true"
DIRECT_ARGS = {     # file -> template arguments of every launch line -> None (tabled) or the switch that alone reaches it
    "conv2d_direct_v_f16.hip": {"2, 2, true, true": None, "2, 2, true": "ACCFLOW_DIRECT_W4=0", "1, 2, true": None},
    "conv2d_direct_v_bf16x3.hip": {"2, 2, false, true": None, "2, 2": "ACCFLOW_DIRECT_W4=0", "1, 2": None},
    "conv2d_direct_v_bf16x6.hip": {"2, 3, false, true": None, "2, 3": "ACCFLOW_DIRECT_W4=0", "1, 3": None},
    "conv2d_direct_v_f16n.hip": {"2, 2, true, true, true, false, 7, false, 9, 3": None, "2, 2, true, true, true": None,
                                 "1, 2, true, false, true": None},
    "conv2d_direct_v_bf16n.hip": {"2, 2, false, true, true": None, "2, 3, false, true, true": None, "1, 2, false, false, true": None,
                                  "1, 3, false, false, true": None},
    "conv2d_direct_v_s16.hip": {"2, 2, " + _S16: None, "1, 2, true, false, false, true": None},
    "conv2d_direct_v_s16tg.hip": {"2, 2, " + _S16 + ", 7, true": None},
    "conv2d_direct_v_s16k.hip": {"2, 2, " + _S16 + ", 7, false, 5, 5": None, "2, 2, " + _S16 + ", 7, false, 5, 1": None},
    "conv2d_direct_v_s16k9.hip": {"2, 2, " + _S16 + ", 7, true, 9, 3": None, "2, 2, " + _S16 + ", 7, false, 9, 3": None,
                                  "1, 2, true, false, false, true, 7, false, 9, 3": None},
}
SWITCH_ONLY = sorted((f, a, s) for f, d in DIRECT_ARGS.items() for a, s in d.items() if s)
S16M_ARGS = {"conv_s16m_v0.hip": ["0, true", "0"], "conv_s16m_v1.hip": ["1, true", "1"], "conv_s16m_v2.hip": ["2"],
             "conv_s16m_v3.hip": ["3, true", "3"]}
IM2COL_CASES = (11, 12, 21, 22)
F32_CASES = (1412, 1411, 2212, 2211, 1431, 2222, 2221)


def direct_instantiation(tc, loop, tapgemm, norm, mode, s16_in, k):
    """(file, template arguments) of the direct kernel a plan launches (conv2d_direct.hip: launch_conv_direct)."""
    if tapgemm:
        return ("conv2d_direct_v_s16k9.hip", "2, 2, " + _S16 + ", 7, true, 9, 3") if loop == TAP9 else ("conv2d_direct_v_s16tg.hip", "2, 2, " + _S16 + ", 7, true")
    if s16_in:
        if loop == TAP5:
            return "conv2d_direct_v_s16k.hip", "2, 2, " + _S16 + ", 7, false, 5, %d" % k[1]
        if loop == TAP9:
            return "conv2d_direct_v_s16k9.hip", ("2, 2, " + _S16 if tc == 2 else "1, 2, true, false, false, true") + ", 7, false, 9, 3"
        return "conv2d_direct_v_s16.hip", "2, 2, " + _S16 if tc == 2 else "1, 2, true, false, false, true"
    f16 = mode == MODE["f16x3"]
    nt = 2 if mode == MODE["bf16x3"] else 3
    if norm:
        if f16:
            if tc == 2:
                return "conv2d_direct_v_f16n.hip", "2, 2, true, true, true" + (", false, 7, false, 9, 3" if loop == TAP9 else "")
            return "conv2d_direct_v_f16n.hip", "1, 2, true, false, true"
        return "conv2d_direct_v_bf16n.hip", "%d, %d, false, %s, true" % (tc, nt, "true" if tc == 2 else "false")
    if f16:
        return "conv2d_direct_v_f16.hip", "2, 2, true, true" if tc == 2 else "1, 2, true"
    return "conv2d_direct_v_bf16x%d.hip" % (3 if nt == 2 else 6), "2, %d, false, true" % nt if tc == 2 else "1, %d" % nt


def instantiations(row):
    """Every instantiation the row runs: [(file, id)]; a tail cut runs the head's and the tail's."""
    fam, (tc, tp, wc, wp, lay), loop, tapgemm, norm, w4, mode, z, ch0 = row.key
    if fam == DIRECT:
        s16_in = row.s16
        out = [direct_instantiation(tc, loop, tapgemm, norm, mode, s16_in, row.k)]
        if ch0:     # conv_plan_part: the tail on the 64-channel kernel; its S16 loop is 9-tap for 3x3, generic otherwise
            tl = (TAP9 if row.k == (3, 3) else GENERIC) if s16_in else GENERIC
            out.append(direct_instantiation(1, tl, 0, norm, mode, s16_in, row.k))
        return out
    if fam == S16M:
        return [("conv_s16m_v%d.hip" % lay, "%d, true" % lay if (loop == TAP9 and lay != 2) else "%d" % lay)]
    if fam == IM2COL:
        return [("conv2d_bf16s.hip", "%d mode %d" % (tc * 10 + tp, mode))]
    if fam == F32:
        return [("conv2d_f32.hip", "%d" % (wc * 1000 + wp * 100 + tc * 10 + tp))]
    if fam == STEM:
        return [("conv_stem.hip", "stem")]
    co = 2 if row.cout <= 2 else 4
    return [("conv_small.hip", "%s<%d>" % ("small_patch" if fam == SMALL_PATCH else "small", co))]


# ------------------------------------------------------------------------------------------------
# the descriptor of a row without a GPU: PackedConv's pack rules and the callers' workspace rule, restated


_loaded = []


def _lib():
    if not _loaded:
        from accflow_amd import build as _b
        _b.build(force=False, verbose=False)
        from accflow_amd import _lib as L
        _loaded.extend([L, L.load()])
    return _loaded


DUMMY = 0x10000     # a non-null pointer that nothing dereferences: the plan is host code over the descriptor's scalars


def plan_descriptor(row):
    L, lib = _lib()
    d = L.ConvDesc()
    B, H, W = row.shape
    OH, OW, cout, cin, (kh, kw) = row.OH, row.OW, row.cout, row.cin, row.k
    px = B * OH * OW
    words = lambda c, h, w: lib.accflow_s16_item_words(c, h, w)  # noqa: E731
    f16 = row.mode == "f16x3"
    d.B, d.H, d.W, d.OH, d.OW, d.Cout = B, H, W, OH, OW, cout
    d.CoutPad = lib.accflow_conv_coutpad(cout)
    d.mode, d.guard = MODE[row.mode], DUMMY
    d.bias = DUMMY if row.bias else None
    d.out, d.out_bs = DUMMY, row.n_out * OH * OW
    offer = not row.nokws and px <= KSPLIT_MAX_PIXELS and cout > 4
    if row.kind == "multi":        # ops.conv2d_multi over PackedMulti.from_cat
        d.nsrc = len(row.cins)
        for s, c in enumerate(row.cins):
            sr = d.src[s]
            sr.ptr, sr.bs, sr.C, sr.Hs, sr.Ws = DUMMY, words(c, H, W), c, H, W
            sr.step, sr.oy, sr.ox, sr.KH, sr.KW, sr.padH, sr.padW = 1, 0, 0, kh, kw, row.pad[0], row.pad[1]
        d.src[0].reserved = row.lay + 1
        d.H, d.W = OH, OW
        d.KH = d.KW = d.stride = 1
        d.wpatch16 = d.wscale16 = DUMMY
        if offer:
            d.kws, d.kws_elems = DUMMY, 4 * px * cout
        return d
    # PackedConv: which packs exist
    has_split = cout > 4
    has_patch = has_split and row.stride == 1 and cin >= 16
    has_split16 = has_split and cout > 32
    d.C0, d.C1 = row.cins[0], (row.cins[1] if len(row.cins) > 1 else 0)
    d.KH, d.KW, d.stride, d.padH, d.padW = kh, kw, row.stride, row.pad[0], row.pad[1]
    d.wpack = d.ktab = DUMMY
    d.Kpad = lib.accflow_conv_kpad(cin, kh, kw)
    d.in0 = DUMMY
    d.in1 = DUMMY if d.C1 else None
    if row.s16:
        d.in_fmt = 3 if d.C1 else 1
        d.in0_bs, d.in1_bs = words(d.C0, H, W), (words(d.C1, H, W) if d.C1 else 0)
    else:
        d.in0_bs, d.in1_bs = d.C0 * H * W, d.C1 * H * W
    if row.kind == "tapgemm":      # ops.conv2d_tapgemm: conv1 here, conv2 = 3x3 -> 2 channels as 18 tap rows
        assert row.s16 and has_patch and f16
        d.act, d.epi = 1, 5
        d.wpatch = d.wpatch16 = d.wscale16 = DUMMY
        d.tg_w16 = d.tg_scale = d.tg_out = DUMMY
        d.tg_rows, d.tg_coutpad = 18, 128
        d.tg_out_bs, d.tg_out_ps = 18 * H * W, B * 18 * H * W
        d.out, d.out_bs = None, 0
        return d
    d.epi = {"store": 0, "res_relu": 1, "gru_zr": 2, "gru_q": 3, "accum": 4}[row.epi]
    d.act = {"store": 0, "res_relu": 1, "gru_zr": 2, "gru_q": 3, "accum": 0}[row.epi]
    d.wsplit = DUMMY if has_split else None
    if row.s16 or row.out16:       # ops._FORM_S16
        assert f16 and (has_patch or has_split16)      # (without the patch pack: the stem with an S16 copy)
        d.wpatch = d.wpatch16 = DUMMY if has_patch else None
        d.wscale16 = DUMMY
        d.wsplit16 = DUMMY if has_split16 else None
        if row.out16:
            d.out16, d.out16_bs = DUMMY, words(row.n_out, OH, OW)
        if offer:
            d.kws, d.kws_elems = DUMMY, 4 * px * cout
    else:                          # ops._conv2d
        d.wpatch = DUMMY if has_patch else None
        if f16 and (has_patch or has_split16):
            d.wpatch16 = DUMMY if has_patch else None
            d.wsplit16 = DUMMY if has_split16 else None
            d.wscale16 = DUMMY
        if has_patch and offer:
            d.kws, d.kws_elems = DUMMY, 4 * px * cout
    if row.epi in ("res_relu", "accum", "gru_zr", "gru_q"):
        d.e0, d.e0_bs = DUMMY, row.n_out * OH * OW
    if row.epi == "gru_q":
        d.e1, d.e1_bs = DUMMY, cout * OH * OW
    if row.epi == "gru_zr":
        d.out2, d.out2_bs = DUMMY, row.n_out * OH * OW
    if row.pre:
        d.pre, d.pre_bs = DUMMY, cout * OH * OW
    if row.norm:
        assert lib.accflow_conv_in_norm_supported(ctypes.byref(d)) == 1, row
        d.in_norm = DUMMY
    if row.stats:
        slots = lib.accflow_conv_stat_slots(ctypes.byref(d))
        if slots > 0:
            d.stats, d.stat_slots = DUMMY, slots
    return d


def query(lib, dref):
    out = (ctypes.c_int * 16)()
    rc = lib.accflow_conv_plan_query(dref, out, 16)
    return rc, dict(zip(PLAN, list(out)))


def key_of(p):
    return (p["family"], (p["tc"], p["tp"], p["wc"], p["wp"], p["lay"]), p["loop"], p["tapgemm"], p["norm"], p["w4"], p["mode"],
            p["Z"] > 1, p["ch0"])


def assert_plan(row, rc, p):
    assert rc == 0, (row, p)
    assert key_of(p) == row.key, (row, key_of(p), row.key)
    if row.stats:
        assert p["slots"] == row.slots, (row, p)
    if row.tail:
        assert (p["ch0"], p["Zhead"], p["Ztail"]) == row.tail, (row, p)
    else:
        assert p["ch0"] == 0 and p["Zhead"] == 0 and p["Ztail"] == 0, (row, p)


# ------------------------------------------------------------------------------------------------
# inputs and float64 references (computed once per `share`, never modified)


def s16_value(x32):
    return R.s16_value(x32)[0]


_inputs = {}


def probes(row):
    """The two taps whose loss the gate must notice: the last weight and the first one (a tail cut: of the tail's first channel)."""
    first = row.tail[0] if row.tail else 0
    return (row.cout - 1, row.cin - 1, row.k[0] - 1, row.k[1] - 1), (first, 0, 0, 0)


def inputs(row):
    if row.share in _inputs:
        return _inputs[row.share]
    g = torch.Generator().manual_seed(zlib.crc32(row.share.encode()) & 0x7FFFFFFF)
    B, H, W = row.shape
    K = row.cin * row.k[0] * row.k[1]
    I = {}
    if row.norm:        # the raw output of a convolution and its InstanceNorm {mean, rstd} per plane (float32, as finalised)
        x = torch.randn(B, row.cin, H, W, generator=g) * 1.5 + 0.3
        mu = x.double().mean(dim=(2, 3))
        rstd = 1.0 / torch.sqrt(x.double().var(dim=(2, 3), unbiased=False) + 1e-5)
        I["in_norm"] = torch.stack([mu, rstd], dim=2).float()
        I["x"] = [x]
    else:
        I["x"] = [torch.randn(B, c, H, W, generator=g) for c in row.cins]
        if row.s16:
            I["x"] = [s16_value(x) for x in I["x"]]
    I["w"] = torch.randn(row.cout, row.cin, *row.k, generator=g) * (2.0 / K) ** 0.5
    # rows of different magnitude get their own fp16 row scale (wscale16): a scale read at the wrong channel - the tail cut
    # advances that pointer by ch0 - is off by a power of two.  Neither row is one test_gate_has_teeth probes.
    if row.cout > 2:
        I["w"][1] *= 2.0 ** -3
    if row.tail:
        I["w"][row.tail[0] + 1] *= 2.0 ** -6
    for co, ci, ky, kx in probes(row):      # the weights test_gate_has_teeth zeroes: one standard deviation, not the luck of the draw
        I["w"][co, ci, ky, kx] = (2.0 / K) ** 0.5 * (1.0 if I["w"][co, ci, ky, kx] >= 0 else -1.0)
    I["b"] = torch.randn(row.cout, generator=g) * 0.1 if row.bias else None
    no = (B, row.n_out, row.OH, row.OW)
    if row.epi in ("res_relu", "accum"):
        I["e0"] = torch.randn(no, generator=g)
    if row.epi in ("gru_zr", "gru_q"):
        I["e0"] = torch.tanh(torch.randn(no, generator=g))
    if row.epi == "gru_q":
        I["e1"] = torch.rand(no, generator=g)
    if row.pre:
        I["pre"] = torch.randn(B, row.cout, row.OH, row.OW, generator=g) * 0.2
    if row.kind == "tapgemm":
        I["w2"] = torch.randn(2, row.cout, 3, 3, generator=g) * (2.0 / (row.cout * 9)) ** 0.5
        I["b2"] = torch.randn(2, generator=g) * 0.1
    _inputs[row.share] = I
    return I


def conv_input64(row, I):
    x = torch.cat(I["x"], 1).double()
    if row.norm:
        mr = I["in_norm"].double()
        x = torch.relu((x - mr[:, :, 0, None, None]) * mr[:, :, 1, None, None])
    return x


def raw64(row, I, x=None, w=None):
    """conv + bias (+ pre) in float64"""
    x = conv_input64(row, I) if x is None else x
    w = I["w"].double() if w is None else w
    y = F.conv2d(x, w, I["b"].double() if I["b"] is not None else None, stride=row.stride, padding=row.pad)
    return y + I["pre"].double() if row.pre else y


def finish64(row, I, y):
    """the epilogue in float64: {output name: tensor}"""
    if row.kind == "tapgemm":
        return {"out": F.conv2d(torch.relu(y), I["w2"].double(), I["b2"].double(), padding=1)}
    if row.epi == "store":
        return {"out": y}
    if row.epi == "res_relu":
        return {"out": torch.relu(I["e0"].double() + torch.relu(y))}
    if row.epi == "accum":
        return {"out": I["e0"].double() + y}
    if row.epi == "gru_zr":
        hd = row.cout // 2
        return {"z": torch.sigmoid(y[:, :hd]), "rh": torch.sigmoid(y[:, hd:]) * I["e0"].double()}
    z = I["e1"].double()
    return {"h": (1 - z) * I["e0"].double() + z * torch.tanh(y)}


_refs = {}


def reference(row):
    """(raw float64 conv, {name: float64 reference}) of the row's share and epilogue"""
    k = (row.share, row.epi, row.kind)
    if k not in _refs:
        I = inputs(row)
        y = raw64(row, I)
        _refs[k] = (y, finish64(row, I, y))
    return _refs[k]


_norm_gates = {}


def norm_bf16x3_gate(row):
    """(MARGIN x (E32 + E_split), E32, E_split) for normalise-on-load in bf16x3, per the module docstring."""
    if row.name not in _norm_gates:
        _norm_gates[row.name] = _norm_bf16x3_gate(row)
    return _norm_gates[row.name]


def _norm_bf16x3_gate(row):
    I = inputs(row)
    ref = reference(row)[1]["out"]
    x32 = torch.cat(I["x"], 1)
    mr = I["in_norm"]
    xn32 = torch.relu((x32 - mr[:, :, 0, None, None]) * mr[:, :, 1, None, None])
    y32 = F.conv2d(xn32, I["w"], I["b"], stride=row.stride, padding=row.pad)
    e32 = float((y32.double() - ref).abs().max())
    a0, a1 = R.split_bf16(xn32, 2)
    w0, w1 = R.split_bf16(I["w"], 2)
    conv = lambda a, w: F.conv2d(a, w, None, stride=row.stride, padding=row.pad)  # noqa: E731
    ys = conv(a0, w0) + conv(a0, w1) + conv(a1, w0) + (I["b"].double().view(1, -1, 1, 1) if I["b"] is not None else 0.0)
    esplit = float((ys - ref).abs().max())
    return MARGIN * (e32 + esplit), e32, esplit


def gates(row):
    """{output name: (atol, rtol)}; an S16 destination adds its storage term where it is compared"""
    if row.kind == "tapgemm":
        return {"out": (2e-6 * float(reference(row)[1]["out"].abs().max()) + 1e-6, 0.0)}
    if row.epi == "gru_zr":
        return {"z": (1e-5, 0.0), "rh": (1e-5, 0.0)}
    if row.epi == "gru_q":
        return {"h": (2e-5, 0.0)}
    if row.norm:
        return {"out": (norm_bf16x3_gate(row)[0], 0.0) if row.mode == "bf16x3" else (5e-5, 1e-5)}
    if row.key[0] in (SMALL, SMALL_PATCH, F32):
        return {"out": (2e-5, 1e-4)}
    return {"out": ({"bf16x3": 2e-3, "bf16x6": 3e-5, "f16x3": 1e-4}[row.mode], 0.0)}


# ------------------------------------------------------------------------------------------------
# CPU tests


@pytest.mark.parametrize("row", ROWS, ids=repr)
def test_row_plans_as_stated(row):
    _, lib = _lib()
    d = plan_descriptor(row)
    rc, p = query(lib, ctypes.byref(d))
    assert_plan(row, rc, p)


def test_plan_query_refuses_what_the_launch_refuses():
    _, lib = _lib()
    d = plan_descriptor(BY_NAME["direct 40->96 3x3 f16x3"])
    out = (ctypes.c_int * 16)()
    assert lib.accflow_conv_plan_query(ctypes.byref(d), out, 15) == 1 and lib.accflow_conv_plan_query(None, out, 16) == 1
    assert lib.accflow_conv_plan_query(ctypes.byref(d), None, 16) == 1 and lib.accflow_conv_plan_query(ctypes.byref(d), out, 16) == 0
    d.stats, d.stat_slots = DUMMY, 7                 # not the slot count of the planned route (8)
    assert lib.accflow_conv_plan_query(ctypes.byref(d), out, 16) == 1
    d = plan_descriptor(BY_NAME["im2col 64x64 16->64 3x3 s2 f16x3"])
    d.in_norm = DUMMY                                # the im2col kernel cannot normalise on load
    assert lib.accflow_conv_plan_query(ctypes.byref(d), out, 16) == 1
    d = plan_descriptor(BY_NAME["direct 40->96 3x3 f16x3"])
    d.Kpad += 32                                     # conv_validate
    assert lib.accflow_conv_plan_query(ctypes.byref(d), out, 16) == 1 and list(out) == [0] * 16


def test_table_is_complete():
    """Every instantiation a default process can launch has a row; the sources are counted, so a new launch line or `case`
    fails here until it gets a row (or a named switch-only entry)."""
    def src(name):
        return open(os.path.join(CSRC, name)).read()
    tabled = set()
    for r in ROWS:
        tabled.update(instantiations(r))
    # the direct kernel's launch lines
    files = sorted(f for f in os.listdir(CSRC) if re.fullmatch(r"conv2d_direct_v_\w+\.hip", f))
    assert files == sorted(DIRECT_ARGS), files
    n = 0
    for f in files:
        got = re.findall(r"hipLaunchKernelGGL\(\(conv2d_direct_bf16s_kernel<([^>]*)>\)", src(f))
        assert sorted(got) == sorted(DIRECT_ARGS[f]), (f, got)
        for a in got:
            n += 1
            if DIRECT_ARGS[f][a] is None:
                assert (f, a) in tabled, "no row runs %s <%s>" % (f, a)
            else:
                assert (f, a) not in tabled and DIRECT_ARGS[f][a].startswith("ACCFLOW_"), (f, a)
    assert n == 24 and len(SWITCH_ONLY) == 3
    # the `case` labels of the im2col launcher (each tile in the three split modes) and of the fp32-MFMA launcher
    body = src("conv2d_bf16s.hip").split("int accflow_launch_conv_bf16s(")[1].split("\n}\n")[0]
    assert tuple(int(c) for c in re.findall(r"^\s*case (\d+):", body, flags=re.M)) == IM2COL_CASES
    for c in IM2COL_CASES:
        for m in SPLIT_MODES:
            assert ("conv2d_bf16s.hip", "%d mode %d" % (c, MODE[m])) in tabled, (c, m)
    body = src("conv2d_f32.hip").split("int accflow_launch_conv_f32(const")[1].split("\n}\n")[0]
    assert tuple(int(c) for c in re.findall(r"^\s*case (\d+):", body, flags=re.M)) == F32_CASES
    for c in F32_CASES:
        assert ("conv2d_f32.hip", "%d" % c) in tabled, c
    # the multi-source launch lines
    files = sorted(f for f in os.listdir(CSRC) if re.fullmatch(r"conv_s16m_v\d\.hip", f))
    assert files == sorted(S16M_ARGS)
    for f in files:
        got = re.findall(r"\(conv_s16m_kernel<([^>]*)>\)", src(f))
        assert got == S16M_ARGS[f], (f, got)
        for a in got:
            assert (f, a) in tabled, (f, a)
    # the <= 4-channel kernels (accflow_launch_conv_small) and the stem
    conv = src("conv_small.hip")
    for co in (2, 4):
        assert conv.count("hipLaunchKernelGGL((conv2d_small_cout_kernel<%d>)" % co) == 1 and ("conv_small.hip", "small<%d>" % co) in tabled
        assert conv.count("hipLaunchKernelGGL((conv2d_small_cout_patch_kernel<%d>)" % co) == 1 and ("conv_small.hip", "small_patch<%d>" % co) in tabled
    assert len(re.findall(r"hipLaunchKernelGGL\(\(conv2d_small_cout", conv)) == 4
    assert ("conv_stem.hip", "stem") in tabled
    # the restated launch rules: the lines they restate
    direct = src("conv2d_direct.hip")
    for line in ("rc = p.loop == CONV_LOOP_TAP9 ? accflow_direct_launch_s16k9(d, 2, true, grid, st) : accflow_direct_launch_s16tg(d, grid, st);",
                 "if (p.loop == CONV_LOOP_TAP5) rc = accflow_direct_launch_s16k(d, 5, grid, st);",
                 "else if (p.loop == CONV_LOOP_TAP9) rc = accflow_direct_launch_s16k9(d, p.tc, false, grid, st);",
                 "else rc = accflow_direct_launch_s16(d, p.tc, grid, st);",
                 "rc = f16 ? accflow_direct_launch_f16_norm(d, p.tc, p.loop == CONV_LOOP_TAP9, grid, st) : accflow_direct_launch_bf16_norm(d, p.tc, nt, grid, st);",
                 "rc = f16 ? accflow_direct_launch_f16(d, p.tc, p.w4, grid, st) : accflow_direct_launch_bf16(d, p.tc, nt, p.w4, grid, st);"):
        assert line in direct, line
    plan = src("conv_plan.cpp")
    assert "return plan_direct_tile(part, tail ? 1 : 2, false, p);" in plan
    assert "else if (sw.direct_kt9 && (tc == 1 || p.w4) && k3) p.loop = CONV_LOOP_TAP9;" in plan


def tap_moved(row, I, y, co, ci, ky, kx):
    """The reference with w[co, ci, ky, kx] zeroed: only channel `co` of the raw convolution moves, by that weight times the
    shifted input channel."""
    x = conv_input64(row, I)[:, ci:ci + 1]
    onehot = torch.zeros(1, 1, *row.k, dtype=torch.float64)
    onehot[0, 0, ky, kx] = 1.0
    y2 = y.clone()
    y2[:, co:co + 1] -= float(I["w"][co, ci, ky, kx]) * F.conv2d(x, onehot, stride=row.stride, padding=row.pad)
    return finish64(row, I, y2)


@pytest.mark.parametrize("row", ROWS, ids=repr)
def test_gate_has_teeth(row):
    I = inputs(row)
    y, ref = reference(row)
    g = gates(row)
    for co, ci, ky, kx in probes(row):
        moved = tap_moved(row, I, y, co, ci, ky, kx)
        worst = 0.0
        for name, r in ref.items():
            atol, rtol = g[name]
            worst = max(worst, float(((moved[name] - r).abs() / (atol + rtol * r.abs())).max()))
        assert worst > TEETH, (row, (co, ci, ky, kx), worst)


# ------------------------------------------------------------------------------------------------
# GPU tests


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as o
    assert torch.cuda.is_available()
    assert o.KSPLIT_MAX_PIXELS == KSPLIT_MAX_PIXELS and o.USE_KSPLIT and o.USE_PATCH and not o.S16_VIA_MULTI
    return o


@pytest.fixture
def trace(monkeypatch):
    """[(rc, plan)] of every accflow_conv2d_f32 call: the plan query sees the descriptor the launch gets."""
    from accflow_amd import _lib as L
    lib = L.load()
    real = lib.accflow_conv2d_f32
    calls = []

    def wrapper(dref, stream):
        calls.append(query(lib, dref))
        return real(dref, stream)
    monkeypatch.setattr(lib, "accflow_conv2d_f32", wrapper)
    return calls


def framed(B, C, H, W):
    """A (B, C, H, W) destination inside a sentinel-filled buffer, 8 channels of margin on either side."""
    big = torch.full((B, C + 16, H, W), SENT, dtype=torch.float32, device="cuda")
    return big, big[:, 8:8 + C]


def frame_intact(big, C):
    return bool((big[:, :8] == SENT).all()) and bool((big[:, 8 + C:] == SENT).all())


def run_row(ops, row):
    """-> ({name: fp32 tensor on the CPU}, {name: S16 copy as fp32}, statistics or None, intact)"""
    I = inputs(row)
    B, H, W = row.shape
    dv = lambda t: t.cuda() if t is not None else None  # noqa: E731
    act = {"store": ops.ACT_NONE, "res_relu": ops.ACT_RELU, "accum": ops.ACT_NONE, "gru_zr": ops.ACT_SIGMOID, "gru_q": ops.ACT_TANH}[row.epi]
    epi = {"store": ops.EPI_STORE, "res_relu": ops.EPI_RES_RELU, "accum": ops.EPI_ACCUM, "gru_zr": ops.EPI_GRU_ZR, "gru_q": ops.EPI_GRU_Q}[row.epi]
    out, out16, stats, intact = {}, {}, None, True
    with ops.conv_mode(row.mode), ops.ksplit_scope(not row.nokws):
        xs = [dv(x) for x in I["x"]]
        if row.s16:
            xs = [ops.S16.from_float(x) for x in xs]
            for a, x in zip(xs, I["x"]):
                assert torch.equal(a.to_float().cpu(), x)         # the reference reads exactly what the tensor holds
        if row.kind == "tapgemm":
            p1 = ops.PackedConv(dv(I["w"]), dv(I["b"]), padding=row.pad)
            p2 = ops.PackedConv(dv(I["w2"]), dv(I["b2"]), padding=1)
            assert ops.tapgemm_eligible(p1, p2, xs[0])
            big, dst = framed(B, 2, H, W)
            ops.conv2d_tapgemm(p1, p2, xs[0], out=dst)
            return {"out": dst.cpu()}, out16, None, frame_intact(big, 2)
        big, dst = framed(B, row.n_out, row.OH, row.OW)
        if row.kind == "multi":
            pk = ops.PackedMulti.from_cat(dv(I["w"]), dv(I["b"]), list(row.cins), row.pad)
            ops.conv2d_multi(pk, xs, out=dst, lay=row.lay)
            return {"out": dst.cpu()}, out16, None, frame_intact(big, row.n_out)
        pk = ops.PackedConv(dv(I["w"]), dv(I["b"]), stride=row.stride, padding=row.pad, C0=row.cins[0])
        kw = dict(out=dst, act=act, epi=epi)
        if "e0" in I:
            kw["e0"] = dv(I["e0"])
        if "e1" in I:
            kw["e1"] = dv(I["e1"])
        if row.pre:
            kw["pre"] = dv(I["pre"])
        big2 = None
        if row.epi == "gru_zr":
            big2, kw["out2"] = framed(B, row.n_out, row.OH, row.OW)
        big16 = None
        if row.out16:
            big16 = ops.S16.empty(B, row.n_out + 16, row.OH, row.OW, dst.device)
            big16.data.fill_(SENT16)
            kw["out16"] = big16.channels(8, 8 + row.n_out)
        if row.norm:
            kw["in_norm"] = dv(I["in_norm"])
        if row.stats:
            kw["want_stats"] = True
        r = ops.conv2d(pk, xs[0], xs[1] if len(xs) > 1 else None, **kw)
        assert r is not None, "the planned route normalises on load"
        if row.stats:
            stats = r[1]
        intact = frame_intact(big, row.n_out)
        if row.epi == "gru_zr":
            out["z"], out["rh"] = dst.cpu(), kw["out2"].cpu()
            intact = intact and frame_intact(big2, row.n_out)
        else:
            out["h" if row.epi == "gru_q" else "out"] = dst.cpu()
        if row.out16:
            out16["out"] = kw["out16"].to_float().cpu()
            O = row.n_out // 8
            intact = intact and bool((big16.data[:, :1] == SENT16).all()) and bool((big16.data[:, 1 + O:] == SENT16).all())
    return out, out16, stats, intact


@gpu
@pytest.mark.parametrize("row", ROWS, ids=repr)
def test_route_vs_float64(ops, trace, row):
    ops.guard_tripped()
    out, out16, stats, intact = run_row(ops, row)
    assert not ops.guard_tripped(), "the inputs are inside the fp16 split's range"
    # the route: the one launch of the row (the pack kernels do not go through accflow_conv2d_f32)
    assert len(trace) == 1, trace
    assert_plan(row, *trace[0])
    assert intact, "something outside the destination's channels changed"
    ref, g = reference(row)[1], gates(row)
    assert sorted(out) == sorted(ref)
    worst = 0.0
    for name, r in ref.items():
        atol, rtol = g[name]
        tol = atol + rtol * r.abs()
        ratio = float(((out[name].double() - r).abs() / tol).max())
        worst = max(worst, ratio)
        extra = ""
        if row.norm and row.mode == "bf16x3":
            extra = " (gate %.3e = %g x (E32 %.3e + E_split %.3e))" % ((atol, MARGIN) + norm_bf16x3_gate(row)[1:])
        print("%s [%s]: max err %.3e, err / gate %.3f%s" % (row, name, float((out[name].double() - r).abs().max()), ratio, extra))
        assert ratio <= 1.0, (row, name, ratio)
        if name in out16:
            tol16 = tol + S16_REL * r.abs() + S16_ABS
            ratio16 = float(((out16[name].double() - r).abs() / tol16).max())
            print("%s [%s, S16 copy]: err / (gate + storage) %.3f" % (row, name, ratio16))
            assert ratio16 <= 1.0, (row, name, ratio16)
    if row.stats:
        assert (stats is not None) == (row.slots > 0), row
    if stats is not None:
        # {sum, M2, n} per slot: every output pixel counted once, and the planes' means are the reference's (the mean of
        # errors within the gate is within the gate; 1e-6 for the fp32 partial sums)
        part = stats.partial.double().cpu()
        assert stats.slots == row.slots and tuple(part.shape) == (row.shape[0], row.cout, row.slots, 3)
        assert bool((part[..., 2].sum(dim=2) == row.OH * row.OW).all()), "every output pixel counted exactly once"
        r = ref["out"]
        mean = part[..., 0].sum(dim=2) / (row.OH * row.OW)
        atol, rtol = g["out"]
        assert float((mean - r.mean(dim=(2, 3))).abs().max()) <= atol + rtol * float(r.abs().max()) + 1e-6
