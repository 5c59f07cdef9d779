"""The fp16 range guard of every kernel that reports to it: each reporting site is made to trip, and to stay quiet, from both
sides of the threshold, at the positions where a kernel can forget an operand.

The f16x3 mode carries an activation as fp16 hi + lo of x * 2^4.  A kernel that performs the split ORs 1 into a device flag
when !(|x * 16| < 65520) - that is |x| >= 4095.0, +-inf or NaN - and ops.with_range_guard / ops.optimistic /
parallel.SequencePipeline re-run the stage in bf16x6 when they read 1.  The thresholds are the code's, not measured:
    TRIP = 4095.0        CLEAR = nextafter(float32(4095), 0) = 4095 - 2^-12
A value that cannot be placed exactly (a convolution output) is put on its side by the float64 reference, with a margin of
2^-10 (4 at this magnitude; the kernels err by ~1e-3 there): |ref| * 16 <= 65520 (1 - 2^-10) for every guarded element of a
clear case, >= 65520 (1 + 2^-10) for the probed element of a trip case (test_side_conditions, CPU).

A. Convolutions (rows of test_conv_routes.ROWS, and rows added here where that table has no S16 destination; every launch
   traced and held to the row's plan with C.trace / C.assert_plan; destinations framed by sentinels)
  test_input_side         every f16x3 row with an fp32 source (direct f16, normalise-on-load, im2col, stem, tail cuts, in-kernel
                          and split-K epilogues): one element = CLEAR (quiet, second read False, every output element against
                          float64) and = TRIP (tripped, second read False, frame intact) at: first pixel / channel (the image
                          border's halo), the last contributing pixel of the ragged last tile of the last item in the last
                          channel (the last real channel of a 40-channel source; the channel only the last K-part loads), the
                          first pixel of the second 4 x 32 tile (the halo of the first), a (channel, pixel) that the direct
                          kernel stages only as a thread's second item, the last channel of the first source and the first
                          of the second.  At the first position also -CLEAR, -TRIP, +inf, -inf, NaN.  The
                          normalised value relu((x - mean) * rstd) is what is guarded: the probed channels carry mean 0,
                          rstd 1; negative values are quiet there (they normalise to 0), a raw 5000 with rstd 0.5 is quiet, a
                          raw 13 with rstd 1 / sqrt(1e-5) trips.
  test_bf16_rows_quiet    the bf16x3 / bf16x6 rows with TRIP, 1e4, NaN in the input: the flag stays 0.
  test_output_side        S16 destinations: the general epilogue (fp32 source; Cout 64, 80 - not a multiple of 32 -, 76 - partial
                          last octet; act NONE and RELU), the lean epilogue (S16 source, stem), the multi-source kernel on
                          every layout (lean store; the lean residual form with an fp32 and an S16 residual), GRU_ZR / GRU_Q in
                          the kernel and through the split-K reduce (octet form), STORE / ACCUM / RES_RELU through the
                          reduce's 4-channel form, the tail cut with probes in the head's last and the tail's first channel.
                          One output = w 64 x input 63 (clear) or 65 (trip); ACCUM / RES_RELU: e0 = 4000 / 4200; GRU_ZR: r = 1
                          (pre-activation 4032: fp32 exp(-4032) is 0) and h = CLEAR / TRIP, the z half at pre-activation 4160
                          and, where the row has `pre`, 1e6: quiet; GRU_Q: z = 0, h = CLEAR / TRIP.  Positions: first pixel,
                          last pixel of the last item; first and last channel.
  test_gru_on_s16_state   the packed-operand GRU epilogue (S16 state, pixel-major z / pre): a state at the largest S16 value
                          stays quiet through GRU_ZR (r = 1) and GRU_Q (z = 0); NaN in `pre` trips on r rows and q rows and is
                          quiet on z rows (a gate is not split); inf in `pre` is quiet (sigmoid / tanh give 1).
  test_norm_refuses_s16   normalise-on-load with an S16 destination is refused by ops.conv2d: that combination has no route.
  test_no_stray_read      40-channel and two-source rows with the sources as channel slices (batch-strided) of a buffer whose
                          other channels hold NaN and 1e30: quiet, outputs torch.equal to the dense run.
  Near the top of the range the result must still be right: the clear cases compare with float64 under
      gate = row gate (C.gates) + MARGIN x (E32 + E_split),         MARGIN = C.MARGIN = 4
  E32 = error of a float32 CPU evaluation (F.conv2d + the epilogue in float32) of the same inputs, E_split = error of a
  float64 evaluation of the two-term split model (products hh, hl, lh; activations split as ops.S16.from_float does, weights
  as csrc/pack_terms.h: w 2^k = hi + lo with the row maximum 2^k in [2^10, 2^11)); each is the larger of its value on the
  unspiked frame (once per row) and on the case (E32: the whole spiked item; E_split: the output pixels the spike
  reaches - the others are the frame's).  S16 copies: + S16_REL |ref| + S16_ABS.  The gate and its parts are printed.
  Output-side cases add acc_steps 2^-24 |ref| (case_gate explains: ONE output is large there, E32 is a single draw).
  test_lo_term_has_teeth (CPU): dropping the lo term of the spiked activation (CLEAR * 16 = 65504 + 16) moves the reference
  by more than TEETH x that gate - for the store / residual / accumulate epilogues; a GRU gate fed 4095 x w is saturated and
  cannot show it, which is stated instead of asserted.

B. The other reporters
  test_lookup_s16         corr_lookup_s16 (Sb: P = 99): one pyramid cell = CLEAR / TRIP read with weight 1, at every level, at
                          tap 80 (flushed alone), in the last pixel; a TRIP cell that only zero-weight / no tap reads: quiet.
  test_lookup_alt_s16     corr_lookup_alt_s16 (9 x 11, C = 64): the feature pair q = e_c, k = 8 CLEAR / 8 TRIP e_c (1 / sqrt(C) =
                          1/8: the product is exact), every level (the 2^l x 2^l block of cells it pools), tap 80, last pixel.
  test_aggregate_s16 / _alt   gamma = 0: out = fmap; fmap = CLEAR / TRIP at first / last pixel, first / last octet, last of
                          n = 2 items.
  test_kmajor_packs       corr_volume_disp (fmap1 is packed times 16 / sqrt(C) = 2 at C = 64: threshold 32760; fmap2 times
                          16: 4095), corr_pack (4095), gma_attention_s16 / gma_attention_alt (k times scale 16: 4095 / scale
                          with scale = 1/4 -> 16380; q: 4095): first and last (channel, pixel) of each operand.
                          ops.corr_volume runs bf16x6 in f16x3 mode and reports nowhere: 1e4 stays quiet and finite.
  test_pos_attention_quiet    gma_attention_pos_s16 / _t take no guard: 1e4 in q, flag 0, result finite.

C. test_sites_complete (CPU): the atomicOr( reporting sites of csrc/, counted per file, each mapped to the tests that reach it.

Not built: normalise-on-load with an S16 destination (no route, see above).  Clear-side comparisons of part B use the float64
references and gates of the files they come from (test_lookup_routes, test_alt_corr, test_corr_routes, test_gma_routes).
Deviations from what was asked, each because the arithmetic says so: +-inf in a GRU pre-activation is quiet (sigmoid / tanh
saturate to 1, the result is in range); ops.corr_volume reports nowhere (it runs bf16x6); the lo-term teeth are asserted for
the store / residual / accumulate epilogues only.

Found and fixed: the normalise-on-load kernels formed relu with fmaxf, which turns a NaN into 0 - a NaN in the raw input
reached the convolution as 0 and the guard stayed quiet (test_input_side[in norm ...], `first nan`); the kernel now selects.

Measured on the MI355X, 2026-10-21, all 125 GPU cases passing in 6.3 s - largest error / gate per comparison:
    input side, fp32 output, 30 rows: 0.406 (in no tail 64->200); gates 1.1e-5 (GRU rows) .. 7.4e-3, e.g. direct 40->64 3x3 at
      the last position: 8.97e-4 = 1e-4 + 4 x (E32 4.81e-5 + E_split 1.51e-4), error 0.130 of it
    output side: fp32 0.124, S16 copy 0.121 (both out16 multi lay 3 tap9)
    corr_lookup_s16 0.108;  corr_lookup_alt_s16 0.240;  corr_volume_disp / corr_pack levels 0.621
    gma_attention_s16 0.196;  gma_attention_alt (read back through the aggregation) 0.196;  aggregations: torch.equal to fmap
No gate, margin, shape or input was chosen from these figures.  (Before the accumulator term of case_gate existed, one
output-side case, out16 direct 40->76 relu / channel 75, measured 1.085 of the input-side formula: its E32 had come out at
0.4 ulp of the 4032 output, the kernel's error at 2.4 ulp; the term is derived from the format, see case_gate.)
Mutations of scratch copies of the library, and the cases that then fail: the range check of the second staged item dropped
in store_patch - test_input_side of all 22 direct-kernel rows (the `second staged item` position); of the partial flush in
corr_disp.hip - test_lookup_s16[l0-p0-tap80], [l3-p0-tap80]; of the reduce kernel's 4-channel form - test_output_side of the 5
split-K rows with whole octets that are not GRU_ZR and test_aggregate_guard[*-s16]; the lo term of s16_split2 zeroed - 30
test_input_side, 17 test_output_side, 2 + 2 test_kmajor_packs_* cases.
"""
import copy
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import test_conv_routes as C
import test_lookup_routes as LK

R = C.R
gpu = pytest.mark.gpu
trace = C.trace
TEETH, MARGIN = C.TEETH, C.MARGIN
S16_REL, S16_ABS = C.S16_REL, C.S16_ABS
LIMIT = 65520.0
TRIP = 4095.0
CLEAR = float(torch.nextafter(torch.tensor(4095.0, dtype=torch.float32), torch.tensor(0.0, dtype=torch.float32)))
assert CLEAR == 4095.0 - 2.0 ** -12
CLEAR_BOUND, TRIP_BOUND = LIMIT * (1 - 2.0 ** -10), LIMIT * (1 + 2.0 ** -10)
INF, NAN = float("inf"), float("nan")
W_SPIKE, X_CLEAR, X_TRIP = 64.0, 63.0, 65.0
E0_CLEAR, E0_TRIP = 4000.0, 4200.0
S, E = C.S, C.E


def tripping(v):
    return not (abs(v * 16.0) < LIMIT)


assert not tripping(CLEAR) and tripping(TRIP) and tripping(NAN) and tripping(-INF)


# ------------------------------------------------------------------------------------------------
# rows


class GRow(C.Row):
    """A row of this module: a copy of a C row under its own name / share, or a new one; act: the activation where it is not
    the epilogue's own; probes: (output channel, input channel) pairs whose centre weight is W_SPIKE."""
    act, probes, e0_s16, base_row = None, (), False, None


def derived(row, prefix):
    g = copy.copy(row)
    g.__class__ = GRow
    g.name = g.share = "%s %s" % (prefix, row.name)
    g.base_row = row
    return g


def new_row(name, *a, act=None, e0_s16=False, **kw):
    g = GRow(name, *a, **kw)
    g.act, g.e0_s16 = act, e0_s16
    return g


IN_ROWS = [derived(r, "in") for r in C.ROWS
           if r.mode == "f16x3" and not r.s16 and r.kind == "conv" and r.key[0] in (C.DIRECT, C.IM2COL, C.STEM)]
BF_ROWS = [derived(r, "bf") for r in C.ROWS
           if r.mode in ("bf16x3", "bf16x6") and not r.s16 and r.kind == "conv" and r.key[0] in (C.DIRECT, C.IM2COL)]

OUT_ROWS = [derived(r, "out") for r in C.ROWS if r.out16]
assert [r.base_row.name for r in OUT_ROWS] == ["tail S16 256->192 3x3 res_relu out16", "S16 tap5 64+64->128 5x1 split-K out16",
                                                "S16 tap9 128->128 3x3 out16"]
_d, _s = C.direct, C.s16m
OUT_ROWS += [
    # the general epilogue of the fp32-source direct kernel (conv_epilogue_impl<.., OUT16>)
    new_row("out16 direct 40->64 3x3", (40,), 64, (3, 3), S, _d(1), out16=True),
    new_row("out16 direct 40->64 3x3 relu", (40,), 64, (3, 3), S, _d(1), out16=True, act="relu"),
    new_row("out16 direct 40->80 3x3", (40,), 80, (3, 3), S, _d(2), out16=True),
    new_row("out16 direct 40->76 3x3 relu", (40,), 76, (3, 3), S, _d(2), out16=True, act="relu"),
    # the lean epilogue: S16 source (the table's tap9 row, act NONE) with RELU, and the stem
    new_row("out16 S16 tap9 128->128 3x3 relu", (128,), 128, (3, 3), S, _d(2, loop=C.TAP9), s16=True, out16=True, nokws=True,
            act="relu"),
    new_row("out16 stem 3->64 7x7 s2", (3,), 64, (7, 7), (2, 26, 74), C.plain(C.STEM, "f16x3"), stride=2, out16=True),
    new_row("out16 stem 3->64 7x7 s2 relu", (3,), 64, (7, 7), (2, 26, 74), C.plain(C.STEM, "f16x3"), stride=2, out16=True, act="relu"),
    # GRU_ZR / GRU_Q in the kernel ...
    new_row("out16 gru_zr 32+16->64 1x5", (32, 16), 64, (1, 5), E, _d(1), epi="gru_zr", pre=True, out16=True),
    new_row("out16 gru_zr 48->96 1x5", (48,), 96, (1, 5), E, _d(2), epi="gru_zr", out16=True),
    new_row("out16 gru_q 32+16->32 5x1", (32, 16), 32, (5, 1), E, _d(1), epi="gru_q", pre=True, out16=True),
    new_row("out16 gru_q 48->128 5x1", (48,), 128, (5, 1), E, _d(2), epi="gru_q", pre=True, out16=True),
    new_row("out16 accum 48->64 3x3", (48,), 64, (3, 3), E, _d(1), epi="accum", out16=True),
    new_row("out16 res_relu 48->128 3x3", (48,), 128, (3, 3), E, _d(2), epi="res_relu", out16=True),
    # ... and through the split-K reduce: GRU_ZR takes the octet form, everything else with whole octets the 4-channel form
    new_row("out16 gru_zr 128+16->64 1x5 split-K", (128, 16), 64, (1, 5), E, _d(1, z=True), epi="gru_zr", pre=True, out16=True),
    new_row("out16 gru_zr 144->96 1x5 split-K", (144,), 96, (1, 5), E, _d(2, z=True), epi="gru_zr", out16=True),
    new_row("out16 gru_q 128+16->32 5x1 split-K", (128, 16), 32, (5, 1), E, _d(1, z=True), epi="gru_q", pre=True, out16=True),
    new_row("out16 store 144->64 3x3 split-K", (144,), 64, (3, 3), E, _d(1, z=True), out16=True),
    new_row("out16 store 144->76 3x3 split-K", (144,), 76, (3, 3), E, _d(2, z=True), out16=True),     # (partial octet: the octet form)
    new_row("out16 accum 144->64 3x3 split-K", (144,), 64, (3, 3), E, _d(1, z=True), epi="accum", out16=True),
    new_row("out16 res_relu 144->128 3x3 split-K", (144,), 128, (3, 3), E, _d(2, z=True), epi="res_relu", out16=True),
]
for _lay, _cout in ((0, 128), (1, 64), (2, 64), (3, 96)):
    OUT_ROWS.append(new_row("out16 multi lay %d tap9" % _lay, (32, 32), _cout, (3, 3), S, _s(_lay, C.TAP9), s16=True, nokws=True,
                            kind="multi", lay=_lay, out16=True))
    OUT_ROWS.append(new_row("out16 multi lay %d tap9 relu" % _lay, (32, 32), _cout, (3, 3), S, _s(_lay, C.TAP9), s16=True, nokws=True,
                            kind="multi", lay=_lay, out16=True, act="relu"))
# the lean residual epilogue of the multi-source kernel (Cout a multiple of the layout's rows), fp32 and S16 residual
OUT_ROWS += [
    new_row("out16 multi lay 0 res_relu", (32, 32), 128, (3, 3), S, _s(0, C.TAP9), s16=True, nokws=True, kind="multi", lay=0,
            out16=True, epi="res_relu"),
    new_row("out16 multi lay 1 res_relu S16 e0", (32, 32), 64, (3, 3), S, _s(1, C.TAP9), s16=True, nokws=True, kind="multi", lay=1,
            out16=True, epi="res_relu", e0_s16=True),
]
SLICE_ROWS = [derived(C.BY_NAME[n], "sliced") for n in
              ("direct 40->64 3x3 f16x3", "direct 40->96 3x3 f16x3", "norm f16 generic 40->96 3x3", "gru_zr 32+16->64 1x5",
               "gru_q 32+16->32 5x1", "gru_zr 128+16->64 1x5 split-K", "gru_q 128+16->32 5x1 split-K",
               "S16 tap5 64+64->128 5x1 split-K out16", "multi lay 0 tap9", "multi lay 2 generic")]
ALL_ROWS = IN_ROWS + BF_ROWS + OUT_ROWS + SLICE_ROWS
assert len({r.name for r in ALL_ROWS}) == len(ALL_ROWS)


def act_name(g):
    return g.act or {"store": "none", "res_relu": "relu", "accum": "none", "gru_zr": "sigmoid", "gru_q": "tanh"}[g.epi]


def weight_probes(g):
    """[(output channel, input channel)] whose centre weight is W_SPIKE: one input element then places one output."""
    if g not in OUT_ROWS or (g.epi in ("accum", "res_relu", "gru_q") and not g.e0_s16):
        return []       # (an S16 residual cannot hold the spike itself: that row places its output like a plain store)
    ci = [0, g.cin - 1, 1, g.cin - 2]
    if g.epi == "gru_zr":       # r rows (the S16 copy holds r * h): first and last; one z row
        return [(g.cout // 2, ci[0]), (g.cout - 1, ci[1]), (0, ci[2])]
    co = [0, g.cout - 1] + ([g.tail[0] - 1, g.tail[0]] if g.tail else [])
    return list(zip(co, ci))


def centre(g):
    return g.k[0] // 2, g.k[1] // 2


_inputs = {}


def inputs(g):
    """The row's inputs (CPU, never modified afterwards): the C row's, with W_SPIKE weights for the output probes and
    {mean 0, rstd 1} on the probed channels of a normalise-on-load row."""
    if g.name not in _inputs:
        I = {k: ([t.clone() for t in v] if isinstance(v, list) else v.clone() if v is not None else None)
             for k, v in C.inputs(g.base_row or g).items()}
        if g.norm:
            for c in sorted({p[1] for p in in_positions(g).values()}):
                I["in_norm"][:, c, 0], I["in_norm"][:, c, 1] = 0.0, 1.0
        ky, kx = centre(g)
        for co, ci in weight_probes(g):
            I["w"][co, ci, ky, kx] = W_SPIKE
        if g.e0_s16:
            I["e0"] = C.s16_value(I["e0"])
        _inputs[g.name] = I
    return _inputs[g.name]


def modified(I, mods):
    """A shallow copy of I with the mods applied to clones: (field, index, value); field x0 / x1 = source 0 / 1."""
    J = dict(I)
    J["x"] = list(I["x"])
    done = set()
    for field, idx, val in mods:
        if field in ("x0", "x1"):
            k = int(field[1])
            if field not in done:
                J["x"][k] = J["x"][k].clone()
            J["x"][k][idx] = val
        else:
            if field not in done:
                J[field] = J[field].clone()
            J[field][idx] = val
        done.add(field)
    return J


def x_field(g, c):
    """(field, channel inside the source) of channel c of the concatenated input"""
    return ("x0", c) if c < g.cins[0] else ("x1", c - g.cins[0])


def x_mod(g, b, c, iy, ix, val):
    f, cs = x_field(g, c)
    return (f, (b, cs, iy, ix), val)


# ------------------------------------------------------------------------------------------------
# the three evaluations (float64 reference, float32, float64 of the split model) and the gate


def conv_in(g, I, dtype):
    x = I["x"][0] if len(I["x"]) == 1 else torch.cat(I["x"], 1)
    if g.norm:      # float64: of the float32 data; float32: as a float32 machine forms it
        mr = I["in_norm"].to(dtype)
        x = torch.relu((x.to(dtype) - mr[:, :, 0, None, None]) * mr[:, :, 1, None, None])
    return x.to(dtype)


def split_f16(a32):
    """ops.S16.from_float's arithmetic -> (hi, lo) / 16 in float64"""
    assert a32.dtype == torch.float32
    xs = a32 * 16.0
    hi = xs.half()
    lo = (xs - hi.float()).half()
    return hi.double() / 16.0, lo.double() / 16.0


def split_w16(w32):
    """csrc/pack_terms.h: per output row k with max |w| 2^k in [2^10, 2^11); w 2^k = fp16 hi + fp16 lo -> (hi, lo) 2^-k, float64"""
    m = w32.abs().amax(dim=(1, 2, 3))
    e = torch.frexp(m)[1]
    k = torch.where(m > 0, 11 - e, torch.zeros_like(e)).clamp(-100, 100)
    mul = torch.ldexp(torch.ones_like(m), k).view(-1, 1, 1, 1)
    ws = w32 * mul
    assert bool(((ws / mul) == w32).all())
    hi = ws.half()
    lo = (ws - hi.float()).half()
    return hi.double() / mul.double(), lo.double() / mul.double()


def finish(g, I, y, dtype, sl=None):
    """The epilogue in `dtype` on the raw convolution y (+ bias + pre): {name: tensor}; sl: an index applied to the operands
    (y is then a batch of single pixels (n, Cout))."""
    def op(name):
        t = I[name].to(dtype)
        return t[sl] if sl is not None else t
    a = act_name(g)
    if g.epi == "store":
        return {"out": torch.relu(y) if a == "relu" else y}
    if g.epi == "res_relu":
        return {"out": torch.relu(op("e0") + torch.relu(y))}
    if g.epi == "accum":
        return {"out": op("e0") + y}
    if g.epi == "gru_zr":
        hd = g.cout // 2
        return {"z": torch.sigmoid(y[:, :hd]), "rh": torch.sigmoid(y[:, hd:]) * op("e0")}
    z = op("e1")
    return {"h": (1 - z) * op("e0") + z * torch.tanh(y)}


def conv3(g, I, x64=None):
    """-> (y64, y32 as float64, y_split) raw convolutions + bias + pre of the whole frame"""
    w, b = I["w"], I["b"]
    kw = dict(stride=g.stride, padding=g.pad)
    a64, a32 = conv_in(g, I, torch.float64), conv_in(g, I, torch.float32)
    y64 = F.conv2d(a64, w.double(), b.double() if b is not None else None, **kw)
    y32 = F.conv2d(a32, w, b, **kw)
    ah, al = split_f16(a32)
    wh, wl = split_w16(w)
    ys = F.conv2d(ah, wh + wl, b.double() if b is not None else None, **kw) + F.conv2d(al, wh, None, **kw)
    if g.pre:
        y64, y32, ys = y64 + I["pre"].double(), y32 + I["pre"], ys + I["pre"].double()
    return y64, y32, ys


_base = {}


def base(g):
    """Once per row, on the unspiked inputs: {"ref": {name: float64}, "e32": {name: float}, "es": {name: float}}"""
    if g.name not in _base:
        I = inputs(g)
        y64, y32, ys = conv3(g, I)
        ref = finish(g, I, y64, torch.float64)
        f32 = finish(g, I, y32, torch.float32)
        fs = finish(g, I, ys, torch.float64)
        _base[g.name] = {"ref": ref, "e32": {n: float((f32[n].double() - r).abs().max()) for n, r in ref.items()},
                         "es": {n: float((fs[n] - r).abs().max()) for n, r in ref.items()}}
    return _base[g.name]


def reached(g, mods):
    """The output pixels [(b, oy, ox)] the mods reach: every tap of an input element, the pixel of an epilogue operand."""
    (kh, kw), s, (ph, pw) = g.k, g.stride, g.pad
    out = []
    for field, idx, _ in mods:
        if field in ("x0", "x1"):
            b, _, iy, ix = idx
            for ky in range(kh):
                for kx in range(kw):
                    ny, nx = iy + ph - ky, ix + pw - kx
                    if ny % s == 0 and nx % s == 0 and 0 <= ny // s < g.OH and 0 <= nx // s < g.OW:
                        out.append((b, ny // s, nx // s))
        else:
            out.append((idx[0], idx[2], idx[3]))
    return list(dict.fromkeys(out))


def patches(a, g, pix):
    """(n, Cin, KH, KW): the input window of each output pixel, zero outside the image"""
    (kh, kw), s, (ph, pw) = g.k, g.stride, g.pad
    H, W = a.shape[2:]
    out = a.new_zeros(len(pix), a.shape[1], kh, kw)
    for n, (b, oy, ox) in enumerate(pix):
        y0, x0 = oy * s - ph, ox * s - pw
        ys, xs, ye, xe = max(y0, 0), max(x0, 0), min(y0 + kh, H), min(x0 + kw, W)
        out[n, :, ys - y0:ye - y0, xs - x0:xe - x0] = a[b, :, ys:ye, xs:xe]
    return out


def case_model(g, mods, drop_lo=None):
    """The three evaluations at the pixels the mods reach -> (J, pix, ref {name: (n, C)}, e32 {name}, es {name}).
    drop_lo = (b, c, iy, ix): the reference with the lo term of that activation dropped instead (teeth)."""
    J = modified(inputs(g), mods)
    pix = reached(g, mods)
    assert pix, (g, mods)
    bb, oy, ox = (torch.tensor(v) for v in zip(*pix))
    sl = (bb, slice(None), oy, ox)
    w, b = J["w"], J["b"]
    b64 = b.double() if b is not None else None
    a32 = conv_in(g, J, torch.float32)
    a64 = conv_in(g, J, torch.float64)
    if drop_lo is not None:
        a64 = a64.clone()
        a64[drop_lo] = split_f16(a32[drop_lo].reshape(1))[0][0]
    p64, p32 = patches(a64, g, pix), patches(a32, g, pix)
    y64 = F.conv2d(p64, w.double(), b64)[:, :, 0, 0]
    ah, al = split_f16(p32)
    wh, wl = split_w16(w)
    ys = (F.conv2d(ah, wh + wl, b64) + F.conv2d(al, wh, None))[:, :, 0, 0]
    if g.pre:
        pre = J["pre"][sl]
        y64, ys = y64 + pre.double(), ys + pre.double()
    ref = finish(g, J, y64, torch.float64, sl)
    fs = finish(g, J, ys, torch.float64, sl)
    es = {n: float((fs[n] - r).abs().max()) for n, r in ref.items()}
    if drop_lo is not None:
        return J, pix, ref, None, es
    # E32: F.conv2d in float32 on the whole spiked item (every mod of a case lies in one item), against the frame's float64
    # reference with the reached pixels replaced by the case's
    it = pix[0][0]
    assert all(p[0] == it for p in pix)
    item = (slice(it, it + 1),)
    y32 = F.conv2d(a32[item], w, b, stride=g.stride, padding=g.pad)
    if g.pre:
        y32 = y32 + J["pre"][item]
    f32 = finish(g, J, y32, torch.float32, item)
    e32 = {}
    for n, r0 in base(g)["ref"].items():
        r = r0[item].clone()
        r[0][:, oy, ox] = ref[n].t()
        e32[n] = float((f32[n].double() - r).abs().max())
    return J, pix, ref, e32, es


def acc_steps(g):
    """Roundings of an fp32 accumulator element: 3 products (hh, hl, lh) per 16-deep matrix-core step over the Kpad-deep
    reduction, the scale / bias fma and the epilogue's addition"""
    return 3 * C.cdiv(g.cin * g.k[0] * g.k[1], 16) + 2


def case_gate(g, e32, es, placed=False):
    """{name: (atol, rtol, E32, E_split)}: the row's gate + MARGIN x (E32 + E_split), each E the larger of the frame's and the case's.
    placed (output-side cases): + acc_steps 2^-24 |ref|.  There ONE output element is ~4032 and E32 is a single draw of a
    float32 summation's error at that element - on the input side the spike reaches hundreds of large outputs and the
    maximum is a statistic.  The placed output carries its whole absolute sum (64 x 63 against ~20 for the rest), so every
    rounding of its accumulator is at most 2^-24 |ref|, and there are acc_steps of them: a bound from the format, 5e-6 relative
    at 3 x 3 x 40 channels, where a dropped lo term is 5e-4."""
    bs = base(g)
    out = {}
    for n, (atol, rtol) in C.gates(g).items():
        a, s_ = max(bs["e32"][n], e32[n]), max(bs["es"][n], es[n])
        out[n] = (atol + MARGIN * (a + s_), rtol + (acc_steps(g) * 2.0 ** -24 if placed else 0.0), a, s_)
    return out


# ------------------------------------------------------------------------------------------------
# cases


def contributes(g, iy, ix):
    return bool(reached(g, [("x0", (0, 0, iy, ix), 0.0)]))


def nearest(g, iy, ix):
    B, H, W = g.shape
    best = None
    for y in range(max(0, iy - 2), min(H, iy + 3)):
        for x in range(max(0, ix - 2), min(W, ix + 3)):
            if contributes(g, y, x) and (best is None or abs(y - iy) + abs(x - ix) < abs(best[0] - iy) + abs(best[1] - ix)):
                best = (y, x)
    assert best is not None, (g, iy, ix)
    return best


def second_staged(g):
    """(c, iy, ix) that the direct kernel stages only as a thread's SECOND item (conv2d_direct_kernel.h: item = tid + 256 i ->
    octet = item / NP of the 16-channel chunk, patch pixel = item % NP, NP = (4 + KH - 1) (32 + KW - 1), patch origin = the
    4 x 32 tile's minus the padding): a channel in the upper octet of its chunk and a pixel whose item number is >= 256 in
    every workgroup whose patch holds it."""
    B, H, W = g.shape
    (kh, kw), (ph, pw) = g.k, g.pad
    PH, PW = 4 + kh - 1, 32 + kw - 1
    NP = PH * PW
    assert g.stride == 1 and 2 * NP > 256
    c = max(c for c in range(g.cins[0]) if c % 16 >= 8)
    for iy in range(min(H, 4)):
        for ix in range(min(W, 32)):
            items = []
            for ty in range(C.cdiv(g.OH, 4)):
                for tx in range(C.cdiv(g.OW, 32)):
                    py, px = iy - (4 * ty - ph), ix - (32 * tx - pw)
                    if 0 <= py < PH and 0 <= px < PW:
                        items.append(NP + py * PW + px)
            if items and min(items) >= 256:
                return c, iy, ix
    raise AssertionError(g)


def in_positions(g):
    """{class: (b, c, iy, ix)} of a row's input probes (every one read by some output)"""
    B, H, W = g.shape
    P = {"first": (0, 0) + nearest(g, 0, 0),
         "last": (B - 1, g.cin - 1) + nearest(g, H - 1, W - 1),
         "second tile": (0, g.cin // 2) + nearest(g, min(4 * g.stride, H - 1), min(32 * g.stride, W - 1))}
    if g.key[0] == C.DIRECT:
        P["second staged item"] = (0,) + second_staged(g)
    if len(g.cins) > 1:
        P["first source's last channel"] = (0, g.cins[0] - 1) + nearest(g, H // 2, W // 2)
        P["second source"] = (B - 1, g.cins[0]) + nearest(g, H // 2, W - 1)
    return P


def in_cases(g):
    """[(label, mods, trips, compare)]"""
    out = []
    for name, (b, c, iy, ix) in in_positions(g).items():
        vals = [CLEAR, TRIP] + ([-CLEAR, -TRIP, INF, -INF, NAN] if name == "first" else [])
        for v in vals:
            trips = tripping(v) and not (g.norm and v < 0)      # relu((x - 0) * 1) of a negative value is 0
            out.append(("%s %r" % (name, v), [x_mod(g, b, c, iy, ix, v)], trips, not tripping(v)))
    if g.norm:      # the guarded value is the normalised one
        b, c, iy, ix = in_positions(g)["last"]
        flat = [("x0", (b, c), 0.0), ("in_norm", (b, c, 0), 0.0)]
        out.append(("raw 5000, rstd 0.5", flat + [("in_norm", (b, c, 1), 0.5), ("x0", (b, c, iy, ix), 5000.0)], False, False))
        out.append(("raw 13, rstd 1/sqrt(1e-5)", flat + [("in_norm", (b, c, 1), 1.0 / math.sqrt(1e-5)), ("x0", (b, c, iy, ix), 13.0)],
                    True, False))
    return out


def out_pixels(g):
    return {"first": (0, 0, 0), "last": (g.shape[0] - 1, g.OH - 1, g.OW - 1)}


def in_pixel(g, oy, ox):
    ky, kx = centre(g)
    return oy * g.stride - g.pad[0] + ky, ox * g.stride - g.pad[1] + kx


def out_cases(g):
    """[(label, mods, trips, probed (name, b, channel of the S16 copy, oy, ox) or None)]"""
    out = []
    half = g.cout // 2
    for pname, (b, oy, ox) in out_pixels(g).items():
        iy, ix = in_pixel(g, oy, ox)
        if g.epi == "store" or g.e0_s16:
            for co, ci in weight_probes(g):
                for v in (X_CLEAR, X_TRIP):
                    out.append(("%s ch %d x %g" % (pname, co, v), [x_mod(g, b, ci, iy, ix, v)], v == X_TRIP, ("out", b, co, oy, ox)))
        elif g.epi in ("accum", "res_relu"):
            for co in (0, g.cout - 1) + ((g.tail[0] - 1, g.tail[0]) if g.tail else ()):
                for v in (E0_CLEAR, E0_TRIP):
                    out.append(("%s ch %d e0 %g" % (pname, co, v), [("e0", (b, co, oy, ox), v)], v == E0_TRIP, ("out", b, co, oy, ox)))
        elif g.epi == "gru_q":
            for co in (0, g.cout - 1):
                for v in (CLEAR, TRIP, -TRIP, NAN):
                    out.append(("%s ch %d h %r" % (pname, co, v), [("e0", (b, co, oy, ox), v), ("e1", (b, co, oy, ox), 0.0)],
                                tripping(v), ("h", b, co, oy, ox)))
        else:       # gru_zr: r = sigmoid(64 x 63 + ...) = 1, r * h = h
            (r0, c0), (r1, c1), (z0, cz) = weight_probes(g)
            for co, ci in ((r0, c0), (r1, c1)):
                for v in (CLEAR, TRIP):
                    out.append(("%s ch %d h %r" % (pname, co, v),
                                [x_mod(g, b, ci, iy, ix, X_CLEAR), ("e0", (b, co - half, oy, ox), v)], v == TRIP,
                                ("rh", b, co - half, oy, ox)))
            z = [x_mod(g, b, cz, iy, ix, X_TRIP)] + ([("pre", (b, z0, oy, ox), 1.0e6)] if g.pre else [])
            out.append(("%s z row at 4160%s" % (pname, " + 1e6" if g.pre else ""), z, False, None))
    return out


# ------------------------------------------------------------------------------------------------
# CPU tests


def g_descriptor(g):
    """C.plan_descriptor plus what a row of this module adds: its activation, the S16 copy and the residual of a multi-source row"""
    _, lib = C._lib()
    d = C.plan_descriptor(g)
    d.act = {"none": 0, "relu": 1, "sigmoid": 2, "tanh": 3}[act_name(g)]
    if g.kind == "multi":
        d.epi = {"store": 0, "res_relu": 1}[g.epi]
        if g.out16:
            d.out16, d.out16_bs = C.DUMMY, lib.accflow_s16_item_words(g.n_out, g.OH, g.OW)
        if g.epi == "res_relu":
            d.e0 = C.DUMMY
            d.e0_bs = lib.accflow_s16_item_words(g.cout, g.OH, g.OW) if g.e0_s16 else g.cout * g.OH * g.OW
            d.e0_fmt = 1 if g.e0_s16 else 0
    return d


@pytest.mark.parametrize("g", OUT_ROWS, ids=repr)
def test_guard_rows_plan_as_stated(g):
    _, lib = C._lib()
    d = g_descriptor(g)
    rc, p = C.query(lib, ctypes.byref(d))
    C.assert_plan(g, rc, p)


def test_rows_cover_the_table():
    """Every f16x3 row of C.ROWS is here: as an input-side row (fp32 source), as an output-side row (S16 destination), or
    it has no reporting site of its own (an S16 source with an fp32 destination: its producer was guarded; the tap GEMM's
    intermediate is tripped by tests/test_hip_parity.py); every bf16 row with an fp32 source is a quiet row."""
    mine = {g.base_row.name for g in IN_ROWS + OUT_ROWS + BF_ROWS if g.base_row is not None}
    for r in C.ROWS:
        if r.mode == "f32":
            continue
        if r.s16 and not r.out16:
            assert r.name not in mine
        else:
            assert r.name in mine, r
    assert len(IN_ROWS) >= 30 and {g.key[0] for g in IN_ROWS} == {C.DIRECT, C.IM2COL, C.STEM}
    assert any(g.norm and g.key[7] for g in IN_ROWS) and any(g.tail for g in IN_ROWS)


@pytest.mark.parametrize("g", IN_ROWS + OUT_ROWS, ids=repr)
def test_side_conditions(g):
    """Every guarded element of a clear case is below CLEAR_BOUND (or is the exactly placed CLEAR), the probed element of a
    trip case is above TRIP_BOUND (or the exactly placed TRIP / inf / NaN) and every other one below CLEAR_BOUND."""
    I = inputs(g)
    bs = base(g)
    if g in IN_ROWS or not g.s16:       # the kernel splits the (normalised) fp32 input: the unspiked frame is clear
        a = conv_in(g, I, torch.float64)
        assert float(a.abs().max()) * 16 <= CLEAR_BOUND
    if g in IN_ROWS:
        for label, mods, trips, compare in in_cases(g):
            J = modified(I, mods)
            a = conv_in(g, J, torch.float64)
            bad = ~(a.abs() * 16 < LIMIT)
            assert int(bad.sum()) == (1 if trips else 0), (g, label)
            assert not (compare and trips)
        return
    name16 = {"store": "out", "res_relu": "out", "accum": "out", "gru_zr": "rh", "gru_q": "h"}[g.epi]
    assert float(bs["ref"][name16].abs().max()) * 16 <= CLEAR_BOUND
    for label, mods, trips, probed in out_cases(g):
        J, pix, ref, _, _ = case_model(g, mods)
        v = ref[name16].abs() * 16                  # (n pixels, channels of the S16 copy)
        exact = torch.zeros_like(v, dtype=torch.bool)
        if probed is not None:
            n = pix.index((probed[1], probed[3], probed[4]))
            pv = float(v[n, probed[2]])
            if g.epi in ("gru_zr", "gru_q"):        # placed exactly: r = 1 / z = 0
                want = [m for m in mods if m[0] == "e0"][0][2]
                assert pv == abs(want) * 16 or (pv != pv and want != want), (g, label, pv)
                if g.epi == "gru_zr":
                    assert float(ref["z"].min()) >= 0 and bool((torch.sigmoid(torch.tensor(4000.0)) == 1.0))
            elif trips:
                assert pv >= TRIP_BOUND, (g, label, pv)
            exact[n, probed[2]] = True
            assert tripping(pv / 16) == trips, (g, label, pv)
        rest = v[~exact]
        assert float(rest.max()) <= CLEAR_BOUND, (g, label, float(rest.max()))


TEETH_ROWS = [g for g in IN_ROWS if g.epi in ("store", "res_relu", "accum")]
assert len(TEETH_ROWS) >= 20


@pytest.mark.parametrize("g", TEETH_ROWS, ids=repr)
def test_lo_term_has_teeth(g):
    """CLEAR * 16 = 65504 + 16 (fp16 hi + lo): without the lo term the activation is 4094, and the reference moves by w
    at every tap - more than TEETH x the gate of the case."""
    hi, lo = split_f16(torch.tensor([CLEAR], dtype=torch.float32))
    assert float(hi) == 4094.0 and float(lo) == 1.0
    for label, mods, trips, compare in in_cases(g):
        if not compare or mods[0][2] != CLEAR:
            continue
        f, (b, cs, iy, ix), _ = mods[0]
        c = cs + (g.cins[0] if f == "x1" else 0)
        _, pix, ref, e32, es = case_model(g, mods)
        moved = case_model(g, mods, drop_lo=(b, c, iy, ix))[2]
        gate = case_gate(g, e32, es)
        worst = 0.0
        for n, r in ref.items():
            atol, rtol = gate[n][:2]
            worst = max(worst, float(((moved[n] - r).abs() / (atol + rtol * r.abs())).max()))
        assert worst > TEETH, (g, label, worst)


# ------------------------------------------------------------------------------------------------
# GPU: the convolutions


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as o
    assert torch.cuda.is_available()
    assert o.KSPLIT_MAX_PIXELS == C.KSPLIT_MAX_PIXELS and o.USE_KSPLIT and o.USE_PATCH and not o.S16_VIA_MULTI
    yield o
    _dev.clear()


_dev = {}       # per row on the device: the pack, the inputs, the float64 reference (built once per module)
NAN16 = 0x7E007E00


def dev_state(ops, g):
    if g.name not in _dev:
        I = inputs(g)
        dv = lambda t: t.cuda() if t is not None else None  # noqa: E731
        if g.kind == "multi":
            pk = ops.PackedMulti.from_cat(dv(I["w"]), dv(I["b"]), list(g.cins), g.pad)
        else:
            pk = ops.PackedConv(dv(I["w"]), dv(I["b"]), stride=g.stride, padding=g.pad, C0=g.cins[0])
        D = {k: dv(v) for k, v in I.items() if k not in ("x", "w", "b")}
        D["x"] = [dv(x) for x in I["x"]]
        _dev[g.name] = {"pk": pk, "I": D, "ref": None}
    return _dev[g.name]


def dev_ref(ops, g):
    st = dev_state(ops, g)
    if st["ref"] is None:
        st["ref"] = {n: r.cuda() for n, r in base(g)["ref"].items()}
    return st["ref"]


def sliced_sources(ops, g, xs):
    """The sources as channel slices of one wider buffer per format: 8 channels of NaN / 1e30 before, between and after them
    (the batch stride is then the wide buffer's)."""
    B, _, H, W = xs[0].shape
    tot = sum(x.shape[1] for x in xs) + 8 * (len(xs) + 1)
    out, c = [], 8
    if g.s16:
        wide = torch.full((B, tot // 8, 2, H, W, 4), NAN16, dtype=torch.int32, device="cuda")
        for x in xs:
            n = x.shape[1]
            wide[:, c // 8:(c + n) // 8] = ops.S16.from_float(x).data
            out.append(ops.S16(wide, tot).channels(c, c + n))
            c += n + 8
        return out
    wide = torch.full((B, tot, H, W), NAN, dtype=torch.float32, device="cuda")
    wide[:, 1::2] = 1.0e30
    for x in xs:
        n = x.shape[1]
        wide[:, c:c + n] = x
        out.append(wide[:, c:c + n])
        c += n + 8
    return out


def launch(ops, g, J, sliced=False):
    """One launch of the row on the device inputs J -> ({name: fp32 tensor}, {name: decoded S16 copy}, intact), all on the device"""
    st = dev_state(ops, g)
    pk = st["pk"]
    B = g.shape[0]
    ACT = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "sigmoid": ops.ACT_SIGMOID, "tanh": ops.ACT_TANH}[act_name(g)]
    EPI = {"store": ops.EPI_STORE, "res_relu": ops.EPI_RES_RELU, "accum": ops.EPI_ACCUM, "gru_zr": ops.EPI_GRU_ZR, "gru_q": ops.EPI_GRU_Q}[g.epi]
    out, out16 = {}, {}
    with ops.conv_mode(g.mode), ops.ksplit_scope(not g.nokws):
        xs = J["x"]
        if sliced:
            xs = sliced_sources(ops, g, xs)
        elif g.s16:
            xs = [ops.S16.from_float(x) for x in xs]
        big, dst = C.framed(B, g.n_out, g.OH, g.OW)
        kw = dict(out=dst, act=ACT, epi=EPI)
        for n in ("e0", "e1", "pre"):
            if J.get(n) is not None and (n != "pre" or g.pre):
                kw[n] = J[n]
        if g.e0_s16:
            kw["e0"] = ops.S16.from_float(J["e0"])
        big2 = big16 = None
        if g.epi == "gru_zr":
            big2, kw["out2"] = C.framed(B, g.n_out, g.OH, g.OW)
        if g.out16:
            big16 = ops.S16.empty(B, g.n_out + 16, g.OH, g.OW, dst.device)
            big16.data.fill_(C.SENT16)
            kw["out16"] = big16.channels(8, 8 + g.n_out)
        if g.kind == "multi":
            ops.conv2d_multi(pk, xs, lay=g.lay, **kw)
        else:
            if g.norm:
                kw["in_norm"] = J["in_norm"]
            if g.stats:
                kw["want_stats"] = True
            r = ops.conv2d(pk, xs[0], xs[1] if len(xs) > 1 else None, **kw)
            assert r is not None, "the planned route normalises on load"
        intact = C.frame_intact(big, g.n_out)
        if g.epi == "gru_zr":
            out["z"], out["rh"] = dst, kw["out2"]
            intact = intact and C.frame_intact(big2, g.n_out)
        else:
            out["h" if g.epi == "gru_q" else "out"] = dst
        if g.out16:
            out16["rh" if g.epi == "gru_zr" else "h" if g.epi == "gru_q" else "out"] = kw["out16"].to_float()
            O = (g.n_out + 7) // 8
            intact = intact and bool((big16.data[:, :1] == C.SENT16).all()) and bool((big16.data[:, 1 + O:] == C.SENT16).all())
    return out, out16, intact


def dev_modified(ops, g, mods):
    st = dev_state(ops, g)
    return modified(st["I"], mods)


def check_flag(ops, g, label, trips):
    got = ops.guard_tripped()
    assert got == trips, "%s, %s: the guard %s" % (g, label, "stayed quiet" if trips else "tripped")
    assert not ops.guard_tripped(), "%s, %s: the flag was not reset by the read" % (g, label)


def check_plan(g, trace):
    assert len(trace) == 1, trace
    C.assert_plan(g, *trace[0])
    del trace[:]


def compare_clear(ops, g, label, mods, out, out16, worst, placed=False):
    """Every element against float64: the frame's reference with the reached pixels replaced by the case's."""
    J, pix, ref, e32, es = case_model(g, mods)
    gate = case_gate(g, e32, es, placed)
    bb, oy, ox = (torch.tensor(v).cuda() for v in zip(*pix))
    for n, r0 in dev_ref(ops, g).items():
        r = r0.clone()
        r[bb, :, oy, ox] = ref[n].cuda()
        atol, rtol, a32, as_ = gate[n]
        tol = atol + rtol * r.abs()
        assert bool(torch.isfinite(out[n]).all()), (g, label, n)
        ratio = float(((out[n].double() - r).abs() / tol).max())
        worst[n] = max(worst.get(n, 0.0), ratio)
        print("%s, %s [%s]: gate %.3e = row + %g x (E32 %.3e + E_split %.3e)%s, err / gate %.3f"
              % (g, label, n, atol, MARGIN, a32, as_, " + %.2e |ref|" % rtol if rtol else "", ratio))
        assert ratio <= 1.0, (g, label, n, ratio)
        if n in out16:
            r16 = float(((out16[n].double() - r).abs() / (tol + S16_REL * r.abs() + S16_ABS)).max())
            worst[n + " S16"] = max(worst.get(n + " S16", 0.0), r16)
            assert r16 <= 1.0, (g, label, n, "S16 copy", r16)


@gpu
@pytest.mark.parametrize("g", IN_ROWS, ids=repr)
def test_input_side(ops, trace, g):
    ops.guard_tripped()
    worst = {}
    for label, mods, trips, compare in in_cases(g):
        out, out16, intact = launch(ops, g, dev_modified(ops, g, mods))
        check_flag(ops, g, label, trips)
        check_plan(g, trace)
        assert intact, (g, label, "something outside the destination's channels changed")
        if compare:
            compare_clear(ops, g, label, mods, out, out16, worst)
    print("WORST %s: %s" % (g, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@gpu
@pytest.mark.parametrize("g", BF_ROWS, ids=repr)
def test_bf16_rows_quiet(ops, trace, g):
    ops.guard_tripped()
    b, c, iy, ix = in_positions(g)["first"]
    for v in (TRIP, 1.0e4, NAN):
        out, out16, intact = launch(ops, g, dev_modified(ops, g, [x_mod(g, b, c, iy, ix, v)]))
        check_flag(ops, g, repr(v), False)
        check_plan(g, trace)
        assert intact


@gpu
@pytest.mark.parametrize("g", OUT_ROWS, ids=repr)
def test_output_side(ops, trace, g):
    ops.guard_tripped()
    worst = {}
    for label, mods, trips, probed in out_cases(g):
        out, out16, intact = launch(ops, g, dev_modified(ops, g, mods))
        check_flag(ops, g, label, trips)
        check_plan(g, trace)
        assert intact, (g, label, "something outside the destinations' channels changed")
        if not trips:
            compare_clear(ops, g, label, mods, out, out16, worst, placed=True)
    print("WORST %s: %s" % (g, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@gpu
@pytest.mark.parametrize("g", SLICE_ROWS, ids=repr)
def test_no_stray_read(ops, trace, g):
    """Sources that are channel slices of a buffer full of NaN and 1e30: no unjustified trip, the same bits as from dense copies."""
    ops.guard_tripped()
    J = dev_state(ops, g)["I"]
    dense = launch(ops, g, J)
    check_flag(ops, g, "dense", False)
    check_plan(g, trace)
    sl = launch(ops, g, J, sliced=True)
    check_flag(ops, g, "sliced", False)
    check_plan(g, trace)
    assert dense[2] and sl[2]
    for a, b in zip(dense[:2], sl[:2]):
        assert sorted(a) == sorted(b)
        for n in a:
            assert bool(torch.isfinite(a[n]).all()) and torch.equal(a[n], b[n]), (g, n)


@gpu
def test_norm_refuses_s16(ops):
    g = [r for r in IN_ROWS if r.norm][0]
    st = dev_state(ops, g)
    o16 = ops.S16.empty(g.shape[0], g.n_out, g.OH, g.OW, "cuda")
    with ops.conv_mode("f16x3"), pytest.raises(RuntimeError, match="S16 tensors are for plain"):
        ops.conv2d(st["pk"], st["I"]["x"][0], in_norm=st["I"]["in_norm"], out16=o16)


S16_MAX = (65504.0 + 15.9921875) / 16.0        # the largest value an S16 tensor holds below the threshold: hi = 65504, lo < 16


@gpu
def test_gru_on_s16_state(ops, trace):
    """The packed-operand GRU epilogue (conv_epilogue_gru16): 128 + 128 S16 channels -> 256 (GRU_ZR) / 128 (GRU_Q), 1 x 5."""
    if not ops.conv_gru16_supported():
        pytest.fail("the packed-operand GRU epilogue is part of the default build")
    B, H, W = 2, 13, 37
    g_ = torch.Generator().manual_seed(9161)
    hid = 128
    h = torch.tanh(torch.randn(B, hid, H, W, generator=g_))
    x = torch.relu(torch.randn(B, hid, H, W, generator=g_))
    K = 2 * hid * 5
    probes = [(0, 0, 0, 0), (B - 1, hid - 1, H - 1, W - 1)]
    assert S16_MAX < CLEAR and not tripping(S16_MAX)
    for b, c, y, xx in probes:
        h[b, c, y, xx] = S16_MAX
    h16 = ops.S16.from_float(h.cuda())
    assert torch.equal(h16.to_float().cpu(), C.s16_value(h)) and float(h16.to_float()[0, 0, 0, 0]) == S16_MAX
    x16 = ops.S16.from_float(C.s16_value(x).cuda())
    with ops.conv_mode("f16x3"):
        for epi, cout, pad, k in (("zr", 2 * hid, (0, 2), (1, 5)), ("q", hid, (0, 2), (1, 5))):
            w = torch.randn(cout, 2 * hid, *k, generator=g_) * (2.0 / K) ** 0.5
            bias = torch.randn(cout, generator=g_) * 0.1
            pk = ops.PackedConv(w.cuda(), bias.cuda(), padding=pad, C0=hid)
            for what in ("quiet", "nan", "inf", "z row nan"):
                if what == "z row nan" and epi == "q":
                    continue
                pre = torch.randn(B, cout, H, W, generator=torch.Generator().manual_seed(5)) * 0.2
                for b, c, y, xx in probes:
                    row = (hid + c) if epi == "zr" else c          # the r row / q row of the probed state channel
                    if what == "quiet":
                        pre[b, row, y, xx] = 1.0e6 if epi == "zr" else 0.0      # r = 1: r * h = h
                    elif what == "z row nan":
                        pre[b, c, y, xx] = NAN
                    else:
                        pre[b, row, y, xx] = NAN if what == "nan" else INF
                z = torch.rand(B, hid, H, W, generator=torch.Generator().manual_seed(6))
                for b, c, y, xx in probes:
                    z[b, c, y, xx] = 0.0                                          # z = 0: the new state is the old one
                o16 = ops.S16.empty(B, hid + 16, H, W, "cuda")
                o16.data.fill_(C.SENT16)
                dst16 = o16.channels(8, 8 + hid)
                ops.guard_tripped()
                if epi == "zr":
                    zout = torch.full((B, hid, H, W), C.SENT, device="cuda")
                    ops.conv2d(pk, h16, in1=x16, out=zout, act=ops.ACT_SIGMOID, epi=ops.EPI_GRU_ZR, e0=h16, out16=dst16,
                               fp32_out=False, pre=ops.to_p32(pre.cuda()))
                else:
                    ops.conv2d(pk, h16, in1=x16, out=None, act=ops.ACT_TANH, epi=ops.EPI_GRU_Q, e0=h16, e1=ops.to_p32(z.cuda()),
                               out16=dst16, fp32_out=False, pre=ops.to_p32(pre.cuda()))
                # sigmoid(inf) = tanh(inf) = 1: r * h and the blend stay in range, so only NaN is out of range; a z row is
                # a gate, stored as fp32 and not split
                label = "%s %s" % (epi, what)
                assert ops.guard_tripped() == (what == "nan"), label
                assert not ops.guard_tripped()
                rc, p = trace[-1]
                assert rc == 0 and p["family"] == C.DIRECT and p["loop"] == C.TAP5 and p["Z"] == 1, p
                del trace[:]
                assert bool((o16.data[:, :1] == C.SENT16).all()) and bool((o16.data[:, 17:] == C.SENT16).all())
                if what == "quiet":
                    got16 = dst16.to_float().cpu()
                    for b, c, y, xx in probes:
                        assert float(got16[b, c, y, xx]) == S16_MAX, (label, float(got16[b, c, y, xx]))


# ------------------------------------------------------------------------------------------------
# B. the other reporters

import test_corr_routes as CR  # noqa: E402
from oracle import accflow_oracle as O  # noqa: E402

LOOKUP_SHAPE = "Sb"             # (1, 9, 11): P = 99, the second wave holds 35 pixels; levels 9 x 11, 4 x 5, 2 x 2, 1 x 1
# (level, pixel, integer level coordinate (ux, uy), tap (i, j)): the tap reads cell (ux - 4 + i, uy - 4 + j) with weight 1
LOOKUP_PROBES = [(0, 0, (3, 2), (8, 8)),        # tap n = j 9 + i = 80: the one flushed alone
                 (0, 98, (4, 4), (0, 0)),       # the last pixel, the first tap
                 (1, 98, (2, 1), (4, 4)),
                 (2, 50, (0, 0), (4, 4)),
                 (3, 98, (0, 0), (4, 4)),
                 (3, 0, (-4, -4), (8, 8))]      # the lone tap again, at the 1 x 1 level: cell (0, 0)


def grid_coords(B, H8, W8):
    ys, xs = torch.meshgrid(torch.arange(H8, dtype=torch.float32), torch.arange(W8, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys])[None].repeat(B, 1, 1, 1).contiguous()


def test_lookup_probes_are_what_they_say():
    B, H8, W8 = LK.SHAPES[LOOKUP_SHAPE]
    assert (H8 * W8) % 64 and B == 1
    for l, p, (ux, uy), (i, j) in LOOKUP_PROBES:
        cx, cy = ux - 4 + i, uy - 4 + j
        assert 0 <= cx < (W8 >> l) and 0 <= cy < (H8 >> l) and 0 <= p < H8 * W8
    assert {pr[0] for pr in LOOKUP_PROBES} == {0, 1, 2, 3} and any(pr[3] == (8, 8) for pr in LOOKUP_PROBES)
    assert any(pr[1] == H8 * W8 - 1 for pr in LOOKUP_PROBES)


def lookup_case(probe, v):
    """-> (pyramid, coords) of LOOKUP_SHAPE with cell value v under the probe"""
    B, H8, W8 = LK.SHAPES[LOOKUP_SHAPE]
    l, p, (ux, uy), (i, j) = probe
    pyr = [t.clone() for t in LK.make_pyramid(LOOKUP_SHAPE, "unit")]
    coords = grid_coords(B, H8, W8)
    coords.view(B, 2, -1)[0, 0, p], coords.view(B, 2, -1)[0, 1, p] = float(ux << l) if ux >= 0 else -float((-ux) << l), \
        float(uy << l) if uy >= 0 else -float((-uy) << l)
    pyr[l][p, 0, uy - 4 + j, ux - 4 + i] = v
    return pyr, coords


def decode88(o16):
    hi, lo = LK.s16_halves(o16)
    return LK.ref_order((hi.double() + lo.double()) / 16.0)


@gpu
@pytest.mark.parametrize("probe", LOOKUP_PROBES, ids=lambda p: "l%d-p%d-tap%d" % (p[0], p[1], p[3][1] * 9 + p[3][0]))
def test_lookup_s16(ops, probe):
    B, H8, W8 = LK.SHAPES[LOOKUP_SHAPE]
    l, p, (ux, uy), (i, j) = probe
    vals = [CLEAR, TRIP] + ([-CLEAR, -TRIP, NAN, INF] if probe is LOOKUP_PROBES[0] else [])
    ops.guard_tripped()
    for v in vals:
        pyr, coords = lookup_case(probe, v)
        dp = ops.DispPyramid.from_rowmajor([LK.dev(t) for t in pyr], B, H8, W8)
        wide, o16 = LK.sentinel_dest16(ops, B, 4 * LK.S16_LEVEL_CHANNELS, H8, W8)
        ops.corr_lookup_s16(dp, LK.dev(coords), o16)
        assert ops.guard_tripped() == tripping(v), (probe, v)
        assert not ops.guard_tripped()
        LK.assert_sentinels16("lookup %r" % (probe,), wide)
        if not tripping(v):
            ref, m, _ = LK.lookup(pyr, coords, 4)
            assert float(ref[0, l * 81 + i * 9 + j].view(-1)[p]) == v             # read with weight 1
            LK.within("guard L4 %r %r" % (probe, v), decode88(o16), ref, LK.gate_of(m) + LK.s16_term(ref))
    # a TRIP cell no tap reads (outside the 10 x 10 window), and one that only zero-weight taps read (its last column)
    if l == 0 and probe is LOOKUP_PROBES[0]:
        for cell in ((8, 10), (3, ux - 4 + 9)):
            pyr, coords = lookup_case(probe, 1.0)
            pyr[0][p, 0, cell[0], cell[1]] = TRIP
            dp = ops.DispPyramid.from_rowmajor([LK.dev(t) for t in pyr], B, H8, W8)
            wide, o16 = LK.sentinel_dest16(ops, B, 4 * LK.S16_LEVEL_CHANNELS, H8, W8)
            ops.corr_lookup_s16(dp, LK.dev(coords), o16)
            assert not ops.guard_tripped(), ("unread cell", cell)
            ref, m, _ = LK.lookup(pyr, coords, 4)
            assert float(ref.abs().max()) < 10
            LK.within("guard L4 unread %r" % (cell,), decode88(o16), ref, LK.gate_of(m) + LK.s16_term(ref))


ALT_C = 64              # 1 / sqrt(C) = 1 / 8 exactly
ALT_CH = 5


def alt_case(probe, v):
    """Frames (2, ALT_C, 9, 11): channel ALT_CH is zero but for q = 1 at the probed pixel (whose other channels are zero) and
    k = 8 v over the level-0 pixels of the probed cell: the tap is 1 x 8 v / 8 = v exactly, every other element is unmoved."""
    B, H8, W8 = LK.SHAPES[LOOKUP_SHAPE]
    l, p, (ux, uy), (i, j) = probe
    fr = torch.randn(2, ALT_C, H8, W8, generator=torch.Generator().manual_seed(4711))
    fr[:, ALT_CH] = 0.0
    base_fr = fr.clone()
    fr[0, :, p // W8, p % W8] = 0.0
    base_fr[0, :, p // W8, p % W8] = 0.0
    fr[0, ALT_CH, p // W8, p % W8] = 1.0
    cx, cy = ux - 4 + i, uy - 4 + j
    fr[1, ALT_CH, cy << l:(cy + 1) << l, cx << l:(cx + 1) << l] = 8.0 * v
    _, coords = lookup_case(probe, 0.0)
    return fr, base_fr, coords


def alt_ref64(fr, coords):
    return O.corr_lookup(O.corr_pyramid(fr[0:1].double(), fr[1:2].double()), coords.double())


@gpu
@pytest.mark.parametrize("probe", LOOKUP_PROBES, ids=lambda p: "l%d-p%d-tap%d" % (p[0], p[1], p[3][1] * 9 + p[3][0]))
def test_lookup_alt_s16(ops, probe):
    B, H8, W8 = LK.SHAPES[LOOKUP_SHAPE]
    l, p, (ux, uy), (i, j) = probe
    vals = [CLEAR, TRIP] + ([-TRIP, NAN] if probe is LOOKUP_PROBES[0] else [])
    ops.guard_tripped()
    for v in vals:
        fr, base_fr, coords = alt_case(probe, v)
        pairs = ops.AltPairs(ops.corr_alt_pyramid(fr.cuda()), [0], [1])
        wide, o16 = LK.sentinel_dest16(ops, B, 4 * LK.S16_LEVEL_CHANNELS, H8, W8)
        ops.corr_lookup_alt_s16(pairs, coords.cuda(), o16)
        assert ops.guard_tripped() == tripping(v), (probe, v)
        assert not ops.guard_tripped()
        LK.assert_sentinels16("alt lookup %r" % (probe,), wide)
        if not tripping(v):
            ref = alt_ref64(fr, coords)
            assert float(ref[0, l * 81 + i * 9 + j].view(-1)[p]) == v
            rms = float(alt_ref64(base_fr, coords).pow(2).mean().sqrt())           # tests/test_alt_corr.py: 1e-4 of the RMS
            LK.within("guard alt %r %r" % (probe, v), decode88(o16), ref, 1e-4 * rms + LK.s16_term(ref))
    if probe is LOOKUP_PROBES[0]:           # k = 8 TRIP where no tap of the probed pixel reaches: quiet
        fr, _, coords = alt_case(probe, 1.0)
        fr[1, ALT_CH, 8, 10] = 8.0 * TRIP
        pairs = ops.AltPairs(ops.corr_alt_pyramid(fr.cuda()), [0], [1])
        wide, o16 = LK.sentinel_dest16(ops, B, 4 * LK.S16_LEVEL_CHANNELS, H8, W8)
        ops.corr_lookup_alt_s16(pairs, coords.cuda(), o16)
        assert not ops.guard_tripped()


AGG_D, AGG_N = 128, 2
AGG_SHAPES = [(7, 9), (10, 13)]         # P = 63 and 130 (tests/test_gma_routes.py): one and two 128-pixel blocks, ragged both


def agg_probes(h, w):
    P = h * w
    return [(0, 0, 0), (AGG_N - 1, AGG_D - 1, P - 1), (AGG_N - 1, 0, P - 1), (0, AGG_D - 1, 0)]       # (item, channel, pixel)


def agg_operands(h, w, item, ch, pix, v):
    g = torch.Generator().manual_seed(977 + h * w)
    qk = torch.randn(1, 2 * AGG_D, h, w, generator=g)
    val = torch.randn(AGG_N, AGG_D, h, w, generator=g)
    fmap = torch.randn(AGG_N, AGG_D, h, w, generator=g)
    fmap.view(AGG_N, AGG_D, -1)[item, ch, pix] = v
    return qk, val, fmap


def run_agg(ops, kind, qk, val, fmap):
    """gamma = 0 -> (out fp32, decoded S16 copy, both framed by sentinels)"""
    h, w = fmap.shape[2:]
    n, D = AGG_N, AGG_D
    gam = torch.zeros(1, device="cuda")
    fm = fmap.cuda()
    big = torch.full((n, D + 16, h, w), C.SENT, device="cuda")
    s16 = ops.S16(torch.full((n, D // 8 + 2, 2, h, w, 4), C.SENT16, dtype=torch.int32, device="cuda"), D + 16)
    o16 = s16.channels(8, 8 + D)
    args = (fm.data_ptr(), fm.stride(0), gam, big[0, 8:].data_ptr(), big.stride(0), o16.ptr(), s16.bs, n, D, h, w)
    with ops.conv_mode("f16x3"):
        if kind == "s16":
            a16 = ops.gma_attention_s16(qk.cuda(), D, D ** -0.5)
            ops.guard_tripped()
            ops.gma_aggregate_s16(a16.ptr(), val.cuda(), *args)
        else:
            handle = ops.gma_attention_alt(qk.cuda(), D, D ** -0.5)
            ops.guard_tripped()
            ops.gma_aggregate_alt(handle, 0, val.cuda(), *args)
    torch.cuda.synchronize()
    assert bool((big[:, :8] == C.SENT).all()) and bool((big[:, 8 + D:] == C.SENT).all())
    assert bool((s16.data[:, 0] == C.SENT16).all()) and bool((s16.data[:, -1] == C.SENT16).all())
    return big[:, 8:8 + D].cpu(), o16.to_float().cpu()


@gpu
@pytest.mark.parametrize("kind", ["s16", "alt"])
@pytest.mark.parametrize("hw", AGG_SHAPES, ids=lambda s: "%dx%d" % s)
def test_aggregate_guard(ops, kind, hw):
    h, w = hw
    for item, ch, pix in agg_probes(h, w):
        for v in (CLEAR, TRIP) + ((-TRIP, NAN) if (item, ch, pix) == (0, 0, 0) else ()):
            qk, val, fmap = agg_operands(h, w, item, ch, pix, v)
            out, out16 = run_agg(ops, kind, qk, val, fmap)
            assert ops.guard_tripped() == tripping(v), (kind, hw, item, ch, pix, v)
            assert not ops.guard_tripped()
            if not tripping(v):
                assert torch.equal(out, fmap), "gamma = 0 returns fmap"
                err = (out16.double() - fmap.double()).abs()
                assert bool((err <= S16_REL * fmap.double().abs() + S16_ABS).all()), (kind, hw, item, ch, pix)
                assert float(out16.view(AGG_N, AGG_D, -1)[item, ch, pix]) == 4095.0    # CLEAR * 16 = 65504 + 16 after lo's rounding


PACK_C, PACK_HW = 64, (8, 10)            # P = 80 of 128 padded pixel columns, W8 even: the register-only GEMM and its packs
Q_THRESH = 4095.0 * math.sqrt(PACK_C)    # fmap1 is packed times 16 / sqrt(C) = 2 (corr_volume.hip: cscale * fs): 32760
ATT_SCALE = 0.25
K_THRESH = 4095.0 / ATT_SCALE            # k is packed times scale * 16 = 4 (gma.hip: scale * fs): 16380


def below(x):
    return float(torch.nextafter(torch.tensor(x, dtype=torch.float32), torch.tensor(0.0, dtype=torch.float32)))


def pack_probes(C_, P):
    return [(0, 0), (C_ - 1, P - 1)]       # (channel, pixel)


def test_pack_thresholds_are_the_sources():
    """cscale = 1.0f / sqrtf(C) and fs = 2^ACCFLOW_F16_ASHIFT as csrc/corr_volume.hip and csrc/gma.hip / gma_alt.hip apply them"""
    src = lambda n: open(os.path.join(C.CSRC, n)).read()  # noqa: E731
    cv = src("corr_volume.hip")
    assert "accflow_pack_kmajor(fmap1 + (long long)b * C * P, P, C, Kpad, CoutPad, wsplit, cscale * fs, f16 ? 1 : 0, guard, st);" in cv
    assert "accflow_pack_kmajor(fmap2 + (long long)b * C * P, P, C, Kpad, CoutPad, bsplit, fs, f16 ? 1 : 0, guard, st);" in cv
    assert "const float cscale = 1.0f / sqrtf((float)C);" in cv and "const float fs = f16 ? ldexpf(1.0f, ACCFLOW_F16_ASHIFT) : 1.0f;" in cv
    assert "rc = accflow_corr_level0_bf16s(fmap1, fmap2, lvl0, ws, B, C, H8, W8, mode, 0, nullptr, st, nullptr, nullptr);" in cv   # corr_volume: no guard
    for f in ("gma.hip", "gma_alt.hip"):
        t = src(f)
        assert "accflow_pack_kmajor(q + (long long)D * P, P, D, Kpad, Ppad, kp, scale * fs, 1, guard, st);" in t
        assert "accflow_pack_kmajor(q, P, D, Kpad, Ppad, qp, fs, 1, guard, st);" in t
    cs = float(CR.cscale32(PACK_C)) * 16.0
    assert cs == 2.0 and not (Q_THRESH * cs < LIMIT) and below(Q_THRESH) * cs < LIMIT
    assert not (K_THRESH * ATT_SCALE * 16.0 < LIMIT) and below(K_THRESH) * ATT_SCALE * 16.0 < LIMIT


@gpu
@pytest.mark.parametrize("entry", ["disp", "packed", "volume"])
def test_kmajor_packs_corr(ops, entry):
    h, w = PACK_HW
    P = h * w
    for operand, thr in ((0, Q_THRESH if entry == "disp" else TRIP), (1, TRIP)):
        for c, px in pack_probes(PACK_C, P):
            for v in (below(thr), thr, -thr, NAN):
                maps = CR.make_maps("unit", 2, PACK_C, h, w).clone()
                maps.view(2, PACK_C, P)[operand, c, px] = v
                f1, f2 = maps[0:1].contiguous(), maps[1:2].contiguous()
                ops.guard_tripped()
                with ops.conv_mode("f16x3"):
                    if entry == "volume":       # runs bf16x6 in this mode and reports nowhere
                        lv = ops.corr_volume(f1.cuda(), f2.cuda())
                        assert not ops.guard_tripped()
                        assert bool(torch.isfinite(lv[0]).all()) == (v == v)
                        continue
                    if entry == "disp":
                        dp = ops.corr_volume_disp(f1.cuda(), f2.cuda())
                    else:
                        dp = ops.corr_volume_disp_packed(ops.corr_pack(maps.cuda()), [0], [1])
                trips = not (abs(v) < thr)
                assert ops.guard_tripped() == trips, (entry, operand, c, px, v)
                assert not ops.guard_tripped()
                if not trips:
                    route = CR.corr_route(entry, "f16x3", PACK_C, h, w)
                    ref = CR.pyramid(CR.level0_ref64(f1, f2))
                    e32 = CR.errs(CR.pyramid(CR.level0_f32(f1, f2)), ref)
                    es = CR.errs(CR.pyramid(CR.level0_design(route[1], route[2], f1, f2)), ref)
                    got = [t.view(1, P, *t.shape[2:]).cpu() for t in dp.to_rowmajor()]
                    for l in range(4):
                        e = float((got[l].double() - ref[l]).abs().max())
                        gate = CR.MARGIN * (e32[l] + es[l])
                        print("guard corr %s operand %d (%d, %d) level %d: err / gate %.3f" % (entry, operand, c, px, l, e / gate))
                        assert e <= gate, (entry, operand, c, px, l, e / gate)


@gpu
@pytest.mark.parametrize("entry", ["s16", "alt"])
def test_kmajor_packs_attention(ops, entry):
    D, (h, w) = 128, (3, 5)
    P = h * w
    for operand, thr in ((0, TRIP), (1, K_THRESH)):          # q = qk[:, :D], k = qk[:, D:]
        for c, px in pack_probes(D, P):
            for v in (below(thr), thr, -thr, NAN):
                qk = R.make_qk("mid", 1, D, h, w).clone()
                qk.view(1, 2, D, P)[0, operand, c, px] = v
                ops.guard_tripped()
                with ops.conv_mode("f16x3"):
                    if entry == "s16":
                        a16 = ops.gma_attention_s16(qk.cuda(), D, ATT_SCALE)
                    else:
                        handle = ops.gma_attention_alt(qk.cuda(), D, ATT_SCALE)
                trips = not (abs(v) < thr)
                assert ops.guard_tripped() == trips, (entry, operand, c, px, v)
                assert not ops.guard_tripped()
                if trips:
                    continue
                ref = R.softmax64(qk, D, ATT_SCALE)
                e32 = float((R.softmax32(qk, D, ATT_SCALE).double() - ref).abs().max())
                es = float((R.att_emulations("A4", qk, D, ATT_SCALE)["design"] - ref).abs().max())
                gate = R.MARGIN * (e32 + es) + S16_REL * ref + S16_ABS
                if entry == "s16":
                    R.within("guard attention_s16 %d (%d, %d)" % (operand, c, px), a16.to_float().view(1, P, P).transpose(1, 2), ref, gate)
                else:       # the handle keeps no matrix: identity values through the aggregation give it back, row by row
                    eye = torch.zeros(1, D, h, w)
                    eye.view(1, D, P)[0, :P, :] = torch.eye(P)
                    zero = torch.zeros(1, D, h, w, device="cuda")
                    out = torch.empty(1, D, h, w, device="cuda")
                    ops.gma_aggregate_alt(handle, 0, eye.cuda(), zero.data_ptr(), zero.stride(0), torch.ones(1, device="cuda"),
                                          out.data_ptr(), out.stride(0), None, 0, 1, D, h, w)
                    assert not ops.guard_tripped()
                    R.within("guard attention_alt %d (%d, %d)" % (operand, c, px), out.view(1, D, P)[:, :P].transpose(1, 2), ref, gate)


@gpu
def test_pos_attention_quiet(ops):
    """gma_attention_pos_* take no guard (their content scores are bf16x6): 1e4 in q, the thread's flag stays 0, the result is finite."""
    D, (h, w), M = 128, (3, 5), 8
    g = torch.Generator().manual_seed(31)
    qk = R.make_qk("mid", 1, D, h, w).clone()
    qk[0, 3, 1, 2] = 1.0e4
    rh, rw = torch.randn(2 * M - 1, D, generator=g) * 0.1, torch.randn(2 * M - 1, D, generator=g) * 0.1
    ops.guard_tripped()
    with ops.conv_mode("f16x3"):
        tab = ops.gma_pos_tables(qk.cuda(), rh.cuda(), rw.cuda(), D, D ** -0.5)
        for content in (True, False):
            a16 = ops.gma_attention_pos_s16(qk.cuda(), tab, D, D ** -0.5, content)
            at = ops.gma_attention_pos_t(qk.cuda(), tab, D, D ** -0.5, content)
            assert not ops.guard_tripped()
            assert bool(torch.isfinite(a16.to_float()).all()) and bool(torch.isfinite(at).all())


# ------------------------------------------------------------------------------------------------
# C. completeness

MINE = "tests/test_guard_routes.py::"
SITES = {   # file -> [(a line of the site's kernel or function that names it, the tests that make it trip)], in file order
    "conv2d_bf16s_kernel.h": [("if constexpr (F16) s16_split8(xr, terms[0], terms[1], bad);", MINE + "test_input_side[in im2col ...]")],
    "conv2d_direct_kernel.h": [("va = fmaxf(va, 0.0f) * S16_SCALE;", "tests/test_hip_parity.py (the tap GEMM's intermediate)"),
                               ("auto store_patch = [&](int stage, int cc) {", MINE + "test_input_side[in direct / norm / tail / gru ...]")],
    "conv_common.h": [("void conv_epilogue_impl(", MINE + "test_output_side[out16 direct ..., out16 gru_* / accum / res_relu in the kernel]"),
                      ("void conv_epilogue_lean(", MINE + "test_output_side[out S16 tap9 ..., out16 stem ..., out16 multi lay * tap9]"),
                      ("void conv_epilogue_gru16(", MINE + "test_gru_on_s16_state")],
    "conv_ksplit.hip": [("void conv_ksplit_reduce_s16_kernel(", MINE + "test_output_side[out16 gru_zr ... split-K], [out16 store 144->76 3x3 split-K]"),
                        ("void conv_ksplit_reduce_s16q_kernel(", MINE + "test_output_side[out16 store / accum / res_relu / gru_q ... split-K]")],
    "conv_pack.hip": [("void conv_pack_kmajor_kernel(", MINE + "test_kmajor_packs_corr, test_kmajor_packs_attention")],
    "conv_s16m_kernel.h": [("void conv_epilogue_lean_res(", MINE + "test_output_side[out16 multi lay * res_relu]")],
    "conv_stem.hip": [("bad0 |= s16_bad(a);", MINE + "test_input_side[in stem 3->64 7x7 s2]")],
    "corr_alt.hip": [("void corr_lookup_alt_kernel(", MINE + "test_lookup_alt_s16")],
    "corr_disp.hip": [("void corr_lookup_disp_kernel(", MINE + "test_lookup_s16")],
    "corr_lookup_conv.hip": [("if (!(mx < S16_LIMIT_BITS) && a.guard) atomicOr(a.guard, 1);", "tests/test_lookup_fused.py, tests/test_lookup_routes.py (the fused lookup into convc1)")],
    "gma_alt.hip": [("void gma_alt_epilogue_kernel(", MINE + "test_aggregate_guard[alt]")],
    "misc.hip": [("atomicOr(guard, 1)", "tests/test_sampling_ops.py, tests/test_instance_norm.py (to_s16, the instance_norm forms, blend, get_occ)")] * 6,
    "sampling.hip": [("atomicOr(guard, 1)", "tests/test_sampling_ops.py (flow_from_coords_s16, the deform columns)")] * 2,
}


def test_sites_complete():
    """Every atomicOr( of csrc/ is a reporting site of this table, file by file and in order; a new one fails here until it has a
    case.  (gma_aggregate_s16 reports through conv_epilogue_impl / the reduce kernels with the channel-block scatter:
    test_aggregate_guard[s16].)"""
    found = {}
    for f in sorted(os.listdir(C.CSRC)):
        text = open(os.path.join(C.CSRC, f)).read()
        n = len(re.findall(r"atomicOr\(", text))
        if n:
            found[f] = (n, text)
    assert sorted(found) == sorted(SITES), sorted(found)
    total = 0
    for f, rows in SITES.items():
        n, text = found[f]
        assert n == len(rows), (f, n, len(rows))
        pos = 0
        for marker, tests in rows:
            assert tests
            at = text.find(marker, pos)
            assert at >= 0, (f, marker)
            nxt = text.find("atomicOr(", at)
            assert nxt >= 0, (f, marker)
            pos = nxt + 1 if marker.startswith("atomicOr(") else at + 1
        total += n
    assert total == 23
    mine = open(__file__).read()
    for name in ("test_input_side", "test_output_side", "test_gru_on_s16_state", "test_kmajor_packs_corr", "test_kmajor_packs_attention",
                 "test_lookup_alt_s16", "test_lookup_s16", "test_aggregate_guard"):
        assert "def %s(" % name in mine


S16_FUNCTIONS = ("s16_bad", "s16_bad2", "s16_split2", "s16_split1", "s16_split8", "s16_join")


def test_format_in_one_place():
    """csrc/s16_format.h is the only file that knows the S16 arithmetic: no other file of csrc/ names the range limit (as a
    number or as its bit pattern), converts to a 2-wide fp16 vector or casts a float to fp16, and the header defines each of its
    functions once.  (pack_terms.h casts to fp16 too: the WEIGHT split - another rounding path, documented there - is not this
    format; it is the one exemption, and for the casts only.)"""
    half2 = set()
    texts = {}
    for f in sorted(os.listdir(C.CSRC)):
        texts[f] = open(os.path.join(C.CSRC, f)).read()
        half2 |= set(re.findall(r"typedef\s+_Float16\s+(\w+)\s+__attribute__\(\(ext_vector_type\(2\)\)\)", texts[f]))
    fmt = texts.pop("s16_format.h")
    assert len(texts) > 40 and half2
    for f, text in texts.items():
        assert "65520" not in text and "0x477ff000" not in text.lower(), f
        for target in re.findall(r"__builtin_convertvector\([^;]*?,\s*(\w+)\s*\)", text):
            assert target not in half2, (f, target)
        assert not re.search(r"typedef\s+_Float16\s+\w+\s+__attribute__\(\(ext_vector_type\(2\)\)\)", text), f
        if f != "pack_terms.h":
            assert "(_Float16)" not in text, f
    for name in S16_FUNCTIONS:
        defs = re.findall(r"^__device__ __forceinline__ \w+ %s\(" % name, fmt, flags=re.M)
        assert len(defs) == 1, (name, len(defs))
    assert fmt.count("65520.0f") == 1 and fmt.lower().count("0x477ff000") == 1
    assert fmt.count("__builtin_convertvector(") == 3 and fmt.count("s16_split2(a, b, h[j], l[j]);") == 1
