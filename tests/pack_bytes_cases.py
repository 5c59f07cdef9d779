"""The cases of tests/test_pack_bytes.py and tests/golden/make_pack_bytes_golden.py: every weight / operand pack of the kernel
library and the host routes built on them (correlation GEMM, GMA attention and aggregation), as SHA-256 digests of the bytes
they write.

run_case(name) -> {buffer label: sha256 hex}.  Inputs are seeded on the CPU.  Pack cases call the C entry points through
accflow_amd._lib with ZERO-FILLED output buffers sized by the library's own *_elems / *_bytes functions plus GUARD_BYTES, and
digest each buffer whole - the third fp16 term slot and the guard words included, so a stray or missing write shows.  Route
cases go through the accflow_amd.ops functions; while one runs, torch.empty / torch.empty_like hand out zeroed memory
(zero_filled), so the padding lanes those functions leave unwritten are deterministic and whole tensors can be digested.

Weights (weight()): rows scaled over logspace(-3, 1) as in test_backward.test_fused_pack_equals_the_single_purpose_packs, row
min(3, Cout - 1) all zero (row-scale exponent 0), row 0 with largest magnitude exactly 2^-3 (an frexpf boundary of the row
scale: 2^-3 = 0.5 * 2^-2).
"""
import contextlib
import ctypes
import hashlib

import torch

GUARD_BYTES = 64 * 4
MODES = {"bf16x3": 2, "bf16x6": 3, "f16x3": 4}      # ACCFLOW_CONV_* (include/accflow_hip.h)

# (Cout, Cin, KH, KW, C0, variant) of test_fused_pack_equals_the_single_purpose_packs
SHAPES = [(64, 40, 3, 3, None, False), (130, 24, 1, 1, None, False), (27, 128, 3, 3, None, False), (2, 256, 3, 3, None, False),
          (96, 3, 7, 7, None, False), (128, 384, 1, 5, 256, False), (128, 128, 3, 3, None, True), (40, 64, 3, 3, None, "scale")]
MULTI = ((16, 3, 128), 27, 1, 5)                    # the smallest three-source case of tests/test_s16m.py (CAT_CASES)
GRIDS = ((8, 8), (9, 10))
DQK = 128


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def zeros(nbytes):
    return torch.zeros(int(nbytes) + GUARD_BYTES, dtype=torch.uint8, device="cuda")


@contextlib.contextmanager
def zero_filled():
    """torch.empty / empty_like return zeros: what an ops function allocates and does not write is deterministic."""
    saved = torch.empty, torch.empty_like
    torch.empty, torch.empty_like = torch.zeros, torch.zeros_like
    try:
        yield
    finally:
        torch.empty, torch.empty_like = saved


def weight(Cout, Cin, KH, KW, seed=None):
    g = gen(Cout + Cin if seed is None else seed)
    w = torch.randn(Cout, Cin, KH, KW, generator=g) * torch.logspace(-3, 1, Cout).view(-1, 1, 1, 1)
    w[min(3, Cout - 1)] = 0.0
    w[0] = w[0].clamp(-0.0625, 0.0625)
    w[0, 0, 0, 0] = 0.125
    assert float(w[0].abs().max()) == 0.125 and float(w[min(3, Cout - 1)].abs().max()) == 0.0
    return w, g


def done(lib_rc, bufs):
    assert lib_rc == 0, lib_rc
    torch.cuda.synchronize()
    return {k: sha(v) for k, v in bufs.items()}


# ------------------------------------------------------------------------------------------------
# pack entry points

def shape_id(s):
    Cout, Cin, KH, KW, C0, variant = s
    return "%dx%dx%dx%d%s%s" % (Cout, Cin, KH, KW, "" if C0 is None else "_c0%d" % C0,
                                {False: "", True: "_tapmajor", "scale": "_scale"}[variant])


def pack_case(s, entry):
    from accflow_amd import _lib
    lib = _lib.load()
    Cout, Cin, KH, KW, C0, variant = s
    w, g = weight(Cout, Cin, KH, KW)
    sc = (torch.rand(Cout, generator=g) + 0.5).cuda() if variant == "scale" else None
    w = w.cuda()
    tap_major = variant is True
    tflip = entry == "all_tflip"
    if tflip:                                # logical weight (Cin, Cout, KH, KW)[o][c] = w[c][o] flipped
        Cout, Cin = Cin, Cout
    C0 = Cin if (C0 is None or tflip) else C0
    Kpad, CoutPad = lib.accflow_conv_kpad(Cin, KH, KW), lib.accflow_conv_coutpad(Cout)
    npatch = lib.accflow_conv_patch_elems(Cout, Cin, KH, KW)
    args = (vp(w), vp(sc), Cout, Cin, KH, KW)
    if entry == "f32":
        b = {"wpack": zeros(Kpad * CoutPad * 4), "ktab": zeros(Kpad * 16)}
        return done(lib.accflow_conv_pack_f32(*args, C0, int(tap_major), vp(b["wpack"]), vp(b["ktab"]), stream()), b)
    if entry == "bf16s":
        b = {"wsplit": zeros(3 * Kpad * CoutPad * 2)}
        return done(lib.accflow_conv_pack_bf16s(*args, vp(b["wsplit"]), stream()), b)
    if entry == "patch":
        b = {"wpatch": zeros(npatch * 2)}
        return done(lib.accflow_conv_pack_patch(*args, vp(b["wpatch"]), stream()), b)
    if entry == "patch16":
        b = {"wpatch16": zeros(npatch * 2), "wscale16": zeros(CoutPad * 4)}
        return done(lib.accflow_conv_pack_patch16(*args, vp(b["wpatch16"]), vp(b["wscale16"]), stream()), b)
    if entry == "split16":
        b = {"wsplit16": zeros(3 * Kpad * CoutPad * 2), "wscale16": zeros(CoutPad * 4)}
        return done(lib.accflow_conv_pack_split16(*args, vp(b["wsplit16"]), vp(b["wscale16"]), stream()), b)
    # the fused entry point with the packs ops.PackedConv asks for (stride 1)
    has_split = not tap_major and Cout > 4
    has_patch, has_split16 = has_split and Cin >= 16, has_split and Cout > 32
    b = {"wpack": zeros(Kpad * CoutPad * 4), "ktab": zeros(Kpad * 16)}
    if has_split:
        b["wsplit"] = zeros(3 * Kpad * CoutPad * 2)
    if has_patch:
        b["wpatch"], b["wpatch16"] = zeros(npatch * 2), zeros(npatch * 2)
    if has_split16:
        b["wsplit16"] = zeros(3 * Kpad * CoutPad * 2)
    if has_patch or has_split16:
        b["wscale16"] = zeros(CoutPad * 4)
    return done(lib.accflow_conv_pack_all_f32(*args, C0, int(tap_major), int(tflip), vp(b["wpack"]), vp(b["ktab"]), vp(b.get("wsplit")),
                                              vp(b.get("wpatch")), vp(b.get("wpatch16")), vp(b.get("wscale16")), vp(b.get("wsplit16")),
                                              stream()), b)


def multi16_case():
    from accflow_amd import _lib
    lib = _lib.load()
    cs, Cout, KH, KW = MULTI
    n = len(cs)
    ws = [weight(Cout, c, KH, KW, seed=100 + i)[0].cuda() for i, c in enumerate(cs)]
    arr = lambda v: (ctypes.c_int * n)(*v)  # noqa: E731
    C, kh, kw = arr(cs), arr([KH] * n), arr([KW] * n)
    b = {"wpatch16": zeros(lib.accflow_conv_multi_pack_elems(Cout, n, C, kh, kw) * 2),
         "wscale16": zeros(lib.accflow_conv_coutpad(Cout) * 4)}
    wp = (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws])
    return done(lib.accflow_conv_pack_multi16(wp, None, Cout, n, C, kh, kw, vp(b["wpatch16"]), vp(b["wscale16"]), stream()), b)


def fmaps(F, C, H, W, seed):
    return torch.randn(F, C, H, W, generator=gen(seed))


def corr_pack_case(mode, C, H, W, huge=False):
    from accflow_amd import _lib
    lib = _lib.load()
    F = 2
    x = fmaps(F, C, H, W, 7 * C + H)
    if huge:
        x[1, 3, 2, 5] = 1.0e5                # * 2^4 is outside fp16: the range guard reports it
    x = x.cuda()
    b = {"packs": zeros(F * lib.accflow_corr_pack_bytes(C, H, W)), "guard": torch.zeros(1, dtype=torch.int32, device="cuda")}
    return done(lib.accflow_corr_pack_f32(vp(x), vp(b["packs"]), MODES[mode], vp(b["guard"]), F, C, H, W, stream()), b)


# ------------------------------------------------------------------------------------------------
# host routes, through accflow_amd.ops

def levels(pyr):
    return {"lvl%d" % i: t for i, t in enumerate(pyr)}


def corr_volume_case(mode, H, W):
    from accflow_amd import ops
    f = fmaps(4, 32, H, W, 31).cuda()
    with zero_filled():
        lv = ops.corr_volume(f[:2], f[2:], mode=MODES[mode])
    return done(0, levels(lv))


def corr_disp_case(mode, H, W):
    from accflow_amd import ops
    f = fmaps(4, 32, H, W, 32).cuda()
    ops.guard_tripped()
    with zero_filled():
        pyr = ops.corr_volume_disp(f[:2], f[2:], mode=MODES[mode])
    out = done(0, levels(pyr.levels))
    assert not ops.guard_tripped()
    return out


def corr_packed_case(mode, H, W):
    from accflow_amd import ops
    f = fmaps(3, 32, H, W, 33).cuda()
    ops.guard_tripped()
    with zero_filled():
        packs = ops.corr_pack(f, mode=MODES[mode])
        pyr = ops.corr_volume_disp_packed(packs, [0, 2, 1], [1, 0, 1])
    out = done(0, dict(levels(pyr.levels), packs=packs.data))
    assert not ops.guard_tripped()
    return out


def gma_inputs(B, n, H, W):
    g = gen(1000 * B + 10 * H + W)
    qk = torch.randn(B, 2 * DQK, H, W, generator=g) * 1.5
    v = torch.randn(n, DQK, H, W, generator=g)
    v[0, 5] *= 2.0 ** -9
    v[0, 7] = 0.0
    fmap = torch.randn(n, DQK, H, W, generator=g)
    return qk.cuda(), v.cuda(), fmap.cuda(), torch.tensor([0.37]).cuda()


def gma_t_case(mode, B, H, W):
    from accflow_amd import ops
    qk, v, fmap, gamma = gma_inputs(B, B, H, W)
    ops.guard_tripped()
    with zero_filled(), ops.conv_mode(mode):
        at = ops.gma_attention_t(qk, DQK, DQK ** -0.5)
        out = ops.gma_aggregate_t(at, v, fmap, gamma)
    d = done(0, {"attnT": at, "out": out})
    assert not ops.guard_tripped()
    return d


def gma_shared_case(kind, H, W):
    """n = 2 items on one attention: the stored S16 route (kind "s16") or alternate_attention ("alt")."""
    from accflow_amd import ops
    n = 2
    qk, v, fmap, gamma = gma_inputs(1, n, H, W)
    ops.guard_tripped()
    out = torch.zeros(n, DQK, H, W, device="cuda")
    out16 = ops.S16.empty(n, DQK, H, W, "cuda", zero=True)
    ptrs = (fmap.data_ptr(), fmap.stride(0), gamma, out.data_ptr(), out.stride(0), out16.ptr(), out16.bs, n, DQK, H, W)
    with zero_filled():
        if kind == "s16":
            a16 = ops.gma_attention_s16(qk, DQK, DQK ** -0.5)
            ops.gma_aggregate_s16(a16.ptr(), v, *ptrs)
            kept = {"attn16": a16.data}
        else:
            h = ops.gma_attention_alt(qk, DQK, DQK ** -0.5)
            ops.gma_aggregate_alt(h, 0, v, *ptrs)
            kept = {"packs": h.packs, "stats": h.stats}
    d = done(0, dict(kept, out=out, out16=out16.data))
    assert not ops.guard_tripped()
    return d


def _cases():
    c = {}
    for s in SHAPES:
        Cout, Cin, _, _, _, variant = s
        for entry in ("f32", "bf16s", "patch", "patch16", "split16", "all"):
            c["pack %s %s" % (entry, shape_id(s))] = (pack_case, s, entry)
        if variant is False and Cin > 4:     # (not tap_major and sc is None and Cin > 4)
            c["pack all_tflip %s" % shape_id(s)] = (pack_case, s, "all_tflip")
    c["pack multi16 %s" % "+".join(map(str, MULTI[0]))] = (multi16_case,)
    for mode in ("bf16x3", "bf16x6", "f16x3"):
        for C in (32, 256):
            for H, W in GRIDS:
                c["corr_pack %s C%d %dx%d" % (mode, C, H, W)] = (corr_pack_case, mode, C, H, W)
    c["corr_pack f16x3 C32 8x8 out-of-range"] = (corr_pack_case, "f16x3", 32, 8, 8, True)
    c["corr_volume bf16x6 8x8"] = (corr_volume_case, "bf16x6", 8, 8)
    for mode in ("f16x3", "bf16x6"):
        for H, W in ((8, 16), (9, 10)):
            c["corr_volume_disp %s %dx%d" % (mode, H, W)] = (corr_disp_case, mode, H, W)
            c["corr_volume_disp_packed %s %dx%d" % (mode, H, W)] = (corr_packed_case, mode, H, W)
    for mode in ("f16x3", "bf16x6"):
        for B, (H, W) in ((1, GRIDS[0]), (2, GRIDS[0]), (2, GRIDS[1])):
            c["gma_t %s B%d %dx%d" % (mode, B, H, W)] = (gma_t_case, mode, B, H, W)
    for kind in ("s16", "alt"):
        for H, W in GRIDS:
            c["gma_%s n2 %dx%d" % (kind, H, W)] = (gma_shared_case, kind, H, W)
    return c


CASES = _cases()


def run_case(name):
    fn, *args = CASES[name]
    return fn(*args)
