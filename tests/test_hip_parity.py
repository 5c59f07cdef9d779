"""GPU parity: every HIP entry point (through the C-ABI) against the CPU oracle on the same seeded
inputs, then the composed estimators / accumulation module against the oracle and the golden fixtures
produced by the reference.  Tolerances are written next to each check; floating point throughout, the
north-star gate is 1e-3 px mean EPE on flows."""
import pytest
import torch

from oracle import accflow_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def dev(t):
    return t.cuda()


def maxerr(a, b):
    return float((a.detach().cpu() - b.detach().cpu()).abs().max())


def check(a, b, atol, rtol=1e-4, what=""):
    a, b = a.detach().cpu(), b.detach().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    assert bool((err <= tol).all()), "%s: max err %.3e, tol %.1e+%.0e*|ref|" % (what, float(err.max()), atol, rtol)


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------
# convolution


CONV_CASES = [
    # Cin, Cout, KH, KW, stride, padH, padW, B, H, W
    (3, 64, 7, 7, 2, 3, 3, 2, 40, 56),       # encoder stem
    (64, 64, 3, 3, 1, 1, 1, 2, 20, 28),
    (64, 96, 3, 3, 2, 1, 1, 1, 20, 28),      # strided, 96 channels (-> 64 ch x 64 px tiles at this size)
    (64, 96, 1, 1, 2, 0, 0, 1, 20, 28),      # downsample 1x1 s2
    (324, 256, 1, 1, 1, 0, 0, 1, 16, 32),    # convc1
    (256, 192, 3, 3, 1, 1, 1, 1, 16, 32),
    (2, 128, 7, 7, 1, 3, 3, 1, 16, 32),      # convf1 (K = 98, padded to 112)
    (256, 126, 3, 3, 1, 1, 1, 1, 16, 32),    # Cout not a multiple of 32
    (384, 128, 1, 5, 1, 0, 2, 1, 16, 32),    # GRU horizontal
    (384, 128, 5, 1, 1, 2, 0, 1, 16, 32),    # GRU vertical
    (256, 2, 3, 3, 1, 1, 1, 1, 16, 32),      # flow head conv2
    (256, 576, 1, 1, 1, 0, 0, 1, 16, 32),    # mask head
    (257, 256, 3, 3, 1, 1, 1, 1, 16, 32),    # AccPlus conv1 (odd Cin)
    (128, 27, 3, 3, 1, 1, 1, 1, 16, 32),     # ZeroConv
    (128, 1, 3, 3, 1, 1, 1, 3, 17, 23),      # blending mask, ragged sizes
    (128, 256, 3, 3, 1, 1, 1, 11, 60, 128),  # large pixel count -> 128x128 tiles
    (128, 256, 3, 3, 1, 1, 1, 2, 60, 128),   # -> 128 ch x 64 px tiles
    (128, 27, 3, 3, 1, 1, 1, 16, 60, 128),   # -> 32 ch x 256 px tiles
    (64, 64, 3, 3, 1, 1, 1, 4, 120, 128),    # -> 64 ch x 128 px tiles
    (64, 96, 3, 3, 2, 1, 1, 2, 240, 512),    # -> 96 ch x 128 px tiles
    (256, 4, 3, 3, 1, 1, 1, 2, 16, 32),      # small-Cout direct kernel, 4 channels
    (96, 3, 1, 5, 1, 0, 2, 1, 9, 11),        # small-Cout patch kernel, 3 channels, ragged
    (8, 2, 3, 3, 1, 1, 1, 1, 10, 12),        # small-Cout gather kernel (fewer than 16 input channels)
    (40, 2, 3, 3, 2, 1, 1, 1, 10, 12),       # small-Cout gather kernel (strided)
    (256, 2, 3, 3, 1, 1, 1, 3, 60, 128),     # flow head conv2 at working size
    (64, 64, 3, 3, 1, 1, 1, 7, 240, 512),    # encoder layer at working size
    (96, 48, 5, 1, 1, 2, 0, 16, 122, 250),   # large grid, ragged sizes, 48 channels
]


from test_conv_routes import trace  # noqa: E402,F401  (fixture: the plan of every accflow_conv2d_f32 call)

# the CONV_CASES entries whose comments name a tile or a small-Cout kernel: (family, wc, wp, tc, tp) of the plan (conv_plan.h;
# family 6 = fp32 MFMA, 1 = small-Cout patch kernel, 0 = small-Cout gather kernel)
CONV_TILES = {
    (64, 96, 3, 3, 2, 1, 1, 1, 20, 28): (6, 2, 2, 1, 1),
    (128, 256, 3, 3, 1, 1, 1, 11, 60, 128): (6, 2, 2, 2, 2),
    (128, 256, 3, 3, 1, 1, 1, 2, 60, 128): (6, 2, 2, 2, 1),
    (128, 27, 3, 3, 1, 1, 1, 16, 60, 128): (6, 1, 4, 1, 2),
    (64, 64, 3, 3, 1, 1, 1, 4, 120, 128): (6, 2, 2, 1, 2),
    (64, 96, 3, 3, 2, 1, 1, 2, 240, 512): (6, 1, 4, 3, 1),
    (96, 3, 1, 5, 1, 0, 2, 1, 9, 11): (1, 0, 0, 0, 0),
    (8, 2, 3, 3, 1, 1, 1, 1, 10, 12): (0, 0, 0, 0, 0),
    (40, 2, 3, 3, 2, 1, 1, 1, 10, 12): (0, 0, 0, 0, 0),
}
assert all(c in CONV_CASES for c in CONV_TILES)


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d(ops, case, trace):
    import torch.nn.functional as F
    Cin, Cout, KH, KW, st, pH, pW, B, H, W = case
    g = gen(hash(case) & 0xFFFF)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, KH, KW, generator=g) * (2.0 / (Cin * KH * KW)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    ref = F.conv2d(x, w, b, stride=st, padding=(pH, pW))
    pk = ops.PackedConv(dev(w), dev(b), stride=st, padding=(pH, pW))
    out = ops.conv2d(pk, dev(x), mode=ops.CONV_F32)
    check(out, ref, 2e-5, what="conv %s" % (case,))
    check(ops.conv2d(pk, dev(x), act=ops.ACT_RELU, mode=ops.CONV_F32), torch.relu(ref), 2e-5, what="conv+relu")
    assert len(trace) == 2 and all(rc == 0 for rc, _ in trace)
    if case in CONV_TILES:
        for _, p in trace:
            assert (p["family"], p["wc"], p["wp"], p["tc"], p["tp"]) == CONV_TILES[case], (case, p)


@pytest.mark.parametrize("mode,atol", [("bf16x3", 2e-3), ("bf16x6", 3e-5), ("f16x3", 1e-4)])
@pytest.mark.parametrize("case", [c for c in CONV_CASES if c[1] > 32])
def test_conv2d_split_bf16(ops, case, mode, atol):
    """split-operand matrix-core paths: same convolution, operands split into 2 / 3 bf16 terms or fp16 hi + lo.
    Tolerances: 3 * 2^-16 (bf16x3) resp. ~2^-22 (bf16x6, f16x3) relative per product on O(1) outputs; the print below
    shows the measured errors (f16x3 ~2x bf16x6)."""
    import torch.nn.functional as F
    Cin, Cout, KH, KW, st, pH, pW, B, H, W = case
    g = gen(hash(case) & 0xFFFF)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, KH, KW, generator=g) * (2.0 / (Cin * KH * KW)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    ref = F.conv2d(x, w, b, stride=st, padding=(pH, pW))
    pk = ops.PackedConv(dev(w), dev(b), stride=st, padding=(pH, pW))
    m = {"bf16x3": ops.CONV_BF16X3, "bf16x6": ops.CONV_BF16X6, "f16x3": ops.CONV_F16X3}[mode]
    out = ops.conv2d(pk, dev(x), mode=m)
    check(out, ref, atol, rtol=0, what="conv %s %s" % (mode, case))
    err = (out.cpu() - ref).abs()
    print("split conv", mode, case, "max err %.2e mean %.2e" % (float(err.max()), float(err.mean())))


def test_conv2d_f16x3_range_guard(ops):
    """f16x3 (direct kernel, operands as fp16 hi + lo): fp32-class error inside fp16's range, the guard flag when an
    activation leaves it, and with_range_guard's bf16x6 recomputation."""
    import torch.nn.functional as F
    g = gen(41)
    x = torch.randn(2, 64, 24, 40, generator=g)
    w = torch.randn(96, 64, 3, 3, generator=g) * 0.06
    b = torch.randn(96, generator=g) * 0.1
    pk = ops.PackedConv(dev(w), dev(b), padding=1)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1).float()
    ops.guard_tripped()
    got = ops.conv2d(pk, dev(x), mode=ops.CONV_F16X3)
    assert pk.wpatch16 is not None and pk.wscale16 is not None
    check(got, ref, 2e-5, rtol=0, what="f16x3 in range")
    assert not ops.guard_tripped()
    big = x.clone()
    big[1, 3, 5, 7] = 5000.0  # * 2^ACCFLOW_F16_ASHIFT = 80000 > 65504: not representable in the scaled split
    ops.conv2d(pk, dev(big), mode=ops.CONV_F16X3)
    assert ops.guard_tripped() and not ops.guard_tripped()  # reported once, then reset
    ok = x.clone()
    ok[1, 3, 5, 7] = 4000.0   # still inside
    check(ops.conv2d(pk, dev(ok), mode=ops.CONV_F16X3), F.conv2d(ok.double(), w.double(), b.double(), padding=1).float(),
          1e-4, rtol=1e-6, what="f16x3 near the top of the range")
    assert not ops.guard_tripped()
    with ops.conv_mode("f16x3"):
        out = ops.with_range_guard(lambda: ops.conv2d(pk, dev(big)))
        assert ops.current_mode() == ops.CONV_F16X3 and not ops.guard_tripped()
    check(out, F.conv2d(big, w, b, padding=1), 2e-3, rtol=1e-5, what="guarded recomputation in bf16x6")


@pytest.mark.parametrize("wmag,xmag", [(1.0, 1.0), (2.0 ** -6, 1.0), (1.0, 2.0 ** -8), (2.0 ** -6, 2.0 ** -8), (2.0 ** -12, 2.0 ** -8),
                                       (2.0 ** 8, 2.0 ** 4)])
def test_conv2d_f16x3_error_model(ops, wmag, xmag):
    """The fp16 hi + lo split with power-of-two row / activation scales: error RELATIVE to the output magnitude stays
    fp32-class whatever the magnitudes of weights and activations (released checkpoints have |w| ~ 1e-2 and
    ZeroConv-scaled branches far below; include/accflow_hip.h states the model).  Gate 5e-6 of the output RMS."""
    import torch.nn.functional as F
    g = gen(43)
    x = torch.randn(2, 128, 24, 40, generator=g) * xmag
    w = torch.randn(192, 128, 3, 3, generator=g) * (0.03 * wmag)
    w[5] *= 2.0 ** -9       # rows of very different magnitude get their own scale
    w[7, 3] *= 2.0 ** -14   # a tiny weight inside a normal row
    b = torch.randn(192, generator=g) * 0.1 * wmag * xmag
    pk = ops.PackedConv(dev(w), dev(b), padding=1)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ops.guard_tripped()
    for mode, gate in ((ops.CONV_F16X3, 5e-6), (ops.CONV_BF16X6, 5e-6)):
        got = ops.conv2d(pk, dev(x), mode=mode).cpu().double()
        rms = ref.pow(2).mean(dim=(0, 2, 3), keepdim=True).sqrt()          # per output channel
        rel = ((got - ref).abs() / rms).max()
        print("f16x3 error model: |w| x %.1e, |x| x %.1e, mode %d: max err / channel rms = %.2e" % (wmag, xmag, mode, float(rel)))
        assert float(rel) <= gate, (wmag, xmag, mode, float(rel))
    assert not ops.guard_tripped()


@pytest.mark.parametrize("cout,kh,kw", [(2, 3, 3), (1, 3, 3), (4, 1, 5), (3, 5, 1)])
def test_conv2d_small_cout_tap_sum(ops, cout, kh, kw):
    """<= 4 output channels at working size: all taps as one 1x1 matrix-core conv + accflow_tap_sum_f32 (bias,
    activation, in-place accumulate, two sources), against F.conv2d and against the dedicated small-Cout kernel."""
    import torch.nn.functional as F
    g = gen(100 + cout * 10 + kh)
    B, H, W = 2, 44, 96
    a, c = torch.randn(B, 128, H, W, generator=g), torch.randn(B, 64, H, W, generator=g)
    w = torch.randn(cout, 192, kh, kw, generator=g) * 0.04
    b = torch.randn(cout, generator=g)
    pk = ops.PackedConv(dev(w), dev(b), padding=(kh // 2, kw // 2), C0=128)
    assert pk.ztaps is not None
    ref = F.conv2d(torch.cat([a, c], 1), w, b, padding=(kh // 2, kw // 2))
    got = ops.conv2d(pk, dev(a), in1=dev(c), mode=ops.CONV_BF16X6)
    check(got, ref, 3e-5, what="tap-sum conv")
    check(got, ops.conv2d(pk, dev(a), in1=dev(c), mode=ops.CONV_F32), 3e-5, what="tap-sum vs small-Cout kernel")
    check(ops.conv2d(pk, dev(a), in1=dev(c), act=ops.ACT_SIGMOID), torch.sigmoid(ref), 2e-5, what="tap-sum + sigmoid (default mode)")
    acc0 = torch.randn(B, cout, H, W, generator=g)
    buf = dev(acc0).contiguous()
    ops.conv2d(pk, dev(a), in1=dev(c), out=buf, epi=ops.EPI_ACCUM, e0=buf)
    check(buf, acc0 + ref, 3e-5, what="tap-sum accumulate in place")


def test_conv2d_split_bf16_epilogues_and_sources(ops):
    import torch.nn.functional as F
    g = gen(7)
    B, H, W, hd = 2, 12, 40, 128
    h = torch.tanh(torch.randn(B, hd, H, W, generator=g))
    x = torch.randn(B, 256, H, W, generator=g)
    wq = torch.randn(hd, hd + 256, 5, 1, generator=g) * 0.02
    bq = torch.randn(hd, generator=g) * 0.1
    z = torch.rand(B, hd, H, W, generator=g)
    rh = torch.randn(B, hd, H, W, generator=g) * 0.3
    q = torch.tanh(F.conv2d(torch.cat([rh, x], 1), wq, bq, padding=(2, 0)))
    ref = (1 - z) * h + z * q
    pq = ops.PackedConv(dev(wq), dev(bq), padding=(2, 0), C0=hd)
    for mode, atol in ((ops.CONV_BF16X3, 1e-3), (ops.CONV_BF16X6, 2e-5)):
        hb = dev(h).contiguous()
        ops.conv2d(pq, dev(rh), in1=dev(x), out=hb, act=ops.ACT_TANH, epi=ops.EPI_GRU_Q, e0=hb, e1=dev(z), mode=mode)
        check(hb, ref, atol, rtol=0, what="split q conv mode %d" % mode)


def test_conv2d_two_sources_slices_and_scale(ops):
    import torch.nn.functional as F
    g = gen(5)
    B, H, W = 2, 12, 20
    a, c = torch.randn(B, 128, H, W, generator=g), torch.randn(B, 70, H, W, generator=g)
    w = torch.randn(40, 198, 3, 3, generator=g) * 0.03
    b = torch.randn(40, generator=g)
    sc = torch.rand(40, generator=g) + 0.5
    ref = F.conv2d(torch.cat([a, c], 1), w * sc[:, None, None, None], b, padding=1)
    pk = ops.PackedConv(dev(w), dev(b), stride=1, padding=1, scale=dev(sc), C0=128)
    big_in = torch.zeros(B, 300, H, W).cuda()
    big_in[:, 100:228] = dev(a)
    big_out = torch.zeros(B, 90, H, W).cuda()
    ops.conv2d(pk, big_in[:, 100:228], in1=dev(c), out=big_out[:, 10:50])
    check(big_out[:, 10:50], ref, 3e-5, what="two-source sliced conv")
    assert float(big_out[:, :10].abs().max()) == 0 and float(big_out[:, 50:].abs().max()) == 0


def test_conv2d_epilogues(ops):
    import torch.nn.functional as F
    g = gen(6)
    B, H, W, hd = 2, 10, 18, 128
    h = torch.tanh(torch.randn(B, hd, H, W, generator=g))
    x = torch.randn(B, 64, H, W, generator=g)
    wz, wr, wq = [torch.randn(hd, hd + 64, 1, 5, generator=g) * 0.05 for _ in range(3)]
    bz, br, bq = [torch.randn(hd, generator=g) * 0.1 for _ in range(3)]
    hx = torch.cat([h, x], 1)
    z = torch.sigmoid(F.conv2d(hx, wz, bz, padding=(0, 2)))
    r = torch.sigmoid(F.conv2d(hx, wr, br, padding=(0, 2)))
    q = torch.tanh(F.conv2d(torch.cat([r * h, x], 1), wq, bq, padding=(0, 2)))
    hn = (1 - z) * h + z * q
    HX = dev(hx).contiguous()
    zr = ops.PackedConv(dev(torch.cat([wz, wr])), dev(torch.cat([bz, br])), padding=(0, 2))
    Z = torch.empty(B, hd, H, W).cuda()
    RH = torch.empty(B, hd, H, W).cuda()
    ops.conv2d(zr, HX, out=Z, act=ops.ACT_SIGMOID, epi=ops.EPI_GRU_ZR, e0=HX[:, :hd], out2=RH)
    check(Z, z, 1e-5, what="z gate")
    check(RH, r * h, 1e-5, what="r*h")
    pq = ops.PackedConv(dev(wq), dev(bq), padding=(0, 2), C0=hd)
    ops.conv2d(pq, RH, in1=HX[:, hd:], out=HX[:, :hd], act=ops.ACT_TANH, epi=ops.EPI_GRU_Q, e0=HX[:, :hd], e1=Z)
    check(HX[:, :hd], hn, 2e-5, what="h update (in place)")
    # residual + relu, accumulate
    w3 = torch.randn(64, 64, 3, 3, generator=g) * 0.05
    res = torch.randn(B, 64, H, W, generator=g)
    p3 = ops.PackedConv(dev(w3), None, padding=1)
    ref = torch.relu(res + torch.relu(F.conv2d(x, w3, None, padding=1)))
    check(ops.conv2d(p3, dev(x), act=ops.ACT_RELU, epi=ops.EPI_RES_RELU, e0=dev(res)), ref, 2e-5, what="res relu")
    w2 = torch.randn(2, 64, 3, 3, generator=g) * 0.05
    co = torch.randn(B, 2, H, W, generator=g)
    p2 = ops.PackedConv(dev(w2), dev(torch.zeros(2)), padding=1)
    cod = dev(co).contiguous()
    ops.conv2d(p2, dev(x), out=cod, epi=ops.EPI_ACCUM, e0=cod)
    check(cod, co + F.conv2d(x, w2, None, padding=1), 2e-5, what="accumulate in place")


@pytest.mark.parametrize("case", [
    # Cin, Cout, KH, KW, stride, B, H, W        kernel family the dispatcher picks
    (96, 96, 3, 3, 1, 2, 24, 64),              # direct kernel, 128-channel form with 96 live rows (one slot per 4x32 tile)
    (128, 128, 3, 3, 1, 2, 13, 37),            # same, ragged tiles (masked pixels must not count)
    (64, 64, 3, 3, 1, 2, 24, 64),              # direct kernel, 64-channel form (two slots per tile)
    (64, 64, 3, 3, 1, 1, 9, 70),               # same, ragged
    (64, 128, 5, 1, 1, 2, 16, 64),             # direct kernel, 128 channels (4 x 1 wave layout)
    (3, 64, 7, 7, 2, 2, 64, 128),              # im2col kernel: encoder stem
    (64, 96, 3, 3, 2, 2, 32, 128),             # im2col kernel: strided 3x3
    (64, 96, 1, 1, 2, 2, 32, 128),             # im2col kernel: downsample 1x1
    (96, 128, 3, 3, 2, 7, 120, 256),           # im2col kernel at working size
    (64, 64, 3, 3, 1, 7, 240, 512),            # direct kernel at working size (1920 slots per plane)
])
def test_conv_epilogue_instance_norm_stats(ops, case):
    """InstanceNorm statistics gathered in the convolution epilogue (accflow_conv_desc.stats) + the single-pass
    normalisation against nn.InstanceNorm2d semantics (extractor.py:36-39: per plane, biased variance, eps 1e-5) and
    against the three-pass kernel, all three fused modes."""
    import torch.nn.functional as F
    Cin, Cout, KH, KW, st, B, H, W = case
    g = gen(77)
    x = torch.randn(B, Cin, H, W, generator=g) * 1.5 + 0.3
    w = torch.randn(Cout, Cin, KH, KW, generator=g) * (2.0 / (Cin * KH * KW)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.5          # a per-channel offset: mean^2 / var up to ~1
    pk = ops.PackedConv(dev(w), dev(b), stride=st, padding=(KH // 2, KW // 2))
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=st, padding=(KH // 2, KW // 2))
    mu = ref.mean(dim=(2, 3), keepdim=True)
    var = ref.var(dim=(2, 3), unbiased=False, keepdim=True)
    nrm = ((ref - mu) / torch.sqrt(var + 1e-5)).float()
    res = torch.randn(nrm.shape, generator=g)
    want = {0: nrm, 1: torch.relu(nrm), 2: torch.relu(res + torch.relu(nrm))}
    for mode in (ops.CONV_F16X3, ops.CONV_BF16X6):
        y, stt = ops.conv2d(pk, dev(x), want_stats=True, mode=mode)
        assert stt is not None, "this shape must take a statistics-gathering kernel"
        check(y, ref.float(), 3e-5, what="conv output %s" % (case,))
        n = stt.partial[..., 2].sum(dim=2).cpu()
        assert bool((n == ref.shape[2] * ref.shape[3]).all()), "every output pixel counted exactly once"
        for nm in (0, 1, 2):
            got = ops.instance_norm(y.clone(), nm, res=dev(res) if nm == 2 else None, stats=stt)
            check(got, want[nm], 3e-5, rtol=1e-5, what="single-pass instance norm mode %d %s" % (nm, case))
            old = ops.instance_norm(y.clone(), nm, res=dev(res) if nm == 2 else None)
            check(got, old, 1e-5, rtol=1e-5, what="vs three-pass kernel mode %d" % nm)
    # normalise-on-load: a following stride-1 convolution reads relu(norm(y)) straight from the raw y (direct kernel)
    if st == 1:
        w2 = torch.randn(Cout, Cout, 3, 3, generator=g) * (2.0 / (Cout * 9)) ** 0.5
        pk2 = ops.PackedConv(dev(w2), None, padding=1)
        ref2 = F.conv2d(torch.relu(nrm), w2, None, padding=1)
        for mode in (ops.CONV_F16X3, ops.CONV_BF16X6):
            y, stt = ops.conv2d(pk, dev(x), want_stats=True, mode=mode)
            mr = ops.instance_stats_finalize(stt)
            check(mr[..., 0], mu.float().reshape(B, Cout), 2e-5, rtol=1e-5, what="finalised mean")
            r = ops.conv2d(pk2, y, want_stats=True, in_norm=mr, mode=mode)
            assert r is not None, "a 3x3 stride-1 conv of <= 256 channels must normalise on load"
            check(r[0], ref2, 5e-5, rtol=1e-5, what="normalise-on-load conv %s" % (case,))
        # the exact fp32-MFMA mode has no normalise-on-load form: the caller is told (None) and normalises itself
        assert ops.conv2d(pk2, y, in_norm=mr, mode=ops.CONV_F32) is None
    # a conv with an activation cannot gather statistics; a route without support reports None
    with pytest.raises(RuntimeError):
        ops.conv2d(pk, dev(x), act=ops.ACT_RELU, want_stats=True)
    _, none = ops.conv2d(pk, dev(x), want_stats=True, mode=ops.CONV_F32)
    assert none is None


def test_deform_conv(ops):
    g = gen(8)
    B, C, H, W = 2, 128, 14, 22
    x = torch.randn(B, C, H, W, generator=g)
    off = torch.randn(B, 18, H, W, generator=g) * 2.5
    off[0, :, :2] *= 6  # push some samples far outside
    m = torch.rand(B, 9, H, W, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) * 0.04
    b = torch.randn(C, generator=g) * 0.1
    ref = O.deform_conv2d(x, off, m, w, b)
    pk = ops.PackedConv(dev(w), dev(b), stride=1, padding=1, tap_major=True)
    out = ops.conv2d(pk, dev(x), offset=dev(off), dmask=dev(m), mode=ops.CONV_F32)   # fused fp32-MFMA kernel
    check(out, ref, 3e-5, what="deformable conv (fused fp32 kernel)")
    for mode, tol in ((ops.CONV_BF16X6, 3e-5), (ops.CONV_F16X3, 1e-4)):           # columns + 1x1 matrix-core conv
        assert pk.zcols is not None
        out = ops.conv2d(pk, dev(x), offset=dev(off), dmask=dev(m), mode=mode)
        check(out, ref, tol, what="deformable conv (two-pass, mode %d)" % mode)
    # the view-sliced operands AccFlow passes (offset / mask are channel slices of one tensor)
    om = dev(torch.cat([off, m], 1)).contiguous()
    check(ops.conv2d(pk, dev(x), offset=om[:, :18], dmask=om[:, 18:]), ref, 1e-4, what="deformable conv, sliced operands")


def test_deform_conv_vs_independent_known_answers(ops, golden):
    """HIP deformable conv (every route) against float64 vectors computed independently of the oracle
    (tests/golden/make_deform_golden.py: scalar loops after torchvision's CPU kernel / expected_fn), with sample
    positions on every branch of the boundary rule."""
    g = golden("deform_conv_kat")
    for tag in "ab":
        a = {k: T(g[tag + "_" + k]) for k in ("x", "offset", "mask", "weight", "bias", "out")}
        pk = ops.PackedConv(dev(a["weight"]), dev(a["bias"]), stride=1, padding=1, tap_major=True)
        for mode, tol in ((ops.CONV_F32, 1e-5), (ops.CONV_BF16X6, 1e-5), (ops.CONV_F16X3, 2e-5), (ops.CONV_BF16X3, 2e-3)):
            out = ops.conv2d(pk, dev(a["x"]), offset=dev(a["offset"]), dmask=dev(a["mask"]), mode=mode)
            check(out, a["out"], tol, rtol=1e-5, what="deform conv vs independent vectors (%s, mode %d)" % (tag, mode))


# ------------------------------------------------------------------------------------------------
# correlation volume / lookup


@pytest.mark.parametrize("shape", [(2, 256, 16, 32), (1, 256, 17, 23), (1, 64, 9, 8)])
def test_corr_volume_pyramid(ops, shape):
    g = gen(10)
    f1, f2 = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    ref = O.corr_pyramid(f1, f2)
    for mode, tol in ((ops.CONV_F32, 2e-5), (ops.CONV_BF16X6, 3e-5), (ops.CONV_BF16X3, 2e-3)):
        got = ops.corr_volume(dev(f1), dev(f2), mode=mode)
        for l in range(4):
            assert tuple(got[l].shape) == tuple(ref[l].shape)
            check(got[l], ref[l], tol, rtol=0 if mode == ops.CONV_BF16X3 else 1e-4,
                  what="pyramid level %d %s mode %d" % (l, shape, mode))


@pytest.mark.parametrize("shape", [(2, 16, 32), (1, 17, 23), (3, 60, 128)])
def test_corr_lookup(ops, shape):
    B, h, w = shape
    g = gen(11)
    P = h * w
    pyr = [torch.randn(B * P, 1, h >> l, w >> l, generator=g) for l in range(4)]
    coords = O.coords_grid(B, h, w) + 5.0 * torch.randn(B, 2, h, w, generator=g)
    coords[0, :, 0, :4] = torch.tensor([[-30.0, -3.5, 1e5, float(w) + 2.25], [2.0, -9.0, 3.0, float(h) - 0.5]])
    coords[0, :, 1, :2] = torch.tensor([[4.0, float(w - 1)], [0.0, float(h - 1)]])  # exact integers / borders
    ref = O.corr_lookup(pyr, coords)
    got = ops.corr_lookup([dev(p) for p in pyr], dev(coords))
    check(got, ref, 2e-5, what="lookup %s" % (shape,))


@pytest.mark.parametrize("shape", [(2, 256, 16, 32), (1, 256, 17, 23), (1, 64, 9, 11), (1, 256, 15, 130),
                                   (2, 256, 60, 128)])
def test_corr_disp_volume_and_lookup(ops, shape):
    """the displacement-indexed hot-path layout: a pure permutation of the row-major pyramid (bit-exact, the same
    matrix-core main loop), pooled levels bit-exact, lookup equal to the oracle's"""
    g = gen(23)
    B, C, h, w = shape
    f1, f2 = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    ref = O.corr_pyramid(f1, f2)
    for mode, tol in ((ops.CONV_BF16X6, 3e-5), (ops.CONV_BF16X3, 2e-3), (ops.CONV_F16X3, 1e-4)):
        dp = ops.corr_volume_disp(dev(f1), dev(f2), mode=mode)
        rm = dp.to_rowmajor()
        base = ops.corr_volume(dev(f1), dev(f2), mode=mode)
        for l in range(4):
            assert tuple(dp.levels[l].shape) == (B, (h * w + 127) // 128, h >> l, w >> l, 128)
            if mode != ops.CONV_F16X3:  # (the row-major volume has no fp16 form: it runs bf16x6 in that mode)
                assert torch.equal(rm[l], base[l]), "displaced level %d is not a permutation of the row-major one" % l
            check(rm[l], ref[l], tol, rtol=0 if mode == ops.CONV_BF16X3 else 1e-4, what="disp pyramid level %d" % l)
        back = ops.DispPyramid.from_rowmajor(base, B, h, w)
        P = h * w
        for l in range(4):
            if mode != ops.CONV_F16X3:  # (padding lanes p >= P of the last 128-pixel block are never written nor read)
                assert torch.equal(back._unblocked(back.levels[l], h >> l, w >> l), dp._unblocked(dp.levels[l], h >> l, w >> l))
    # coherent flow (the layout's design case), noise, and out-of-range / integer / border coordinates
    smooth = torch.nn.functional.interpolate(3.0 * torch.randn(B, 2, 3, 4, generator=g), size=(h, w), mode="bilinear",
                                             align_corners=True)
    for k, flow in enumerate((smooth, 4.0 * torch.randn(B, 2, h, w, generator=g), torch.zeros(B, 2, h, w))):
        coords = O.coords_grid(B, h, w) + flow
        if k == 1:
            coords[0, :, 0, :4] = torch.tensor([[-30.0, -3.5, 1e5, float(w) + 2.25], [2.0, -9.0, 3.0, float(h) - 0.5]])
            coords[0, :, 1, :3] = torch.tensor([[4.0, float(w - 1), 0.0], [0.0, float(h - 1), -1.0]])
            coords[0, :, 2, :2] = torch.tensor([[-1e9, float("inf")], [1e9, 0.0]])
        want = O.corr_lookup(ref, torch.nan_to_num(coords, posinf=1e6, neginf=-1e6).clamp(-1e6, 1e6))
        dp = ops.corr_volume_disp(dev(f1), dev(f2), mode=ops.CONV_BF16X6)
        got = ops.corr_lookup(dp, dev(coords))
        check(got, want, 3e-5, what="disp lookup %s flow %d" % (shape, k))
        base = ops.corr_volume(dev(f1), dev(f2), mode=ops.CONV_BF16X6)
        assert torch.equal(got, ops.corr_lookup(base, dev(coords))), "disp vs row-major lookup kernel"


def test_corr_disp_pool_and_limits(ops):
    g = gen(29)
    B, h, w = 2, 19, 27
    P = h * w
    lvl0 = torch.randn(B * P, 1, h, w, generator=g)
    ref = [lvl0]
    for _ in range(3):
        ref.append(torch.nn.functional.avg_pool2d(ref[-1], 2, stride=2))
    d0 = ops.DispPyramid.from_rowmajor([dev(lvl0)], B, h, w).levels[0]
    dp = ops.corr_disp_pool(d0, h, w)
    rm = dp.to_rowmajor()
    for l in range(4):
        check(rm[l], ref[l], 1e-6, what="displaced pool level %d" % l)
    assert ops.corr_disp_supported(90, 160) and ops.corr_disp_supported(135, 240)  # no per-pair size limit any more
    with pytest.raises(RuntimeError):
        ops.corr_volume_disp(dev(torch.zeros(1, 8, 16, 16)), dev(torch.zeros(1, 8, 16, 16)), mode=ops.CONV_F32)


def test_corr_lookup_golden(ops, golden):
    g = golden("raft_c1")
    pyr = ops.corr_volume(dev(T(g["fmap1"])), dev(T(g["fmap2"])))
    sel = g["pyr_sel"]
    for l in range(4):
        check(pyr[l].cpu()[sel], T(g["pyr%d" % l]), 1e-4, what="golden pyramid %d" % l)
    check(ops.corr_lookup(pyr, dev(T(g["coords_r"]))), T(g["lookup_r"]), 1e-4, what="golden lookup")


# ------------------------------------------------------------------------------------------------
# sampling ops, norms, element-wise


def test_convex_upsample(ops):
    g = gen(12)
    flow = torch.randn(2, 2, 11, 19, generator=g) * 3
    mask = torch.randn(2, 576, 11, 19, generator=g) * 2
    check(ops.convex_upsample(dev(flow), dev(mask)), O.convex_upsample(flow, mask), 2e-5, what="convex upsample")


def test_backwarp_getocc_downflow(ops, golden):
    g = gen(13)
    img = torch.randn(2, 37, 20, 28, generator=g)
    img2 = torch.randn(2, 37, 20, 28, generator=g)
    flow = torch.randn(2, 2, 20, 28, generator=g) * 4
    flow[0, :, 0, :3] = torch.tensor([[-40.0, 0.0, 27.0], [0.0, -1.0, 19.0]])
    check(ops.backwarp(dev(img), dev(flow)), O.backwarp(img, flow), 1e-5, what="backwarp")
    check(ops.get_occ(dev(flow), dev(img), dev(img2), binary=False), O.get_occ(flow, img, img2, binary=False), 1e-5,
          what="emap")
    ob = ops.get_occ(dev(flow), dev(img), dev(img2), binary=True).cpu()
    ref = O.get_occ(flow, img, img2)
    err = O.get_occ_error(flow, img, img2)
    flips = ob != ref
    assert not bool(flips.any()) or bool(((err[flips] - 1.0).abs() < 1e-5).all())
    # mean abs error below / above the 1.0 threshold in different pixels: scale so that the threshold sits at the
    # median of the per-pixel error (37 channels of |N(0,1) - warp| average ~1.1 unscaled)
    s = 1.0 / float(err.median())
    ob = ops.get_occ(dev(flow), dev(img * s), dev(img2 * s), binary=True).cpu()
    ref = O.get_occ(flow, img * s, img2 * s)
    err = O.get_occ_error(flow, img * s, img2 * s)
    assert 0.2 < float(ref.mean()) < 0.8, "the mixed-threshold case must have both classes"
    flips = ob != ref
    assert not bool(flips.any()) or bool(((err[flips] - 1.0).abs() < 1e-5).all())
    h = golden("harness")
    check(ops.backwarp(dev(T(h["img"])), dev(T(h["fflow"]))), T(h["warped"]), 1e-5, what="golden backwarp")
    check(ops.downflow8(dev(T(h["big"]))), T(h["down"]), 1e-5, what="golden downflow8")
    # white noise at 480x1024: source coordinates near 1000 px carry ~6e-5 px of fp32 rounding and the field's
    # gradient is O(1)/px, so 1e-4 is the conditioning of the op itself; a smooth field pins the arithmetic
    big = torch.randn(1, 2, 480, 1024, generator=g)
    check(ops.downflow8(dev(big)), O.downflow8(big), 1e-4, what="downflow8 480x1024 (noise)")
    ys, xs = torch.meshgrid(torch.arange(480.0), torch.arange(1024.0), indexing="ij")
    smooth = torch.stack([3 * torch.sin(xs / 90) + ys / 200, 2 * torch.cos(ys / 70) - xs / 300])[None]
    check(ops.downflow8(dev(smooth)), O.downflow8(smooth), 2e-6, what="downflow8 480x1024 (smooth)")


def test_instance_norm_and_elementwise(ops):
    g = gen(14)
    x = torch.randn(3, 5, 24, 40, generator=g) * 3 + 1.5
    res = torch.randn(3, 5, 24, 40, generator=g)
    n = O._instance_norm(x)
    check(ops.instance_norm(dev(x).clone(), 0), n, 2e-5, what="IN")
    check(ops.instance_norm(dev(x).clone(), 1), torch.relu(n), 2e-5, what="IN+relu")
    check(ops.instance_norm(dev(x).clone(), 2, res=dev(res)), torch.relu(res + torch.relu(n)), 2e-5, what="IN+res")
    xo = torch.randn(1, 3, 7, 9, generator=g)  # HW not a multiple of 4
    check(ops.instance_norm(dev(xo).clone(), 0), O._instance_norm(xo), 2e-5, what="IN odd")
    c = torch.randn(2, 256, 6, 10, generator=g)
    buf = torch.zeros(2, 300, 6, 10).cuda()
    ops.split_tanh_relu(dev(c), buf[:, :128], buf[:, 128:256], 128, 128)
    check(buf[:, :128], torch.tanh(c[:, :128]), 1e-6, what="tanh split")
    check(buf[:, 128:256], torch.relu(c[:, 128:]), 0, what="relu split")
    fi = torch.randn(2, 2, 6, 10, generator=g)
    cg = ops.coords_grid(2, 6, 10, "cuda", flow_init=dev(fi))
    check(cg, O.coords_grid(2, 6, 10) + fi, 0, what="coords grid")
    d0 = torch.zeros(2, 2, 6, 10).cuda()
    ops.flow_from_coords(cg, dst0=d0, dst1=buf[:, 298:300])
    check(d0, fi, 1e-6, what="flow from coords")
    check(buf[:, 298:300], fi, 1e-6, what="flow from coords (slice)")
    f1, f2 = torch.randn(2, 8, 6, 10, generator=g), torch.randn(2, 8, 6, 10, generator=g)
    m = torch.rand(2, 1, 6, 10, generator=g)
    check(ops.blend(dev(f1), dev(f2), dev(m)), f1 * m + (1 - m) * f2, 1e-6, what="blend")
    check(ops.activation_(dev(f1)[:, 2:5], ops.ACT_SIGMOID), torch.sigmoid(f1[:, 2:5]), 1e-6, what="sigmoid slice")


def test_gma_attention_aggregate(ops):
    g = gen(15)
    B, D, h, w = 2, 128, 9, 14
    qk = torch.randn(B, 2 * D, h, w, generator=g)
    q, k = qk[:, :D].reshape(B, D, -1), qk[:, D:].reshape(B, D, -1)
    ref = torch.softmax(torch.matmul((D ** -0.5) * q.transpose(1, 2), k), -1)
    attn = ops.gma_attention(dev(qk), D, D ** -0.5)
    check(attn[:, 0], ref, 1e-6, rtol=1e-4, what="attention")
    v = torch.randn(B, D, h, w, generator=g)
    fmap = torch.randn(B, D, h, w, generator=g)
    gamma = torch.tensor([0.7])
    agg = torch.matmul(ref, v.reshape(B, D, -1).transpose(1, 2)).transpose(1, 2).reshape(B, D, h, w)
    out = ops.gma_aggregate(dev(ref[:, None].contiguous()), dev(v), dev(fmap), dev(gamma))
    check(out, fmap + 0.7 * agg, 2e-5, what="aggregate")
    # transposed hot-path variants (aggregation on the split-bf16 matrix cores)
    attn_t = ops.gma_attention_t(dev(qk), D, D ** -0.5)
    check(attn_t, ref.transpose(1, 2), 1e-6, rtol=1e-4, what="transposed attention")
    out_t = ops.gma_aggregate_t(attn_t, dev(v), dev(fmap), dev(gamma), mode=ops.CONV_BF16X6)
    check(out_t, fmap + 0.7 * agg, 3e-5, what="aggregate (bf16x6, transposed)")


def test_gma_shared_attention_runs(ops):
    """Pairs out of the same image1 share ONE attention matrix and go through one stacked aggregation GEMM
    (RAFTGMA._prepare_context): same numbers as one attention per item."""
    import argparse
    from accflow_amd.networks.gma.modules import Aggregate, Attention
    g = gen(151)
    args = argparse.Namespace(position_only=False, position_and_content=False, num_heads=1)
    att = Attention(args=args, dim=128, heads=1, max_pos_size=160, dim_head=128).cuda().eval()
    agg = Aggregate(args=args, dim=128, dim_head=128, heads=1).cuda().eval()
    with torch.no_grad():
        att.to_qk.weight.copy_(dev(torch.randn(256, 128, 1, 1, generator=g) * 0.1))
        agg.to_v.weight.copy_(dev(torch.randn(128, 128, 1, 1, generator=g) * 0.1))
        agg.gamma.fill_(0.6)
    for h, w in ((8, 16), (7, 9)):   # 128 pixels: the f16x3 GEMM; 63 pixels: ragged, bf16x6 per item
        ctx = torch.randn(3, 128, h, w, generator=g).relu()
        items = [0, 0, 1, 2, 2, 2, 0]          # a run of 2, a single, a run of 3, and a non-adjacent repeat
        inp = dev(ctx[items])
        motion = dev(torch.randn(len(items), 128, h, w, generator=g))
        for mode in (ops.CONV_F16X3, ops.CONV_BF16X6):
            with ops.conv_mode(mode):
                per_item = agg(att.forward_t(inp), motion)
                runs = [[0, 0, 2], [1, 2, 3], [2, 3, 6], [0, 6, 7]]
                shared = agg(att.forward_t(dev(ctx), runs=runs), motion)
            # (not bitwise: the stacked GEMM runs on another kernel / tile / split-K than the per-item batch)
            check(shared, per_item.cpu(), 2e-5, what=f"shared attention ({h}x{w}, mode {mode})")


# ------------------------------------------------------------------------------------------------
# composed modules


def _models(name):
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    m = build_flow_estimator(name)
    sd = make_state_dict(m)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval(), sd


def _pair(seed, H, W):
    from accflow_amd.data.synthetic import make_sequence, normalize
    fr = [normalize(f) for f in make_sequence(seed, 2, H, W)]
    return fr[1], fr[0]


def test_encoders_vs_golden(ops, golden):
    g = golden("raft_c1")
    m, sd = _models("raft")
    i1, i2 = _pair(int(g["seed"]), int(g["H"]), int(g["W"]))
    f1, f2 = m.fnet([dev(i1), dev(i2)])
    check(f1, T(g["fmap1"]), 3e-4, what="fnet fmap1 vs reference")
    check(f2, T(g["fmap2"]), 3e-4, what="fnet fmap2 vs reference")
    check(m.cnet(dev(i1)), T(g["cnet"]), 3e-4, what="cnet vs reference")


def test_update_block_vs_golden(ops, golden):
    g = golden("raft_c1")
    m, sd = _models("raft")
    cnet = T(g["cnet"])
    net, inp = torch.tanh(cnet[:, :128]), torch.relu(cnet[:, 128:])
    B, _, h, w = cnet.shape
    flow = T(g["coords_r"]) - O.coords_grid(B, h, w)
    net1, mask1, delta1 = m.update_block(dev(net), dev(inp), dev(T(g["lookup_r"])), dev(flow))
    check(net1, T(g["ub_net"]), 1e-4, what="update block net")
    check(mask1[:, ::9], T(g["ub_mask_s"]), 1e-4, what="update block mask")
    check(delta1, T(g["ub_delta"]), 1e-4, what="update block delta")
    check(m.upsample_flow(dev(flow + T(g["ub_delta"])), mask1), T(g["upsample"]), 3e-4, what="upsample_flow")


@pytest.mark.parametrize("name", ["raft", "gma"])
def test_estimator_c1_vs_golden_and_oracle(ops, golden, name):
    """C1: 128x256, iters 1/4/12 (+flow_init); gate: mean EPE <= 1e-3 px vs the reference's outputs; max EPE about 4x the
    largest measured on the MI355X (in the messages)."""
    g = golden(name + "_c1")
    m, sd = _models(name)
    i1, i2 = _pair(int(g["seed"]), int(g["H"]), int(g["W"]))
    gate, measured = {"raft": (2e-4, 4.35e-5), "gma": (2e-3, 4.39e-4)}[name]
    for it in (1, 4, 12):
        out = m(dev(i1), dev(i2), iters=it).cpu()
        ref = T(g["flow_it%d" % it])
        me, mx = O.epe(out if it == 12 else out[:, :, ::2, ::2], ref)
        assert me <= 1e-3 and mx <= gate, (name, it, me, mx, "measured max %.2e" % measured)
    out = m(dev(i1), dev(i2), iters=4, flow_init=dev(T(g["flow_init"]))).cpu()
    me, mx = O.epe(out[:, :, ::2, ::2], T(g["flow_it4_init"]))
    gate, measured = {"raft": (1e-4, 2.01e-5), "gma": (1e-3, 1.49e-4)}[name]
    assert me <= 1e-3 and mx <= gate, (name, "flow_init", me, mx, "measured max %.2e" % measured)
    # batch of 2 different pairs == two single calls (batching must not change results)
    j1, j2 = _pair(1001, int(g["H"]), int(g["W"]))
    both = m(dev(torch.cat([i1, j1])), dev(torch.cat([i2, j2])), iters=4).cpu()
    solo = m(dev(j1), dev(j2), iters=4).cpu()
    assert maxerr(both[1:], solo) <= 1e-4


def test_accflow_c1_vs_golden(ops, golden):
    from accflow_amd.data.synthetic import make_sequence, make_state_dict, normalize
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.AccFlow_ import AccFlow
    g = golden("accflow_c1")
    model = AccFlow(build_flow_estimator("acc|raft"))
    model.load_state_dict(make_state_dict(model), strict=True)
    model = model.cuda().eval()
    frames = [dev(normalize(f)) for f in make_sequence(int(g["seed"]), int(g["n_frames"]), int(g["H"]), int(g["W"]))]
    outs = model(images=frames, test_mode=False)
    assert len(outs) == int(g["n_frames"]) - 2
    for k, o in enumerate(outs):
        me, mx = O.epe(o.cpu(), T(g["out%d" % k]))
        assert me <= 1e-3 and mx <= 5e-4, ("accflow out", k, me, mx, "measured max 1.12e-4")
    # the step API of the reference (AccFlow.iter) gives the same first output
    small, up = model.iter(frames[2], frames[1], frames[0], None)
    check(small, T(g["s2_out_small"]), 2e-4, rtol=1e-3, what="iter out_small")
    me, mx = O.epe(up.cpu(), T(g["out0"]))
    assert me <= 1e-3, ("iter", me, mx)


def test_accplus_module_vs_golden(ops, golden):
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.AccFlow_ import AccFlow
    g = golden("accflow_c1")
    model = AccFlow(build_flow_estimator("acc|raft"))
    sd = make_state_dict(model)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    f_ini, f, c1, o = (T(g["s2_" + k]) for k in ("f_ini", "f", "c1", "o"))
    enc = model.flow_encoder([dev(T(g["s2_flow_ini"])), dev(T(g["s2_dflow"])), dev(T(g["s2_F2n"]))])
    check(enc[0], f_ini, 2e-4, rtol=1e-3, what="flow_encoder f_ini")
    check(enc[2], f, 2e-4, rtol=1e-3, what="flow_encoder f")
    f_acc = model.accplus(enc[1], enc[2], dev(o), dev(c1))
    check(f_acc, T(g["s2_f_acc"]), 3e-4, rtol=1e-3, what="accplus (incl. deformable conv)")


def test_product_refuses_cpu():
    from accflow_amd.networks import build_flow_estimator
    m = build_flow_estimator("raft").eval()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 128, 256), torch.zeros(1, 3, 128, 256))


# ------------------------------------------------------------------------------------------------
# evaluation harness (test_cvo.py:53-101) and full-size checks


def test_harness_vs_golden(ops, golden):
    from accflow_amd import eval_cvo
    g = golden("harness")
    occ_bw, occ_fw = eval_cvo.calc_occ_mask(dev(T(g["bflow"])), dev(T(g["fflow"])))
    assert float((occ_bw.cpu() != T(g["occ_bw"])).float().mean()) < 2e-3
    assert float((occ_fw.cpu() != T(g["occ_fw"])).float().mean()) < 2e-3
    e = eval_cvo.cal_epe(dev(T(g["pred"])), dev(T(g["bflow"])), dev(T(g["occ_bw"])))
    for got, key in zip(e, ("epe_all", "epe_occ", "epe_vis")):
        check(got, T(g[key]), 1e-5, what=key)


def test_raft_c2_480x1024_vs_reference(ops, golden):
    """BASELINE configs[1]: RAFT direct, one 480x1024 pair, 12 iters, against the reference's own output
    (every 8th pixel stored).  Gate: mean EPE <= 1e-3 px."""
    g = golden("raft_c2")
    m, sd = _models("raft")
    i1, i2 = _pair(int(g["seed"]), int(g["H"]), int(g["W"]))
    out = m(dev(i1), dev(i2), iters=12)
    me, mx = O.epe(out[:, :, ::8, ::8].cpu(), T(g["flow_it12_s8"]))
    assert me <= 1e-3 and mx <= 5e-4, (me, mx, "measured max 1.12e-4")
    assert bool(torch.isfinite(out).all())


def test_accflow_c3_7x480x1024_vs_reference(ops, golden):
    """BASELINE configs[2]: 7-frame 480x1024 AccFlow(RAFT); all 5 accumulated flows vs the reference."""
    from accflow_amd.data.synthetic import make_sequence, make_state_dict, normalize
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.AccFlow_ import AccFlow
    g = golden("accflow_c3")
    model = AccFlow(build_flow_estimator("acc|raft"))
    model.load_state_dict(make_state_dict(model), strict=True)
    model = model.cuda().eval()
    frames = [dev(normalize(f)) for f in make_sequence(int(g["seed"]), 7, 480, 1024)]
    outs = model(images=frames)
    assert len(outs) == 5
    for k, o in enumerate(outs):
        me, mx = O.epe(o[:, :, ::8, ::8].cpu(), T(g["out%d" % k]))
        assert me <= 1e-3 and mx <= 2e-3, (k, me, mx, "measured max 2.94e-4")
    # a batch of two sequences == each alone (sequence sharding relies on it)
    frames2 = [dev(normalize(f)) for f in make_sequence(1000, 7, 480, 1024, batch=2)]
    outs2 = model(images=frames2)
    # (tile shapes - hence summation order - depend on the grid size, so this is equality up to fp32 rounding
    # amplified by 12 GRU iterations, not bitwise)
    me, mx = O.epe(outs2[-1][:1].cpu(), outs[-1].cpu())
    assert me <= 1e-4 and mx <= 2e-3, (me, mx)


def test_full_size_properties(ops):
    """Size-independent properties at the full 60x128 / 480x1024 working sizes."""
    g = gen(21)
    B, h, w = 2, 60, 128
    # convex upsampling: a constant flow and any mask give 8x that constant in the interior (weights sum to 1)
    flow = torch.zeros(B, 2, h, w) + torch.tensor([1.25, -0.5]).view(1, 2, 1, 1)
    mask = torch.randn(B, 576, h, w, generator=g)
    up = ops.convex_upsample(dev(flow), dev(mask)).cpu()
    assert float((up[:, 0, 8:-8, 8:-8] - 10.0).abs().max()) < 1e-5 and float((up[:, 1, 8:-8, 8:-8] + 4.0).abs().max()) < 1e-5
    # backwarp by zero flow is the identity; by an integer shift it is a shift with zero fill
    img = torch.randn(1, 8, 480, 1024, generator=g)
    z = torch.zeros(1, 2, 480, 1024)
    assert maxerr(ops.backwarp(dev(img), dev(z)), img) == 0.0
    z[:, 0] = 3.0
    sh = ops.backwarp(dev(img), dev(z)).cpu()
    assert float((sh[..., :-3] - img[..., 3:]).abs().max()) == 0.0 and float(sh[..., -3:].abs().max()) == 0.0
    # lookup is linear in the volume; at integer coordinates it reads volume entries exactly
    P = h * w
    pa = [torch.randn(P, 1, h >> l, w >> l, generator=g) for l in range(4)]
    pb = [torch.randn(P, 1, h >> l, w >> l, generator=g) for l in range(4)]
    coords = O.coords_grid(1, h, w) + 3.0 * torch.randn(1, 2, h, w, generator=g)
    la = ops.corr_lookup([dev(t) for t in pa], dev(coords))
    lb = ops.corr_lookup([dev(t) for t in pb], dev(coords))
    lab = ops.corr_lookup([dev(2 * x - 3 * y) for x, y in zip(pa, pb)], dev(coords))
    check(lab, 2 * la.cpu() - 3 * lb.cpu(), 2e-5, what="lookup linearity")
    c0 = O.coords_grid(1, h, w)
    l0 = ops.corr_lookup([dev(t) for t in pa], dev(c0)).cpu()
    centre = l0[0, 4 * 9 + 4].reshape(-1)  # level 0, zero offset == V0[p][p]
    diag = pa[0][:, 0].reshape(P, P).diagonal()
    assert float((centre - diag).abs().max()) == 0.0
    # correlation volume: symmetric under swapping the feature maps (transpose), pyramid level sizes
    f1, f2 = torch.randn(1, 256, 20, 24, generator=g), torch.randn(1, 256, 20, 24, generator=g)
    v12 = ops.corr_volume(dev(f1), dev(f2))
    v21 = ops.corr_volume(dev(f2), dev(f1))
    a = v12[0].view(480, 480).cpu()
    bt = v21[0].view(480, 480).cpu().t()
    assert float((a - bt).abs().max()) < 1e-4
    assert [tuple(t.shape[2:]) for t in v12] == [(20, 24), (10, 12), (5, 6), (2, 3)]


def test_gma_accflow_mid_size_vs_oracle(ops):
    """AccFlow(GMA) (BASELINE configs[4] family) at 192x320, 3 frames, against the oracle run on the same inputs:
    exercises attention / aggregation inside the accumulation path at a size the CPU finishes in seconds."""
    from accflow_amd.data.synthetic import make_sequence, make_state_dict, normalize
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.AccFlow_ import AccFlow
    model = AccFlow(build_flow_estimator("acc|gma"))
    sd = make_state_dict(model)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    model.ofe_iters = 6
    frames = [normalize(f) for f in make_sequence(1003, 3, 192, 320)]
    out = model(images=[dev(f) for f in frames])[-1].cpu()
    ref = O.accflow_forward(sd, frames, iters=6, gma=True)[-1]
    me, mx = O.epe(out, ref)
    assert me <= 1e-3 and mx <= 2e-2, (me, mx)


def _accflow(name, **kw):
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.AccFlow_ import AccFlow
    model = AccFlow(build_flow_estimator(name), **kw)
    sd = make_state_dict(model)
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval(), sd


def test_accflow_gma_c5_7x720x1280_vs_reference(ops, golden):
    """BASELINE configs[4]: 7-frame 720x1280 AccFlow(GMA) - P = 14 400 query pixels, 829 MB of attention per image1,
    4.2 GB correlation pyramids - against the reference's own outputs (every 8th pixel; make_golden.py --c5)."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    g = golden("accflow_gma_c5")
    model, _ = _accflow("acc|gma")
    frames = [dev(normalize(f)) for f in make_sequence(int(g["seed"]), 7, 720, 1280)]
    outs = model(images=frames)
    assert len(outs) == 5
    for k, o in enumerate(outs):
        me, mx = O.epe(o[:, :, ::8, ::8].cpu(), T(g["out%d" % k]))
        print("C5 out%d: EPE mean %.2e max %.2e" % (k, me, mx))
        assert me <= 1e-3 and mx <= 5e-3, (k, me, mx, "measured max 1.00e-3")


def test_c5_size_properties(ops):
    """Size-independent properties at C5's 90x160 working size (P = 14 400): displaced pyramid is an exact permutation
    of the row-major one, lookups agree between the layouts and read exact entries at integer coordinates, attention
    rows sum to 1 in both storage orders."""
    g = gen(55)
    h, w = 90, 160
    P = h * w
    f1, f2 = torch.randn(1, 256, h, w, generator=g), torch.randn(1, 256, h, w, generator=g)
    with ops.conv_mode("bf16x6"):
        dp = ops.corr_volume_disp(dev(f1), dev(f2))
        rm = ops.corr_volume(dev(f1), dev(f2))
    back = dp.to_rowmajor()
    for l in range(4):
        assert tuple(back[l].shape) == (P, 1, h >> l, w >> l)
        # level 0 comes from two different GEMM kernels (same arithmetic, different summation order)
        check(back[l], rm[l], 3e-5, what="C5 displaced level %d vs row-major" % l)
    again = ops.corr_disp_pool(dp.levels[0], h, w)
    for l in range(1, 4):  # (valid query pixels: the padding lanes of the last 128-pixel block are never written)
        assert maxerr(again._unblocked(again.levels[l], h >> l, w >> l), dp._unblocked(dp.levels[l], h >> l, w >> l)) == 0.0
    coords = O.coords_grid(1, h, w) + 5.0 * torch.randn(1, 2, h, w, generator=g)
    check(ops.corr_lookup(dp, dev(coords)), ops.corr_lookup(back, dev(coords)), 1e-5, what="C5 lookup, displaced vs row-major")
    c0 = O.coords_grid(1, h, w)
    l0 = ops.corr_lookup(dp, dev(c0)).cpu()
    diag = back[0][:, 0].reshape(P, P).diagonal().cpu()
    assert float((l0[0, 4 * 9 + 4].reshape(-1) - diag).abs().max()) == 0.0
    qk = torch.randn(1, 256, h, w, generator=g)
    at = ops.gma_attention_t(dev(qk), 128, 128 ** -0.5)       # [j][i]
    rows = at.sum(dim=1).cpu()
    assert float((rows - 1.0).abs().max()) < 1e-4
    del at
    a = ops.gma_attention(dev(qk), 128, 128 ** -0.5)
    assert float((a.sum(dim=-1).cpu() - 1.0).abs().max()) < 1e-4


@pytest.mark.parametrize("wscale,xscale", [(2.0 ** -6, 2.0 ** -8)])
def test_modules_f16x3_small_magnitudes(ops, wscale, xscale):
    """Update block and AccPlus with every conv weight scaled by 2^-6 and the activations fed in scaled by 2^-8
    (the regime of trained / ZeroConv-scaled checkpoints where an unscaled fp16 lo term would be subnormal):
    f16x3 against the oracle, error relative to the output's magnitude."""
    from accflow_amd.networks.AccFlow_ import AccPlus
    g = gen(61)
    m, sd = _models("raft")
    sd2 = {k: (v * wscale if (k.startswith("update_block.") and k.endswith(".weight")) else v) for k, v in sd.items()}
    m.load_state_dict(sd2, strict=True)
    B, h, w = 2, 24, 40
    net = torch.tanh(torch.randn(B, 128, h, w, generator=g)) * xscale
    inp = torch.relu(torch.randn(B, 128, h, w, generator=g)) * xscale
    corr = torch.randn(B, 324, h, w, generator=g) * xscale
    flow = torch.randn(B, 2, h, w, generator=g) * xscale
    rn, rm, rd = O.update_block(net, inp, corr, flow, sd2)
    with ops.conv_mode("f16x3"):
        n1, m1, d1 = m.update_block(dev(net), dev(inp), dev(corr), dev(flow))
    for name, got, ref in (("net", n1, rn), ("mask", m1, rm), ("delta", d1, rd)):
        rel = float((got.cpu() - ref).abs().max() / ref.abs().max())
        print("small-magnitude update block %s: max err / max |ref| = %.2e (|ref| max %.2e)" % (name, rel, float(ref.abs().max())))
        assert rel <= 5e-6, (name, rel)
    acc = AccPlus(128)
    from accflow_amd.data.synthetic import make_state_dict
    asd = make_state_dict(acc)
    asd2 = {k: (v * wscale if (k.endswith(".weight") and "conv2.4" not in k) else v) for k, v in asd.items()}
    acc.load_state_dict(asd2, strict=True)
    acc = acc.cuda().eval()
    df, f, c = [torch.randn(B, 128, h, w, generator=g) * xscale for _ in range(3)]
    o = (torch.rand(B, 1, h, w, generator=g) > 0.3).float()
    ref, _ = O.accplus(df, f, o, c, {"accplus." + k: v for k, v in asd2.items()})
    with ops.conv_mode("f16x3"):
        got = acc(dev(df), dev(f), dev(o), dev(c)).cpu()
    rel = float((got - ref).abs().max() / ref.abs().max())
    print("small-magnitude AccPlus: max err / max |ref| = %.2e (|ref| max %.2e)" % (rel, float(ref.abs().max())))
    assert rel <= 5e-6, rel


def test_guard_through_every_entry_point(ops):
    """An activation outside the fp16 split's range must be caught (bf16x6 recomputation, finite result equal to the
    oracle's) through iter(), estimate_small / fuse_chain (the two halves of forward_pair_sharded) and sub-module
    forwards, not only through forward()."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    model, sd = _accflow("acc|raft")
    model.ofe_iters = 2
    frames = [normalize(f) for f in make_sequence(1001, 3, 128, 256)]
    hot = [f.clone() for f in frames]
    hot[2][0, 1, 40, 100] = 6.0e3             # x 2^4 leaves fp16's range in the first conv's input patch
    cold_ref = O.accflow_forward(sd, frames, iters=2)[-1]
    # what the guarded call must return: the unconditional fp32-equivalent arithmetic on the same inputs (a 3e4 spike in
    # a [-1, 1] image makes the instance-normalised features ill-conditioned, so the oracle is only a loose check here)
    with ops.conv_mode("bf16x6"):
        ref = model(images=[dev(f) for f in hot])[-1].cpu()
        again = model(images=[dev(f) for f in hot])[-1].cpu()
        ref_iter = model.iter(dev(hot[2]), dev(hot[1]), dev(hot[0]), None)[1].cpu()   # (iter() runs the estimator's default 12 iterations)
    assert maxerr(again, ref) == 0.0, ("the path must be deterministic run to run", maxerr(again, ref))
    me, mx = O.epe(ref, O.accflow_forward(sd, hot, iters=2)[-1])
    print("hot input, bf16x6 vs oracle: EPE mean %.2e max %.2e" % (me, mx))
    assert bool(torch.isfinite(ref).all()) and me <= 5e-2
    with ops.conv_mode("f16x3"):
        ops.guard_tripped()
        ops.guard_report()
        out = model(images=[dev(f) for f in hot])[-1].cpu()
        assert bool(torch.isfinite(out).all()) and not ops.guard_tripped()
        # round 4: the guard retries per STAGE and reports which (a spike in the image reaches every stage here: cnet and
        # the context encoder have no per-sample norm, so the stages they feed see it too; the selectivity of the
        # fallback is checked in test_guard_at_trained_magnitudes_falls_back_per_stage)
        trips = ops.guard_report()
        print("stages that fell back:", trips)
        known = ("BasicEncoder.forward", "RAFT.refine", "AccFlow.context", "AccFlow.fuse_chain")
        assert trips and all(t in known for t in trips), trips
        assert maxerr(out, ref) <= 2e-3, ("forward", maxerr(out, ref))
        small, up = model.iter(dev(hot[2]), dev(hot[1]), dev(hot[0]), None)
        assert bool(torch.isfinite(up).all()) and maxerr(up, ref_iter) <= 2e-3, ("iter", maxerr(up, ref_iter))
        # pair-sharded halves, world size 1 (no process group): the same path the multi-GPU mode runs per rank
        out_ps = model.forward_pair_sharded([dev(f) for f in hot])[-1].cpu()
        assert bool(torch.isfinite(out_ps).all()) and maxerr(out_ps, ref) <= 1e-3, ("pair_sharded", maxerr(out_ps, ref))
        # a sub-module called on its own
        x = torch.randn(1, 2, 16, 32, generator=gen(3))
        x[0, 0, 3, 3] = 1.0e4
        fe = model.flow_encoder(dev(x)).cpu()
        check(fe, O.flow_encoder(x, sd), 2e-2, rtol=1e-4, what="guarded FlowEncoder")
        # and the untouched inputs still take the fast path with the same answer as the oracle
        me, mx = O.epe(model(images=[dev(f) for f in frames])[-1].cpu(), cold_ref)
        assert me <= 1e-3, me


def test_guard_at_trained_magnitudes_falls_back_per_stage(ops):
    """no released checkpoint exists offline, so whether the fp16 split's fast path survives the
    activation magnitudes of TRAINED un-normalised encoders (AccFlow's `context` has no norm at all, AccFlow_.py:152; cnet's
    `inp` is a bare ReLU) is emulated: the head convolutions of `cnet` and `context` are scaled so that their outputs reach
    10^3 - 10^4 (beyond 4095 = 65520 / 2^4).  The forward must stay within the parity gate of the oracle ON THE SAME
    WEIGHTS, only the stages that read those tensors may fall back, and the report says which."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    model, sd = _accflow("acc|raft")
    model.ofe_iters = 2
    sd = {k: v.clone() for k, v in sd.items()}
    frames = [normalize(f) for f in make_sequence(1003, 3, 128, 256)]
    with torch.no_grad():
        base = O.accflow_forward(sd, frames, iters=2)[-1]
    for case, keys, expect in (("context", ("context.conv2.weight", "context.conv2.bias"), ("AccFlow.context", "fuse_chain")),
                               ("cnet", ("ofe.cnet.conv2.weight", "ofe.cnet.conv2.bias"), ("refine",))):
        sd2 = {k: v.clone() for k, v in sd.items()}
        probe = O.basic_encoder(frames[0], sd2, "context" if case == "context" else "ofe.cnet", "none" if case == "context" else "batch")
        scale = 6.0e3 / float(probe.abs().max())
        for k in keys:
            sd2[k] = sd2[k] * scale
        model.load_state_dict(sd2, strict=True)
        with torch.no_grad():
            ref = O.accflow_forward(sd2, frames, iters=2)[-1]
        with ops.conv_mode("f16x3"):
            ops.guard_report()
            out = model(images=[dev(f) for f in frames])[-1].cpu()
            trips = ops.guard_report()
        me, mx = O.epe(out, ref)
        mag = float(ref.abs().mean())
        print("%s head x %.0f: activations to 6e3, EPE vs oracle %.2e (max %.2e, mean |flow| %.2f), stages that fell back: %s"
              % (case, scale, me, mx, mag, trips))
        assert bool(torch.isfinite(out).all()) and me <= 1e-3 * max(1.0, mag), (case, me, mag)
        assert trips and all(any(e in t for e in expect) for t in trips), (case, trips)   # nothing else fell back
    model.load_state_dict(sd, strict=True)
    with ops.conv_mode("f16x3"):
        ops.guard_report()
        me, _ = O.epe(model(images=[dev(f) for f in frames])[-1].cpu(), base)
        assert me <= 1e-3 and ops.guard_report() == []


def test_s16_lookup_vs_oracle_directly(ops):
    """accflow_corr_lookup_disp_s16 against the oracle's CorrBlock lookup (raft/corr.py:24-45), not only against the
    library's fp32 form: de-split the 4 x 88 pre-split channels ((hi + lo) / 2^4), undo the per-level (row, column) tap
    order and compare with O.corr_lookup on the same volume and coordinates."""
    g = gen(21)
    B, C, H8, W8 = 2, 64, 16, 24
    f1, f2 = torch.randn(B, C, H8, W8, generator=g), torch.randn(B, C, H8, W8, generator=g)
    coords = O.coords_grid(B, H8, W8) + torch.randn(B, 2, H8, W8, generator=g) * 3.0
    coords[0, :, 0, 0] = torch.tensor([-7.5, 3.25])            # a window partly outside
    coords[1, :, 5, 5] = torch.tensor([4.0, 9.0])              # integer coordinates
    want = O.corr_lookup(O.corr_pyramid(f1, f2), coords)       # (B, 324, H8, W8)
    with ops.conv_mode("f16x3"):
        pyr = ops.corr_volume_disp(dev(f1), dev(f2))
        out16 = ops.S16.empty(B, ops.LOOKUP_S16_CHANNELS, H8, W8, pyr.levels[0].device, zero=True)
        ops.corr_lookup_s16(pyr, dev(coords), out16)
    got88 = out16.to_float().cpu().view(B, 4, 88, H8, W8)
    assert float(got88[:, :, 81:].abs().max()) == 0.0          # the 7 tail channels of each level are zero
    got = got88[:, :, :81].reshape(B, 4, 9, 9, H8, W8).transpose(2, 3).reshape(B, 324, H8, W8)   # [l][j][i] -> l*81 + i*9 + j
    check(got, want, 2e-5, rtol=1e-5, what="S16 lookup vs oracle")


def test_threads_and_data_parallel(ops, golden):
    """SURVEY 8(b) threading clause (test_cvo.py:18,26 drives the model through nn.DataParallel = one host thread per
    GPU): two Python threads run model.forward concurrently on the same GPU - one of them on inputs that trip the
    fp16 range guard, so its bf16x6 retry must not change what the other thread computes - and
    nn.DataParallel(model, device_ids=[0]) gives the plain model's result."""
    import threading
    from accflow_amd.data.synthetic import make_sequence, normalize
    model, sd = _accflow("acc|raft")
    model.ofe_iters = 3
    fa = [dev(normalize(f)) for f in make_sequence(1002, 4, 128, 256)]
    fb = [f.clone() for f in fa]
    fb[3][0, 0, 10:14, 20:24] = 2.0e4
    with ops.conv_mode("f16x3"):
        ra = [o.clone() for o in model(images=fa)]
        rb = [o.clone() for o in model(images=fb)]
    torch.cuda.synchronize()
    results, errors = {}, []

    def work(tag, frames, n):
        try:
            torch.cuda.set_device(0)
            with ops.conv_mode("f16x3"), torch.cuda.stream(torch.cuda.Stream()):
                for _ in range(n):
                    outs = model(images=frames)
                torch.cuda.current_stream().synchronize()
            results[tag] = outs
        except Exception as e:  # noqa: BLE001
            errors.append((tag, repr(e)))

    ts = [threading.Thread(target=work, args=("a", fa, 3)), threading.Thread(target=work, args=("b", fb, 3))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for k in range(len(ra)):
        assert maxerr(results["a"][k], ra[k]) <= 1e-5, ("thread a", k, maxerr(results["a"][k], ra[k]))
        assert maxerr(results["b"][k], rb[k]) <= 1e-3, ("thread b", k, maxerr(results["b"][k], rb[k]))
    dp = torch.nn.DataParallel(model, device_ids=[0])
    with ops.conv_mode("f16x3"):
        od = dp(images=fa, test_mode=False)
    assert len(od) == len(ra)
    for k in range(len(ra)):
        assert maxerr(od[k], ra[k]) <= 1e-5


def test_encoder_schedules(ops, monkeypatch):
    """RAFT.estimate_pairs' encoder schedules (raft.ENCODER_STREAMS; round 6): 1 = cnet on the second pair-group stream underneath
    fnet, 2 = the pair groups fork at an event behind the correlation operand packs and build their pyramids underneath cnet,
    3 = both.
    Same bits as 0 (one after the other, then the fork) - for a clean sequence, for one that trips the f16x3 range guard (the
    optimistic pass uses the schedule, the stage-by-stage retry falls back to 0), in bf16x6, and for the GMA estimator."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    from accflow_amd.networks.raft import raft as raft_mod
    for name in ("acc|raft", "acc|gma"):
        model, sd = _accflow(name)
        model.ofe_iters = 2
        clean = [dev(normalize(f)) for f in make_sequence(1200, 4, 128, 256)]
        hot = [f.clone() for f in clean]
        hot[1][0, 1, 30:34, 40:44] = 2.0e4
        results = {}
        for sched in (0, 1, 2, 3):
            monkeypatch.setattr(raft_mod, "ENCODER_STREAMS", sched)
            for mode in ("f16x3", "bf16x6"):
                with ops.conv_mode(mode):
                    results[(sched, mode, "clean")] = [o.clone() for o in model(images=clean)]
            with ops.conv_mode("f16x3"):
                ops.guard_report()
                results[(sched, "f16x3", "hot")] = [o.clone() for o in model(images=hot)]
                assert ops.guard_report(), "the hot frame must trip the guard"
        torch.cuda.synchronize()
        for key in [k for k in results if k[0]]:
            for a_, b_ in zip(results[key], results[(0,) + key[1:]]):
                assert bool(torch.isfinite(a_).all()) and torch.equal(a_, b_), (name, key)


@pytest.mark.parametrize("split", [False, True])
def test_sequence_pipeline(ops, monkeypatch, split):
    """parallel.SequencePipeline (fusion chain of sequence k on a side stream underneath the estimator of k+1):
    every sequence's outputs equal model(images) bit for bit; a sequence that trips the f16x3 range guard comes back
    recomputed in bf16x6 without disturbing its neighbours; warm-start models and 2-frame inputs pass through.
    split: parallel.PIPELINE_SPLIT - the encoders on the caller's stream, the refinement homed on a pair-group stream."""
    from accflow_amd import parallel as parallel_mod
    from accflow_amd.data.synthetic import make_sequence, normalize
    from accflow_amd.parallel import SequencePipeline
    monkeypatch.setattr(parallel_mod, "PIPELINE_SPLIT", split)
    model, sd = _accflow("acc|raft")
    model.ofe_iters = 3
    seqs = [[dev(normalize(f)) for f in make_sequence(1010 + k, 4, 128, 256)] for k in range(4)]
    seqs[2][3][0, 0, 10:14, 20:24] = 2.0e4      # this one leaves the fp16 split's range
    from accflow_amd.networks.AccFlow_ import pipeline_chain_arithmetic
    with ops.conv_mode("f16x3"):
        # (the pipelined modes run the chain's batch-1 convolutions without split-K - another order of the same fp32 sums:
        # model(images) inside pipeline_chain_arithmetic() is what they equal bit for bit, the plain forward to ~1e-6 px)
        with pipeline_chain_arithmetic():
            refs = [[o.clone() for o in model(images=fr)] for fr in seqs]
        plain = [o.clone() for o in model(images=seqs[0])]
        assert all(maxerr(a_, b_) <= 1e-4 for a_, b_ in zip(refs[0], plain))
        with ops.conv_mode("bf16x6"), pipeline_chain_arithmetic():
            hot_ref = [o.clone() for o in model(images=seqs[2])]
        pipe = SequencePipeline(model)
        got = []
        for fr in seqs:
            r = pipe.submit(fr)
            if r is not None:
                got.append(r)
        got.append(pipe.flush())
        assert pipe.flush() is None
    assert len(got) == len(seqs)
    for k, (g_, r_) in enumerate(zip(got, refs)):
        assert len(g_) == len(r_) == 2
        for a_, b_ in zip(g_, r_):
            assert bool(torch.isfinite(a_).all())
            assert torch.equal(a_, b_), ("sequence %d differs from model(images)" % k, maxerr(a_, b_))
    for a_, b_ in zip(got[2], hot_ref):
        assert torch.equal(a_, b_), "the tripped sequence must be the bf16x6 result"
    # the rotating-root stream mode (one rank = root of every sequence): the same contract, and no host synchronisation
    # inside its loop - the estimator's range flag rides in the all_gather payload, the chain's is read at the harvest
    with ops.conv_mode("f16x3"):
        ops.guard_report()
        st = model.forward_pair_sharded_stream(seqs)
        assert ops.guard_report() == ["AccFlow.forward_pair_sharded_stream"]
    assert sorted(st) == list(range(len(seqs)))
    for k in st:
        for a_, b_ in zip(st[k], hot_ref if k == 2 else refs[k]):
            assert torch.equal(a_, b_), ("stream mode, sequence %d" % k, maxerr(a_, b_))
    # other conv modes: no flag, same overlap
    with ops.conv_mode("bf16x6"):
        with pipeline_chain_arithmetic():
            ref = model(images=seqs[0])
        pipe = SequencePipeline(model)
        assert pipe.submit(seqs[0]) is None
        out = pipe.flush()
    assert all(torch.equal(a_, b_) for a_, b_ in zip(out, ref))
    # pass-through cases
    pipe = SequencePipeline(model)
    assert pipe.submit(seqs[0][:2]) is None and pipe.flush() == []
    warm, _ = _accflow("acc|raft", warm_start=True, warm_iters=2)
    warm.ofe_iters = 3
    pw = SequencePipeline(warm)
    pw.submit(seqs[1])
    ow = pw.flush()
    rw = warm(images=seqs[1])
    assert all(torch.equal(a_, b_) for a_, b_ in zip(ow, rw))


def test_sequence_pipeline_full_size_many_steps(ops):
    """The pipeline at the benchmark's size (7 x 480x1024) over several back-to-back steps without a synchronisation in
    between: tensors that one stream allocates and another one uses (the encoder outputs and - round 6 - the refinement's
    prepared pyramids / workspaces, built on the caller's stream and used by the pair-group streams) must outlive that use.  A
    lifetime bug here does not show at the small shapes of test_sequence_pipeline (it did not, in development): it needs the
    caller's stream to allocate multi-GB activations while the previous refinement is still running.  Every step's outputs
    equal the plain forward's bits (pipeline arithmetic), no step trips the range guard."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    from accflow_amd.networks.AccFlow_ import pipeline_chain_arithmetic
    from accflow_amd.parallel import SequencePipeline
    model, sd = _accflow("acc|raft")
    model.ofe_iters = 4
    seqs = [[dev(normalize(f)) for f in make_sequence(1400 + k, 7, 480, 1024)] for k in range(2)]
    with ops.conv_mode("f16x3"):
        with pipeline_chain_arithmetic():
            refs = [[o.clone() for o in model(images=fr)] for fr in seqs]
        pipe = SequencePipeline(model)
        got, trips = [], []
        for k in range(7):
            pend = pipe.pending
            r = pipe.submit(seqs[k & 1])
            if pend is not None and pend[1] is not None:
                trips.append(int(pend[1].item()))
            if r is not None:
                got.append(r)
        pend = pipe.pending
        got.append(pipe.flush())
        trips.append(int(pend[1].item()))
    assert trips == [0] * 7, trips
    assert len(got) == 7
    for k, outs in enumerate(got):
        for a_, b_ in zip(outs, refs[k & 1]):
            assert torch.equal(a_, b_), ("step %d" % k, maxerr(a_, b_))


def test_cvo_scale_batch_invariance(ops):
    """The shape test_cvo.py really drives (test_cvo.py:114-116: batch 10, CVO frames 512x512, 7 frames): one forward
    over N = 10 sequences = 110 estimator pairs per launch, through the sequence pipeline, equals the same sequences
    run one at a time (no cross-item arithmetic; only tile / split-K choices differ with the batch)."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    from accflow_amd.parallel import SequencePipeline
    model, sd = _accflow("acc|raft")
    model.ofe_iters = 4
    N, H, W = 10, 512, 512
    frames = [dev(normalize(f)) for f in make_sequence(1300, 7, H, W, batch=N)]
    pipe = SequencePipeline(model)
    assert pipe.submit(frames) is None
    outs = pipe.flush()
    assert len(outs) == 5 and tuple(outs[-1].shape) == (N, 2, H, W) and bool(torch.isfinite(outs[-1]).all())
    for n in (0, 7):
        single = model(images=[f[n:n + 1].contiguous() for f in frames])
        for k in (0, 4):
            me, mx = O.epe(outs[k][n:n + 1].cpu(), single[k].cpu())
            assert me <= 1e-4 and mx <= 5e-3, ("batch item %d, output %d" % (n, k), me, mx)
    del outs, single
    torch.cuda.empty_cache()


def test_warm_start_vs_oracle(ops):
    """AccFlow(warm_start=True) - long-range pairs seeded through flow_init with the composed
    accumulated flow - against the oracle's restatement of the same schedule; estimate_pairs(flow_init=...) against
    per-pair forward(flow_init=...); flow composition against the oracle."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    g = gen(71)
    a, b = torch.randn(2, 2, 20, 28, generator=g) * 3, torch.randn(2, 2, 20, 28, generator=g) * 3
    check(ops.compose_flow(dev(a), dev(b)), O.compose_flow(a, b), 1e-5, what="compose_flow")
    model, sd = _accflow("acc|raft", warm_start=True, warm_iters=3)
    model.ofe_iters = 4
    frames = [normalize(f) for f in make_sequence(1004, 4, 128, 256)]
    outs = model(images=[dev(f) for f in frames])
    refs = O.accflow_forward_warm(sd, frames, iters=4, warm_iters=3)
    assert len(outs) == len(refs) == 2
    for k, (o, r) in enumerate(zip(outs, refs)):
        me, mx = O.epe(o.cpu(), r)
        print("warm start out%d: EPE mean %.2e max %.2e" % (k, me, mx))
        assert me <= 1e-3 and mx <= 5e-4, (k, me, mx, "measured max 8.13e-5")
    ofe = model.ofe
    fi = torch.randn(2, 2, 16, 32, generator=g) * 0.5
    both = ofe.estimate_pairs([dev(f) for f in frames], [(2, 1), (3, 0)], iters=3, flow_init=dev(fi))
    one = ofe(dev(frames[3]), dev(frames[0]), iters=3, flow_init=dev(fi[1:]))
    assert maxerr(both[1:], one) <= 1e-4
    # the default (cold) schedule is untouched by the option
    cold, _ = _accflow("acc|raft")
    cold.ofe_iters = 4
    me, mx = O.epe(cold(images=[dev(f) for f in frames])[-1].cpu(), O.accflow_forward(sd, frames, iters=4)[-1])
    assert me <= 1e-3


def test_rccl_world_size_1_real_model(ops):
    """The multi-GPU code path on the RCCL backend with the REAL model at C1 size: init_process_group("nccl") with one
    rank (the GPU box has one MI355X), run_sequence_sharded's gather and AccFlow.forward_pair_sharded's all_gather
    (dtype / contiguity / device of the collectives' operands, HSA_ENABLE_IPC_MODE_LEGACY=0 environment)."""
    import os
    import torch.distributed as dist
    from accflow_amd.data.synthetic import make_sequence, normalize
    from accflow_amd.parallel import run_sequence_sharded
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = "29533"
    model, sd = _accflow("acc|raft")
    model.ofe_iters = 2
    seqs = [[dev(normalize(f)) for f in make_sequence(1010 + s, 4, 128, 256)] for s in range(2)]
    want = [model(images=s)[-1].cpu() for s in seqs]
    from accflow_amd.networks.AccFlow_ import pipeline_chain_arithmetic
    with pipeline_chain_arithmetic():      # (the pipelined modes' chain: no split-K in its batch-1 convolutions)
        want_p = [model(images=s)[-1].cpu() for s in seqs]
    assert all(maxerr(a, b) <= 2e-4 for a, b in zip(want_p, want))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        got = run_sequence_sharded(lambda s: model(images=s)[-1], seqs, dst=0)
        assert len(got) == 2
        for a, b in zip(got, want):
            assert maxerr(a, b) <= 1e-5
        from accflow_amd.parallel import SequencePipeline
        got_p = run_sequence_sharded(SequencePipeline(model), seqs, dst=0)
        assert len(got_p) == 2 and all(maxerr(a, b) <= 1e-5 for a, b in zip(got_p, want_p))
        # world size 1 goes through gather_to_root's shortcut; force the collective itself as well
        t = want[0].cuda().contiguous()
        bufs = [torch.empty_like(t)]
        dist.gather(t, gather_list=bufs, dst=0)
        assert maxerr(bufs[0], want[0]) == 0.0
        lst = [torch.empty_like(t)]
        dist.all_gather(lst, t)
        assert maxerr(lst[0], want[0]) == 0.0
        ps = model.forward_pair_sharded(seqs[0])
        assert maxerr(ps[-1], want[0]) <= 1e-5
        # the rotating-root stream mode (one rank: it is the root of every sequence; the chain of sequence k runs on the side
        # stream underneath the estimator of sequence k + 1, the all_gather runs per sequence)
        st = model.forward_pair_sharded_stream(seqs)
        assert sorted(st) == [0, 1] and all(maxerr(st[k][-1], want_p[k]) <= 1e-5 for k in st)
    finally:
        dist.destroy_process_group()


def test_pair_sharded_equals_forward_c3(ops, golden):
    """The strong-scaling path at full size before a node exists: AccFlow.forward_pair_sharded on 7 x 480x1024 (world
    size 1, RCCL group initialised so that the all_gather really runs) == model(images) bit for bit - same kernels,
    same batch composition - and within the 1e-3 px gate of the reference's outputs; time printed."""
    import os
    import time
    import torch.distributed as dist
    from accflow_amd.data.synthetic import make_sequence, normalize
    g = golden("accflow_c3")
    model, _ = _accflow("acc|raft")
    frames = [dev(normalize(f)) for f in make_sequence(int(g["seed"]), 7, 480, 1024)]
    want = model(images=frames)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = "29541"
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        got = model.forward_pair_sharded(frames, dst=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            got = model.forward_pair_sharded(frames, dst=0)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / 3 * 1e3
    finally:
        dist.destroy_process_group()
    assert len(got) == 5
    for k, (a, b) in enumerate(zip(got, want)):
        assert maxerr(a, b) == 0.0, k
        me, mx = O.epe(a[:, :, ::8, ::8].cpu(), T(g["out%d" % k]))
        assert me <= 1e-3 and mx <= 2e-2, (k, me, mx)
    print("forward_pair_sharded, 7x480x1024, 1 rank: %.2f ms per sequence" % ms)


def test_zero_conv2d_forward(ops):
    """networks/modules.py:94-97: ZeroConv2d.forward = conv3x3(x) * exp(3 * scale) (called stand-alone; AccPlus folds the
    same factor into its packed weights)."""
    import torch.nn.functional as F
    from accflow_amd.networks.modules import ZeroConv2d
    g = gen(91)
    m = ZeroConv2d(128, 27)
    with torch.no_grad():
        m.conv.weight.copy_(torch.randn(27, 128, 3, 3, generator=g) * 0.03)
        m.conv.bias.copy_(torch.randn(27, generator=g) * 0.1)
        m.scale.copy_(torch.randn(1, 27, 1, 1, generator=g) * 0.3)
    x = torch.randn(2, 128, 20, 28, generator=g)
    ref = F.conv2d(x, m.conv.weight, m.conv.bias, padding=1) * torch.exp(m.scale * 3)
    got = m.cuda()(dev(x))
    check(got, ref.detach(), 3e-5, rtol=1e-5, what="ZeroConv2d.forward")
    # the pack is keyed on the `scale` PARAMETER: the same parameter -> the same pack object (exp(3*scale) is not even
    # recomputed); an in-place update of `scale` alone (optimizer step, partial load) -> a fresh pack with the new factor
    pk0 = m._packs.conv("z", m.conv, scale=m.out_scale, scale_dep=m.scale)
    m(dev(x))
    assert m._packs.conv("z", m.conv, scale=m.out_scale, scale_dep=m.scale) is pk0
    with torch.no_grad():
        m.scale.mul_(-0.5)
    ref2 = F.conv2d(x, m.conv.weight.cpu(), m.conv.bias.cpu(), padding=1) * torch.exp(m.scale.cpu() * 3)
    check(m(dev(x)), ref2.detach(), 3e-5, rtol=1e-5, what="ZeroConv2d.forward after an in-place scale update")
    assert m._packs.conv("z", m.conv, scale=m.out_scale, scale_dep=m.scale) is not pk0
    with pytest.raises(RuntimeError):
        m(x)  # CPU tensor into a module that lives on the GPU: no CPU path in the product


def test_gru_context_hoist_and_flow_stack(ops):
    """Two exact re-arrangements of the update block: (1) the GRU gate convs cut along their input channels - the
    iteration-invariant context third convolved once and added through `pre` in the GRU epilogues - against the uncut
    convolution (both epilogues, large and split-K grids); (2) convf1's 7x7 convolution of the 2-channel flow as a 1x7
    convolution of the row-shifted 16-channel stack."""
    import torch.nn.functional as F
    g = gen(101)
    for B, h, w in ((1, 16, 32), (4, 60, 128)):
        hs = torch.tanh(torch.randn(B, 128, h, w, generator=g))
        inp = torch.relu(torch.randn(B, 128, h, w, generator=g))
        mot = torch.randn(B, 128, h, w, generator=g)
        wz = torch.randn(256, 384, 1, 5, generator=g) * 0.03
        bz = torch.randn(256, generator=g) * 0.1
        full = F.conv2d(torch.cat([hs, inp, mot], 1), wz, bz, padding=(0, 2))
        z_ref, r_ref = torch.sigmoid(full[:, :128]), torch.sigmoid(full[:, 128:])
        wv = torch.cat([wz[:, :128], wz[:, 256:]], 1).contiguous()
        pkv = ops.PackedConv(dev(wv), dev(bz), padding=(0, 2), C0=128)
        pkc = ops.PackedConv(dev(wz[:, 128:256].contiguous()), None, padding=(0, 2))
        pre = ops.conv2d(pkc, dev(inp))
        z = torch.empty(B, 128, h, w, device="cuda")
        rh = torch.empty(B, 128, h, w, device="cuda")
        ops.conv2d(pkv, dev(hs), in1=dev(mot), out=z, act=ops.ACT_SIGMOID, epi=ops.EPI_GRU_ZR, e0=dev(hs), out2=rh, pre=pre)
        check(z, z_ref, 2e-5, what="z gate with hoisted context (B=%d)" % B)
        check(rh, r_ref * hs, 2e-5, what="r*h with hoisted context (B=%d)" % B)
        wq = torch.randn(128, 384, 5, 1, generator=g) * 0.03
        bq = torch.randn(128, generator=g) * 0.1
        q_ref = torch.tanh(F.conv2d(torch.cat([r_ref * hs, inp, mot], 1), wq, bq, padding=(2, 0)))
        h_ref = (1 - z_ref) * hs + z_ref * q_ref
        pkqv = ops.PackedConv(dev(torch.cat([wq[:, :128], wq[:, 256:]], 1).contiguous()), dev(bq), padding=(2, 0), C0=128)
        pkqc = ops.PackedConv(dev(wq[:, 128:256].contiguous()), None, padding=(2, 0))
        hd = dev(hs).clone()
        ops.conv2d(pkqv, dev(r_ref * hs), in1=dev(mot), out=hd, act=ops.ACT_TANH, epi=ops.EPI_GRU_Q, e0=hd, e1=dev(z_ref),
                   pre=ops.conv2d(pkqc, dev(inp)))
        check(hd, h_ref, 3e-5, what="h update with hoisted context (B=%d)" % B)
        with pytest.raises(RuntimeError):
            ops.conv2d(pkc, dev(inp), pre=pre)   # the addend exists for the GRU epilogues only
        # (2) flow stack
        flow = torch.randn(B, 2, h, w, generator=g) * 4
        wf = torch.randn(128, 2, 7, 7, generator=g) * 0.1
        bf = torch.randn(128, generator=g) * 0.1
        ref = torch.relu(F.conv2d(flow, wf, bf, padding=3))
        stack = torch.empty(B, 16, h, w, device="cuda")
        f2 = torch.empty(B, 2, h, w, device="cuda")
        ops.flow_from_coords(dev(flow), dst0=f2, stack16=stack, is_flow=True)
        assert maxerr(f2, flow) == 0.0
        want = torch.zeros(B, 16, h, w)
        for c in range(2):
            for ky in range(7):
                lo, hi = max(0, 3 - ky), min(h, h + 3 - ky)
                want[:, c * 7 + ky, lo:hi] = flow[:, c, lo + ky - 3:hi + ky - 3]
        assert maxerr(stack, want) == 0.0
        w2 = torch.zeros(128, 16, 1, 7)
        w2[:, :14, 0] = wf.reshape(128, 14, 7)
        pks = ops.PackedConv(dev(w2), dev(bf), padding=(0, 3))
        check(ops.conv2d(pks, stack, act=ops.ACT_RELU), ref, 3e-5, what="convf1 as a 1x7 conv of the flow stack (B=%d)" % B)
        coords = O.coords_grid(B, h, w) + flow
        ops.flow_from_coords(dev(coords), dst0=f2, stack16=stack)
        check(stack, want, 2e-5, what="flow stack from coordinates")


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
def test_corr_per_frame_packs(ops, mode):
    """accflow_corr_pack_f32 + accflow_corr_volume_disp_packed_f32: per-frame operand packs reused by several pairs give the
    very values of the per-pair call (C = 256: the 1/sqrt(C) moved into the accumulator scale is a power of two), and
    estimate_pairs through them equals per-pair forward calls."""
    g = gen(111)
    F_, C, h, w = 4, 256, 20, 26
    fm = torch.randn(F_, C, h, w, generator=g)
    idx1, idx2 = [2, 2, 1, 3, 3], [1, 0, 0, 2, 0]
    with ops.conv_mode(mode):
        packs = ops.corr_pack(dev(fm))
        pp = ops.corr_volume_disp_packed(packs, idx1, idx2)
        ref = ops.corr_volume_disp(dev(fm[idx1]), dev(fm[idx2]))
        # (bf16 terms: bitwise the per-pair call's values; fp16 split: the per-pair call folds 1/sqrt(C) into the query
        # map BEFORE splitting, which cancels its 2^4 activation scale, so its small values sit in the subnormal-lo regime
        # the per-frame pack avoids - equal to fp32 rounding, not bitwise)
        for l in range(4):
            err = maxerr(pp._unblocked(pp.levels[l], h >> l, w >> l), ref._unblocked(ref.levels[l], h >> l, w >> l))
            assert err == 0.0 if mode == "bf16x6" else err <= 3e-6, (l, err)
        with pytest.raises(RuntimeError):
            ops.corr_volume_disp_packed(packs, [0, 4], [0, 0])
    want = O.corr_pyramid(fm[idx1], fm[idx2])
    back = pp.to_rowmajor()
    for l in range(4):
        check(back[l], want[l], 3e-5, what="packed correlation level %d vs oracle" % l)
    from accflow_amd.data.synthetic import make_sequence, normalize
    m, _ = _models("raft")
    frames = [dev(normalize(f)) for f in make_sequence(1021, 4, 128, 256)]
    pairs = [(2, 1), (2, 0), (1, 0), (3, 2), (3, 0)]
    with ops.conv_mode(mode):
        both = m.estimate_pairs(frames, pairs, iters=3)
        for k, (i, j) in enumerate(pairs):
            one = m(frames[i], frames[j], iters=3)
            assert maxerr(both[k:k + 1], one) <= 2e-4, (k, maxerr(both[k:k + 1], one))


def test_folded_fusion_chain_matches_the_stepwise_chain(ops, monkeypatch):
    """AccFlow.fuse_chain hoists everything that does not depend on the accumulated flow out of the sequential loop
    (one _StepInputs over all steps: FlowEncoder of flow_ini / dflow, the occlusion and error maps and the blending mask, batched
    over the steps).  Same operators on the same values, so both forms must agree far inside the parity budget; batch 2
    exercises the (step, sample) indexing of the batched tensors.  With and without the deferred upsampling: hoisted and not
    deferred, every step blends into its own pre-split tensor and runs the whole decoder."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    from accflow_amd.networks import AccFlow_ as A
    if not (ops.s16_active() and A.USE_S16_CHAIN):
        pytest.skip("the folded chain is the S16 chain's")
    model, _ = _accflow("acc|raft")
    frames = [dev(normalize(f)) for f in make_sequence(321, 5, 128, 192, batch=2)]
    monkeypatch.setattr(A, "USE_CHAIN_HOIST", "0")
    stepwise = [o.cpu() for o in model(frames)]
    for hoist, defer in (("1", True), ("auto", True), ("1", False), ("auto", False)):
        monkeypatch.setattr(A, "USE_CHAIN_HOIST", hoist)
        monkeypatch.setattr(A, "USE_CHAIN_DEFER_UP", defer)
        got = [o.cpu() for o in model(frames)]
        assert len(got) == len(stepwise) == 3
        for a, b in zip(got, stepwise):
            me, mx = O.epe(a, b)
            print("hoist %s, deferral %s: EPE mean %.3e max %.3e" % (hoist, defer, me, mx))
            assert me <= 2e-5 and mx <= 2e-3, (hoist, defer, me, mx)


def test_deferred_upsampling_matches_the_per_step_decoder(ops, monkeypatch):
    """AccFlow.fuse_chain leaves the mask head + convex upsampling of every step out of the sequential loop and runs them
    once over all steps (only the 1/8-resolution flow feeds the next step, AccFlow_.py:171-175).  Same operators and values
    (the flow / mask heads' first convolutions run as two launches instead of one merged one)."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    from accflow_amd.networks import AccFlow_ as A
    if not (ops.s16_active() and A.USE_S16_CHAIN):
        pytest.skip("the deferred form belongs to the S16 chain")
    model, _ = _accflow("acc|raft")
    frames = [dev(normalize(f)) for f in make_sequence(654, 5, 128, 192, batch=2)]
    monkeypatch.setattr(A, "USE_CHAIN_HOIST", "0")     # (the deferral is the one loop's: with hoisting, see the test above)
    monkeypatch.setattr(A, "USE_CHAIN_DEFER_UP", True)
    deferred = [o.cpu() for o in model(frames)]
    monkeypatch.setattr(A, "USE_CHAIN_DEFER_UP", False)
    stepwise = [o.cpu() for o in model(frames)]
    assert len(deferred) == len(stepwise) == 3 and all(tuple(o.shape) == (2, 2, 128, 192) for o in deferred)
    for a, b in zip(deferred, stepwise):
        me, mx = O.epe(a, b)
        assert me <= 2e-5 and mx <= 2e-3, (me, mx)
