"""Every route of csrc/backward.hip against torch autograd of the SAME operator in float64 on the CPU, element by element
(tests/test_backward.py's measure: the largest absolute error over the RMS of the reference gradient, and its tolerances: 1e-4
for the convolution and deformable gradients, 1e-5 for the element-wise kernels and the convex upsampling, torch.equal where
the result is exact).

Weight gradient.  accflow_conv_wgrad_f32 chooses between three kernels and cuts the pixel axis into gridDim.z parts; which of
them a shape gets is asked from accflow_conv_wgrad_plan (backward.conv_wgrad_plan - the launcher's own host function) and
ASSERTED before the gradient is checked, so a case keeps exercising what its comment says:
    general / fast128 / fast64 with 20 live parts and one empty, parts that begin mid-row and mid-item (WGRAD_SPLIT_CASES),
    odd part lengths, stride 2 under a split, single-step problems, the fast predicate's fall-back edges at W % 8 == 0,
    tile edges in Cout and in J = Cin KH KW, bias=False (db == nullptr) on each kernel, channel slices on the general kernel
    with Z > 1; every split case twice (float atomics over the parts: 1e-5 apart).
Deformable backward.  accflow_deform_conv_backward_f32 runs deform_backward_lds_kernel<16> up to 1024 pixels, <8> up to 2048,
<4> up to 4096 (at 4096 exactly 65536 bytes of dynamic LDS) and the global-atomic deform_backward_kernel above; DEFORM_CASES
has a plane in each range and on both sides of the last boundary, channel counts that leave a ragged last channel group, offset
and mask as slices of one 27-channel tensor and x as a slice (the layouts of train.py), offsets that leave the image.
Input gradient, zero insertion and the small kernels: see the tests."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-4        # convolution and deformable gradients (tests/test_backward.py)
TOL_EW = 1e-5     # element-wise kernels, convex upsampling, two runs of one split weight gradient


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel(got, want):
    want = want.float()
    rms = float(want.pow(2).mean().sqrt().clamp_min(1e-30))
    return float((got.cpu() - want).abs().max()) / rms


@pytest.fixture(scope="module")
def bw():
    from accflow_amd import backward
    return backward


# ------------------------------------------------------------------------------------------------ weight gradient

def wgrad_check(bw, case, kernel, Z=None, per=None, steps=None, grid_xy=None, bias=True, sliced=False, twice=None):
    """Assert the planned route of `case`, then dw / db against float64 autograd.  Returns the plan."""
    B, Cin, Cout, H, W, KH, KW, s, pH, pW = case
    OH, OW = (H + 2 * pH - KH) // s + 1, (W + 2 * pW - KW) // s + 1
    g = gen(sum(case) + 7 * Cout)
    if sliced:
        X, DY = torch.randn(B, Cin + 9, H, W, generator=g), torch.randn(B, Cout + 7, OH, OW, generator=g)
        xc, dc = slice(4, 4 + Cin), slice(3, 3 + Cout)
    else:
        X, DY = torch.randn(B, Cin, H, W, generator=g), torch.randn(B, Cout, OH, OW, generator=g)
        xc = dc = slice(None)
    x, dy = X[:, xc], DY[:, dc]
    plan = bw.conv_wgrad_plan(B, Cin, Cout, H, W, KH, KW, stride=s, padding=(pH, pW),
                              x_bs=x.stride(0) if B > 1 else None, dy_bs=dy.stride(0) if B > 1 else None)
    assert plan["kernel"] == kernel and plan["terms"] == 3, plan
    for name, want in (("steps", steps), ("steps_per_part", per)):
        assert want is None or plan[name] == want, (name, plan)
    assert Z is None or plan["grid"][2] == Z, plan
    assert grid_xy is None or plan["grid"][:2] == grid_xy, plan
    w64 = torch.zeros(Cout, Cin, KH, KW, dtype=torch.double, requires_grad=True)
    F.conv2d(x.double(), w64, None, stride=s, padding=(pH, pW)).backward(dy.double())
    xg, dyg = X.cuda()[:, xc], DY.cuda()[:, dc]
    dw, db = bw.conv_wgrad(xg, dyg, KH, KW, stride=s, padding=(pH, pW), bias=bias)
    e = rel(dw, w64.grad)
    print("wgrad", case, plan, "dw %.2e" % e)
    assert e < TOL, ("dw", e, plan)
    if bias:
        e = rel(db, dy.double().sum((0, 2, 3)))
        print("db %.2e" % e)
        assert e < TOL, ("db", e, plan)
    else:
        assert db is None
    if plan["grid"][2] > 1 if twice is None else twice:
        again, _ = bw.conv_wgrad(xg, dyg, KH, KW, stride=s, padding=(pH, pW), bias=bias)
        e = rel(again, dw.cpu())
        print("second run %.2e" % e)
        assert e < TOL_EW, ("second run", e, plan)
    return plan


# B, Cin, Cout, H, W, KH, KW, stride, padH, padW -> kernel, steps, Z, steps per part
WGRAD_SPLIT_CASES = {
    # 20 live parts and an empty one; the parts begin at pixel 160 k: mid-row (160 % 24 = 16) and mid-item (an item = 168 px)
    "fast64-21-parts": ((19, 8, 40, 7, 24, 3, 3, 1, 1, 1), "fast64", 200, 21, 10),
    "fast128-21-parts": ((19, 8, 72, 7, 24, 3, 3, 1, 1, 1), "fast128", 200, 21, 10),
    # W = 23: the 8-pixel chunks straddle rows and items inside split parts
    "general-21-parts": ((19, 8, 72, 7, 23, 3, 3, 1, 1, 1), "general", 192, 21, 10),
    # 9 steps per part: a part ends on the FIRST register set of the two-step pipeline
    "fast128-odd-parts": ((13, 8, 72, 9, 24, 3, 3, 1, 1, 1), "fast128", 176, 20, 9),
    "fast64-odd-parts": ((13, 8, 40, 9, 24, 3, 3, 1, 1, 1), "fast64", 176, 20, 9),
    "general-stride2-split": ((11, 8, 72, 9, 23, 3, 3, 2, 1, 1), "general", 42, 5, 9),
}


@pytest.mark.parametrize("name", sorted(WGRAD_SPLIT_CASES))
def test_wgrad_split_parts(bw, name):
    case, kernel, steps, Z, per = WGRAD_SPLIT_CASES[name]
    plan = wgrad_check(bw, case, kernel, Z=Z, per=per, steps=steps, grid_xy=(1, 1))
    live = sum(1 for z in range(Z) if z * per < steps)
    assert live == {"21-parts": 20, "odd-parts": 20, "stride2-split": 5}[name.split("-", 1)[1]], plan


@pytest.mark.parametrize("name", ["fast64-21-parts", "fast128-21-parts", "general-21-parts"])
def test_wgrad_without_bias(bw, name):
    """db == nullptr (train.py: the ZeroConv scale gradient) on each kernel: dw as before, no db."""
    case, kernel, steps, Z, per = WGRAD_SPLIT_CASES[name]
    wgrad_check(bw, case, kernel, Z=Z, per=per, steps=steps, bias=False)


# a single 16-pixel step, half of it past the last pixel (the second prefetch is skipped); the fast predicate's fall-back
# edges at W % 8 == 0: KW - 1 - padW = 2, OW != W, stride 2
WGRAD_EDGE_CASES = [
    ((1, 8, 40, 1, 8, 3, 3, 1, 1, 1), "fast64", 1),
    ((1, 8, 72, 1, 8, 3, 3, 1, 1, 1), "fast128", 1),
    ((1, 8, 40, 3, 3, 3, 3, 1, 1, 1), "general", 1),
    ((1, 8, 40, 2, 8, 3, 3, 1, 1, 1), "fast64", 1),        # exactly one full step
    ((1, 8, 40, 3, 8, 3, 3, 1, 1, 1), "fast64", 2),        # two steps: the second prefetch runs, the third does not
    ((2, 8, 40, 6, 16, 5, 5, 1, 2, 2), "general", 12),
    ((2, 8, 40, 6, 16, 3, 3, 1, 1, 0), "general", 11),
    ((2, 8, 40, 6, 16, 3, 3, 2, 1, 1), "general", 3),
    ((2, 8, 40, 6, 16, 1, 1, 2, 0, 0), "general", 3),
]


@pytest.mark.parametrize("case,kernel,steps", WGRAD_EDGE_CASES)
def test_wgrad_single_steps_and_predicate_edges(bw, case, kernel, steps):
    J = case[1] * case[5] * case[6]
    wgrad_check(bw, case, kernel, Z=1, per=steps, steps=steps, grid_xy=(-(-J // (256 if kernel == "fast64" else 128)), 1))


@pytest.mark.parametrize("Cout,kernel,gy", [(64, "fast64", 1), (65, "fast128", 1), (128, "fast128", 1), (129, "fast128", 2)])
def test_wgrad_tile_edges_in_cout(bw, Cout, kernel, gy):
    wgrad_check(bw, (19, 8, Cout, 7, 24, 3, 3, 1, 1, 1), kernel, Z=21, per=10, steps=200, grid_xy=(1, gy))


@pytest.mark.parametrize("Cout,kernel", [(40, "fast64"), (72, "fast128")])
@pytest.mark.parametrize("J", [128, 129, 256, 257])
def test_wgrad_tile_edges_in_j(bw, J, Cout, kernel):
    """J = Cin KH KW at the column-tile edges of both fast tiles (1x1 kernel, Cin = J), under the 21-part split."""
    gx = -(-J // 256) if kernel == "fast64" else -(-J // 128)
    wgrad_check(bw, (19, J, Cout, 7, 24, 1, 1, 1, 0, 0), kernel, Z=21, per=10, steps=200, grid_xy=(gx, 1))


@pytest.mark.parametrize("name", ["general-21-parts", "general-stride2-split", "fast64-21-parts", "fast128-odd-parts"])
def test_wgrad_on_channel_slices_under_a_split(bw, name):
    """x and dy are channel slices of wider tensors (batch stride != C H W) and the pixel axis is split: a part that begins
    mid-item must step over the slice's gap to the next item."""
    case, kernel, steps, Z, per = WGRAD_SPLIT_CASES[name]
    wgrad_check(bw, case, kernel, Z=Z, per=per, steps=steps, sliced=True)


# ------------------------------------------------------------------------------------------------ input gradient

DGRAD_CASES = [
    # B, Cin, Cout, H, W, KH, KW, stride, padH, padW, dy is a channel slice
    (2, 24, 40, 7, 20, 1, 3, 1, 0, 1, False),
    (2, 24, 40, 9, 16, 3, 1, 1, 1, 0, False),
    (2, 24, 48, 11, 8, 5, 1, 1, 2, 0, False),
    (2, 16, 32, 6, 16, 2, 3, 1, 0, 1, False),
    (2, 24, 40, 7, 20, 1, 3, 1, 0, 1, True),
    (2, 64, 96, 11, 15, 3, 3, 2, 1, 1, True),        # stride 2, dy a slice
    (2, 64, 96, 10, 14, 3, 3, 2, 1, 1, False),       # (H + 2p - K) % 2 == 1: the dilated buffer ends in a zero row and column
    (2, 64, 96, 10, 14, 1, 1, 2, 0, 0, True),        # the same for the 1x1 downsample, sliced
]


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_conv_dgrad_vs_autograd(bw, case):
    B, Cin, Cout, H, W, KH, KW, s, pH, pW, sliced = case
    g = gen(sum(case[:10]))
    x64 = torch.randn(B, Cin, H, W, generator=g).double().requires_grad_()
    w = torch.randn(Cout, Cin, KH, KW, generator=g) / (Cin * KH * KW) ** 0.5
    y = F.conv2d(x64, w.double(), None, stride=s, padding=(pH, pW))
    DY = torch.randn(B, Cout + (6 if sliced else 0), y.shape[2], y.shape[3], generator=g)
    lo = 4 if sliced else 0
    y.backward(DY[:, lo:lo + Cout].double())
    dx = bw.conv_dgrad(DY.cuda()[:, lo:lo + Cout], w.cuda(), (H, W), stride=s, padding=(pH, pW))
    e = rel(dx, x64.grad)
    print("dgrad", case, "%.2e" % e)
    assert e < TOL, e


@pytest.mark.parametrize("stride,extra", [(2, (0, 0)), (2, (1, 1)), (3, (0, 0)), (3, (2, 1))])
def test_dilate_is_zero_insertion(stride, extra):
    """accflow_dilate_f32 called directly: a sliced source, strides 2 and 3, a destination with trailing zero rows / columns
    (what conv_dgrad allocates when (H + 2p - K) % stride != 0); the destination starts as NaN - the entry zeroes it."""
    from accflow_amd import _lib
    from accflow_amd.ops import _p, _stream
    lib = _lib.load()
    B, C, OH, OW = 3, 5, 7, 11          # 1155 elements: four full blocks and a ragged fifth
    SRC = torch.randn(B, C + 4, OH, OW, generator=gen(31 + stride)).cuda()
    src = SRC[:, 3:3 + C]
    Hd, Wd = (OH - 1) * stride + 1 + extra[0], (OW - 1) * stride + 1 + extra[1]
    dst = torch.full((B, C, Hd, Wd), float("nan"), device="cuda")
    assert lib.accflow_dilate_f32(_p(src), src.stride(0), _p(dst), B, C, OH, OW, Hd, Wd, stride, _stream()) == 0
    want = torch.zeros(B, C, Hd, Wd)
    want[:, :, :(OH - 1) * stride + 1:stride, :(OW - 1) * stride + 1:stride] = src.cpu()
    assert torch.equal(dst.cpu(), want)
    # a destination too small for the last sample is refused
    assert lib.accflow_dilate_f32(_p(src), src.stride(0), _p(dst), B, C, OH, OW, (OH - 1) * stride, Wd, stride, _stream()) == 1


# ------------------------------------------------------------------------------------------------ deformable backward

def deform_operands(H, W, C, seed, collide=0):
    """x as a slice of a wider tensor, offset (18) and mask (9) as slices of one 27-channel tensor.  Offsets randn * 4 (samples
    leave the image), or - collide = n - offsets that pull all nine taps of every pixel onto n source cells.  No sample lies
    on an integer coordinate in fp32 (h = -1 and h = H included): the derivative of the bilinear weights there is a
    convention, and the float64 reference would round the position to the other side."""
    B, Cout = 2, 5
    g = gen(seed)
    X = torch.randn(B, C + 3, H, W, generator=g)
    OM = torch.empty(B, 27, H, W)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    if collide:
        which = torch.randint(0, collide, (B, H, W), generator=g)
        ty = (torch.arange(collide) * 7 % (H - 1)).float() + 0.3        # targets inside the image, fractions .3 / .7
        tx = (torch.arange(collide) * 5 % (W - 1)).float() + 0.7
    else:
        OM[:, :18] = torch.randn(B, 18, H, W, generator=g) * 4
    OM[:, 18:] = torch.rand(B, 9, H, W, generator=g)
    for t in range(9):
        for axis, base in ((0, ys - 1 + t // 3), (1, xs - 1 + t % 3)):
            o = OM[:, 2 * t + axis]
            if collide:
                o.copy_((ty, tx)[axis][which] - base)
            for _ in range(3):
                pos = base + o                                          # fp32, the kernels' own sum
                o[pos == pos.floor()] += 0.37
            assert not bool((base + o == (base + o).floor()).any())
    w = torch.randn(Cout, C, 3, 3, generator=g) / (9 * C) ** 0.5
    b = torch.randn(Cout, generator=g)
    dy = torch.randn(B, Cout, H, W, generator=g)
    return X, OM, w, b, dy


def deform_check(bw, H, W, C, seed, collide=0, need_dx=True):
    from oracle import accflow_oracle as O
    X, OM, w, b, dy = deform_operands(H, W, C, seed, collide)
    t64 = [t.double().requires_grad_() for t in (X[:, 2:2 + C], OM[:, :18], OM[:, 18:], w, b)]
    O.deform_conv2d(*t64).backward(dy.double())
    if collide:     # the case is what it claims: the input gradient lives on a handful of pixels
        assert int((t64[0].grad.abs().sum((0, 1)) > 0).sum()) <= 4 * collide
    Xc, OMc = X.cuda(), OM.cuda()
    got = bw.deform_conv_backward(Xc[:, 2:2 + C], OMc[:, :18], OMc[:, 18:], w.cuda(), dy.cuda(), need_dx=need_dx)
    if not need_dx:
        assert got[0] is None
    errs = {}
    for name, t, want in zip(("dx", "doffset", "dmask", "dweight", "dbias"), got, t64):
        if t is not None:
            errs[name] = rel(t, want.grad)
    print("deform", (H, W, C, collide), {k: "%.2e" % e for k, e in errs.items()})
    assert all(e < TOL for e in errs.values()), errs
    return errs


DEFORM_CASES = [
    # H, W, C: the kernel accflow_deform_conv_backward_f32 picks at H W pixels, channel groups
    (25, 43, 12),      # 1075 px: <8>, groups of 8 + 4
    (41, 50, 6),       # 2050 px: <4>, groups of 4 + 2
    (64, 64, 6),       # 4096 px: <4> with exactly 65536 bytes of LDS (the coarse plane of a 512 x 512 frame)
    (17, 241, 24),     # 4097 px: the global-atomic kernel, groups of 16 + 8
    (32, 32, 20),      # 1024 px: <16> at its upper edge, groups of 16 + 4
    (32, 64, 8),       # 2048 px: <8> at its upper edge, one full group
]


@pytest.mark.parametrize("H,W,C", DEFORM_CASES)
def test_deform_backward_routes(bw, H, W, C):
    """Measured on an MI355X (dx, d offset, d mask, d weight, d bias; largest error over the reference's RMS): all planes
    <= 2.4e-6, 2.3e-6, 1.2e-6, 1.9e-5, 4.2e-7 (d weight runs over the forward's re-formed columns).  17 x 241 is the case that
    found the kernels' position arithmetic wanting: they summed (float)(pixel + tap) + offset, a multiple of 2^-16 px at
    x = 128 .. 256, and d offset was 1.10e-4 of its RMS from float64 (d mask 6.7e-5, dx 4.6e-5; 3.3e-5 at 64 x 64) - the float64
    reference itself moved by those amounts when evaluated at the rounded positions.  They now keep (cell, fraction)
    (deform_cell, csrc/backward.hip)."""
    deform_check(bw, H, W, C, seed=H * W + C)


@pytest.mark.parametrize("H,W,C,cells", [(20, 27, 20, 8), (41, 50, 6, 8), (17, 241, 20, 16)])
def test_deform_backward_colliding_samples(bw, H, W, C, cells):
    """All nine taps of every pixel sample one of `cells` source cells: thousands of LDS (<16>, <4>) or global float atomics
    land on the same four addresses per cell and channel."""
    deform_check(bw, H, W, C, seed=H + W + C, collide=cells)


def test_deform_backward_without_dx(bw):
    deform_check(bw, 25, 43, 12, seed=3, need_dx=False)


# ------------------------------------------------------------------------------------------------ small kernels

@pytest.mark.parametrize("shape", [(1,), (255,), (257,), (2, 2, 9, 7)])
def test_l1_grad_sizes_ties_and_signed_zeros(bw, shape):
    g = gen(41 + len(shape))
    p, t = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    n = p.numel()
    pf, tf = p.view(-1), t.view(-1)
    pf[0::5] = tf[0::5]                         # exact ties (n = 1: its only element)
    pf[3::7], tf[3::7] = 0.0, -0.0              # signed zeros, both ways: a difference of (+-)0
    pf[4::7], tf[4::7] = -0.0, 0.0
    for scale in (1.0 / n, 0.3):
        got = bw.l1_grad(p.cuda(), t.cuda(), scale).cpu()
        assert torch.equal(got, torch.sign(p - t) * torch.tensor(scale, dtype=torch.float32))
        assert got.shape == p.shape
    if n == 1:
        for a, b in ((1.5, 0.5), (0.5, 1.5)):
            got = bw.l1_grad(torch.tensor([a]).cuda(), torch.tensor([b]).cuda(), 0.25).cpu()
            assert torch.equal(got, torch.tensor([0.25 if a > b else -0.25]))


def test_add_on_two_slices(bw):
    """B = 3, C H W = 315 (no multiple of 256), both operands slices; the channels around the destination slice stay."""
    g = gen(43)
    a, b = torch.randn(3, 12, 5, 9, generator=g), torch.randn(3, 10, 5, 9, generator=g)
    A, Bc = a.cuda(), b.cuda()
    out = bw.add_(A[:, 3:10], Bc[:, 2:9])
    a[:, 3:10] += b[:, 2:9]
    assert torch.equal(A.cpu(), a) and torch.equal(Bc.cpu(), b) and out.data_ptr() == A[:, 3:10].data_ptr()


@pytest.mark.parametrize("act", ["relu", "sigmoid", "tanh"])
def test_act_backward_slices_and_saturated_outputs(bw, act):
    """B = 3, C H W = 315, dy / y / dx all slices of wider tensors; relu outputs of exactly 0 and -0.0, sigmoid outputs of
    exactly 0 and 1, tanh outputs of exactly -1 and +1: the gradient there is exactly 0."""
    from accflow_amd import ops
    g = gen(47)
    pre = torch.randn(3, 7, 5, 9, generator=g, dtype=torch.double)
    kind = (torch.arange(pre.numel()) % 11).view(pre.shape)
    for k, v in enumerate((0.0, -0.0, -800.0, 40.0)):    # sigmoid(-800) = 0 and sigmoid(40) = 1 in float64 already; tanh: -1, +1
        pre[kind == k] = v
    pre.requires_grad_()
    y = getattr(torch, act)(pre)
    DY = torch.randn(3, 11, 5, 9, generator=g)
    y.backward(DY[:, 2:9].double())
    y32 = y.detach().float()
    if act == "relu":
        y32[kind == 1] = -0.0                            # (whatever sign relu(-0.0) came out with)
        assert bool(torch.signbit(y32).any()) and bool((y32[kind == 0] == 0).all())
    elif act == "sigmoid":
        assert bool((y32[kind == 2] == 0).all()) and bool((y32[kind == 3] == 1).all())
    Y = torch.randn(3, 13, 5, 9, generator=g)
    Y[:, 4:11] = y32
    code = {"relu": ops.ACT_RELU, "sigmoid": ops.ACT_SIGMOID, "tanh": ops.ACT_TANH}[act]
    OUT = torch.full((3, 9, 5, 9), 7.0).cuda()
    got = bw.act_backward(DY.cuda()[:, 2:9], Y.cuda()[:, 4:11], code, out=OUT[:, 1:8]).cpu()
    e = rel(got, pre.grad)
    print("act", act, "%.2e" % e)
    assert e < TOL_EW, e
    flat_zero = (kind <= 2) if act == "relu" else (kind == 2) | (kind == 3)
    assert torch.equal(got[flat_zero], torch.zeros(int(flat_zero.sum())))
    assert bool((OUT.cpu()[:, 0] == 7.0).all()) and bool((OUT.cpu()[:, 8] == 7.0).all())     # nothing outside the slice


@pytest.mark.parametrize("B,C,H,W", [(2, 1, 5, 7), (3, 2, 3, 5), (2, 2, 19, 27)])
def test_blend_backward_few_channels_and_saturated_mask(bw, B, C, H, W):
    """C = 1 and 2, odd H W (35, 15; 513 pixels per item: more than one block), mask values of exactly 0 and 1."""
    g = gen(53 + C + H)
    f1, f2 = (torch.randn(B, C, H, W, generator=g, dtype=torch.double, requires_grad=True) for _ in range(2))
    m = torch.rand(B, 1, H, W, generator=g, dtype=torch.double)
    m.view(-1)[0::4], m.view(-1)[1::4] = 0.0, 1.0
    m.requires_grad_()
    dy = torch.randn(B, C, H, W, generator=g)
    (f1 * m + (1 - m) * f2).backward(dy.double())
    d1, d2, dm = bw.blend_backward(dy.cuda(), f1.detach().float().cuda(), f2.detach().float().cuda(), m.detach().float().cuda())
    errs = (rel(d1, f1.grad), rel(d2, f2.grad), rel(dm, m.grad))
    print("blend", (B, C, H, W), errs)
    assert max(errs) < TOL_EW, errs
    zero, one = (m.detach() == 0).expand(B, C, H, W), (m.detach() == 1).expand(B, C, H, W)
    assert torch.equal(d1.cpu()[zero], torch.zeros(int(zero.sum()))) and torch.equal(d2.cpu()[one], torch.zeros(int(one.sum())))
    assert torch.equal(d1.cpu()[one], dy[one]) and torch.equal(d2.cpu()[zero], dy[zero])


@pytest.mark.parametrize("B,H8,W8,logits", [(1, 1, 1, "randn"), (1, 1, 5, "randn"), (3, 4, 1, "randn"), (2, 5, 7, "randn"),
                                           (2, 5, 7, "x30"), (1, 2, 3, "equal")])
def test_convex_upsample_backward_shapes_and_logits(bw, B, H8, W8, logits):
    """Single rows / columns / one coarse pixel (every neighbour but the centre is padding), 35 coarse pixels over two items;
    logits scaled by 30 (without the max subtraction exp overflows; the softmax is nearly one-hot) and nine equal logits.
    Measured on an MI355X: d flow <= 1.7e-6; d mask equals the float64 gradient rounded to fp32 in every case.  The x30 case is
    why the kernel keeps softmax, t and d mask in double: in fp32 d mask was 1.32e-5 of its RMS away (torch's fp32 CPU operators
    on the same formula: 1.32e-5 as well) - with near one-hot weights the gradient is heavy-tailed, its largest element 37 x the
    RMS, so 1e-5 of the RMS is two fp32 ulps of it, and s_k (t_k - sum_j s_j t_j) with s_k = 0.999 subtracts two numbers of ~34
    that fp32 holds to 3.8e-6."""
    from oracle import accflow_oracle as O
    g = gen(59 + B + H8 + W8)
    # (fp32 values, so that the kernel and the reference see the SAME flow: with near one-hot weights d mask = s (t - sum s t) is a
    # difference of nearly equal numbers, and a flow rounded for one side only shows there at 2e-5 of the small RMS)
    flow = torch.randn(B, 2, H8, W8, generator=g).double().requires_grad_()
    mask = torch.randn(B, 576, H8, W8, generator=g)
    if logits == "x30":
        mask = mask * 30
        assert float(mask.max()) > 89          # exp(89) overflows fp32
    elif logits == "equal":
        mask = torch.full_like(mask, 0.7)
    mask = mask.double().requires_grad_()
    up = O.convex_upsample(flow, mask)
    dup = torch.randn(up.shape, generator=g)
    up.backward(dup.double())
    dflow, dmask = bw.convex_upsample_backward(dup.cuda(), flow.detach().float().cuda(), mask.detach().float().cuda())
    errs = (rel(dflow, flow.grad), rel(dmask, mask.grad))
    print("convex upsample", (B, H8, W8, logits), errs)
    assert max(errs) < TOL_EW, errs
