"""RAFT-small on the GPU: the radius-3 lookup and upflow8 kernels, the bottleneck encoders, the ConvGRU update block, the
estimator end to end and AccFlow on top of it.

References.
  * tests/golden/raft_small_c1*.npz: what the reference's RAFT(small=True) computes on the CPU for the project's seeded
    weights and frames at 128 x 192 (1/8 grid 16 x 24) and 136 x 200 (17 x 25: odd level sizes, partial 64-pixel
    workgroups) - tests/golden/make_raft_small_golden.py.
  * `lookup_restated`: the reference's CorrBlock.__call__ (grid_sample, align_corners, zero padding) in float64.
  * float64 F.interpolate for upflow8.

Tolerances.
  * lookup: 2e-5 (+ 1e-4 relative), what test_hip_parity.test_corr_lookup allows the same arithmetic at radius 4.
  * the radius-4 lookup: the kernel became a template on the radius; its radius-4 instantiation must still return the bits of
    the stand-alone radius-4 kernel of the displaced layout (csrc/corr_disp.hip, untouched: the same fma chain, documented to
    return identical bits) - `torch.equal`.
  * upflow8: 4 * 2^-23 * 8 * max|flow| - the kernel takes the interpolation fraction from an integer remainder (one rounding),
    forms four weights (two roundings each) and sums one product and three fused multiply-adds; the factor 8 is exact.
  * encoders 3e-4 and update block 1e-4: the gates of test_encoders_vs_golden / test_update_block_vs_golden.
  * estimator: mean EPE <= 1e-3 px (the project's gate); max EPE <= 4 x the largest value measured on the MI355X (MAX_EPE,
    the margin of the existing C1 test for box-to-box spread).  The fixture's own floor is not zero: the reference's fp32 CPU
    output at 128 x 192 and 12 iterations moves by 8.5e-5 px (max) between 1 and 8 host threads.
  * batching: 1e-4, as test_estimator_c1_vs_golden_and_oracle.
  * AccFlow: mean EPE <= 1e-3, max <= 5e-4, the step API's 1/8 output 2e-4 (+ 1e-3 relative): test_accflow_c1_vs_golden.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import accflow_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy
GRIDS = [(16, 24), (17, 25)]
FILES = {(16, 24): "raft_small_c1", (17, 25): "raft_small_c1_ragged"}
# largest max EPE (px) against the fixtures measured on the MI355X, per fixture, over iters 1 / 4 / 12 / flow_init and both modes
# (both at 12 iterations in f16x3; bf16x6: 1.720e-4 / 1.430e-4; iters 1: 1.6e-5, iters 4: 5.5e-5, flow_init: 5.4e-5)
MAX_EPE = {"raft_small_c1": 1.725e-4, "raft_small_c1_ragged": 1.459e-4}


def dev(t):
    return t.cuda()


def maxerr(a, b):
    return float((a.detach().cpu() - b.detach().cpu()).abs().max())


def check(a, b, atol, rtol=1e-4, what=""):
    a, b = a.detach().cpu(), b.detach().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    print("%s: max err %.3e" % (what, float(err.max())))
    assert bool((err <= tol).all()), "%s: max err %.3e, tol %.1e+%.0e*|ref|" % (what, float(err.max()), atol, rtol)


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """A device error poisons the process: nothing more is started on the GPU after one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, session stopped: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def small(ops):
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks.raft.raft import RAFT, small_args
    m = RAFT(small_args())
    m.load_state_dict(make_state_dict(m), strict=True)
    return m.cuda().eval()


def frames(seed, n, H, W):
    from accflow_amd.data.synthetic import make_sequence, normalize
    return [normalize(f) for f in make_sequence(seed, n, H, W)]


def pair(seed, H, W):
    fr = frames(seed, 2, H, W)
    return fr[1], fr[0]


# ------------------------------------------------------------------------------------------------ lookup
def sample_points(coords, r, level):
    """(B h w, 2r+1, 2r+1, 2) positions (x, y) the reference samples in pyramid level `level` (corr.py:30-38)."""
    B, _, h, w = coords.shape
    c = coords.double().permute(0, 2, 3, 1).reshape(B * h * w, 1, 1, 2)
    d = torch.linspace(-r, r, 2 * r + 1, dtype=torch.float64)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, 2 * r + 1, 2 * r + 1, 2)
    return c / 2 ** level + delta


def sample_zeros(plane, at):
    """bilinear_sampler (utils.py:66-80): grid_sample, align_corners, zero padding - in float64."""
    hl, wl = plane.shape[-2:]
    grid = torch.stack([2 * at[..., 0] / (wl - 1) - 1, 2 * at[..., 1] / (hl - 1) - 1], dim=-1)
    return F.grid_sample(plane.double(), grid, align_corners=True)


def as_lookup(per_level, coords):
    B, _, h, w = coords.shape
    return torch.cat([v.view(B, h, w, -1) for v in per_level], dim=-1).permute(0, 3, 1, 2).contiguous()


def lookup_restated(pyr, coords, r):
    """CorrBlock.__call__ of the reference (corr.py:24-45) in float64."""
    return as_lookup([sample_zeros(lvl, sample_points(coords, r, l)) for l, lvl in enumerate(pyr)], coords)


def fixture_position_bound(pyr, coords, r):
    """What a stored fp32 lookup of the reference may be off by because of ITS sampling positions: bilinear_sampler maps a
    position to [-1, 1] and grid_sample maps it back, five fp32 roundings (multiply, divide, subtract; add, multiply) of
    numbers up to |x| / ((W-1)/2) + 2, i.e. a position error of up to dx = 5 * 2^-24 * (|x| + W) pixels (dy alike).  A bilinear
    sample moves by at most |v01 - v00| + ... <= 2 max|tap| per pixel of position error along each axis, and the taps in reach
    are bounded by the 3 x 3 maximum of |level| around the four corners - sampled on the level padded by one cell, so that a
    position exactly on the frame's outside border (weight exactly 0 in exact arithmetic) sees the cell it may leak from."""
    out = []
    for l, lvl in enumerate(pyr):
        hl, wl = lvl.shape[-2:]
        at = sample_points(coords, r, l)
        reach = F.max_pool2d(F.pad(lvl.double().abs(), (2, 2, 2, 2)), 3, stride=1)        # (N, 1, hl + 2, wl + 2)
        taps = sample_zeros(reach, at + 1.0)
        dx = 5 * 2.0 ** -24 * (at[..., 0].abs() + wl)
        dy = 5 * 2.0 ** -24 * (at[..., 1].abs() + hl)
        out.append(2 * (dx + dy).unsqueeze(1) * taps)
    return as_lookup(out, coords)


@pytest.fixture(scope="module")
def lookup_inputs():
    """Per grid: a random row-major pyramid of B = 2 and coordinates around the identity, some well outside the frame, some
    exact integers and borders."""
    made = {}
    for h, w in GRIDS:
        g = torch.Generator().manual_seed(31 + h)
        B, P = 2, h * w
        pyr = [torch.randn(B * P, 1, h >> l, w >> l, generator=g) for l in range(4)]
        coords = O.coords_grid(B, h, w) + 5.0 * torch.randn(B, 2, h, w, generator=g)
        coords[0, :, 0, :4] = torch.tensor([[-30.0, -3.5, 1e5, float(w) + 2.25], [2.0, -9.0, 3.0, float(h) - 0.5]])
        coords[0, :, 1, :3] = torch.tensor([[4.0, float(w - 1), 0.0], [0.0, float(h - 1), -1.0]])
        coords[1, :, 2, :3] = torch.tensor([[-4000.0, 300.0, float(w) + 40.0], [-250.0, 7e4, float(h) + 40.0]])
        made[(h, w)] = (pyr, coords, lookup_restated(pyr, coords, 3).float())
    return made


@pytest.mark.parametrize("grid", GRIDS)
def test_lookup_r3_vs_float64_restatement(ops, lookup_inputs, grid):
    pyr, coords, want = lookup_inputs[grid]
    h, w = grid
    assert tuple(want.shape) == (2, 196, h, w)
    dp = [dev(p) for p in pyr]
    got = ops.corr_lookup(dp, dev(coords), radius=3)
    assert tuple(got.shape) == (2, 196, h, w)
    check(got, want, 2e-5, what="lookup r3 %dx%d" % grid)
    # a channel-slice destination (the batch stride of the larger buffer), the channels around it untouched
    big = torch.full((2, 196 + 24, h, w), 7.0, device="cuda")
    assert ops.corr_lookup(dp, dev(coords), out=big[:, 8:204], radius=3).data_ptr() == big[:, 8:204].data_ptr()
    assert torch.equal(big[:, 8:204], got) and bool((big[:, :8] == 7.0).all()) and bool((big[:, 204:] == 7.0).all())
    with pytest.raises(RuntimeError):
        ops.corr_lookup(dp, dev(coords), out=big[:, :195], radius=3)
    with pytest.raises(NotImplementedError):
        ops.corr_lookup(dp, dev(coords), radius=2)


@pytest.mark.parametrize("grid", GRIDS)
def test_lookup_r4_bits_unchanged(ops, lookup_inputs, grid):
    """The templated kernel's radius-4 instantiation against the stand-alone radius-4 kernel of the displaced layout on the
    same pyramid and coordinates: bit for bit (and against float64, as before)."""
    pyr, coords, _ = lookup_inputs[grid]
    h, w = grid
    dp = [dev(p) for p in pyr]
    got = ops.corr_lookup(dp, dev(coords))
    assert tuple(got.shape) == (2, 324, h, w)
    assert ops.corr_disp_supported(h, w)
    alone = ops.corr_lookup(ops.DispPyramid.from_rowmajor(dp, 2, h, w), dev(coords))
    assert torch.equal(got, alone)
    check(got, lookup_restated(pyr, coords, 4).float(), 2e-5, what="lookup r4 %dx%d" % grid)


@pytest.mark.parametrize("grid", GRIDS)
def test_lookup_r3_vs_golden(ops, golden, grid):
    """The reference's own lookup values: its pyramid is restated in float64 from the stored feature maps (corr.py:47-55 and
    the three avg_pool2d levels), so that only the lookup kernel stands between the fixture and the result.

    The fixture's pyramid is an fp32 matrix product, and that is the fixture's own error: each entry sums C = 128 products,
    whose rounding errors add up to about sqrt(C) 2^-24 sum_c |f1_c f2_c| / sqrt(C) (the probabilistic bound of a length-C fp32
    dot product) - little against a large correlation, but not against one whose terms cancel.  The lookup is a convex
    combination of entries, so the same lookup of the pyramid of sum_c |f1_c| |f2_c| / sqrt(C) bounds the error it inherits;
    that is added to the kernel's 2e-5 (+ 1e-4 relative), and so is fixture_position_bound.  (First written without the two:
    9.5e-5 at lookup0, where the kernel copies entries or writes zeros - the reference's fp32 round trip of an integer
    position just outside the frame had leaked 1e-6 of the border cell into a tap that is exactly 0.)"""
    g = golden(FILES[grid])
    f1, f2 = T(g["fmap1"]).double(), T(g["fmap2"]).double()
    B, C, h, w = f1.shape
    assert (h, w) == grid

    def pyramid(a, b):
        lvl = (torch.matmul(a.view(B, C, h * w).transpose(1, 2), b.view(B, C, h * w)) / np.sqrt(C)).view(B * h * w, 1, h, w)
        pyr = [lvl]
        for _ in range(3):
            pyr.append(F.avg_pool2d(pyr[-1], 2, stride=2))
        return pyr

    exact = pyramid(f1, f2)
    dp = [dev(p.float()) for p in exact]
    mass = pyramid(f1.abs(), f2.abs())
    sel = T(g["lookup_sel"])
    pick = lambda t: t.cpu().reshape(B, 196, h * w)[:, :, sel]

    def check_golden(coords, want, what):
        got = pick(ops.corr_lookup(dp, dev(coords), radius=3))
        inherited = pick(lookup_restated(mass, coords, 3)) * np.sqrt(C) * 2.0 ** -24 + pick(fixture_position_bound(exact, coords, 3))
        err = (got - want).abs()
        tol = 2e-5 + 1e-4 * want.abs() + inherited.float()
        print("%s: max err %.3e, largest err / tol %.3f (inherited bound up to %.3e)"
              % (what, float(err.max()), float((err / tol).max()), float(inherited.max())))
        assert bool((err <= tol).all()), what

    if "lookup0_sel" in g:
        check_golden(O.coords_grid(B, h, w), T(g["lookup0_sel"]), "golden lookup0")
        want_r = pick(T(golden(FILES[grid] + "_ub")["lookup_r"]))
    else:
        want_r = T(g["lookup_r_sel"])
    check_golden(T(g["coords_r"]), want_r, "golden lookup_r %dx%d" % grid)


def test_corr_block_radius3(ops, golden):
    """CorrBlock(radius=3): the row-major pyramid whatever the layout switch says, no pre-split lookup; against the golden
    lookup through the project's own correlation volume (1e-4, the gate of test_corr_lookup_golden)."""
    from accflow_amd.networks.raft.corr import CorrBlock
    g = golden("raft_small_c1_ragged")
    cb = CorrBlock(dev(T(g["fmap1"])), dev(T(g["fmap2"])), radius=3)
    assert cb.radius == 3 and not cb.supports_s16() and isinstance(cb.corr_pyramid, list)
    out = cb(dev(T(g["coords_r"])))
    B, _, h, w = out.shape
    check(out.cpu().reshape(B, 196, h * w)[:, :, T(g["lookup_sel"])], T(g["lookup_r_sel"]), 1e-4, what="CorrBlock r3 vs golden")


# ------------------------------------------------------------------------------------------------ upflow8
@pytest.mark.parametrize("grid", GRIDS)
def test_upflow8_vs_float64(ops, grid):
    h, w = grid
    g = torch.Generator().manual_seed(5 + w)
    flow = torch.randn(3, 2, h, w, generator=g) * 4
    flow[1] = 30.0 * F.interpolate(torch.randn(1, 2, 3, 4, generator=g), size=(h, w), mode="bilinear", align_corners=True)[0]
    want = 8 * F.interpolate(flow.double(), size=(8 * h, 8 * w), mode="bilinear", align_corners=True)
    tol = 4 * 2.0 ** -23 * 8 * float(flow.abs().max())
    got = ops.upflow8(dev(flow))
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 2, 8 * h, 8 * w)
    err = float((got.cpu().double() - want).abs().max())
    print("upflow8 %dx%d: max err %.3e, tolerance %.3e" % (h, w, err, tol))
    assert err <= tol
    # a batch-slice output (the pair groups write into slices of one tensor) and a channel-slice input
    whole = torch.full((5, 2, 8 * h, 8 * w), -3.0, device="cuda")
    wide = torch.zeros(3, 6, h, w, device="cuda")
    wide[:, 2:4] = dev(flow)
    assert ops.upflow8(wide[:, 2:4], out=whole[1:4]).data_ptr() == whole[1:4].data_ptr()
    assert torch.equal(whole[1:4], got) and bool((whole[0] == -3.0).all()) and bool((whole[4] == -3.0).all())
    with pytest.raises(RuntimeError):
        ops.upflow8(dev(flow), out=whole[:2])


def test_upflow8_vs_golden(ops, golden):
    g = golden("raft_small_c1")
    flow = T(g["up_flow"])
    _, _, h, w = flow.shape
    tol = 4 * 2.0 ** -23 * 8 * float(flow.abs().max())
    # The fixture is the reference's fp32 F.interpolate, which forms the source position as the fp32 product scale * index:
    # two roundings, an error of up to 2^-23 (h - 1) rows / 2^-23 (w - 1) columns, which the interpolation multiplies by the
    # difference of two neighbouring cells (and upflow8 by 8).  That is the fixture's own error, added to the kernel's bound.
    step = max(float((flow[..., 1:, :] - flow[..., :-1, :]).abs().max()), float((flow[..., :, 1:] - flow[..., :, :-1]).abs().max()))
    ref_err = 8 * 2.0 ** -23 * (h + w) * step
    err = maxerr(ops.upflow8(dev(flow))[:, :, ::2, ::2], T(g["upflow8"]))
    print("upflow8 vs golden: max err %.3e, kernel bound %.3e + fixture bound %.3e" % (err, tol, ref_err))
    assert err <= tol + ref_err


# ------------------------------------------------------------------------------------------------ modules
@pytest.mark.parametrize("grid", GRIDS)
def test_small_encoders_vs_golden(ops, golden, small, grid):
    g = golden(FILES[grid])
    i1, i2 = pair(int(g["seed"]), int(g["H"]), int(g["W"]))
    f1, f2 = small.fnet([dev(i1), dev(i2)])
    assert f1._base is not None and f1._base.shape[0] == 2          # frame-major views of one tensor (encode_frames)
    check(f1, T(g["fmap1"]), 3e-4, what="small fnet fmap1 %dx%d" % grid)
    check(f2, T(g["fmap2"]), 3e-4, what="small fnet fmap2 %dx%d" % grid)
    cnet = small.cnet(dev(i1))
    if grid == (16, 24):
        check(cnet, T(golden("raft_small_c1_ub")["cnet"]), 3e-4, what="small cnet")
    else:
        check(cnet[:, ::4], T(g["cnet_s4"]), 3e-4, what="small cnet (ragged)")
    with ops.conv_mode(ops.CONV_BF16X6):
        check(small.fnet([dev(i1), dev(i2)])[1], T(g["fmap2"]), 3e-4, what="small fnet fmap2 bf16x6 %dx%d" % grid)


def test_small_update_block_vs_golden(ops, golden, small):
    g = golden("raft_small_c1_ub")
    cnet = T(g["cnet"])
    net, inp = torch.tanh(cnet[:, :96]), torch.relu(cnet[:, 96:])
    B, _, h, w = cnet.shape
    flow = T(g["coords_r"]) - O.coords_grid(B, h, w)
    for mode in (ops.CONV_F16X3, ops.CONV_BF16X6):
        with ops.conv_mode(mode):
            net1, mask1, delta1 = small.update_block(dev(net), dev(inp), dev(T(g["lookup_r"])), dev(flow))
        assert mask1 is None
        check(net1, T(g["ub_net"]), 1e-4, what="small update block net (mode %d)" % mode)
        check(delta1, T(g["ub_delta"]), 1e-4, what="small update block delta (mode %d)" % mode)


# ------------------------------------------------------------------------------------------------ estimator
@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("grid", GRIDS)
def test_small_estimator_vs_golden(ops, golden, small, grid, mode):
    name = FILES[grid]
    g = golden(name)
    i1, i2 = pair(int(g["seed"]), int(g["H"]), int(g["W"]))
    measured = MAX_EPE[name]
    with ops.conv_mode(mode):
        for it in (1, 4, 12):
            out = small(dev(i1), dev(i2), iters=it).cpu()
            assert tuple(out.shape) == (1, 2, int(g["H"]), int(g["W"]))
            me, mx = O.epe(out if it == 12 else out[:, :, ::2, ::2], T(g["flow_it%d" % it]))
            print("%s %s iters %d: mean EPE %.3e max EPE %.3e" % (name, mode, it, me, mx))
            assert me <= 1e-3 and mx <= 4 * measured, (name, mode, it, me, mx, "measured max %.2e" % measured)
        out = small(dev(i1), dev(i2), iters=4, flow_init=dev(T(g["flow_init"]))).cpu()
        me, mx = O.epe(out[:, :, ::2, ::2], T(g["flow_it4_init"]))
        print("%s %s flow_init: mean EPE %.3e max EPE %.3e" % (name, mode, me, mx))
        assert me <= 1e-3 and mx <= 4 * measured, (name, mode, "flow_init", me, mx, "measured max %.2e" % measured)
    print("stages re-run in bf16x6 by the range guard:", ops.guard_report())


def test_small_batch_of_two_pairs_equals_single_calls(ops, small):
    i1, i2 = pair(1000, 136, 200)
    j1, j2 = pair(1001, 136, 200)
    both = small(dev(torch.cat([i1, j1])), dev(torch.cat([i2, j2])), iters=4).cpu()
    assert maxerr(both[:1], small(dev(i1), dev(i2), iters=4)) <= 1e-4
    assert maxerr(both[1:], small(dev(j1), dev(j2), iters=4)) <= 1e-4


def test_small_estimate_pairs_equals_per_pair_forward(ops, small):
    """Three frames, four pairs (two pair groups on their streams): every frame encoded once, against one forward per pair;
    with flow_init, reused features and return_low; and the warm-started video loop on top."""
    fr = [dev(f) for f in frames(1000, 3, 128, 192)]
    pairs = [(1, 0), (2, 1), (2, 0), (0, 2)]
    feats = {}
    up, low = small.estimate_pairs(fr, pairs, iters=4, features=feats, return_low=True)
    assert tuple(up.shape) == (4, 2, 128, 192) and tuple(low.shape) == (4, 2, 16, 24)
    assert sorted(feats["fmap"]) == [0, 1, 2] and feats["fmap"][0].shape[1] == 128
    for k, (i, j) in enumerate(pairs):
        assert maxerr(up[k:k + 1], small(fr[i], fr[j], iters=4)) <= 1e-4, (i, j)
    assert torch.equal(ops.upflow8(low.contiguous()), up)
    g = torch.Generator().manual_seed(3)
    fi = dev(0.5 * torch.randn(4, 2, 16, 24, generator=g))
    seeded = small.estimate_pairs(fr, pairs, iters=3, flow_init=fi, features=feats)
    for k, (i, j) in enumerate(pairs):
        assert maxerr(seeded[k:k + 1], small(fr[i], fr[j], iters=3, flow_init=fi[k:k + 1])) <= 1e-4, (i, j)
    vup, vlow = small.estimate_video(fr, iters=(4, 2))
    assert tuple(vup.shape) == (2, 2, 128, 192) and tuple(vlow.shape) == (2, 2, 16, 24)
    assert maxerr(vup[:1], small(fr[0], fr[1], iters=4)) <= 1e-4
    seed = ops.forward_interpolate(vlow[:1].contiguous())
    assert maxerr(vup[1:], small(fr[1], fr[2], iters=2, flow_init=seed)) <= 1e-4
    cold_up, _ = small.estimate_video(fr, iters=4, warm_start=False)
    assert maxerr(cold_up[1:], small(fr[1], fr[2], iters=4)) <= 1e-4


def test_accflow_on_raft_small_vs_golden(ops, golden):
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks.AccFlow_ import AccFlow
    from accflow_amd.networks.raft.raft import RAFT, small_args
    g = golden("raft_small_c1")
    model = AccFlow(RAFT(small_args()))
    model.load_state_dict(make_state_dict(model), strict=True)
    model = model.cuda().eval()
    n = int(g["acc_n_frames"])
    fr = [dev(f) for f in frames(int(g["seed"]), n, int(g["H"]), int(g["W"]))]
    outs = model(images=fr, test_mode=False)
    assert len(outs) == n - 2
    for k, o in enumerate(outs):
        me, mx = O.epe(o.cpu()[:, :, ::2, ::2], T(g["acc_out%d" % k]))
        print("AccFlow(RAFT-small) out %d: mean EPE %.3e max EPE %.3e" % (k, me, mx))
        assert me <= 1e-3 and mx <= 5e-4, ("accflow(raft-small) out", k, me, mx)
    out_small, up = model.iter(fr[2], fr[1], fr[0], None)
    check(out_small, T(g["acc_s2_out_small"]), 2e-4, rtol=1e-3, what="AccFlow(RAFT-small) iter out_small")
    me, mx = O.epe(up.cpu()[:, :, ::2, ::2], T(g["acc_out0"]))
    assert me <= 1e-3, ("iter", me, mx)
    warm = model.forward_warm(fr)
    assert len(warm) == n - 2 and tuple(warm[0].shape) == tuple(outs[0].shape) and bool(torch.isfinite(warm[0]).all())
    # (another schedule of the same estimate - a composed seed and fewer iterations for the long pair: not comparable to a
    # tolerance, the figure is printed)
    print("AccFlow(RAFT-small) forward_warm vs forward: mean / max EPE %.3e / %.3e" % O.epe(warm[0].cpu(), outs[0].cpu()))
