"""Resampling at the frame / flow-file boundary on the GPU: ops.frames_from_u8(size=, interp=), ops.flow_resize,
frames.FrameScaler, infer.run's size options and eval_hs_sintel.run (csrc/frame_io.hip).

Bounds, from the arithmetic and not from what the kernels give: a bilinear result goes through three lerps
(f == 0 ? a : a + f (b - a)), each at most four fp32 roundings of half an ulp at magnitude <= 256 (2^-17), so 12 * 2^-17 ~
9.2e-5: 1e-4 in levels and 1e-6 on the normalised output (x 2/255, plus the division's rounding) against float64
F.interpolate(align_corners=False).  For flows the same count is relative: 2^-19 of the largest magnitude among an output's
four taps, times the scale factor.  Everything else here is bit equality: the padding against F.pad(mode="replicate") of the
same call's unpadded result, an exact 2x reduction against the 2 x 2 mean, a same-size resize against today's kernels, area
against float32(sum) / float32(count) over integer windows, the file codings against the same call's "nchw" result.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frame_io_ref as R
import frame_resize_ref as Z

pytestmark = pytest.mark.gpu


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


def same_bits(got, want):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    return torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


def on_device(hwc, layout):
    return (hwc if layout == "hwc" else hwc.permute(0, 3, 1, 2)).contiguous().cuda()


def case_id(case):
    (N, H, W), (h, w) = case
    return "%dx%dx%d-%dx%d" % (N, H, W, h, w)


# ------------------------------------------------------------------------------------------------
# ingest


@pytest.mark.parametrize("case", Z.BILINEAR_CASES, ids=case_id)
def test_bilinear_ingest_against_float64(ops, case):
    (N, H, W), size = case
    # (random bytes all over - the ramp that ingest_bytes starts with is linear in x and y, and a lerp of it is exact - with
    # the largest step, 0 next to 255, in the first pixels)
    hwc = torch.randint(0, 256, (N, H, W, 3), generator=torch.Generator().manual_seed(H * 100 + W), dtype=torch.uint8)
    hwc[:, 0, 0], hwc[:, 0, -1], hwc[:, -1, 0] = 0, 255, 255
    for bgr in (False, True):
        ref = Z.bilinear_f64(Z.levels(hwc, bgr), size)
        ref_n = 2 * (ref / 255.0) - 1
        for layout in ("hwc", "chw"):
            dev = on_device(hwc, layout)
            plain = ops.frames_from_u8(dev, layout=layout, bgr=bgr, normalize=False, size=size)
            norm = ops.frames_from_u8(dev, layout=layout, bgr=bgr, size=size)
            assert plain.shape == norm.shape == (N, 3) + tuple(size) and plain.dtype == norm.dtype == torch.float32
            e, en = float((plain.cpu().double() - ref).abs().max()), float((norm.cpu().double() - ref_n).abs().max())
            print("%s %s bgr=%d: %.3g levels, %.3g normalised" % (case_id(case), layout, bgr, e, en))
            assert e <= 1e-4 and en <= 1e-6, (layout, bgr, e, en)
            for pad in Z.PADS[1:]:
                for normalize, unpadded in ((False, plain), (True, norm)):
                    got = ops.frames_from_u8(dev, layout=layout, bgr=bgr, pad=pad, normalize=normalize, size=size)
                    assert same_bits(got, F.pad(unpadded.cpu(), list(pad), mode="replicate")), (layout, bgr, pad, normalize)


def test_exact_halving_is_the_box_mean(ops):
    hwc = R.ingest_bytes(1, 16, 32, seed=11)
    for bgr in (False, True):
        x = Z.levels(hwc, bgr).float()
        box = x.reshape(1, 3, 8, 2, 16, 2).sum(dim=(3, 5)) / 4.0            # (sums below 1024 and a division by 4: exact)
        for layout in ("hwc", "chw"):
            dev = on_device(hwc, layout)
            for interp in ("bilinear", "area"):
                assert same_bits(ops.frames_from_u8(dev, layout=layout, bgr=bgr, normalize=False, size=(8, 16), interp=interp), box)
                assert same_bits(ops.frames_from_u8(dev, layout=layout, bgr=bgr, size=(8, 16), interp=interp), 2 * (box / 255.0) - 1)


@pytest.mark.parametrize("shape", R.INGEST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_same_size_is_todays_ingest(ops, shape):
    N, H, W = shape
    hwc = R.ingest_bytes(N, H, W, seed=H * 100 + W)
    for layout in ("hwc", "chw"):
        dev = on_device(hwc, layout)
        for bgr in (False, True):
            for normalize in (False, True):
                for pad in Z.PADS:
                    want = ops.frames_from_u8(dev, layout=layout, bgr=bgr, pad=pad, normalize=normalize)
                    assert same_bits(want, R.ingest_reference(hwc, pad, bgr=bgr, normalize=normalize))
                    for interp in ("bilinear", "area"):
                        got = ops.frames_from_u8(dev, layout=layout, bgr=bgr, pad=pad, normalize=normalize, size=(H, W), interp=interp)
                        assert same_bits(got, want), (layout, bgr, normalize, pad, interp)


def test_all_256_codes_through_an_identity_resize(ops):
    hwc = R.all_codes_frame()
    for layout in ("hwc", "chw"):
        for bgr in (False, True):
            want = R.ingest_reference(hwc, (0, 0, 0, 0), bgr=bgr)
            assert same_bits(ops.frames_from_u8(on_device(hwc, layout), layout=layout, bgr=bgr, size=(8, 32)), want), (layout, bgr)


@pytest.mark.parametrize("case", Z.AREA_CASES, ids=case_id)
def test_area_ingest_bitwise(ops, case):
    (N, H, W), size = case
    hwc = R.ingest_bytes(N, H, W, seed=H * 100 + W + 1)
    for bgr in (False, True):
        for normalize in (False, True):
            want = Z.area_reference(hwc, size, bgr=bgr, normalize=normalize)
            for layout in ("hwc", "chw"):
                dev = on_device(hwc, layout)
                got = ops.frames_from_u8(dev, layout=layout, bgr=bgr, normalize=normalize, size=size, interp="area")
                assert same_bits(got, want), (layout, bgr, normalize)
                padded = ops.frames_from_u8(dev, layout=layout, bgr=bgr, pad=Z.PADS[1], normalize=normalize, size=size, interp="area")
                assert same_bits(padded, F.pad(want, list(Z.PADS[1]), mode="replicate")), (layout, bgr, normalize)
    # torch's own area mode, to its float32 rounding: the windows are the same
    torch_area = F.interpolate(Z.levels(hwc).float(), size=size, mode="area")
    assert torch.allclose(Z.area_reference(hwc, size, normalize=False), torch_area, rtol=0, atol=1e-4)


@pytest.mark.parametrize("interp", ["bilinear", "area"])
def test_layouts_give_the_dense_tensors_bits(ops, interp):
    """A pitched view (row stride > 3 W), a base 1 and 2 bytes off a dword, a sliced batch."""
    N, H, W, size, pad = 3, 13, 19, (8, 12), (1, 2, 3, 4)
    hwc = R.ingest_bytes(N, H, W, seed=4)
    for layout in ("hwc", "chw"):
        src = on_device(hwc, layout)
        assert src.data_ptr() % 4 == 0
        want = ops.frames_from_u8(src, layout=layout, pad=pad, size=size, interp=interp)
        pitch = 3 * W + 5
        if layout == "hwc":
            pitched = torch.zeros((N, H, pitch), dtype=torch.uint8, device="cuda")[:, :, :3 * W].unflatten(2, (W, 3))
            assert pitched.stride(1) == pitch > 3 * W
        else:
            pitched = torch.zeros((N, 3, H, pitch), dtype=torch.uint8, device="cuda")[..., :W]
            assert pitched.stride(2) == pitch > W
        pitched.copy_(src)
        assert same_bits(ops.frames_from_u8(pitched, layout=layout, pad=pad, size=size, interp=interp), want), (layout, "pitched")
        for off in (1, 2):
            flat = torch.zeros(src.numel() + off, dtype=torch.uint8, device="cuda")
            shifted = flat[off:].view(src.shape)
            shifted.copy_(src)
            assert shifted.data_ptr() % 4 == off
            assert same_bits(ops.frames_from_u8(shifted, layout=layout, pad=pad, size=size, interp=interp), want), (layout, off)
        assert same_bits(ops.frames_from_u8(src[::2], layout=layout, pad=pad, size=size, interp=interp), want[::2]), layout
        assert same_bits(ops.frames_from_u8(src[1:2], layout=layout, pad=pad, size=size, interp=interp), want[1:2]), layout
        big = torch.full((N, 5, 8 + 7, 12 + 3), 7.0, device="cuda")
        out = big[:, 1:4]
        assert ops.frames_from_u8(src, layout=layout, pad=pad, size=size, interp=interp, out=out).data_ptr() == out.data_ptr()
        assert same_bits(out, want) and (big[:, 0] == 7).all() and (big[:, 4] == 7).all()


# ------------------------------------------------------------------------------------------------
# flow


def check_flow_resize(ops, flow, crop, size):
    """"nchw" against float64 within the 2^-19 bound; "f32" and "u16" against the same call's "nchw" result, bit for bit."""
    y0, x0, Hc, Wc = crop
    H, W = size
    N = flow.shape[0]
    dev = flow.cuda()
    got = ops.flow_resize(dev, size, crop=crop)
    assert got.shape == (N, 2, H, W) and got.dtype == torch.float32
    win = flow[:, :, y0:y0 + Hc, x0:x0 + Wc]
    factor = torch.tensor([W / Wc, H / Hc], dtype=torch.float64).view(1, 2, 1, 1)
    ref = Z.bilinear_f64(win, size) * factor
    bound = Z.tap_bound(win, size) * factor * 2.0 ** -19
    err = (got.cpu().double() - ref).abs()
    print("flow %s of %s -> %s: worst error / bound %.3g" % (crop, tuple(flow.shape), size, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    host = got.cpu()
    assert same_bits(ops.flow_resize(dev, size, crop=crop, coding="f32"), host.permute(0, 2, 3, 1).contiguous())
    for scale in (64.0, 128.0):
        for be in (False, True):
            codes = ops.flow_resize(dev, size, crop=crop, coding="u16", scale=scale, big_endian=be)
            assert codes.dtype == torch.uint16 and codes.shape == (N, H, W, 3)
            assert np.array_equal(codes.cpu().numpy(), R.u16_reference(host.numpy(), (0, 0, H, W), scale, be)), (scale, be)
    return got


def test_flow_resize_against_float64(ops):
    g = torch.Generator().manual_seed(21)
    check_flow_resize(ops, 40 * torch.randn(2, 2, 24, 32, generator=g), (3, 2, 13, 19), (26, 38))
    check_flow_resize(ops, 40 * torch.randn(1, 2, 8, 12, generator=g), (0, 0, 8, 12), (5, 7))
    # a window that touches the padding on every side, and the padding holds 1e30: the result must not see it
    flow = torch.full((1, 2, 16, 24), 1e30)
    flow[:, :, 2:14, 3:21] = 40 * torch.randn(1, 2, 12, 18, generator=g)
    got = check_flow_resize(ops, flow, (2, 3, 12, 18), (24, 35))
    assert float(got.abs().max()) < 1e4
    got = check_flow_resize(ops, flow, (2, 3, 12, 18), (7, 10))
    assert float(got.abs().max()) < 1e4
    # a batch slice as the source and a slice as the destination
    flow = 40 * torch.randn(4, 2, 10, 14, generator=g)
    dev = flow.cuda()
    want = ops.flow_resize(dev, (15, 9), crop=(1, 2, 8, 11))
    assert torch.equal(ops.flow_resize(dev[::2], (15, 9), crop=(1, 2, 8, 11)), want[::2])
    big = torch.zeros((4, 3, 15, 9), device="cuda")
    out = big[:, :2]
    assert ops.flow_resize(dev, (15, 9), crop=(1, 2, 8, 11), out=out).data_ptr() == out.data_ptr()
    assert torch.equal(out, want) and (big[:, 2] == 0).all()


def planted_flow(N, Hp, Wp, crop, seed):
    """40 randn with +-600 (codes 0 and 65535 at both scales), NaN and +-inf planted inside the crop window."""
    g = torch.Generator().manual_seed(seed)
    flow = 40 * torch.randn(N, 2, Hp, Wp, generator=g)
    y0, x0, H, W = crop
    spots = [(y0, x0), (y0 + H - 1, x0 + W - 1), (y0 + H // 2, x0 + W // 2), (y0, x0 + W - 1), (y0 + H - 1, x0), (y0 + H // 3, x0 + W // 3)]
    values = [600.0, -600.0, float("nan"), float("inf"), -float("inf"), 511.99]
    for k, ((y, x), v) in enumerate(zip(spots, values)):
        flow[k % N, k % 2, y, x] = v
    return flow


@pytest.mark.parametrize("shape", ((1, 8, 8), (2, 13, 21), (1, 16, 31)), ids=lambda s: "x".join(map(str, s)))
def test_same_size_flow_resize_is_flow_export(ops, shape):
    N, H, W = shape
    crop = (2, 3, H, W)
    dev = planted_flow(N, H + 5, W + 4, crop, seed=H * 100 + W).cuda()
    want = ops.flow_export(dev, crop=crop)
    assert same_bits(ops.flow_resize(dev, (H, W), crop=crop, coding="f32"), want)
    assert same_bits(ops.flow_resize(dev, (H, W), crop=crop), want.permute(0, 3, 1, 2).contiguous())
    for scale in (64.0, 128.0):
        for be in (False, True):
            a = ops.flow_resize(dev, (H, W), crop=crop, coding="u16", scale=scale, big_endian=be)
            b = ops.flow_export(dev, crop=crop, coding="u16", scale=scale, big_endian=be)
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), (scale, be)


@pytest.mark.parametrize("factor", [1, 2])
def test_non_finite_taps_reach_their_outputs_only(ops, factor):
    g = torch.Generator().manual_seed(9)
    Hc, Wc, crop = 8, 12, (1, 2, 8, 12)
    flow = 40 * torch.randn(1, 2, 11, 16, generator=g)
    flow[0, 0, 1 + 3, 2 + 4] = float("nan")                  # u at window pixel (3, 4)
    flow[0, 1, 1 + 5, 2 + 7] = float("inf")                  # v at window pixel (5, 7)
    H, W = factor * Hc, factor * Wc
    bad_u, bad_v = torch.zeros(H, W, dtype=torch.bool), torch.zeros(H, W, dtype=torch.bool)
    bad_u[np.ix_(Z.touched(Hc, H, 3), Z.touched(Wc, W, 4))] = True
    bad_v[np.ix_(Z.touched(Hc, H, 5), Z.touched(Wc, W, 7))] = True
    assert int(bad_u.sum()) == int(bad_v.sum()) == (1 if factor == 1 else 16)       # (2x: four outputs per axis blend an interior tap)
    dev = flow.cuda()
    got = ops.flow_resize(dev, (H, W), crop=crop).cpu()
    assert torch.equal(~torch.isfinite(got[0, 0]), bad_u) and torch.equal(~torch.isfinite(got[0, 1]), bad_v)
    codes = torch.from_numpy(ops.flow_resize(dev, (H, W), crop=crop, coding="u16").cpu().numpy().astype(np.int64))[0]
    assert torch.equal(codes[..., 2] == 0, bad_u | bad_v)
    assert (codes[..., 0][bad_u] == 0).all() and (codes[..., 1][bad_v] == 0).all()
    assert (codes[..., 0][~bad_u] != 0).all() and (codes[..., 1][~bad_v] != 0).all()       # (|40 randn| stays far inside +-512)


# ------------------------------------------------------------------------------------------------
# arguments


def test_argument_errors_launch_nothing(ops):
    import ctypes
    from accflow_amd import _lib
    lib = _lib.load()
    hwc = R.ingest_bytes(1, 8, 8, seed=1).cuda()
    for size in ((0, 4), (4, -1), (4.5, 4), (4, 4.0), (4,), 4, "ab", (1 << 20, 4)):
        with pytest.raises(RuntimeError, match="size"):
            ops.frames_from_u8(hwc, size=size)
    with pytest.raises(RuntimeError, match="interp"):
        ops.frames_from_u8(hwc, size=(4, 4), interp="bicubic")
    with pytest.raises(RuntimeError, match="interp"):
        ops.frames_from_u8(hwc, interp="nearest")
    out = torch.full((1, 3, 4, 4), 7.0, device="cuda")
    with pytest.raises(RuntimeError, match="out must be"):
        ops.frames_from_u8(hwc, size=(4, 5), out=out)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.frames_from_u8(hwc, size=(4, 4), pad=(1, 0, 0, 0), out=out)
    huge = torch.zeros((1, 4096, 4096, 3), dtype=torch.uint8, device="cuda")      # (a 4097 x 4097 window: 2^24 pixels and more)
    with pytest.raises(RuntimeError, match="2\\^24"):
        ops.frames_from_u8(huge, size=(1, 1), interp="area", out=out[:, :, :1, :1])
    flow = torch.zeros((1, 2, 8, 12), device="cuda")
    fout = torch.full((1, 2, 4, 4), 7.0, device="cuda")
    for crop in ((0, 0, 9, 12), (-1, 0, 4, 4), (0, 5, 8, 8), (0, 0, 0, 4), (1, 2, 3)):
        with pytest.raises(RuntimeError, match="crop"):
            ops.flow_resize(flow, (4, 4), crop=crop, out=fout)
    with pytest.raises(RuntimeError, match="size"):
        ops.flow_resize(flow, (4, 0))
    with pytest.raises(RuntimeError, match="coding"):
        ops.flow_resize(flow, (4, 4), coding="flo")
    with pytest.raises(RuntimeError, match="out must be"):
        ops.flow_resize(flow, (4, 5), out=fout)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.flow_resize(flow, (4, 4), coding="f32", out=fout)
    with pytest.raises(RuntimeError, match="scale"):
        ops.flow_resize(flow, (4, 4), coding="u16", scale=0.0)

    # the C entry points refuse the same with 1
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ingest(H=8, W=8, oh=4, ow=4, interp=0, pads=(0, 0, 0, 0), src=hwc, N=1):
        return lib.accflow_frames_from_u8_resized(p(src), 0, 3 * W, 0, 0, 0, 1, p(out), 3 * 16, N, H, W, pads[0], pads[1], pads[2],
                                                  pads[3], oh, ow, interp, st)
    assert ingest(oh=0) == 1 and ingest(ow=-3) == 1 and ingest(interp=2) == 1 and ingest(interp=-1) == 1
    assert ingest(pads=(0, -1, 0, 0)) == 1 and ingest(N=0) == 1 and ingest(oh=32769) == 1
    assert ingest(H=4096, W=4096, oh=1, ow=1, interp=1, src=huge) == 1

    def resize(crop=(0, 0, 8, 12), H=4, W=4, coding=2):
        return lib.accflow_flow_resize(p(flow), 2 * 8 * 12, 8, 12, crop[0], crop[1], crop[2], crop[3], H, W, p(fout), 0, coding, 64.0,
                                       0, 1, st)
    assert resize(crop=(0, 0, 9, 12)) == 1 and resize(crop=(0, 5, 8, 8)) == 1 and resize(crop=(-1, 0, 4, 4)) == 1
    assert resize(H=0) == 1 and resize(W=32769) == 1 and resize(coding=3) == 1 and resize(coding=-1) == 1
    torch.cuda.synchronize()
    assert (out == 7).all() and (fout == 7).all()
    # ... and take the good call
    assert ingest() == 0 and resize() == 0
    torch.cuda.synchronize()
    assert same_bits(out, ops.frames_from_u8(hwc, size=(4, 4))) and (fout == 0).all()


# ------------------------------------------------------------------------------------------------
# FrameScaler


@pytest.mark.parametrize("mode", ["sintel", "kitti"])
def test_frame_scaler_without_a_size_is_the_padder(ops, mode):
    from accflow_amd.frames import FramePadder, FrameScaler
    N, H, W = 2, 13, 21
    dev = R.ingest_bytes(N, H, W, seed=8).cuda()
    padder, scaler = FramePadder((H, W), mode), FrameScaler((H, W), pad=mode)
    assert scaler.size == (H, W) and scaler.padder.crop == padder.crop
    for bgr in (False, True):
        assert same_bits(scaler.ingest(dev, bgr=bgr), padder.ingest(dev, bgr=bgr))
    x = padder.ingest(dev)
    flow = planted_flow(N, x.shape[2], x.shape[3], padder.crop, seed=3).cuda()
    assert same_bits(scaler.export(flow), padder.export(flow))
    for be in (False, True):
        a, b = scaler.export(flow, coding="u16", scale=128.0, big_endian=be), padder.export(flow, coding="u16", scale=128.0, big_endian=be)
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert same_bits(scaler.flow(flow), padder.unpad(flow))
    # a size argument that changes nothing is the padder as well
    assert same_bits(FrameScaler((H, W), max_side=21, pad=mode).ingest(dev), x)


def test_frame_scaler_half_size(ops):
    from accflow_amd.frames import FrameScaler
    H, W = 32, 48
    scaler = FrameScaler((H, W), scale=0.5)
    assert scaler.size == (16, 24) and scaler.padder.crop == (0, 0, 16, 24)
    hwc = R.ingest_bytes(2, H, W, seed=6)
    x = scaler.ingest(hwc.cuda())
    assert same_bits(x, ops.frames_from_u8(hwc.cuda(), size=(16, 24)))
    box = Z.levels(hwc).float().reshape(2, 3, 16, 2, 24, 2).sum(dim=(3, 5)) / 4.0
    assert same_bits(x, 2 * (box / 255.0) - 1)
    g = torch.Generator().manual_seed(1)
    work = (40 * torch.randn(2, 2, 16, 24, generator=g)).cuda()              # (16 x 24 needs no padding: the model's flow as it is)
    assert same_bits(scaler.export(work), ops.flow_resize(work, (H, W), coding="f32"))
    assert scaler.export(work).shape == (2, H, W, 2) and same_bits(scaler.flow(work), ops.flow_resize(work, (H, W)))
    for be in (False, True):
        a, b = scaler.export(work, coding="u16", big_endian=be), ops.flow_resize(work, (H, W), coding="u16", big_endian=be)
        assert a.shape == (2, H, W, 3) and np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    # a working size that needs padding: 18 x 26 -> 24 x 32, the frame's window at (3, 3)
    scaler = FrameScaler((36, 52), scale=0.5)
    assert scaler.size == (18, 26) and scaler.padder.crop == (3, 3, 18, 26)
    g = torch.Generator().manual_seed(2)
    flow = torch.full((2, 2, 24, 32), 1e30)
    flow[:, :, 3:21, 3:29] = 40 * torch.randn(2, 2, 18, 26, generator=g)
    dev = flow.cuda()
    work = scaler.padder.unpad(dev).contiguous()
    assert same_bits(scaler.flow(dev), ops.flow_resize(work, (36, 52)))
    assert same_bits(scaler.flow(scaler.padder.unpad(dev)), ops.flow_resize(work, (36, 52)))
    assert same_bits(scaler.export(dev), ops.flow_resize(work, (36, 52), coding="f32"))
    a = scaler.export(dev, coding="u16", scale=128.0, big_endian=True)
    b = ops.flow_resize(work, (36, 52), coding="u16", scale=128.0, big_endian=True)
    assert a.shape == (2, 36, 52, 3) and np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert float(scaler.flow(dev).abs().max()) < 1e4
    with pytest.raises(RuntimeError, match="made for"):
        scaler.ingest(hwc.cuda())


# ------------------------------------------------------------------------------------------------
# end to end


def synthetic_u8_frames(n, H, W, seed=1000):
    from accflow_amd.data.synthetic import make_sequence
    return [f[0].permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8).contiguous() for f in make_sequence(seed, n, H, W)]


@pytest.fixture(scope="module")
def model():
    from accflow_amd.eval_cvo import build_model
    return build_model("acc", "raft", None, None, torch.device("cuda"))


def test_infer_at_a_working_size(ops, model, tmp_path):
    """256 x 512 frames (twice 128 x 256, the smallest frame of tests/test_accflow_stream.py) with max_side=256."""
    from accflow_amd import frames, infer, viz
    H, W, iters, n = 256, 512, 4, 5
    paths = []
    for k, im in enumerate(synthetic_u8_frames(n, H, W)):
        paths.append(str(tmp_path / ("frame_%03d.png" % k)))
        viz.write_png(paths[-1], im)
    out = tmp_path / "out"
    flows = infer.run(paths, str(out), iters=iters, flo=True, png=True, model=model, max_side=256)
    working = infer.run(paths, None, iters=iters, model=model, max_side=256, flows_at="working")
    scaler = frames.FrameScaler((H, W), max_side=256)
    assert scaler.size == (128, 256) and len(flows) == len(working) == n - 2
    for i, (got, small) in enumerate(zip(flows, working), start=2):
        assert got.shape == (1, 2, H, W) and small.shape == (1, 2, 128, 256) and torch.isfinite(got).all()
        assert torch.equal(got, scaler.flow(small)), i
        back = frames.read_flo(str(out / ("flow_%d_to_0.flo" % i)))
        assert back.shape == (H, W, 2) and back.tobytes() == got[0].permute(1, 2, 0).contiguous().cpu().numpy().tobytes(), i
        assert frames.read_image(str(out / ("flow_%d_to_0.png" % i))).shape == (H, W, 3)
    # files at the working size
    small_out = tmp_path / "small"
    infer.run(paths, str(small_out), iters=iters, flo=True, model=model, size=(128, 256), flows_at="working")
    back = frames.read_flo(str(small_out / "flow_2_to_0.flo"))
    assert back.tobytes() == working[0][0].permute(1, 2, 0).contiguous().cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="flows_at"):
        infer.run(paths, None, model=model, flows_at="both")


def test_infer_without_the_new_arguments_is_todays_run(ops, model, tmp_path):
    """Today's run, restated: FramePadder.ingest, AccFlowStream, unpad."""
    from accflow_amd import frames, infer, viz
    from accflow_amd.networks.AccFlow_ import AccFlowStream
    H, W, iters = 125, 250, 4
    u8 = synthetic_u8_frames(4, H, W)
    paths = []
    for k, im in enumerate(u8):
        paths.append(str(tmp_path / ("frame_%03d.png" % k)))
        viz.write_png(paths[-1], im)
    padder = frames.FramePadder((H, W), "sintel")
    x = padder.ingest(torch.stack(u8).cuda())

    def streamed():
        s = AccFlowStream(model, iters=iters)
        outs = []
        with torch.no_grad():
            for i in range(4):
                outs += s.push(x[i:i + 1])
        return outs
    first, second = streamed(), streamed()
    assert len(first) == 2 and all(torch.equal(a, b) for a, b in zip(first, second)), "two identical AccFlowStream runs are not bit-equal"
    out = tmp_path / "out"
    flows = infer.run(paths, str(out), iters=iters, flo=True, model=model)
    assert len(flows) == 2
    for i, (got, want) in enumerate(zip(flows, first), start=2):
        assert torch.equal(got, padder.unpad(want)), i
        back = frames.read_flo(str(out / ("flow_%d_to_0.flo" % i)))
        assert back.tobytes() == padder.export(want.contiguous())[0].cpu().numpy().tobytes(), i
    # the size options spelled out as "nothing"
    again = infer.run(paths, None, iters=iters, model=model, size=None, scale=None, max_side=None, interp="bilinear", flows_at="source")
    assert all(torch.equal(a, b) for a, b in zip(again, flows))


def test_eval_hs_sintel(ops, model, tmp_path):
    from accflow_amd import eval_hs_sintel, frames, viz
    H, W, H0, W0 = 128, 256, 160, 320
    g = torch.Generator().manual_seed(12)
    chosen = {}
    for s in range(2):
        root = tmp_path / ("sample_%d" % s)
        os.makedirs(str(root / "2_imgs")), os.makedirs(str(root / "43_imgs"))
        hs = synthetic_u8_frames(5, H0, W0, seed=2000 + s)
        for k, im in enumerate(hs):
            viz.write_png(str(root / "43_imgs" / ("frame_%04d.png" % k)), im)
        for k, im in enumerate(synthetic_u8_frames(2, H, W, seed=2000 + s)):
            viz.write_png(str(root / "2_imgs" / ("frame_%04d.png" % k)), im)
        frames.write_flo(str(root / "gt.flo"), (3 * torch.randn(H, W, 2, generator=g)).numpy())
        occ = (torch.rand(H, W, 1, generator=g) < 0.25).to(torch.uint8) * 255
        viz.write_png(str(root / "occ.png"), occ.expand(H, W, 3).contiguous())
        chosen["sample_%d" % s] = hs[::2]
    res = eval_hs_sintel.run(str(tmp_path), interv=2, model=model, keep_flows=True, verbose=False)
    assert [e["name"] for e in res["samples"]] == ["sample_0", "sample_1"]
    padder = frames.FramePadder((H, W))
    for e in res["samples"]:
        assert all(np.isfinite(e[k]) and e[k] > 0 for k in ("epe_all", "epe_occ", "epe_vis"))
        # by hand: the chosen frames, last first, resized in the ingest launch, through the model
        u8 = torch.stack(chosen[e["name"]][::-1]).cuda()
        x = ops.frames_from_u8(u8, pad=tuple(padder._pad), size=(H, W))
        with torch.no_grad():
            want = model([x[k:k + 1] for k in range(3)])[-1]
        assert e["flow"].shape == (1, 2, H, W) and torch.equal(e["flow"], padder.unpad(want))
    for k in ("epe_all", "epe_occ", "epe_vis"):
        assert res["mean"][k] == pytest.approx(sum(e[k] for e in res["samples"]) / 2, rel=1e-12)
    with pytest.raises(ValueError, match="does not divide"):
        eval_hs_sintel.run(str(tmp_path), interv=3, model=model, verbose=False)
