"""ops.frames_from_u8 / ops.flow_export (csrc/frame_io.hip), frames.FramePadder and accflow_amd.infer on the GPU.

Ingest: bit for bit (the float32 words compared as integers) against the CPU reference
F.pad(2 * (x.float() / 255.0) - 1, pad, mode="replicate"), with normalize=False against F.pad(x.float(), ...).  Bit equality is
derived, not measured: there are 256 input codes, torch's result for each is one correctly rounded division followed by an
exact doubling and one rounded subtraction, and padding copies values.  On the CPU numpy and torch agree on all 256 codes, a
multiplication by the reciprocal differs from them on 111 and a float64 evaluation rounded once on 128 - so the test bites on
the shortcuts a kernel writer would take.  Every sample starts with the bytes 0..255 in order; one extra frame holds all 256
codes in each channel.  Shapes (frame_io_ref.INGEST_SHAPES): the smallest at which each path can go wrong; each runs in both
layouts, channel orders and pad modes, and once more from a pitched view (row pitch 3 W + 5 bytes) and from a view whose base
is one byte past a dword boundary - both force the byte path and must give the aligned run's bits.

Export: "f32" bitwise against flow[:, :, y0:y0+H, x0:x0+W].permute(0, 2, 3, 1); "u16" exact against numpy in float32,
np.trunc(np.clip(np.float32(s) * f + np.float32(32768), 0, 65535)), with +-600 (beyond both ends of the code range), NaN and
+-inf planted, both byte orders, s = 64 and 128.  The shapes are the padded outputs of the ingest cases with the padder's crop:
odd x0, W % 4 != 0, groups that start off a dword.

End to end: accflow_amd.infer.run on four 125 x 250 frames (padded to 128 x 256, the estimator's minimum) against
AccFlowStream on the frames prepared with torch operators - torch.equal, under the precondition, asserted first as in
tests/test_accflow_stream.py, that two identical stream runs are bit-equal; the .flo files read back bit-equal and the KITTI
PNGs decode to the "u16" codes.
"""
import numpy as np
import pytest
import torch

import frame_io_ref as R

pytestmark = pytest.mark.gpu
MODES = ("sintel", "kitti")


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
    got = got.cpu()
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    return torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


def device_views(hwc, layout):
    """The same frames on the device three times: dense and dword-aligned, with a row pitch of 3 W + 5 bytes, and from a base
    one byte past a dword boundary.  layout "chw": planar (N,3,H,W)."""
    src = (hwc if layout == "hwc" else hwc.permute(0, 3, 1, 2)).contiguous()
    aligned = src.cuda()
    assert aligned.data_ptr() % 4 == 0 and aligned.is_contiguous()
    N, H, W = hwc.shape[:3]
    pitch = 3 * W + 5
    if layout == "hwc":
        buf = torch.zeros((N, H, pitch), dtype=torch.uint8, device="cuda")
        pitched = buf[:, :, :3 * W].unflatten(2, (W, 3))
        strides = (H * pitch, pitch, 3, 1)
    else:
        buf = torch.zeros((N, 3, H, pitch), dtype=torch.uint8, device="cuda")
        pitched = buf[..., :W]
        strides = (3 * H * pitch, H * pitch, pitch, 1)
    assert all(s == e for s, e, n in zip(pitched.stride(), strides, pitched.shape) if n > 1)     # (a dimension of 1 has no stride to speak of)
    pitched.copy_(aligned)
    flat = torch.zeros(src.numel() + 1, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 4 == 0
    shifted = flat[1:].view(src.shape)
    shifted.copy_(aligned)
    assert shifted.data_ptr() % 4 == 1
    return aligned, pitched, shifted


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", R.INGEST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ingest_bitwise(ops, shape, mode):
    from accflow_amd.frames import FramePadder
    N, H, W = shape
    hwc = R.ingest_bytes(N, H, W, seed=H * 100 + W)
    assert hwc[:, 0, 0, 0].tolist() == [0] * N and hwc.reshape(N, -1)[0, :min(256, 3 * H * W)].tolist() == list(range(min(256, 3 * H * W)))
    padder = FramePadder((H, W), mode)
    l, r, t, b = padder._pad
    for layout in ("hwc", "chw"):
        views = device_views(hwc, layout)
        for bgr in (False, True):
            want = R.ingest_reference(hwc, padder._pad, bgr=bgr)
            assert want.shape == (N, 3, H + t + b, W + l + r) and want.shape[2] % 8 == 0 and want.shape[3] % 8 == 0
            first = padder.ingest(views[0], layout=layout, bgr=bgr)
            assert same_bits(first, want), (layout, bgr, "aligned")
            for what, v in zip(("pitched", "base + 1"), views[1:]):
                got = padder.ingest(v, layout=layout, bgr=bgr)
                assert same_bits(got, want) and torch.equal(got, first), (layout, bgr, what)
        for v in views:
            assert same_bits(padder.ingest(v, layout=layout, normalize=False), R.ingest_reference(hwc, padder._pad, normalize=False)), layout
    # a single (H,W,3) frame is a batch of one
    assert torch.equal(padder.ingest(hwc[0].cuda()), padder.ingest(hwc[:1].cuda()))
    assert padder.unpad(first).shape == (N, 3, H, W)


def test_ingest_all_256_codes(ops):
    hwc = R.all_codes_frame()
    for c in range(3):
        assert sorted(hwc[0, :, :, c].reshape(-1).tolist()) == list(range(256))
    for layout in ("hwc", "chw"):
        for bgr in (False, True):
            want = R.ingest_reference(hwc, (0, 0, 0, 0), bgr=bgr)
            for v in device_views(hwc, layout):
                assert same_bits(ops.frames_from_u8(v, layout=layout, bgr=bgr), want), (layout, bgr)
    # the 256 values themselves, against numpy's float32 as well
    codes = np.arange(256, dtype=np.float32)
    by_numpy = np.float32(2) * (codes / np.float32(255)) - np.float32(1)
    got = ops.frames_from_u8(hwc.cuda())[0, 0].reshape(-1).cpu().numpy()
    assert got.tobytes() == by_numpy.tobytes()
    assert got[0] == -1.0 and got[255] == 1.0


@pytest.mark.parametrize("pad", [(0, 0, 0, 0), (5, 0, 0, 2), (1, 6, 9, 0)])
def test_ingest_explicit_pads(ops, pad):
    N, H, W = 2, 13, 21
    hwc = R.ingest_bytes(N, H, W, seed=77)
    for layout in ("hwc", "chw"):
        for v in device_views(hwc, layout):
            got = ops.frames_from_u8(v, layout=layout, bgr=True, pad=pad)
            assert got.shape == (N, 3, H + pad[2] + pad[3], W + pad[0] + pad[1])
            assert same_bits(got, R.ingest_reference(hwc, pad, bgr=True)), (layout, pad)


def test_ingest_out_and_batch_slices(ops):
    N, H, W = 3, 9, 40
    hwc = R.ingest_bytes(N, H, W, seed=5)
    pad = (0, 0, 3, 4)
    want = R.ingest_reference(hwc, pad)
    dev = hwc.cuda()
    big = torch.full((N, 5, 16, 40), 7.0, device="cuda")
    out = big[:, 1:4]                                          # dense samples, a batch stride of 5 planes
    assert ops.frames_from_u8(dev, pad=pad, out=out).data_ptr() == out.data_ptr()
    assert same_bits(out, want) and (big[:, 0] == 7).all() and (big[:, 4] == 7).all()
    # every second sample of the source: the sample stride is the tensor's
    assert same_bits(ops.frames_from_u8(dev[::2], pad=pad), want[::2])
    assert same_bits(ops.frames_from_u8(dev[1:2], pad=pad), want[1:2])
    # a window of a larger frame: rows, columns and base all off the frame's own
    win = dev[:, 2:7, 3:30]
    assert same_bits(ops.frames_from_u8(win, pad=(2, 1, 0, 1)), R.ingest_reference(hwc[:, 2:7, 3:30], (2, 1, 0, 1)))
    with pytest.raises(RuntimeError, match="dense"):
        ops.frames_from_u8(dev, pad=pad, out=torch.zeros((N, 3, 16, 80), device="cuda")[..., ::2])


# ------------------------------------------------------------------------------------------------
# export


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


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", R.INGEST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_export(ops, shape, mode):
    from accflow_amd.frames import FramePadder
    N, H, W = shape
    padder = FramePadder((H, W), mode)
    l, r, t, b = padder._pad
    Hp, Wp = H + t + b, W + l + r
    flow = planted_flow(N, Hp, Wp, padder.crop, seed=H * 100 + W)
    dev = flow.cuda()
    # "f32": the window, interleaved, bit for bit (NaN payloads included)
    want = flow[:, :, t:t + H, l:l + W].permute(0, 2, 3, 1).contiguous()
    got = padder.export(dev)
    assert got.shape == (N, H, W, 2) and same_bits(got, want)
    assert same_bits(ops.flow_export(dev), flow.permute(0, 2, 3, 1).contiguous())
    # "u16": exact, both byte orders, both scales
    fnp = flow.numpy()
    for scale in (64.0, 128.0):
        for be in (False, True):
            ref = R.u16_reference(fnp, padder.crop, scale, be)
            got = padder.export(dev, coding="u16", scale=scale, big_endian=be)
            assert got.dtype == torch.uint16 and got.shape == (N, H, W, 3)
            assert np.array_equal(got.cpu().numpy(), ref), (scale, be)
    ref = R.u16_reference(fnp, padder.crop, 64.0, False)
    if H * W >= 6:                                                  # (all six planted values fit)
        assert (ref[..., 2] == 0).sum() == 3 and ref[..., :2].max() == 65535 and (ref[..., :2] == 0).sum() >= 4
    # a batch slice as the destination, int16 storage, samples starting off a dword (H W odd: 6 H W bytes is 2 mod 4)
    big = torch.zeros((N, H * W * 3 + 1), dtype=torch.int16, device="cuda")
    out = big[:, 1:].view(N, H, W, 3)
    assert ops.flow_export(dev, crop=padder.crop, coding="u16", out=out).data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy().view(np.uint16), ref) and (big[:, 0] == 0).all()


def test_export_batch_slices_and_big_values(ops):
    g = torch.Generator().manual_seed(3)
    flow = 40 * torch.randn(4, 2, 16, 24, generator=g)
    flow[0, 0, 0, :6] = torch.tensor([3.0e38, -3.0e38, 511.984375, 512.0, -512.0, -512.0078125])   # 64 f + 32768: inf, -inf, 65535, 65536, 0, -0.5
    dev = flow.cuda()
    sl = dev[::2]
    assert not sl.is_contiguous()
    assert same_bits(ops.flow_export(sl, crop=(1, 2, 13, 21)), flow[::2, :, 1:14, 2:23].permute(0, 2, 3, 1).contiguous())
    got = ops.flow_export(dev, coding="u16").cpu().numpy()
    assert np.array_equal(got, R.u16_reference(flow.numpy(), (0, 0, 16, 24), 64.0, False))
    assert got[0, 0, :6, 0].tolist() == [65535, 0, 65535, 65535, 0, 0] and (got[..., 2] == 1).all()
    big = torch.zeros((4, 16, 24, 2 + 1), device="cuda")
    with pytest.raises(RuntimeError, match="dense"):
        ops.flow_export(dev, out=big[..., :2])


# ------------------------------------------------------------------------------------------------
# end to end


def synthetic_u8_frames(n, H, W, seed=1000):
    from accflow_amd.data.synthetic import make_sequence
    return [f[0].permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8).contiguous() for f in make_sequence(seed, n, H, W)]


@pytest.fixture(scope="module")
def model():
    from accflow_amd.eval_cvo import build_model
    return build_model("acc", "raft", None, None, torch.device("cuda"))


def test_infer_end_to_end(ops, model, tmp_path):
    from accflow_amd import frames, infer, viz
    from accflow_amd.networks.AccFlow_ import AccFlowStream
    H, W, iters = 125, 250, 4
    u8 = synthetic_u8_frames(4, H, W)
    paths = []
    for k, im in enumerate(u8):
        paths.append(str(tmp_path / ("frame_%03d.png" % k)))
        viz.write_png(paths[-1], im)
    padder = frames.FramePadder((H, W), "sintel")
    assert padder._pad == [3, 3, 1, 2]
    prepared = R.ingest_reference(torch.stack(u8), padder._pad).cuda()          # the torch route, on the CPU
    assert prepared.shape == (4, 3, 128, 256)

    def streamed():
        s = AccFlowStream(model, iters=iters)
        outs = []
        for i in range(4):
            outs += s.push(prepared[i:i + 1])
        return outs
    first, second = streamed(), streamed()
    assert len(first) == 2 and all(torch.equal(a, b) for a, b in zip(first, second)), "two identical AccFlowStream runs are not bit-equal"
    out = tmp_path / "out"
    flows = infer.run(str(tmp_path / "frame_*.png"), str(out), iters=iters, flo=True, kitti=True, png=True, model=model)
    assert len(flows) == 2
    for i, (got, want) in enumerate(zip(flows, first), start=2):
        assert got.shape == (1, 2, H, W) and torch.isfinite(got).all()
        assert torch.equal(got, padder.unpad(want)), i
        hw2 = got[0].permute(1, 2, 0).contiguous().cpu()
        back = frames.read_flo(str(out / ("flow_%d_to_0.flo" % i)))
        assert back.shape == (H, W, 2) and back.tobytes() == hw2.numpy().tobytes(), i
        codes, _ = R.decode_png((out / ("flow_%d_to_0_kitti.png" % i)).read_bytes())
        assert codes.dtype == np.uint16
        assert np.array_equal(codes, R.u16_reference(want.cpu().numpy(), padder.crop, 64.0, False)[0]), i
        assert (codes[..., 2] == 1).all()
        assert frames.read_image(str(out / ("flow_%d_to_0.png" % i))).shape == (H, W, 3)
    assert sorted(p.name for p in out.iterdir()) == sorted(
        ["flow_%d_to_0%s" % (i, ext) for i in (2, 3) for ext in (".flo", "_kitti.png", ".png")])


def test_infer_direct(ops, model, tmp_path):
    """--acc direct: the estimator on (frame i, frame 0); a PPM sequence, the `kitti` pad mode, BGR order."""
    from accflow_amd import frames, infer
    H, W = 125, 250
    u8 = synthetic_u8_frames(3, H, W, seed=1001)
    for k, im in enumerate(u8):
        (tmp_path / ("%d.ppm" % k)).write_bytes(b"P6\n# frame %d\n%d %d\n255\n" % (k, W, H) + im.numpy().tobytes())
    flows = infer.run(str(tmp_path), None, acc="direct", iters=4, pad="kitti", bgr=True, model=model.ofe)
    assert len(flows) == 1 and flows[0].shape == (1, 2, H, W) and torch.isfinite(flows[0]).all()
    padder = frames.FramePadder((H, W), "kitti")
    x = padder.ingest(torch.stack(u8).cuda(), bgr=True)
    assert same_bits(x, R.ingest_reference(torch.stack(u8), padder._pad, bgr=True))
    with pytest.raises(ValueError, match="at least 3"):
        infer.run([str(tmp_path / "0.ppm"), str(tmp_path / "1.ppm")], None, model=model)
