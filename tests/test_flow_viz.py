"""ops.flow_maxrad / ops.flow_to_rgb (csrc/flow_viz.hip) and accflow_amd.viz on the GPU, against the float64 restatement and
the comparison rule of tests/flow_viz_ref.py (derived there, not measured) and against the reference's own pictures
(tests/golden/flow_viz.npz).

Inputs (recipes in flow_viz_ref): smooth = interpolate(8 randn(B, 2, 3, 4)), noise = 5 randn; a non-zero |v| is kept at least
1e-3 |u|, so only exact signed zeros sit on the colour seam.  Shapes (B, H, W):
    (1, 1, 1)      the degenerate case                       (2, 3, 5)      45-byte packed samples: the second base is odd
    (1, 37, 67)    W % 4 != 0                                (3, 16, 130)   a batch with W % 4 != 0
    (2, 70, 130)   9100 pixels: three runs of 4096 per sample
The two shapes under 1000 pixels use seeds without a component in the rule's tau band and are compared exactly; for the
others the band holds 0.15 - 0.8 % of the components (cap: 1.5 %, asserted before the output is looked at).

The scale is compared bit for bit with numpy's float32.  Measured on an MI355X: see DESIGN.md 4.8.
"""
import functools

import numpy as np
import pytest
import torch

import flow_viz_ref as R

pytestmark = pytest.mark.gpu
#        B  H   W    smooth seed, noise seed
CASES = ((1, 1, 1, 1, 1), (2, 3, 5, 2, 2), (1, 37, 67, 11, 12), (3, 16, 130, 13, 14), (2, 70, 130, 15, 16))
IDS = ["%dx%dx%d" % c[:3] for c in CASES]
RECIPES = ("smooth", "noise")


@functools.lru_cache(maxsize=None)
def case_flow(case, recipe):
    B, H, W, s_smooth, s_noise = case
    flow = R.smooth_flow(B, H, W, s_smooth) if recipe == "smooth" else R.noise_flow(B, H, W, s_noise)
    return flow, flow.cuda()


def exact(case):
    return case[1] * case[2] < 1000


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32).tolist()


def np_scales(flow, clip=None):
    return np.array([R.max_radius32(f, clip) for f in flow.numpy()], dtype=np.float32)


def check_batch(img, flow, scales, what, **kw):
    img = img.cpu().numpy()
    stats = [R.check_image(img[b], flow[b].numpy(), scales[b], what="%s sample %d" % (what, b), **kw) for b in range(flow.shape[0])]
    print("%s: band components %s, rad-1 pixels %s, worst |x - round(x)| of a component off floor(x): %.2e" % (
        what, [s[0] for s in stats], [s[1] for s in stats], max(s[2] for s in stats)))
    return stats


# ------------------------------------------------------------------------------------------------
# 1. the scale


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_maxrad_bits(case, recipe):
    from accflow_amd import ops
    flow, dev = case_flow(case, recipe)
    for clip in (None, 4.0):
        want = np_scales(flow, clip)
        assert bits(ops.flow_maxrad(dev, clip=clip)) == want.view(np.uint32).tolist(), clip
        shared = ops.flow_maxrad(dev, clip=clip, shared=True)
        assert bits(shared) == [int(want.max().view(np.uint32))] * case[0], clip
    assert float(np_scales(flow, 4.0).max()) <= 4.0 * 2 ** 0.5 * (1 + 1e-6) and (np_scales(flow) > 0).all()


@pytest.mark.parametrize("where", [0, 9099, 8192 + 300], ids=["first", "last", "last-run"])
def test_maxrad_wherever_the_maximum_sits(where):
    from accflow_amd import ops
    flow = case_flow(CASES[4], "noise")[0].clone()
    flow.view(2, 2, -1)[1, :, where] = torch.tensor([50.0, -40.0])
    got = ops.flow_maxrad(flow.cuda())
    assert bits(got) == np_scales(flow).view(np.uint32).tolist()
    assert got[1].item() == float(np.sqrt(np.float32(4100.0))) and got[0].item() < 40


def test_maxrad_skips_unknown_pixels():
    from accflow_amd import ops
    flow = case_flow(CASES[3], "noise")[0].clone()                   # (3, 2, 16, 130)
    flat = flow.view(3, 2, -1)
    clean = np_scales(flow)
    flat[0, 0, 5], flat[0, 1, 77], flat[0, 0, 2079], flat[0, 1, 1000] = float("nan"), float("inf"), float("-inf"), 1e10
    flat[0, 1, 5] = 1e6                                               # the partner of a NaN does not count either
    flat[1] = torch.tensor([float("nan"), 2e9]).view(2, 1)            # an all-unknown sample
    want = np_scales(flow)
    assert want[1] == 0 and want[0] <= clean[0] and want[2] == clean[2]
    assert bits(ops.flow_maxrad(flow.cuda())) == want.view(np.uint32).tolist()
    assert bits(ops.flow_maxrad(flow.cuda(), shared=True)) == [int(want.max().view(np.uint32))] * 3
    # 1e9 itself is a flow, the next float is not
    edge = torch.zeros(1, 2, 2, 2)
    edge[0, 0, 0, 0], edge[0, 1, 1, 1] = 1e9, float(np.nextafter(np.float32(1e9), np.float32(2e9)))
    assert ops.flow_maxrad(edge.cuda()).item() == 1e9
    # np.clip comes first: it brings +inf and 1e10 back to the clip value (and leaves NaN alone)
    assert bits(ops.flow_maxrad(flow.cuda(), clip=3.0)) == np_scales(flow, 3.0).view(np.uint32).tolist()


def test_a_sample_does_not_depend_on_its_batch():
    from accflow_amd import ops
    flow = torch.cat([case_flow(CASES[4], "noise")[0], case_flow(CASES[4], "smooth")[0]])      # (4, 2, 70, 130)
    dev = flow.cuda()
    alone = [ops.flow_maxrad(dev[b:b + 1]) for b in range(4)]
    want = [bits(a)[0] for a in alone]
    assert want == np_scales(flow).view(np.uint32).tolist() and len(set(want)) == 4
    assert bits(ops.flow_maxrad(dev)) == want
    order = [2, 0, 3, 1]
    assert bits(ops.flow_maxrad(dev[order].contiguous())) == [want[i] for i in order]
    big = torch.full((4, 5, 70, 130), 1e4, device="cuda")
    big[:, 2:4] = dev
    sl = big[:, 2:4]                                                  # batch stride 5 H W, channel block dense
    assert not sl.is_contiguous() and bits(ops.flow_maxrad(sl)) == want
    imgs = ops.flow_to_rgb(dev, ops.flow_maxrad(dev))
    assert torch.equal(ops.flow_to_rgb(sl, ops.flow_maxrad(sl)), imgs)
    assert torch.equal(ops.flow_to_rgb(dev[3:4], alone[3]), imgs[3:4])


# ------------------------------------------------------------------------------------------------
# 2. the colours


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_colours_vs_float64(case, recipe):
    from accflow_amd import viz
    flow, dev = case_flow(case, recipe)
    scales = np_scales(flow)
    what = "%s %s" % (IDS[CASES.index(case)], recipe)
    check_batch(viz.flow_to_image(dev), flow, scales, what + " per-sample", exact=exact(case))
    check_batch(viz.flow_to_image(dev, max_rad="batch"), flow, [scales.max()] * case[0], what + " batch", exact=exact(case))
    clip = 4.0
    check_batch(viz.flow_to_image(dev, clip_flow=clip), flow, np_scales(flow, clip), what + " clip", clip=clip, caps=not exact(case))


def test_colours_vs_reference_pictures(golden):
    from accflow_amd import viz
    from accflow_amd.networks.gma.utils import flow_viz as gma_viz
    from accflow_amd.networks.raft.utils import flow_viz as raft_viz
    from test_flow_viz_host import EXACT, GENERATED, HAND_MADE, case_of
    g = golden("flow_viz")
    for name in GENERATED + EXACT + HAND_MADE:
        flow, want, scale, clip, bgr = case_of(g, name)
        dev = torch.from_numpy(flow).cuda()
        fixed = float(scale) if name.startswith("fixed") else None
        got = viz.flow_to_image(dev, max_rad=fixed, clip_flow=clip, convert_to_bgr=bgr).cpu().numpy()
        n_band, n_one, worst = R.check_image(got, flow, scale, clip=clip, bgr=bgr, exact=name in EXACT, caps=name in GENERATED, what=name)
        differ = int((got != want).sum())
        print("%s: %d components differ from the reference's picture (band %d, rad-1 pixels %d)" % (name, differ, n_band, n_one))
        # the reference's picture obeys the same rule (test_flow_viz_host): the two can differ only where the rule leaves a choice
        assert differ <= n_band + 3 * n_one, name
        if name in EXACT or name == "seam_1x4":
            assert differ == 0, name
        if fixed is None:
            hwc = np.ascontiguousarray(flow.transpose(1, 2, 0))
            again = raft_viz.flow_to_image(hwc, clip_flow=clip, convert_to_bgr=bgr)
            assert isinstance(again, np.ndarray) and again.dtype == np.uint8 and np.array_equal(again, got), name
    assert gma_viz.flow_to_image is raft_viz.flow_to_image


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_channel_orders_and_layouts_are_permutations(case):
    from accflow_amd import viz
    flow, dev = case_flow(case, "smooth")
    rgb = viz.flow_to_image(dev)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (case[0], case[1], case[2], 3) and rgb.is_contiguous()
    bgr = viz.flow_to_image(dev, convert_to_bgr=True)
    assert torch.equal(bgr, rgb.flip(-1))
    chw = viz.flow_to_image(dev, layout="chw")
    assert tuple(chw.shape) == (case[0], 3, case[1], case[2]) and torch.equal(chw, rgb.permute(0, 3, 1, 2))
    assert torch.equal(viz.flow_to_image(dev, layout="chw", convert_to_bgr=True), bgr.permute(0, 3, 1, 2))
    # a single (2,H,W) flow gives a single picture
    one = viz.flow_to_image(dev[0])
    assert tuple(one.shape) == (case[1], case[2], 3) and torch.equal(one, rgb[0])
    assert torch.equal(viz.flow_to_image(dev[0], layout="chw"), chw[0])


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("case", CASES[:4], ids=IDS[:4])
def test_output_into_a_slice_leaves_the_surroundings_alone(case, layout):
    from accflow_amd import ops
    B, H, W = case[:3]
    flow, dev = case_flow(case, "noise")
    scale = ops.flow_maxrad(dev)
    want = ops.flow_to_rgb(dev, scale, layout=layout)
    n = 3 * H * W
    shape = (B, H, W, 3) if layout == "hwc" else (B, 3, H, W)
    # packed: every byte offset mod 4 as the first sample's base, an odd pitch; planar: dword-aligned base and pitch
    for off, pitch in (((1, n + 7), (2, n + 9), (3, n + 5), (4, n + 6)) if layout == "hwc" else ((4, (n + 3) // 4 * 4 + 8),)):
        buf = torch.full((B, pitch), 7, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 4 == 0
        out = buf[:, off:off + n].view(shape)
        assert ops.flow_to_rgb(dev, scale, layout=layout, out=out).data_ptr() == out.data_ptr()
        assert torch.equal(out, want), (off, pitch)
        assert bool((buf[:, :off] == 7).all()) and bool((buf[:, off + n:] == 7).all()), (off, pitch)
    if layout == "chw" and B > 1 and n % 4:
        with pytest.raises(RuntimeError, match="aligned"):            # dense planar samples of 3 H W bytes: the second base is odd
            ops.flow_to_rgb(dev, scale, layout=layout, out=torch.zeros(shape, dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------------------------------------
# 3. special pixels


def image_of(pixels, **kw):
    """pixels: a list of (u, v) -> the (N, 3) colours of a 1 x N flow."""
    from accflow_amd import viz
    flow = torch.tensor(pixels, dtype=torch.float32).t().contiguous().view(1, 2, 1, len(pixels))
    return viz.flow_to_image(flow.cuda(), **kw)[0, 0].cpu().tolist(), flow


def test_zero_flow_is_white():
    from accflow_amd import ops, viz
    z = torch.zeros(2, 2, 9, 13, device="cuda")
    assert bits(ops.flow_maxrad(z)) == [0, 0]
    for layout in ("hwc", "chw"):
        assert bool((viz.flow_to_image(z, layout=layout) == 255).all())
    assert bool((viz.flow_to_image(-z) == 255).all())                 # (-0, -0) as well
    img, _ = image_of([(0.0, 0.0), (3.0, 4.0), (0.0, -0.0)])
    assert img[0] == [255, 255, 255] and img[2] == [255, 255, 255] and img[1] != [255, 255, 255]


def test_seam_pixels():
    img, _ = image_of([(1.0, 0.0), (1.0, -0.0), (2.0, 0.0), (0.0, 0.0)])
    assert img == [[255, 127, 127], [255, 127, 149], [255, 0, 0], [255, 255, 255]]
    img, _ = image_of([(1.0, 0.0), (1.0, -0.0), (2.0, 0.0), (0.0, 0.0)], convert_to_bgr=True)
    assert img == [[127, 127, 255], [149, 127, 255], [0, 0, 255], [255, 255, 255]]
    # the sign of the zero survives the clip (np.clip keeps -0.0) and the division
    img, _ = image_of([(1.0, 0.0), (1.0, -0.0), (2.0, 0.0), (0.0, 0.0)], clip_flow=5.0)
    assert img == [[255, 127, 127], [255, 127, 149], [255, 0, 0], [255, 255, 255]]
    img, _ = image_of([(1.0, 0.0), (1.0, -0.0)], max_rad=2.0)
    assert img == [[255, 127, 127], [255, 127, 149]]


def test_axis_and_diagonal_directions(golden):
    g = golden("flow_viz")
    flow, want = g["axes_1x9.flow"], g["axes_1x9.img"]
    img, _ = image_of([(float(u), float(v)) for u, v in zip(flow[0, 0], flow[1, 0])])
    R.check_image(np.array([img], dtype=np.uint8), flow, R.max_radius32(flow), exact=True, what="axes")
    assert img == want[0].tolist()
    # east (3, 0) is wheel[0], pure red washed out by its radius; west (-3, 0) is fk = 27 on the cyan-to-blue segment
    assert img[0][0] == 255 and img[0][1] == img[0][2] < 255 and img[4][0] < img[4][1] < img[4][2] == 255


def test_unknown_pixels_are_black_and_disturb_nothing():
    from accflow_amd import viz
    flow = case_flow(CASES[2], "smooth")[0].clone()                   # (1, 2, 37, 67)
    holes = {(0, 0): (float("nan"), 1.0), (5, 66): (2.0, float("inf")), (36, 66): (float("-inf"), float("nan")),
             (17, 30): (1e10, 0.0), (17, 31): (0.0, -1e10), (36, 0): (float("nan"), float("nan"))}
    skipped = flow.clone()
    for (y, x), (u, v) in holes.items():
        flow[0, :, y, x] = torch.tensor([u, v])
        skipped[0, :, y, x] = 0.0                                     # a zero flow takes no part in the maximum either
    for kw in ({}, {"layout": "chw"}, {"max_rad": "batch"}, {"clip_flow": None, "convert_to_bgr": True}):
        got, ref = viz.flow_to_image(flow.cuda(), **kw), viz.flow_to_image(skipped.cuda(), **kw)
        if kw.get("layout") == "chw":
            got, ref = got.permute(0, 2, 3, 1), ref.permute(0, 2, 3, 1)
        hole = torch.zeros(37, 67, dtype=torch.bool)
        for y, x in holes:
            hole[y, x] = True
            assert got[0, y, x].tolist() == [0, 0, 0] and ref[0, y, x].tolist() == [255, 255, 255]
        assert torch.equal(got[0].cpu()[~hole], ref[0].cpu()[~hole])
    check_batch(viz.flow_to_image(flow.cuda()), flow, np_scales(flow), "unknown pixels")


def test_fixed_scale_below_the_maximum():
    from accflow_amd import viz
    flow, dev = case_flow(CASES[3], "smooth")
    scales = np_scales(flow)
    fixed = float(np.float32(0.3) * scales.min())
    beyond = np.mean([(R.colours64(f, fixed)[2] > 1).mean() for f in flow.numpy()])
    assert beyond > 0.5                                               # more than half the pixels take the 0.75 branch
    got = viz.flow_to_image(dev, max_rad=fixed)
    check_batch(got, flow, [np.float32(fixed)] * 3, "fixed scale")
    assert torch.equal(viz.flow_to_image(dev, max_rad=torch.full((3,), fixed, device="cuda")), got)
    assert int(got.max()) <= 255 and float((got.float().amax(-1) == 191).float().mean()) > 0.5   # floor(255 * 0.75) caps them
    per = torch.tensor([fixed, 1e3, float(scales[2])], device="cuda")
    mixed = viz.flow_to_image(dev, max_rad=per)
    assert torch.equal(mixed[0], got[0]) and torch.equal(mixed[2], viz.flow_to_image(dev)[2])
    check_batch(mixed, flow, per.cpu().numpy(), "per-sample fixed scales")


def test_a_300_px_maximum(golden):
    from accflow_amd import ops, viz
    flow = golden("flow_viz")["big300_8x16.flow"]
    s = R.max_radius32(flow)
    assert 299.9 < s < 300.1 and np.float32(s) + np.float32(1e-5) == np.float32(s)
    dev = torch.from_numpy(flow)[None].cuda()
    assert bits(ops.flow_maxrad(dev)) == [int(s.view(np.uint32))]
    n_band, n_one, _ = R.check_image(viz.flow_to_image(dev)[0].cpu().numpy(), flow, s, what="300 px")
    assert n_one == 1                                                 # the pixel that sets the scale: rad = 1 to an ulp


# ------------------------------------------------------------------------------------------------
# 4. no transfer, train_acc


def counting_host_reads(monkeypatch):
    reads = []
    for name in ("item", "__float__", "__int__", "__bool__", "cpu", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **kw):
            if self.is_cuda:
                reads.append(_name)
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    return reads


def test_flow_to_image_makes_no_device_to_host_transfer(monkeypatch):
    from accflow_amd import viz
    flow, dev = case_flow(CASES[3], "smooth")
    want = viz.flow_to_image(dev).cpu()
    reads = counting_host_reads(monkeypatch)
    a = viz.flow_to_image(dev, max_rad=None)
    b = viz.flow_to_image(dev, max_rad="batch", clip_flow=4.0, convert_to_bgr=True, layout="chw")
    c = viz.flow_to_image(dev, max_rad=3.5)
    monkeypatch.undo()
    assert reads == [], reads
    assert a.is_cuda and b.is_cuda and c.is_cuda and torch.equal(a.cpu(), want)


def test_validate_keeps_and_train_acc_writes_visual_samples(monkeypatch, tmp_path):
    import torch.nn.functional as F
    from accflow_amd import train_acc, viz
    B, H, W, n_out = 2, 24, 40, 5
    g = torch.Generator().manual_seed(41)

    def enlarge(t):
        return F.interpolate(t, size=(H, W), mode="bilinear", align_corners=True)
    batches, outs = [], []
    for _ in range(2):
        bflows = enlarge(4 * torch.randn(B, 2 * n_out, 3, 4, generator=g))
        batches.append({"imgs": torch.randint(0, 256, (B, 21, H, W), generator=g).float(), "bflows": bflows})
        outs.append([(bflows[:, 2 * k:2 * k + 2] + 2.0 * enlarge(torch.randn(B, 2, 5, 6, generator=g))).contiguous().cuda()
                     for k in range(n_out)])
    served = []

    def model(imgs):
        served.append(len(served))
        return outs[served[-1]]
    plain, _ = train_acc.validate(model, batches, torch.device("cuda"), None)
    served.clear()
    reads = counting_host_reads(monkeypatch)
    kept = {0: None, 5: None}                                         # visual_samples = [0, 5]: the validation has 2 batches
    got, last = train_acc.validate(model, batches, torch.device("cuda"), None, keep=kept)
    monkeypatch.undo()
    assert reads == ["cpu", "tolist"] or reads == ["cpu"], reads       # the one transfer at the end of the validation
    assert got == plain and torch.equal(last, outs[1][-1])
    assert kept[5] is None and torch.equal(kept[0], outs[0][-1][:1])
    log_dir = str(tmp_path / "logs" / "exp")
    train_acc.save_visual_samples(kept, log_dir, 1200)
    path = tmp_path / "logs" / "exp" / "val" / "im000" / "001200.png"
    assert path.is_file() and sorted(p.name for p in (tmp_path / "logs" / "exp" / "val").iterdir()) == ["im000"]
    back, filters = R.decode_png(path.read_bytes())
    assert set(filters) == {0}
    assert np.array_equal(back, viz.flow_to_image(outs[0][-1][:1])[0].cpu().numpy())
    # without the key nothing is kept and no val/ directory appears
    other = str(tmp_path / "logs" / "other")
    train_acc.save_visual_samples({int(i): None for i in train_acc.DEFAULTS["visual_samples"]}, other, 1200)
    assert not (tmp_path / "logs" / "other").exists()
