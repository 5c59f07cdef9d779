"""The flow colour coding without a GPU: the float64 restatement of tests/flow_viz_ref.py against the reference's pictures
(tests/golden/flow_viz.npz) under the derived rule, viz.write_png against a decoder written here (and PIL where it imports),
train_acc's `visual_samples` option, the C entries' argument checks and what viz.flow_to_image refuses."""
import ctypes
import os

import numpy as np
import pytest
import torch

import flow_viz_ref as R

GENERATED = ("smooth_37x67", "smooth_16x130", "noise_70x130", "clip_24x40", "bgr_24x40", "fixed_24x40")
EXACT = ("tiny_1x1", "tiny_3x5_a", "tiny_3x5_b", "axes_1x9", "zero_4x6")
HAND_MADE = ("seam_1x4", "big300_8x16")


def case_of(g, name):
    clip = float(g[name + ".clip"][0])
    return g[name + ".flow"], g[name + ".img"], g[name + ".scale"][0], (None if clip < 0 else clip), bool(g[name + ".bgr"][0])


def test_wheel_from_the_definition():
    w = R.WHEEL
    assert w.shape == (55, 3) and w.min() == 0 and w.max() == 255
    assert w[0].tolist() == [255, 0, 0] and w[54].tolist() == [255, 0, 43] and w[15].tolist() == [255, 255, 0]
    assert w[14].tolist() == [255, 238, 0] and w[21].tolist() == [0, 255, 0] and w[25].tolist() == [0, 255, 255]
    assert w[36].tolist() == [0, 0, 255] and w[49].tolist() == [255, 0, 255]
    # on every segment one channel is 255 at both ends of every step: a third of all components is saturated
    nxt = np.roll(w, -1, axis=0)
    assert (((w == 255) & (nxt == 255)).sum(axis=1) >= 1).all()


@pytest.mark.parametrize("name", GENERATED + EXACT + HAND_MADE)
def test_restatement_vs_reference_pictures(golden, name):
    g = golden("flow_viz")
    flow, img, scale, clip, bgr = case_of(g, name)
    if not name.startswith("fixed"):
        assert R.max_radius32(flow, clip).tobytes() == np.float32(scale).tobytes()
    n_band, n_one, worst = R.check_image(img, flow, scale, clip=clip, bgr=bgr, exact=name in EXACT, caps=name in GENERATED, what=name)
    print("%s: %d band components, %d rad-1 pixels, reference off floor(x) by at most %.2e" % (name, n_band, n_one, worst))
    if name == "seam_1x4":
        assert img[0].tolist() == [[255, 127, 127], [255, 127, 149], [255, 0, 0], [255, 255, 255]]
    if name == "zero_4x6":
        assert (img == 255).all()
    if name == "fixed_24x40":
        assert (R.colours64(flow, scale)[2] > 1).mean() > 0.5


def test_saturated_share_and_unknown_pixels():
    g = np.random.default_rng(7)
    flow = (5 * g.standard_normal((2, 40, 50))).astype(np.float32)
    s = R.max_radius32(flow)
    x = R.expectation(flow, s)["x"]
    assert abs((x == 255).mean() - 1 / 3) < 0.01                       # the saturated channel: exactly 255 in float64 too
    bad = flow.copy()
    bad[0, 3, 4], bad[1, 5, 6], bad[0, 7, 8], bad[1, 9, 9] = np.nan, np.inf, -np.inf, 1e10
    assert R.max_radius32(bad).tobytes() == R.max_radius32(np.where(R.unknown(bad), 0, bad).astype(np.float32)).tobytes()
    e = R.expectation(bad, s)
    assert int(e["unknown"].sum()) == 4 and (e["x"][e["unknown"]] == 0).all() and (e["hi"][e["unknown"]] == 0).all()
    assert R.max_radius32(np.full((2, 3, 3), np.nan, dtype=np.float32)) == 0
    # np.clip keeps the sign of a zero and turns negative components into +0
    c = R.clip32(np.array([-0.0, 0.0, -2.0, 9.0], dtype=np.float32), 5.0)
    assert c.tolist() == [0.0, 0.0, 0.0, 5.0] and np.signbit(c).tolist() == [True, False, False, False]


# ------------------------------------------------------------------------------------------------
# write_png


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (37, 67)])
def test_write_png(tmp_path, shape):
    from accflow_amd import viz
    img = np.random.default_rng(shape[0]).integers(0, 256, shape + (3,), dtype=np.uint8)
    img[0, 0] = (255, 0, 43)
    for k, src in enumerate((img, torch.from_numpy(img))):
        path = str(tmp_path / ("a%d.png" % k))
        viz.write_png(path, src)
        back, filters = R.decode_png(open(path, "rb").read())
        assert back.dtype == np.uint8 and np.array_equal(back, img) and set(filters) == {0}
        try:
            from PIL import Image
        except ImportError:
            continue
        with Image.open(path) as im:
            assert im.mode == "RGB" and im.size == (shape[1], shape[0]) and np.array_equal(np.asarray(im), img)


def test_write_png_refuses_other_images(tmp_path):
    from accflow_amd import viz
    path = str(tmp_path / "x.png")
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32),
                np.zeros((3, 4, 4), np.uint8), np.zeros((0, 4, 3), np.uint8), torch.zeros(4, 4, 3)):
        with pytest.raises(ValueError):
            viz.write_png(path, bad)
    assert not os.path.exists(path)


# ------------------------------------------------------------------------------------------------
# options, argument checks


def test_parse_options_visual_samples(tmp_path):
    from accflow_amd import train_acc
    plain, ref = tmp_path / "plain.yml", tmp_path / "ref.yml"
    plain.write_text("exp_name: acc|raft\n")
    ref.write_text("exp_name: acc|raft\nvisual_samples: [0, 1, 2]\n")
    assert train_acc.parse_options(str(plain)).visual_samples == []
    assert train_acc.parse_options(str(ref)).visual_samples == [0, 1, 2]
    assert train_acc.DEFAULTS["visual_samples"] == []


def test_entry_points_reject_bad_arguments():
    from accflow_amd import _lib
    lib = _lib.load()
    assert "accflow_flow_maxrad_ws_bytes" in _lib.RETURNS_LONGLONG
    z, nz = ctypes.c_void_p(0), ctypes.c_void_p(256)        # (nz is never dereferenced: the checks come before any launch)
    mx, rgb, wsb = lib.accflow_flow_maxrad_f32, lib.accflow_flow_to_rgb_u8, lib.accflow_flow_maxrad_ws_bytes
    sizes = ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, -8, 8), (1, 8, -3), (1, 65536, 65536), (65536, 8, 8))
    for B, H, W in sizes:
        assert wsb(B, H, W) == 0
    assert wsb(1, 1, 1) == 4 and wsb(7, 1, 1) == 28
    assert wsb(1, 64, 64) == 4 and wsb(1, 64, 65) == 8 and wsb(2, 70, 130) == 2 * 3 * 4     # runs of 4096 pixels
    assert wsb(5, 264, 520) * 3 == wsb(3, 264, 520) * 5                                     # the cut does not depend on B
    ok = [nz, 128, -1.0, 0, nz, nz, 1, 8, 8, z]
    for i in (0, 4, 5):
        a = list(ok)
        a[i] = z
        assert mx(*a) == 1, i
    for B, H, W in sizes:
        a = list(ok)
        a[6:9] = [B, H, W]
        assert mx(*a) == 1, (B, H, W)
    ok = [nz, 128, nz, -1.0, nz, 192, 0, 0, 1, 8, 8, z]
    for i in (0, 2, 4):
        a = list(ok)
        a[i] = z
        assert rgb(*a) == 1, i
    for B, H, W in sizes:
        a = list(ok)
        a[8:11] = [B, H, W]
        assert rgb(*a) == 1, (B, H, W)
    for ptr, bs, B in ((257, 192, 1), (258, 192, 2), (256, 193, 2), (256, 194, 3)):         # planar and not dword-aligned
        a = list(ok)
        a[4], a[5], a[6], a[8] = ctypes.c_void_p(ptr), bs, 1, B
        assert rgb(*a) == 1, (ptr, bs, B)


def test_flow_to_image_refuses_cpu_tensors_and_bad_arguments(monkeypatch):
    from accflow_amd import _lib, ops, viz

    def untouchable():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", untouchable)
    f = torch.zeros(2, 2, 8, 12)
    for t in (f, f[0]):
        with pytest.raises(RuntimeError, match="MI355X"):
            viz.flow_to_image(t)
    with pytest.raises(RuntimeError, match="MI355X"):
        viz.save_flow(f, "unused.png")
    with pytest.raises(RuntimeError, match=r"\(B,2,H,W\)"):
        viz.flow_to_image(torch.zeros(8, 12))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.flow_maxrad(f)
    with pytest.raises(RuntimeError, match=r"\(B,2,H,W\)"):
        ops.flow_maxrad(torch.zeros(2, 3, 8, 12))
    with pytest.raises(RuntimeError, match="clip"):
        ops.flow_maxrad(f, clip=-1.0)
    with pytest.raises(RuntimeError, match="layout"):
        ops.flow_to_rgb(f, torch.zeros(2), layout="nhwc")
    with pytest.raises(RuntimeError, match="maxrad"):
        ops.flow_to_rgb(f, torch.zeros(3))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.flow_to_rgb(f, torch.zeros(2), out=torch.zeros(2, 3, 8, 12, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.flow_to_rgb(f, torch.zeros(2))
    assert not os.path.exists("unused.png")
