"""The frame / flow-file boundary without a GPU: FramePadder's arithmetic against InputPadder's, .flo files against the bytes the
reference's writeFlow produced (tests/golden/frame_io.npz), the PNG / PPM reader against an encoder written for the tests
(tests/frame_io_ref.py) and against PIL where it imports, write_png16, what the two ops refuse before they touch the device,
and the new C entries' argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

import frame_io_ref as R


def test_pads_equal_input_padder():
    from accflow_amd.frames import FramePadder
    from accflow_amd.networks.raft.utils.utils import InputPadder
    for mode in ("sintel", "kitti"):
        for H in range(1, 41):
            for W in range(1, 41):
                p, q = FramePadder((H, W), mode), InputPadder((1, 3, H, W), mode)
                assert p._pad == q._pad, (mode, H, W)
                l, r, t, b = p._pad
                assert (H + t + b) % 8 == 0 and (W + l + r) % 8 == 0 and p.crop == (t, l, H, W)
                x = torch.zeros(1, 2, H + t + b, W + l + r)
                assert p.unpad(x).shape == q.unpad(x).shape == (1, 2, H, W)
                assert p.unpad(x).data_ptr() == q.unpad(x).data_ptr()          # a view of the same window
    assert FramePadder((3, 436, 1024))._pad == [0, 0, 2, 2] and FramePadder((375, 1242), "kitti")._pad == [3, 3, 0, 1]


# ------------------------------------------------------------------------------------------------
# .flo


@pytest.mark.parametrize("name", ["flo_3x5", "flo_13x21"])
def test_flo_against_the_reference_bytes(golden, tmp_path, name):
    from accflow_amd import frames
    g = golden("frame_io")
    flow, want = g[name + ".flow"], g[name + ".bytes"].tobytes()
    assert flow.dtype == np.float32 and flow.shape[2] == 2 and len(want) == 12 + flow.nbytes
    for k, src in enumerate((flow, torch.from_numpy(flow))):
        path = str(tmp_path / ("%s_%d.flo" % (name, k)))
        frames.write_flo(path, src)
        assert open(path, "rb").read() == want
        back = frames.read_flo(path)
        assert back.dtype == np.float32 and back.shape == flow.shape and back.tobytes() == flow.tobytes()


def test_flo_refuses(tmp_path):
    from accflow_amd import frames
    path = str(tmp_path / "x.flo")
    for bad in (np.zeros((4, 4), np.float32), np.zeros((2, 4, 4), np.float32), np.zeros((4, 4, 2), np.float64), np.zeros((0, 4, 2), np.float32)):
        with pytest.raises(ValueError):
            frames.write_flo(path, bad)
    assert not os.path.exists(path)
    open(path, "wb").write(b"HEIP" + b"\0" * 20)                 # (b"PIEH" is the tag itself)
    with pytest.raises(ValueError, match="tag"):
        frames.read_flo(path)
    frames.write_flo(path, np.zeros((3, 5, 2), np.float32))
    data = open(path, "rb").read()
    open(path, "wb").write(data[:-4])
    with pytest.raises(ValueError, match="payload"):
        frames.read_flo(path)


# ------------------------------------------------------------------------------------------------
# PNG, PPM


def picture(H, W, C, seed):
    """smooth ramps plus noise: every filter has something to predict, and every byte value occurs somewhere"""
    g = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    img = np.stack([(7 * xs + 3 * ys + 40 * c) % 256 for c in range(C)], axis=-1) + g.integers(-9, 10, (H, W, C))
    img = (img % 256).astype(np.uint8)
    img[0, 0], img[-1, -1] = 255, 0
    return img


def as_rgb(img):
    return np.repeat(img, 3, axis=2) if img.shape[2] == 1 else np.ascontiguousarray(img[:, :, :3])


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (37, 67)])
def test_read_image_returns_what_write_png_wrote(tmp_path, shape):
    from accflow_amd import frames, viz
    img = picture(shape[0], shape[1], 3, shape[0])
    path = str(tmp_path / "a.png")
    viz.write_png(path, img)
    back = frames.read_image(path)
    assert back.dtype == np.uint8 and back.flags.c_contiguous and np.array_equal(back, img)


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("filt", list(R.FILTERS))
def test_read_image_every_filter(tmp_path, filt, channels):
    from accflow_amd import frames
    img = picture(11, 17, channels, 10 * channels + R.FILTERS[filt])
    data = R.encode_png(img, R.FILTERS[filt])
    back, filters = R.decode_png(data)                         # the encoder against the tests' own decoder first
    assert np.array_equal(back, img) and set(filters) == {R.FILTERS[filt]}
    path = str(tmp_path / "f.png")
    open(path, "wb").write(data)
    got = frames.read_image(path)
    assert got.dtype == np.uint8 and got.shape == (11, 17, 3) and np.array_equal(got, as_rgb(img))
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert np.array_equal(np.asarray(im.convert("RGB")), got)


def test_read_image_mixed_filters_and_split_idat(tmp_path):
    from accflow_amd import frames
    img = picture(13, 9, 3, 5)
    data = R.encode_png(img, [y % 5 for y in range(13)], idat_split=20)
    assert data.count(b"IDAT") == 2
    path = str(tmp_path / "m.png")
    open(path, "wb").write(data)
    assert np.array_equal(frames.read_image(path), img)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert np.array_equal(np.asarray(im.convert("RGB")), img)


def test_read_image_refuses(tmp_path):
    from accflow_amd import frames
    img = picture(4, 6, 3, 1)
    path = str(tmp_path / "bad.png")
    cases = (("interlaced", R.encode_png(img, 0, interlace=1)),
             ("bit depth 16", R.encode_png(img.astype(np.uint16) * 257, 0, depth=16)),
             ("checksum", R.encode_png(img, 0)[:-20] + b"\xff" + R.encode_png(img, 0)[-19:]),
             ("neither a PNG", b"\xff\xd8\xff\xe0" + b"\0" * 32),
             ("neither a PNG", b"P3\n1 1\n255\n1 2 3\n"),
             ("maxval", b"P6\n1 1\n65535\n" + b"\0" * 6),
             ("pixel data", b"P6\n2 2\n255\n" + b"\0" * 11))
    for reason, data in cases:
        open(path, "wb").write(data)
        with pytest.raises(ValueError, match=reason):
            frames.read_image(path)


def test_read_ppm_with_comments(tmp_path):
    from accflow_amd import frames
    img = picture(5, 7, 3, 2)
    path = str(tmp_path / "c.ppm")
    for header in (b"P6\n7 5\n255\n", b"P6\n# made by hand\n7 5\n255\n", b"P6 7 # width\n# a line of its own\n  5\n#x\n255\n", b"P6\r\n7\t5 255 "):
        open(path, "wb").write(header + img.tobytes())
        assert np.array_equal(frames.read_image(path), img), header
    # the byte after the maxval's single whitespace is data, even when it looks like whitespace or a comment
    img[0, 0] = (ord("#"), ord(" "), ord("\n"))
    open(path, "wb").write(b"P6\n7 5\n255\n" + img.tobytes())
    assert np.array_equal(frames.read_image(path), img)


def test_load_frames(tmp_path):
    from accflow_amd import frames, viz
    imgs = [picture(6, 10, 3, k) for k in range(3)]
    paths = []
    for k, im in enumerate(imgs):
        paths.append(str(tmp_path / ("%02d.png" % k)))
        viz.write_png(paths[-1], im)
    got = frames.load_frames(paths, "cpu")
    assert got.dtype == torch.uint8 and got.shape == (3, 6, 10, 3) and np.array_equal(got.numpy(), np.stack(imgs))
    other = str(tmp_path / "other.png")
    viz.write_png(other, picture(6, 11, 3, 9))
    with pytest.raises(ValueError, match="6 x 11"):
        frames.load_frames(paths + [other], "cpu")
    with pytest.raises(ValueError, match="no frames"):
        frames.load_frames([], "cpu")


@pytest.mark.parametrize("shape", [(1, 1), (5, 7)])
def test_write_png16_round_trip(tmp_path, shape):
    from accflow_amd import frames
    g = np.random.default_rng(3)
    img = g.integers(0, 65536, shape + (3,), dtype=np.uint16)
    img[0, 0] = (0x0102, 0xFF00, 1)
    be = img.byteswap()                                        # what flow_export(big_endian=True) leaves in memory on this host
    assert be.tobytes() == img.astype(">u2").tobytes()
    for k, src in enumerate((be, torch.from_numpy(be.view(np.int16)), torch.from_numpy(be))):
        path = str(tmp_path / ("k%d.png" % k))
        frames.write_png16(path, src)
        back, filters = R.decode_png(open(path, "rb").read())
        assert back.dtype == np.uint16 and np.array_equal(back, img) and set(filters) == {0}
        try:
            from PIL import Image
        except ImportError:
            continue
        with Image.open(path) as im:
            assert im.size == (shape[1], shape[0]) and im.mode in ("RGB", "RGB;16", "I;16")
    with pytest.raises(ValueError):
        frames.write_png16(str(tmp_path / "no.png"), np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(ValueError):
        frames.write_png16(str(tmp_path / "no.png"), np.zeros((4, 4), np.uint16))


def test_tests_own_codec_depth16():
    img = np.random.default_rng(4).integers(0, 65536, (4, 5, 3), dtype=np.uint16)
    for f in range(5):
        back, filters = R.decode_png(R.encode_png(img, f, depth=16))
        assert np.array_equal(back, img) and set(filters) == {f}


# ------------------------------------------------------------------------------------------------
# argument checks


def test_ops_refuse_before_the_device(monkeypatch):
    from accflow_amd import _lib, frames, ops

    def untouchable():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", untouchable)
    u8 = torch.zeros(2, 8, 12, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.frames_from_u8(u8)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.frames_from_u8(u8.permute(0, 3, 1, 2).contiguous(), layout="chw", pad=(1, 2, 3, 4))
    with pytest.raises(RuntimeError, match="CUDA"):
        frames.FramePadder((8, 12)).ingest(u8)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.frames_from_u8(u8.float())
    with pytest.raises(RuntimeError, match=r"\(N,H,W,3\)"):
        ops.frames_from_u8(u8[0])
    with pytest.raises(RuntimeError, match=r"\(N,3,H,W\)"):
        ops.frames_from_u8(u8, layout="chw")
    with pytest.raises(RuntimeError, match="layout"):
        ops.frames_from_u8(u8, layout="nhwc")
    for pad in ((0, 0, -1, 0), (1, 2, 3), (0, 0, 0, 1.5), 3):
        with pytest.raises(RuntimeError, match="pad"):
            ops.frames_from_u8(u8, pad=pad)
    with pytest.raises(RuntimeError, match="adjacent"):
        ops.frames_from_u8(u8[:, :, ::2])
    with pytest.raises(RuntimeError, match="adjacent"):
        ops.frames_from_u8(u8.permute(0, 3, 1, 2), layout="chw")      # a packed frame seen as planes: a row's bytes are 3 apart
    with pytest.raises(RuntimeError, match="out must be"):
        ops.frames_from_u8(u8, pad=(1, 0, 0, 0), out=torch.zeros(2, 3, 8, 12))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.frames_from_u8(u8, out=torch.zeros(2, 3, 8, 12, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="made for"):
        frames.FramePadder((8, 16)).ingest(u8)

    f = torch.zeros(2, 2, 8, 12)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.flow_export(f)
    with pytest.raises(RuntimeError, match="CUDA"):
        frames.FramePadder((5, 9)).export(torch.zeros(1, 2, 8, 16), coding="u16")
    with pytest.raises(RuntimeError, match="coding"):
        ops.flow_export(f, coding="u8")
    with pytest.raises(RuntimeError, match=r"\(B,2,H,W\)"):
        ops.flow_export(torch.zeros(2, 3, 8, 12))
    with pytest.raises(RuntimeError, match=r"\(B,2,H,W\)"):
        ops.flow_export(f[0])
    for crop in ((0, 0, 9, 12), (-1, 0, 4, 4), (0, 10, 4, 4), (0, 0, 0, 4), (1, 2, 3)):
        with pytest.raises(RuntimeError, match="crop"):
            ops.flow_export(f, crop=crop)
    with pytest.raises(RuntimeError, match="scale"):
        ops.flow_export(f, coding="u16", scale=0.0)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.flow_export(f, out=torch.zeros(2, 8, 12, 3))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.flow_export(f, coding="u16", out=torch.zeros(2, 8, 12, 3))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.flow_export(f, crop=(1, 1, 4, 4), out=torch.zeros(2, 8, 12, 2))
    with pytest.raises(RuntimeError, match="dense"):
        ops.flow_export(f, out=torch.zeros(2, 8, 12, 4)[..., :2])


def test_new_symbols_and_entry_points_reject_bad_arguments():
    from accflow_amd import _lib
    from accflow_amd.build import SOURCES
    assert "frame_io.hip" in SOURCES
    for name, nargs in (("accflow_frames_from_u8", 17), ("accflow_flow_export", 15)):
        assert len(_lib.SIGNATURES[name]) == nargs and name not in _lib.RETURNS_LONGLONG
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "accflow_hip.h")).read()
    assert "int accflow_frames_from_u8(" in header and "int accflow_flow_export(" in header
    lib = _lib.load()
    z, nz = ctypes.c_void_p(0), ctypes.c_void_p(256)           # (nz is never dereferenced: the checks come before any launch)
    ingest, export = lib.accflow_frames_from_u8, lib.accflow_flow_export
    sizes = ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, -8, 8), (1, 8, -3), (1, 65536, 65536), (65536, 8, 8))
    ok = [nz, 288, 36, 0, 0, 0, 1, nz, 288, 1, 8, 12, 0, 0, 0, 0, z]
    for i in (0, 7):
        a = list(ok)
        a[i] = z
        assert ingest(*a) == 1, i
    for N, H, W in sizes:
        a = list(ok)
        a[9:12] = [N, H, W]
        assert ingest(*a) == 1, (N, H, W)
    for i in (12, 13, 14, 15):
        a = list(ok)
        a[i] = -1
        assert ingest(*a) == 1, i
    for i, v in ((14, 2 ** 31 - 8), (12, 2 ** 31 - 12), (1, -288), (2, -36), (7, ctypes.c_void_p(258))):   # padded size, strides, out off a dword
        a = list(ok)
        a[i] = v
        assert ingest(*a) == 1, (i, v)
    ok = [nz, 192, 8, 12, 0, 0, 8, 12, nz, 768, 0, 64.0, 0, 1, z]
    for i in (0, 8):
        a = list(ok)
        a[i] = z
        assert export(*a) == 1, i
    for N, H, W in sizes:
        a = list(ok)
        a[13], a[2], a[3] = N, H, W
        assert export(*a) == 1, (N, H, W)
    for crop in ((0, 0, 9, 12), (0, 0, 8, 13), (1, 0, 8, 12), (0, 1, 8, 12), (-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0),
                 (2 ** 31 - 1, 0, 2, 2), (0, 2 ** 31 - 1, 2, 2)):
        a = list(ok)
        a[4:8] = crop
        assert export(*a) == 1, crop
    for coding in (-1, 2):
        a = list(ok)
        a[10] = coding
        assert export(*a) == 1, coding
    for ptr, bs, coding, N in ((258, 768, 0, 1), (256, 770, 0, 2), (257, 576, 1, 1), (256, 577, 1, 2), (256, -768, 0, 2)):
        a = list(ok)
        a[8], a[9], a[10], a[13] = ctypes.c_void_p(ptr), bs, coding, N
        assert export(*a) == 1, (ptr, bs, coding, N)
