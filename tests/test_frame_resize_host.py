"""Resampling at the frame / flow-file boundary without a GPU: FrameScaler's size arithmetic and argument errors, the
High_Speed_Sintel data set on a tree written here, infer's parser, and the two new entry points' declarations, bindings and
argument checks (which come before any launch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import frame_resize_ref as Z


# (source (H, W), the size argument, the working (h, w))
SIZES = (
    ((436, 1024), {}, (436, 1024)),
    ((2160, 3840), {"size": (540, 960)}, (540, 960)),
    ((2160, 3840), {"scale": 0.25}, (540, 960)),
    ((32, 48), {"scale": 0.5}, (16, 24)),
    ((17, 33), {"scale": 0.5}, (9, 17)),                  # 8.5 and 16.5: halves round up
    ((15, 31), {"scale": 0.5}, (8, 16)),                  # 7.5 -> 8, 15.5 -> 16
    ((10, 100), {"scale": 0.5}, (8, 50)),                 # 5 -> the floor of 8
    ((9, 9), {"scale": 0.1}, (8, 8)),
    ((100, 200), {"scale": 1.5}, (150, 300)),
    ((3, 7), {"scale": 1.0}, (8, 8)),                     # the floor holds for an unchanged side too
    ((2160, 3840), {"max_side": 960}, (540, 960)),
    ((3840, 2160), {"max_side": 960}, (960, 540)),
    ((436, 1024), {"max_side": 1024}, (436, 1024)),       # equal to the longer side: unchanged
    ((436, 1024), {"max_side": 2048}, (436, 1024)),       # smaller than max_side: unchanged, never enlarged
    ((5, 7), {"max_side": 7}, (5, 7)),
    ((3, 4), {"max_side": 2}, (2, 2)),                    # 3 * 2 / 4 = 1.5 -> 2
    ((1, 4), {"max_side": 2}, (1, 2)),                    # 0.5 -> 1
    ((1, 1000), {"max_side": 10}, (1, 10)),               # 0.01 -> 0, at least 1
    ((1080, 1920), {"max_side": 1024}, (576, 1024)),
    ((437, 1025), {"max_side": 512}, (218, 512)),         # 437 * 512 / 1025 = 218.29
)


@pytest.mark.parametrize("dims,kw,want", SIZES, ids=lambda v: str(v).replace(" ", ""))
def test_frame_scaler_size_arithmetic(dims, kw, want):
    from accflow_amd.frames import FramePadder, FrameScaler, working_size
    s = FrameScaler(dims, **kw)
    assert s.size == want == working_size(dims, **kw) and all(isinstance(v, int) for v in s.size)
    assert (s.ht, s.wd) == dims and s.resizes == (want != dims)
    assert isinstance(s.padder, FramePadder) and (s.padder.ht, s.padder.wd) == want
    assert FrameScaler((2, 3) + dims, **kw).size == want                      # dims: the last two of a shape


def test_frame_scaler_argument_errors():
    from accflow_amd.frames import FrameScaler
    for kw in ({"size": (8, 8), "scale": 0.5}, {"size": (8, 8), "max_side": 8}, {"scale": 0.5, "max_side": 8},
               {"size": (8, 8), "scale": 1.0, "max_side": 8}):
        with pytest.raises(RuntimeError, match="at most one"):
            FrameScaler((16, 16), **kw)
    with pytest.raises(RuntimeError, match="interp"):
        FrameScaler((16, 16), interp="bicubic")
    for size in ((0, 8), (8, -8), (8.0, 8), (8,), "ab", 8):
        with pytest.raises(RuntimeError, match="size"):
            FrameScaler((16, 16), size=size)
    for scale in (0, -0.5, float("nan"), float("inf"), "x"):
        with pytest.raises(RuntimeError, match="scale"):
            FrameScaler((16, 16), scale=scale)
    for m in (0, -4, 8.0, True):
        with pytest.raises(RuntimeError, match="max_side"):
            FrameScaler((16, 16), max_side=m)
    # the padder's pad modes pass through
    assert FrameScaler((20, 20), scale=0.5, pad="kitti").padder._pad == [3, 3, 0, 6]
    assert FrameScaler((20, 20), scale=0.5).padder._pad == [3, 3, 3, 3]


def test_ops_refuse_before_the_library():
    """What needs no device to be refused: the operands never leave the CPU."""
    from accflow_amd import ops
    u8 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    for size in ((0, 4), (4, -1), (4.5, 4), (4,), "ab"):
        with pytest.raises(RuntimeError, match="size"):
            ops.frames_from_u8(u8, size=size)
    with pytest.raises(RuntimeError, match="interp"):
        ops.frames_from_u8(u8, size=(4, 4), interp="lanczos")
    with pytest.raises(RuntimeError, match="out must be"):
        ops.frames_from_u8(u8, size=(4, 4), out=torch.zeros((1, 3, 4, 5)))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.frames_from_u8(u8, size=(4, 4))
    flow = torch.zeros((1, 2, 8, 12))
    with pytest.raises(RuntimeError, match="crop"):
        ops.flow_resize(flow, (4, 4), crop=(0, 0, 9, 12))
    with pytest.raises(RuntimeError, match="coding"):
        ops.flow_resize(flow, (4, 4), coding="png")
    with pytest.raises(RuntimeError, match="size"):
        ops.flow_resize(flow, (4, 4.5))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.flow_resize(flow, (4, 4))


def test_entry_points_are_declared_bound_and_reject_bad_arguments():
    from accflow_amd import _lib
    header = open(os.path.join(ROOT, "include", "accflow_hip.h")).read()
    lib = _lib.load()
    for name in ("accflow_frames_from_u8_resized", "accflow_flow_resize"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
        assert callable(getattr(lib, name))
    # the arguments of accflow_frames_from_u8, then out_h, out_w, interp, then the stream
    old, new = _lib.SIGNATURES["accflow_frames_from_u8"], _lib.SIGNATURES["accflow_frames_from_u8_resized"]
    assert new == old[:-1] + [ctypes.c_int] * 3 + old[-1:]
    for word in ("(2x+1) n_in - n_out", "floor(num / den)", "f == 0 ? a : a + f (b - a)", "2^24"):
        assert word in header, word
    z, nz = ctypes.c_void_p(0), ctypes.c_void_p(256)          # (nz is never dereferenced: the checks come before any launch)

    def ingest(src=nz, out=nz, N=1, H=8, W=8, pads=(0, 0, 0, 0), oh=4, ow=4, interp=0, s_row=24):
        return lib.accflow_frames_from_u8_resized(src, 0, s_row, 0, 0, 0, 1, out, 48, N, H, W, pads[0], pads[1], pads[2], pads[3],
                                                  oh, ow, interp, z)
    assert ingest(src=z) == 1 and ingest(out=z) == 1 and ingest(out=ctypes.c_void_p(258)) == 1
    assert ingest(oh=0) == 1 and ingest(ow=0) == 1 and ingest(oh=-4) == 1 and ingest(interp=2) == 1 and ingest(interp=-1) == 1
    assert ingest(N=0) == 1 and ingest(N=65536) == 1 and ingest(H=0) == 1 and ingest(pads=(0, 0, -1, 0)) == 1 and ingest(s_row=-24) == 1
    assert ingest(oh=32769) == 1 and ingest(ow=32769) == 1 and ingest(H=32769) == 1 and ingest(W=32769) == 1
    assert ingest(H=4096, W=4096, oh=1, ow=1, interp=1) == 1          # a 4097 x 4097 area window: 2^24 pixels or more
    assert ingest(H=32768, W=32768, oh=8, ow=8, interp=1) == 1

    def resize(flow=nz, out=nz, Hp=8, Wp=12, crop=(0, 0, 8, 12), H=4, W=4, coding=2, N=1, o_bs=0):
        return lib.accflow_flow_resize(flow, 2 * Hp * Wp, Hp, Wp, crop[0], crop[1], crop[2], crop[3], H, W, out, o_bs, coding, 64.0, 0,
                                       N, z)
    assert resize(flow=z) == 1 and resize(out=z) == 1 and resize(N=0) == 1 and resize(Hp=0) == 1
    for crop in ((0, 0, 9, 12), (0, 0, 8, 13), (-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (5, 0, 4, 4), (0, 9, 4, 4)):
        assert resize(crop=crop) == 1, crop
    assert resize(H=0) == 1 and resize(W=-1) == 1 and resize(H=32769) == 1 and resize(coding=3) == 1 and resize(coding=-1) == 1
    assert resize(Hp=32769, Wp=4, crop=(0, 0, 32769, 4)) == 1
    assert resize(out=ctypes.c_void_p(258)) == 1 and resize(out=ctypes.c_void_p(258), coding=0) == 1
    assert resize(out=ctypes.c_void_p(257), coding=1) == 1 and resize(N=2, o_bs=6, coding=2) == 1 and resize(N=2, o_bs=-8) == 1


def test_reference_geometry_is_float64_interpolate():
    """The integer restatement the GPU tests' bounds rest on, against the yardstick itself."""
    g = torch.Generator().manual_seed(0)
    for (n_in, n_out) in ((13, 8), (7, 16), (21, 10), (1, 8), (5, 17), (19, 12), (8, 8)):
        x = torch.rand(1, 1, 1, n_in, generator=g, dtype=torch.float64) * 255
        want = Z.bilinear_f64(x, (1, n_out))[0, 0, 0]
        got = torch.tensor([float(x[0, 0, 0, a]) + float(f) * (float(x[0, 0, 0, b]) - float(x[0, 0, 0, a])) for a, b, f in Z.taps(n_in, n_out)],
                           dtype=torch.float64)
        assert float((got - want).abs().max()) <= 1e-11, (n_in, n_out)
    assert Z.touched(8, 8, 3) == [3] and Z.touched(8, 16, 3) == [5, 6, 7, 8] and Z.touched(8, 16, 0) == [0, 1, 2]


# ------------------------------------------------------------------------------------------------
# High-Speed Sintel


def write_sample(root, n_hs, H, W, H0, W0, seed, ext=".png"):
    from accflow_amd import frames, viz
    g = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "2_imgs")), os.makedirs(os.path.join(root, "43_imgs"))
    hs = [g.integers(0, 256, (H0, W0, 3), dtype=np.uint8) for _ in range(n_hs)]
    for k, im in enumerate(hs):
        viz.write_png(os.path.join(root, "43_imgs", "frame_%04d%s" % (k, ext)), im)
    ori = [g.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2)]
    for k, im in enumerate(ori):
        viz.write_png(os.path.join(root, "2_imgs", "frame_%04d.png" % k), im)
    flow = g.standard_normal((H, W, 2)).astype(np.float32)
    frames.write_flo(os.path.join(root, "flow.flo"), flow)
    occ = (g.random((H, W)) < 0.3).astype(np.uint8) * 255
    viz.write_png(os.path.join(root, "occ.png"), np.ascontiguousarray(np.repeat(occ[..., None], 3, axis=2)))
    return hs, ori, flow, occ


def test_high_speed_sintel(tmp_path):
    from accflow_amd.data.dataset import High_Speed_Sintel, fetch_sintel_dataloader
    from data import dataset as drop_in
    assert drop_in.High_Speed_Sintel is High_Speed_Sintel and drop_in.fetch_sintel_dataloader is fetch_sintel_dataloader
    H, W, H0, W0 = 12, 20, 18, 30
    written = {name: write_sample(str(tmp_path / name), 7, H, W, H0, W0, seed) for seed, name in enumerate(("alley", "bamboo", "cave"))}
    ds = High_Speed_Sintel(str(tmp_path), 3)
    assert len(ds) == 3 and [os.path.basename(p) for p in ds.sample_list] == ["alley", "bamboo", "cave"]
    for index, name in enumerate(("alley", "bamboo", "cave")):
        hs, ori, flow, occ = written[name]
        s = ds[index]
        assert sorted(s) == ["gt_flow", "hs_sintel_u8", "occ_mask", "sintel_imgs"]
        assert s["gt_flow"].shape == (2, H, W) and s["gt_flow"].dtype == torch.float32
        assert np.array_equal(s["gt_flow"].numpy(), flow.transpose(2, 0, 1))
        assert s["occ_mask"].shape == (1, H, W) and s["occ_mask"].dtype == torch.float32
        assert np.array_equal(s["occ_mask"].numpy()[0], (occ == 255).astype(np.float32))
        assert len(s["sintel_imgs"]) == 2
        for got, want in zip(s["sintel_imgs"], ori):
            assert got.shape == (3, H, W) and got.dtype == torch.float32 and np.array_equal(got.numpy(), want.transpose(2, 0, 1))
        # every third frame, both ends included, as decoded: uint8, the files' own size
        assert len(s["hs_sintel_u8"]) == 3
        for got, want in zip(s["hs_sintel_u8"], hs[::3]):
            assert got.shape == (H0, W0, 3) and got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
    assert [len(High_Speed_Sintel(str(tmp_path), i)[0]["hs_sintel_u8"]) for i in (1, 2, 6)] == [7, 4, 2]
    for interv in (4, 5):
        with pytest.raises(ValueError, match="does not divide"):
            High_Speed_Sintel(str(tmp_path), interv)[0]
    with pytest.raises(ValueError, match="interv"):
        High_Speed_Sintel(str(tmp_path), 0)
    ds = High_Speed_Sintel(str(tmp_path), 6, blacklist=["bamboo"])
    assert [os.path.basename(p) for p in ds.sample_list] == ["alley", "cave"]
    loader, ds = fetch_sintel_dataloader(str(tmp_path), interv=2, batch=2, blacklist=["cave"])
    batches = list(loader)
    assert len(ds) == 2 and len(batches) == 1
    b = batches[0]
    assert b["gt_flow"].shape == (2, 2, H, W) and b["occ_mask"].shape == (2, 1, H, W)
    assert len(b["hs_sintel_u8"]) == 4 and b["hs_sintel_u8"][0].shape == (2, H0, W0, 3) and b["hs_sintel_u8"][0].dtype == torch.uint8
    assert len(b["sintel_imgs"]) == 2 and b["sintel_imgs"][1].shape == (2, 3, H, W)


def test_high_speed_sintel_refuses_jpeg(tmp_path):
    from accflow_amd.data.dataset import High_Speed_Sintel
    write_sample(str(tmp_path / "alley"), 3, 8, 8, 8, 8, 0, ext=".jpg")          # (PNG bytes under a .jpg name would decode:
    with open(str(tmp_path / "alley" / "43_imgs" / "frame_0000.jpg"), "wb") as f:     # give the first one a JPEG's start)
        f.write(b"\xff\xd8\xff\xe0" + b"\0" * 32)
    with pytest.raises(ValueError, match="JPEG and other formats are not supported"):
        High_Speed_Sintel(str(tmp_path), 1)[0]


# ------------------------------------------------------------------------------------------------
# parsers


def test_infer_parser():
    from accflow_amd import infer
    ap = infer.build_parser()
    a = ap.parse_args(["--frames", "in", "--out", "o"])
    assert (a.size, a.scale, a.max_side, a.interp, a.flows_at) == (None, None, None, "bilinear", "source")
    a = ap.parse_args(["--frames", "in", "--out", "o", "--size", "1024x436", "--interp", "area", "--flows-at", "working"])
    assert a.size == (436, 1024) and a.interp == "area" and a.flows_at == "working"          # WxH on the line, (h, w) inside
    assert ap.parse_args(["--frames", "in", "--out", "o", "--scale", "0.25"]).scale == 0.25
    assert ap.parse_args(["--frames", "in", "--out", "o", "--max-side", "960"]).max_side == 960
    for bad in (["--size", "1024"], ["--size", "0x436"], ["--size", "axb"], ["--interp", "cubic"], ["--flows-at", "both"],
                ["--size", "8x8", "--scale", "0.5"], ["--scale", "0.5", "--max-side", "8"], ["--max-side", "1.5"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["--frames", "in", "--out", "o"] + bad)
    assert infer.parse_size("960X540") == (540, 960)


def test_eval_hs_sintel_parser():
    from accflow_amd import eval_hs_sintel
    ap = eval_hs_sintel.build_parser()
    a = ap.parse_args(["--root", "d"])
    assert (a.root, a.interv, a.acc, a.ofe, a.acc_ckpt, a.ofe_ckpt) == ("d", 6, "acc", "raft", None, None)
    a = ap.parse_args(["--root", "d", "--interv", "7", "--acc", "direct", "--ofe", "gma", "--ofe_ckpt", "w.pth"])
    assert (a.interv, a.acc, a.ofe, a.ofe_ckpt) == (7, "direct", "gma", "w.pth")
    with pytest.raises(SystemExit):
        ap.parse_args([])
