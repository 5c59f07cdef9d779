"""Fixture of the flow colour coding (reference utils/flow_viz.py): float32 flows and the uint8 pictures the REFERENCE's numpy
code paints for them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_flow_viz_golden.py <path of the reference checkout>

The reference's module is loaded from its file (numpy only), nothing of it is copied: tests/golden/flow_viz.npz holds arrays
only.  Per case: `<case>.flow` (2,H,W) float32, `<case>.img` (H,W,3) uint8, `<case>.scale` float32 (the largest radius
numpy's float32 finds, or the fixed scale), `<case>.clip` float32 (-1: none), `<case>.bgr` uint8.  The archive is written with
fixed member time stamps, so a second run reproduces the file byte for byte.

Cases (recipes: tests/flow_viz_ref.py; every case passes through flow_to_image unless noted):
    smooth_37x67, smooth_16x130    interpolate(8 randn(1, 2, 3, 4))
    noise_70x130                   5 randn
    clip_24x40                     smooth, clip_flow = 6 (negative components become 0)
    bgr_24x40                      smooth, convert_to_bgr
    fixed_24x40                    smooth at 0.3 of its largest radius: the components are divided by (scale + 1e-5) in float32
                                   here and go through flow_uv_to_colors - more than half the pixels take the 0.75 branch
    tiny_1x1, tiny_3x5_a, tiny_3x5_b   noise; seeds without a component in the comparison's tau band (asserted below)
    seam_1x4                       (1, 0), (1, -0), (2, 0), (0, 0)
    axes_1x9                       the eight axis and diagonal directions at radius 3, and (7.3, 0.9), which sets the scale
    zero_4x6                       zeros
    big300_8x16                    smooth, rescaled to a largest radius of about 300 px (r + 1e-5 == r in float32)
"""
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import flow_viz_ref as R  # noqa: E402

OUT = os.path.join(HERE, "flow_viz.npz")
TINY_SEEDS = {"tiny_1x1": (1, 1, 3), "tiny_3x5_a": (3, 5, 4), "tiny_3x5_b": (3, 5, 5)}


def cases():
    """(name, flow (2,H,W) float32 ndarray, clip or None, bgr, fixed scale or None)"""
    def np0(t):
        return t[0].numpy().astype(np.float32)
    yield "smooth_37x67", np0(R.smooth_flow(1, 37, 67, 101)), None, False, None
    yield "smooth_16x130", np0(R.smooth_flow(1, 16, 130, 102)), None, False, None
    yield "noise_70x130", np0(R.noise_flow(1, 70, 130, 103)), None, False, None
    yield "clip_24x40", np0(R.smooth_flow(1, 24, 40, 104)), 6.0, False, None
    yield "bgr_24x40", np0(R.smooth_flow(1, 24, 40, 105)), None, True, None
    f = np0(R.smooth_flow(1, 24, 40, 106))
    yield "fixed_24x40", f, None, False, np.float32(0.3) * R.max_radius32(f)
    for name, (H, W, seed) in TINY_SEEDS.items():
        yield name, np0(R.noise_flow(1, H, W, seed)), None, False, None
    yield "seam_1x4", np.array([[[1.0, 1.0, 2.0, 0.0]], [[0.0, -0.0, 0.0, 0.0]]], dtype=np.float32), None, False, None
    d = np.float32(3.0 / np.sqrt(2.0))
    yield "axes_1x9", np.array([[[3, d, 0, -d, -3, -d, 0, d, 7.3]], [[0, d, 3, d, 0, -d, -3, -d, 0.9]]], dtype=np.float32), None, False, None
    yield "zero_4x6", np.zeros((2, 4, 6), dtype=np.float32), None, False, None
    f = np0(R.smooth_flow(1, 8, 16, 107))
    yield "big300_8x16", (f * (np.float32(300.0) / R.max_radius32(f))).astype(np.float32), None, False, None


def load_reference(root):
    spec = importlib.util.spec_from_file_location("_reference_flow_viz", os.path.join(root, "utils", "flow_viz.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_npz(path, arrays):
    """np.savez without the clock: every member stamped 1980-01-01, stored uncompressed, in the given order."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as zf:
        for name, arr in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    arrays = []
    for name, flow, clip, bgr, fixed in cases():
        assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[0] == 2
        hwc = np.ascontiguousarray(flow.transpose(1, 2, 0))
        if fixed is None:
            img = ref.flow_to_image(hwc, clip_flow=clip, convert_to_bgr=bgr)
            scale = R.max_radius32(flow, clip)
        else:
            scale = np.float32(fixed)
            div = scale + np.float32(1e-5)
            assert div.dtype == np.float32
            img = ref.flow_uv_to_colors(flow[0] / div, flow[1] / div, bgr)
        assert img.dtype == np.uint8 and img.shape == flow.shape[1:] + (3,)
        e = R.expectation(flow, scale, clip)
        # what the comparison rule has to excuse in the reference's own picture: nothing but the rad-1 pixel
        plain = img[..., ::-1] if bgr else img
        off = (plain != np.floor(e["x"])) & ~e["near_one"][..., None]
        if name in TINY_SEEDS or name == "axes_1x9":
            assert not e["band"].any() and not e["near_one"].any(), name
        if name.startswith("fixed"):
            assert (R.colours64(flow, scale, clip)[2] > 1).mean() > 0.5, name
        print("%-14s %-12s band %5.2f %%  rad-1 pixels %d  reference != floor(x): %d  beyond the scale %4.1f %%" % (
            name, flow.shape[1:], 100.0 * e["band"].mean(), int(e["near_one"].sum()), int(off.sum()),
            100.0 * float((R.colours64(flow, scale, clip)[2] > 1).mean())))
        arrays += [(name + ".flow", flow), (name + ".img", img), (name + ".scale", np.float32(scale).reshape(1)),
                   (name + ".clip", np.array([-1.0 if clip is None else clip], dtype=np.float32)),
                   (name + ".bgr", np.array([int(bgr)], dtype=np.uint8))]
    write_npz(OUT, arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
