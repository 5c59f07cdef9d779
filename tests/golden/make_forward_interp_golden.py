"""Fixture of forward_interpolate (reference networks/raft/utils/utils.py:31-63): input flows and what the REFERENCE's function
returns for them (scipy.interpolate.griddata, method="nearest", on the CPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_forward_interp_golden.py <path of the reference checkout>

The reference's utils module is loaded from its file (it needs torch, numpy and scipy only), nothing of it is copied: the
fixture tests/golden/forward_interp.npz holds arrays only - `<case>.flow` (2, h, w) float32 and `<case>.out` (2, h, w) float32.
The archive is written with fixed member time stamps, so a second run reproduces the file byte for byte.

Cases (one torch.Generator seeded with 0, drawn in this order):
    rand3_16x32    randn * 3
    rand3_33x47    randn * 3        (odd sizes; P = 1 551 is more than one LDS chunk of the kernel plus a tail)
    rand12_13x19   randn * 12       (most sources leave the frame)
    zero_16x32     zeros            (row 0 and column 0 are invalid: the bounds are strict)
    shift_16x32    constant (+3, -2)
    smooth_33x47   dx = 2.5 + 0.05 x, dy = -1.5 + 0.03 y
"""
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "forward_interp.npz")


def cases():
    g = torch.Generator().manual_seed(0)
    yield "rand3_16x32", torch.randn(2, 16, 32, generator=g) * 3
    yield "rand3_33x47", torch.randn(2, 33, 47, generator=g) * 3
    yield "rand12_13x19", torch.randn(2, 13, 19, generator=g) * 12
    yield "zero_16x32", torch.zeros(2, 16, 32)
    shift = torch.empty(2, 16, 32)
    shift[0], shift[1] = 3.0, -2.0
    yield "shift_16x32", shift
    ys, xs = torch.meshgrid(torch.arange(33.0), torch.arange(47.0), indexing="ij")
    yield "smooth_33x47", torch.stack([2.5 + 0.05 * xs, -1.5 + 0.03 * ys], dim=0)


def load_reference(root):
    path = os.path.join(root, "networks", "raft", "utils", "utils.py")
    spec = importlib.util.spec_from_file_location("_reference_raft_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.forward_interpolate


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
    forward_interpolate = load_reference(sys.argv[1])
    arrays = []
    for name, flow in cases():
        flow = flow.float().contiguous()
        out = forward_interpolate(flow)
        assert out.dtype == torch.float32 and out.shape == flow.shape
        arrays += [(name + ".flow", flow.numpy()), (name + ".out", out.numpy())]
        print("%-14s %s" % (name, tuple(flow.shape)))
    write_npz(OUT, arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
