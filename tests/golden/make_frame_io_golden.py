"""Fixture of the flow files (reference utils/frame_utils.py): float32 flows and the bytes the REFERENCE's writeFlow puts
into a .flo file for them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_frame_io_golden.py <path of the reference checkout>

The reference's module is loaded from its file, nothing of it is copied: tests/golden/frame_io.npz holds arrays only.  Per
case `<case>.flow` (H,W,2) float32 and `<case>.bytes` uint8, the whole file.  frame_utils imports cv2, PIL, einops and torch at
its top; writeFlow needs none of them, so whichever does not import here is replaced by an empty stub module for the load.
The archive is written with fixed member time stamps, so a second run reproduces the file byte for byte.  Not needed at
test time.

Cases: flo_3x5 and flo_13x21, 20 * standard_normal from numpy's default_rng(seed 31 and 32), float32.
"""
import importlib
import importlib.util
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "frame_io.npz")
CASES = (("flo_3x5", 3, 5, 31), ("flo_13x21", 13, 21, 32))


def case_flow(H, W, seed):
    return (20 * np.random.default_rng(seed).standard_normal((H, W, 2))).astype(np.float32)


class _Stub(types.ModuleType):
    """Stands for a module this machine lacks: every attribute is another stub, every call returns None."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub(self.__name__ + "." + name)

    def __call__(self, *args, **kwargs):
        return None


def load_reference(root):
    for name in ("cv2", "PIL", "PIL.Image", "einops", "torch", "torch.nn", "torch.nn.functional"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = _Stub(name)
    spec = importlib.util.spec_from_file_location("_reference_frame_utils", os.path.join(root, "utils", "frame_utils.py"))
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
    with tempfile.TemporaryDirectory() as tmp:
        for name, H, W, seed in CASES:
            flow = case_flow(H, W, seed)
            path = os.path.join(tmp, name + ".flo")
            ref.writeFlow(path, flow)
            data = np.frombuffer(open(path, "rb").read(), dtype=np.uint8)
            assert data.size == 12 + 8 * H * W, (name, data.size)
            back = ref.readFlow(path)
            assert back.dtype == np.float32 and back.tobytes() == flow.tobytes(), name
            print("%-10s %d bytes" % (name, data.size))
            arrays += [(name + ".flow", flow), (name + ".bytes", data)]
    write_npz(OUT, arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
