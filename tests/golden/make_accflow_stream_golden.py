"""Generate tests/golden/accflow_stream_c1.npz: the REFERENCE AccFlow(RAFT) on CPU over a 7-frame sequence at the smallest
valid frame size - five accumulation steps, i.e. four carries of F(i-1 -> 0), where accflow_c1 (4 frames) has one.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_accflow_stream_golden.py

The reference is imported at run time the way make_golden.py does it (same torchvision stub, same seeded name-keyed weights
loaded with strict=True); the fixture holds tensors only: out0..out4 = F(2->0) .. F(6->0), every second row and column,
plus seed, H, W, n_frames.  The frames are make_sequence(seed, n_frames, H, W), normalised.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
from make_golden import import_reference, make_sequence, make_state_dict, normalize, npy  # noqa: E402

SEED, N_FRAMES, H, W = 1000, 7, 128, 256


@torch.no_grad()
def main():
    torch.set_num_threads(8)
    build, AccFlow = import_reference()
    model = AccFlow(build("acc|raft").eval()).eval()
    model.load_state_dict(make_state_dict(model), strict=True)
    frames = [normalize(f) for f in make_sequence(SEED, N_FRAMES, H, W)]
    outs = model(images=frames, test_mode=False)
    assert len(outs) == N_FRAMES - 2
    g = {"H": H, "W": W, "seed": SEED, "n_frames": N_FRAMES}
    for k, o in enumerate(outs):
        g["out%d" % k] = npy(o[:, :, ::2, ::2])
    path = os.path.join(HERE, "accflow_stream_c1.npz")
    np.savez_compressed(path, **g)
    print("accflow_stream_c1", {k: v.shape for k, v in g.items() if hasattr(v, "shape")}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
