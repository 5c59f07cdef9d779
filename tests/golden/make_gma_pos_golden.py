"""Golden fixture of GMA's two positional attention variants, produced by running the REFERENCE implementation on the CPU
(make_golden.py's import_reference; nothing from the reference is copied: the fixture holds tensors only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_gma_pos_golden.py      ->  tests/golden/gma_pos_c1.npz

The reference's RAFTGMA with num_heads = 1, mixed_precision = True (the factory's value; autocast disables itself on the
CPU, so the run is fp32 as for the other goldens), position_only / position_and_content set, and make_state_dict's
weights unchanged; pair (seed 1000, 128 x 256) as for gma_c1.  Per mode m in ("po", "pc") - position_only,
position_and_content:
    <m>_attn_rowsum, <m>_attn_rows (the 32 rows attn_rows_sel, chosen as make_golden.py chooses them),
    <m>_motion_global for motion = randn(1, 128, h, w) from torch.Generator().manual_seed(motion_seed), every second channel,
    <m>_flow_it1, _flow_it4, _flow_it4_init, _flow_it12, all subsampled ::2.
flow_init is shared by the modes.  (flow_it12 whole and every channel of motion_global would make the file 1.4 MB; a
committed file stays below 1 MiB.)
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_golden as MG  # noqa: E402
from accflow_amd.data.synthetic import make_state_dict  # noqa: E402

MOTION_SEED = 77
MODES = {"po": dict(position_only=True, position_and_content=False),
         "pc": dict(position_only=False, position_and_content=True)}


@torch.no_grad()
def main():
    torch.set_num_threads(8)
    MG.import_reference()
    from networks.gma.gma import RAFTGMA
    H, W = 128, 256
    i1, i2 = MG.pair(1000, H, W)
    h, w = H // 8, W // 8
    P = h * w
    rows = np.arange(0, P, max(1, P // 32))[:32]
    gen = torch.Generator().manual_seed(7)
    torch.randn((1, 2, h, w), generator=gen)                       # (make_golden.py draws coords_r first: the same flow_init)
    fi = 0.5 * torch.randn((1, 2, h, w), generator=gen)
    motion = torch.randn((1, 128, h, w), generator=torch.Generator().manual_seed(MOTION_SEED))
    g = {"H": H, "W": W, "seed": 1000, "motion_seed": MOTION_SEED, "attn_rows_sel": rows.astype(np.int64),
         "flow_init": MG.npy(fi)}
    for tag, flags in MODES.items():
        torch.manual_seed(0)
        model = RAFTGMA(argparse.Namespace(num_heads=1, mixed_precision=True, **flags)).eval()
        model.load_state_dict(make_state_dict(model), strict=True)
        cnet = model.cnet(i1)
        inp = torch.relu(cnet[:, 128:])
        attn = model.att(inp)
        g[tag + "_attn_rowsum"] = MG.npy(attn.sum(-1))
        g[tag + "_attn_rows"] = MG.npy(attn[:, 0, rows])
        g[tag + "_motion_global"] = MG.npy(model.update_block.aggregator(attn, motion)[:, ::2])
        for it in (1, 4, 12):
            out = model(i1, i2, iters=it)
            g["%s_flow_it%d" % (tag, it)] = MG.npy(out[:, :, ::2, ::2])
        g[tag + "_flow_it4_init"] = MG.npy(model(i1, i2, iters=4, flow_init=fi)[:, :, ::2, ::2])
    path = os.path.join(HERE, "gma_pos_c1.npz")
    np.savez_compressed(path, **g)
    print("gma_pos_c1", os.path.getsize(path), {k: v.shape for k, v in g.items() if hasattr(v, "shape")})


if __name__ == "__main__":
    main()
