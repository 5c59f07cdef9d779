"""Generate the RAFT-small fixtures by running the REFERENCE implementation on CPU (see make_golden.py, whose helpers
this script imports: the torchvision stub, the deterministic weights and frames).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_raft_small_golden.py

The reference's RAFT(small=True, mixed_precision=False) with make_state_dict weights loaded strictly, on the frames of
make_sequence(1000, ...).  Three files, each below the size limit for a committed file (together below raft_c1.npz):

  raft_small_c1.npz         128 x 192 (1/8 grid 16 x 24, the smallest at which the reference itself is finite): fmap1, fmap2,
                            the radius-3 lookup at coords0 (LOOKUP_SEL query pixels) and at coords0 + 6 randn, upflow8 of a
                            stored flow, the flows at iters 1 / 4 and at iters 4 with flow_init (every 2nd pixel) and at iters 12, and the
                            output of a three-frame AccFlow(RAFT-small) (every 2nd pixel) with its 1/8-resolution form
  raft_small_c1_ub.npz      128 x 192: cnet, and one SmallUpdateBlock call (net, delta) on the lookup at coords0 + 6 randn
  raft_small_c1_ragged.npz  136 x 200 (17 x 25: odd level sizes, partial 64-pixel workgroups): fmap1, fmap2, cnet (every 4th
                            channel), the lookup at coords0 + 6 randn (LOOKUP_SEL query pixels), the same flows
Fixtures hold tensors only.
"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
from make_golden import make_sequence, make_state_dict, normalize, npy, pair  # noqa: E402

LOOKUP_SEL = 96      # query pixels whose lookup is stored where the whole tensor is not needed as an input


def small_model():
    from networks.raft.raft import RAFT
    torch.manual_seed(0)
    model = RAFT(argparse.Namespace(small=True, mixed_precision=False)).eval()
    model.load_state_dict(make_state_dict(model), strict=True)
    assert len(model.state_dict()) == 106 and sum(p.numel() for p in model.parameters()) == 990162
    return model


def select(P):
    return np.arange(0, P, max(1, P // LOOKUP_SEL))[:LOOKUP_SEL].astype(np.int64)


@torch.no_grad()
def golden_small(model, H, W, tag, full):
    from networks.raft.corr import CorrBlock
    from networks.raft.utils.utils import coords_grid, upflow8
    i1, i2 = pair(1000, H, W)
    g = {"H": H, "W": W, "seed": 1000}
    fmap1, fmap2 = model.fnet([i1, i2])
    cnet = model.cnet(i1)
    g["fmap1"], g["fmap2"] = npy(fmap1), npy(fmap2)
    cb = CorrBlock(fmap1.float(), fmap2.float(), radius=3)
    B, _, h, w = fmap1.shape
    sel = select(h * w)
    g["lookup_sel"] = sel
    coords0 = coords_grid(B, h, w, device="cpu")
    gen = torch.Generator().manual_seed(7)
    coords_r = coords0 + 6.0 * torch.randn(coords0.shape, generator=gen)
    g["coords_r"] = npy(coords_r)
    lookup0, lookup_r = cb(coords0), cb(coords_r)
    assert lookup_r.shape[1] == 4 * 49
    flat = lambda t: npy(t.reshape(B, t.shape[1], h * w)[:, :, sel])
    if full:
        g["lookup0_sel"], g["lookup_r"] = flat(lookup0), npy(lookup_r)
    else:
        g["lookup_r_sel"] = flat(lookup_r)
        g["cnet_s4"] = npy(cnet[:, ::4])
    for it in (1, 4, 12):
        out = model(i1, i2, iters=it)
        assert bool(torch.isfinite(out).all()), (tag, it)
        g["flow_it%d" % it] = npy(out if it == 12 else out[:, :, ::2, ::2])
    fi = 0.5 * torch.randn(coords0.shape, generator=gen)
    g["flow_init"] = npy(fi)
    g["flow_it4_init"] = npy(model(i1, i2, iters=4, flow_init=fi)[:, :, ::2, ::2])
    if full:
        net, inp = torch.split(cnet, [96, 64], dim=1)
        net, inp = torch.tanh(net), torch.relu(inp)
        flow_r = coords_r - coords0
        net1, mask1, delta1 = model.update_block(net, inp, lookup_r, flow_r)
        assert mask1 is None
        g["up_flow"] = npy(flow_r + delta1)
        g["upflow8"] = npy(upflow8(flow_r + delta1)[:, :, ::2, ::2])
        ub = {"H": H, "W": W, "seed": 1000, "cnet": npy(cnet), "coords_r": g["coords_r"], "lookup_r": g.pop("lookup_r"),
              "ub_net": npy(net1), "ub_delta": npy(delta1)}
        # (the lookup at coords0 + 6 randn is an INPUT of the update-block call: stored once, in that file)
        np.savez_compressed(os.path.join(HERE, tag + "_ub.npz"), **ub)
        print(tag + "_ub", {k: v.shape for k, v in ub.items() if hasattr(v, "shape")})
    return g


@torch.no_grad()
def golden_accflow_small(AccFlow, model, H, W, n_frames, g):
    acc = AccFlow(model).eval()
    acc.load_state_dict(make_state_dict(acc), strict=True)
    frames = [normalize(f) for f in make_sequence(1000, n_frames, H, W)]
    cap = {}
    hook = acc.flow_decoder.register_forward_hook(lambda mod, inp, out: cap.setdefault("dec", out))
    outs = acc(images=frames, test_mode=False)
    hook.remove()
    assert len(outs) == n_frames - 2
    g["acc_n_frames"] = n_frames
    for k, o in enumerate(outs):
        g["acc_out%d" % k] = npy(o[:, :, ::2, ::2])
    g["acc_s2_out_small"] = npy(cap["dec"][0])


if __name__ == "__main__":
    torch.set_num_threads(8)
    build, AccFlow = MG.import_reference()
    model = small_model()
    g = golden_small(model, 128, 192, "raft_small_c1", full=True)
    # (AccFlow loads its own name-keyed weights into the estimator: "ofe.*" keys, other values than the bare estimator's)
    golden_accflow_small(AccFlow, small_model(), 128, 192, 3, g)
    np.savez_compressed(os.path.join(HERE, "raft_small_c1.npz"), **g)
    print("raft_small_c1", {k: v.shape for k, v in g.items() if hasattr(v, "shape")})
    g = golden_small(small_model(), 136, 200, "raft_small_c1_ragged", full=False)
    np.savez_compressed(os.path.join(HERE, "raft_small_c1_ragged.npz"), **g)
    print("raft_small_c1_ragged", {k: v.shape for k, v in g.items() if hasattr(v, "shape")})
