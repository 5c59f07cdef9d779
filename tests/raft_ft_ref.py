"""The update block's fine-tuning graph (accflow_amd/train_raft.py) restated for torch autograd from the oracle's differentiable
pieces - O.corr_pyramid, O.corr_lookup, O.update_block, O.convex_upsample - in the dtype of its inputs (float64 in the tests).

O.raft_forward is NOT used: it does not detach.  This helper places what the reference's training graph has beyond the
inference forward:
  * coords1 is detached at the top of every iteration (raft.py:128 of the reference);
  * one prediction per iteration, loss = sum_i gamma^(n-1-i) mean |flow_up_i - gt| (loss.py:10-13);
  * the feature maps and the context features are constants (frozen encoders), only `update_block.*` carries gradient."""
import torch

from oracle import accflow_oracle as O

PREFIX = "update_block."


def update_block_names(sd):
    return [k for k in sd if k.startswith(PREFIX)]


def predictions(sd, fmap1, fmap2, cnet, iters, flow_init=None):
    """-> [flow_up_0 .. flow_up_{iters-1}] with the per-iteration detach; sd: state_dict (update_block.* may require grad)."""
    pyr = [lvl.detach() for lvl in O.corr_pyramid(fmap1.detach(), fmap2.detach())]
    cnet = cnet.detach()
    net, inp = torch.tanh(cnet[:, :128]), torch.relu(cnet[:, 128:])
    B, _, h, w = cnet.shape
    coords0 = O.coords_grid(B, h, w, dtype=cnet.dtype)
    coords1 = coords0.clone() if flow_init is None else coords0 + flow_init
    ups = []
    for _ in range(iters):
        coords1 = coords1.detach()
        corr = O.corr_lookup(pyr, coords1)
        flow = coords1 - coords0
        net, mask, delta = O.update_block(net, inp, corr, flow, sd)
        coords1 = coords1 + delta
        ups.append(O.convex_upsample(coords1 - coords0, mask))
    return ups


def sequence_loss(ups, gt, gamma):
    n = len(ups)
    loss = 0.0
    for i, up in enumerate(ups):
        loss = loss + gamma ** (n - 1 - i) * (up - gt).abs().mean()
    return loss


def loss_and_grads(sd, fmap1, fmap2, cnet, gt, iters, gamma, flow_init=None, dtype=torch.float64):
    """-> (loss, {update_block.* name: gradient}, predictions) in `dtype` on the CPU."""
    cast = lambda t: t.detach().to("cpu", dtype)          # noqa: E731
    sd = {k: cast(v) for k, v in sd.items() if k.startswith(PREFIX)}
    for v in sd.values():
        v.requires_grad_(True)
    ups = predictions(sd, cast(fmap1), cast(fmap2), cast(cnet), iters, None if flow_init is None else cast(flow_init))
    loss = sequence_loss(ups, cast(gt), gamma)
    names = list(sd)
    grads = torch.autograd.grad(loss, [sd[k] for k in names])
    return float(loss.detach()), dict(zip(names, grads)), [u.detach() for u in ups]


def encode(sd, image1, image2, dtype=torch.float64):
    """The oracle's frozen encoders (fnet: instance norm, cnet: eval-mode batch norm) -> (fmap1, fmap2, cnet)."""
    cast = lambda t: t.detach().to("cpu", dtype)          # noqa: E731
    sd = {k: cast(v) for k, v in sd.items() if k.startswith(("fnet.", "cnet."))}
    with torch.no_grad():
        B = image1.shape[0]
        fmaps = O.basic_encoder(torch.cat([cast(image1), cast(image2)], 0), sd, "fnet", "instance")
        cnet = O.basic_encoder(cast(image1), sd, "cnet", "batch")
    return fmaps[:B], fmaps[B:], cnet
