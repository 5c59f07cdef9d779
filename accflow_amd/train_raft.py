"""One fine-tuning step of RAFT's update block through the refinement loop, on the HIP library (SURVEY section 2 rows 11-12;
reference: fine_tune.py:203-243, loss.py:4-25, raft/raft.py:94-146, raft/update.py).  Stage 1 of estimator fine-tuning.

What carries gradients, and why this much can be trained without the backward of the correlation lookup or of the encoders'
normalisations (stage 2, not built):
  * RAFT.forward detaches coords1 at the top of every iteration (raft.py:128), so the lookup and `coords1 - coords0` - the two
    inputs of the motion encoder - carry gradient towards the feature maps only; with fnet / cnet frozen they are constants;
  * net = tanh(cnet[:, :128]) and inp = relu(cnet[:, 128:]) are constants for the same reason;
  * gradient therefore reaches the 30 parameters of `update_block.*` through the hidden state (the one path between
    iterations), delta_flow, the mask head and the convex upsampling: convolutions, relu, sigmoid, tanh, concatenations and
    the two GRU gate products.

Per iteration, on a tape (train.Tape's closures): lookup (the inference kernel, fp32) and flow -> motion encoder (5
convolutions; cor / flo and the GRU input are written straight into their concatenation buffers) -> SepConvGRU (per half-step:
z and r as ONE 256-channel convolution over [h | x], backward.gru_reset_forward writes r*h into [r*h | x], q, and
backward.gru_update_forward writes the new state into the NEXT half-step's [h | x]) -> flow head (its second convolution
accumulates into coords1, raft.py:136) and mask head (the 0.25 of update.py:135 folded into the pack, as Tape.zero_conv folds
its factor) -> flow_up = convex_upsample(coords1 - coords0, mask).  loss = sum_i gamma^(iters-1-i) mean |flow_up_i - gt|
(loss.py:10-13; backward.seq_l1: fixed-order sums on the device).  The backward of a half-step is one closure: the gate
kernels hand the convolutions their PRE-activation gradients (sigmoid' and tanh' folded in), the convolutions' input gradients
come back as whole [. | x] tensors whose halves go to the state and to the iteration's x gradient.

Arithmetic follows train.forward_backward: the forward convolutions run in f16x3 under one guard flag, a tripped step is undone
(param.grad restored) and redone in bf16x6; the backward convolutions always run bf16x6.  Gradients are ADDED into `param.grad`
of `update_block.*`; nothing else is touched.

Parity: tests/test_fine_tune.py (float64 autograd of the same graph restated from the oracle's pieces, tests/raft_ft_ref.py)
and tests/test_fine_tune_host.py (that restatement against the reference's own autograd, tests/golden/raft_ft_grad.npz)."""
import torch

from . import backward as B
from . import ops, train
from .networks.raft.corr import CorrBlock      # (the volume and its fp32 lookup: the inference kernels)
from .train import Tape, Var

STAGE2 = ("stage 2 of estimator fine-tuning (the backward of the correlation lookup, of InstanceNorm / batch-statistics "
          "BatchNorm, of GMA's aggregator and of the ConvGRU) is not built")
HIDDEN = 128


def check_model(model):
    """fine-tuning is built for the full RAFT's BasicUpdateBlock (SepConvGRU, mask head) only."""
    from .networks.raft.raft import RAFT
    if not isinstance(model, RAFT):
        raise NotImplementedError("fine_tune: %s is not a RAFT estimator; %s" % (type(model).__name__, STAGE2))
    if model.small:
        raise NotImplementedError("fine_tune: RAFT-small (ConvGRU, no mask head) belongs to %s" % STAGE2)
    if type(model) is not RAFT:
        raise NotImplementedError("fine_tune: %s (attention, aggregator) belongs to %s" % (type(model).__name__, STAGE2))


def trainable_parameters(model):
    """The parameters this stage trains: update_block.* (30 tensors, 3 120 960 elements for the full RAFT)."""
    return [p for n, p in model.named_parameters() if n.startswith("update_block.")]


def freeze_encoders(model):
    """fnet / cnet frozen and in eval() (BatchNorm on its running statistics); update_block trainable."""
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith("update_block.")
    model.eval()
    return model


class _XGrad:
    """Gradient of one iteration's GRU input x = [inp | motion | flow], summed over the four gate convolutions reading it."""
    __slots__ = ("g",)

    def __init__(self):
        self.g = None

    def acc(self, d):
        if self.g is None:
            self.g = d          # (a channel slice of an input-gradient tensor this closure owns)
        else:
            B.add_(self.g, d)


class RaftTape(Tape):
    """train.Tape with the operators of the refinement loop: convolutions that write into channel slices of concatenation
    buffers, stacked convolutions (z and r), a constant output factor (the mask head's 0.25), the GRU half-step."""

    def conv_backward(self, x, g, convs, need_dx, scale=None):
        """Parameter gradients of y = scale * cat_c conv_c(x) from g = dL/dy at the PRE-activation -> dL/dx (or None)."""
        KH, KW = convs[0].kernel_size
        pad = tuple(convs[0].padding)
        with train._param_grad_stream(g, x):
            dw, db = B.conv_wgrad(x, g, KH, KW, padding=pad)
            if scale is not None:          # gradients w.r.t. the FOLDED weights -> the parameters'
                dw, db = dw * scale, db * scale
            o = 0
            for c in convs:
                n = c.out_channels
                self._pacc(c.weight, dw[o:o + n])
                self._pacc(c.bias, db[o:o + n])
                o += n
        if not need_dx:
            return None
        ws = tuple(c.weight for c in convs)
        if len(ws) == 1 and scale is None:
            weight = ws[0]
        else:
            def weight():
                w = torch.cat([p.detach().float() for p in ws], dim=0)
                return w if scale is None else w * scale
        return B.conv_dgrad(g, weight, tuple(x.shape[2:]), padding=pad, deps=ws)

    def conv_to(self, x, convs, pk, act=ops.ACT_NONE, out=None, grad_of=None, scale=None):
        """act(scale * cat_c conv_c(x)) into `out` (a channel slice of a wider buffer, or None).  grad_of: a callable giving
        the output's gradient at backward time when the output lives inside such a buffer (default: the returned Var's)."""
        y = ops.conv2d(pk, x.v, act=act, out=out)
        o = Var(y)

        def bw():
            g = grad_of() if grad_of is not None else o.g
            if g is None:
                return
            if act != ops.ACT_NONE:
                g = B.act_backward(g, y, act)
            dx = self.conv_backward(x.v, g, convs, x.needs, scale)
            if dx is not None:
                x.acc(dx)
        self.fns.append(bw)
        return o

    def flow_update(self, head, conv, pk, coords1):
        """coords1 += conv(head) in place (raft.py:136; coords1 is detached) -> the Var of flow = coords1 - coords0."""
        ops.conv2d(pk, head.v, out=coords1, epi=ops.EPI_ACCUM, e0=coords1)
        flow = torch.empty_like(coords1)
        ops.flow_from_coords(coords1, dst0=flow)
        o = Var(flow)

        def bw():
            if o.g is None:
                return
            head.acc(self.conv_backward(head.v, o.g, [conv], True))
        self.fns.append(bw)
        return o

    def gru_half(self, gru, s, pk_zr, pk_q, hbuf, h, rbuf, h_out, xg):
        """One SepConvGRU half-step (update.py:46-51 / :54-59).  hbuf = [h | x] with h.v = hbuf[:, :128]; rbuf = [. | x], whose
        first 128 channels receive r*h; h_out: the (B, 128, h, w) slice the new state is written to."""
        hd = HIDDEN
        convz, convr, convq = (getattr(gru, "conv%s%s" % (g, s)) for g in "zrq")
        zr = ops.conv2d(pk_zr, hbuf, act=ops.ACT_SIGMOID)
        z, r = zr[:, :hd], zr[:, hd:]
        B.gru_reset_forward(r, h.v, out=rbuf[:, :hd])
        q = ops.conv2d(pk_q, rbuf, act=ops.ACT_TANH)
        B.gru_update_forward(z, h.v, q, out=h_out)
        o = Var(h_out)

        def bw():
            if o.g is None:
                return
            dazr = torch.empty_like(zr)
            _, daq, dh = B.gru_update_backward(o.g, z, h.v, q, daz=dazr[:, :hd])
            d_rbuf = self.conv_backward(rbuf, daq, [convq], True)
            B.gru_reset_backward(d_rbuf[:, :hd], r, h.v, dh, dar=dazr[:, hd:])
            xg.acc(d_rbuf[:, hd:])
            d_hbuf = self.conv_backward(hbuf, dazr, [convz, convr], True)
            B.add_(dh, d_hbuf[:, :hd])
            xg.acc(d_hbuf[:, hd:])
            h.acc(dh)
        self.fns.append(bw)
        return o


def _packs(ub):
    """The update block's packs for the tape (PackCache: rebuilt when a parameter's version moves).  The plain ones are the
    inference path's entries; the GRU's are whole-input packs of their own (inference cuts the context features out)."""
    pk, e, g, f = ub._packs, ub.encoder, ub.gru, ub.flow_head
    P = {"c1": pk.conv("c1", e.convc1), "c2": pk.conv("c2", e.convc2), "f1": pk.conv("ft.f1", e.convf1),
         "f2": pk.conv("f2", e.convf2), "cf": pk.conv("cf", e.conv), "fh1": pk.conv("fh1", f.conv1), "fh2": pk.conv("fh2", f.conv2),
         "m0": pk.conv("m0", ub.mask[0]), "m2": pk.conv("m2", ub.mask[2], const_scale=0.25)}
    for s in ("1", "2"):
        P["zr" + s] = pk.conv_cat("ft.zr" + s, [getattr(g, "convz" + s), getattr(g, "convr" + s)])
        P["q" + s] = pk.conv("ft.q" + s, getattr(g, "convq" + s))
    return P


def _iteration(t, ub, P, corr_fn, coords1, hbuf, net):
    """One refinement iteration on the tape.  hbuf: this iteration's [h | x] buffer whose first 128 channels hold the state
    (`net`, a Var over that slice).  -> (next iteration's buffer, its state Var, flow Var, mask Var)."""
    R = ops.ACT_RELU
    e, hd = ub.encoder, HIDDEN
    Bn, _, h, w = hbuf.shape
    dev = hbuf.device

    def buf(c):
        return torch.empty((Bn, c, h, w), dtype=torch.float32, device=dev)
    # coords1 is detached (raft.py:128): the lookup and the flow are constants of the iteration
    corr = Var(corr_fn(coords1), needs=False)
    flow_in = hbuf[:, hd + 254:hd + 256]
    ops.flow_from_coords(coords1, dst0=flow_in)
    xg = _XGrad()
    # ---- motion encoder (update.py:89-97): cor | flo and [.. | motion | flow] are written in place ----
    corflo = Var(buf(256))
    c1 = t.conv_to(corr, [e.convc1], P["c1"], R)
    t.conv_to(c1, [e.convc2], P["c2"], R, out=corflo.v[:, :192], grad_of=lambda: None if corflo.g is None else corflo.g[:, :192])
    f1 = t.conv_to(Var(flow_in, needs=False), [e.convf1], P["f1"], R)
    t.conv_to(f1, [e.convf2], P["f2"], R, out=corflo.v[:, 192:], grad_of=lambda: None if corflo.g is None else corflo.g[:, 192:])
    t.conv_to(corflo, [e.conv], P["cf"], R, out=hbuf[:, hd + 128:hd + 254],
              grad_of=lambda: None if xg.g is None else xg.g[:, 128:254])
    # ---- SepConvGRU (update.py:45-60): x = hbuf[:, 128:] is copied beside the three other first operands ----
    rbuf1, hbuf2, rbuf2, nxt = buf(hd + 256), buf(hd + 256), buf(hd + 256), buf(hd + 256)
    for b in (rbuf1, hbuf2, rbuf2):
        ops.copy_into(hbuf[:, hd:], b[:, hd:])
    h1 = t.gru_half(ub.gru, "1", P["zr1"], P["q1"], hbuf, net, rbuf1, hbuf2[:, :hd], xg)
    h2 = t.gru_half(ub.gru, "2", P["zr2"], P["q2"], hbuf2, h1, rbuf2, nxt[:, :hd], xg)
    # ---- heads (update.py:13-14, :133-135) ----
    head = t.conv_to(h2, [ub.flow_head.conv1], P["fh1"], R)
    flow = t.flow_update(head, ub.flow_head.conv2, P["fh2"], coords1)
    m0 = t.conv_to(h2, [ub.mask[0]], P["m0"], R)
    mask = t.conv_to(m0, [ub.mask[2]], P["m2"], scale=0.25)
    return nxt, h2, flow, mask


def _forward_backward(model, fmap1, fmap2, cnet_feat, flow_gt, iters, gamma, flow_init, mode):
    ub = model.update_block
    fmap1, fmap2 = fmap1.detach().float().contiguous(), fmap2.detach().float().contiguous()
    cnet_feat = cnet_feat.detach().float().contiguous()
    gt = flow_gt.detach().float().contiguous()
    Bn, _, h, w = cnet_feat.shape
    dev = cnet_feat.device
    if tuple(gt.shape) != (Bn, 2, 8 * h, 8 * w):
        raise RuntimeError("fine_tune: flow_gt is %s, expected %s" % (tuple(gt.shape), (Bn, 2, 8 * h, 8 * w)))
    hd = HIDDEN
    with ops.conv_mode(mode):
        P = _packs(ub)
        corr_fn = CorrBlock(fmap1, fmap2, radius=model.args.corr_radius)
        hbuf = torch.empty((Bn, hd + 256, h, w), dtype=torch.float32, device=dev)
        ops.split_tanh_relu(cnet_feat, hbuf[:, :hd], hbuf[:, hd:hd + 128], hd, 128)       # raft.py:117-119, no gradient
        inp = hbuf[:, hd:hd + 128]
        coords1 = ops.coords_grid(Bn, h, w, dev, flow_init=flow_init)
        t = RaftTape()
        net = Var(hbuf[:, :hd], needs=False)
        loss = torch.zeros(1, dtype=torch.float64, device=dev)
        ups = []
        for i in range(iters):
            nxt, net, flow, mask = _iteration(t, ub, P, corr_fn, coords1, hbuf, net)
            ops.copy_into(inp, nxt[:, hd:hd + 128])
            hbuf = nxt
            up = t.convex_upsample(flow, mask)
            up.g = B.seq_l1(up.v, gt, gamma ** (iters - 1 - i), loss)
            ups.append(up.v)
        t.backward()
    train.join_param_grads(dev)
    return float(loss.item()), ups


def forward_backward(model, fmap1, fmap2, cnet_feat, flow_gt, iters=12, gamma=0.85, flow_init=None):
    """sequence_loss_raft over `iters` refinement iterations from given encoder outputs, and its gradients w.r.t.
    update_block.* (ADDED into param.grad).  fmap1 / fmap2 (B, 256, h, w), cnet_feat (B, 256, h, w), flow_gt (B, 2, 8h, 8w).
    -> (loss, [flow_up_0 .. flow_up_{iters-1}]).  f16x3 forward under one guard flag; a tripped step is undone and redone in
    bf16x6 (ops.guard_report() then lists "train_raft.forward_backward")."""
    check_model(model)
    if iters < 1:
        raise ValueError("iters must be >= 1")
    args = (model, fmap1, fmap2, cnet_feat, flow_gt, iters, gamma, flow_init)
    mode = train.TRAIN_CONV_MODE
    if mode != "f16x3" or ops.inside_guard():
        return _forward_backward(*args, mode)
    params = trainable_parameters(model)
    saved = [None if p.grad is None else p.grad.detach().clone() for p in params]
    flag = torch.zeros(1, dtype=torch.int32, device=cnet_feat.device)
    with ops.guard_scope(flag):
        out = _forward_backward(*args, "f16x3")
    if not int(flag.item()):
        return out
    ops.note_guard_trip("train_raft.forward_backward")
    for p, g in zip(params, saved):
        p.grad = g
    return _forward_backward(*args, "bf16x6")


def forward_backward_frames(model, image1, image2, flow_gt, iters=12, gamma=0.85, flow_init=None):
    """forward_backward behind the frozen encoders, which run on the inference path under no_grad (each a guarded stage)."""
    check_model(model)
    with torch.no_grad():
        image1, image2 = image1.float().contiguous(), image2.float().contiguous()
        fmap1, fmap2 = model.fnet([image1, image2])
        cnet_feat = model.cnet(image1)
    return forward_backward(model, fmap1, fmap2, cnet_feat, flow_gt, iters, gamma, flow_init)


def train_step(model, optimizer, image1, image2, flow_gt, iters=12, gamma=0.85, clip=1.0, scheduler=None, group=None):
    """zero_grad / forward / backward / clip / step of fine_tune.py:205-243 (no GradScaler: nothing here computes in fp16
    without its range guard); with torch.distributed initialised the gradients are averaged over the ranks first."""
    optimizer.zero_grad(set_to_none=True)
    loss, ups = forward_backward_frames(model, image1, image2, flow_gt, iters, gamma)
    params = trainable_parameters(model)
    train.allreduce_grads(params, group)
    torch.nn.utils.clip_grad_norm_(params, clip)
    optimizer.step()
    if scheduler is not None:
        scheduler.step()
    return loss, ups
