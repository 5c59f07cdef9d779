"""The fusion heads' graph with GIVEN ReLU masks - test infrastructure of tests/test_train_tape.py and
tests/test_train_tape_host.py.

A restatement of oracle/accflow_oracle.py's flow_encoder, basic_encoder(kind="none"), accplus, blending and flow_decoder, line
for line, in the dtype of its inputs, in which every ReLU is a SITE keyed by the parameter-name prefix of the convolution that
feeds it ("flow_encoder.conv1", "context.layer2.0.conv2", "accplus.conv4.2", ...; the residual joins: "context.layerL.B.join"):
    masks is None          the site is torch.relu(pre)                  - the oracle's graph, bit for bit
    masks[site] given      the site is pre * masks[site] (a 0/1 tensor) - the graph with a FIXED activation pattern
Every function also returns its pre-activations by site.

Why: two evaluations of the same graph in different arithmetic put a handful of pre-activations of ~1e-7 of their layer's RMS
on different sides of a ReLU; one such unit moves single parameter gradients by ~1e-2 of their RMS, which says nothing about
the backward kernels.  With the pattern fixed to the one the tape actually took, the gradient is a smooth function of the
inputs and compares element by element; the pattern itself is checked separately (mask_disagreements).
Sigmoid, tanh, the convex upsampling and the deformable sampling are the oracle's own functions."""
import torch

from oracle import accflow_oracle as O

_conv = O._conv


def _site(pre, site, masks, pres):
    pres[site] = pre
    if masks is None:
        return torch.relu(pre)
    return pre * masks[site].to(pre.dtype)


def flow_encoder(x, sd, masks=None, p="flow_encoder"):
    """O.flow_encoder -> (out, pres)"""
    pres = {}
    x = _site(_conv(x, sd, p + ".conv1", padding=3), p + ".conv1", masks, pres)
    x = _site(_conv(x, sd, p + ".conv2", padding=1), p + ".conv2", masks, pres)
    return _conv(x, sd, p + ".conv3"), pres


def _residual_block(x, sd, p, stride, masks, pres):
    """O.residual_block with identity norms"""
    y = _site(_conv(x, sd, p + ".conv1", stride=stride, padding=1), p + ".conv1", masks, pres)
    y = _site(_conv(y, sd, p + ".conv2", padding=1), p + ".conv2", masks, pres)
    if (p + ".downsample.0.weight") in sd:
        x = _conv(x, sd, p + ".downsample.0", stride=stride)
    return _site(x + y, p + ".join", masks, pres)


def context_encoder(x, sd, masks=None, p="context"):
    """O.basic_encoder(x, sd, p, "none") -> (out, pres)"""
    pres = {}
    x = _site(_conv(x, sd, p + ".conv1", stride=2, padding=3), p + ".conv1", masks, pres)
    for li, st in ((1, 1), (2, 2), (3, 2)):
        x = _residual_block(x, sd, "%s.layer%d.0" % (p, li), st, masks, pres)
        x = _residual_block(x, sd, "%s.layer%d.1" % (p, li), 1, masks, pres)
    return _conv(x, sd, p + ".conv2"), pres


def accplus(df, f, o, c, sd, masks=None, p="accplus", scale_factor=3):
    """O.accplus -> (out, extra, pres).  scale_factor: ZeroConv2d's 3 - what the teeth test of the gate replaces."""
    pres = {}
    x = torch.cat([df, f, o], 1)
    x = _conv(_site(_conv(x, sd, p + ".conv1.0", padding=1), p + ".conv1.0", masks, pres), sd, p + ".conv1.2", padding=1)
    x = torch.cat([x, c], 1)
    x = _site(_conv(x, sd, p + ".conv2.0", padding=1), p + ".conv2.0", masks, pres)
    x = _site(_conv(x, sd, p + ".conv2.2", padding=1), p + ".conv2.2", masks, pres)
    x = _conv(x, sd, p + ".conv2.4.conv", padding=1) * torch.exp(sd[p + ".conv2.4.scale"] * scale_factor)
    off, m = x[:, :18], torch.sigmoid(x[:, 18:27])
    f_ = O.deform_conv2d(f, off, m, sd[p + ".dconv.weight"], sd[p + ".dconv.bias"])
    x = torch.cat([f_, df, o], 1)
    x = _conv(_site(_conv(x, sd, p + ".conv3.0", padding=1), p + ".conv3.0", masks, pres), sd, p + ".conv3.2", padding=1)
    x = torch.cat([x, c, f_, df], 1)
    x = _site(_conv(x, sd, p + ".conv4.0", padding=1), p + ".conv4.0", masks, pres)
    x = _site(_conv(x, sd, p + ".conv4.2", padding=1), p + ".conv4.2", masks, pres)
    return _conv(x, sd, p + ".conv4.4"), dict(off=off, m=m, f_=f_), pres


def blending_mask(emap, sd, masks=None, p="blending"):
    """the mask of O.blending -> (m, pres)"""
    pres = {}
    x = _site(_conv(emap, sd, p + ".mask.0"), p + ".mask.0", masks, pres)
    return torch.sigmoid(_conv(x, sd, p + ".mask.2", padding=1)), pres


def blend(f1, f2, m):
    return f1 * m + (1 - m) * f2


def blending(f1, f2, emap, sd, masks=None, p="blending"):
    """O.blending -> (out, pres)"""
    m, pres = blending_mask(emap, sd, masks, p)
    return blend(f1, f2, m), pres


def flow_decoder(x, sd, masks=None, p="flow_decoder"):
    """O.flow_decoder -> (flow_small, up, pres)"""
    pres = {}
    flow_small = _conv(_site(_conv(x, sd, p + ".flow.0", padding=1), p + ".flow.0", masks, pres), sd, p + ".flow.2", padding=1)
    mask = 1.0 * _conv(_site(_conv(x, sd, p + ".mask.0", padding=1), p + ".mask.0", masks, pres), sd, p + ".mask.2")
    return flow_small, O.convex_upsample(flow_small, mask), pres


# ---- helpers shared by the CPU and the GPU tests ---------------------------------------------------------------------------
def signs(pres):
    """the activation pattern an evaluation took: {site: pre > 0} as 0/1 tensors of the pre-activation's dtype"""
    return {k: (v > 0).to(v.dtype) for k, v in pres.items()}


def leaves(sd, prefix, dtype=torch.float64):
    """{name: leaf tensor requiring a gradient} for the parameters under `prefix` (`sd`: a state_dict of tensors)"""
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()
            if k.startswith(prefix) and v.is_floating_point()}


def rms(t):
    return float(t.detach().double().pow(2).mean().sqrt())


def grad_error(got, want):
    """largest |got - want| over the RMS of want (the measure of tests/test_train.py's GRAD_TOL)"""
    want = want.detach().double()
    return float((got.detach().double().cpu().reshape(want.shape) - want).abs().max()) / max(rms(want), 1e-300)


def mask_disagreements(masks, pres64, fwd_gate):
    """Per site: units whose mask differs from the sign of the float64 pre-activation, the cap max(1, 1e-5 x units), and the
    largest |pre64| among them over (fwd_gate x the site's RMS).  -> {site: (count, cap, worst)}; the condition is
    count <= cap and worst < 1."""
    out = {}
    for site, pre in pres64.items():
        m = masks[site].detach().cpu().to(torch.bool).reshape(pre.shape)
        bad = m != (pre.detach() > 0)
        n = int(bad.sum())
        worst = float(pre.detach()[bad].abs().max()) / (fwd_gate * rms(pre)) if n else 0.0
        out[site] = (n, max(1, int(1e-5 * pre.numel())), worst)
    return out


# ---- the cases of tests/test_train_tape.py (the CPU tests run the same ones with an fp32 evaluation in place of the GPU) ----
GRAD_TOL = 2e-4                                    # tests/test_train.py:16 - of the gradient's RMS, per element
CONV_GATE = {"f16x3": 1e-4, "bf16x6": 3e-5}        # tests/test_conv_routes.py: per convolution, of the output's scale
# convolutions on the module's longest path (the forward gate is CONV_GATE x this, of the output's RMS)
PATH_CONVS = {"flow_encoder": 3, "context": 14, "accplus": 11, "blending": 2, "flow_decoder": 2}
MODULES = tuple(PATH_CONVS)
SHAPES = {"b2_8x9": (2, 8, 9), "b1_13x17": (1, 13, 17)}      # batch, coarse h, w (images: 64 x 72, 104 x 136)
SEED = 8


def forward_gate(module, mode):
    return CONV_GATE[mode] * PATH_CONVS[module]


def state_dict():
    """make_state_dict weights of AccFlow(build_flow_estimator("acc|raft")) without the estimator's, on the CPU in fp32"""
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.AccFlow_ import AccFlow
    sd = make_state_dict(AccFlow(build_flow_estimator("acc|raft")))
    return {k: v for k, v in sd.items() if not k.startswith("ofe.")}


def case_inputs(shape, sd, batch=None, seed=SEED):
    """Seeded fp32 inputs of every module at SHAPES[shape] (batch: another batch size at the same planes).  Flows ~ 2.5 N(0, 1)
    px; context features N(0, 1); o a 0/1 map; the error map |N(0, 1)|; df / f / f_ini: O.flow_encoder (float64, rounded to
    fp32) of the flows; G_*: the upstream gradient of each module's output."""
    N, h, w = SHAPES[shape]
    N = N if batch is None else batch
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    x = {"flow%d" % i: 2.5 * rn(N, 2, h, w) for i in range(3)}
    x["image"] = 2 * torch.rand(N, 3, 8 * h, 8 * w, generator=g) - 1
    x["c"] = rn(N, 128, h, w)
    x["o"] = (torch.rand(N, 1, h, w, generator=g) < 0.7).float()
    x["emap"] = rn(N, 128, h, w).abs()
    sd64 = {k: v.double() for k, v in sd.items()}
    enc = O.flow_encoder(torch.cat([x["flow0"], x["flow1"], x["flow2"]], 0).double(), sd64).float()
    x["f_ini"], x["df"], x["f"] = enc[:N].contiguous(), enc[N:2 * N].contiguous(), enc[2 * N:].contiguous()
    x["G_fe0"], x["G_fe2"] = rn(N, 128, h, w), rn(N, 128, h, w)
    x["G_c"], x["G_acc"], x["G_blend"] = rn(N, 128, h, w), rn(N, 128, h, w), rn(N, 128, h, w)
    x["G_up"] = rn(N, 2, 8 * h, 8 * w)
    return x


# module -> (inputs that want a gradient, inputs that do not, upstream gradients in the order of `outs`)
SPEC = {"flow_encoder": ((), ("flow0", "flow1", "flow2"), ("G_fe0", "G_fe2")),
        "context": ((), ("image",), ("G_c",)),
        "accplus": (("df", "f", "c"), ("o",), ("G_acc",)),
        "blending": (("f_ini", "f"), ("emap",), ("G_blend",)),
        "flow_decoder": (("f_ini",), (), ("G_up",))}


def evaluate(module, x, sd, masks=None, dtype=torch.float64, **kw):
    """The module on the case's inputs `x` in `dtype` with autograd of sum_i (outs[i] * G_i).sum().
    -> dict(outs=[checked outputs], extra=[other outputs], pres={site: pre-activation}, grads={parameter name or
    "in/<input>": gradient}).  flow_encoder gets the three flows as one batch; the gradient arrives on parts 0 and 2 only."""
    wants, plain, gs = SPEC[module]
    P = leaves(sd, module + ".", dtype)
    I = {k: x[k].to(dtype).clone().requires_grad_(True) for k in wants}
    I.update({k: x[k].to(dtype) for k in plain})
    extra = []
    if module == "flow_encoder":
        N = x["flow0"].shape[0]
        enc, pres = flow_encoder(torch.cat([I["flow0"], I["flow1"], I["flow2"]], 0), P, masks)
        outs, extra = [enc[:N], enc[2 * N:]], [enc[N:2 * N]]
    elif module == "context":
        out, pres = context_encoder(I["image"], P, masks)
        outs = [out]
    elif module == "accplus":
        out, _, pres = accplus(I["df"], I["f"], I["o"], I["c"], P, masks, **kw)
        outs = [out]
    elif module == "blending":
        out, pres = blending(I["f_ini"], I["f"], I["emap"], P, masks)
        outs = [out]
    else:
        small, up, pres = flow_decoder(I["f_ini"], P, masks)
        outs, extra = [up], [small]
    loss = sum((o * x[k].to(dtype)).sum() for o, k in zip(outs, gs))
    names = list(P) + ["in/" + k for k in wants]
    gr = torch.autograd.grad(loss, list(P.values()) + [I[k] for k in wants])
    return dict(outs=[o.detach() for o in outs], extra=[e.detach() for e in extra],
                pres={k: v.detach() for k, v in pres.items()}, grads=dict(zip(names, gr)))
