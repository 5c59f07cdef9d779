"""The fusion heads' training tape (accflow_amd/train.py: Tape, Var, the *_fw module functions, step mode, the redo branch
of forward_backward) against float64 autograd, element by element and free of ReLU kinks.

The backward kernels have their own float64 tests (tests/test_backward.py, tests/test_backward_routes.py); this file tests the
code that COMBINES them into gradients.  Method (tests/acc_train_ref.py): the tape's own activation pattern (`Var.v > 0` at
every ReLU site, logged by a RecordingTape defined here - train.py is unchanged) is handed to a float64 restatement of the
oracle's graph, whose gradient of (out * G).sum() for a seeded G is then a smooth function and compares per element; the
pattern is checked on its own against the float64 signs.

  test_glue_*        Var.acc, Tape.cat / add_relu / batch_slices / split_offsets_mask / _pacc on hand-made Vars: copies,
                     additions and one activation - exact, or one fp32 rounding per operation where stated.
  test_module        flow_encoder_fw, context_fw, accplus_fw, blending_fw, flow_decoder_fw x (f16x3, bf16x6) x (batch 2 at
                     8 x 9 coarse, batch 1 at 13 x 17): guard quiet, needs=False inputs without a gradient, shapes, every input
                     and parameter gradient, the forward output, the masks.
  test_step_mode     S = 3, N = 2 at 8 x 9: the step loop of train._forward_backward (BATCHED_BACKWARD) on one tape in step
                     mode, the same steps on one plain tape per step, and two forward + backward passes into one param.grad.
  test_redo_path     train.forward_backward with injected flows beyond the fp16 split's range: tripped, undone, redone.

That the reference plus plain fp32 arithmetic fits these gates, and that the gradient gate rejects a restatement without
ZeroConv2d's factor 3 ten times over, is shown without a GPU in tests/test_train_tape_host.py.

Gates - none of them, nor a shape or a seed, was chosen from the figures below:
  gradients  2e-4 of the gradient's RMS per element (GRAD_TOL of tests/test_train.py, the project's gate for these heads);
  forward    (f16x3 1e-4 | bf16x6 3e-5, the per-convolution gates of tests/test_conv_routes.py) x the convolutions on the
             module's longest path, of the output's RMS, against the UNGATED float64 output;
  masks      per site at most max(1, 1e-5 x units) units differ from the sign of the float64 pre-activation, each with
             |pre64| below the forward gate x the site's RMS;
  redo       loss and predictions bit for bit, gradients 1e-5 of the RMS + the fp32 spacing of the 1 + g sums (float atomics
             in the weight-gradient kernels: tests/test_fine_tune.py::test_tripped_step_is_undone_and_redone_in_bf16x6).

Measured on the MI355X, 2026-10-21, every test passing - worst gradient error / its gate, forward error / its gate, mask
disagreements on the GPU; per module as (batch 2 at 8 x 9 | batch 1 at 13 x 17):
                  f16x3                                      bf16x6
  flow_encoder    0.012 0.008 0  |  0.010 0.007 0            0.014 0.025 0  |  0.010 0.029 0
  context         0.155 0.002 0  |  0.176 0.001 0            0.137 0.007 0  |  0.187 0.006 0
  accplus         0.104 0.003 0  |  0.100 0.004 0            0.178 0.014 0  |  0.197 0.021 0
  blending        0.013 0.006 0  |  0.032 0.006 0            0.016 0.017 0  |  0.028 0.019 0
  flow_decoder    0.074 0.022 0  |  0.090 0.040 0            0.107 0.103 0  |  0.135 0.132 0
  step mode       0.153 0.006 1                              0.253 0.024 0
    (one tape per step 0.148 / 0.250; two passes 0.133 / 0.258 of 2 x the gate; the one disagreeing unit lies within its bound)
  redo path       gradients 0.58 of their tolerance; all 73 parameters receive a gradient; loss 5578.11 in both runs
  split_offsets_mask's sigmoid: 1.75 x 2^-24 (bound 4 x 2^-24)
No test failed on the parent commit: no defect was found in train.py or backward.py.
"""
import hashlib
import os
import re

import numpy as np
import pytest
import torch

import acc_train_ref as A

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                     # one fp32 rounding, relative
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tape_class():
    from accflow_amd import ops, train

    class RecordingTape(train.Tape):
        """Logs (site, Var) for every ReLU: a convolution with a fused ReLU under the parameter-name prefix of its module,
        a residual join under `context.layerL.B.join`.  In step mode a node is logged when it is made (k == 0); its
        full-batch `.v` is read after end_steps."""

        def __init__(self, model):
            super().__init__()
            self.names = {id(m): n for n, m in model.named_modules()}
            self.log, self.last = [], None

        def conv(self, x, conv, pk, act=ops.ACT_NONE):
            out = super().conv(x, conv, pk, act)
            self.last = self.names[id(conv)]
            if act == ops.ACT_RELU and self.k in (None, 0):
                self.log.append((self.last, out))
            return out

        def add_relu(self, a, b):
            out = super().add_relu(a, b)
            self.log.append((".".join(self.last.split(".")[:3]) + ".join", out))
            return out
    return RecordingTape


def _masks(log, sl=slice(None)):
    sites = [s for s, _ in log]
    assert len(set(sites)) == len(sites), sites
    return {s: (v.v[sl] > 0).double().cpu() for s, v in log}


@pytest.fixture(scope="module")
def model():
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.AccFlow_ import AccFlow
    m = AccFlow(build_flow_estimator("acc|raft"))
    m.load_state_dict(make_state_dict(m), strict=True)
    assert float(m.accplus.conv2[4].scale.detach().abs().max()) > 0.2          # the exp(3 scale) factor is live
    return m.cuda().eval()


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _sd(model):
    return _cached("sd", lambda: {k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith("ofe.")})


def _digest(masks):
    h = hashlib.sha1()
    for k in sorted(masks):
        h.update(k.encode())
        h.update(np.packbits(masks[k].numpy().astype(bool)).tobytes())
    return h.hexdigest()


def _clear_grads(model):
    for p in model.parameters():
        p.grad = None


def _fwd_err(got, want):
    return float((got.detach().double().cpu() - want).abs().max()) / A.rms(want)


def _check_masks(masks, pres64, fgate):
    assert sorted(masks) == sorted(pres64), (sorted(masks), sorted(pres64))
    dis = A.mask_disagreements(masks, pres64, fgate)
    assert all(n <= cap and w < 1.0 for n, cap, w in dis.values()), {k: v for k, v in dis.items() if v[0]}
    return sum(v[0] for v in dis.values()), max(v[2] for v in dis.values())


def _check_param_grads(model, prefixes, want, scale=1.0):
    """Every parameter under `prefixes` holds a gradient of its shape that equals `scale` x the reference within `scale` x the
    gate (of the reference's RMS); nothing else holds one.  -> the worst error over that bound, and where."""
    worst = (0.0, None)
    for name, p in model.named_parameters():
        if not name.startswith(prefixes):
            assert p.grad is None, name
            continue
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32, name
        e = A.grad_error(p.grad, scale * want[name])            # = |g - scale x ref| / (scale x RMS of ref)
        worst = max(worst, (e / A.GRAD_TOL, name))
    return worst


# ---- glue operators -----------------------------------------------------------------------------------------------------
def _rn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def test_glue_var_acc():
    """first assignment, then addition (one fp32 add per element: IEEE, the CPU's fp32 sum is the expected value)"""
    from accflow_amd import train
    g1, g2, g3 = _rn(1, 2, 5, 3, 7), _rn(2, 2, 5, 3, 7), _rn(3, 2, 5, 3, 7)
    c1, c2, c3 = g1.cpu(), g2.cpu(), g3.cpu()
    v = train.Var(_rn(0, 2, 5, 3, 7))
    assert v.g is None
    v.acc(g1)
    assert v.g is g1 and torch.equal(g1.cpu(), c1)
    v.acc(g2)
    assert v.g is g1 and torch.equal(g2.cpu(), c2)                                   # added in place; the addend untouched
    assert torch.equal(v.g.cpu(), c1 + c2)
    v.acc(g3)
    assert torch.equal(v.g.cpu(), (c1 + c2) + c3) and torch.equal(g3.cpu(), c3)
    w = train.Var(_rn(0, 2, 5, 3, 7), needs=False)
    w.acc(g2)
    assert w.g is None


def test_glue_cat():
    """three parts: one with needs=False, one that already holds a gradient, one that takes a private copy"""
    from accflow_amd import train
    a, b, c = train.Var(_rn(1, 2, 3, 5, 7), needs=False), train.Var(_rn(2, 2, 4, 5, 7)), train.Var(_rn(3, 2, 6, 5, 7))
    gb = _rn(4, 2, 4, 5, 7)
    b.g = gb.clone()
    t = train.Tape()
    out = t.cat([a, b, c])
    assert out.needs and torch.equal(out.v, torch.cat([a.v, b.v, c.v], 1))
    G = _rn(5, 2, 13, 5, 7)
    out.g = G.clone()
    t.backward()
    assert a.g is None
    assert torch.equal(b.g.cpu(), gb.cpu() + G[:, 3:7].cpu())                       # one fp32 add
    assert torch.equal(c.g, G[:, 7:13]) and c.g.is_contiguous()
    assert c.g.untyped_storage().data_ptr() != out.g.untyped_storage().data_ptr()
    assert b.g.untyped_storage().data_ptr() != out.g.untyped_storage().data_ptr()
    c.acc(_rn(6, 2, 6, 5, 7))
    b.acc(_rn(7, 2, 4, 5, 7))
    assert torch.equal(out.g, G)                                                     # later additions stay in the parts
    assert torch.equal(c.g.cpu(), G[:, 7:13].cpu() + _rn(6, 2, 6, 5, 7).cpu())
    # no part wants a gradient: neither does the result
    assert not train.Tape().cat([train.Var(a.v, needs=False), train.Var(b.v, needs=False)]).needs


def test_glue_add_relu():
    from accflow_amd import train
    for b_has_grad in (False, True):
        a, b = train.Var(_rn(1, 2, 5, 3, 7)), train.Var(_rn(2, 2, 5, 3, 7))
        gb = _rn(8, 2, 5, 3, 7)
        if b_has_grad:
            b.g = gb.clone()
        t = train.Tape()
        out = t.add_relu(a, b)
        want = torch.relu(a.v.cpu() + b.v.cpu())                                    # one fp32 add, then a selection
        assert torch.equal(out.v.cpu(), want) and int((want > 0).sum()) not in (0, want.numel())
        G = _rn(3, 2, 5, 3, 7)
        out.g = G.clone()
        t.backward()
        g = G.cpu() * (want > 0)
        assert torch.equal(a.g.cpu(), g)
        assert torch.equal(b.g.cpu(), gb.cpu() + g if b_has_grad else g)
        assert a.g.untyped_storage().data_ptr() != b.g.untyped_storage().data_ptr()
        before = b.g.clone()
        a.acc(_rn(4, 2, 5, 3, 7))
        assert torch.equal(b.g, before) and torch.equal(a.g.cpu(), g + _rn(4, 2, 5, 3, 7).cpu())
        before = a.g.clone()
        b.acc(_rn(5, 2, 5, 3, 7))
        assert torch.equal(a.g, before) and torch.equal(out.g, G)


def test_glue_batch_slices():
    """only some slices received a gradient: the others are zero-filled; none received one: x gets nothing"""
    from accflow_amd import train
    x = train.Var(_rn(1, 6, 4, 3, 5))
    t = train.Tape()
    outs = t.batch_slices(x, 2)
    assert len(outs) == 3 and all(torch.equal(o.v, x.v[2 * i:2 * i + 2]) for i, o in enumerate(outs))
    g0, g2 = _rn(2, 2, 4, 3, 5), _rn(3, 2, 4, 3, 5)
    outs[0].g, outs[2].g = g0.clone(), g2.clone()
    t.backward(keep=True)
    assert torch.equal(x.g, torch.cat([g0, torch.zeros_like(g0), g2], 0))
    t.backward()                                                                     # a second delivery adds (Var.acc)
    assert torch.equal(x.g.cpu(), torch.cat([g0 + g0, torch.zeros_like(g0), g2 + g2], 0).cpu())
    y = train.Var(_rn(1, 6, 4, 3, 5))
    t = train.Tape()
    t.batch_slices(y, 2)
    t.backward()
    assert y.g is None
    z = train.Var(_rn(1, 6, 4, 3, 5), needs=False)
    t = train.Tape()
    t.batch_slices(z, 3)[1].g = _rn(4, 3, 4, 3, 5)
    t.backward()
    assert z.g is None


def test_glue_split_offsets_mask():
    """27 channels in: 18 offsets pass through, sigmoid on the last 9.  Forward: expf to 1 ulp (2 roundings' worth), one add,
    one divide -> 4 x 2^-24 relative.  Backward of the sigmoid from its OUTPUT s: (g s)(1 - s), three roundings."""
    from accflow_amd import train
    om = train.Var(3.0 * _rn(1, 2, 27, 5, 7))
    t = train.Tape()
    off, msk = t.split_offsets_mask(om)
    assert torch.equal(off.v, om.v[:, :18]) and tuple(msk.v.shape) == (2, 9, 5, 7)
    s64 = torch.sigmoid(om.v[:, 18:].double().cpu())
    e = float(((msk.v.double().cpu() - s64).abs() / s64).max())
    print("split_offsets_mask: sigmoid forward %.2f x 2^-24 relative (bound 4)" % (e / U))
    assert e <= 4 * U
    t.backward(keep=True)
    assert om.g is None                                                              # nothing arrived: nothing delivered
    goff, gm = _rn(2, 2, 18, 5, 7), _rn(3, 2, 9, 5, 7)
    s = msk.v.double().cpu()
    want_m = gm.double().cpu() * s * (1 - s)
    # the mask alone: the offsets' 18 channels are zero-filled
    msk.g = gm.clone()
    t.backward(keep=True)
    assert torch.equal(om.g[:, :18], torch.zeros_like(goff))
    assert bool(((om.g[:, 18:].double().cpu() - want_m).abs() <= 3 * U * (1 + 2.0 ** -20) * want_m.abs()).all())
    # both (a fresh Var: acc would add)
    om.g, off.g = None, goff.clone()
    t.backward()
    assert torch.equal(om.g[:, :18], goff)
    assert bool(((om.g[:, 18:].double().cpu() - want_m).abs() <= 3 * U * (1 + 2.0 ** -20) * want_m.abs()).all())


def test_glue_pacc():
    from accflow_amd import train
    p = torch.nn.Parameter(_rn(1, 4, 3, 1, 1))
    g = _rn(2, 3, 4).t()                                                             # (4, 3), not contiguous
    train.Tape._pacc(p, g)
    assert p.grad.shape == p.shape and p.grad.is_contiguous() and torch.equal(p.grad.reshape(4, 3), g)
    assert p.grad.untyped_storage().data_ptr() != g.untyped_storage().data_ptr()
    g2 = _rn(3, 4, 3)
    train.Tape._pacc(p, g2)
    assert torch.equal(p.grad.cpu().reshape(4, 3), g.cpu() + g2.cpu())               # one fp32 add into the existing .grad
    assert torch.equal(g2, _rn(3, 4, 3))
    train.Tape._pacc(None, g2)
    train.Tape._pacc(p, None)
    assert torch.equal(p.grad.cpu().reshape(4, 3), g.cpu() + g2.cpu())


# ---- the modules --------------------------------------------------------------------------------------------------------
def _run_module(module, model, x, mode):
    from accflow_amd import ops, train
    t = _tape_class()(model)
    wants, plain, gs = A.SPEC[module]
    cu = lambda k: x[k].cuda().contiguous()          # noqa: E731
    V = {k: train.Var(cu(k), needs=True) for k in wants}
    V.update({k: train.Var(cu(k), needs=False) for k in plain})
    _clear_grads(model)
    ops.guard_report()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    extra = []
    with ops.conv_mode(mode), ops.guard_scope(flag):
        if module == "flow_encoder":
            o3 = train.flow_encoder_fw(t, model.flow_encoder, [cu("flow0"), cu("flow1"), cu("flow2")])
            assert len(o3) == 3
            outs, extra = [o3[0], o3[2]], [o3[1]]
        elif module == "context":
            outs = [train.context_fw(t, model.context, cu("image"))]
        elif module == "accplus":
            outs = [train.accplus_fw(t, model.accplus, V["df"], V["f"], V["o"], V["c"])]
        elif module == "blending":
            outs = [train.blending_fw(t, model.blending, V["f_ini"], V["f"], cu("emap"))]
        else:
            small, up = train.flow_decoder_fw(t, model.flow_decoder, V["f_ini"])
            outs, extra = [up], [small]
        for o, k in zip(outs, gs):
            o.g = cu(k).clone()
        t.backward()
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and ops.guard_report() == []                       # the guard stays quiet
    assert t.fns == []
    return t, V, outs, extra


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("shape", list(A.SHAPES))
@pytest.mark.parametrize("module", A.MODULES)
def test_module(model, module, shape, mode):
    sd = _sd(model)
    x = _cached(("x", shape), lambda: A.case_inputs(shape, sd))
    r64 = _cached(("r64", module, shape), lambda: A.evaluate(module, x, sd))
    t, V, outs, extra = _run_module(module, model, x, mode)
    fgate = A.forward_gate(module, mode)
    # forward against the UNGATED float64 graph
    fwd = max(_fwd_err(o.v, w) for o, w in zip(outs + extra, r64["outs"] + r64["extra"]))
    # the activation pattern the tape took
    masks = _masks(t.log)
    ndis, wdis = _check_masks(masks, r64["pres"], fgate)
    gated = _cached(("gated", module, shape, _digest(masks)), lambda: A.evaluate(module, x, sd, masks=masks))
    # gradients
    wants, plain, _ = A.SPEC[module]
    for k in plain:
        assert V[k].g is None, k
    for e in extra:
        assert e.g is None or module == "flow_decoder"          # (FlowEncoder's middle slice got none; `small` got the upsampling's)
    worst = _check_param_grads(model, (module + ".",), gated["grads"])
    for k in wants:
        assert V[k].g is not None and V[k].g.shape == V[k].v.shape, k
        worst = max(worst, (A.grad_error(V[k].g, gated["grads"]["in/" + k]) / A.GRAD_TOL, "in/" + k))
    print("%s %s %s: gradient %.3f of its gate (%s), forward %.3f of its gate (%.1e), mask disagreements %d (worst |pre64| %.2e "
          "of its bound)" % (module, shape, mode, worst[0], worst[1], fwd / fgate, fgate, ndis, wdis))
    _clear_grads(model)
    assert fwd <= fgate
    assert worst[0] <= 1.0, worst


# ---- step mode ----------------------------------------------------------------------------------------------------------
S_STEPS, N_STEP = 3, 2
STEP_CONVS = A.PATH_CONVS["flow_encoder"] + A.PATH_CONVS["accplus"] + A.PATH_CONVS["flow_decoder"]   # FlowEncoder(F2n) -> up
STEP_PREFIXES = ("flow_encoder.", "accplus.", "blending.", "flow_decoder.")


def _step_inputs(model):
    x = A.case_inputs("b2_8x9", _sd(model), batch=S_STEPS * N_STEP, seed=A.SEED + 1)
    return dict(flow_ini=x["flow0"], dflow=x["flow1"], F0=x["flow2"][:N_STEP].contiguous(), c=x["c"], o=x["o"], emap=x["emap"],
                G=x["G_up"])


def _steps_on_one_tape(model, z, mode):
    """the step loop of train._forward_backward under BATCHED_BACKWARD, estimator and context encoder replaced by `z`"""
    from accflow_amd import ops, train
    S, N = S_STEPS, N_STEP
    cu = {k: v.cuda().contiguous() for k, v in z.items()}
    tc = _tape_class()(model)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    with ops.conv_mode(mode), ops.guard_scope(flag):
        fe = train.flow_encoder_fw(tc, model.flow_encoder, [cu["flow_ini"], cu["dflow"]])
        m_full = train.blending_mask_fw(tc, model.blending, cu["emap"])
        hoisted = len(tc.log)
        c1, o_all = train.Var(cu["c"]), train.Var(cu["o"], needs=False)
        F2n = train.Var(torch.empty((S * N, 2) + tuple(cu["F0"].shape[2:]), dtype=torch.float32, device="cuda"), needs=False)
        pkf, fe_m = model.flow_encoder._packs, model.flow_encoder
        tc.begin_steps(S, N)
        prev = cu["F0"]
        for k in range(S):
            tc.step(k)
            ops.copy_into(prev.contiguous(), F2n.v[k * N:(k + 1) * N])
            f = tc.conv(F2n, fe_m.conv1, pkf.conv("1", fe_m.conv1), act=ops.ACT_RELU)
            f = tc.conv(f, fe_m.conv2, pkf.conv("2", fe_m.conv2), act=ops.ACT_RELU)
            f = tc.conv(f, fe_m.conv3, pkf.conv("3", fe_m.conv3))
            f_acc = train.accplus_fw(tc, model.accplus, fe[1], f, o_all, c1)
            f_fuse = tc.blend(fe[0], f_acc, m_full)
            small, up = train.flow_decoder_fw(tc, model.flow_decoder, f_fuse)
            prev = small.v[k * N:(k + 1) * N]
        tc.end_steps()
        assert tc.pos == len(tc.nodes) and tuple(up.v.shape) == tuple(cu["G"].shape)
        up.g = cu["G"].clone()
        tc.backward()
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and o_all.g is None and F2n.g is None
    return dict(up=up.v, small=small.v, F2n=F2n.v, c_grad=c1.g, hoisted=_masks(tc.log[:hoisted]), steps=_masks(tc.log[hoisted:]))


def _steps_on_plain_tapes(model, z, mode):
    """the same steps as train._forward_backward runs them without BATCHED_BACKWARD: one plain tape per step, one shared tape
    for what does not depend on the accumulated flow"""
    from accflow_amd import ops, train
    S, N = S_STEPS, N_STEP
    cu = {k: v.cuda().contiguous() for k, v in z.items()}
    T = _tape_class()
    tc = T(model)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ups, smalls, logs = [], [], []
    with ops.conv_mode(mode), ops.guard_scope(flag):
        fe = train.flow_encoder_fw(tc, model.flow_encoder, [cu["flow_ini"], cu["dflow"]])
        f_ini_s, df_s = tc.batch_slices(fe[0], N), tc.batch_slices(fe[1], N)
        m_s = tc.batch_slices(train.blending_mask_fw(tc, model.blending, cu["emap"]), N)
        c1 = train.Var(cu["c"])
        c1_s = tc.batch_slices(c1, N)
        prev = cu["F0"]
        for k in range(S):
            sl = slice(k * N, (k + 1) * N)
            t = T(model)
            f = train.flow_encoder_fw(t, model.flow_encoder, [prev])[0]
            f_acc = train.accplus_fw(t, model.accplus, df_s[k], f, train.Var(cu["o"][sl], needs=False), c1_s[k])
            small, up = train.flow_decoder_fw(t, model.flow_decoder, t.blend(f_ini_s[k], f_acc, m_s[k]))
            up.g = cu["G"][sl].clone()
            t.backward()
            prev = small.v
            ups.append(up.v)
            smalls.append(small.v)
            logs.append(_masks(t.log))
        tc.backward()
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    steps = {s: torch.cat([lg[s] for lg in logs], 0) for s in logs[0]}
    return dict(up=torch.cat(ups, 0), small=torch.cat(smalls, 0), c_grad=c1.g, hoisted=_masks(tc.log), steps=steps)


def _steps_reference(model, z, F2n, hoisted=None, steps=None):
    """float64, step by step; step k's incoming flow is the detached `F2n[k]` the tape delivered (step 0: the injected flow)"""
    S, N = S_STEPS, N_STEP
    sd = _sd(model)
    P = {}
    for pre in STEP_PREFIXES:
        P.update(A.leaves(sd, pre))
    d = {k: v.double() for k, v in z.items()}
    c = d["c"].clone().requires_grad_(True)
    pres = {}
    enc, pr = A.flow_encoder(torch.cat([d["flow_ini"], d["dflow"]], 0), P, hoisted)
    pres.update(pr)
    m_all, pr = A.blending_mask(d["emap"], P, hoisted)
    pres.update(pr)
    f_ini, df = enc[:S * N], enc[S * N:]
    loss, ups, smalls, spres = 0.0, [], [], []
    for k in range(S):
        sl = slice(k * N, (k + 1) * N)
        mk = None if steps is None else {s: v[sl] for s, v in steps.items()}
        f, p1 = A.flow_encoder(F2n[sl].double(), P, mk)
        f_acc, _, p2 = A.accplus(df[sl], f, d["o"][sl], c[sl], P, mk)
        small, up, p3 = A.flow_decoder(A.blend(f_ini[sl], f_acc, m_all[sl]), P, mk)
        loss = loss + (up * d["G"][sl]).sum()
        ups.append(up.detach())
        smalls.append(small.detach())
        spres.append({**p1, **p2, **p3})
    gr = torch.autograd.grad(loss, list(P.values()) + [c])
    grads = dict(zip(list(P) + ["in/c"], gr))
    return dict(up=torch.cat(ups, 0), small=torch.cat(smalls, 0), grads=grads, hoisted={k: v.detach() for k, v in pres.items()},
                steps={s: torch.cat([p[s].detach() for p in spres], 0) for s in spres[0]})


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
def test_step_mode(model, mode):
    z = _cached("z", lambda: _step_inputs(model))
    _clear_grads(model)
    one = _steps_on_one_tape(model, z, mode)
    g_one = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    F2n = one["F2n"].cpu()
    assert torch.equal(F2n[:N_STEP], z["F0"]) and torch.equal(F2n[N_STEP:], one["small"].cpu()[:-N_STEP])     # the chain of flows
    free = _steps_reference(model, z, F2n)
    fgate = A.CONV_GATE[mode] * STEP_CONVS
    fwd = max(_fwd_err(one["up"], free["up"]), _fwd_err(one["small"], free["small"]))
    nd_h, wd_h = _check_masks(one["hoisted"], free["hoisted"], fgate)
    nd_s, wd_s = _check_masks(one["steps"], free["steps"], fgate)
    gated = _steps_reference(model, z, F2n, one["hoisted"], one["steps"])
    worst = _check_param_grads(model, STEP_PREFIXES, gated["grads"])
    assert one["c_grad"].shape == z["c"].shape
    worst = max(worst, (A.grad_error(one["c_grad"], gated["grads"]["in/c"]) / A.GRAD_TOL, "in/c"))
    # one plain tape per step: the same kernels on the same data forward, the same sums in another order backward
    _clear_grads(model)
    plain = _steps_on_plain_tapes(model, z, mode)
    assert torch.equal(plain["up"], one["up"]) and torch.equal(plain["small"], one["small"])
    assert all(torch.equal(plain["hoisted"][s], one["hoisted"][s]) for s in one["hoisted"])
    assert sorted(plain["steps"]) == sorted(one["steps"]) and all(torch.equal(plain["steps"][s], one["steps"][s]) for s in one["steps"])
    worst_p = _check_param_grads(model, STEP_PREFIXES, gated["grads"])
    worst_p = max(worst_p, (A.grad_error(plain["c_grad"], gated["grads"]["in/c"]) / A.GRAD_TOL, "in/c"))
    # two forward + backward passes into the same param.grad add
    _clear_grads(model)
    for n, p in model.named_parameters():
        if n in g_one:
            p.grad = g_one[n].clone()
    again = _steps_on_one_tape(model, z, mode)
    assert torch.equal(again["up"], one["up"])
    worst_2 = _check_param_grads(model, STEP_PREFIXES, gated["grads"], scale=2.0)
    print("step mode %s: gradient %.3f of its gate (%s), one tape per step %.3f (%s), two passes %.3f of 2 x the gate (%s); forward "
          "%.3f of its gate (%.1e); mask disagreements %d" % (mode, worst[0], worst[1], worst_p[0], worst_p[1], worst_2[0],
                                                               worst_2[1], fwd / fgate, fgate, nd_h + nd_s))
    _clear_grads(model)
    assert fwd <= fgate
    assert worst[0] <= 1.0 and worst_p[0] <= 1.0 and worst_2[0] <= 1.0, (worst, worst_p, worst_2)


# ---- the redo path of train.forward_backward ----------------------------------------------------------------------------
def _s16_limit():
    """the largest magnitude the fp16 split holds, from csrc/s16_format.h and the activation shift it scales by"""
    fmt = open(os.path.join(ROOT, "accflow_amd", "csrc", "s16_format.h")).read()
    hdr = open(os.path.join(ROOT, "include", "accflow_hip.h")).read()
    limit = float(re.search(r"constexpr float S16_LIMIT = ([0-9.]+)f;", fmt).group(1))
    shift = int(re.search(r"#define\s+ACCFLOW_F16_ASHIFT\s+(\d+)", hdr).group(1))
    assert "S16_SCALE = (float)(1 << ACCFLOW_F16_ASHIFT)" in fmt
    return limit / (1 << shift)


def test_redo_path(model, monkeypatch):
    """4 frames at 64 x 72, batch 1; of the injected 1/8-resolution flows the long-range ones (i -> 0, i >= 2: FlowEncoder's
    and the error map's input) are ~2 x the fp16 split's limit, the others ~2.5 px; param.grad pre-set to ones.  The f16x3 run
    trips, is undone and redone in bf16x6: it equals the bf16x6-only run."""
    from accflow_amd import ops, train
    from accflow_amd.data.synthetic import make_sequence, normalize
    limit = _s16_limit()
    assert limit == 4095.0
    frames = [normalize(f).cuda() for f in make_sequence(31, 4, 64, 72)]
    g = torch.Generator().manual_seed(A.SEED + 2)
    gts = [(3.0 * torch.randn(1, 2, 64, 72, generator=g)).cuda() for _ in range(2)]
    far = lambda p: p[1] == 0 and p[0] >= 2          # noqa: E731
    small = {p: ((2 * limit if far(p) else 2.5) * torch.randn(1, 2, 8, 9, generator=g)).cuda() for p in model.pair_schedule(4)}
    assert all((float(v.abs().max()) > limit) == far(p) for p, v in small.items()) and sum(map(far, small)) == 2
    params = train.trainable_parameters(model)
    monkeypatch.setattr(train, "BATCHED_BACKWARD", True)

    def run():
        _clear_grads(model)
        for p in params:
            p.grad = torch.ones_like(p)
        loss, outs = train.forward_backward(model, frames, gts, small=small)
        torch.cuda.synchronize()
        return loss, outs, [p.grad.detach().clone() for p in params]
    ops.guard_report()
    monkeypatch.setattr(train, "TRAIN_CONV_MODE", "f16x3")
    loss_a, outs_a, grads_a = run()
    assert "train.forward_backward" in ops.guard_report()
    monkeypatch.setattr(train, "TRAIN_CONV_MODE", "bf16x6")
    loss_b, outs_b, grads_b = run()
    assert ops.guard_report() == []
    assert np.isfinite(loss_a) and loss_a == loss_b
    assert len(outs_a) == 2 and all(torch.equal(a, b) for a, b in zip(outs_a, outs_b))
    assert all(p.grad is None for n, p in model.named_parameters() if n.startswith("ofe."))
    worst, still = 0.0, 0
    for p, a, b in zip(params, grads_a, grads_b):
        assert bool(torch.isfinite(a).all()), tuple(p.shape)
        still += int(torch.equal(b, torch.ones_like(b)))
        rms = float((b - 1).pow(2).mean().sqrt().clamp_min(1e-30))
        tol = 1e-5 * rms + torch.finfo(torch.float32).eps * b.abs()          # (eps |b|: the fp32 spacing of the 1 + g sums)
        worst = max(worst, float(((a - b).abs() / tol).max()))
    print("redo path: loss %.6g, gradients %.3f of their tolerance; %d of %d parameters received no gradient" % (
        loss_a, worst, still, len(params)))
    _clear_grads(model)
    assert still < len(params) // 2                    # (a step whose gradients all vanish would compare ones with ones)
    assert worst <= 1.0
