"""Fine-tuning RAFT's update block through the refinement loop (accflow_amd/train_raft.py, accflow_amd/fine_tune.py) on the GPU:
the gate / loss kernels against float64 autograd with DERIVED bounds, the taped loop's gradients against the float64
restatement of the training graph (tests/raft_ft_ref.py, itself pinned on the reference's autograd by
tests/test_fine_tune_host.py), the tape's forward against the inference path, the guard's redo, the weight packs after an
optimizer step, and the front end end to end."""
import functools

import numpy as np
import pytest
import torch

import raft_ft_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # unit roundoff of fp32
GRAD_TOL = 1e-4           # of the gradient's RMS (tests/test_train.py:181)


@functools.lru_cache(maxsize=None)
def _model():
    from accflow_amd import train_raft
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    model = build_flow_estimator("raft")
    model.load_state_dict(make_state_dict(model), strict=True)
    return train_raft.freeze_encoders(model.cuda())


def _clear(model):
    for p in model.parameters():
        p.grad = None


# ---- gate kernels -----------------------------------------------------------------------------------------------------------
def _operand(shape, gen, kind, sliced, c0=0):
    """An fp32 CUDA operand of `shape`; sliced: a channel slice (starting at channel c0) of a 384-channel buffer."""
    Bn, C, H, W = shape
    v = torch.randn(shape, generator=gen)
    v = torch.sigmoid(v) if kind == "gate" else torch.tanh(v) if kind == "tanh" else v
    if not sliced:
        return v.cuda()
    buf = torch.full((Bn, 384, H, W), float("nan")).cuda()
    buf[:, c0:c0 + C] = v.cuda()
    return buf[:, c0:c0 + C]


def _dst(shape, sliced, c0=0):
    Bn, C, H, W = shape
    if not sliced:
        return torch.full(shape, float("nan")).cuda(), None
    buf = torch.full((Bn, 384, H, W), 7.0).cuda()
    return buf[:, c0:c0 + C], buf


def _within(got, want, terms, what):
    """|got - want| <= 8 u * (sum of the absolute values of the output's terms): each output is a sum of at most two products of
    at most four fp32 factors, evaluated with at most 6 roundings (one per operation) - first-order error <= 6 u per term."""
    err = (got.double().cpu() - want).abs()
    bound = 8 * U * terms
    assert bool((err <= bound).all()), (what, float((err - bound).max()))


GATE_SHAPES = [(1, 128, 5, 7), (2, 128, 16, 16), (2, 3, 5, 7)]      # (the last: a plane that is no multiple of 4 elements)


@pytest.mark.parametrize("shape", GATE_SHAPES)
@pytest.mark.parametrize("sliced", [False, True])
def test_gate_kernels_against_float64_autograd(shape, sliced):
    from accflow_amd import backward as B
    gen = torch.Generator().manual_seed(sum(shape) + int(sliced))
    C = shape[1]
    z, r = _operand(shape, gen, "gate", sliced, 1), _operand(shape, gen, "gate", sliced, 129)     # (channel 1: 4-byte aligned only)
    h, q = _operand(shape, gen, "tanh", sliced, 0), _operand(shape, gen, "tanh", sliced, 256)
    g, drh = _operand(shape, gen, "any", sliced, 128), _operand(shape, gen, "any", False)
    dh0 = torch.randn(shape, generator=gen)
    zd, rd, hd, qd = (t.double().cpu().requires_grad_(True) for t in (z, r, h, q))
    gd, drhd = g.double().cpu(), drh.double().cpu()
    # forward
    rh_dst, rh_buf = _dst(shape, sliced, 0)
    hn_dst, hn_buf = _dst(shape, sliced, 384 - C)
    assert B.gru_reset_forward(r, h, out=rh_dst) is rh_dst
    B.gru_update_forward(z, h, q, out=hn_dst)
    rh_w, hn_w = rd * hd, (1 - zd) * hd + zd * qd
    _within(rh_dst, rh_w.detach(), (rd * hd).abs().detach(), "rh")
    _within(hn_dst, hn_w.detach(), (((1 - zd) * hd).abs() + (zd * qd).abs()).detach(), "h_new")
    if sliced:     # nothing outside the destination slices was written
        assert bool((rh_buf[:, C:] == 7.0).all()) and bool((hn_buf[:, :384 - C] == 7.0).all())
    torch.cuda.synchronize()
    # backward: autograd w.r.t. the activations' outputs, sigmoid' / tanh' folded in float64
    dz, dq, dh_u = torch.autograd.grad(hn_w, [zd, qd, hd], gd)
    dr, dh_r = torch.autograd.grad(rh_w, [rd, hd], drhd)
    zc, rc, hc, qc = (t.detach() for t in (zd, rd, hd, qd))
    daz_dst, _ = _dst(shape, sliced, 0)
    dar_dst, dar_buf = _dst(shape, sliced, 128 if C <= 128 else 0)
    daz, daq, dh = B.gru_update_backward(g, z, h, q, daz=daz_dst)
    assert daz is daz_dst
    _within(daz, dz * zc * (1 - zc), (gd * qc * zc * (1 - zc)).abs() + (gd * hc * zc * (1 - zc)).abs(), "daz")
    _within(daq, dq * (1 - qc * qc), (gd * zc).abs() + (gd * zc * qc * qc).abs(), "daq")
    _within(dh, dh_u, gd.abs() + (gd * zc).abs(), "dh")
    acc = dh0.cuda()
    dar = B.gru_reset_backward(drh, r, h, acc, dar=dar_dst)
    _within(dar, dr * rc * (1 - rc), (drhd * hc * rc).abs() + (drhd * hc * rc * rc).abs(), "dar")
    _within(acc, dh0.double() + dh_r, dh0.double().abs() + (drhd * rc).abs(), "dh +=")
    with pytest.raises(RuntimeError):
        B.gru_reset_forward(r, h[:, :C - 1])


SEQ_SHAPES = [(1, 2, 40, 56), (1, 2, 5, 7), (1, 1, 3, 1), (2, 2, 128, 160)]     # 4-wide, scalar, tiny, several workgroups


@pytest.mark.parametrize("shape", SEQ_SHAPES)
def test_seq_l1_gradient_exact_loss_reproducible(shape):
    from accflow_amd import backward as B
    gen = torch.Generator().manual_seed(shape[2])
    pred, gt = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    gt.view(-1)[::7] = pred.view(-1)[::7]                 # ties: the gradient is 0 there (torch's abs backward)
    weight, n = 0.85 ** 3, pred.numel()
    p, t = pred.cuda(), gt.cuda()
    runs = []
    for _ in range(2):
        loss = torch.zeros(1, dtype=torch.float64, device="cuda")
        runs.append((B.seq_l1(p, t, weight, loss), loss))
    (d0, l0), (d1, l1) = runs
    assert torch.equal(d0, d1) and torch.equal(l0, l1)                      # two launches: bit-identical
    want_d = torch.sign(pred - gt) * float(np.float32(weight / n))
    assert torch.equal(d0.cpu(), want_d.float())                            # the gradient: exact
    assert int((d0 == 0).sum()) >= n // 7
    want_l = weight * float((pred.double() - gt.double()).abs().mean())
    assert abs(float(l0) - want_l) <= 1e-6 * want_l
    B.seq_l1(p, t, 1.0, l0)                                                 # the term is ADDED to loss_out
    assert abs(float(l0) - (want_l + want_l / weight)) <= 1e-6 * (want_l + want_l / weight)
    with pytest.raises(RuntimeError):
        B.seq_l1(p, t, 1.0, torch.zeros(1, device="cuda"))


# ---- the taped loop against the float64 restatement -------------------------------------------------------------------------
CASES = {"b1_16x20_i3": (1, 16, 20, 3, 0.8), "b2_16x16_i2": (2, 16, 16, 2, 0.85)}   # 16: the smallest side with a 2 x 2 level 3


@functools.lru_cache(maxsize=None)
def _case(name):
    """Seeded random features and the float64 reference (computed once, shared by the tests that need it)."""
    Bn, h, w, iters, gamma = CASES[name]
    g = torch.Generator().manual_seed(100 + h + w)
    fmap1, fmap2 = torch.randn(Bn, 256, h, w, generator=g), torch.randn(Bn, 256, h, w, generator=g)
    cnet = torch.randn(Bn, 256, h, w, generator=g)
    gt = 3.0 * torch.randn(Bn, 2, 8 * h, 8 * w, generator=g)
    torch.set_num_threads(8)
    loss, grads, ups = R.loss_and_grads(_model().state_dict(), fmap1, fmap2, cnet, gt, iters, gamma)
    return (fmap1.cuda(), fmap2.cuda(), cnet.cuda(), gt.cuda()), iters, gamma, loss, grads, ups


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_gradients_match_float64_autograd(case, mode, monkeypatch):
    """Every update_block parameter within 1e-4 of its gradient's RMS, the loss within 1e-5 relative; frozen parameters keep
    grad None; the f16x3 run stays in f16x3 (no guard trip on in-range features)."""
    from accflow_amd import ops, train, train_raft
    feats, iters, gamma, loss_w, grads_w, ups_w = _case(case)
    monkeypatch.setattr(train, "TRAIN_CONV_MODE", mode)
    model = _model()
    _clear(model)
    ops.guard_report()
    loss, ups = train_raft.forward_backward(model, *feats, iters=iters, gamma=gamma)
    torch.cuda.synchronize()
    assert ops.guard_report() == []
    print(case, mode, "loss rel", abs(loss - loss_w) / loss_w)
    assert len(ups) == iters and all(tuple(a.shape) == tuple(b.shape) for a, b in zip(ups, ups_w))
    named = dict(model.named_parameters())
    assert sorted(grads_w) == sorted(n for n in named if n.startswith("update_block."))
    assert all(p.grad is None for n, p in named.items() if not n.startswith("update_block."))
    worst = {}
    for n, want in grads_w.items():
        got = named[n].grad
        assert got is not None and got.shape == named[n].shape, n
        rms = float(want.pow(2).mean().sqrt().clamp_min(1e-300))
        worst[n] = float((got.double().cpu() - want).abs().max()) / rms
    print(case, mode, "worst", max(worst.items(), key=lambda kv: kv[1]))
    assert abs(loss - loss_w) <= 1e-5 * loss_w
    bad = {k: v for k, v in worst.items() if v > GRAD_TOL}
    assert not bad, bad
    _clear(model)


def test_gradients_are_added_and_flow_init_is_honoured():
    """A second call ADDS into param.grad; flow_init moves the start (raft.py:123-124) on both sides alike."""
    from accflow_amd import train_raft
    (fmap1, fmap2, cnet, gt), iters, gamma, _, _, _ = _case("b1_16x20_i3")
    g = torch.Generator().manual_seed(3)
    fi = 2.0 * torch.randn(1, 2, 16, 20, generator=g)
    loss_w, grads_w, _ = R.loss_and_grads(_model().state_dict(), fmap1, fmap2, cnet, gt, 2, gamma, flow_init=fi)
    model = _model()
    _clear(model)
    loss, _ = train_raft.forward_backward(model, fmap1, fmap2, cnet, gt, iters=2, gamma=gamma, flow_init=fi.cuda())
    assert abs(loss - loss_w) <= 1e-5 * loss_w
    once = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    train_raft.forward_backward(model, fmap1, fmap2, cnet, gt, iters=2, gamma=gamma, flow_init=fi.cuda())
    named = dict(model.named_parameters())
    for n, want in grads_w.items():
        rms = float(want.pow(2).mean().sqrt())
        assert float((once[n].double().cpu() - want).abs().max()) / rms <= GRAD_TOL, n
        assert float((named[n].grad.double().cpu() - 2 * want).abs().max()) / rms <= 2 * GRAD_TOL, n
    _clear(model)


def test_last_prediction_agrees_with_the_inference_refinement():
    """The tape's forward against RAFT._refine on the same features (the inference path: pre-split tensors, fused lookup,
    hoisted context convolutions): mean EPE <= 1e-4 px, the path-versus-path gate of tests/test_alt_corr.py:334."""
    from accflow_amd import train_raft
    (fmap1, fmap2, cnet, gt), iters, gamma, _, _, _ = _case("b2_16x16_i2")
    model = _model()
    _, ups = train_raft.forward_backward(model, fmap1, fmap2, cnet, gt, iters=4, gamma=gamma)
    with torch.no_grad():
        want = model._refine_guarded(fmap1, fmap2, cnet, 4, None)
    epe = float((ups[-1] - want).pow(2).sum(dim=1).sqrt().mean())
    print("tape vs _refine mean EPE", epe)
    assert epe <= 1e-4
    _clear(model)


def test_tripped_step_is_undone_and_redone_in_bf16x6(monkeypatch):
    """inp scaled by 1e4 leaves the fp16 split's range: the f16x3 step trips, its gradients are dropped (what param.grad held
    before stays) and the step is redone in bf16x6 - the result is the bf16x6-only run's: the forward bit for bit, the gradients
    up to the order of the weight-gradient kernels' float atomics (1e-5 of the RMS)."""
    from accflow_amd import ops, train, train_raft
    (fmap1, fmap2, cnet, gt), iters, gamma, _, _, _ = _case("b1_16x20_i3")
    cnet = cnet.clone()
    cnet[:, 128:] *= 1e4
    model = _model()
    params = train_raft.trainable_parameters(model)

    def run():
        _clear(model)
        for p in params:
            p.grad = torch.ones_like(p)
        loss, ups = train_raft.forward_backward(model, fmap1, fmap2, cnet, gt, iters=2, gamma=gamma)
        torch.cuda.synchronize()
        return loss, ups, [p.grad.detach().clone() for p in params]
    ops.guard_report()
    monkeypatch.setattr(train, "TRAIN_CONV_MODE", "f16x3")
    loss_a, ups_a, grads_a = run()
    assert "train_raft.forward_backward" in ops.guard_report()
    monkeypatch.setattr(train, "TRAIN_CONV_MODE", "bf16x6")
    loss_b, ups_b, grads_b = run()
    assert ops.guard_report() == []
    assert loss_a == loss_b and np.isfinite(loss_a)
    assert all(torch.equal(a, b) for a, b in zip(ups_a, ups_b))
    for p, a, b in zip(params, grads_a, grads_b):
        rms = float((b - 1).pow(2).mean().sqrt().clamp_min(1e-30))
        assert float((a - b).abs().max()) <= 1e-5 * rms + 1e-6, tuple(p.shape)     # (1e-6: fp32 spacing of the 1 + g sums)
    _clear(model)


def test_weights_stay_live_after_an_optimizer_step():
    """After one step fnet / cnet are bit-identical and update_block.* moved; the inference forward of the stepped model equals
    that of a fresh model loaded from its state_dict: the weight packs (keyed on the parameters' versions), the workspace's
    cached launches and the hoisted context convolutions follow the new weights."""
    from accflow_amd import train_raft
    from accflow_amd.data.synthetic import make_sequence, make_state_dict, normalize
    from accflow_amd.networks import build_flow_estimator
    model = build_flow_estimator("raft")
    model.load_state_dict(make_state_dict(model), strict=True)
    model = train_raft.freeze_encoders(model.cuda())
    fr = [normalize(f).cuda() for f in make_sequence(21, 2, 128, 160)]
    g = torch.Generator().manual_seed(8)
    gt = (3.0 * torch.randn(1, 2, 128, 160, generator=g)).cuda()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    out0 = model(fr[1], fr[0], iters=3)                       # (fills every cache with the OLD weights)
    opt = torch.optim.AdamW(train_raft.trainable_parameters(model), lr=1e-3, weight_decay=1e-5, eps=1e-8)
    loss, ups = train_raft.train_step(model, opt, fr[1], fr[0], gt, iters=2)
    assert np.isfinite(loss) and len(ups) == 2
    after = model.state_dict()
    for k, v in before.items():
        if k.startswith("update_block."):
            assert not torch.equal(v, after[k]), k
        else:
            assert torch.equal(v, after[k]), k
    out1 = model(fr[1], fr[0], iters=3)
    fresh = build_flow_estimator("raft")
    fresh.load_state_dict({k: v.detach().cpu() for k, v in after.items()}, strict=True)
    out2 = fresh.cuda().eval()(fr[1], fr[0], iters=3)
    assert torch.equal(out1, out2)
    assert not torch.equal(out0, out1)


def test_fine_tune_cli_runs_and_saves(tmp_path, monkeypatch):
    """The front end end to end on synthetic sequences: two steps at crop 128, batch 1, one validation batch; latest.pth loads
    strictly into RAFT under the `module.` prefix."""
    from accflow_amd import fine_tune
    from accflow_amd.eval_cvo import _strip_module
    from accflow_amd.networks import build_flow_estimator
    monkeypatch.setenv("ACCFLOW_SYNTH_SAMPLES", "2")
    monkeypatch.delenv("ACCFLOW_CVO_LMDB", raising=False)
    monkeypatch.delenv("ACCFLOW_SYNTHETIC", raising=False)
    cfg = tmp_path / "c.yml"
    cfg.write_text("exp_name: RAFT-debug\nepochs: 1\nbatch_per_gpu: 1\nimage_size: [128, 128]\nlog_freq: 1\nvalid_freq: 1000\n"
                   "flow_pretrained: none.pth\nlr: !!float 1.2e-4\nvalid_iters: 4\n")
    with pytest.raises(SystemExit):                 # no LMDB, no checkpoint, no --synthetic: a real run is refused
        fine_tune.main(["-c", str(cfg), "--steps", "2", "--out", str(tmp_path)])
    n = fine_tune.main(["-c", str(cfg), "--steps", "2", "--out", str(tmp_path), "--valid-batches", "1", "--synthetic"])
    assert n == 2
    ck = tmp_path / "checkpoints" / "RAFT-debug"
    names = sorted(p.name for p in ck.iterdir())
    assert names == ["000002.pth", "000002.state", "final.pth", "latest.pth", "latest.state"]
    sd = torch.load(ck / "latest.pth")
    assert all(k.startswith("module.") for k in sd)
    build_flow_estimator("raft").load_state_dict(_strip_module(sd), strict=True)
    st = torch.load(ck / "latest.state")
    assert st["iter"] == 2 and st["synthetic"] is True and {"optimizer", "scheduler", "best_epe"} <= set(st)
    with pytest.raises(SystemExit):                 # a fresh run never overwrites
        fine_tune.main(["-c", str(cfg), "--steps", "1", "--out", str(tmp_path), "--synthetic"])
