"""CPU side of the update block's fine-tuning (accflow_amd/train_raft.py, accflow_amd/fine_tune.py):
  * tests/raft_ft_ref.py - the training graph restated from the oracle's differentiable pieces, the reference of the GPU tests -
    against the REFERENCE's own autograd: tests/golden/raft_ft_grad.npz (made by tests/golden/make_raft_ft_golden.py: the
    reference RAFT in fp32 / eval() on a seeded 128 x 160 pair, 3 iterations, one prediction per iteration);
  * the front end's host logic: pair / label selection, option defaults, the trainable set, the refusals, the checkpoint keys."""
import argparse

import numpy as np
import pytest
import torch

import raft_ft_ref as R

GRAD_TOL = 1e-4       # of the gradient's RMS, per sampled element: the project's gate for the heads (tests/test_train.py:181)


def _model():
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    model = build_flow_estimator("raft")
    model.load_state_dict(make_state_dict(model), strict=True)
    return model


@pytest.fixture(scope="module")
def fixture_run(golden):
    """The float64 restatement on the fixture's frames, through the oracle's encoders: computed once."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    G = golden("raft_ft_grad")
    H, W = int(G["H"]), int(G["W"])
    fr = [normalize(f) for f in make_sequence(int(G["seed"]), 2, H, W)]
    i1, i2 = fr[1], fr[0]                                   # (make_golden.pair: flow from frame 1 to frame 0)
    g = torch.Generator().manual_seed(int(G["gt_seed"]))
    gt = 3.0 * torch.randn(1, 2, H, W, generator=g)
    sd = _model().state_dict()
    torch.set_num_threads(8)
    fmap1, fmap2, cnet = R.encode(sd, i1, i2)
    loss, grads, ups = R.loss_and_grads(sd, fmap1, fmap2, cnet, gt, int(G["iters"]), float(G["gamma"]))
    return G, loss, grads, ups, (sd, fmap1, fmap2, cnet)


def test_restatement_reproduces_the_reference_autograd(fixture_run):
    """Every update_block parameter: max error of the sampled gradient elements <= 1e-4 of that gradient's RMS; the norm and
    the loss likewise.  Measured: worst parameter 6.0e-5 (update_block.gru.convr1.weight) - the fixture is the reference's
    fp32 evaluation, the restatement runs in float64."""
    G, loss, grads, ups, _ = fixture_run
    names = [str(s) for s in G["names"]]
    assert sorted(names) == sorted(grads) and len(names) == 30
    assert abs(loss - float(G["loss"])) <= 1e-5 * float(G["loss"])
    assert float((ups[-1][:, :, ::4, ::4].float() - torch.from_numpy(G["last"])).abs().max()) < 1e-3
    worst = {}
    for n in names:
        g = grads[n].reshape(-1)
        l2 = float(G["l2/" + n])
        rms = l2 / g.numel() ** 0.5
        d = g[::int(G["step/" + n])] - torch.from_numpy(G["val/" + n]).double()
        worst[n] = max(float(d.abs().max()) / rms, abs(float(g.norm()) - l2) / l2)
    print("worst", max(worst.items(), key=lambda kv: kv[1]))
    bad = {k: v for k, v in worst.items() if v > GRAD_TOL}
    assert not bad, bad


def test_fixture_is_small_and_holds_no_feature_maps(golden):
    import os
    from conftest import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "raft_ft_grad.npz")) < 1_000_000
    G = golden("raft_ft_grad")
    assert all(G["val/" + str(n)].size <= 2048 for n in G["names"])
    assert not any(k.startswith(("fmap", "cnet")) for k in G)


def test_fp32_restatement_stays_close_to_float64():
    """The helper on given random features (B = 1, 16 x 20 coarse, 3 iterations, gamma 0.8) in fp32 against float64: what the
    1e-4 gate of the GPU tests leaves to the arithmetic of an fp32 evaluation (measured 3.7e-5 with these seeds)."""
    sd = _model().state_dict()
    g = torch.Generator().manual_seed(11)
    fmap1, fmap2 = torch.randn(1, 256, 16, 20, generator=g), torch.randn(1, 256, 16, 20, generator=g)
    cnet = torch.randn(1, 256, 16, 20, generator=g)
    gt = 3.0 * torch.randn(1, 2, 128, 160, generator=g)
    l64, g64, _ = R.loss_and_grads(sd, fmap1, fmap2, cnet, gt, 3, 0.8)
    l32, g32, _ = R.loss_and_grads(sd, fmap1, fmap2, cnet, gt, 3, 0.8, dtype=torch.float32)
    assert abs(l32 - l64) <= 1e-5 * l64
    worst = max(float((g32[k].double() - g64[k]).abs().max() / g64[k].pow(2).mean().sqrt()) for k in g64)
    print("fp32 vs float64 worst", worst)
    assert worst <= GRAD_TOL


def test_sequence_loss_weights():
    """loss.py:10-13: prediction i of n is weighted gamma^(n-1-i) - the last one counts fully."""
    ups = [torch.full((1, 2, 8, 8), float(v), dtype=torch.float64) for v in (1.0, 2.0, 4.0)]
    gt = torch.zeros(1, 2, 8, 8, dtype=torch.float64)
    assert float(R.sequence_loss(ups, gt, 0.5)) == pytest.approx(0.25 * 1 + 0.5 * 2 + 1.0 * 4)
    assert float(R.sequence_loss(ups, gt, 0.85)) == pytest.approx(0.85 ** 2 * 1 + 0.85 * 2 + 4)


# ---- host logic of the front end -----------------------------------------------------------------------------------------
def _batch():
    imgs = ["I%d" % i for i in range(7)]
    labels = {"fflows": ["F0>%d" % i for i in range(2, 7)], "bflows": ["F%d>0" % i for i in range(2, 7)],
              "delta_fflows": ["F%d>%d" % (i, i + 1) for i in range(6)], "delta_bflows": ["F%d>%d" % (i + 1, i) for i in range(6)]}
    return imgs, labels


@pytest.mark.parametrize("interval", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("direction", [1, -1])
def test_pair_and_label_selection(interval, direction):
    """fine_tune.py:211-222 for all 12 (interval, direction) values."""
    from accflow_amd.fine_tune import select_pair
    imgs, labels = _batch()
    (a, b), label = select_pair(imgs, labels, interval, direction)
    if interval == 1:
        assert (a, b, label) == (("I0", "I1", "F0>1") if direction == 1 else ("I1", "I0", "F1>0"))
    elif direction == 1:
        assert (a, b, label) == ("I0", "I%d" % interval, "F0>%d" % interval)
    else:
        assert (a, b, label) == ("I%d" % interval, "I0", "F%d>0" % interval)


def test_selection_rejects_what_the_reference_never_draws():
    from accflow_amd.fine_tune import draw_interval, select_pair
    imgs, labels = _batch()
    for bad in ((0, 1), (7, 1), (2, 0)):
        with pytest.raises(ValueError):
            select_pair(imgs, labels, *bad)
    drawn = {draw_interval() for _ in range(400)}
    assert drawn <= {(i, d) for i in range(1, 7) for d in (-1, 1)} and len(drawn) == 12


def test_option_defaults(tmp_path):
    from accflow_amd import fine_tune, train_acc
    cfg = tmp_path / "c.yml"
    cfg.write_text("exp_name: RAFT-cvo\nlr: !!float 1.2e-4\n")
    o = fine_tune.parse_options(str(cfg))
    assert (o.iters, o.valid_iters, o.gamma) == (12, 20, 0.85)
    for k, v in train_acc.DEFAULTS.items():
        assert getattr(o, k) == v or k == "lr"
    cfg.write_text("exp_name: RAFT-cvo\niters: 8\nvalid_iters: 32\ngamma: 0.8\n")
    o = fine_tune.parse_options(str(cfg))
    assert (o.iters, o.valid_iters, o.gamma) == (8, 32, 0.8)
    cfg.write_text("iters: 8\n")
    with pytest.raises(ValueError):
        fine_tune.parse_options(str(cfg))


def test_trainable_set_is_the_update_block():
    from accflow_amd import train_raft
    model = train_raft.freeze_encoders(_model())
    named = dict(model.named_parameters())
    want = [n for n in named if n.startswith("update_block.")]
    assert len(want) == 30 and sum(named[n].numel() for n in want) == 3120960
    got = train_raft.trainable_parameters(model)
    assert len(got) == 30 and all(a is named[n] for a, n in zip(got, want))
    assert all(p.requires_grad == n.startswith("update_block.") for n, p in named.items())
    assert not model.training and all(not m.training for m in model.modules())
    assert sorted(want) == sorted(R.update_block_names(model.state_dict()))


def test_small_and_gma_are_refused_with_stage_2():
    from accflow_amd import train_raft
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.raft.raft import RAFT, small_args
    z = torch.zeros(1, 256, 16, 16)
    for model in (RAFT(small_args()), build_flow_estimator("gma")):
        with pytest.raises(NotImplementedError, match="stage 2"):
            train_raft.check_model(model)
        with pytest.raises(NotImplementedError, match="stage 2"):
            train_raft.forward_backward(model, z, z, z, torch.zeros(1, 2, 128, 128))
        with pytest.raises(NotImplementedError, match="stage 2"):
            train_raft.forward_backward_frames(model, torch.zeros(1, 3, 128, 128), torch.zeros(1, 3, 128, 128),
                                               torch.zeros(1, 2, 128, 128))
    train_raft.check_model(_model())


def test_checkpoint_keys_carry_the_module_prefix(tmp_path):
    """The estimator's WHOLE state_dict under `module.` (the reference's nn.DataParallel saves), loadable strictly."""
    from accflow_amd import train_acc, train_raft
    from accflow_amd.eval_cvo import _strip_module
    model = train_raft.freeze_encoders(_model())
    args = argparse.Namespace(lr=1.2e-4, wdecay=1e-5, epsilon=1e-8)
    opt, sch = train_acc.fetch_optimizer(args, train_raft.trainable_parameters(model), 10)
    train_acc.save_ckpt(3, sch, opt, model, str(tmp_path), True, {"best_epe": 1.0})
    sd = torch.load(tmp_path / "latest.pth")
    assert all(k.startswith("module.") for k in sd)
    assert {k[7:] for k in sd} == set(model.state_dict())
    assert any(k.startswith("module.fnet.") for k in sd) and any(k.startswith("module.cnet.") for k in sd)
    _model().load_state_dict(_strip_module(sd), strict=True)
    assert torch.load(tmp_path / "latest.state")["iter"] == 3


def test_synthetic_adjacent_labels():
    from accflow_amd.data.synthetic import gt_flow
    from accflow_amd.fine_tune import synthetic_delta_labels
    d = synthetic_delta_labels(torch.zeros(2, 3, 32, 40))
    f, b = d["delta_fflows"][0], d["delta_bflows"][0]
    assert tuple(f.shape) == tuple(b.shape) == (2, 2, 32, 40)
    assert torch.equal(f[0], torch.as_tensor(gt_flow(0, 1, 32, 40)).float()) and torch.equal(f[0], f[1])
    assert torch.equal(b[1], torch.as_tensor(gt_flow(1, 0, 32, 40)).float())
    assert not np.allclose(f.numpy(), 0.0)
