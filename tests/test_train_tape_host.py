"""tests/acc_train_ref.py (the fusion heads' graph with given ReLU masks) against the oracle, and the gates of
tests/test_train_tape.py against plain fp32 arithmetic - no GPU.

  test_restatement_is_the_oracle    masks=None, float64: every restated function equals the oracle's (torch.equal); gated
                                    with its own signs it gives the same values and, through autograd, the same gradients.
  test_fp32_evaluation_fits_the_gates   at every shape of the GPU tests an fp32 CPU evaluation stands in for the tape: the
                                    sites where its masks differ from float64's signs stay within the cap, and its gradients
                                    against float64 gated by ITS masks stay within HALF the gradient gate - the reference plus
                                    plain fp32 arithmetic fits the gate with room for the kernels' own summation order.  The
                                    figures are printed (measured: gradients 3e-6 .. 2e-5 of the RMS; one disagreeing unit,
                                    in the context encoder at 104 x 136, which moves the UNGATED comparison to 8e-2).
  test_gate_has_teeth               ZeroConv2d's factor 3 dropped from the restatement: the gradient gate rejects it 10 x over.
"""
import functools

import pytest
import torch

import acc_train_ref as A
from oracle import accflow_oracle as O


@functools.lru_cache(maxsize=None)
def _sd():
    return A.state_dict()


@functools.lru_cache(maxsize=None)
def _case(shape):
    return A.case_inputs(shape, _sd())


@functools.lru_cache(maxsize=None)
def _ref64(module, shape):
    return A.evaluate(module, _case(shape), _sd())


def test_restatement_is_the_oracle():
    sd = {k: v.double() for k, v in _sd().items()}
    x = {k: v.double() for k, v in _case("b2_8x9").items()}
    flows = torch.cat([x["flow0"], x["flow1"], x["flow2"]], 0)
    got = {"flow_encoder": A.flow_encoder(flows, sd), "context": A.context_encoder(x["image"], sd),
           "accplus": A.accplus(x["df"], x["f"], x["o"], x["c"], sd), "blending": A.blending(x["f_ini"], x["f"], x["emap"], sd),
           "flow_decoder": A.flow_decoder(x["f_ini"], sd)}
    want = {"flow_encoder": (O.flow_encoder(flows, sd),), "context": (O.basic_encoder(x["image"], sd, "context", "none"),),
            "accplus": O.accplus(x["df"], x["f"], x["o"], x["c"], sd), "blending": (O.blending(x["f_ini"], x["f"], x["emap"], sd),),
            "flow_decoder": O.flow_decoder(x["f_ini"], sd)}
    sites = {"flow_encoder": 2, "context": 1 + 6 * 3, "accplus": 6, "blending": 1, "flow_decoder": 2}
    for m in A.MODULES:
        *outs, pres = got[m]
        assert len(pres) == sites[m] and all(k.startswith(m + ".") for k in pres), (m, sorted(pres))
        for a, b in zip(outs, want[m]):
            if isinstance(b, dict):
                assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in b), m
            else:
                assert torch.equal(a, b), m
        # gated with its own signs: the same graph
        free = A.evaluate(m, _case("b2_8x9"), _sd())
        own = A.evaluate(m, _case("b2_8x9"), _sd(), masks=A.signs(free["pres"]))
        assert all(torch.equal(a, b) for a, b in zip(free["outs"] + free["extra"], own["outs"] + own["extra"])), m
        assert all(torch.equal(free["pres"][k], own["pres"][k]) for k in free["pres"]), m
        assert sorted(free["grads"]) == sorted(own["grads"])
        for k in free["grads"]:
            assert torch.equal(free["grads"][k], own["grads"][k]), (m, k)


@pytest.mark.parametrize("shape", list(A.SHAPES))
@pytest.mark.parametrize("module", A.MODULES)
def test_fp32_evaluation_fits_the_gates(module, shape):
    x, sd = _case(shape), _sd()
    r64 = _ref64(module, shape)
    r32 = A.evaluate(module, x, sd, dtype=torch.float32)
    masks = A.signs(r32["pres"])
    gated = A.evaluate(module, x, sd, masks=masks)
    fgate = A.forward_gate(module, "bf16x6")                  # the tighter of the two modes' forward gates
    dis = A.mask_disagreements(masks, r64["pres"], fgate)
    errs = {k: A.grad_error(r32["grads"][k], gated["grads"][k]) for k in gated["grads"]}
    ungated = max(A.grad_error(r32["grads"][k], r64["grads"][k]) for k in r64["grads"])
    fwd = max(float((a.double() - b).abs().max()) / A.rms(b) for a, b in zip(r32["outs"], r64["outs"]))
    worst = max(errs, key=errs.get)
    print("%s %s: fp32 vs float64 - gradient %.2e of the RMS at %s (gate %.0e; against the UNGATED float64 graph %.2e), forward "
          "%.2e (gate %.1e), mask disagreements %d over %d sites (worst |pre64| %.2e of its bound)"
          % (module, shape, errs[worst], worst, A.GRAD_TOL, ungated, fwd, fgate, sum(v[0] for v in dis.values()), len(dis),
             max(v[2] for v in dis.values())))
    assert all(n <= cap and w < 1.0 for n, cap, w in dis.values()), {k: v for k, v in dis.items() if v[0]}
    assert fwd <= fgate
    assert errs[worst] <= 0.5 * A.GRAD_TOL, (worst, errs[worst])


def test_gate_has_teeth():
    """accplus.conv2.4.scale's factor 3 dropped (exp(scale) for exp(3 scale)) in the restatement, everything else the
    reference's own: the scale's gradient, and the gradients of everything in front of the ZeroConv2d, leave the gate by more
    than 10 x."""
    x, sd = _case("b2_8x9"), _sd()
    good = _ref64("accplus", "b2_8x9")
    bad = A.evaluate("accplus", x, sd, masks=A.signs(good["pres"]), scale_factor=1)
    errs = {k: A.grad_error(bad["grads"][k], good["grads"][k]) for k in good["grads"]}
    print("factor 3 dropped: accplus.conv2.4.scale %.2e, accplus.conv2.0.weight %.2e, in/c %.2e of the RMS (gate %.0e)"
          % (errs["accplus.conv2.4.scale"], errs["accplus.conv2.0.weight"], errs["in/c"], A.GRAD_TOL))
    for k in ("accplus.conv2.4.scale", "accplus.conv2.4.conv.weight", "accplus.conv2.2.weight", "accplus.conv2.0.weight", "in/c"):
        assert errs[k] > 10 * A.GRAD_TOL, (k, errs[k])
