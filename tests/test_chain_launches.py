"""Every schedule of AccFlow's fusion chain launches what it launched before the chain's copies became one step and one loop.

tests/golden/chain_launches_parent.json holds, for the cases below, the ordered calls into the kernel library as the commit
named in its "recorded_at" issued them on the GPU (tests/golden/make_chain_launch_golden.py): conv_desc_cases.Recorder in its
forward mode - the five convolution entry points, every descriptor field, pointers as labels - extended by the other entry
points the chain launches (EXTRA: scalar arguments, pointers as labels).  Distinct calls are stored once for the whole file, a
convolution as (entry point, summary, descriptor digest), and each case as its order of indices into them.  Each test replays
one case on the current tree and compares call by call, with the type and shape of what was returned and the range guard.

Frames and synthetic weights are test_ragged_frames': B is 104x136 (a 13x17 grid), E 64x72 (8x9, the smallest the correlation
route takes); 2 estimator iterations.
"""
import json
import os

import pytest
import torch

import conv_desc_cases as C
import test_ragged_frames as RF

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_launches_parent.json")
MAX_BYTES = 100 * 1024
EXTRA = ("accflow_to_s16_f32", "accflow_flow_from_coords_s16", "accflow_get_occ_s16", "accflow_get_occ_f32", "accflow_blend_s16",
         "accflow_blend_f32", "accflow_deform_columns_s16", "accflow_convex_upsample_f32", "accflow_compose_flow_f32",
         "accflow_downflow8_f32", "accflow_copy_f32")


def frames(tag, n, N=1):
    return [f.cuda() for f in RF.frames(tag, n, N)]


def warm_model():
    def make():
        from accflow_amd.networks import build_flow_estimator
        from accflow_amd.networks.AccFlow_ import AccFlow
        m = AccFlow(build_flow_estimator("acc|raft"), warm_start=True)
        m.load_state_dict(RF.weights("acc|raft")[0], strict=True)
        return m.cuda().eval()
    return RF.cached(("model", "acc|raft warm"), make)


def pushes(model, fr, chunk):
    from accflow_amd.networks.AccFlow_ import AccFlowStream
    s = AccFlowStream(model)
    return [s.push(fr[k:k + chunk]) for k in range(0, len(fr), chunk)]


def forward_hoisted_deferred(m):
    """model(images), 5 frames: the hoisted and deferred chain, the context encoder on the side stream"""
    return m(images=frames("B", 5))


def forward_hoisted_deferred_batch2(m):
    """... with two samples: the (step, sample) indexing of the batched invariants"""
    return m(images=frames("E", 5, 2))


def sequence_pipeline(m):
    """the stepwise and deferred chain without split-K, through the side-stream harness"""
    from accflow_amd.parallel import SequencePipeline
    pipe = SequencePipeline(m)
    return [pipe.submit(frames("B", 5)), pipe.flush()]


def stream_chunk2(m):
    """AccFlowStream: a pending push, a forward of 4 frames, then carried state into a 3-frame stepwise chain"""
    return pushes(m, frames("B", 5), 2)


def stream_chunk3_batch2(m):
    """AccFlowStream with two samples: the encoders sample by sample (_encode_per_sample)"""
    return pushes(m, frames("E", 5, 2), 3)


def warm_start(m):
    """forward_warm on 4 frames and the same frames one by one through AccFlowStream"""
    w = warm_model()
    w.ofe_iters = 2
    try:
        return [w(images=frames("B", 4)), pushes(w, frames("B", 4), 1)]
    finally:
        del w.ofe_iters


def iter_module_form(m):
    """iter(): the module-form step"""
    I1, I2, In = frames("B", 3)
    return m.iter(I1, I2, In, None)


def forward_stepwise_per_step_decoder(m):
    """hoisting and deferral off: every step encodes its own inputs and runs the whole decoder"""
    from accflow_amd.networks import AccFlow_ as A
    with C.patched(A, USE_CHAIN_HOIST="0", USE_CHAIN_DEFER_UP=False):
        return m(images=frames("B", 5))


CASES = {f.__name__: f for f in (forward_hoisted_deferred, forward_hoisted_deferred_batch2, sequence_pipeline, stream_chunk2,
                                 stream_chunk3_batch2, warm_start, iter_module_form, forward_stepwise_per_step_decoder)}


def run_case(ops, name):
    """-> (calls, returns, guard_tripped, texts): the calls as tuples - a convolution as (entry point, summary, digest) [+ what
    the query returned], any other entry point with its arguments - from a fresh split-K scratch and a quiet guard, as
    conv_desc_cases.run_case starts; texts: digest -> the descriptor's text, for the failure message."""
    assert ops.current_mode() == ops.CONV_F16X3
    ops._tls.__dict__.pop("ksplit_ws", None)
    ops.guard_tripped()
    ops.guard_report()
    m = RF.model("acc|raft")
    saved = m.__dict__.get("ofe_iters")
    m.ofe_iters = 2
    rec = C.Recorder(ops, forward=True, extra=EXTRA)
    try:
        with rec, torch.no_grad():
            ret = C.shape_of(CASES[name](m), ops)
        torch.cuda.synchronize()
    finally:
        if saved is None:
            del m.ofe_iters
        else:
            m.ofe_iters = saved
    tripped = ops.guard_tripped() or bool(ops.guard_report())
    calls, texts = [], {}
    for c in rec.calls:
        if len(c) > 1 and isinstance(c[1], str) and "=" in c[1]:
            texts[C.digest(c[1])] = c[1]
            c = [c[0], C.summary(c[1]), C.digest(c[1])] + c[2:]
        calls.append(tuple(c))
    return calls, ret, tripped, texts


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_cases():
    g = golden()
    assert list(g["cases"]) == list(CASES), sorted(set(g["cases"]) ^ set(CASES))
    assert len(g["recorded_at"]) == 40
    assert os.path.getsize(GOLDEN) < MAX_BYTES


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_launches_as_recorded(name):
    from accflow_amd import ops
    assert torch.cuda.is_available()
    g = golden()
    want = g["cases"][name]
    calls, returns, tripped, texts = run_case(ops, name)
    calls = json.loads(json.dumps(calls))
    assert not tripped, "the inputs are inside the fp16 split's range"
    assert json.loads(json.dumps(returns)) == want["returns"], (name, returns, want["returns"])
    for k, (iw, got) in enumerate(zip(want["calls"], calls)):
        w = g["distinct"][iw]
        assert w == got, "%s, call %d: recorded %s, now %s = %s" % (name, k, w, got, texts.get(got[2] if len(got) > 2 else None))
    assert len(calls) == len(want["calls"]), (name, len(calls), len(want["calls"]))
