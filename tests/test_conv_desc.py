"""ops.py hands the kernel library the descriptors it handed it before the descriptor builder was unified.

tests/golden/conv_desc_parent.json holds, for every case of tests/conv_desc_cases.py, the ordered calls of the five
convolution entry points as the parent commit issued them on the GPU (tests/golden/make_conv_desc_golden.py): every
descriptor field, pointers as labels.  Each test replays one case on the current tree and compares call by call, field by
field, together with what the op returned, what it raised and the range guard.

Cases: every row of test_conv_routes.ROWS through its run_row; the branches that table does not reach (pixel-major store,
packed-operand GRU, S16-only destinations, the tap-sum and deformable diversions, the A/B switches, conv2d_multi's variants,
the split-K offer's edges, the replay cache of conv2d / conv2d_tapgemm / corr_lookup_s16, the profiler's figures); and one
forward of RAFT, GMA and AccFlow.
"""
import json
import os

import pytest
import torch

import conv_desc_cases as C

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_desc_parent.json")
MAX_BYTES = 100 * 1024


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_cases():
    g = golden()
    assert list(g) == list(C.CASES), sorted(set(g) ^ set(C.CASES))
    assert os.path.getsize(GOLDEN) < MAX_BYTES


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as o
    assert torch.cuda.is_available()
    assert o.USE_KSPLIT and o.USE_PATCH and not o.S16_VIA_MULTI and o.USE_TAPSUM and o.TAPSUM_F16 and o.USE_DEFORM_COLUMNS
    return o


def fields(text):
    return dict(kv.split("=", 1) for kv in text.split())


def assert_call(name, k, want, got):
    assert want[0] == got[0], (name, k, want[0], got[0])
    if len(want) > 1 and isinstance(want[1], str) and "=" in want[1]:
        fw, fg = fields(want[1]), fields(got[1])
        diff = {f: (fw.get(f, "0"), fg.get(f, "0")) for f in sorted(set(fw) | set(fg)) if fw.get(f) != fg.get(f)}
        assert not diff, "%s, call %d (%s): {field: (recorded, now)} = %s" % (name, k, want[0], diff)
        assert want[2:] == got[2:], (name, k, want, got)
    else:
        assert want == got, (name, k, want, got)


@gpu
@pytest.mark.parametrize("name", list(C.CASES))
def test_descriptors_as_recorded(ops, name):
    want = golden()[name]
    got = C.run_case(ops, name)
    texts = got.pop("_texts", {})
    got = json.loads(json.dumps(got))
    assert not got["guard_tripped"], "the inputs are inside the fp16 split's range"
    assert got.get("raises") == want.get("raises"), name
    assert got.get("returns") == want.get("returns"), (name, got.get("returns"), want.get("returns"))
    if name in C.FORWARDS:
        for k, (iw, ig) in enumerate(zip(want["calls"], got["calls"])):
            w, g = want["distinct"][iw], got["distinct"][ig]
            assert w == g, "%s, call %d: recorded %s, now %s = %s" % (name, k, w, g, texts.get(g[2] if len(g) > 2 else None))
        assert len(got["calls"]) == len(want["calls"]), (name, len(got["calls"]), len(want["calls"]))
        return
    for k, (w, g) in enumerate(zip(want["calls"], got["calls"])):
        assert_call(name, k, w, g)
    assert len(got["calls"]) == len(want["calls"]), (name, [c[0] for c in got["calls"]], [c[0] for c in want["calls"]])
