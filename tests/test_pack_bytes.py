"""The weight / operand packs and the GEMM host routes built on them write the bytes they wrote before the pack kernels
moved to csrc/conv_pack.hip and their numeric rules (row scale, term splits, k-table entry) to csrc/pack_terms.h.

tests/golden/pack_bytes_parent.json holds, for every case of tests/pack_bytes_cases.py, the SHA-256 digest of each buffer
as the parent commit wrote it on the GPU (tests/golden/make_pack_bytes_golden.py; every case was run twice there and
recorded only when both runs agreed).  test_fused_pack_equals_the_single_purpose_packs compares two paths that share the
rules, so it cannot see a mistake made in the shared rule; this one can.
Recorded again since ("_rerecorded" in the file says which and why): levels 1..3 of the four corr_volume_disp_packed cases,
whose C = 32 makes the accumulator scale no power of two - the level-1 emission of corr_disp_store2 scales every tap
before it sums since tests/test_corr_routes.py holds it to the pool of the stored level 0; their lvl0 and packs digests,
and every other case, are the first recording's.

Cases: the five single-purpose pack entry points and accflow_conv_pack_all_f32 (plain and transpose_flip) on the eight
shapes of that test, accflow_conv_pack_multi16 on three sources, accflow_corr_pack_f32 in the three split modes (one input
out of the fp16 range, guard word included); through accflow_amd.ops the correlation volume (row-major, displaced, from
per-frame packs) and GMA's attention + aggregation on the transposed, the pre-split and the matrix-free route.
"""
import json
import os

import pytest

import pack_bytes_cases as C

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_bytes_parent.json")
MAX_BYTES = 64 * 1024


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


RECORDED = [k for k in golden() if not k.startswith("_")]


def test_golden_covers_the_cases():
    g = golden()
    assert set(g["_unstable"]) <= set(C.CASES)
    assert RECORDED == [k for k in C.CASES if k not in g["_unstable"]], sorted(set(RECORDED) ^ set(C.CASES))
    assert os.path.getsize(GOLDEN) < MAX_BYTES
    for name in RECORDED:
        assert g[name] and all(len(d) == 64 and set(d) <= set("0123456789abcdef") for d in g[name].values()), name


@gpu
@pytest.mark.parametrize("name", RECORDED)
def test_bytes_as_recorded(name):
    want = golden()[name]
    got = C.run_case(name)
    assert sorted(got) == sorted(want), (name, sorted(got), sorted(want))
    diff = [k for k in want if got[k] != want[k]]
    assert not diff, "%s: buffers %s differ from the parent's bytes" % (name, diff)
