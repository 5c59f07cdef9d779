"""forward_interpolate (reference networks/raft/utils/utils.py:31-63; csrc/forward_interp.hip): RAFT's warm start for video.

References.
  * tests/golden/forward_interp.npz: what the reference's function (scipy griddata, nearest) returns for six flows
    (tests/golden/make_forward_interp_golden.py).
  * `restate`: a float64 NumPy brute force with the kernel's rules - source s sits at (xs + dx, ys + dy) in float64 (the
    reference adds an int64 grid to a float32 flow), is valid iff 0 < x1 < w and 0 < y1 < h (NaN and +-inf fail every
    comparison), every target takes the valid source with the smallest (x1 - x0)^2 + (y1 - y0)^2, each product and the sum
    rounded once, an exact tie goes to the lowest row-major source index (argmin returns the first minimum of the sources
    in ascending order), and an item without a valid source is all zeros.

Tolerances.  None: the outputs are COPIES of input values, so every comparison is `==`.  Against the reference's outputs the
only exemption is a target whose two smallest squared distances differ by at most 1e-9 relative - scipy's k-d tree resolves
such a tie in an unspecified way - and at most 0.5 % of a case's targets may be exempt (measured: 0 exempt targets and 0
mismatches in all six cases).  Against `restate` the kernel has no exemption at all.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

CASES = ["rand3_16x32", "rand3_33x47", "rand12_13x19", "zero_16x32", "shift_16x32", "smooth_33x47"]
TIE_REL = 1e-9
EXEMPT_CAP = 0.005
FAR = 1000.0          # a flow that takes its source out of every frame used here


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "forward_interp.npz")))


def restate(flow, want_near_ties=False):
    """flow: (2, h, w) float32 array -> (2, h, w) float32 [, (h, w) bool: targets whose two nearest sources are within TIE_REL]."""
    flow = np.asarray(flow, dtype=np.float32)
    _, h, w = flow.shape
    rows, cols = np.indices((h, w)).reshape(2, -1).astype(np.float64)     # every cell, row-major: target AND source grid
    u, v = flow.reshape(2, -1)
    with np.errstate(invalid="ignore"):
        px, py = cols + u.astype(np.float64), rows + v.astype(np.float64)
        kept = np.flatnonzero((0 < px) & (px < w) & (0 < py) & (py < h))  # (ascending source index)
    out = np.zeros((2, h * w), dtype=np.float32)
    near = np.zeros(h * w, dtype=bool)
    if kept.size:
        px, py = px[kept], py[kept]
        for t0 in range(0, h * w, 512):                                   # (targets in blocks: P x P doubles are too many)
            ex = px[None, :] - cols[t0:t0 + 512, None]
            ey = py[None, :] - rows[t0:t0 + 512, None]
            d = ex * ex + ey * ey
            k = kept[np.argmin(d, axis=1)]                                # (first minimum = lowest source index)
            out[:, t0:t0 + 512] = flow.reshape(2, -1)[:, k]
            if want_near_ties and d.shape[1] > 1:
                two = np.partition(d, 1, axis=1)[:, :2]
                near[t0:t0 + 512] = (two[:, 1] - two[:, 0]) <= TIE_REL * two[:, 1]
    out = out.reshape(2, h, w)
    return (out, near.reshape(h, w)) if want_near_ties else out


def assert_equals_reference(got, fixture, name):
    """`got` == the reference's output for fixture case `name`, but for near-tie targets (at most EXEMPT_CAP of them)."""
    want = fixture[name + ".out"]
    _, near = restate(fixture[name + ".flow"], want_near_ties=True)
    exempt = int(near.sum())
    wrong = int(((np.asarray(got) != want).any(axis=0) & ~near).sum())
    print("%s: %d targets, %d exempt (near ties), %d mismatches" % (name, near.size, exempt, wrong))
    assert exempt <= EXEMPT_CAP * near.size, (name, exempt, near.size)
    assert wrong == 0, (name, wrong)


# ---------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(fixture, name):
    flow = fixture[name + ".flow"]
    assert flow.dtype == np.float32 and fixture[name + ".out"].dtype == np.float32
    assert flow.shape == fixture[name + ".out"].shape == (2,) + tuple(int(v) for v in name.split("_")[1].split("x"))
    assert_equals_reference(restate(flow), fixture, name)


def test_restatement_rules():
    """A self-check of the test-local oracle `restate` alone, on hand-made flows: it runs no product code (and passes without the
    feature).  The kernel meets the same rules in the GPU tests below."""
    z = restate(np.zeros((2, 4, 5), np.float32))
    assert not z.any()                                     # (every source keeps its own flow: zeros)
    f = np.full((2, 9, 9), FAR, np.float32)
    assert not restate(f).any()                            # no valid source: zeros
    f[:, 0, 3] = (3, 4)                                    # index 3 lands at (x, y) = (6, 4)
    f[:, 8, 8] = (-6, -4)                                  # index 80 lands at (2, 4)
    out = restate(f)
    assert (out[:, :, :4] == np.array([-6, -4], np.float32)[:, None, None]).all()
    assert (out[:, :, 4:] == np.array([3, 4], np.float32)[:, None, None]).all()      # x = 4 ties: the lower index
    f = np.full((2, 5, 6), np.nan, np.float32)
    f[:, 2, 2] = (0.5, 0.25)
    f[1, 3, 3] = 0.0                                       # NaN in one component only: invalid
    assert (restate(f) == np.array([0.5, 0.25], np.float32)[:, None, None]).all()


def test_helper_is_importable_where_the_reference_has_it():
    from accflow_amd import ops
    from accflow_amd.networks.raft.utils.utils import forward_interpolate as a
    from accflow_amd.networks.gma.utils.utils import forward_interpolate as b
    from accflow_amd.networks.utils import forward_interpolate as c
    from networks.utils import forward_interpolate as d
    assert a is b is c is d and callable(ops.forward_interpolate)
    for fn in (a, ops.forward_interpolate):                # no CPU path: the usual error
        with pytest.raises(RuntimeError):
            fn(torch.zeros(2, 4, 5))
    from accflow_amd.networks.raft.raft import RAFT
    from accflow_amd.networks.gma.gma import RAFTGMA
    assert issubclass(RAFTGMA, RAFT) and callable(RAFTGMA.estimate_video)


# ---------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def fi():
    from accflow_amd import ops
    assert torch.cuda.is_available()
    return ops.forward_interpolate


def run(fi, flow):
    return fi(torch.from_numpy(np.ascontiguousarray(flow)).cuda()).cpu()


def restate_batch(flows):
    return torch.from_numpy(np.stack([restate(f) for f in flows]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_kernel_vs_reference_fixture(fi, fixture, name):
    got = run(fi, fixture[name + ".flow"])                 # (2, h, w) in, (2, h, w) out
    assert got.dtype == torch.float32 and tuple(got.shape) == fixture[name + ".flow"].shape
    assert_equals_reference(got.numpy(), fixture, name)


BATCHES = {
    "16x32 B=3": ["rand3_16x32", "zero_16x32", "shift_16x32"],
    "16x32 B=2": ["shift_16x32", "rand3_16x32"],
    "33x47 B=2": ["rand3_33x47", "smooth_33x47"],          # P = 1 551: one full LDS chunk plus a tail
    "33x47 B=3": ["smooth_33x47", "rand3_33x47", "smooth_33x47"],
    "13x19 B=1": ["rand12_13x19"],                         # P = 247: fewer targets than one workgroup has threads
}


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(BATCHES))
def test_kernel_equals_restatement_on_fixture_batches(fi, fixture, key):
    flows = np.stack([fixture[n + ".flow"] for n in BATCHES[key]])
    assert torch.equal(run(fi, flows), restate_batch(flows))


@pytest.mark.gpu
def test_kernel_equals_restatement_at_working_size(fi):
    """60 x 128 = the 1/8 resolution of 480 x 1024: 240 workgroups, 8 LDS chunks, every share of the source split busy."""
    g = torch.Generator().manual_seed(11)
    flows = (torch.randn(1, 2, 60, 128, generator=g) * 3).numpy()
    assert torch.equal(run(fi, flows), restate_batch(flows))


@pytest.mark.gpu
@pytest.mark.parametrize("low_first", [True, False])
def test_exact_tie_takes_the_lowest_source_index(fi, low_first):
    """Two valid sources at (x, y) = (2, 4) and (6, 4) of a 9 x 9 grid, integer flows: every distance is exact, column
    x = 4 is equidistant and must take the source with the lower row-major index - whichever side it landed on."""
    f = np.full((2, 9, 9), FAR, np.float32)
    if low_first:
        f[:, 0, 3], f[:, 8, 8] = (-1, 4), (-2, -4)         # index 3 -> (2, 4), index 80 -> (6, 4)
        left, right, tie = (-1, 4), (-2, -4), (-1, 4)
    else:
        f[:, 0, 3], f[:, 8, 8] = (3, 4), (-6, -4)          # index 3 -> (6, 4), index 80 -> (2, 4)
        left, right, tie = (-6, -4), (3, 4), (3, 4)
    out = run(fi, f)
    col = lambda v: torch.tensor(v, dtype=torch.float32)[:, None, None]
    assert torch.equal(out[:, :, :4], col(left).expand(2, 9, 4))
    assert torch.equal(out[:, :, 5:], col(right).expand(2, 9, 4))
    assert torch.equal(out[:, :, 4:5], col(tie).expand(2, 9, 1))
    assert torch.equal(out, torch.from_numpy(restate(f)))


@pytest.mark.gpu
def test_single_valid_source_fills_the_frame(fi):
    f = np.full((1, 2, 13, 19), FAR, np.float32)
    f[0, :, 7, 11] = (-2.25, 3.5)
    out = run(fi, f)
    assert torch.equal(out, torch.tensor([-2.25, 3.5])[None, :, None, None].expand(1, 2, 13, 19))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["far", "nan", "+inf", "-inf"])
def test_item_without_a_valid_source_is_zeros(fi, fixture, kind):
    """The reference raises inside scipy; here that item of a batch of three is zeros and its neighbours are unaffected."""
    fill = {"far": FAR, "nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind]
    flows = np.stack([fixture["rand3_16x32.flow"], np.full((2, 16, 32), fill, np.float32), fixture["shift_16x32.flow"]])
    out = run(fi, flows)
    assert not out[1].any() and torch.isfinite(out).all()
    assert torch.equal(out, restate_batch(flows))


@pytest.mark.gpu
def test_nan_in_one_component_invalidates_the_source(fi, fixture):
    f = fixture["rand3_33x47.flow"].copy()
    g = torch.Generator().manual_seed(3)
    hit = torch.rand(33, 47, generator=g).numpy()
    f[0][hit < 0.2] = np.nan                               # x only
    f[1][hit > 0.8] = np.nan                               # y only
    f[1][(hit > 0.4) & (hit < 0.45)] = np.inf
    out = run(fi, f)
    assert torch.isfinite(out).all()
    assert torch.equal(out, torch.from_numpy(restate(f)))


@pytest.mark.gpu
def test_wrapper_inputs_out_and_repeatability(fi, fixture):
    from accflow_amd.networks.raft.utils.utils import forward_interpolate
    flows = np.stack([fixture["rand3_33x47.flow"], fixture["smooth_33x47.flow"]])
    want = restate_batch(flows)
    x = torch.from_numpy(flows).cuda()
    nc = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)           # channel-last memory: not contiguous
    assert not nc.is_contiguous() and torch.equal(fi(nc).cpu(), want)
    half = x.half()
    got = fi(half)
    assert got.dtype == torch.float32 and got.device == x.device
    assert torch.equal(got.cpu(), restate_batch(half.float().cpu().numpy()))
    out = torch.full_like(x, 7.0)
    assert fi(x, out=out) is out and torch.equal(out.cpu(), want)
    with pytest.raises(RuntimeError):
        fi(x, out=x)
    store = torch.zeros(x.numel() + 8, device="cuda")
    shifted_in, shifted_out = store[:x.numel()].view_as(x), store[8:].view_as(x)      # partly overlapping views of one storage
    with pytest.raises(RuntimeError):
        fi(shifted_in, out=shifted_out)
    with pytest.raises(RuntimeError):
        fi(x, out=torch.empty(2, 2, 33, 48, device="cuda"))
    first, second = fi(x), fi(x)
    assert first.data_ptr() != second.data_ptr() and torch.equal(first, second)
    # the reference's helper: (2, h, w) in, (2, h, w) float out - here on the input's device; a batch too
    one = forward_interpolate(x[1])
    assert one.is_cuda and tuple(one.shape) == (2, 33, 47) and torch.equal(one.cpu(), want[1])
    assert torch.equal(forward_interpolate(x).cpu(), want)
