"""RAFT's warm start over a frame stream: estimate_pairs(return_low=True) and estimate_video (networks/raft/raft.py, inherited
by RAFTGMA) at the smallest valid frame size, 128 x 256 (1/8 resolution 16 x 32), T = 4 frames, N = 1 and 2, iters = 3.

What is pinned here is the ORDER of the calls, the seeds and the batching - every comparison of two ways to run the same
launches is torch.equal; the precondition, that two identical estimate_pairs calls are bit-equal, is asserted first.  The
arithmetic of the pieces is pinned elsewhere (tests/test_hip_parity.py: the estimators against the reference's outputs;
tests/test_forward_interp.py: the interpolation kernel).  One comparison crosses two different routes - estimate_pairs on
encoded frames against forward() on the two images, with the same flow_init - and uses the gates of the existing flow_init
golden check (test_estimator_c1_vs_golden_and_oracle: mean EPE <= 1e-3 px, max <= 1e-4 px RAFT / 1e-3 px GMA; measured on
the MI355X: max 1.5e-5 px RAFT, 1.3e-4 px GMA).  A batched call and a one-pair call are compared on the SAME encoder
outputs (`features=`): the refinement is bit-stable under batching, the encoders are not (4 frames against 2 in one encoder
call take other convolution schedules; test_return_low prints that difference in flow_low as information - it is fp32
rounding, up to 6e-6 px RAFT and 5e-5 px GMA on the MI355X, and not pinned here).
"""
import pytest
import torch

from oracle import accflow_oracle as O

pytestmark = pytest.mark.gpu

H, W, T, ITERS = 128, 256, 4, 3
PAIRS = [(t, t + 1) for t in range(T - 1)]
INIT_GATE = {"raft": 1e-4, "gma": 1e-3}      # max EPE of the flow_init golden check


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module", params=["raft", "gma"])
def model(request):
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    m = build_flow_estimator(request.param)
    m.load_state_dict(make_state_dict(m), strict=True)
    return request.param, m.cuda().eval()


@pytest.fixture(scope="module", params=[1, 2])
def frames(request):
    from accflow_amd.data.synthetic import make_sequence, normalize
    return [normalize(f).cuda() for f in make_sequence(1004, T, H, W, batch=request.param)]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def test_return_low(ops, model, frames):
    name, m = model
    N = frames[0].shape[0]
    plain = m.estimate_pairs(frames, PAIRS, ITERS)
    assert torch.equal(plain, m.estimate_pairs(frames, PAIRS, ITERS))            # precondition: run-to-run bit-equal
    up, low = m.estimate_pairs(frames, PAIRS, ITERS, return_low=True)
    assert tuple(up.shape) == (len(PAIRS) * N, 2, H, W) and tuple(low.shape) == (len(PAIRS) * N, 2, H // 8, W // 8)
    assert low.dtype == torch.float32 and low.is_contiguous()
    assert torch.equal(up, plain)                                                # the default path returns what it did
    assert isinstance(plain, torch.Tensor)
    feats = m.encode_pairs(frames, PAIRS)        # (both calls refine the SAME encoder outputs: the frames encoded once)
    assert same(m.estimate_pairs(frames, PAIRS, ITERS, features=feats, return_low=True), (up, low))
    for k, pair in enumerate(PAIRS):
        up1, low1 = m.estimate_pairs(frames, [pair], ITERS, features=feats, return_low=True)
        d_low = float((low[k * N:(k + 1) * N] - low1).abs().max())
        d_up = float((up[k * N:(k + 1) * N] - up1).abs().max())
        print("%s N=%d pair %s: batched vs one-pair call, max |d flow_low| %.3e, max |d flow_up| %.3e" % (name, N, pair, d_low, d_up))
        assert torch.equal(low[k * N:(k + 1) * N], low1)
        own = m.estimate_pairs(frames, [pair], ITERS, return_low=True)[1]     # (information: this pair's two frames encoded alone)
        print("%s N=%d pair %s: one-pair call on its own encoder outputs, max |d flow_low| %.3e" % (
            name, N, pair, float((low[k * N:(k + 1) * N] - own).abs().max())))
        # the low-resolution flow is what the full-resolution one was upsampled from: same call, same pair
        assert torch.equal(up1, m.estimate_pairs(frames, [pair], ITERS, features=feats))


def test_cold_video_is_one_batched_call(ops, model, frames):
    name, m = model
    want = m.estimate_pairs(frames, PAIRS, ITERS, return_low=True)
    assert same(want, m.estimate_pairs(frames, PAIRS, ITERS, return_low=True))   # precondition
    assert same(m.estimate_video(frames, iters=ITERS, warm_start=False), want)
    feats = m.encode_pairs(frames, PAIRS)
    assert same(m.estimate_video(frames, iters=ITERS, warm_start=False, pairs=PAIRS, features=feats), want)


def written_out(ops, m, frames, first, rest):
    feats = m.encode_pairs(frames, PAIRS, None)
    ups, lows = [], []
    for k, pair in enumerate(PAIRS):
        seed = ops.forward_interpolate(lows[-1]) if k else None
        up, low = m.estimate_pairs(frames, [pair], first if k == 0 else rest, flow_init=seed, features=feats, return_low=True)
        ups.append(up)
        lows.append(low)
    return torch.cat(ups), torch.cat(lows)


def test_warm_video_is_the_loop_written_out(ops, model, frames):
    name, m = model
    want = written_out(ops, m, frames, ITERS, ITERS)
    assert same(want, written_out(ops, m, frames, ITERS, ITERS))                 # precondition
    got = m.estimate_video(frames, iters=ITERS)                                  # (warm_start defaults to True)
    assert same(got, want)
    assert same(m.estimate_video(frames, iters=ITERS, warm_start=True, pairs=PAIRS), want)


def test_seed_is_used(ops, model, frames):
    name, m = model
    N = frames[0].shape[0]
    warm_up, warm_low = m.estimate_video(frames, iters=ITERS, warm_start=True)
    cold_up, cold_low = m.estimate_video(frames, iters=ITERS, warm_start=False)
    seed = ops.forward_interpolate(warm_low[:N])
    direct = m(frames[1], frames[2], iters=ITERS, flow_init=seed)
    me, mx = O.epe(warm_up[N:2 * N].cpu(), direct.cpu())
    print("%s N=%d: warm pair 1 vs forward(flow_init=seed): EPE mean %.2e max %.2e" % (name, N, me, mx))
    assert me <= 1e-3 and mx <= INIT_GATE[name], (name, me, mx)
    me_c, mx_c = O.epe(warm_up[N:2 * N].cpu(), cold_up[N:2 * N].cpu())
    print("%s N=%d: warm pair 1 vs cold pair 1: EPE mean %.2e max %.2e" % (name, N, me_c, mx_c))
    assert not torch.equal(warm_up[N:2 * N], cold_up[N:2 * N])                   # another start, another result


def test_iters_pair(ops, model, frames):
    name, m = model
    N = frames[0].shape[0]
    up, low = m.estimate_video(frames, iters=(ITERS, 2))
    assert tuple(up.shape) == (len(PAIRS) * N, 2, H, W) and tuple(low.shape) == (len(PAIRS) * N, 2, H // 8, W // 8)
    assert torch.isfinite(up).all() and torch.isfinite(low).all()
    assert same((up, low), written_out(ops, m, frames, ITERS, 2))
    assert not torch.equal(up[N:], m.estimate_video(frames, iters=ITERS)[0][N:])                      # `rest` is used
