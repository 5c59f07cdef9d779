"""AccFlowStream (networks/AccFlow_.py): backward accumulation over a frame stream, frames pushed `chunk` at a time, against
the reference, against the project's other routes to the same flows, and its state.

Frames are 128 x 256 (1/8 grid 16 x 32, the smallest valid size) unless a test says otherwise; the sequence is the fixtures'
make_sequence(1000, 7, 128, 256).

References and gates.
  * tests/golden/accflow_c1.npz (4 frames: one carry) with the gates of test_hip_parity.test_accflow_c1_vs_golden, mean EPE
    <= 1e-3 px and max <= 5e-4 px.
  * tests/golden/accflow_stream_c1.npz (7 frames: the reference's AccFlow(RAFT) on the CPU, every second row and column of
    F(2->0) .. F(6->0) - tests/golden/make_accflow_stream_golden.py): mean EPE <= 1e-3 px, the project's gate; max EPE <= 4 x
    FORWARD_MAX_EPE, what forward() itself measured against that fixture on the MI355X per output (the margin
    test_raft_small.py uses for box-to-box spread).
  * the project's other routes - forward(), the chain of iter() calls, forward_warm: mean <= 1e-4 px, max <= 2e-3 px, the
    "pipeline vs forward" gate of test_alt_corr.py.  The routes batch the encoders differently (a push encodes its new frames
    only) and take the pair-major correlation route where forward() takes the per-frame operand packs: fp32 rounding.
  * batching: 1e-4 (max abs), as test_estimator_c1_vs_golden_and_oracle.
  * "equal" is torch.equal, under the precondition - asserted first - that two identical forward() calls are bit-equal.
  * memory: see the two tests.

Measured on the MI355X (2026-10-20, f16x3 unless stated; max EPE in px; the tests print every figure):
  * forward() vs accflow_stream_c1, out0..out4: 9.946e-5, 9.253e-5, 1.006e-4, 7.490e-5, 6.853e-5 (mean 7.8e-6 .. 8.7e-6);
    under bf16x6 8.2e-5, 7.0e-5, 7.3e-5, 7.2e-5, 9.7e-5.
  * stream vs accflow_stream_c1: chunk 1 and 3: 7.8e-5, 1.22e-4, 6.8e-5, 7.6e-5, 8.8e-5; chunk 2: 8.4e-5, 7.9e-5, 7.0e-5,
    7.4e-5, 8.3e-5; chunk 5: forward()'s for out0..out2, then 8.1e-5, 8.7e-5; means 7.7e-6 .. 8.7e-6.  Frames 0-3 in f16x3,
    4-6 in bf16x6: 8.4e-5, 7.9e-5, 6.8e-5, 7.0e-5, 9.7e-5.  accflow_c1, chunk 1: 1.10e-4, 1.22e-4.
  * one push of 7 frames vs forward(): bit-equal.  chunk 1 vs the iter() chain: <= 7.0e-5 (mean <= 3.6e-6).  chunk 2 vs
    forward(): RAFTGMA <= 1.44e-4 (mean <= 1.13e-5), RAFT-small <= 1.48e-4 (9.2e-6), alternate_corr <= 1.02e-4 (5.6e-6),
    bf16x6 <= 1.06e-4 (7.8e-6).  warm start, chunk 1 and 3 vs forward_warm: <= 1.47e-4 (7.8e-6).
  * allocated after push 3 and after push 11: 478 046 720 B both.  Peak at 256 x 512, 13 frames: forward() 2522 MB, stream
    chunk=1 1264 MB.
  * batch of two vs each sample alone: <= 6.3e-5 px (see test_batch_of_two).
"""
import pytest
import torch

from oracle import accflow_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy
H, W, SEED, N_FRAMES = 128, 256, 1000, 7
# max EPE (px) of forward() against accflow_stream_c1.npz measured on the MI355X, out0 .. out4
FORWARD_MAX_EPE = (9.946e-5, 9.253e-5, 1.006e-4, 7.490e-5, 6.853e-5)
ROUTE_GATE = (1e-4, 2e-3)      # mean, max EPE between two routes of the project to the same flow


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """A device error poisons the process: nothing more is started on the GPU after one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, session stopped: %s" % e, returncode=3)


def accflow(name="acc|raft", ofe=None, **kw):
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.AccFlow_ import AccFlow
    model = AccFlow(build_flow_estimator(name) if ofe is None else ofe, **kw)
    model.load_state_dict(make_state_dict(model), strict=True)
    return model.cuda().eval()


def sequence(n=N_FRAMES, h=H, w=W, seed=SEED, batch=1):
    from accflow_amd.data.synthetic import make_sequence, normalize
    return [normalize(f).cuda() for f in make_sequence(seed, n, h, w, batch=batch)]


def streamed(model, frames, chunk, stream=None):
    from accflow_amd.networks.AccFlow_ import AccFlowStream
    s = AccFlowStream(model) if stream is None else stream
    outs = []
    for k in range(0, len(frames), chunk):
        got = s.push(frames[k:k + chunk])
        want = max(0, min(k + chunk, len(frames)) - max(k, 2))
        assert len(got) == want and s.n_frames == min(k + chunk, len(frames)), (k, len(got), want, s.n_frames)
        outs += got
    return outs


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def routes_agree(got, want, what, gate=ROUTE_GATE):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == torch.float32 and a.shape == b.shape
        me, mx = O.epe(a.cpu(), b.cpu())
        print("%s out%d: EPE mean %.2e max %.2e" % (what, k, me, mx))
        assert me <= gate[0] and mx <= gate[1], (what, k, me, mx)


def against_stream_golden(g, outs, what):
    assert len(outs) == int(g["n_frames"]) - 2
    figures = [O.epe(o.cpu()[:, :, ::2, ::2], T(g["out%d" % k])) for k, o in enumerate(outs)]
    for k, (me, mx) in enumerate(figures):
        print("%s out%d vs the reference: EPE mean %.3e max %.3e (forward() measured max %.3e)" % (what, k, me, mx, FORWARD_MAX_EPE[k]))
    for k, (me, mx) in enumerate(figures):
        assert torch.isfinite(outs[k]).all()
        assert me <= 1e-3 and mx <= 4 * FORWARD_MAX_EPE[k], (what, k, me, mx, "forward() measured max %.3e" % FORWARD_MAX_EPE[k])


@pytest.fixture(scope="module")
def model(ops):
    return accflow()


@pytest.fixture(scope="module")
def frames():
    return sequence()


@pytest.fixture(scope="module")
def forward7(model, frames):
    """forward() on the 7 frames, computed once; the precondition of every `equal` below is asserted here."""
    outs = model(images=frames)
    assert same(outs, model(images=frames)), "two identical forward() calls are not bit-equal"
    return outs


def test_precondition_and_forward_vs_golden(golden, forward7):
    """forward() is bit-stable run to run, and stands where FORWARD_MAX_EPE says against the 7-frame fixture."""
    against_stream_golden(golden("accflow_stream_c1"), forward7, "forward()")


def test_accflow_c1_vs_golden(golden, model):
    g = golden("accflow_c1")
    fr = sequence(int(g["n_frames"]), int(g["H"]), int(g["W"]), int(g["seed"]))
    outs = streamed(model, fr, 1)
    assert len(outs) == 2
    for k, o in enumerate(outs):     # out1 is the carried step
        me, mx = O.epe(o.cpu(), T(g["out%d" % k]))
        print("stream chunk=1 vs accflow_c1 out%d: EPE mean %.2e max %.2e" % (k, me, mx))
        assert me <= 1e-3 and mx <= 5e-4, (k, me, mx)


@pytest.mark.parametrize("chunk", [1, 2, 3, 5])
def test_stream_vs_golden(golden, model, frames, chunk):
    against_stream_golden(golden("accflow_stream_c1"), streamed(model, frames, chunk), "stream chunk=%d" % chunk)


def test_one_push_vs_forward(model, frames, forward7):
    routes_agree(streamed(model, frames, N_FRAMES), forward7, "one push of 7 vs forward()")


def test_chunk1_vs_iter_chain(model, frames):
    """The reference's step API carries out_small from call to call: a stream that carried downflow8 of the upsampled flow
    instead would differ from it at every step after the first."""
    want, small = [], None
    for i in range(2, N_FRAMES):
        small, up = model.iter(frames[i], frames[i - 1], frames[0], small)
        want.append(up)
    routes_agree(streamed(model, frames, 1), want, "stream chunk=1 vs iter() chain")


@pytest.mark.parametrize("case", ["gma", "small", "alt_corr"])
def test_chunk2_vs_forward_other_estimators(ops, case):
    from accflow_amd.networks.raft.raft import RAFT, small_args
    if case == "small":
        m, fr = accflow(ofe=RAFT(small_args())), sequence(w=192)
    else:
        m, fr = accflow("acc|gma" if case == "gma" else "acc|raft"), sequence()
    if case == "alt_corr":
        m.ofe.args.alternate_corr = True
    routes_agree(streamed(m, fr, 2), m(images=fr), "%s: stream chunk=2 vs forward()" % case)


def test_warm_start_vs_forward_warm(ops, frames):
    m = accflow(warm_start=True, warm_iters=6)
    want = m(images=frames)
    assert len(want) == N_FRAMES - 2
    for chunk in (1, 3):
        routes_agree(streamed(m, frames, chunk), want, "warm start: stream chunk=%d vs forward_warm" % chunk)


def test_batch_of_two(model):
    """N = 2 through one stream against each sample through its own, 7 frames, chunk 2, max |difference| <= 1e-4 px.

    The stream runs the three encoders sample by sample when N > 1 (AccFlowStream._encode_per_sample): the convolution
    planner's schedule depends on the images per encoder call, and with the encoders batched over the samples this test
    measured up to 1.50e-4 px (sample 1, out3; chunk 3: 2.25e-4) - a last-bit difference in an encoder output, grown over 12
    iterations and the chain.  The estimator's refinement and the chain stay batched; on identical inputs they were bit-equal
    between N = 2 and N = 1 at 3 and 4 local frames.  Measured on the MI355X now: sample 0 3.5e-5, 3.5e-5, 9.5e-6, 8.1e-6,
    8.6e-6 px for out0..out4, sample 1 6.3e-5, 5.6e-5, 1.9e-5, 2.9e-5, 1.8e-5."""
    fr = sequence(batch=2)
    both = streamed(model, fr, 2)
    errs = {}
    for n in range(2):
        solo = streamed(model, [f[n:n + 1] for f in fr], 2)
        for k, (a, b) in enumerate(zip(both, solo)):
            errs[n, k] = float((a[n:n + 1] - b).abs().max())
            print("batch sample %d out%d: max |d| %.2e" % (n, k, errs[n, k]))
    assert max(errs.values()) <= 1e-4, errs


def test_reset_and_refused_push(model, frames):
    from accflow_amd.networks.AccFlow_ import AccFlowStream
    s = AccFlowStream(model)
    first = streamed(model, frames, 2, stream=s)
    s.reset()
    assert s.n_frames == 0
    assert same(streamed(model, frames, 2, stream=s), first)
    # a refused push in the middle of a stream changes nothing
    s.reset()
    outs = streamed(model, frames[:4], 2, stream=s)
    for bad in (frames[4][:, :, :120], torch.cat([frames[4], frames[4]]), frames[4].cpu()):
        with pytest.raises((ValueError, RuntimeError)):
            s.push([frames[4], bad])
        assert s.n_frames == 4
    outs += s.push(frames[4:6]) + s.push(frames[6:])
    assert same(outs, first)


def test_accumulate_video(model, frames):
    got = list(model.accumulate_video(iter(frames), chunk=3))
    assert [i for i, _ in got] == list(range(2, N_FRAMES))
    assert same([f for _, f in got], streamed(model, frames, 3))


def test_bf16x6_stream_vs_forward(ops, model, frames):
    with ops.conv_mode("bf16x6"):
        want = model(images=frames)
        got = streamed(model, frames, 2)
    routes_agree(got, want, "bf16x6: stream chunk=2 vs forward()")


def test_mode_change_between_pushes(ops, golden, model, frames):
    """Frames 0-3 in f16x3, 4-6 in bf16x6: the cached features of frames 0 and 3 were made in the other mode and are made
    again from the kept images."""
    from accflow_amd.networks.AccFlow_ import AccFlowStream
    s = AccFlowStream(model)
    outs = s.push(frames[:4])
    with ops.conv_mode("bf16x6"):
        outs += s.push(frames[4:])
    against_stream_golden(golden("accflow_stream_c1"), outs, "f16x3 then bf16x6")


def test_state_is_constant(model):
    """13 frames, one per push: what stays allocated after push 3 (the first that computes) and after push 11 may differ by
    1 MiB at the most - one leaked 128 x 256 frame per push would be 3 MB over those 8 pushes."""
    from accflow_amd.networks.AccFlow_ import AccFlowStream
    fr = sequence(13)
    s = AccFlowStream(model)
    held = {}
    for k, f in enumerate(fr, start=1):
        outs = s.push(f)
        assert len(outs) == (1 if k >= 3 else 0)
        del outs
        if k in (3, 11):
            torch.cuda.synchronize()
            held[k] = torch.cuda.memory_allocated()
    print("allocated after push 3: %d B, after push 11: %d B" % (held[3], held[11]))
    assert abs(held[11] - held[3]) <= 1 << 20, held


def test_peak_memory_256x512(model):
    """13 frames at 256 x 512.  A correlation pyramid is 2048^2 x 4 B x 85/64 = 22.3 MB per pair; forward() holds the 23 of
    its pair schedule at once, the stream's largest push (the first: 3 pairs) three.  At least half of that difference must
    show in the peaks."""
    fr = sequence(13, 256, 512)
    peaks = {}
    for what in ("forward", "stream"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        outs = model(images=fr) if what == "forward" else streamed(model, fr, 1)
        assert len(outs) == 11
        torch.cuda.synchronize()
        peaks[what] = torch.cuda.max_memory_allocated()
        del outs
    pyramid = 2048 ** 2 * 4 * 85 / 64
    print("peak allocated: forward() %.1f MB, stream chunk=1 %.1f MB; one pyramid %.1f MB" % (
        peaks["forward"] / 1e6, peaks["stream"] / 1e6, pyramid / 1e6))
    assert peaks["forward"] - peaks["stream"] >= 0.5 * (23 - 3) * pyramid, peaks
