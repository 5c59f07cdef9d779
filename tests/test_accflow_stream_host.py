"""AccFlowStream's host side without a GPU: what it refuses, and that a refusal leaves the stream as it was."""
import pytest
import torch


def _model():
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.AccFlow_ import AccFlow
    return AccFlow(build_flow_estimator("acc|raft")).eval()


def test_exports():
    import networks.AccFlow_ as shim
    from accflow_amd.networks.AccFlow_ import AccFlowStream
    assert shim.AccFlowStream is AccFlowStream


def test_chunk_below_one_raises():
    m = _model()
    for chunk in (0, -1, 1.5):
        with pytest.raises(ValueError):
            m.accumulate_video([], chunk=chunk)      # (at the call, not at the first next())
    assert list(m.accumulate_video([], chunk=2)) == []


def test_estimator_without_estimate_pairs_is_refused():
    from accflow_amd.networks.AccFlow_ import AccFlow, AccFlowStream
    with pytest.raises(TypeError):
        AccFlowStream(AccFlow(torch.nn.Identity()))


def test_cpu_frame_is_refused_and_state_unchanged(monkeypatch):
    from accflow_amd.networks import AccFlow_ as A
    s = A.AccFlowStream(_model())
    assert s.n_frames == 0 and s.push([]) == []
    with pytest.raises(RuntimeError, match="MI355X"):
        s.push(torch.zeros(1, 3, 128, 256))
    assert s.n_frames == 0 and s._pending == [] and s._state is None and s._like is None
    # frames 0 and 1 are only buffered - no kernel runs - so with the device check out of the way they can be CPU tensors here
    f0, f1 = torch.zeros(1, 3, 128, 256), torch.ones(1, 3, 128, 256)
    with monkeypatch.context() as mp:
        mp.setattr(A, "require_cuda", lambda *t: None)
        assert s.push(f0) == [] and s.n_frames == 1
        assert s.push([f1]) == [] and s.n_frames == 2
        with pytest.raises(ValueError):
            s.push(torch.zeros(1, 3, 120, 256))            # another shape than the stream's
        with pytest.raises(ValueError):
            s.push(torch.zeros(2, 3, 128, 256))            # another batch size
        with pytest.raises(ValueError):
            s.push(torch.zeros(3, 128, 256))
    kept = list(s._pending)
    with pytest.raises(RuntimeError, match="MI355X"):
        s.push([torch.zeros(1, 3, 128, 256)])
    assert s.n_frames == 2 and s._state is None and len(s._pending) == 2
    assert all(a is b for a, b in zip(s._pending, kept))
    assert torch.equal(s._pending[0], f0) and torch.equal(s._pending[1], f1)
    s.reset()
    assert s.n_frames == 0 and s._pending == []
