"""alternate_corr (the reference's args.alternate_corr, raft/raft.py:45-46): the CorrBlock lookup computed on the fly from the
feature maps (csrc/corr_alt.hip, networks/raft/corr.py AlternateCorrBlock) - against float64, against the volume lookups of
the same library, through RAFT / AccFlow against the reference's golden outputs, its memory, a 4K sequence, and the switch."""
import math

import pytest
import torch

from oracle import accflow_oracle as O

T = torch.from_numpy
gpu = pytest.mark.gpu


def dev(t):
    return t.cuda()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def maxerr(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def _coords(B, h, w, g, kind):
    if kind == "smooth":
        flow = torch.nn.functional.interpolate(3.0 * torch.randn(B, 2, 3, 4, generator=g), size=(h, w), mode="bilinear",
                                               align_corners=True)
    elif kind == "noise":
        flow = 4.0 * torch.randn(B, 2, h, w, generator=g)
    elif kind == "wild":        # boxes beyond the LDS budget: the tiles' direct-read path
        flow = 40.0 * torch.randn(B, 2, h, w, generator=g)
    else:
        flow = torch.zeros(B, 2, h, w)
    c = O.coords_grid(B, h, w) + flow
    if kind == "noise":         # tests/test_lookup_fused.py's special coordinates
        c[0, :, 0, :4] = torch.tensor([[-30.0, -3.5, 1e5, float(w) + 2.25], [2.0, -9.0, 3.0, float(h) - 0.5]])
        c[0, :, 1, :3] = torch.tensor([[4.0, float(w - 1), 0.0], [0.0, float(h - 1), -1.0]])
        c[0, :, 2, :2] = torch.tensor([[-1e9, float("inf")], [1e9, 0.0]])
        c[0, :, 3, :3] = torch.tensor([[float("nan"), -7.5, float("-inf")], [2.0, 3.25, float("nan")]])
    return c


def _want64(f1, f2, coords):
    pyr = O.corr_pyramid(f1.double(), f2.double())
    c = torch.nan_to_num(coords, nan=-1e6, posinf=1e6, neginf=-1e6).clamp(-1e6, 1e6)
    return O.corr_lookup(pyr, c.double())


# (B, F, C, H8, W8): ragged last tiles (W8 % 16, H8 % 4), odd level sizes (18x22: level 3 is 2x2), more items than frames
ALT_CASES = [(2, 4, 256, 16, 32), (3, 2, 256, 18, 22), (1, 2, 64, 9, 11), (4, 3, 256, 60, 128)]


@gpu
@pytest.mark.parametrize("case", ALT_CASES)
def test_alt_lookup_vs_float64_and_volume(ops, case):
    from accflow_amd.networks.raft.corr import AlternateCorrBlock
    B, F, C, h, w = case
    g = gen(41)
    frames = torch.randn(F, C, h, w, generator=g)
    idx1 = [b % F for b in range(B)]                   # repeated frame indices
    idx2 = [(b * 2 + 1) % F for b in range(B)]
    f1, f2 = frames[idx1], frames[idx2]
    blk = AlternateCorrBlock.from_frames(dev(frames), idx1, idx2)
    with pytest.raises(AttributeError):
        blk.corr_pyramid
    for kind in ("smooth", "noise", "zero", "wild"):
        coords = _coords(B, h, w, g, kind)
        want = _want64(f1, f2, coords)
        got = blk(dev(coords))
        rms = float(want.pow(2).mean().sqrt())
        err = maxerr(got, want)
        assert bool(torch.isfinite(got).all())
        # (item 1 of the 18x22 case correlates a frame with itself: |f|^2 / 16 = 16 at zero displacement, ~10x the RMS)
        assert err <= 1e-4 * rms, ("alt lookup vs float64", case, kind, err / rms, "measured <= 7.6e-5 of the RMS")
        # the fp32 volume + lookup of the same library: the same values up to fp32 rounding
        vol = ops.corr_volume(dev(f1), dev(f2), mode=ops.CONV_F32)
        e2 = maxerr(got, ops.corr_lookup(vol, dev(coords)))
        assert e2 <= 5e-5 * rms, ("alt lookup vs volume lookup", case, kind, e2 / rms, "measured <= 2.7e-5")
    # the plain constructor is the same block as from_frames over [fmap1; fmap2]
    blk2 = AlternateCorrBlock(dev(f1), dev(f2))
    coords = _coords(B, h, w, g, "smooth")
    assert torch.equal(blk2(dev(coords)), blk(dev(coords)))


def _decode(out16):
    """S16 (B, C, H, W) -> fp32 (B, 8*ceil(C/8), H, W): (hi + lo) / 2^4."""
    d = out16.data.view(torch.float16)                                   # (B, O, 2, H, W, 8)
    v = (d[:, :, 0].float() + d[:, :, 1].float()) / 16.0                 # (B, O, H, W, 8)
    B, O_, H, W, _ = v.shape
    return v.permute(0, 1, 4, 2, 3).reshape(B, O_ * 8, H, W)


def _to88(corr):
    B, _, h, w = corr.shape
    c = corr.view(B, 4, 9, 9, h, w).transpose(2, 3).reshape(B, 4, 81, h, w)
    z = torch.zeros((B, 4, 88, h, w), dtype=corr.dtype, device=corr.device)
    z[:, :, :81] = c
    return z.view(B, 352, h, w)


@gpu
@pytest.mark.parametrize("case", [(2, 3, 256, 16, 32), (3, 2, 256, 18, 22), (2, 2, 256, 60, 128)])
def test_alt_lookup_s16(ops, case):
    from accflow_amd.networks.raft.corr import AlternateCorrBlock
    B, F, C, h, w = case
    g = gen(43)
    frames = torch.randn(F, C, h, w, generator=g)
    idx1, idx2 = [b % F for b in range(B)], [(b + 1) % F for b in range(B)]
    blk = AlternateCorrBlock.from_frames(dev(frames), idx1, idx2)
    with ops.conv_mode("f16x3"):
        for kind in ("smooth", "noise"):
            coords = dev(_coords(B, h, w, g, kind))
            ref32 = _to88(blk(coords))
            out16 = ops.S16.empty(B, ops.LOOKUP_S16_CHANNELS, h, w, coords.device)
            ops.guard_tripped()
            blk.lookup_s16(coords, out16)
            assert not ops.guard_tripped()
            got = _decode(out16)
            rms = float(ref32.pow(2).mean().sqrt())
            # the split keeps ~22 bits: |(hi + lo) / 16 - x| <= 2^-22 |x|
            assert maxerr(got, ref32) <= 2.0 ** -21 * float(ref32.abs().max()), ("S16 decode", case, kind)
            # the volume's S16 lookup, channel for channel, padding zeros included
            dp = ops.corr_volume_disp(dev(frames[idx1]), dev(frames[idx2]), mode=ops.CONV_BF16X6)
            vol16 = ops.S16.empty(B, ops.LOOKUP_S16_CHANNELS, h, w, coords.device)
            ops.corr_lookup_s16(dp, coords, vol16)
            ref = _decode(vol16)
            pad = torch.tensor([(c % 88) >= 81 for c in range(352)])
            assert torch.equal(out16.data.view(B, 44, 2, h, w, 4)[:, 10::11, :, :, :, 1:].cpu(),
                               vol16.data.view(B, 44, 2, h, w, 4)[:, 10::11, :, :, :, 1:].cpu())
            assert float(got[:, pad].abs().max()) == 0.0 and float(ref[:, pad].abs().max()) == 0.0
            assert maxerr(got, ref) <= 1e-4 * rms, ("alt S16 vs volume S16", case, kind, maxerr(got, ref) / rms)


# ------------------------------------------------------------------------------------------------
# estimators


def _raft(name="raft"):
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    m = build_flow_estimator(name)
    m.load_state_dict(make_state_dict(m), strict=True)
    return m.cuda().eval()


def _pair(seed, H, W):
    from accflow_amd.data.synthetic import make_sequence, normalize
    fr = [normalize(f) for f in make_sequence(seed, 2, H, W)]
    return fr[1], fr[0]


@gpu
def test_raft_alternate_c1_c2_vs_reference(ops, golden):
    """raft_c1 (iters 1/4/12, flow_init) and raft_c2 (480x1024) with alternate_corr: the golden tests' gates."""
    m = _raft()
    m.args.alternate_corr = True
    g = golden("raft_c1")
    i1, i2 = _pair(int(g["seed"]), int(g["H"]), int(g["W"]))
    for it in (1, 4, 12):
        out = m(dev(i1), dev(i2), iters=it).cpu()
        me, mx = O.epe(out if it == 12 else out[:, :, ::2, ::2], T(g["flow_it%d" % it]))
        assert me <= 1e-3 and mx <= 2e-4, (it, me, mx)
    out = m(dev(i1), dev(i2), iters=4, flow_init=dev(T(g["flow_init"]))).cpu()
    me, mx = O.epe(out[:, :, ::2, ::2], T(g["flow_it4_init"]))
    assert me <= 1e-3 and mx <= 1e-4, ("flow_init", me, mx)
    g = golden("raft_c2")
    i1, i2 = _pair(int(g["seed"]), int(g["H"]), int(g["W"]))
    out = m(dev(i1), dev(i2), iters=12)
    me, mx = O.epe(out[:, :, ::8, ::8].cpu(), T(g["flow_it12_s8"]))
    assert me <= 1e-3 and mx <= 5e-4, ("c2", me, mx)
    assert bool(torch.isfinite(out).all())


def _accflow():
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.AccFlow_ import AccFlow
    model = AccFlow(build_flow_estimator("acc|raft"))
    model.load_state_dict(make_state_dict(model), strict=True)
    return model.cuda().eval()


@gpu
def test_accflow_alternate_c3_pipeline_and_memory(ops, golden):
    """AccFlow(RAFT) C3 (7x480x1024) with alternate_corr against the reference (test_accflow_c3_7x480x1024_vs_reference's
    gates), through parallel.SequencePipeline, and its peak memory against the default path's in the same process."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    from accflow_amd.parallel import SequencePipeline
    g = golden("accflow_c3")
    model = _accflow()
    frames = [dev(normalize(f)) for f in make_sequence(int(g["seed"]), 7, 480, 1024)]
    model.ofe.args.alternate_corr = False
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    model(images=frames)
    torch.cuda.synchronize()
    peak_off = torch.cuda.max_memory_allocated() - base
    model.ofe.args.alternate_corr = True
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    outs = model(images=frames)
    torch.cuda.synchronize()
    peak_on = torch.cuda.max_memory_allocated() - base
    assert len(outs) == 5
    for k, o in enumerate(outs):
        me, mx = O.epe(o[:, :, ::8, ::8].cpu(), T(g["out%d" % k]))
        assert me <= 1e-3 and mx <= 2e-3, (k, me, mx)
    # the default path holds 11 pyramids of 313 MB
    assert peak_off - peak_on >= 3.0e9, ("peak allocated GB off / on", peak_off / 1e9, peak_on / 1e9)
    pipe = SequencePipeline(model)
    assert pipe.submit(frames) is None
    got = pipe.flush()
    assert len(got) == 5
    for a, b in zip(got, outs):
        me, mx = O.epe(a.cpu(), b.cpu())
        assert me <= 1e-4 and mx <= 2e-3, ("pipeline vs forward", me, mx)


@gpu
def test_alt_lookup_4k_sampled_vs_float64(ops):
    """Kernel level at 2160x3840 (H8 = 270, W8 = 480): 256 sampled query pixels against float64 from the host features."""
    from accflow_amd.networks.raft.corr import AlternateCorrBlock
    h, w, C = 270, 480, 256
    g = gen(47)
    frames = torch.randn(2, C, h, w, generator=g)
    smooth = torch.nn.functional.interpolate(6.0 * torch.randn(1, 2, 4, 6, generator=g), size=(h, w), mode="bilinear",
                                             align_corners=True)
    coords = O.coords_grid(1, h, w) + smooth
    blk = AlternateCorrBlock.from_frames(dev(frames), [0], [1])
    got = blk(dev(coords))[0].cpu()                                      # (324, h, w)
    ys = torch.randint(0, h, (256,), generator=g)
    xs = torch.randint(0, w, (256,), generator=g)
    f1 = frames[0].double()[:, ys, xs].t()                               # (S, C)
    lvl = frames[1].double()[None]
    d = torch.arange(-4, 6, dtype=torch.float64)
    worst = 0.0
    for l in range(4):
        if l:
            lvl = torch.nn.functional.avg_pool2d(lvl, 2, 2)
        Hl, Wl = lvl.shape[2:]
        cx, cy = coords[0, 0, ys, xs].double() / 2 ** l, coords[0, 1, ys, xs].double() / 2 ** l
        x0, y0 = torch.floor(cx), torch.floor(cy)
        ax, ay = cx - x0, cy - y0
        xx = (x0[:, None] + d[None]).long()                               # (S, 10) window columns
        yy = (y0[:, None] + d[None]).long()
        inside = ((yy >= 0) & (yy < Hl))[:, :, None] & ((xx >= 0) & (xx < Wl))[:, None, :]
        tg = lvl[0][:, yy.clamp(0, Hl - 1)[:, :, None], xx.clamp(0, Wl - 1)[:, None, :]]   # (C, S, 10, 10)
        win = torch.einsum("sc,csrq->srq", f1, tg) / math.sqrt(C) * inside
        for i in range(9):
            for j in range(9):
                v = (win[:, j, i] * (1 - ax) * (1 - ay) + win[:, j, i + 1] * ax * (1 - ay) + win[:, j + 1, i] * (1 - ax) * ay
                     + win[:, j + 1, i + 1] * ax * ay)
                worst = max(worst, float((got[l * 81 + i * 9 + j, ys, xs].double() - v).abs().max()))
    assert worst <= 1e-5, ("4K sampled alt lookup vs float64", worst)


@gpu
def test_accflow_alternate_4k(ops):
    """AccFlow(RAFT) on one 7x2160x3840 sequence with alternate_corr (its volume would need ~1 TB): 5 finite flows, peak
    allocated memory under a bound set from the measured figure + ~25 %."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    model = _accflow()
    model.ofe.args.alternate_corr = True
    frames = [dev(normalize(f)) for f in make_sequence(7, 7, 2160, 3840)]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    outs = model(images=frames)
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 1e9
    assert len(outs) == 5
    for o in outs:
        assert tuple(o.shape) == (1, 2, 2160, 3840) and bool(torch.isfinite(o).all())
    assert peak <= 32.0, ("peak allocated GB", peak, "measured 25.7")


# ------------------------------------------------------------------------------------------------
# the switch


def test_alternate_switch_host():
    """args.alternate_corr is read at forward time; ACCFLOW_ALTERNATE_CORR switches every estimator on (CPU: no launch)."""
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.raft import raft as R
    m = build_flow_estimator("raft")
    saved = R.ALTERNATE_CORR
    try:
        R.ALTERNATE_CORR = False
        assert m.args.alternate_corr is False and not m._alternate()
        assert not m._packs_usable({}, [(0, 1)])
        m.args.alternate_corr = True
        assert m._alternate()
        m.args.alternate_corr = False
        R.ALTERNATE_CORR = True
        assert m._alternate() and build_flow_estimator("gma")._alternate()
    finally:
        R.ALTERNATE_CORR = saved


@gpu
def test_default_unchanged_and_switch(ops, monkeypatch):
    """Flag off: the refinement builds CorrBlock (the fused lookup -> convc1 path); flipping ofe.args.alternate_corr between
    two forwards switches the path, and in that mode encode_pairs builds no correlation operand packs."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    from accflow_amd.networks.raft import raft as R
    from accflow_amd.networks.raft.corr import AlternateCorrBlock, CorrBlock
    monkeypatch.setattr(R, "ALTERNATE_CORR", False)
    seen = []
    orig = R.RAFT._lookup_and_flow

    def spy(self, ws, corr_fn, coords1):
        seen.append(type(corr_fn))
        return orig(self, ws, corr_fn, coords1)
    monkeypatch.setattr(R.RAFT, "_lookup_and_flow", spy)
    m = _raft()
    i1, i2 = _pair(5, 128, 256)
    a = m(dev(i1), dev(i2), iters=2)
    assert seen and set(seen) == {CorrBlock}
    seen.clear()
    m.args.alternate_corr = True
    b = m(dev(i1), dev(i2), iters=2)
    assert seen and set(seen) == {AlternateCorrBlock}
    assert O.epe(a.cpu(), b.cpu())[0] <= 1e-4
    seen.clear()
    m.args.alternate_corr = False
    c = m(dev(i1), dev(i2), iters=2)
    assert set(seen) == {CorrBlock} and O.epe(a.cpu(), c.cpu())[1] <= 1e-5
    # estimate_pairs (AccFlow's entry): the default builds per-frame operand packs and packed volumes, the alternate mode
    # neither - one AltPyramid of the frames instead
    built = []
    for name in ("corr_pack", "corr_volume_disp_packed", "corr_alt_pyramid"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a_, _fn=fn, _n=name, **k_: built.append(_n) or _fn(*a_, **k_))
    frames = [dev(normalize(f)) for f in make_sequence(3, 3, 128, 256)]
    pairs = [(0, 1), (1, 2), (0, 2), (2, 1)]
    seen.clear()
    ref = m.estimate_pairs(frames, pairs, iters=2)
    assert set(seen) == {CorrBlock} and "corr_pack" in built and "corr_alt_pyramid" not in built
    m.args.alternate_corr = True
    seen.clear()
    built.clear()
    feats = m.encode_pairs(frames, pairs)
    assert "corr_packs" not in feats and "fmap_event" not in feats
    out = m.estimate_pairs(frames, pairs, iters=2)
    assert set(seen) == {AlternateCorrBlock} and built == ["corr_alt_pyramid"], built
    assert O.epe(out.cpu(), ref.cpu())[0] <= 1e-4


@gpu
def test_alt_block_inside_graph_capture(ops):
    """AlternateCorrBlock built and looked up inside a captured graph (the training step captures its forward): the replay
    gives the eager result."""
    from accflow_amd.networks.raft.corr import AlternateCorrBlock
    g = gen(53)
    frames = dev(torch.randn(3, 256, 16, 32, generator=g))
    coords = dev(_coords(2, 16, 32, g, "smooth"))
    want = AlternateCorrBlock.from_frames(frames, [2, 0], [1, 2])(coords)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        AlternateCorrBlock.from_frames(frames, [2, 0], [1, 2])(coords)      # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = AlternateCorrBlock.from_frames(frames, [2, 0], [1, 2])(coords)
    got.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
