"""GMA's positional attention on the GPU (csrc/gma_pos.hip; args.position_only / args.position_and_content): the tables
kernel, every attention route in both modes, the modules, and the estimator end to end against the reference's fixture
tests/golden/gma_pos_c1.npz.  References, error model, routes, input classes and the case table are those of
tests/test_gma_pos_host.py (which pins the restatement to the reference's attention and shows the gates' teeth on the
CPU): gate = MARGIN (E32 + E_split), MARGIN = 4, an S16 output adds 2^-22 a + 2^-29 per element; every yardstick is
computed at run time from the float64 reference, none from what the kernels return.

The aggregation gates of the module cases are tests/test_gma_routes.py's chain gates, restated: E32 is the float32 CPU
evaluation of attention then fmap + gamma attn v, E_split the float64 evaluation of the designed operands - the designed
attention rounded to fp32 (S16 mode: to its stored pair) through the aggregation's arithmetic: f32 for gma_aggregate,
f16x3 on the stored pair for gma_aggregate_s16 (v * gamma row-scaled into [2^10, 2^11), fp16 hi + lo, products hh + hl +
lh), bf16x6 for the ragged per-item route of gma_aggregate_t.  qk and v are what the modules' own 1x1 convolutions give
on the device in the mode of the case, so the gate holds the attention and the aggregation, not those convolutions.

Measured on the MI355X, 2026-10-20, every case passing - largest error / gate: tables 0.50, P1 0.52, P2 0.31, P3 0.62,
P4 0.57 (gate + storage term), modules forward 0.27, forward_t 0.18; shared runs equal per-item results bit for bit;
gma_pos_c1 at 12 iterations: max EPE 9.9e-5 px (position_only) and 3.0e-4 px (position_and_content) against the 2e-3 gate.
No gate, margin or input was chosen from these figures.
"""
import pytest
import torch

import test_gma_pos_host as M

gpu = pytest.mark.gpu
pytestmark = gpu
D, MAXPOS, MARGIN = M.D, M.MAXPOS, M.MARGIN
SCALE = D ** -0.5
MODES = {"po": dict(position_only=True), "pc": dict(position_and_content=True)}


def dev(t):
    return t.cuda()


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as o
    assert torch.cuda.is_available()
    return o


def within(tag, got, ref, gate):
    """|got - ref| <= gate; prints the largest error-to-gate ratio."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), tag + ": NaN"
    gate = torch.as_tensor(gate, dtype=torch.float64).expand_as(ref)
    r = float(((got - ref).abs() / gate.clamp_min(1e-300)).max())
    print("RATIO %s %.3f" % (tag, r))
    assert r <= 1.0, "%s: error / gate = %.3f" % (tag, r)


# ------------------------------------------------------------------------------------------------
# tables

TABLE_CASES = [(1 + (k + n) % 2, h, w, mp) for k, (h, w) in enumerate(M.SHAPES) for n, mp in enumerate((MAXPOS, max(h, w)))]


@pytest.mark.parametrize("case", TABLE_CASES, ids=M.case_id)
def test_tables_vs_float64(ops, case):
    """Both tables, separately (a swapped pair fails), at M = 160 and at M = max(h, w), where the first and the last
    embedding row are read; gate MARGIN E32 (fp32 operands, fp32 FMA: E_split = 0)."""
    B, h, w, mp = case
    qk = M.make_qk("mid", B, h, w)
    Eh, Ew = M.make_emb("mid", B, h, w, mp)
    assert tuple(Eh.shape) == (2 * mp - 1, D)
    ref = M.pos_tables(qk[:, :D].double() * SCALE, Eh.double(), Ew.double(), mp)
    e32 = M.pos_tables(qk[:, :D] * M.f32(SCALE), Eh, Ew, mp)
    tab = ops.gma_pos_tables(dev(qk), dev(Eh), dev(Ew), D, SCALE)
    assert tuple(tab.shape) == (B, h + w, h * w)
    for name, got, r64, r32 in (("A", tab[:, :h], ref[0], e32[0]), ("Bw", tab[:, h:], ref[1], e32[1])):
        gate = MARGIN * float((r32.double() - r64).abs().max())
        within("tables %s %s" % (name, M.case_id(case)), got.transpose(1, 2), r64, gate)
    if h != w:
        with pytest.raises(RuntimeError):       # (the wrong table shape is refused, not read out of bounds)
            ops.gma_attention_pos_t(dev(qk), tab[:, :h + w - 1].contiguous(), D, SCALE, True)


def test_tables_refuse_a_grid_above_max_pos(ops):
    Eh, Ew = M.make_emb("mid", 1, 3, 3, 8)
    with pytest.raises(ValueError, match="9.*8"):
        ops.gma_pos_tables(torch.zeros(1, 2 * D, 9, 4, device="cuda"), dev(Eh), dev(Ew), D, SCALE)
    with pytest.raises(ValueError, match="9.*8"):
        ops.gma_pos_tables(torch.zeros(1, 2 * D, 4, 9, device="cuda"), dev(Eh), dev(Ew), D, SCALE)


# ------------------------------------------------------------------------------------------------
# attention routes


def run_attention(ops, entry, mode, qk, tab, content):
    """-> attention [b][i][j] on the device (fp32)."""
    B, _, h, w = qk.shape
    P = h * w
    with ops.conv_mode(mode):
        if entry == "i":
            return ops.gma_attention_pos(qk, tab, D, SCALE, content)[:, 0]
        if entry == "t":
            return ops.gma_attention_pos_t(qk, tab, D, SCALE, content).transpose(1, 2)
        a16 = ops.gma_attention_pos_s16(qk, tab, D, SCALE, content)
    assert a16.shape == (B, P, h, w)
    if P % 8:                                   # the tail octet: channels j >= P are stored as zeros
        halfs = a16.data.contiguous().view(torch.float16).view(B, (P + 7) // 8, 2, h, w, 8)
        assert bool((halfs[:, -1, :, :, :, P % 8:] == 0).all()), "tail octet not zero-filled"
    return a16.to_float().view(B, P, P).transpose(1, 2)


@pytest.mark.parametrize("case", M.ATT_CASES, ids=M.case_id)
def test_attention_route_vs_float64(ops, case):
    route, entry, mode, content, B, h, w, cls = case
    m = M.att_model(case)
    assert M.pos_route(entry, mode, h * w) == route and bool(torch.isfinite(m["ref"]).all())
    qk = dev(M.make_qk(cls, B, h, w))
    Eh, Ew = M.make_emb(cls, B, h, w)
    ops.guard_tripped()
    tab = ops.gma_pos_tables(qk, dev(Eh), dev(Ew), D, SCALE)
    got = run_attention(ops, entry, mode, qk, tab, content)
    within("%s %s" % (route, M.case_id(case[1:])), got, m["ref"], m["gate"])
    if cls == "zero" and content and entry != "s16":     # ... which is the content-only reference; so is the content-only op
        with ops.conv_mode(mode):
            plain = ops.gma_attention(qk, D, SCALE)[:, 0] if entry == "i" else ops.gma_attention_t(qk, D, SCALE).transpose(1, 2)
        within("%s content-only op" % route, plain, m["ref"], m["gate"])
    assert not ops.guard_tripped()


# ------------------------------------------------------------------------------------------------
# modules


def split_f16(x32):
    hi = x32.half()
    lo = (x32 - hi.float()).half()
    return hi.double(), lo.double()


def mm(wterm, aterm):
    """sum_j w[b][r][j] a[b][i][j] in float64."""
    return torch.matmul(wterm, aterm.transpose(1, 2))


def row_scaled_weights(v32, gamma):
    """w = fp32(v * gamma) * 2^k, k per row from the row maximum of |v| times |gamma| (fp32) so that it lies in [2^10, 2^11)."""
    g = torch.tensor(gamma, dtype=torch.float32)
    m = v32.abs().amax(dim=2) * g.abs()
    _, e = torch.frexp(m)
    k = torch.where((m > 0) & (m < 3.0e38), (11 - e).clamp(-100, 100), torch.zeros_like(e))
    sc = torch.pow(torch.tensor(2.0, dtype=torch.float64), k.double())[:, :, None]
    return ((v32 * g).double() * sc).float(), 1.0 / sc


def agg_design(arith, attn32, v32, gamma, a16=None):
    """fmap-less aggregation (B, R, P) float64 by the route's designed operand arithmetic (tests/test_gma_routes.py)."""
    if arith == "f32":
        return M.f32(gamma) * mm(v32.double(), attn32.double())
    if arith == "f16x3_s16":
        w, inv = row_scaled_weights(v32, gamma)
        wh, wl = split_f16(w)
        ah, al = a16
        return (mm(wh, ah) + mm(wh, al) + mm(wl, ah)) * inv / M.ASC
    assert arith == "bf16x6"
    wt, at = M.split_bf16(v32 * torch.tensor(gamma, dtype=torch.float32), 3), M.split_bf16(attn32, 3)
    return mm(wt[0], at[0] + at[1] + at[2]) + mm(wt[1], at[0] + at[1]) + mm(wt[2], at[0])


def make_modules(flags, seed):
    from accflow_amd.networks.gma.gma import gma_args
    from accflow_amd.networks.gma.modules import Aggregate, Attention
    g = M.gen(seed)
    args = gma_args(**flags)
    att = Attention(args=args, dim=128, heads=1, max_pos_size=MAXPOS, dim_head=128).cuda().eval()
    agg = Aggregate(args=args, dim=128, dim_head=128, heads=1).cuda().eval()
    with torch.no_grad():
        att.to_qk.weight.copy_(dev(torch.randn(256, 128, 1, 1, generator=g) * 0.1))
        att.pos_emb.rel_height.weight.copy_(dev(torch.randn(2 * MAXPOS - 1, 128, generator=g)))
        att.pos_emb.rel_width.weight.copy_(dev(torch.randn(2 * MAXPOS - 1, 128, generator=g)))
        agg.to_v.weight.copy_(dev(torch.randn(128, 128, 1, 1, generator=g) * 0.1))
        agg.gamma.fill_(0.6)
    return att, agg, g


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("tag", ["po", "pc"])
def test_attention_modules_into_aggregate_vs_float64(ops, tag, mode):
    """Attention.forward (row-major -> gma_aggregate) and Attention.forward_t (f16x3: the S16 matrix -> gma_aggregate_s16;
    bf16x6: fp32 j-major -> gma_aggregate_t, ragged) followed by Aggregate, against float64 fmap + gamma * attn @ v."""
    att, agg, g = make_modules(MODES[tag], 31)
    content = tag == "pc"
    B, h, w, gamma = 2, 7, 9, 0.6
    P = h * w
    inp = dev(torch.randn(B, 128, h, w, generator=g).relu())
    motion = torch.randn(B, 128, h, w, generator=g)
    ops.guard_tripped()
    with ops.conv_mode(mode):
        qk = ops.conv2d(att._packs.conv("qk", att.to_qk), inp).cpu()
        v = ops.conv2d(agg._packs.conv("v", agg.to_v), dev(motion)).cpu().view(B, 128, P)
        handle = att.forward_t(inp)
        out_t = agg(handle, dev(motion))
        out_i = agg(att(inp), dev(motion))
    assert (handle.attn16 is not None) == (mode == "f16x3") and (handle.attn_t is None) == (mode == "f16x3")
    Eh, Ew = att.pos_emb.rel_height.weight.detach().cpu(), att.pos_emb.rel_width.weight.detach().cpu()
    f1 = motion.view(B, 128, P)
    a64 = M.attention(qk, Eh, Ew, MAXPOS, SCALE, content)
    ref = f1.double() + M.f32(gamma) * mm(v.double(), a64)
    a32 = M.attention(qk, Eh, Ew, MAXPOS, SCALE, content, torch.float32)
    e32 = float(((f1 + M.f32(gamma) * torch.matmul(v, a32.transpose(1, 2))).double() - ref).abs().max())
    for name, got, design, arith in (("forward", out_i, None, "f32"),
                                     ("forward_t", out_t, "bf16x6" if content else None, "f16x3_s16" if mode == "f16x3" else "bf16x6")):
        a_design = M.attention(qk, Eh, Ew, MAXPOS, SCALE, content, design=design).float()
        pair = None
        if arith == "f16x3_s16":
            a_design, hi, lo = M.s16_value(a_design)
            pair = (hi, lo)
        esplit = float((f1.double() + agg_design(arith, a_design, v, gamma, pair) - ref).abs().max())
        within("modules %s %s %s" % (tag, mode, name), got.view(B, 128, P), ref, MARGIN * (e32 + esplit))
    assert not ops.guard_tripped()


@pytest.mark.parametrize("tag", ["po", "pc"])
def test_shared_attention_runs_with_positions(ops, tag):
    """tests/test_hip_parity.py::test_gma_shared_attention_runs' item list and tolerance on the positional attention: the
    tables and the matrix are built per distinct image1, runs of items share them."""
    att, agg, g = make_modules(MODES[tag], 151)
    for h, w in ((8, 16), (7, 9)):
        ctx = torch.randn(3, 128, h, w, generator=g).relu()
        items = [0, 0, 1, 2, 2, 2, 0]
        inp = dev(ctx[items])
        motion = dev(torch.randn(len(items), 128, h, w, generator=g))
        for mode in (ops.CONV_F16X3, ops.CONV_BF16X6):
            with ops.conv_mode(mode):
                per_item = agg(att.forward_t(inp), motion)
                runs = [[0, 0, 2], [1, 2, 3], [2, 3, 6], [0, 6, 7]]
                shared = agg(att.forward_t(dev(ctx), runs=runs), motion)
            err = float((shared - per_item).abs().max())
            print("shared runs %s %dx%d mode %d: %.2e" % (tag, h, w, mode, err))
            assert err <= 2e-5, (tag, h, w, mode, err)


@pytest.mark.parametrize("tag", ["po", "pc"])
def test_modules_refuse_what_is_not_built(ops, tag):
    att, _, _ = make_modules(MODES[tag], 5)
    with pytest.raises(NotImplementedError):
        att.forward_alt(torch.zeros(1, 128, 8, 8, device="cuda"))
    for shape in ((1, 128, 161, 2), (1, 128, 2, 161)):
        for fn in (att.forward, att.forward_t):
            with pytest.raises(ValueError, match="161.*160"):
                fn(torch.zeros(shape, device="cuda"))


# ------------------------------------------------------------------------------------------------
# end to end


def _pair(seed, H, W):
    from accflow_amd.data.synthetic import make_sequence, normalize
    fr = [normalize(f) for f in make_sequence(seed, 2, H, W)]
    return fr[1], fr[0]


def _spy(monkeypatch, ops, names, seen):
    for name in names:
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a_, _fn=fn, _n=name, **k_: seen.append(_n) or _fn(*a_, **k_))


ATT_OPS = ("gma_attention", "gma_attention_t", "gma_attention_s16", "gma_attention_alt", "gma_pos_tables", "gma_attention_pos",
           "gma_attention_pos_t", "gma_attention_pos_s16")


@pytest.mark.parametrize("f32mode", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("tag", ["po", "pc"])
def test_gma_pos_c1_golden(ops, golden, monkeypatch, tag, f32mode):
    """RAFTGMA(gma_args(...)) with make_state_dict's weights against the reference's run (gma_pos_c1.npz, every flow subsampled
    ::2) at iters 1 / 4 / 12 and with flow_init, under test_gma_c1_golden_with_alternate_attention's gates; the default mode
    (S16) and fp32 mode.  alternate_attention is set: a positional model stays on the stored matrix."""
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks.gma.gma import RAFTGMA, gma_args
    from oracle import accflow_oracle as O
    g = golden("gma_pos_c1")
    m = RAFTGMA(gma_args(**MODES[tag]))
    m.load_state_dict(make_state_dict(m), strict=True)
    m = m.cuda().eval()
    m.args.alternate_attention = True
    seen = []
    _spy(monkeypatch, ops, ATT_OPS, seen)
    i1, i2 = _pair(int(g["seed"]), int(g["H"]), int(g["W"]))
    T = torch.from_numpy
    import contextlib
    with (ops.conv_mode(ops.CONV_F32) if f32mode else contextlib.nullcontext()):
        assert f32mode or ops.s16_active()
        for it in (1, 4, 12):
            out = m(dev(i1), dev(i2), iters=it).cpu()
            me, mx = O.epe(out[:, :, ::2, ::2], T(g["%s_flow_it%d" % (tag, it)]))
            print("gma_pos_c1 %s %s it%d: EPE mean %.2e max %.2e" % (tag, "f32" if f32mode else "s16", it, me, mx))
            assert me <= 1e-3 and mx <= 2e-3, (it, me, mx)
        out = m(dev(i1), dev(i2), iters=4, flow_init=dev(T(g["flow_init"]))).cpu()
        me, mx = O.epe(out[:, :, ::2, ::2], T(g[tag + "_flow_it4_init"]))
        print("gma_pos_c1 %s flow_init: EPE mean %.2e max %.2e" % (tag, me, mx))
        assert me <= 1e-3 and mx <= 1e-3, ("flow_init", me, mx)
    assert set(seen) == {"gma_pos_tables", "gma_attention_pos" if f32mode else "gma_attention_pos_s16"}, set(seen)


def test_accflow_with_positional_gma(ops):
    from accflow_amd.data.synthetic import make_sequence, make_state_dict, normalize
    from accflow_amd.networks.AccFlow_ import AccFlow
    from accflow_amd.networks.gma.gma import RAFTGMA, gma_args
    model = AccFlow(RAFTGMA(gma_args(position_and_content=True)))
    model.load_state_dict(make_state_dict(model), strict=True)
    model = model.cuda().eval()
    frames = [dev(normalize(f)) for f in make_sequence(1003, 3, 128, 192)]
    outs = model(images=frames)
    assert len(outs) >= 1
    for o in outs:
        assert tuple(o.shape) == (1, 2, 128, 192) and bool(torch.isfinite(o).all())
