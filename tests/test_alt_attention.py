"""alternate_attention (csrc/gma_alt.hip): GMA's aggregation from the packs of q and k and the per-query softmax statistics,
without the P x P attention matrix - ops.gma_attention_alt / ops.gma_aggregate_alt, Attention.forward_alt, the
`args.alternate_attention` / ACCFLOW_ALTERNATE_ATTENTION switch of RAFTGMA.

Error model: tests/test_gma_routes.py's, with its float64 references and its emulation of the split arithmetic (imported,
not restated).  Per case, at run time, max |got - ref64| <= MARGIN (E32 + E_split), MARGIN = 4:
    ref64    fmap + gamma * softmax_j(scale q_i . k_j) @ v in float64;
    E32      the error of the same formula in torch float32 on the CPU;
    E_split  the error of a float64 evaluation of the kernel's designed operand arithmetic (its header comment): q 2^4 and
             fp32(k scale 2^4) split as fp16 hi + lo with the products hi.hi + lo.hi + hi.lo (A4's), the softmax of those logits
             rounded to fp32, times 2^4 and split as fp16 hi + lo (the pair route G7 reads from memory, here made in registers),
             v * gamma row-scaled and split as G7's, products hi.hi + hi.lo + lo.hi;
    the pre-split output adds the storage term 2^-22 |a| + 2^-29 outside the margin.
One-hot attention: test_gma_routes' permutation gate, 4 eps (|fmap| + |gamma v|) + E_split per element.
The C5 memory bound 4 P^2 / 8 is derived (packs 14.7 MB, partial statistics 13 MB, v pack, row scales and the partial sums of
four key splits 73.7 MB), not measured.

Measured on the MI355X, 2026-10-18, default mode, every case passing - largest error / gate:
    aggregate vs float64 0.23 (fp32 output), 0.26 (S16 output; 0.93 at gamma = 0, where the gate is the storage term alone)
    shared runs 0.21   one-hot 0.42   64 sampled queries at 180 x 320 0.42   alternate vs stored route 0.035 (of the two gates' sum)
    C5 op level: alternate peak 88.7 MB (handle 14.9 MB), stored route 971 MB; C5 sequence peak 20.10 GB off, 15.05 GB on
    gma_c1 max EPE 4.4e-4 (it 12), AccFlow(GMA) 192 x 320 max 1.6e-4, C5 max 1.09e-3 - the figures of the matrix route
No gate, margin or input was chosen from these figures.
"""
import argparse
import functools
import os

import pytest
import torch

import test_gma_routes as R

gpu = pytest.mark.gpu
D = 128
SCALE = D ** -0.5
SHAPES = ((7, 9), (9, 14), (8, 16), (11, 13), (18, 22), (24, 40))   # P = 63, 126, 128, 143, 396, 960
CLASSES = ("diffuse", "mid", "peaked", "huge")


def dev(t):
    return t.cuda()


# ------------------------------------------------------------------------------------------------
# the model of a call: reference, yardsticks, gate (CPU)


def design_rows(qk, sel=None):
    """The designed probabilities of the queries `sel` (all when None), [i][j] float64: A4's logits, exact sums."""
    q, k = qk[0, :D].reshape(D, -1), qk[0, D:].reshape(D, -1)
    qh, ql = R.split_f16(q * R.ASC)
    kh, kl = R.split_f16(k * torch.tensor(R.f32(SCALE) * R.ASC, dtype=torch.float32))
    if sel is not None:
        qh, ql = qh[:, sel], ql[:, sel]
    return torch.softmax((qh.t() @ kh + ql.t() @ kh + qh.t() @ kl) / (R.ASC * R.ASC), dim=1)


def rows64(qk, sel=None):
    q, k = qk[0, :D].reshape(D, -1).double(), qk[0, D:].reshape(D, -1).double()
    if sel is not None:
        q = q[:, sel]
    return torch.softmax(q.t() @ k * SCALE, dim=1)


def rows32(qk, sel=None):
    q, k = qk[0, :D].reshape(D, -1), qk[0, D:].reshape(D, -1)
    if sel is not None:
        q = q[:, sel]
    return torch.softmax(torch.matmul(q.t(), k) * R.f32(SCALE), dim=1)


def alt_model(qk, v, fmap, gamma, sel=None, perm=None):
    """qk (1, 2 D, h, w); v, fmap (n, D, P): the n items share the attention.  -> ref (n, D, S) float64 over the queries `sel`,
    gate (same shape), E32, E_split and the teeth ratios of the weakened emulations."""
    n, _, P = v.shape
    v1, f1 = v.reshape(1, n * D, P), fmap.reshape(1, n * D, P)
    fs = f1 if sel is None else f1[:, :, sel]
    g32 = float(R.f32(gamma))
    ref = fs.double() + g32 * R.mm(v1.double(), rows64(qk, sel)[None])
    e32 = float(((fs + R.f32(gamma) * torch.matmul(v1, rows32(qk, sel).t()[None])).double() - ref).abs().max())
    a32, hi, lo = R.s16_value(design_rows(qk, sel).float()[None])
    emu = {k_: fs.double() + x for k_, x in R.agg_emulations("f16x3_s16", a32, v1, gamma, (hi, lo)).items()}
    esplit = float((emu["design"] - ref).abs().max())
    if perm is not None:          # (the float64 softmax keeps weights of e^-110 beside the 1: the reference is the permutation itself)
        gv = g32 * v1.double()[:, :, perm]
        assert float((ref - (fs.double() + gv)).abs().max()) < 1e-40
        ref = fs.double() + gv
        esplit = float((emu["design"] - ref).abs().max())
        gate = R.MARGIN * R.EPS * (fs.double().abs() + gv.abs()) + esplit
    else:
        gate = torch.full_like(ref, R.MARGIN * (e32 + esplit))
    weak = {k_: float(((x - ref).abs() / gate.clamp_min(1e-300)).max()) for k_, x in emu.items() if k_ != "design"}
    S = ref.shape[2]
    return {"ref": ref.view(n, D, S), "gate": gate.view(n, D, S), "e32": e32, "esplit": esplit, "weak": weak}


def case_inputs(case):
    h, w, n, cls, gamma, sliced = case
    P = h * w
    qk = R.make_qk(cls, 1, D, h, w)
    s = R._seed("alt", h, w, n, cls)
    v = R.make_v(n, D, P, s)
    fmap = torch.randn(n, D, P, generator=R.gen(s + 1)) * (2.0 ** -6 if cls == "diffuse" else 1.0)
    return qk, v, fmap


@functools.lru_cache(maxsize=None)
def case_model(case):
    qk, v, fmap = case_inputs(case)
    return alt_model(qk, v, fmap, case[4])


CASES = []     # (h, w, n, cls, gamma, sliced)
_i = 0
for _hw in SHAPES:
    for _n in (1, 2, 3):
        _ok = [c for c in CLASSES if c != "diffuse" or _hw[0] * _hw[1] > 128]
        CASES.append((_hw[0], _hw[1], _n, _ok[_i % len(_ok)], R.GAMMAS[_i % 2], _i % 3 == 1))
        _i += 1
for _c in CLASSES:                                         # every class at the ragged two-tile shape and at 960 pixels (8 key splits)
    for _hw in ((11, 13), (24, 40)):
        CASES.append((_hw[0], _hw[1], 2, _c, 0.37, False))
CASES += [(7, 9, 2, "mid", 0.0, False), (11, 13, 3, "peaked", 0.0, True), (18, 22, 1, "mid", -0.5, True),
          (8, 16, 3, "peaked", -0.5, False)]
CASES = list(dict.fromkeys(CASES))


def case_id(c):
    return "%dx%d-n%d-%s-g%s%s" % (c[0], c[1], c[2], c[3], c[4], "-sliced" if c[5] else "")


def test_cases_cover_what_the_issue_lists():
    assert {(c[0], c[1]) for c in CASES} == set(SHAPES) and {c[2] for c in CASES} == {1, 2, 3}
    assert {c[3] for c in CASES} == set(CLASSES) and {c[4] for c in CASES} == set(R.GAMMAS) and {c[5] for c in CASES} == {True, False}
    for c in CASES:
        assert c[3] != "diffuse" or c[0] * c[1] > 128
    huge = R.make_qk("huge", 1, D, 11, 13)
    assert float(R.logits64(huge, D, SCALE).abs().max()) > 200


TEETH = [c for c in CASES if c[3] in ("mid", "peaked") and c[4] != 0.0]


@pytest.mark.parametrize("case", TEETH, ids=case_id)
def test_gate_has_teeth(case):
    """(CPU) The designed arithmetic without the lo term of p - or of v - lands >= 8x over the gate."""
    m = case_model(case)
    assert set(m["weak"]) == {"no attention lo", "no weight lo"}
    for name, r in m["weak"].items():
        assert r >= R.TEETH, (name, m["weak"], m["e32"], m["esplit"])


# ------------------------------------------------------------------------------------------------
# GPU: the ops


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as o
    assert torch.cuda.is_available()
    assert o.s16_active()
    return o


def run_alt(ops, handle, g, v, fmap, gamma, sliced, h, w):
    """ops.gma_aggregate_alt with out only, out16 only and both (R.run_aggregation_s16's checks): -> (fp32, S16 as float)."""
    n = v.shape[0]
    gm = dev(torch.tensor([gamma]))
    v, fmap = dev(v).view(n, D, h, w), dev(fmap).view(n, D, h, w)
    C3, c0 = (3 * D, D) if sliced else (D, 0)
    big = torch.full((n, C3, h, w), R.SENT, device="cuda")
    fbuf = torch.full((n, C3, h, w), R.SENT, device="cuda")
    fbuf[:, :D] = fmap
    O16 = (C3 + 7) // 8
    outs = []
    for want32, want16 in ((True, False), (False, True), (True, True)):
        big.fill_(R.SENT)
        s16 = ops.S16(torch.full((n, O16, 2, h, w, 4), R.SENT16, dtype=torch.int32, device="cuda"), C3)
        o16 = s16.channels(c0, c0 + D)
        ops.gma_aggregate_alt(handle, g, v, fbuf[0].data_ptr(), fbuf.stride(0), gm,
                              big[0, c0:].data_ptr() if want32 else None, big.stride(0) if want32 else 0,
                              o16.ptr() if want16 else None, s16.bs if want16 else 0, n, D, h, w)
        if want32:
            outs.append(big[:, c0:c0 + D].clone())
            assert bool((big[:, :c0] == R.SENT).all()) and bool((big[:, c0 + D:] == R.SENT).all()), "wrote outside the out slice"
        else:
            assert bool((big == R.SENT).all())
        if want16:
            outs.append(o16.to_float())
            keep = torch.ones(O16, dtype=torch.bool, device="cuda")
            keep[c0 // 8:(c0 + D) // 8] = False
            assert bool((s16.data[:, keep] == R.SENT16).all()), "wrote outside the out16 slice"
        else:
            assert bool((s16.data == R.SENT16).all())
        if want32 and want16:
            assert torch.equal(o16.data, ops.to_s16(outs[-2].contiguous()).data)
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
    assert bool((fbuf[:, :D] == fmap).all())
    return outs[0], outs[1]


@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_aggregate_alt_vs_float64(ops, case):
    h, w, n, cls, gamma, sliced = case
    m = case_model(case)
    qk, v, fmap = case_inputs(case)
    ops.guard_tripped()
    handle = ops.gma_attention_alt(dev(qk), D, SCALE)
    assert handle.nbytes == handle.packs.numel() + 8 * h * w and handle.packs.numel() == 2 * 512 * (-(-h * w // 128) * 128)
    got, got16 = run_alt(ops, handle, 0, v, fmap, gamma, sliced, h, w)
    ref, gate = m["ref"].view(n, D, h, w), m["gate"].view(n, D, h, w)
    R.within("ALT " + case_id(case), got, ref, gate)
    R.within("ALT " + case_id(case) + " out16", got16, ref, gate + R.S16_REL * ref.abs() + R.S16_ABS)
    if gamma == 0.0:
        assert torch.equal(got.cpu(), fmap.view(n, D, h, w))
    assert not ops.guard_tripped()


@gpu
@pytest.mark.parametrize("hw", [(8, 16), (7, 9), (11, 13)])
def test_aggregate_alt_shared_runs(ops, hw):
    """The run list of test_gma_shared_attention_runs - a run of 2, a single, a run of 3, a non-adjacent repeat - through
    Aggregate._aggregate16 on one handle of three attentions; every run against float64."""
    from accflow_amd.networks.gma.modules import Aggregate, TransposedAttention
    h, w = hw
    P = h * w
    runs = [[0, 0, 2], [1, 2, 3], [2, 3, 6], [0, 6, 7]]
    qk = torch.cat([R.make_qk(c, 1, D, h, w) for c in ("mid", "peaked", "huge")])
    v = R.make_v(7, D, P, R._seed("runs", h, w))
    fmap = torch.randn(7, D, P, generator=R.gen(R._seed("runs", h, w) + 1))
    args = argparse.Namespace(position_only=False, position_and_content=False, num_heads=1)
    agg = Aggregate(args=args, dim=D, dim_head=D, heads=1).cuda().eval()
    with torch.no_grad():
        agg.gamma.fill_(0.37)
    handle = ops.gma_attention_alt(dev(qk), D, SCALE)
    assert len(handle) == 3
    out = torch.full((7, D, h, w), R.SENT, device="cuda")
    fm = dev(fmap).view(7, D, h, w)
    agg._aggregate16(TransposedAttention(None, runs, alt=handle), dev(v).view(7, D, h, w), fm, fm.stride(0), out, None)
    for g, b0, b1 in runs:
        m = alt_model(qk[g:g + 1], v[b0:b1], fmap[b0:b1], 0.37)
        R.within("ALT runs %dx%d [%d, %d)" % (h, w, b0, b1), out[b0:b1], m["ref"].view(b1 - b0, D, h, w), m["gate"].view(b1 - b0, D, h, w))


def onehot_qk(h, w):
    """q = c k[perm] with unit keys: logit (i, perm_i) = 250, every other one at least 100 below: each row a permutation."""
    P = h * w
    g = R.gen(R._seed("onehot", h, w))
    k = torch.randn(D, P, generator=g)
    k = k / k.norm(dim=0, keepdim=True)
    perm = torch.randperm(P, generator=g)
    q = k[:, perm] * (250.0 / SCALE)
    return torch.cat([q, k]).view(1, 2 * D, h, w).contiguous(), perm


def test_onehot_inputs_are_a_permutation():
    for h, w in ((7, 9), (11, 13), (18, 22)):
        qk, perm = onehot_qk(h, w)
        a = design_rows(qk).float()
        want = torch.zeros(h * w, h * w)
        want[torch.arange(h * w), perm] = 1.0
        assert torch.equal(a, want) and torch.equal(rows64(qk).float(), want) and not torch.equal(perm, torch.arange(h * w))
        lg = R.logits64(qk, D, SCALE)[0]
        assert float((lg.max(dim=1).values - lg.topk(2, dim=1).values[:, 1]).min()) > 110   # exp(-110) is 0 in float32
        assert float(qk.abs().max()) * R.ASC < 65504


@gpu
@pytest.mark.parametrize("hw", [(7, 9), (11, 13), (18, 22)])
@pytest.mark.parametrize("n", [1, 3])
def test_aggregate_alt_onehot(ops, hw, n):
    h, w = hw
    P = h * w
    qk, perm = onehot_qk(h, w)
    s = R._seed("onehot v", h, w, n)
    v, fmap = R.make_v(n, D, P, s), torch.randn(n, D, P, generator=R.gen(s + 1))
    m = alt_model(qk, v, fmap, -0.5, perm=perm)
    ops.guard_tripped()
    got, got16 = run_alt(ops, ops.gma_attention_alt(dev(qk), D, SCALE), 0, v, fmap, -0.5, False, h, w)
    R.within("ALT onehot %dx%d n%d" % (h, w, n), got, m["ref"].view(n, D, h, w), m["gate"].view(n, D, h, w))
    assert not ops.guard_tripped()


@gpu
@pytest.mark.parametrize("case", [(7, 9, 2, "mid"), (11, 13, 3, "peaked"), (24, 40, 2, "diffuse"), (18, 22, 1, "huge")],
                         ids=lambda c: "%dx%d-n%d-%s" % c)
def test_alt_equals_stored_route_within_both_gates(ops, case):
    """A4 -> G7 on the same inputs: both routes have the designed arithmetic of alt_model, so the difference is at most the
    sum of their (equal) gates; two calls of the alternate op give the same bits."""
    h, w, n, cls = case
    qk, v, fmap = case_inputs((h, w, n, cls, 0.37, False))
    m = alt_model(qk, v, fmap, 0.37)
    gm = dev(torch.tensor([0.37]))
    dv, df = dev(v).view(n, D, h, w), dev(fmap).view(n, D, h, w)
    a16 = ops.gma_attention_s16(dev(qk), D, SCALE)
    stored = torch.empty(n, D, h, w, device="cuda")
    ops.gma_aggregate_s16(a16.ptr(), dv, df.data_ptr(), df.stride(0), gm, stored.data_ptr(), stored.stride(0), None, 0, n, D, h, w)
    outs = []
    for _ in range(2):
        handle = ops.gma_attention_alt(dev(qk), D, SCALE)
        o = torch.empty(n, D, h, w, device="cuda")
        ops.gma_aggregate_alt(handle, 0, dv, df.data_ptr(), df.stride(0), gm, o.data_ptr(), o.stride(0), None, 0, n, D, h, w)
        outs.append(o)
    assert torch.equal(outs[0], outs[1])
    R.within("ALT vs stored %dx%d n%d %s" % case, outs[0], stored.cpu(), 2.0 * m["gate"].view(n, D, h, w))


@gpu
def test_alt_refuses_other_head_sizes(ops):
    qk = dev(torch.randn(1, 64, 4, 4))
    with pytest.raises(RuntimeError):
        ops.gma_attention_alt(qk, 32, 32 ** -0.5)
    handle = ops.gma_attention_alt(dev(torch.randn(1, 256, 4, 4)), D, SCALE)
    v = dev(torch.randn(1, 32, 4, 4))
    with pytest.raises(RuntimeError):
        ops.gma_aggregate_alt(handle, 0, v, v.data_ptr(), v.stride(0), dev(torch.ones(1)), v.data_ptr(), v.stride(0), None, 0, 1, 32, 4, 4)


@gpu
def test_memory_at_the_c5_working_size(ops):
    """90 x 160, n = 2, at op level: the handle plus the workspaces of both alternate ops peak below 4 P^2 / 8 = 104 MB
    (derived: module docstring); the stored route's peak is at least the matrix, 829 MB."""
    h, w, n = 90, 160, 2
    P = h * w
    g = R.gen(77)
    qk = dev(torch.randn(1, 2 * D, h, w, generator=g))
    v, fm = dev(torch.randn(n, D, h, w, generator=g)), dev(torch.randn(n, D, h, w, generator=g))
    gm = dev(torch.tensor([0.37]))
    out = torch.empty_like(fm)
    ops.guard_tripped()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    handle = ops.gma_attention_alt(qk, D, SCALE)
    ops.gma_aggregate_alt(handle, 0, v, fm.data_ptr(), fm.stride(0), gm, out.data_ptr(), out.stride(0), None, 0, n, D, h, w)
    torch.cuda.synchronize()
    peak_alt = torch.cuda.max_memory_allocated() - base
    print("C5 op-level peak: alternate %.1f MB, handle %.1f MB" % (peak_alt / 1e6, handle.nbytes / 1e6))
    assert handle.nbytes <= 1032 * (P + 127) and peak_alt < 4 * P * P / 8, (peak_alt, handle.nbytes)
    assert bool(torch.isfinite(out).all()) and not ops.guard_tripped()
    del handle
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a16 = ops.gma_attention_s16(qk, D, SCALE)
    ops.gma_aggregate_s16(a16.ptr(), v, fm.data_ptr(), fm.stride(0), gm, out.data_ptr(), out.stride(0), None, 0, n, D, h, w)
    torch.cuda.synchronize()
    peak_stored = torch.cuda.max_memory_allocated() - base
    print("C5 op-level peak: stored %.1f MB" % (peak_stored / 1e6))
    assert peak_stored >= 4 * P * P


# ------------------------------------------------------------------------------------------------
# GPU: through the models


def _models(name):
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    m = build_flow_estimator(name)
    sd = make_state_dict(m)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval(), sd


def _accflow(name):
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.AccFlow_ import AccFlow
    model = AccFlow(build_flow_estimator(name))
    sd = make_state_dict(model)
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval(), sd


def _pair(seed, H, W):
    from accflow_amd.data.synthetic import make_sequence, normalize
    fr = [normalize(f) for f in make_sequence(seed, 2, H, W)]
    return fr[1], fr[0]


def _spy(monkeypatch, ops, names, seen):
    for name in names:
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a_, _fn=fn, _n=name, **k_: seen.append(_n) or _fn(*a_, **k_))


MATRIX_OPS = ("gma_attention", "gma_attention_t", "gma_attention_s16", "gma_aggregate", "gma_aggregate_t", "gma_aggregate_s16")
ALT_OPS = ("gma_attention_alt", "gma_aggregate_alt")


@gpu
def test_gma_c1_golden_with_alternate_attention(ops, golden, monkeypatch):
    """test_estimator_c1_vs_golden_and_oracle[gma]'s gates (iters 1 / 4 / 12, flow_init) with args.alternate_attention."""
    from oracle import accflow_oracle as O
    g = golden("gma_c1")
    m, _ = _models("gma")
    m.args.alternate_attention = True
    seen = []
    _spy(monkeypatch, ops, MATRIX_OPS + ALT_OPS, seen)
    i1, i2 = _pair(int(g["seed"]), int(g["H"]), int(g["W"]))
    T = torch.from_numpy
    for it in (1, 4, 12):
        out = m(dev(i1), dev(i2), iters=it).cpu()
        me, mx = O.epe(out if it == 12 else out[:, :, ::2, ::2], T(g["flow_it%d" % it]))
        print("gma_c1 alt it%d: EPE mean %.2e max %.2e" % (it, me, mx))
        assert me <= 1e-3 and mx <= 2e-3, (it, me, mx)
    out = m(dev(i1), dev(i2), iters=4, flow_init=dev(T(g["flow_init"]))).cpu()
    me, mx = O.epe(out[:, :, ::2, ::2], T(g["flow_it4_init"]))
    assert me <= 1e-3 and mx <= 1e-3, ("flow_init", me, mx)
    assert set(seen) == set(ALT_OPS), set(seen)


@gpu
def test_gma_accflow_mid_size_vs_oracle_with_alternate_attention(ops):
    """test_gma_accflow_mid_size_vs_oracle's run and gates (192 x 320, 3 frames, the CPU oracle) with the switch on."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    from oracle import accflow_oracle as O
    model, sd = _accflow("acc|gma")
    model.ofe.args.alternate_attention = True
    model.ofe_iters = 6
    frames = [normalize(f) for f in make_sequence(1003, 3, 192, 320)]
    out = model(images=[dev(f) for f in frames])[-1].cpu()
    ref = O.accflow_forward(sd, frames, iters=6, gma=True)[-1]
    me, mx = O.epe(out, ref)
    print("AccFlow(GMA) 192x320 alt: EPE mean %.2e max %.2e" % (me, mx))
    assert me <= 1e-3 and mx <= 2e-2, (me, mx)


@gpu
def test_accflow_gma_c5_with_alternate_attention_and_memory(ops, golden):
    """test_accflow_gma_c5_7x720x1280_vs_reference's gates with the switch on, through forward and
    SequencePipeline; the peak allocation is lower than with the switch off by at least one matrix (4 P^2 bytes: the
    sequence holds six)."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    from accflow_amd.parallel import SequencePipeline
    from oracle import accflow_oracle as O
    g = golden("accflow_gma_c5")
    model, _ = _accflow("acc|gma")
    frames = [dev(normalize(f)) for f in make_sequence(int(g["seed"]), 7, 720, 1280)]
    P = 90 * 160
    peaks = {}
    for on in (False, True):
        model.ofe.args.alternate_attention = on
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        outs = model(images=frames)
        torch.cuda.synchronize()
        peaks[on] = torch.cuda.max_memory_allocated() - base
        if not on:
            del outs
    assert len(outs) == 5
    for k, o in enumerate(outs):
        me, mx = O.epe(o[:, :, ::8, ::8].cpu(), torch.from_numpy(g["out%d" % k]))
        print("C5 alt out%d: EPE mean %.2e max %.2e" % (k, me, mx))
        assert me <= 1e-3 and mx <= 5e-3, (k, me, mx)
    print("C5 peak allocated GB: off %.2f on %.2f" % (peaks[False] / 1e9, peaks[True] / 1e9))
    assert peaks[False] - peaks[True] >= 4 * P * P, peaks
    pipe = SequencePipeline(model)
    assert pipe.submit(frames) is None
    got = pipe.flush()
    assert len(got) == 5
    for a, b in zip(got, outs):
        me, mx = O.epe(a.cpu(), b.cpu())
        assert me <= 1e-4 and mx <= 2e-3, ("pipeline vs forward", me, mx)


@gpu
def test_large_frame_1440x2560(ops):
    """P = 57 600: past the stored route's 32-bit limit (4 P^2 = 13.3 GB per matrix).  One aggregate call at op level, 64
    sampled queries against float64 under test_aggregate_alt_vs_float64's gate; then a 3-frame AccFlow(GMA) with both
    alternates on gives finite flows."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    h, w, n = 180, 320, 2
    P = h * w
    g = R.gen(91)
    qk = torch.randn(1, 2 * D, P, generator=g) * 1.5
    qk = qk.view(1, 2 * D, h, w)
    v, fmap = R.make_v(n, D, P, 92), torch.randn(n, D, P, generator=g)
    sel = torch.randperm(P, generator=g)[:64]
    sel[0], sel[1] = P - 1, 0
    m = alt_model(qk, v, fmap, 0.37, sel=sel)
    ops.guard_tripped()
    handle = ops.gma_attention_alt(dev(qk), D, SCALE)
    out = torch.empty(n, D, h, w, device="cuda")
    df = dev(fmap).view(n, D, h, w)
    ops.gma_aggregate_alt(handle, 0, dev(v).view(n, D, h, w), df.data_ptr(), df.stride(0), dev(torch.tensor([0.37])),
                          out.data_ptr(), out.stride(0), None, 0, n, D, h, w)
    assert bool(torch.isfinite(out).all()) and not ops.guard_tripped()
    R.within("ALT 180x320 sampled", out.view(n, D, P)[:, :, dev(sel)], m["ref"], m["gate"])
    del handle, out
    model, _ = _accflow("acc|gma")
    model.ofe.args.alternate_attention = True
    model.ofe.args.alternate_corr = True
    frames = [dev(normalize(f)) for f in make_sequence(11, 3, 1440, 2560)]
    outs = model(images=frames)
    assert len(outs) >= 1
    for o in outs:
        assert tuple(o.shape) == (1, 2, 1440, 2560) and bool(torch.isfinite(o).all())


# ------------------------------------------------------------------------------------------------
# the switch


def test_switch_host():
    """args.alternate_attention is set to False when absent and read at forward time; ACCFLOW_ALTERNATE_ATTENTION switches
    every GMA estimator on (CPU: no launch) - as alternate_corr's switch is read."""
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.gma import gma as G
    assert G.ALTERNATE_ATTENTION == (os.environ.get("ACCFLOW_ALTERNATE_ATTENTION", "0") == "1")
    m = build_flow_estimator("gma")
    saved = G.ALTERNATE_ATTENTION
    try:
        G.ALTERNATE_ATTENTION = False
        assert m.args.alternate_attention is False and not m._alternate_attention()
        m.args.alternate_attention = True
        assert m._alternate_attention()
        m.args.alternate_attention = False
        G.ALTERNATE_ATTENTION = True
        assert m._alternate_attention() and build_flow_estimator("gma")._alternate_attention()
    finally:
        G.ALTERNATE_ATTENTION = saved


@gpu
def test_default_unchanged_and_switch(ops, monkeypatch):
    """Off: no gma_*_alt call, and the result equals, bit for bit, a run made before the flag was touched.  On: only the
    alternate ops run - no builder of a P x P matrix is called.  fp32 mode and ACCFLOW_S16=0 keep the matrix."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    from accflow_amd.networks.gma import gma as G
    monkeypatch.setattr(G, "ALTERNATE_ATTENTION", False)
    m, _ = _models("gma")
    frames = [dev(normalize(f)) for f in make_sequence(3, 3, 128, 256)]
    pairs = [(0, 1), (0, 2), (1, 2), (0, 1)]
    before = m.estimate_pairs(frames, pairs, iters=3).clone()
    seen = []
    _spy(monkeypatch, ops, MATRIX_OPS + ALT_OPS, seen)
    m.args.alternate_attention = True
    on = m.estimate_pairs(frames, pairs, iters=3).clone()
    assert seen and set(seen) == set(ALT_OPS), set(seen)
    seen.clear()
    m.args.alternate_attention = False
    off = m.estimate_pairs(frames, pairs, iters=3)
    assert seen and not set(seen) & set(ALT_OPS)
    assert torch.equal(off, before)
    from oracle import accflow_oracle as O
    assert O.epe(on.cpu(), before.cpu())[0] <= 1e-4
    seen.clear()
    monkeypatch.setattr(G, "ALTERNATE_ATTENTION", True)
    m.estimate_pairs(frames, pairs, iters=1)
    assert set(seen) == set(ALT_OPS)
    for ctx in (ops.conv_mode(ops.CONV_F32), ops.conv_mode(ops.CONV_BF16X6)):
        seen.clear()
        with ctx:
            m.estimate_pairs(frames, pairs, iters=1)
        assert seen and not set(seen) & set(ALT_OPS)
    seen.clear()
    monkeypatch.setattr(ops, "USE_S16", False)
    m.estimate_pairs(frames, pairs, iters=1)
    assert seen and not set(seen) & set(ALT_OPS)


@gpu
def test_aggregate_alt_inside_graph_capture(ops):
    """One aggregate call captured in a HIP graph and replayed gives the bits of the eager call."""
    h, w, n = 11, 13, 2
    qk, v, fmap = case_inputs((h, w, n, "mid", 0.37, False))
    handle = ops.gma_attention_alt(dev(qk), D, SCALE)
    gm = dev(torch.tensor([0.37]))
    dv, df = dev(v).view(n, D, h, w), dev(fmap).view(n, D, h, w)
    want = torch.empty(n, D, h, w, device="cuda")
    ops.gma_aggregate_alt(handle, 0, dv, df.data_ptr(), df.stride(0), gm, want.data_ptr(), want.stride(0), None, 0, n, D, h, w)
    got = torch.zeros(n, D, h, w, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):      # (warm-up outside the capture)
        ops.gma_aggregate_alt(handle, 0, dv, df.data_ptr(), df.stride(0), gm, got.data_ptr(), got.stride(0), None, 0, n, D, h, w)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gma_aggregate_alt(handle, 0, dv, df.data_ptr(), df.stride(0), gm, got.data_ptr(), got.stride(0), None, 0, n, D, h, w)
    got.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
