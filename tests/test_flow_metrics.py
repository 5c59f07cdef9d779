"""ops.fb_occlusion / ops.flow_metrics (csrc/flow_metrics.hip) and accflow_amd.metrics on the GPU, against float64
references written HERE, against the reference's own output (tests/golden/harness.npz) and against the torch route they
replace (eval_cvo.calc_occ_mask + cal_epe, train_acc.sequence_loss_metrics).

Inputs.  A smooth flow pair: f = a 3 x 4 grid of 6 * randn, bilinearly enlarged; b = -warp(f, -f) + 0.3 * an enlarged 5 x 7
grid of randn, i.e. roughly the inverse of f plus a disturbance of the size of the threshold.  Measured on the CPU for the
five cases below: between 15 % and 84 % of either mask is occluded (random-noise flows give masks that are 99 % ones and test
nothing).

Masks.  d = |diff| - thr is evaluated in float64 from the same float32 inputs (the sample position x + u is formed in float32
and clamped as the kernel does it).  A float32 evaluation of the formula differs from float64 by at most 1.4e-4 px on these
cases (the largest at W = 301, where x + u has the coarsest ulp), so pixels with |d| < MARGIN = 4e-4 are left out and
everywhere else the kernel's bit must equal d > 0.  What the margin may hide is capped BEFORE the kernel is looked at: at
most 0.5 % of a mask may be left out (at a 2e-4 margin it is <= 0.051 % with these inputs).

Sums.  Columns 0, 1 and 6 against float64 sums of the same float32 inputs: relative error <= (4 + log2(pixels per stage-1
partial)) * 2^-23 of the sum of absolute terms - two roundings for the element plus the fp32 tree; stage 2 is in double.
Columns 2 and 7 exact.  The three counts within +- the number of pixels whose float64 EPE lies within 1e-5 of the threshold,
and that number is at most 0.1 % of the pixels.

Measured on an MI355X: see DESIGN.md 4.7.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
T = torch.from_numpy
MARGIN = 4e-4
MAX_EXCLUDED = 5e-3
ALPHA, BETA = 0.01, 0.5
RUN = 4096                      # pixels per stage-1 partial (test_stage1_run_length pins it through the workspace query)
CASES = ((2, 37, 53, 21), (3, 40, 64, 22), (1, 64, 200, 23), (2, 9, 301, 24), (1, 130, 70, 25))
IDS = ["%dx%dx%d" % c[:3] for c in CASES]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def grid32(H, W):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return xs, ys


def clamp_like_make_taps(s):
    """fminf(fmaxf(s, -1e6), 1e6): fmaxf drops a NaN operand, so NaN becomes -1e6."""
    return torch.nan_to_num(s, nan=-1.0e6, posinf=1.0e6, neginf=-1.0e6).clamp(-1.0e6, 1.0e6)


def sample_zeros(plane, flow, dtype):
    """bilinear-zeros sample of plane (B,C,H,W) at p + flow, in `dtype`, by make_taps' rules: the position is formed in float32
    and clamped; a corner outside the plane has weight 0 and reads element 0 (0 * plane[0]: 0 unless that element is not
    finite)."""
    B, C, H, W = plane.shape
    xs, ys = grid32(H, W)
    sx = clamp_like_make_taps(xs + flow[:, 0]).to(dtype)
    sy = clamp_like_make_taps(ys + flow[:, 1]).to(dtype)
    x0, y0 = sx.floor(), sy.floor()
    ax, ay = sx - x0, sy - y0
    x0, y0 = x0.long(), y0.long()
    flat = plane.to(dtype).reshape(B, C, H * W)
    acc = torch.zeros(B, C, H, W, dtype=dtype)
    for dy, dx, w in ((0, 0, (1 - ax) * (1 - ay)), (0, 1, ax * (1 - ay)), (1, 0, (1 - ax) * ay), (1, 1, ax * ay)):
        xx, yy = x0 + dx, y0 + dy
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        off = torch.where(ok, yy * W + xx, torch.zeros_like(xx))
        wt = torch.where(ok, w, torch.zeros_like(w))
        v = flat.gather(2, off.reshape(B, 1, -1).expand(B, C, -1)).reshape(B, C, H, W)
        acc = acc + v * wt[:, None]
    return acc


def warp(img, flow):
    return sample_zeros(img, flow, torch.float32)


def enlarge(t, H, W):
    return F.interpolate(t, size=(H, W), mode="bilinear", align_corners=True)


@functools.lru_cache(maxsize=None)
def smooth_pair(B, H, W, seed):
    g = gen(seed)
    f = enlarge(6 * torch.randn(B, 2, 3, 4, generator=g), H, W)
    b = -warp(f, -f) + 0.3 * enlarge(torch.randn(B, 2, 5, 7, generator=g), H, W)
    return b.contiguous(), f.contiguous()


def margin64(own, other, alpha=ALPHA, beta=BETA):
    """d = |own + other(p + own)| - (alpha (|own| + |other|) + beta) in float64, (B,H,W); alpha and beta as the float32 values
    the kernel receives."""
    o64, t64 = own.double(), other.double()
    n = (o64 + sample_zeros(other, own, torch.float64)).pow(2).sum(1).sqrt()
    mag = o64.pow(2).sum(1).sqrt() + t64.pow(2).sum(1).sqrt()
    return n - (f32(alpha) * mag + f32(beta))


@functools.lru_cache(maxsize=None)
def smooth_case(B, H, W, seed):
    """(bflow, fflow, d_bw, d_fw) on the CPU, with the cap on what the margin hides asserted on the float64 side."""
    b, f = smooth_pair(B, H, W, seed)
    d_bw, d_fw = margin64(b, f), margin64(f, b)
    for name, d in (("bw", d_bw), ("fw", d_fw)):
        share = float((d.abs() < MARGIN).double().mean())
        print("excluded share %s %s: %.4f %%, occluded %.1f %%" % (name, (B, H, W), 100 * share, 100 * float((d > 0).double().mean())))
        assert share <= MAX_EXCLUDED, (name, share)
    return b, f, d_bw, d_fw


@functools.lru_cache(maxsize=None)
def device_masks(B, H, W, seed):
    from accflow_amd import ops
    b, f = smooth_pair(B, H, W, seed)
    bw, fw = ops.fb_occlusion(b.cuda(), f.cuda())
    return bw, fw


def assert_bits(mask, d, what):
    """mask (B,1,H,W) from the kernel against d (B,H,W): only 0.0 / 1.0, and equal to d > 0 outside the margin."""
    m = mask.cpu()[:, 0]
    assert bool(((m == 0) | (m == 1)).all()), what
    decided = d.abs() >= MARGIN                  # (False for a NaN d)
    wrong = decided & (m != (d > 0).float())
    assert not bool(wrong.any()), "%s: %d wrong bits, largest |d| among them %.3e" % (
        what, int(wrong.sum()), float(d[wrong].abs().max()))


# ------------------------------------------------------------------------------------------------
# 1. masks against float64


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_masks_vs_float64(case):
    b, f, d_bw, d_fw = smooth_case(*case)
    bw, fw = device_masks(*case)
    assert tuple(bw.shape) == tuple(fw.shape) == (case[0], 1, case[1], case[2]) and bw.dtype == torch.float32
    assert_bits(bw, d_bw, "occ_bw")
    assert_bits(fw, d_fw, "occ_fw")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_single_masks_strided_outputs_and_sliced_inputs(case):
    from accflow_amd import ops
    B, H, W, _ = case
    b, f = smooth_pair(*case)
    bw, fw = device_masks(*case)
    bd, fd = b.cuda(), f.cuda()
    only_bw = ops.fb_occlusion(bd, fd, want=("bw",))
    only_fw = ops.fb_occlusion(bd, fd, want=("fw",))
    assert only_bw[1] is None and only_fw[0] is None
    assert torch.equal(only_bw[0], bw) and torch.equal(only_fw[1], fw)
    # outputs: channel slices of a larger tensor (batch stride 5 HW), untouched around them
    big = torch.full((B, 5, H, W), 7.0, device="cuda")
    got = ops.fb_occlusion(bd, fd, out_bw=big[:, 1:2], out_fw=big[:, 3:4])
    assert got[0].data_ptr() == big[:, 1:2].data_ptr() and got[1].data_ptr() == big[:, 3:4].data_ptr()
    assert torch.equal(big[:, 1:2], bw) and torch.equal(big[:, 3:4], fw)
    assert bool((big[:, (0, 2, 4)] == 7.0).all())
    # inputs: channel slices of one (B, 6, H, W) tensor
    both = torch.full((B, 6, H, W), float("nan"), device="cuda")
    both[:, 1:3], both[:, 4:6] = bd, fd
    sl = ops.fb_occlusion(both[:, 1:3], both[:, 4:6])
    assert torch.equal(sl[0], bw) and torch.equal(sl[1], fw)


# ------------------------------------------------------------------------------------------------
# 2. masks against what exists


def test_masks_vs_reference_output(golden):
    from accflow_amd import ops
    g = golden("harness")
    bw, fw = ops.fb_occlusion(T(g["bflow"]).cuda(), T(g["fflow"]).cuda())
    for name, got in (("occ_bw", bw), ("occ_fw", fw)):
        share = float((got.cpu() != T(g[name])).float().mean())
        print("mismatch share against the reference, %s: %.2e" % (name, share))
        assert share < 2e-3, (name, share)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_masks_vs_calc_occ_mask(case):
    from accflow_amd import eval_cvo
    b, f, d_bw, d_fw = smooth_case(*case)
    bw, fw = device_masks(*case)
    old_bw, old_fw = eval_cvo.calc_occ_mask(b.cuda(), f.cuda())
    for name, new, old, d in (("bw", bw, old_bw, d_bw), ("fw", fw, old_fw, d_fw)):
        differ = (new != old).cpu()[:, 0]
        assert bool((d[differ].abs() < MARGIN).all()), (name, int(differ.sum()), float(d[differ].abs().max()))


# ------------------------------------------------------------------------------------------------
# 3. edge semantics


def test_zero_flows_are_nowhere_occluded():
    from accflow_amd import ops
    z = torch.zeros(2, 2, 19, 67, device="cuda")
    bw, fw = ops.fb_occlusion(z, z)
    assert not bool(bw.any()) and not bool(fw.any())


@pytest.mark.parametrize("alpha", (0.01, 0.7))
def test_constant_flow_that_leaves_the_frame(alpha):
    """Every sample lies outside: diff = the flow itself, so the bit is |f| > alpha (|f| + |b|) + beta, the same for every
    pixel; evaluated here on the host.  alpha = 0.7: the shorter flow of the pair is NOT occluded, the longer one is."""
    from accflow_amd import ops
    B, H, W = 2, 21, 70
    f = torch.zeros(B, 2, H, W)
    b = torch.zeros(B, 2, H, W)
    f[:, 0], f[:, 1] = W + 5.0, 3.0
    b[:, 0], b[:, 1] = -2.0, -(10.0 * H)
    nf, nb = math.hypot(W + 5.0, 3.0), math.hypot(2.0, 10.0 * H)
    thr = f32(alpha) * (nf + nb) + BETA
    assert abs(nf - thr) > 1.0 and abs(nb - thr) > 1.0          # far from the boundary: float32 decides as the host does
    bw, fw = ops.fb_occlusion(b.cuda(), f.cuda(), alpha=alpha)
    assert bool((fw == float(nf > thr)).all()) and bool((bw == float(nb > thr)).all())
    if alpha == 0.7:
        assert nf < thr < nb


def test_non_finite_flows():
    """A handful of NaN / +-inf / 1e9 entries: no fault, only 0 / 1 come out, and every pixel whose float64 result is a
    number outside the margin still matches (a NaN result - the pixel's own flow, or a sampled neighbourhood that holds a
    non-finite value - is the kernel's 0 by the comparison and is not checked against float64)."""
    from accflow_amd import ops
    B, H, W, seed = CASES[0]
    b, f = [t.clone() for t in smooth_pair(B, H, W, seed)]
    nan, inf = float("nan"), float("inf")
    for t, spots in ((f, ((0, 0, 5, 7, nan), (0, 1, 20, 30, inf), (1, 0, 11, 2, -inf), (1, 1, 36, 52, 1.0e9), (1, 0, 3, 40, -1.0e9))),
                     (b, ((0, 1, 8, 8, nan), (0, 0, 30, 10, -inf), (1, 1, 0, 1, inf), (1, 0, 25, 25, 1.0e9)))):
        for n, c, y, x, v in spots:
            t[n, c, y, x] = v
    d_bw, d_fw = margin64(b, f), margin64(f, b)
    checked = float(((d_bw.abs() >= MARGIN) & (d_fw.abs() >= MARGIN)).double().mean())
    assert checked > 0.95, checked                               # the specials leave nearly every pixel checkable
    bw, fw = ops.fb_occlusion(b.cuda(), f.cuda())
    torch.cuda.synchronize()
    assert_bits(bw, d_bw, "occ_bw")
    assert_bits(fw, d_fw, "occ_fw")
    sums = ops.flow_metrics(f.cuda(), b.cuda(), fflow=f.cuda())   # the fused mode reads the same addresses
    torch.cuda.synchronize()
    assert float(sums[:, 7].min()) == H * W


# ------------------------------------------------------------------------------------------------
# 4. sums against float64


def test_stage1_run_length():
    from accflow_amd import _lib
    q = _lib.load().accflow_flow_metrics_ws_bytes
    assert q(1, 1, RUN) == 32 and q(1, 1, RUN + 1) == 64 and q(3, 1, RUN) == 96


@functools.lru_cache(maxsize=None)
def metric_case(B, H, W, seed):
    """(pred, gt, binary mask, fractional mask) on the CPU: pred = gt + 2.5 * smooth noise, so that 1, 3 and 5 px all split the
    pixels."""
    gt, _ = smooth_pair(B, H, W, seed)
    g = gen(seed + 100)
    pred = gt + 2.5 * enlarge(torch.randn(B, 2, 6, 9, generator=g), H, W)
    w = enlarge(torch.randn(B, 1, 4, 5, generator=g), H, W)
    return pred.contiguous(), gt, (w > 0).float().contiguous(), w.abs().contiguous()


def sums64(pred, gt, mask):
    d = pred.double() - gt.double()
    epe = d.pow(2).sum(1).sqrt()
    m = mask.double()[:, 0] if mask is not None else torch.zeros_like(epe)
    l1 = d.abs().sum(1)
    cols = [epe, epe * m, m, (epe < 1).double(), (epe < 3).double(), (epe < 5).double(), l1, torch.ones_like(epe)]
    return torch.stack([c.flatten(1).sum(1) for c in cols], dim=1), epe


def assert_sums(got, pred, gt, mask, what, exact_mask):
    B, _, H, W = pred.shape
    got = got.cpu()
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, 8)
    want, epe = sums64(pred, gt, mask)
    rel = (4 + math.log2(min(RUN, H * W))) * 2.0 ** -23
    for col in (0, 1, 6) + (() if exact_mask else (2,)):
        err = (got[:, col] - want[:, col]).abs()            # (every term is >= 0: the sum of absolute terms is the sum)
        print("%s column %d: error / bound = %.3f" % (what, col, float((err / (rel * want[:, col]).clamp_min(1e-300)).max())))
        assert bool((err <= rel * want[:, col]).all()), (what, col, err.tolist(), (rel * want[:, col]).tolist())
    if exact_mask:
        assert torch.equal(got[:, 2], want[:, 2]), what
    assert torch.equal(got[:, 7], torch.full((B,), float(H * W), dtype=torch.float64)), what
    for col, thr in ((3, 1.0), (4, 3.0), (5, 5.0)):
        near = ((epe - thr).abs() < 1e-5).flatten(1).sum(1).double()
        assert bool((near <= 1e-3 * H * W).all()), (what, thr, near.tolist())
        assert bool(((got[:, col] - want[:, col]).abs() <= near).all()), (what, col, got[:, col].tolist(), want[:, col].tolist())
        share = want[:, col] / (H * W)
        assert bool(((share > 0.002) & (share < 0.998)).all()), (what, thr, share.tolist())   # the threshold splits the pixels


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sums_vs_float64(case):
    from accflow_amd import ops
    pred, gt, mbin, mfrac = metric_case(*case)
    pd, gd = pred.cuda(), gt.cuda()
    s0 = ops.flow_metrics(pd, gd)
    assert not bool(s0[:, 1:3].any())
    assert_sums(s0, pred, gt, None, "mode 0", True)
    assert_sums(ops.flow_metrics(pd, gd, mask=mbin.cuda()), pred, gt, mbin, "mode 1, binary mask", True)
    assert_sums(ops.flow_metrics(pd, gd, mask=mfrac.cuda()), pred, gt, mfrac, "mode 1, weights", False)
    # operands as channel slices of larger tensors
    B, H, W, _ = case
    big = torch.full((B, 7, H, W), float("nan"), device="cuda")
    big[:, 0:2], big[:, 2:4], big[:, 5:6] = pd, gd, mbin.cuda()
    assert torch.equal(ops.flow_metrics(big[:, 0:2], big[:, 2:4], mask=big[:, 5:6]), ops.flow_metrics(pd, gd, mask=mbin.cuda()))


def test_metrics_vs_reference_output(golden):
    from accflow_amd import metrics
    g = golden("harness")
    m = metrics.flow_metrics(T(g["pred"]).cuda(), T(g["bflow"]).cuda(), T(g["occ_bw"]).cuda())
    for got, key in ((m.epe, "epe_all"), (m.epe_occ, "epe_occ"), (m.epe_vis, "epe_vis")):
        want = T(g[key]).double()
        err = (got.cpu() - want).abs()
        assert bool((err <= 1e-5 + 1e-4 * want.abs()).all()), (key, float(err.max()))       # test_harness_vs_golden's gate
        assert bool((err <= 1e-5).all()), (key, float(err.max()))


# ------------------------------------------------------------------------------------------------
# 5. reproducibility


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_rows_do_not_depend_on_the_batch(mode):
    from accflow_amd import ops
    case = CASES[1]                                   # B = 3
    pred, gt, mbin, _ = metric_case(*case)
    _, f = smooth_pair(*case)
    pd, gd, md, fd = pred.cuda(), gt.cuda(), mbin.cuda(), f.cuda()

    def run(idx):
        kw = {} if mode == 0 else ({"mask": md[idx]} if mode == 1 else {"fflow": fd[idx]})
        return ops.flow_metrics(pd[idx], gd[idx], **kw)
    whole = run(slice(None))
    assert torch.equal(whole, run(slice(None)))       # two calls: equal bits
    for k in range(case[0]):
        assert torch.equal(run(slice(k, k + 1))[0], whole[k]), k
    flipped = run(torch.tensor([2, 1, 0, 1], device="cuda"))            # other places in a batch of another size
    assert torch.equal(flipped, whole[[2, 1, 0, 1]])


def test_several_partials_per_sample():
    from accflow_amd import ops
    B, H, W = 2, 264, 520
    assert H * W > 8 * RUN
    g = gen(31)
    gt = enlarge(6 * torch.randn(B, 2, 3, 4, generator=g), H, W)
    pred = gt + 2.5 * enlarge(torch.randn(B, 2, 6, 9, generator=g), H, W)
    mask = (enlarge(torch.randn(B, 1, 4, 5, generator=g), H, W) > 0).float()
    got = ops.flow_metrics(pred.cuda(), gt.cuda(), mask=mask.cuda())
    assert got[:, 7].tolist() == [float(H * W)] * B
    assert_sums(got, pred, gt, mask, "264x520", True)
    assert torch.equal(ops.flow_metrics(pred[1:].cuda(), gt[1:].cuda(), mask=mask[1:].cuda())[0], got[1])


# ------------------------------------------------------------------------------------------------
# 6. fused mode


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_mode(case):
    from accflow_amd import eval_cvo, metrics, ops
    B, H, W, _ = case
    pred, bflow, _, _ = metric_case(*case)            # (metric_case's gt IS the pair's backward flow)
    b, f, d_bw, _ = smooth_case(*case)
    assert bflow is b
    pd, bd, fd = pred.cuda(), b.cuda(), f.cuda()
    bw, _ = device_masks(*case)
    fused = ops.flow_metrics(pd, bd, fflow=fd)
    assert torch.equal(fused, ops.flow_metrics(pd, bd, mask=bw))
    # against the torch route it replaces
    m = metrics.cvo_metrics(pd, bd, fd)
    assert torch.equal(m.sums, fused)
    old_mask, _ = eval_cvo.calc_occ_mask(bd, fd)
    e_all, e_occ, e_vis = [t.double().cpu() for t in eval_cvo.cal_epe(pd, bd, old_mask)]
    assert bool(((m.epe.cpu() - e_all).abs() <= 1e-5 * e_all).all())
    # the two routes may disagree on the pixels inside the margin: each moves a sum by at most the largest EPE
    n_margin = (d_bw.abs() < MARGIN).flatten(1).sum(1).double()
    epe_max = (pred.double() - b.double()).pow(2).sum(1).sqrt().flatten(1).max(1).values
    n_occ = fused[:, 2].cpu()
    for name, got, want, n in (("occ", m.epe_occ, e_occ, n_occ), ("vis", m.epe_vis, e_vis, H * W - n_occ)):
        # k pixels changing sides turn S / N into (S + s) / (N +- k) with 0 <= s <= k epe_max: a change of
        # |s -+ k S / N| / (N +- k) <= k epe_max / (this route's mask sum)
        tol = 1e-5 + n_margin * epe_max / n
        err = (got.cpu() - want).abs()
        print("epe_%s: error %.3e, of which the margin pixels may make %.3e" % (name, float(err.max()), float((tol - 1e-5).max())))
        assert bool((err <= tol).all()), (name, got.tolist(), want.tolist(), tol.tolist())


def test_occlusion_masks_module_entry():
    from accflow_amd import metrics
    case = CASES[0]
    b, f = smooth_pair(*case)
    bw, fw = device_masks(*case)
    got = metrics.occlusion_masks(b.cuda(), f.cuda())
    assert torch.equal(got[0], bw) and torch.equal(got[1], fw)


# ------------------------------------------------------------------------------------------------
# 7. train_acc.validate


def test_validate_accumulates_on_the_device(monkeypatch):
    from accflow_amd import train_acc
    B, H, W, n_out = 2, 24, 40, 5
    g = gen(41)
    batches, outs = [], []
    for _ in range(2):
        bflows = enlarge(4 * torch.randn(B, 2 * n_out, 3, 4, generator=g), H, W)
        batches.append({"imgs": torch.randint(0, 256, (B, 21, H, W), generator=g).float(), "bflows": bflows})
        outs.append([(bflows[:, 2 * k:2 * k + 2] + 2.0 * enlarge(torch.randn(B, 2, 5, 6, generator=g), H, W)).contiguous()
                     for k in range(n_out)])
    served = []

    def model(imgs):
        assert len(imgs) == 7
        served.append(len(served))
        return [o.cuda() for o in outs[served[-1]]]
    # the parent's formulas, per batch, in double
    want = {k: 0.0 for k in ("val_epe", "val_1px", "val_3px", "val_5px", "val_loss")}
    for batch, out in zip(batches, outs):
        gts = [t.contiguous() for t in batch["bflows"].split(2, dim=1)]
        m = train_acc.sequence_loss_metrics([o.double() for o in out], [t.double() for t in gts])
        m["loss"] = sum(float((o.double() - t.double()).abs().mean()) for o, t in zip(out, gts))
        for k, v in m.items():
            want["val_" + k] += v / len(batches)
    reads = []
    for name in ("item", "__float__", "__int__", "__bool__"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **kw):
            if self.is_cuda:
                reads.append(_name)
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    got, last = train_acc.validate(model, batches, torch.device("cuda"), None)
    monkeypatch.undo()
    assert reads == [], reads                                    # no host read of a device scalar, in any batch
    assert served == [0, 1] and torch.equal(last.cpu(), outs[1][-1])
    assert set(got) == set(want)
    for k in want:
        assert isinstance(got[k], float) and abs(got[k] - want[k]) <= 1e-6 * max(1.0, abs(want[k])), (k, got[k], want[k])
    assert 0.02 < got["val_1px"] < got["val_3px"] < got["val_5px"] <= 1.0
