"""The InstanceNorm chain of the encoders (csrc/misc.hip) on FABRICATED statistics: the merge of the convolution epilogues'
partial records (instance_stats_finalize_kernel), the four single-pass apply kernels (instance_norm_apply_kernel, _s16, _s16res,
_s16proj) and the three-pass instance_norm_kernel, against float64 references written here.

ops.ConvStats(partial, slots) is a plain constructor, so no convolution is needed: a test cuts a plane into groups of any
sizes (empty ones included), computes the records {sum, M2 about the group's mean, n} in float64, rounds them to float32 - these
are the records the kernel reads - and hands them over with any slot count, channel sub-range and partition.

Bounds (u = 2^-24, the unit roundoff of float32; none is taken from what the kernels give):

    finalize: the kernel sums the float32 records in double and rounds ONCE; another summation order in double moves the
      result by ~1e-16 relative, so the float32 value can differ from float32(merge64) only across a rounding tie: 1 ulp.
    apply, fp32: out = fl(fl(x - m) * r) with m = fl(mean), r = fl(rstd).  x - m: one rounding; the product: one; r: one -
      three relative errors of <= u on the result - and m = mean + e, |e| <= u |mean|, moves the result by rstd e.  relu()
      rounds nothing and cannot turn the relative part negative (so a reference of 0 leaves only the rstd e term); mode 2
      adds one rounding at |res + t| = |ref| when res >= 0 (the encoders' residuals are relu outputs, and so are the ones
      here: then ref >= t and the three errors on t are <= 3 u ref).  Together <= 4 u |ref| + u rstd |mean|
      <= 2^-22 (|ref| + rstd |mean|) = APPLY_BOUND.  test_apply_bound_holds_for_float32_arithmetic evaluates the same
      expression with float32 torch ops on the CPU and checks the derivation.
    projection: relu(r + t), t = relu(norm2(x)), r = norm3(proj): the fp32 bound of each term, 2^-22 (|t| + rstd2 |mean2|)
      + 2^-22 (|r| + rstd3 |mean3|) (the rounding of the sum is u |r + t| <= u (|r| + |t|), inside the fourth u of each), plus
      the S16 representation step S16_REL |ref| + S16_ABS - the bound tests/test_sampling_ops.py holds an S16 copy of an fp32
      value to (s16_close, line 971; the constants on line 48, their derivation on lines 25-26).
    three-pass kernel: the same APPLY_BOUND against the plane's own float64 mean and variance.
    single pass against three passes: twice APPLY_BOUND.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
EPS_IN = float(np.float32(1e-5))          # the library receives eps as a float and widens it: this is the value it adds
S16_REL, S16_ABS = 2.0 ** -22, 2.0 ** -29   # tests/test_sampling_ops.py:48
B = 2
KINDS = ("randn", "const", "far", "wide", "spike", "steps")
SLOT_COUNTS = (1, 64, 255, 256, 257, 2047, 2048, 2049, 3600, 5000)
# (C, c0, Ctot): the whole tensor (what every call without a projection does) and sub-ranges with channels on both sides
LAYOUTS = tuple((C, 0, C) for C in (5, 8, 12)) + tuple((C, c0, c0 + C + 1) for C in (5, 8, 12) for c0 in (0, 3, 8))
BANK_C = 21                                # 8 + 12 + 1: the widest layout
LANE = 37                                  # records LANE, LANE + 256, ...: everything one thread of the kernel reads
HW_SHAPES = {1: (1, 1), 3: (1, 3), 60: (6, 10), 63: (7, 9), 64: (8, 8), 511: (7, 73), 512: (16, 32), 516: (12, 43),
             960: (24, 40), 2052: (36, 57)}
# slot counts of the apply cases: far more slots than pixels leaves most of them empty, 2049 and 3600 enter the tail loop
HW_SLOTS = {1: 1, 3: 2, 60: 7, 63: 257, 64: 64, 511: 255, 512: 256, 516: 2048, 960: 2049, 2052: 3600}
APPLY_HW = (1, 60, 63, 960)
THREE_PASS_HW = (1, 3, 63, 64, 511, 512, 516, 2052)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def dev(t):
    return t.cuda()


# ------------------------------------------------------------------------------------------------
# records and float64 references


def make_records(plane_values, sizes):
    """Cut the values into consecutive groups of the given sizes (0 allowed) -> (len(sizes), 3) float32 records
    {sum, M2 about the group's own mean, n}, computed in float64 and rounded once."""
    v = torch.as_tensor(plane_values).double().reshape(-1)
    sizes = torch.as_tensor(sizes, dtype=torch.long).reshape(-1)
    assert int(sizes.sum()) == v.numel() and int(sizes.min()) >= 0
    S = sizes.numel()
    gid = torch.repeat_interleave(torch.arange(S), sizes)
    n = sizes.double()
    s = torch.zeros(S, dtype=torch.float64).index_add_(0, gid, v)
    mean = s / n.clamp(min=1.0)
    m2 = torch.zeros(S, dtype=torch.float64).index_add_(0, gid, (v - mean[gid]) ** 2)
    return torch.stack([s, m2, n], 1).float()


def merge64(records, eps=EPS_IN):
    """(..., S, 3) float32 records -> float64 (mean, rstd) of every plane: mean = sum(s) / sum(n), M2 = sum over n_i > 0 of
    M2_i + (s_i - n_i mean)^2 / n_i, biased variance; a plane without a pixel gives (0, eps^-1/2)."""
    r = records.double()
    s, m2, n = r[..., 0], r[..., 1], r[..., 2]
    N = n.sum(-1)
    has = N > 0
    Ns = torch.where(has, N, torch.ones_like(N))
    mean = torch.where(has, s.sum(-1) / Ns, torch.zeros_like(N))
    live = n > 0
    dd = s - n * mean[..., None]
    term = torch.where(live, m2 + dd * dd / torch.where(live, n, torch.ones_like(n)), torch.zeros_like(n))
    var = torch.where(has, term.sum(-1) / Ns, torch.zeros_like(N))
    return mean, 1.0 / torch.sqrt(var + eps)


def merge_unguarded(records, eps=EPS_IN):
    """Mutant (b): no n > 0 guards."""
    r = records.double()
    s, m2, n = r[..., 0], r[..., 1], r[..., 2]
    N = n.sum(-1)
    mean = s.sum(-1) / N
    dd = s - n * mean[..., None]
    return mean, 1.0 / torch.sqrt((m2 + dd * dd / n).sum(-1) / N + eps)


def merge_m2_about_zero(records, eps=EPS_IN):
    """Mutant (e): the records' M2 taken for sums of squares about 0: var = sum(M2_i) / n - mean^2."""
    r = records.double()
    N = r[..., 2].sum(-1).clamp(min=1.0)
    mean = r[..., 0].sum(-1) / N
    return mean, 1.0 / torch.sqrt(r[..., 1].sum(-1) / N - mean * mean + eps)


def read_planes(partial, slots, Ctot, c0, C):
    """(B, C, slots, 3): the records the kernel's index expression ((b * Ctot + c0 + c) * slots) * 3 reaches in the flat
    table, zeros behind its end (the mutants with a wrong slots / Ctot / c0 read there; the kernel never does)."""
    flat = partial.reshape(-1)
    rows = []
    for b in range(partial.shape[0]):
        for c in range(C):
            at = ((b * Ctot + c0 + c) * slots) * 3
            part = flat[at:at + 3 * slots]
            rows.append(torch.cat([part, torch.zeros(3 * slots - part.numel())]).view(slots, 3))
    return torch.stack(rows).view(partial.shape[0], C, slots, 3)


def stats64(x):
    """float64 (mean, rstd) of the planes of x (B, C, H, W) themselves."""
    xd = x.double().flatten(2)
    return xd.mean(-1), 1.0 / torch.sqrt(xd.var(-1, unbiased=False) + EPS_IN)


def norm64(x, mean, rstd):
    return (x.double() - mean[..., None, None]) * rstd[..., None, None]


def apply64(x, mean, rstd, mode, res=None):
    """mode 0: norm; 1: relu(norm); 2: relu(res + relu(norm))."""
    v = norm64(x, mean, rstd)
    if mode >= 1:
        v = torch.relu(v)
    if mode == 2:
        v = torch.relu(res.double() + v)
    return v


def proj64(x, mean2, rstd2, proj, mean3, rstd3):
    """relu(norm3(proj) + relu(norm2(x))) and its two terms."""
    t, r = torch.relu(norm64(x, mean2, rstd2)), norm64(proj, mean3, rstd3)
    return torch.relu(r + t), t, r


def apply_bound(ref, mean, rstd):
    return 2.0 ** -22 * (ref.abs() + (rstd * mean.abs())[..., None, None])


def ulp32(ref64):
    """float32(ref) and the spacing of float32 there."""
    r32 = ref64.float()
    return r32.double(), torch.from_numpy(np.spacing(np.abs(r32.numpy()))).double()


def off_by_more_than_an_ulp(got64, ref64):
    r32, ulp = ulp32(ref64)
    g32 = got64.float().double()
    return ~torch.isfinite(g32) | ((g32 - r32).abs() > ulp)


def within(tag, got, ref, bound):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), tag + ": not finite"
    err = (got - ref).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print("RATIO %s %.3f" % (tag, ratio))
    assert bool((err <= bound).all()), "%s: error / bound = %.3f" % (tag, ratio)


# ------------------------------------------------------------------------------------------------
# inputs


def values(kind, sizes, g):
    """float32 pixels of one plane, sum(sizes) of them."""
    n = int(sizes.sum())
    if kind == "randn":
        return torch.randn(n, generator=g)
    if kind == "const":                    # every M2_i = 0, and n_i * 2.5 is exact in float32: the mean is 2.5 exactly
        return torch.full((n,), 2.5)
    if kind == "far":
        return 1.0e3 + 1.0e-2 * torch.randn(n, generator=g)
    if kind == "wide":
        return -40.0 + 30.0 * torch.randn(n, generator=g)
    if kind == "spike":
        v = torch.zeros(n)
        if n:
            v[n // 3] = 1.0e3
        return v
    if kind == "steps":                    # constant inside a group: every M2_i = 0, the variance comes from the dd term alone
        return torch.repeat_interleave(2.0 * torch.randn(sizes.numel(), generator=g), sizes)
    if kind == "outside":                  # channels outside [c0, c0 + C): a mis-indexed read lands on a mean of 7
        return 7.0 + 0.5 * torch.randn(n, generator=g)
    raise KeyError(kind)


def ragged_sizes(S, g, last_empty):
    """Group sizes as ragged tiles give them: uneven in 1..128, ~10 % of the slots empty at scattered positions, every slot of
    the 256-stride lane LANE among them, and the last slot when asked (on every second plane: with 2049 slots it is the one
    record of the tail loop, which must meet both a full and an empty one)."""
    sizes = 1 + (128 * torch.rand(S, generator=g) ** 2).long().clamp(max=127)
    if S >= 2:
        sizes[torch.rand(S, generator=g) < 0.09] = 0
        sizes[LANE::256] = 0
        sizes[S - 1] = 0 if last_empty else max(int(sizes[S - 1]), 1)
        if int(sizes.sum()) == 0:
            sizes[0] = 5
    return sizes


def plane_kind(b, c, extra=0):
    return (c + 3 * b + extra) % len(KINDS)


@functools.lru_cache(maxsize=None)
def bank(S):
    """(B, BANK_C, S, 3) records of planes whose value distributions differ from neighbour to neighbour (any 5 consecutive
    channels of the two items hold every kind and a plane without a pixel), and one plane of records for the channels
    outside a sub-range."""
    g = gen(1000 + S)
    rec = torch.zeros(B, BANK_C, S, 3)
    for b in range(B):
        for c in range(BANK_C):
            k = (c + 3 * b) % (len(KINDS) + 1)
            if k == len(KINDS):
                continue                                             # all slots empty
            sizes = ragged_sizes(S, g, last_empty=(b + c) % 2 == 1)
            rec[b, c] = make_records(values(KINDS[k], sizes, g), sizes)
    sizes = ragged_sizes(S, g, last_empty=False)
    return rec, make_records(values("outside", sizes, g), sizes)


def finalize_case(S, C, c0, Ctot):
    rec, outside = bank(S)
    partial = rec[:, :Ctot].clone()
    partial[:, :c0] = outside
    partial[:, c0 + C:] = outside
    return partial.contiguous()


def split_sizes(HW, S, g):
    """S group sizes that sum to HW, cut at random positions (empty groups wherever two cuts coincide)."""
    cuts = torch.sort(torch.randint(0, HW + 1, (S - 1,), generator=g)).values
    edges = torch.cat([torch.zeros(1, dtype=torch.long), cuts, torch.full((1,), HW, dtype=torch.long)])
    return edges[1:] - edges[:-1]


class Case:
    pass


@functools.lru_cache(maxsize=None)
def apply_case(C, HW, S=None, extra=0, seed=0):
    """x (B, C, H, W) with the value kinds mixed over the planes, its fabricated records over S slots, a residual >= 0 and
    the float64 statistics: `mean`, `rstd` merged from the float32 records (what a single-pass kernel is given) and `mean_x`,
    `rstd_x` of the planes themselves (what the three-pass kernel computes)."""
    k = Case()
    k.C, k.HW, k.S = C, HW, HW_SLOTS[HW] if S is None else S
    H, W = HW_SHAPES[HW]
    g = gen(seed + 7919 * C + HW + 31 * k.S)
    x, rec = torch.zeros(B, C, HW), torch.zeros(B, C, k.S, 3)
    for b in range(B):
        for c in range(C):
            sizes = split_sizes(HW, k.S, g)
            x[b, c] = values(KINDS[plane_kind(b, c, extra)], sizes, g)
            rec[b, c] = make_records(x[b, c], sizes)
    k.x, k.records = x.view(B, C, H, W).contiguous(), rec
    k.res = torch.rand(B, C, H, W, generator=g) * (torch.rand(B, C, H, W, generator=g) < 0.8)     # relu-like: >= 0 with zeros
    k.mean, k.rstd = merge64(rec)
    k.mean_x, k.rstd_x = stats64(k.x)
    return k


PROJ_CASES = ((5, 0, 63, 257, 3600), (8, 8, 960, 3600, 257), (12, 8, 60, 257, 3600), (12, 0, 63, 3600, 257))


@functools.lru_cache(maxsize=None)
def proj_case(C, c0, HW, S, Sp):
    """x with S slots; the raw projection = channels [c0, c0 + C) of a tensor of Ctot = c0 + C + 3 channels with Sp slots."""
    k = apply_case(C, HW, S=S)
    p = apply_case(C, HW, S=Sp, extra=2, seed=500)
    out = apply_case(c0 + C + 3, HW, S=Sp, extra=4, seed=900)
    q = Case()
    q.C, q.c0, q.HW, q.Ctot, q.x, q.stats = C, c0, HW, c0 + C + 3, k, p
    q.wide = torch.full((B, q.Ctot) + HW_SHAPES[HW], float("nan"))       # a pixel read outside the slice poisons the result
    q.wide[:, c0:c0 + C] = p.x
    q.records = out.records.clone()                                       # ... and a record read outside it is another plane's
    q.records[:, c0:c0 + C] = p.records
    return q


def proj_reference(q, mean3=None, rstd3=None):
    m3, r3 = (q.stats.mean, q.stats.rstd) if mean3 is None else (mean3, rstd3)
    ref, t, r = proj64(q.x.x, q.x.mean, q.x.rstd, q.stats.x, m3, r3)
    bound = apply_bound(t, q.x.mean, q.x.rstd) + apply_bound(r, q.stats.mean, q.stats.rstd) + S16_REL * ref.abs() + S16_ABS
    return ref, bound


# ------------------------------------------------------------------------------------------------
# CPU: the references themselves


def test_merged_records_agree_with_the_plane_statistics():
    """The float32 rounding of the records is all that separates merge64(make_records(x)) from the statistics of x: 1e-6
    relative.  On the planes whose spread is far below their mean, `relative` means relative to what is summed: a record's
    sum carries u |s_i|, so the mean moves by u |mean| and the variance by ~u E[x^2] - not by u var."""
    g = gen(3)
    for kind in KINDS:
        for S, n in ((1, 40), (7, 60), (300, 5000), (2500, 40000)):
            sizes = split_sizes(n, S, g)
            x = values(kind, sizes, g)
            mean, rstd = merge64(make_records(x, sizes))
            xd = x.double()
            m, v = float(xd.mean()), float(xd.var(unbiased=False))
            var = 1.0 / float(rstd) ** 2 - EPS_IN
            second = v + m * m
            assert abs(float(mean) - m) <= 1e-6 * second ** 0.5, (kind, S)
            assert abs(var - v) <= 1e-6 * second, (kind, S)
            if kind in ("randn", "wide", "spike"):
                assert abs(float(mean) - m) <= 1e-6 * abs(m) and abs(var - v) <= 1e-6 * v, (kind, S)
    empty = make_records(torch.zeros(0), torch.zeros(9, dtype=torch.long))
    mean, rstd = merge64(empty)
    assert float(mean) == 0.0 and np.float32(float(rstd)) == np.float32(EPS_IN ** -0.5)
    # eps is the FLOAT the C entry points take (as nn.InstanceNorm2d adds it in float32): 1e-5 as a double would put the rstd
    # of a plane without a pixel on the neighbouring float32
    assert np.float32(EPS_IN ** -0.5) == np.float32(316.22778) and np.float32(1e-5 ** -0.5) == np.float32(316.22775)


def test_formulas_agree_with_torch_in_float64():
    k = apply_case(5, 63)
    want = F.instance_norm(k.x.double(), eps=EPS_IN)
    res = k.res.double()
    for mode, w in ((0, want), (1, torch.relu(want)), (2, torch.relu(res + torch.relu(want)))):
        got = apply64(k.x, k.mean_x, k.rstd_x, mode, k.res)
        assert float(((got - w).abs() / (1.0 + w.abs())).max()) <= 1e-9, mode     # ("far" planes: x - mean cancels 5 digits)
    q = proj_case(*PROJ_CASES[0])
    mx, rx = stats64(q.x.x)
    mp, rp = stats64(q.stats.x)
    got = proj64(q.x.x, mx, rx, q.stats.x, mp, rp)[0]
    w = torch.relu(F.instance_norm(q.stats.x.double(), eps=EPS_IN) + torch.relu(F.instance_norm(q.x.x.double(), eps=EPS_IN)))
    assert float(((got - w).abs() / (1.0 + w.abs())).max()) <= 1e-9


def test_read_planes_is_the_channel_slice():
    for C, c0, Ctot in LAYOUTS:
        partial = finalize_case(257, C, c0, Ctot)
        assert torch.equal(read_planes(partial, 257, Ctot, c0, C), partial[:, c0:c0 + C])


@pytest.mark.parametrize("HW", sorted(set(APPLY_HW + THREE_PASS_HW)))
def test_apply_bound_holds_for_float32_arithmetic(HW):
    """APPLY_BOUND's derivation, checked: the kernel's expression in float32 on the correctly rounded statistics."""
    k = apply_case(5, HW)
    m32, r32 = k.mean.float()[..., None, None], k.rstd.float()[..., None, None]
    for mode in (0, 1, 2):
        v = (k.x - m32) * r32
        if mode >= 1:
            v = torch.relu(v)
        if mode == 2:
            v = torch.relu(k.res + v)
        ref = apply64(k.x, k.mean, k.rstd, mode, k.res)
        within("float32 arithmetic HW=%d mode %d" % (HW, mode), v, ref, apply_bound(ref, k.mean, k.rstd))


# ------------------------------------------------------------------------------------------------
# CPU: every case can tell a wrong merge from a right one (by more than the GPU tests' tolerance)


@pytest.mark.parametrize("S", SLOT_COUNTS)
def test_mutant_stop_at_record_2048(S):
    """(a) a merge that never enters the tail loop."""
    rec = bank(S)[0]
    mean, rstd = merge64(rec)
    m, r = merge64(rec[:, :, :2048])
    wrong = off_by_more_than_an_ulp(m, mean) | off_by_more_than_an_ulp(r, rstd)
    if S <= 2048:
        assert not bool(wrong.any())                                  # (nothing behind record 2047: these cannot tell)
    else:
        assert int(wrong.sum()) >= 8, S                               # with 2049 slots: the planes whose last slot is full


@pytest.mark.parametrize("S", SLOT_COUNTS)
def test_mutant_no_empty_record_guard(S):
    """(b) must give NaN or inf on every plane that has an empty slot."""
    rec = bank(S)[0]
    has_empty = (rec[..., 2] == 0).any(-1)
    assert bool(has_empty.any()) and bool(torch.isfinite(torch.stack(merge64(rec))).all())
    m, r = merge_unguarded(rec)
    assert bool((~torch.isfinite(r))[has_empty].all()), S
    empty_plane = (rec[..., 2] == 0).all(-1)
    assert int(empty_plane.sum()) == 6
    if S >= 64:                                                       # the inputs are what ragged_sizes promises
        odd = (torch.arange(B)[:, None] + torch.arange(BANK_C)[None]) % 2 == 1
        last = rec[:, :, S - 1, 2]
        assert bool(has_empty.all()) and bool((rec[:, :, LANE::256, 2] == 0).all())
        assert bool((last[odd] == 0).all()) and bool((last[~odd & ~empty_plane] > 0).all())
        share = float((rec[..., 2] == 0)[~empty_plane].float().mean())
        assert 0.05 <= share <= 0.15, share


@pytest.mark.parametrize("S", SLOT_COUNTS)
def test_mutants_wrong_offset_and_m2_about_zero(S):
    """(c) c0 ignored; (e) record M2 taken for a sum of squares about 0."""
    for C, c0, Ctot in LAYOUTS:
        partial = finalize_case(S, C, c0, Ctot)
        mean, rstd = merge64(partial[:, c0:c0 + C])
        if c0:
            m, r = merge64(read_planes(partial, S, Ctot, 0, C))
            assert bool((off_by_more_than_an_ulp(m, mean) | off_by_more_than_an_ulp(r, rstd)).any()), (S, C, c0)
            m, r = merge64(read_planes(partial, S, C, c0, C))         # ... and C in the place of Ctot
            assert bool((off_by_more_than_an_ulp(m, mean) | off_by_more_than_an_ulp(r, rstd)).any()), (S, C, c0)
        m, r = merge_m2_about_zero(partial[:, c0:c0 + C])
        assert bool(off_by_more_than_an_ulp(r, rstd).any()), (S, C, c0)


@pytest.mark.parametrize("case", PROJ_CASES)
def test_mutant_second_tensor_read_with_the_first_one_s_geometry(case):
    """(d) the projection's records read with the slot count / the channel count of x's statistics."""
    q = proj_case(*case)
    ref, bound = proj_reference(q)
    assert torch.equal(read_planes(q.records, q.stats.S, q.Ctot, q.c0, q.C), q.stats.records)
    mutants = [(q.x.S, q.Ctot, q.c0), (q.stats.S, q.C, q.c0)] + ([(q.stats.S, q.Ctot, 0)] if q.c0 else [])
    for slots, Ctot, c0 in mutants:
        m, r = merge64(read_planes(q.records, slots, Ctot, c0, q.C))
        wrong = proj_reference(q, m, r)[0]
        assert bool((~((wrong - ref).abs() <= bound)).any()), (case, slots, Ctot, c0)


# ------------------------------------------------------------------------------------------------
# GPU


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as o
    assert torch.cuda.is_available()
    return o


def conv_stats(ops, records, S):
    return ops.ConvStats(dev(records.contiguous()), S)


@gpu
@pytest.mark.parametrize("S", SLOT_COUNTS)
def test_finalize(ops, S):
    """instance_stats_finalize_kernel over every layout: the register records and (S > 2048) the tail loop, empty records in
    both, planes without a pixel, sub-ranges between other planes' records; within one float32 ulp of the float64 merge, and
    the same bits when run again."""
    for C, c0, Ctot in LAYOUTS:
        partial = finalize_case(S, C, c0, Ctot)
        st = conv_stats(ops, partial, S)
        sub = {} if (c0, Ctot) == (0, C) else {"c0": c0, "C": C}
        got = ops.instance_stats_finalize(st, **sub)
        again = ops.instance_stats_finalize(st, **sub)
        assert tuple(got.shape) == (B, C, 2)
        assert torch.equal(got, again), "finalize is not deterministic"
        got = got.cpu()
        assert bool(torch.isfinite(got).all()), (S, C, c0)
        mean, rstd = merge64(partial[:, c0:c0 + C])
        tag = "S=%d C=%d c0=%d Ctot=%d" % (S, C, c0, Ctot)
        for name, g, ref in (("mean", got[..., 0], mean), ("rstd", got[..., 1], rstd)):
            r32, ulp = ulp32(ref)
            err = (g.double() - r32).abs()
            print("ULPS %s %s %.2f" % (tag, name, float((err / ulp).max())))
            assert bool((err <= ulp).all()), "%s %s: %.2f ulp" % (tag, name, float((err / ulp).max()))
        empty = (partial[:, c0:c0 + C, :, 2] == 0).all(-1)
        assert bool(empty.any())
        assert bool((got[..., 0][empty] == 0.0).all()) and bool((got[..., 1][empty] == float(np.float32(EPS_IN ** -0.5))).all())


def check_apply(tag, k, mode, got, res=None):
    ref = apply64(k.x, k.mean, k.rstd, mode, k.res if res is None else res)
    within(tag, got, ref, apply_bound(ref, k.mean, k.rstd))
    if mode == 0:
        const = torch.tensor([[KINDS[plane_kind(b, c)] == "const" for c in range(k.C)] for b in range(B)])
        assert bool((got.cpu()[const] == 0.0).all()), tag + ": a constant plane must normalise to exact zeros"


@gpu
@pytest.mark.parametrize("HW", APPLY_HW)
def test_apply_fp32(ops, HW):
    """instance_norm_apply_kernel: the float4 path (HW % 4 == 0), the scalar path (63: a thread's four elements straddle two
    planes, and 2 * 5 * 63 = 630 leaves a partial last thread), in place and into a separate tensor."""
    k = apply_case(5, HW)
    st = conv_stats(ops, k.records, k.S)
    for mode in (0, 1, 2):
        res = dev(k.res) if mode == 2 else None
        xd = dev(k.x)
        got = ops.instance_norm(xd, mode, res, stats=st)
        assert got.data_ptr() == xd.data_ptr()
        check_apply("apply HW=%d mode %d in place" % (HW, mode), k, mode, got)
        xd, out = dev(k.x), torch.full(k.x.shape, float("nan"), device="cuda")
        assert ops.instance_norm(xd, mode, res, out=out, stats=st) is out
        assert torch.equal(out, got) and torch.equal(xd.cpu(), k.x)


def s16_forms(ops, k, st, mode, res):
    """The three ways of a pre-split apply call: fp32 in place, fp32 into `out`, S16 only.  Returns (fp32 result, S16)."""
    shape = (B, k.C) + HW_SHAPES[k.HW]
    xd, o16 = dev(k.x), ops.S16.empty(*shape, "cuda")
    o32 = ops.instance_norm(xd, mode, res, stats=st, out16=o16)
    assert o32.data_ptr() == xd.data_ptr()
    assert torch.equal(o16.data, ops.to_s16(o32).data), "the S16 copy is not the split of the fp32 result"
    xd, out, b16 = dev(k.x), torch.full(shape, float("nan"), device="cuda"), ops.S16.empty(*shape, "cuda")
    assert ops.instance_norm(xd, mode, res, out=out, stats=st, out16=b16) is out
    assert torch.equal(out, o32) and torch.equal(b16.data, o16.data) and torch.equal(xd.cpu(), k.x)
    xd, only = dev(k.x), ops.S16.empty(*shape, "cuda")
    assert ops.instance_norm(xd, mode, res, stats=st, out16=only, fp32_out=False) is only
    assert torch.equal(only.data, o16.data), "fp32_out=False changes the S16 result"
    assert torch.equal(xd.cpu(), k.x), "fp32_out=False must leave x alone"
    return o32, o16


@gpu
@pytest.mark.parametrize("HW", APPLY_HW)
@pytest.mark.parametrize("C", [5, 8, 12])
def test_apply_s16(ops, C, HW):
    """instance_norm_apply_s16_kernel and _s16res_kernel: the octet tail (C = 5, 12: channels c >= C of the last octet are
    zero-filled and write nothing), a full octet (8), out == NULL, a float and a pre-split residual."""
    k = apply_case(C, HW)
    st = conv_stats(ops, k.records, k.S)
    ops.guard_tripped()
    for mode in (0, 1, 2):
        o32, _ = s16_forms(ops, k, st, mode, dev(k.res) if mode == 2 else None)
        check_apply("apply s16 C=%d HW=%d mode %d" % (C, HW, mode), k, mode, o32)
    r16 = ops.to_s16(dev(k.res))
    o32, _ = s16_forms(ops, k, st, 2, r16)
    check_apply("apply s16res C=%d HW=%d" % (C, HW), k, 2, o32, res=r16.to_float().cpu())   # the residual as the S16 stores it
    assert not ops.guard_tripped()


@gpu
def test_apply_s16_guard(ops):
    """A residual of 5000 (above 65520 / 16) raises the flag, once; the tame calls around it do not."""
    k = apply_case(12, 60)
    st = conv_stats(ops, k.records, k.S)
    shape = (B, 12) + HW_SHAPES[60]
    ops.guard_tripped()
    ops.instance_norm(dev(k.x), 2, dev(k.res), stats=st, out16=ops.S16.empty(*shape, "cuda"), fp32_out=False)
    assert not ops.guard_tripped()
    res = k.res.clone()
    res[1, 11, 5, 9] = 5000.0
    ops.instance_norm(dev(k.x), 2, dev(res), stats=st, out16=ops.S16.empty(*shape, "cuda"), fp32_out=False)
    assert ops.guard_tripped()
    assert not ops.guard_tripped(), "reported once, then reset"
    ops.instance_norm(dev(k.x), 2, dev(k.res), stats=st, out16=ops.S16.empty(*shape, "cuda"))
    assert not ops.guard_tripped()


@gpu
@pytest.mark.parametrize("case", PROJ_CASES)
def test_projection(ops, case):
    """instance_norm_apply_s16proj_kernel and the SECOND statistics tensor of its finalize launch: another slot count and
    another channel count than the first one's, a channel offset, the projection a slice of a wider (NaN-filled) tensor."""
    q = proj_case(*case)
    shape = (B, q.C) + HW_SHAPES[q.HW]
    ops.guard_tripped()
    wide = dev(q.wide)
    o16 = ops.instance_norm_proj(dev(q.x.x), conv_stats(ops, q.x.records, q.x.S), wide[:, q.c0:q.c0 + q.C],
                                 conv_stats(ops, q.records, q.stats.S), q.c0, ops.S16.empty(*shape, "cuda"))
    ref, bound = proj_reference(q)
    within("projection C=%d c0=%d HW=%d slots %d / %d" % case, o16.to_float(), ref, bound)
    assert not ops.guard_tripped()


def check_three_pass(tag, k, mode, got):
    ref = apply64(k.x, k.mean_x, k.rstd_x, mode, k.res)
    within(tag, got, ref, apply_bound(ref, k.mean_x, k.rstd_x))


@gpu
@pytest.mark.parametrize("HW", THREE_PASS_HW)
def test_three_pass(ops, HW):
    """instance_norm_kernel: planes shorter than the workgroup (idle waves), HW = 1, 511 / 512 / 516 around its width, the
    float4 and the scalar loops, constant planes and planes far from zero.

    This test found the kernel's float32 sums out: on the unit-noise plane of item 1, whose mean is near zero by
    cancellation, the mean carried 26 x 2^-24 of itself at HW = 516 and 4.3 x at 2052 - error / bound 3.995 and 1.055 (the
    kernel's summation order replayed in float32 on the CPU gives the same two figures).  With the sums in double the
    largest error / bound over all cases is 0.51 (MI355X, 2026-10-18)."""
    k = apply_case(5, HW)
    for mode in (0, 1, 2):
        got = ops.instance_norm(dev(k.x), mode, dev(k.res) if mode == 2 else None)
        check_three_pass("three-pass HW=%d mode %d" % (HW, mode), k, mode, got)
        if HW == 1 and mode == 0:
            assert bool((got == 0.0).all())
        out, xd = torch.full(k.x.shape, float("nan"), device="cuda"), dev(k.x)
        assert ops.instance_norm(xd, mode, dev(k.res) if mode == 2 else None, out=out) is out
        assert torch.equal(out, got) and torch.equal(xd.cpu(), k.x)


@gpu
@pytest.mark.parametrize("HW", THREE_PASS_HW)
def test_single_pass_agrees_with_three_pass(ops, HW):
    """The two routes to the same result, on the three-pass cases with fabricated statistics: twice APPLY_BOUND.  (Their
    references differ by the float32 rounding of the records, which the rstd |mean| term of the bound covers: the groups here
    are a few pixels long.)"""
    k = apply_case(5, HW)
    st = conv_stats(ops, k.records, k.S)
    for mode in (0, 1, 2):
        res = dev(k.res) if mode == 2 else None
        one = ops.instance_norm(dev(k.x), mode, res, stats=st)
        check_apply("single pass HW=%d mode %d" % (HW, mode), k, mode, one)
        three = ops.instance_norm(dev(k.x), mode, res)
        ref = apply64(k.x, k.mean_x, k.rstd_x, mode, k.res)
        within("single / three passes HW=%d mode %d" % (HW, mode), one, three.cpu().double(), 2.0 * apply_bound(ref, k.mean_x, k.rstd_x))
