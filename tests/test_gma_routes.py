"""Every arithmetic route of GMA's attention and global-motion aggregation (csrc/gma.hip with its two dispatchers
gma_aggregate_conv / gma_aggregate_s16_impl, on the packs of csrc/conv_pack.hip) against float64 references written HERE:
softmax_j(scale * q_i . k_j) and fmap + gamma * attn @ v, plain torch on the CPU.

Routes (restated by att_route / agg_route below, pinned to the sources by test_host_thresholds_are_the_ones_restated_here):
    A1 gma_attention (fp32 gemm_atb + row softmax)          G1 gma_aggregate_kernel (float4 / scalar staging)
    A2 gma_attention_t, bf16x6 split GEMM + column softmax  G2 LDS-patch direct kernel, fp16 weights, split-K Z <= 4 / fill-based
    A3 gma_attention_t, fp32 gemm_atb + column softmax      G3 im2col kernel, fp16 operands, batched
    A4 gma_attention_s16 (register-only GEMM, S16 output)   G4 im2col bf16x6 / bf16x3, batched; G5 one launch per item (ragged P)
                                                            G6 G4 with B = 1 and Kpad >= 2048: im2col split-K
                                                            G7 gma_aggregate_s16 (in-register / two-pass pack, channel-block scatter)

Error model.  No tolerance is a constant taken from what the kernels return; each case computes its yardstick from the
reference, on its own inputs, at run time:
    E32      max |.| error of the SAME formula evaluated by torch in float32 on the CPU, against float64;
    E_split  max |.| error, against float64, of a float64 evaluation of the route's DESIGNED operand arithmetic (exact sums):
               fp32 routes (A1, A3, G1): 0;
               f16x3 (G2, G3, G7): w = fp32(v * gamma), scaled per row by 2^k so that the row maximum lies in [2^10, 2^11),
                 the attention times 2^ACCFLOW_F16_ASHIFT, both split as fp16 hi + lo, products hi.hi + hi.lo + lo.hi kept
                 (G7: the attention operand IS the stored S16 pair, only v is split); A4: q 2^4 and fp32(k scale 2^4) likewise;
               bf16x6 (A2, G4, G5, G6): 3 bf16 terms per operand, the 6 products t_a + t_b <= 2 of conv2d_bf16s_kernel.h
                 (A2: k carries fp32(1 / sqrt(D)) before its split); bf16x3: 2 terms, products 00, 01, 10.
    gate     max |got - ref64| <= MARGIN (E32 + E_split), MARGIN = 4; A4's stored output adds the S16 storage term
             2^-22 a + 2^-29 per element (outside the margin).
MARGIN = 4 covers what differs from the CPU float32 run: the GPU's summation order (32-deep matrix-core blocks, up to 8
split-K partial sums), expf differences of a couple of ulp, FMA contraction - the cushion tests/test_gru_state.py uses.
One-hot attention (a permutation): the reference is fmap + gamma * v[:, :, perm], exact to two roundings, gated at
4 eps (|fmap| + |gamma v|) + E_split per element.

An aggregation case that tests a route in isolation takes its attention from the CPU: the float64 softmax rounded ONCE to
float32 (for G7: the value of its S16 split, (hi + lo) / 2^4), so an aggregation failure is not blamed on the attention.
One chained case per mode (A2 -> G2, A2 -> G5, A4 -> G7) runs on top of that.

Input classes (conditions asserted on the CPU): diffuse (q, k = randn * 0.05; every weight < 2^-7, which needs P > 128;
fmap scaled by 2^-6 so that the residual add does not set the yardstick - as in every case of a bf16 route), mid (randn * 1.5), peaked (randn * 2.7 with one
key aligned to one query so that max |logit| > 30 and a row maximum > 0.99 hold at every P), one-hot (aggregation only),
huge-logit (attention only: q = c k, max |logit| > 200).  v: randn with one row scaled by 2^-9, one element by 2^-14, one
all-zero row.  gamma in {0.37, -0.5, 0}.  The teeth tests (CPU) show that the gates are not vacuous: one dropped lo term
(bf16 routes: the second term) lands >= 8x over every mid / peaked aggregation gate, the third bf16 term of bf16x6 and
16-bit q / k over every gate (see test_aggregation_gate_has_teeth for why the third term cannot reach 8x).

Not covered: the environment switches read once per process (ACCFLOW_GMA_QK_SPLIT, ACCFLOW_DIRECT_KSPLIT,
ACCFLOW_IM2COL_KSPLIT), shapes past (64, 64) - hence the `chunk` loop of G4 (2^32-byte attention batches) and rows of
more than 16 384 elements (the two-pass pack by length) -, invalid arguments (tests/test_host_logic.py owns those).

Measured on the MI355X, 2026-10-18, f16x3 default mode, every case passing - largest error / gate per route:
    A1 0.32   A2 0.34   A3 0.34   A4 0.55   G1 0.55   G2 0.36   G3 0.45   G4 0.35   G5 0.37   G6 0.37
    G7 0.47 (fp32 output), 0.89 (S16 output, gate + storage term)   chained: A2 -> G2 0.18, A2 -> G5 0.16, A4 -> G7 0.11
Nobody had measured these ratios before; no gate, margin or input was chosen from them.  The teeth figures quoted at the
teeth tests are from the CPU.
"""
import functools
import math
import os

import pytest
import torch

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
MARGIN = 4.0
TEETH = 8.0
S16_REL, S16_ABS = 2.0 ** -22, 2.0 ** -29
ASHIFT = 4                      # ACCFLOW_F16_ASHIFT (include/accflow_hip.h; pinned below)
ASC = float(1 << ASHIFT)
DQK = 128                       # the estimator's dim_head: the attention of every aggregation case is built at D = 128
GAMMAS = (0.37, -0.5, 0.0)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def dev(t):
    return t.cuda()


def cdiv(a, b):
    return -(-a // b)


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------
# the host's dispatch, restated; test_host_thresholds_are_the_ones_restated_here pins it to the sources

DIR_TH, DIR_TW = 4, 32
ROWS16_REG = 8


def kpad(k):
    return cdiv(k, 32) * 32


def fill_z(nb):
    """The part count (<= 8) with the best fill of whole rounds of the 768 workgroup slots."""
    best, Z = 0.0, 1
    for z in range(1, 9):
        fill = (nb * z) / (cdiv(nb * z, 768) * 768)
        if fill > best + 0.03:
            best, Z = fill, z
    return Z


def direct_split(cout, h, w):
    """launch_conv_direct's split-K for the aggregation (kws = 8 * cout * P floats): (branch, Z, Z * nout == kws_elems)."""
    P = h * w
    tc = 2 if cout > 64 else 1
    nb = cdiv(w, DIR_TW) * cdiv(h, DIR_TH) * cdiv(cout, 2 * tc * 32)
    nchunk = cdiv(P, 16)
    branch, Z = "none", 1
    if nchunk >= 256 and nb < 700:
        branch, Z = "fill", fill_z(nb)
    elif nb < 320:
        branch, Z = "small", min(cdiv(512, nb), 4, nchunk // 2)
    Z = max(min(Z, 8), 1)
    return branch, Z, Z == 8


def direct_tail_cut(cout, h, w):
    """accflow_launch_conv_direct cuts Cout = 128 m + (1..64) in two launches - unless a split-K workspace comes with a small grid."""
    nb = cdiv(w, DIR_TW) * cdiv(h, DIR_TH) * cdiv(cout, 128)
    return cout > 128 and 0 < cout % 128 <= 64 and not nb < 320


def im2col_split(B, D, P):
    """launch_conv_bf16s on the per-item packs (64-pixel tiles; 128- or 64-channel tiles): split-K parts."""
    if B != 1 or kpad(P) < 2048:
        return 1
    nb = cdiv(P, 64) * cdiv(D, 128 if D > 64 else 64)
    return min(fill_z(nb), 8) if nb < 700 else 1


def pack_rows16_inreg(P):
    return cdiv(P, 16) * 2 <= ROWS16_REG * 256 and P % 4 == 0


def att_route(entry, mode, D, scale, P):
    """(The split GEMM of A2 is a convolution with P output rows, and accflow_conv2d_f32 has split kernels for more than 32
    rows only: up to 32 pixels take gemm_atb in every mode.)"""
    if entry == "i":
        return "A1"
    if entry == "s16":
        return "A4"
    return "A2" if mode != "f32" and P > 32 and abs(f32(f32(scale) * f32(math.sqrt(D))) - 1.0) < 1e-6 else "A3"


def agg_route(entry, mode, B, D, h, w):
    """-> (route, arithmetic, detail).  entry: "i" = gma_aggregate, "t" = gma_aggregate_t, "s16" = gma_aggregate_s16 (B = the
    n items that share one attention)."""
    P = h * w
    if entry == "i":
        return "G1", "f32", "float4" if P % 4 == 0 else "scalar"
    if entry == "s16":
        return "G7", "f16x3_s16", ("inreg" if pack_rows16_inreg(P) else "twopass",) + direct_split(B * D, h, w)
    if mode == "f16x3" and B == 1 and P >= 16:
        return "G2", "f16x3", direct_split(D, h, w)
    if P % 64 == 0:
        Z = im2col_split(B, D, P)
        if mode == "f16x3":
            return "G3", "f16x3", Z
        return ("G6" if Z > 1 else "G4"), mode, Z
    return "G5", ("bf16x6" if mode == "f16x3" else mode), 1


def test_host_thresholds_are_the_ones_restated_here():
    """The route every case asserts comes from the functions above; they are the host code's only while these lines stand in
    the sources, so a changed threshold fails here instead of moving the coverage silently."""
    def src(*p):
        return open(os.path.join(ROOT, *p)).read()
    csrc = ("accflow_amd", "csrc")
    assert "#define ACCFLOW_F16_ASHIFT %d\n" % ASHIFT in src("include", "accflow_hip.h")
    assert "constexpr int DIR_TH = 4, DIR_TW = 32," in src(*csrc, "conv_tiles.h")
    gma = src(*csrc, "gma.hip")
    assert "if (split_ok && mode != ACCFLOW_CONV_F32 && ws && P > 32 && fabsf(scale * sqrtf((float)D) - 1.0f) < 1e-6f) {" in gma
    assert "ACCFLOW_CONV_BF16X6, 0, nullptr, st, nullptr, nullptr);" in gma            # the split route is bf16x6 in every mode
    assert "const bool vec = (P & 3) == 0;" in gma
    assert "for (int i = threadIdx.x; i < n; i += 256)" in gma                           # row softmax: 256-stride passes
    assert "constexpr int U = 8;" in gma and gma.count("for (int j = wave; j < P; j += 16 * U) {") == 2
    assert "hipLaunchKernelGGL(col_softmax16_kernel, dim3(cdiv(P, 64), B), dim3(1024), 0, st, attnT, P);" in gma
    assert "if (mode == ACCFLOW_CONV_F32) return 1;" in gma
    conv, pack = src(*csrc, "conv2d.hip"), src(*csrc, "conv_pack.hip")
    assert "if (mode == ACCFLOW_CONV_F16X3 && B == 1 && P >= 16) {" in gma
    assert "const bool f16 = mode == ACCFLOW_CONV_F16X3 && (P % 64) == 0;" in gma
    assert "if (mode == ACCFLOW_CONV_F16X3 && !f16) mode = ACCFLOW_CONV_BF16X6;" in gma
    assert "if (P % 64 == 0) {" in gma and "if (D <= 32) return 1;" in gma
    assert "if (conv_plan_direct(d, D > 64 ? 2 : 1, false, p)) return 1;" in gma
    assert "if (conv_plan_direct(d, Cout > 64 ? 2 : 1, false, p)) return 1;" in gma
    assert gma.count("return accflow_launch_conv_direct(d, p, st);") + conv.count("return accflow_launch_conv_direct(d, p, st);") == 3
    assert "d.kws = kws; d.kws_elems = 8LL * D * P;" in gma and "d.kws = kws; d.kws_elems = 8LL * Cout * P;" in gma
    assert "if (B == 1) { d.kws = kws; d.kws_elems = 8LL * D * P; }" in gma
    assert "constexpr int ROWS16_REG = %d;" % ROWS16_REG in pack
    assert "const bool inreg = nchunk <= ROWS16_REG * 256 && !(Cin & 3);" in pack
    # the routing thresholds have one home, the plan unit: one split-K rule and one tail-split rule for every kernel family
    plan = src(*csrc, "conv_plan.cpp")
    assert "return (K + 31) / 32 * 32;" in plan
    assert "return plan_im2col(d, d.Cout > 64 ? 2 : 1, 1, want_stats, true, p);" in plan     # per-item packs: 64-pixel tiles
    assert "const int nchunk = (d.C0 + d.C1 + 15) / 16;" in plan
    assert "p.Z = conv_split_k(d, want_stats, nb, nchunk >= 256, sw.direct_ksplit, nchunk);" in plan
    assert "p.Z = conv_split_k(d, want_stats, nb, d.Kpad >= 2048, conv_switches_get().im2col_ksplit, 0);" in plan
    assert "if (!d.kws || want_stats || d.e0_fmt || d.split_c0) return 1;" in plan
    assert "if (deep && nb < 700) {" in plan and "} else if (nchunk > 0 && nb < 320) {" in plan
    for line in ("Z = (int)((512 + nb - 1) / nb);", "if (Z > 4) Z = 4;", "if (Z > nchunk / 2) Z = nchunk / 2;",
                 "if (Z > 1 && (long long)Z * nout > d.kws_elems) Z = (int)(d.kws_elems / nout);",
                 "const long long nb = (long long)d.B * tiles * cdiv(d.Cout, 2 * tc * 32);",
                 "const long long nb = (long long)cdiv((long long)d.B * OHW, BP) * cdiv(d.Cout, 2 * tc * 32);"):
        assert line in plan, line
    assert "if (d.Cout > 128 && d.Cout % 128 > 0 && d.Cout % 128 <= 64 && pointwise && !want_stats && !d.cb && !(d.kws && nb128 < 320))" in plan
    assert "(long long)d.B * cdiv(d.OW, DIR_TW) * cdiv(d.OH, DIR_TH) * cdiv(d.Cout, 128));" in plan
    assert plan.count("if (fill > best + 0.03) { best = fill; Z = z; }") == 1
    direct = src(*csrc, "conv2d_direct.hip")
    bf = src(*csrc, "conv2d_bf16s_kernel.h")
    moved = [src(*csrc, f) for f in ("conv_small.hip", "corr_volume.hip", "gma_alt.hip")]   # (what conv2d.hip held until the split)
    corr_gemm = src(*csrc, "corr_gemm.hip")
    moved += [src(*csrc, "conv_ksplit.hip"), corr_gemm, src(*csrc, "gma_attn.hip")]         # (... and conv2d_direct.hip until its own)
    for text in [conv, gma, pack, direct, bf, src(*csrc, "conv2d_s16m.hip")] + moved:       # ... and no launcher decides any of it again
        assert "fill > best" not in text and "< 320" not in text and "< 700" not in text and "getenv(\"ACCFLOW_DIRECT" not in text
    # the products the split kernels keep: a = weights, b = activations, terms (2,0) (0,2) (1,1) only with three terms
    for line in ("c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2][tc], b[0][tp], c, 0, 0, 0);",
                 "c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][tc], b[2][tp], c, 0, 0, 0);",
                 "c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][tc], b[1][tp], c, 0, 0, 0);",
                 "c = s_mfma<F16>(a[NT == 3 ? 1 : 1][tc], b[0][tp], c);", "c = s_mfma<F16>(a[0][tc], b[1][tp], c);",
                 "c = s_mfma<F16>(a[0][tc], b[0][tp], c);"):
        assert bf.count(line) == 1, line
    assert "constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};" in corr_gemm


# ------------------------------------------------------------------------------------------------
# seeded inputs (shared by the CPU checks and the GPU cases)

CLASSES = ("diffuse", "mid", "peaked")
QK_STD = {"diffuse": 0.05, "mid": 1.5, "peaked": 2.7}


def _seed(*key):
    s = 17
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % 1000003
    return s


def make_qk(cls, B, D, h, w, scale=None):
    """(B, 2 D, h, w) float32: q = [:, :D], k = [:, D:].  The classes are distributions of the LOGITS: with a scale other than
    D^-1/2, q is multiplied by D^-1/2 / scale so that the logits are those of the class."""
    if scale is not None:
        qk = make_qk(cls, B, D, h, w).clone()
        qk[:, :D] *= D ** -0.5 / scale
        return qk
    P = h * w
    g = gen(_seed("qk", cls, B, D, h, w))
    if cls == "huge":                       # q = c k: the diagonal logit is c |k_i|^2 / sqrt(D); c puts the largest at 250
        k = torch.randn(B, D, P, generator=g)
        c = 250.0 * math.sqrt(D) / float((k * k).sum(1).max())
        return torch.cat([k * c, k], 1).view(B, 2 * D, h, w).contiguous()
    qk = torch.randn(B, 2 * D, P, generator=g) * QK_STD[cls]
    if cls == "peaked":                     # key (3 b + 1) % P lines up with query (5 b + 2) % P: that logit is 40
        for b in range(B):
            q = qk[b, :D, (5 * b + 2) % P]
            qk[b, D:, (3 * b + 1) % P] = q * (40.0 * math.sqrt(D) / float((q * q).sum()))
    return qk.view(B, 2 * D, h, w).contiguous()


def logits64(qk, D, scale):
    B = qk.shape[0]
    q, k = qk[:, :D].reshape(B, D, -1).double(), qk[:, D:].reshape(B, D, -1).double()
    return torch.einsum("bdi,bdj->bij", q, k) * float(scale)


def softmax64(qk, D, scale):
    """[b][i][j] = softmax_j(scale * q_i . k_j), float64."""
    return torch.softmax(logits64(qk, D, scale), dim=2)


def softmax32(qk, D, scale):
    """The same formula by torch in float32 on the CPU (the E32 yardstick)."""
    B = qk.shape[0]
    q, k = qk[:, :D].reshape(B, D, -1), qk[:, D:].reshape(B, D, -1)
    return torch.softmax(torch.matmul(q.transpose(1, 2), k) * f32(scale), dim=2)


def make_v(B, R, P, seed):
    """randn with one row scaled by 2^-9, one element by 2^-14 and one all-zero row (per item)."""
    v = torch.randn(B, R, P, generator=gen(seed))
    v[:, 5 % R] *= 2.0 ** -9
    v[:, 11 % R, P // 2] *= 2.0 ** -14
    v[:, 17 % R] = 0.0
    return v


@functools.lru_cache(maxsize=3)
def agg_attention(cls, B, h, w):
    """The attention operand of an isolated aggregation case, [b][i][j] float32: the float64 softmax at D = 128 rounded
    once; one-hot: a permutation matrix (and its permutation)."""
    P = h * w
    if cls == "onehot":
        perm = torch.stack([torch.randperm(P, generator=gen(_seed("perm", b, h, w))) for b in range(B)])
        a = torch.zeros(B, P, P)
        a.scatter_(2, perm[:, :, None], 1.0)
        return a, perm
    return softmax64(make_qk(cls, B, DQK, h, w), DQK, DQK ** -0.5).float(), None


# ------------------------------------------------------------------------------------------------
# float64 evaluations of the designed operand arithmetic


def split_f16(x32):
    """fp32 -> fp16 hi, lo (as float64): hi = fp16(x), lo = fp16(x - hi), the kernels' split."""
    hi = x32.half()
    lo = (x32 - hi.float()).half()
    return hi.double(), lo.double()


def split_bf16(x32, n):
    terms, r = [], x32.clone()
    for _ in range(n):
        b = r.bfloat16()
        terms.append(b.double())
        r = r - b.float()
    return terms


def s16_value(x32):
    """What an S16 tensor holds for x: (hi + lo) / 2^ASHIFT (exact in fp32), and the pair."""
    hi, lo = split_f16(x32 * ASC)
    return ((hi + lo) / ASC).float(), hi, lo


def row_scaled_weights(v32, gamma):
    """conv_row_scale16_kernel / conv_pack_rows16_kernel: w = fp32(v * gamma) * 2^k, k per row from the row maximum of |v|
    times |gamma| (fp32) so that it lies in [2^10, 2^11); -> (w32 scaled, 2^-k as float64 (B, R, 1))."""
    g = torch.tensor(gamma, dtype=torch.float32)
    m = v32.abs().amax(dim=2) * g.abs()
    _, e = torch.frexp(m)
    k = torch.where((m > 0) & (m < 3.0e38), (11 - e).clamp(-100, 100), torch.zeros_like(e))
    sc = torch.pow(torch.tensor(2.0, dtype=torch.float64), k.double())[:, :, None]
    return ((v32 * g).double() * sc).float(), 1.0 / sc


def mm(wterm, aterm):
    """sum_j w[b][r][j] a[b][i][j] in float64."""
    return torch.matmul(wterm, aterm.transpose(1, 2))


def agg_emulations(arith, attn32, v32, gamma, a16=None):
    """{name: fmap-less result (B, R, P) float64}: "design" and the weakened forms the teeth tests use."""
    if arith == "f32":
        return {"design": float(f32(gamma)) * mm(v32.double(), attn32.double())}
    if arith in ("f16x3", "f16x3_s16"):
        w, inv = row_scaled_weights(v32, gamma)
        wh, wl = split_f16(w)
        ah, al = a16 if arith == "f16x3_s16" else split_f16(attn32 * ASC)
        hh, hl, lh = mm(wh, ah), mm(wh, al), mm(wl, ah)
        s = inv / ASC
        return {"design": (hh + hl + lh) * s, "no attention lo": (hh + lh) * s, "no weight lo": (hh + hl) * s}
    n = 3 if arith == "bf16x6" else 2
    g = torch.tensor(gamma, dtype=torch.float32)
    wt, at = split_bf16(v32 * g, n), split_bf16(attn32, n)
    if n == 3:
        return {"design": mm(wt[0], at[0] + at[1] + at[2]) + mm(wt[1], at[0] + at[1]) + mm(wt[2], at[0]),
                "no third term": mm(wt[0] + wt[1], at[0] + at[1]), "no second term": mm(wt[0], at[0])}
    return {"design": mm(wt[0], at[0] + at[1]) + mm(wt[1], at[0]), "no second term": mm(wt[0], at[0])}


def att_emulations(route, qk, D, scale):
    """{name: attention [b][i][j] float64}: the route's designed logits, and 16-bit operands (2 bf16 terms each)."""
    B = qk.shape[0]
    q, k = qk[:, :D].reshape(B, D, -1), qk[:, D:].reshape(B, D, -1)

    def dots(qt, kt):
        return torch.einsum("bdi,bdj->bij", qt, kt)
    q2, k2 = split_bf16(q, 2), split_bf16(k, 2)
    out = {"16-bit operands": torch.softmax(dots(q2[0] + q2[1], k2[0] + k2[1]) * float(scale), dim=2)}
    if route in ("A1", "A3"):
        out["design"] = softmax64(qk, D, scale)
    elif route == "A2":       # conv_pack_kmajor_kernel: k * cscale, cscale = 1.0f / sqrtf(D), then 3 terms; q: 3 terms in the K loop
        cs = torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(D), dtype=torch.float32))
        kt, qt = split_bf16(k * cs, 3), split_bf16(q, 3)
        out["design"] = torch.softmax(dots(qt[0] + qt[1] + qt[2], kt[0]) + dots(qt[0] + qt[1], kt[1]) + dots(qt[0], kt[2]), dim=2)
    else:                     # A4: fp16 hi + lo of q 2^4 and of k (scale 2^4)
        qh, ql = split_f16(q * ASC)
        kh, kl = split_f16(k * torch.tensor(f32(scale) * ASC, dtype=torch.float32))
        out["design"] = torch.softmax((dots(qh, kh) + dots(ql, kh) + dots(qh, kl)) / (ASC * ASC), dim=2)
    return out


# ------------------------------------------------------------------------------------------------
# the case tables

ATT_CASES = []     # (route, entry, mode, B, D, h, w, cls, scale); scale None = D^-1/2


def _att(route, entry, mode, B, D, hw, cls, scale=None):
    ATT_CASES.append((route, entry, mode, B, D, hw[0], hw[1], cls, scale))


def _cls_for(i, P, classes=CLASSES):
    ok = [c for c in classes if c != "diffuse" or P > 128]
    return ok[i % len(ok)]


_i = 0
for _D in (40, 64, 128):                                                    # A1: 9, 63, 300 (two 256-stride passes), 512
    for _hw in ((3, 3), (7, 9), (12, 25), (16, 32)):
        _att("A1", "i", None, 1, _D, _hw, _cls_for(_i, _hw[0] * _hw[1]))
        _i += 1
_att("A1", "i", None, 2, 128, (7, 9), "peaked")
_att("A1", "i", None, 1, 128, (7, 9), "huge")
# A2 / A3: 9 (fewer rows than the 16 waves), 63, 65 (one live lane in the second column block), 130 (second sweep iteration
# with 2 rows), 512; A3 is A2's shapes with another scale, and in f32 mode
_T_SHAPES = [(1, (3, 3), "mid"), (1, (7, 9), "peaked"), (1, (5, 13), "mid"), (1, (10, 13), "diffuse"), (1, (16, 32), "peaked"),
             (2, (7, 9), "mid"), (2, (16, 32), "diffuse"), (1, (10, 13), "huge")]
for _B, _hw, _c in _T_SHAPES:
    _att("A2" if _hw != (3, 3) else "A3", "t", "f16x3", _B, 128, _hw, _c)       # (<= 32 pixels: gemm_atb in every mode)
_att("A2", "t", "bf16x6", 1, 128, (5, 13), "peaked")
for _B, _hw, _c in _T_SHAPES:
    _att("A3", "t", "f16x3", _B, 128, _hw, _c, 0.05)
    _att("A3", "t", "f32", _B, 128, _hw, _c)
_i = 1
for _D in (32, 128):                                                        # A4: 16, 63, 130, 512; all classes
    for _hw in ((4, 4), (7, 9), (10, 13), (16, 32)):
        _att("A4", "s16", "f16x3", 1, _D, _hw, _cls_for(_i, _hw[0] * _hw[1]))
        _i += 1
for _c in CLASSES + ("huge",):
    _att("A4", "s16", "f16x3", 1, 128, (10, 13), _c)
_att("A4", "s16", "f16x3", 2, 128, (7, 9), "peaked")
_att("A4", "s16", "f16x3", 2, 32, (16, 32), "diffuse")

AGG_CASES = []     # (route, entry, mode, B, D, h, w, cls, gamma, sliced)


def _agg(route, entry, mode, B, D, hw, cls, gamma=0.37, sliced=False):
    c = (route, entry, mode, B, D, hw[0], hw[1], cls, gamma, sliced)
    if c not in AGG_CASES:
        AGG_CASES.append(c)


def _extras(route, entry, mode, B, D, hw, hw_big):
    """Per route: one-hot, gamma = 0 and < 0, the sliced operands, and the diffuse class at a shape of more than 128 pixels."""
    _agg(route, entry, mode, B, D, hw, "onehot")
    _agg(route, entry, mode, B, D, hw, "mid", 0.0)
    _agg(route, entry, mode, B, D, hw, "peaked", -0.5)
    _agg(route, entry, mode, B, D, hw, "mid", 0.37, True)
    _agg(route, entry, mode, B, D, hw_big, "diffuse")


_i = 0
for _D in (40, 128, 200):                                                   # G1: 63 scalar staging, 36 float4 + slab tail, 130, 512
    for _hw in ((7, 9), (6, 6), (10, 13), (16, 32)):
        _agg("G1", "i", None, 2, _D, _hw, _cls_for(_i, _hw[0] * _hw[1]))
        _i += 1
_extras("G1", "i", None, 2, 128, (7, 9), (10, 13))
_i = 0
for _D in (64, 128, 192, 384, 768):                                         # G2: rows; 384 / 768 = stacked runs of 3 / 6 items
    for _hw in ((4, 4), (7, 9), (5, 40), (16, 32), (64, 64)):
        if _hw == (64, 64) and _D not in (128, 384):
            continue
        _agg("G2", "t", "f16x3", 1, _D, _hw, _cls_for(_i, _hw[0] * _hw[1], ("mid", "peaked")))
        _i += 1
_extras("G2", "t", "f16x3", 1, 128, (7, 9), (5, 40))
_agg("G2", "t", "f16x3", 1, 384, (16, 32), "diffuse")
_agg("G5", "t", "f16x3", 1, 128, (3, 3), "mid")                             # f16x3, B = 1, P < 16: the ragged route
_agg("G5", "t", "f16x3", 1, 128, (3, 3), "peaked", -0.5)
for _B, _hw, _c in ((2, (8, 8), "mid"), (3, (8, 8), "peaked"), (2, (16, 32), "peaked"), (3, (16, 32), "mid")):
    _agg("G3", "t", "f16x3", _B, 128, _hw, _c)
    _agg("G4", "t", "bf16x6", _B, 128, _hw, _c)
_extras("G3", "t", "f16x3", 2, 128, (8, 8), (16, 32))
_extras("G4", "t", "bf16x6", 2, 128, (8, 8), (16, 32))
_agg("G4", "t", "bf16x3", 2, 128, (8, 8), "mid")
_agg("G4", "t", "bf16x6", 1, 128, (16, 32), "mid")                          # B = 1 below Kpad = 2048: no im2col split-K
for _hw, _c in (((7, 9), "mid"), ((10, 13), "peaked")):
    _agg("G5", "t", "bf16x6", 2, 128, _hw, _c)
    _agg("G5", "t", "f16x3", 2, 128, _hw, _c)                               # f16x3, B > 1, ragged: falls back to bf16x6 per item
_extras("G5", "t", "bf16x6", 2, 128, (7, 9), (10, 13))
_agg("G6", "t", "bf16x6", 1, 128, (32, 64), "mid")                          # Kpad = 2048: im2col split-K
_agg("G6", "t", "bf16x6", 1, 128, (32, 64), "peaked", -0.5)
_agg("G6", "t", "bf16x6", 1, 128, (32, 64), "diffuse")
_agg("G6", "t", "bf16x6", 1, 128, (32, 64), "onehot")
_agg("G6", "t", "bf16x6", 1, 128, (32, 64), "mid", 0.0, True)
_i = 0
for _n in (1, 2, 3, 6):                                                     # G7: 16, 63 (two-pass pack), 512 (in-register pack)
    for _D in (32, 128):
        for _hw in ((4, 4), (7, 9), (16, 32)):
            _agg("G7", "s16", "f16x3", _n, _D, _hw, _cls_for(_i, _hw[0] * _hw[1]))
            _i += 1
_extras("G7", "s16", "f16x3", 2, 128, (7, 9), (16, 32))
_extras("G7", "s16", "f16x3", 3, 32, (16, 32), (16, 32))

CHAIN_CASES = [     # (attention route, aggregation route, attention entry, mode, B, D, h, w, cls)
    ("A2", "G2", "t", "f16x3", 1, 128, 7, 9, "mid"),
    ("A2", "G5", "t", "bf16x6", 2, 128, 7, 9, "peaked"),
    ("A4", "G7", "s16", "f16x3", 2, 128, 7, 9, "mid"),
]


def case_id(c):
    return "-".join("x".join(map(str, x)) if isinstance(x, tuple) else str(x) for x in c)


# ------------------------------------------------------------------------------------------------
# the models: reference, yardsticks and gate of a case (CPU; cached - the GPU case and the CPU checks share them)


@functools.lru_cache(maxsize=None)
def att_model(case):
    route, entry, mode, B, D, h, w, cls, scale = case
    qk = make_qk(cls, B, D, h, w, scale)
    scale = D ** -0.5 if scale is None else scale
    ref = softmax64(qk, D, scale)
    emu = att_emulations(route, qk, D, scale)
    e32 = float((softmax32(qk, D, scale).double() - ref).abs().max())
    esplit = float((emu["design"] - ref).abs().max())
    gate = MARGIN * (e32 + esplit) + ((S16_REL * ref + S16_ABS) if route == "A4" else 0.0)
    weak = float(((emu["16-bit operands"] - ref).abs() / gate).max())
    return {"ref": ref, "e32": e32, "esplit": esplit, "gate": gate, "weak": weak, "scale": scale,
            "max_logit": float(logits64(qk, D, scale).abs().max())}


def agg_inputs(case):
    """attention [b][i][j] float32 (B items, or the one shared by G7's n items), v, fmap (B, D, P), the permutation, S16 pair."""
    route, entry, mode, B, D, h, w, cls, gamma, sliced = case
    P = h * w
    attn, perm = agg_attention(cls, 1 if entry == "s16" else B, h, w)
    a16 = None
    if entry == "s16":
        attn, hi, lo = s16_value(attn)
        a16 = (hi, lo)
    g = _seed("agg", B, D, h, w, cls)
    v = make_v(B, D, P, g)
    # (the residual add must not set the yardstick where the operand error under test is small: the diffuse class, and the
    # bf16 routes, whose third term carries 2^-17 of an operand)
    small = cls == "diffuse" or agg_route(entry, mode, B, D, h, w)[1].startswith("bf16")
    fmap = torch.randn(B, D, P, generator=gen(g + 1)) * (2.0 ** -6 if small else 1.0)
    return attn, v, fmap, perm, a16


@functools.lru_cache(maxsize=None)
def agg_model(case):
    """Only small tensors are kept (the P x P attention is rebuilt by agg_inputs, itself cached for the last shapes)."""
    route, entry, mode, B, D, h, w, cls, gamma, sliced = case
    attn, v, fmap, perm, a16 = agg_inputs(case)
    _, arith, _ = agg_route(entry, mode, B, D, h, w)
    if entry == "s16":                         # n items x D rows of ONE GEMM against the shared attention
        v1, f1 = v.reshape(1, B * D, -1), fmap.reshape(1, B * D, -1)
    else:
        v1, f1 = v, fmap
    ref = f1.double() + float(f32(gamma)) * mm(v1.double(), attn.double())
    e32 = float(((f1 + f32(gamma) * torch.matmul(v1, attn.transpose(1, 2))).double() - ref).abs().max())
    emu = {k: f1.double() + x for k, x in agg_emulations(arith, attn, v1, gamma, a16).items()}
    esplit = float((emu["design"] - ref).abs().max())
    if cls == "onehot":
        gv = float(f32(gamma)) * torch.gather(v1.double(), 2, perm.expand(v1.shape[0], -1)[:, None, :].expand_as(v1))
        assert torch.equal(ref, f1.double() + gv)
        gate = MARGIN * EPS * (f1.double().abs() + gv.abs()) + esplit
    else:
        gate = torch.full_like(ref, MARGIN * (e32 + esplit))
    weak = {k: float(((x - ref).abs() / gate.clamp_min(1e-300)).max()) for k, x in emu.items() if k != "design"}
    shape = (B, D, h, w)
    return {"ref": ref.view(shape), "gate": gate.view(shape), "e32": e32, "esplit": esplit, "weak": weak, "arith": arith}


# ------------------------------------------------------------------------------------------------
# CPU: input conditions, coverage, teeth


@pytest.mark.parametrize("cls", CLASSES + ("huge",))
@pytest.mark.parametrize("shape", [(1, 128, 3, 3), (2, 128, 7, 9), (1, 128, 10, 13), (1, 32, 16, 32), (1, 128, 16, 32), (1, 128, 32, 64)])
def test_attention_inputs_meet_the_conditions(cls, shape):
    B, D, h, w = shape
    P = h * w
    if cls == "diffuse" and P <= 128:
        assert _cls_for(0, P) != "diffuse"                       # (softmax weights of <= 128 pixels cannot all lie below 2^-7)
        return
    qk = make_qk(cls, B, D, h, w)
    lg = logits64(qk, D, D ** -0.5)
    a = torch.softmax(lg, dim=2)
    assert bool(torch.isfinite(a).all())
    if cls == "diffuse":
        assert float(a.max()) < 2.0 ** -7
    elif cls == "peaked":
        assert float(lg.abs().max()) > 30 and float(a.amax(dim=2).max()) > 0.99
    elif cls == "huge":
        assert float(lg.abs().max()) > 200
        q, k = qk[:, :D].reshape(B, D, -1), qk[:, D:].reshape(B, D, -1)
        lg32 = torch.matmul(q.transpose(1, 2), k) * f32(D ** -0.5)
        assert bool(torch.isinf(torch.exp(lg32)).any())          # an unshifted exp overflows in float32
        assert bool(torch.isfinite(softmax32(qk, D, D ** -0.5)).all())


def test_diffuse_cases_have_more_than_128_pixels():
    for c in ATT_CASES:
        assert c[7] != "diffuse" or c[5] * c[6] > 128, c
    for c in AGG_CASES:
        assert c[7] != "diffuse" or c[5] * c[6] > 128, c
        if c[7] == "diffuse":
            assert float(agg_attention("diffuse", 1, c[5], c[6])[0].max()) < 2.0 ** -7


def test_aggregation_operands_meet_the_conditions():
    v = make_v(2, 128, 63, 5)
    assert bool((v[:, 17] == 0).all()) and float(v[:, 5].abs().max()) < 2.0 ** -6 and float(v[0, 11, 31].abs()) < 2.0 ** -11
    a, perm = agg_attention("onehot", 2, 7, 9)
    assert bool((a.sum(1) == 1).all()) and bool((a.sum(2) == 1).all()) and not torch.equal(perm[0], torch.arange(63))
    assert not torch.equal(a[0], a[0].t())                       # (a transposed operand shows)
    x = torch.randn(1000, generator=gen(3)) * 2.0 ** -9
    y, hi, lo = s16_value(x)
    assert float((y.double() - x.double()).abs().max()) <= S16_REL * float(x.abs().max()) + S16_ABS
    w, inv = row_scaled_weights(v, -0.5)
    m = w.abs().amax(dim=2)
    assert bool(((m >= 1024) & (m < 2048) | (m == 0)).all()) and bool((m[:, 17] == 0).all())
    assert torch.equal((w.double() * inv).float(), v * torch.tensor(-0.5))


def test_cases_cover_the_route_table():
    """Every row of the route table, both split-K branches of G2 (and the exactly-full workspace), both branches of
    conv_pack_rows16_kernel, the one-tile kernel and the declined 192-row cut, every class and gamma per route."""
    for c in ATT_CASES:
        route, entry, mode, B, D, h, w, cls, scale = c
        assert att_route(entry, mode, D, D ** -0.5 if scale is None else scale, h * w) == route, c
    assert {c[0] for c in ATT_CASES} == {"A1", "A2", "A3", "A4"}
    assert {(c[2], c[8]) for c in ATT_CASES if c[0] == "A3"} == {("f16x3", 0.05), ("f32", None), ("f16x3", None)}
    assert [c[5:7] for c in ATT_CASES if c[0] == "A3" and c[2:4] == ("f16x3", 1) and c[8] is None] == [(3, 3)]
    pix = {r: {c[5] * c[6] for c in ATT_CASES if c[0] == r} for r in ("A1", "A2", "A3", "A4")}
    assert pix["A1"] == {9, 63, 300, 512} and pix["A2"] | {9} == pix["A3"] == {9, 63, 65, 130, 512} and pix["A4"] == {16, 63, 130, 512}
    assert {c[4] for c in ATT_CASES if c[0] == "A1"} == {40, 64, 128} and {c[4] for c in ATT_CASES if c[0] == "A4"} == {32, 128}
    for r in ("A1", "A2", "A3", "A4"):
        assert 2 in {c[3] for c in ATT_CASES if c[0] == r}
        assert {c[7] for c in ATT_CASES if c[0] == r} == set(CLASSES) | {"huge"}
    assert {(c[3], c[5] * c[6]) for c in ATT_CASES if c[0] == "A2"} >= {(2, 63), (2, 512)}
    seen = {}
    for c in AGG_CASES:
        route, entry, mode, B, D, h, w, cls, gamma, sliced = c
        got, arith, detail = agg_route(entry, mode, B, D, h, w)
        assert got == route, c
        seen.setdefault(route, []).append((c, arith, detail))
    assert set(seen) == {"G1", "G2", "G3", "G4", "G5", "G6", "G7"}
    for r, items in seen.items():
        assert {c[7] for c, _, _ in items} == set(CLASSES) | {"onehot"}, r
        assert {c[8] for c, _, _ in items} == set(GAMMAS), r
        assert any(c[9] for c, _, _ in items), r
    assert {d for _, _, d in seen["G1"]} == {"float4", "scalar"} and {c[4] for c, _, _ in seen["G1"]} == {40, 128, 200}
    g2 = {(c[4], c[5], c[6]): d for c, _, d in seen["G2"]}
    assert g2[(128, 4, 4)] == ("small", 1, False) and g2[(128, 16, 32)] == ("small", 4, False)
    assert g2[(128, 64, 64)] == ("fill", 8, True) and g2[(384, 64, 64)] == ("fill", 8, True)
    assert {k[0] for k in g2} == {64, 128, 192, 384, 768} and {k[0] for k in g2 if k[1:] == (64, 64)} == {128, 384}
    assert not direct_tail_cut(192, 64, 64) and direct_tail_cut(192, 128, 160)      # (the cut needs >= 160 pixel tiles)
    assert {(c[3], c[5] * c[6]) for c, _, _ in seen["G3"]} >= {(2, 64), (3, 64), (2, 512), (3, 512)}
    assert {a for _, a, _ in seen["G3"]} == {"f16x3"} and {a for _, a, _ in seen["G4"]} == {"bf16x6", "bf16x3"}
    assert {(c[3], c[5] * c[6]) for c, a, _ in seen["G4"] if a == "bf16x6"} >= {(2, 64), (3, 64), (2, 512), (3, 512), (1, 512)}
    assert {(c[2], c[3], c[5] * c[6]) for c, _, _ in seen["G5"]} >= {("bf16x6", 2, 63), ("bf16x6", 2, 130), ("f16x3", 1, 9), ("f16x3", 2, 63)}
    assert {a for _, a, _ in seen["G5"]} == {"bf16x6"}
    assert all(c[3] == 1 and c[5] * c[6] == 2048 and d == 8 for c, _, d in seen["G6"])
    assert {d[0] for _, _, d in seen["G7"]} == {"inreg", "twopass"}
    assert {(c[3], c[4]) for c, _, _ in seen["G7"]} >= {(n, D) for n in (1, 2, 3, 6) for D in (32, 128)}
    assert {c[5] * c[6] for c, _, _ in seen["G7"]} == {16, 63, 512}
    for ar, gr, entry, mode, B, D, h, w, cls in CHAIN_CASES:
        assert att_route(entry, mode, D, D ** -0.5, h * w) == ar and agg_route(entry, mode, B, D, h, w)[0] == gr
    assert max(c[5] * c[6] for c in AGG_CASES + ATT_CASES) == 4096


TEETH_AGG = [c for c in AGG_CASES if c[7] in ("mid", "peaked") and c[8] != 0.0 and c[0] != "G1"]
TEETH_ATT = [c for c in ATT_CASES if c[7] in ("mid", "peaked")]


@pytest.mark.parametrize("case", TEETH_AGG, ids=case_id)
def test_aggregation_gate_has_teeth(case):
    """One dropped lo term of the f16x3 design, or the second bf16 term of a bf16 design, lands >= 8x over the gate.
    The third bf16 term of bf16x6 is held to LESS than the 8x the issue of this file asks for: it must exceed the gate.  Two
    bf16 terms hold an operand to 2^-18 (round to nearest, twice), the gate of a 64- to 2048-term fp32 sum is MARGIN E32 ~
    2^-21 of the result.  Measured on the CPU: 1.66 - 5.4 gates over the bf16x6 cases of 63 to 2048 pixels (11 and 19 at 9
    pixels), with or without the residual; 59 - 353 for either fp16 lo term, 99.9 - 7964 for the second bf16 term.  Inputs
    built for it do not get there either: positive v and attention with every element moved (by < 2^-15 of itself) to the
    neighbour whose third term is the largest positive one, so that all residuals add up, reach 4.5 - 7.8 gates at 63 / 64
    pixels and 2.8 - 5.4 at 512 / 2048.  So a G4 / G5 / G6 kernel that lost its third term would show as 1.7 to 5 gates,
    not 8: the gates of these routes are that much less sharp than the f16x3 ones."""
    m = agg_model(case)
    assert m["weak"], case
    for name, r in m["weak"].items():
        assert r >= (1.0 if name == "no third term" else TEETH), (name, m["weak"], m["e32"], m["esplit"])


@pytest.mark.parametrize("case", TEETH_ATT, ids=case_id)
def test_attention_gate_has_teeth(case):
    """q and k rounded to 16 bits (2 bf16 terms) exceed the gate."""
    m = att_model(case)
    assert m["weak"] > 1.0, (m["weak"], m["e32"], m["esplit"])


# ------------------------------------------------------------------------------------------------
# GPU


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as o
    assert torch.cuda.is_available()          # (every case names its mode: nothing here depends on the process default)
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


SENT = -777.25
SENT16 = 0x7B5A7B5A
MODE = {"f16x3": 4, "bf16x6": 3, "bf16x3": 2}


def run_attention(ops, entry, mode, qk, D, scale):
    """-> attention [b][i][j] on the device (fp32)."""
    B, _, h, w = qk.shape
    P = h * w
    if entry == "i":
        return ops.gma_attention(qk, D, scale)[:, 0]
    if entry == "s16":
        return ops.gma_attention_s16(qk, D, scale).to_float().view(B, P, P).transpose(1, 2)
    with ops.conv_mode(mode):
        return ops.gma_attention_t(qk, D, scale).transpose(1, 2)


@gpu
@pytest.mark.parametrize("case", ATT_CASES, ids=case_id)
def test_attention_route_vs_float64(ops, case):
    route, entry, mode, B, D, h, w, cls, scale = case
    m = att_model(case)
    assert att_route(entry, mode, D, m["scale"], h * w) == route
    assert bool(torch.isfinite(m["ref"]).all()) and (cls != "huge" or m["max_logit"] > 200)
    ops.guard_tripped()
    got = run_attention(ops, entry, mode, dev(make_qk(cls, B, D, h, w, scale)), D, m["scale"])
    within("%s %s" % (route, case_id(case[2:])), got, m["ref"], m["gate"])
    assert not ops.guard_tripped()


def run_aggregation(ops, case, attn, v, fmap, a16=None):
    """-> (out (B, D, h, w), extra checks done); attn [b][i][j] on the device."""
    route, entry, mode, B, D, h, w, cls, gamma, sliced = case
    P = h * w
    g = dev(torch.tensor([gamma]))
    v, fmap = v.view(B, D, h, w), fmap.view(B, D, h, w)
    if entry == "s16":
        return run_aggregation_s16(ops, case, a16, v, fmap, g)
    buf = torch.full((B, D + 5, h, w), SENT, device="cuda") if sliced else None
    out = buf[:, 3:3 + D] if sliced else None
    if entry == "i":
        got = ops.gma_aggregate(attn[:, None].contiguous(), v, fmap, g, out=out)
    else:
        at = attn.transpose(1, 2).contiguous()
        got = ops.gma_aggregate_t(at, v, fmap, g, out=out, mode=MODE[mode])
    if sliced:
        assert bool((buf[:, :3] == SENT).all()) and bool((buf[:, 3 + D:] == SENT).all()), "wrote outside the out slice"
    return got


def run_aggregation_s16(ops, case, a16, v, fmap, g):
    """out only, out16 only and both; residual and outputs as channel slices of sentinel-filled buffers when sliced; the S16
    copy equals ops.to_s16(out) bit for bit."""
    route, entry, mode, n, D, h, w, cls, gamma, sliced = case
    C3 = 3 * D if sliced else D
    c0 = D if sliced else 0
    big = torch.full((n, C3, h, w), SENT, device="cuda")                                   # [fmap | out | sentinel]
    fbuf = torch.full((n, C3, h, w), SENT, device="cuda")
    fbuf[:, :D] = fmap
    O16 = (C3 + 7) // 8
    outs = []
    for want32, want16 in ((True, False), (False, True), (True, True)):
        big.fill_(SENT)
        s16 = ops.S16(torch.full((n, O16, 2, h, w, 4), SENT16, dtype=torch.int32, device="cuda"), C3)
        o16 = s16.channels(c0, c0 + D)
        ops.gma_aggregate_s16(a16.ptr(), v, fbuf[0].data_ptr(), fbuf.stride(0), g,
                              big[0, c0:].data_ptr() if want32 else None, big.stride(0) if want32 else 0,
                              o16.ptr() if want16 else None, s16.bs if want16 else 0, n, D, h, w)
        if want32:
            outs.append(big[:, c0:c0 + D].clone())
            assert bool((big[:, :c0] == SENT).all()) and bool((big[:, c0 + D:] == SENT).all()), "wrote outside the out slice"
        else:
            assert bool((big == SENT).all())
        if want16:
            outs.append(o16.to_float())
            keep = torch.ones(O16, dtype=torch.bool, device="cuda")
            keep[c0 // 8:(c0 + D) // 8] = False
            assert bool((s16.data[:, keep] == SENT16).all()), "wrote outside the out16 slice"
        else:
            assert bool((s16.data == SENT16).all())
        if want32 and want16:
            assert torch.equal(o16.data, ops.to_s16(outs[-2].contiguous()).data)
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
    assert bool((fbuf[:, :D] == fmap).all())
    return outs[0], outs[1]


@gpu
@pytest.mark.parametrize("case", AGG_CASES, ids=case_id)
def test_aggregation_route_vs_float64(ops, case):
    route, entry, mode, B, D, h, w, cls, gamma, sliced = case
    assert agg_route(entry, mode, B, D, h, w)[0] == route
    m = agg_model(case)
    attn, v, fmap, perm, pair = agg_inputs(case)
    tag = "%s %s" % (route, case_id(case[2:]))
    ops.guard_tripped()
    a16 = None
    if entry == "s16":      # the uploaded S16 attention: channels j over the pixels i, and its value is the reference's operand
        a16 = ops.S16.from_float(dev(attn[0].t().contiguous().view(1, h * w, h, w)))
        assert torch.equal(a16.to_float().view(h * w, h * w).t().cpu(), attn[0])
    got = run_aggregation(ops, case, dev(attn), dev(v), dev(fmap), a16)
    if entry == "s16":
        got, got16 = got
        within(tag + " out16", got16, m["ref"], m["gate"] + S16_REL * m["ref"].abs() + S16_ABS)
    within(tag, got, m["ref"], m["gate"])
    if gamma == 0.0:
        assert torch.equal(got.cpu(), fmap.view(B, D, h, w)), tag + ": gamma = 0 must return fmap"
    assert not ops.guard_tripped(), tag + ": range guard"


@gpu
def test_im2col_route_refuses_rows_it_has_no_kernel_for(ops):
    """Up to 32 rows, accflow_conv2d_f32 has fp32 kernels only, and the aggregation packs v as split terms: the im2col route
    (here bf16x6, B = 2) returns an error before anything is launched; the direct kernel (f16x3, B = 1) takes 32 rows."""
    refused = ("G4", "t", "bf16x6", 2, 32, 8, 8, "mid", 0.37, False)
    attn, v, fmap, _, _ = agg_inputs(refused)
    with pytest.raises(RuntimeError):
        run_aggregation(ops, refused, dev(attn), dev(v), dev(fmap))
    taken = ("G2", "t", "f16x3", 1, 32, 8, 8, "mid", 0.37, False)
    assert agg_route(*taken[1:7])[0] == "G2"
    m = agg_model(taken)
    attn, v, fmap, _, _ = agg_inputs(taken)
    ops.guard_tripped()
    within("G2 " + case_id(taken[2:]), run_aggregation(ops, taken, dev(attn), dev(v), dev(fmap)), m["ref"], m["gate"])
    assert not ops.guard_tripped()


@gpu
@pytest.mark.parametrize("case", CHAIN_CASES, ids=case_id)
def test_attention_into_aggregation_vs_float64(ops, case):
    """The device's own attention feeds the aggregation: E32 and E_split are those of the chain (the designed attention,
    rounded to fp32 / to its S16 value, through the designed aggregation)."""
    ar, gr, entry, mode, B, D, h, w, cls = case
    P, gamma, scale = h * w, 0.37, D ** -0.5
    qk = make_qk(cls, B, D, h, w)
    seed = _seed("chain", case_id(case))
    v = make_v(B, D, P, seed)
    fmap = torch.randn(B, D, P, generator=gen(seed + 1))
    nb = 1 if entry == "s16" else B                              # G7: the n = B items share attention 0
    v1, f1 = (v.reshape(1, B * D, P), fmap.reshape(1, B * D, P)) if entry == "s16" else (v, fmap)
    a64 = softmax64(qk, D, scale)[:nb]
    ref = f1.double() + float(f32(gamma)) * mm(v1.double(), a64)
    e32 = float(((f1 + f32(gamma) * torch.matmul(v1, softmax32(qk, D, scale)[:nb].transpose(1, 2))).double() - ref).abs().max())
    a_design = att_emulations(ar, qk, D, scale)["design"][:nb].float()
    pair = None
    if entry == "s16":
        a_design, hi, lo = s16_value(a_design)
        pair = (hi, lo)
    arith = agg_route(entry, mode, B, D, h, w)[1]
    esplit = float((f1.double() + agg_emulations(arith, a_design, v1, gamma, pair)["design"] - ref).abs().max())
    ops.guard_tripped()
    g = dev(torch.tensor([gamma]))
    dv, df = dev(v).view(B, D, h, w), dev(fmap).view(B, D, h, w)
    if entry == "s16":
        a16 = ops.gma_attention_s16(dev(qk), D, scale)
        got = torch.empty(B, D, h, w, device="cuda")
        ops.gma_aggregate_s16(a16.ptr(), dv, df.data_ptr(), df.stride(0), g, got.data_ptr(), got.stride(0), None, 0, B, D, h, w)
    else:
        with ops.conv_mode(mode):
            at = ops.gma_attention_t(dev(qk), D, scale)
            got = ops.gma_aggregate_t(at, dv, df, g)
    within("chain %s->%s %s" % (ar, gr, case_id(case[3:])), got, ref.view(B, D, h, w), MARGIN * (e32 + esplit))
    assert not ops.guard_tripped()
