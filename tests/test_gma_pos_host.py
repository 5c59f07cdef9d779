"""GMA's positional attention (csrc/gma_pos.hip, args.position_only / args.position_and_content) on the CPU: the float64
restatement that tests/test_gma_pos.py holds the kernels to, pinned against the reference's own attention
(tests/golden/gma_pos_c1.npz); the argument checks of the new C entries; and the teeth of the GPU gates.

The restatement.  Query pixel i = (x, y), key pixel j = (u, v) of the h x w grid, M = max_pos_size, q = scale * qk[:, :D],
Eh / Ew the embedding weights (2M - 1, D):
    sim_pos[i, j] = A[i, u] + Bw[i, v],    A[i, u] = <q_i, Eh[u - x + M - 1]>,    Bw[i, v] = <q_i, Ew[v - y + M - 1]>
    position_and_content: softmax_j(<q_i, k_j> + sim_pos[i, j]);   position_only: softmax_j(sim_pos[i, j]).

Error model (tests/test_gma_routes.py's, restated): gate = MARGIN (E32 + E_split), MARGIN = 4; E32 = the same formula by
torch in float32 on the CPU against float64 (for position_only on the j-major routes the formula is the separable form
softmax_u(A) softmax_v(Bw) those kernels compute, see att_model; the float64 reference is the joint softmax everywhere); E_split = a float64 evaluation of the route's designed operand arithmetic
against float64 - 0 for the tables (fp32 operands, fp32 FMA), for the fp32 GEMM routes and for position_only, that file's
bf16x6 model (k times fp32(1 / sqrt(D)) then 3 bf16 terms, q 3 terms, the 6 products t_a + t_b <= 2) for the split content
scores; an S16 output adds the storage term 2^-22 a + 2^-29 per element.  Every yardstick is computed at run time from the
reference; none comes from what the kernels return.

Routes (pos_route below): P1 gma_attention_pos (row-major; fp32 GEMM), P2 gma_attention_pos_t with the split GEMM
(a split mode, P > 32, scale = D^-1/2), P3 gma_attention_pos_t with the fp32 GEMM (f32 mode, or P <= 32), P4
gma_attention_pos_s16 (the scores of P2 / P3 by the same rule, S16 output).  With position_only there is no GEMM: P2 and
P3 are then the same code, run in both modes all the same.

Input classes: mid, peaked, diffuse (tests/test_gma_routes.py's q, k; embeddings randn), posdom (q, k = randn * 0.3,
embeddings scaled so that max |positional logit| = 35 while every content logit stays below 1), zero (embeddings 0:
position_and_content must meet the content-only reference).

Teeth measured on the CPU: the smallest ratio of a mistake's error to the gate, over every non-zero case and both modes,
is about 1e5 (test_index_mistakes_land_over_the_gate prints each).
"""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 4.0
TEETH = 8.0
S16_REL, S16_ABS = 2.0 ** -22, 2.0 ** -29
ASC = 16.0                      # 2^ACCFLOW_F16_ASHIFT
D = 128
MAXPOS = 160
SHAPES = ((3, 3), (7, 9), (5, 13), (13, 10), (16, 32))
CLASSES = ("mid", "peaked", "diffuse", "posdom", "zero")
QK_STD = {"diffuse": 0.05, "mid": 1.5, "peaked": 2.7, "posdom": 0.3, "zero": 1.5}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _seed(*key):
    s = 17
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % 1000003
    return s


# ------------------------------------------------------------------------------------------------
# the restatement, float64 and float32


def rel_index(n, M, flip=False, off=0):
    """[a, b] = b - a + M - 1: the embedding row of key coordinate b for query coordinate a."""
    i = torch.arange(n)
    d = i.view(1, -1) - i.view(-1, 1)
    return (-d if flip else d) + M - 1 + off


def pos_tables(q, Eh, Ew, M, mistake=None):
    """q (B, D, h, w) already scaled -> A (B, P, h), Bw (B, P, w), in q's dtype."""
    B, _, h, w = q.shape
    flip, off = mistake == "delta x - u", -1 if mistake == "M - 2" else 0
    eh = (Ew if mistake == "Ew for height" else Eh)[rel_index(h, M, flip, off)]      # [x, u, d]
    ew = Ew[rel_index(w, M, flip, off)]                                               # [y, v, d]
    A = torch.einsum("bdxy,xud->bxyu", q, eh).reshape(B, h * w, h)
    Bw = torch.einsum("bdxy,yvd->bxyv", q, ew).reshape(B, h * w, w)
    return A, Bw


def pos_logits(A, Bw):
    B, P, h = A.shape
    return (A[:, :, :, None] + Bw[:, :, None, :]).reshape(B, P, P)


def content_logits(qs, k):
    B, Dq = qs.shape[:2]
    return torch.einsum("bdi,bdj->bij", qs.reshape(B, Dq, -1), k.reshape(B, Dq, -1))


def attention(qk, Eh, Ew, M, scale, content, dtype=torch.float64, mistake=None, design=None):
    """[b, i, j]; dtype float32: the E32 evaluation (scale rounded to fp32, as the kernels receive it).  design = "bf16x6":
    the content logits by the split GEMM's operand arithmetic (float64 sums)."""
    Dq = qk.shape[1] // 2
    sc = f32(scale) if dtype == torch.float32 else float(scale)
    qs = qk[:, :Dq].to(dtype) * sc
    lg = pos_logits(*pos_tables(qs, Eh.to(dtype), Ew.to(dtype), M, mistake))
    if content:
        if design == "bf16x6":
            lg = lg + bf16x6_logits(qk, Dq)
        else:
            lg = content_logits(qs, qk[:, Dq:].to(dtype)) + lg
    return torch.softmax(lg, dim=2)


def attention_separable(qk, Eh, Ew, M, scale, dtype=torch.float64):
    """position_only as the j-major kernels evaluate it: softmax_j(A[u] + Bw[v]) = softmax_u(A) softmax_v(Bw)."""
    B, C2, h, w = qk.shape
    sc = f32(scale) if dtype == torch.float32 else float(scale)
    A, Bw = pos_tables(qk[:, :C2 // 2].to(dtype) * sc, Eh.to(dtype), Ew.to(dtype), M)
    return (torch.softmax(A, 2)[:, :, :, None] * torch.softmax(Bw, 2)[:, :, None, :]).reshape(B, h * w, h * w)


def split_bf16(x32, n):
    terms, r = [], x32.clone()
    for _ in range(n):
        b = r.bfloat16()
        terms.append(b.double())
        r = r - b.float()
    return terms


def bf16x6_logits(qk, Dq):
    """tests/test_gma_routes.py's model of the split QK GEMM: k * fp32(1 / sqrt(D)) then 3 bf16 terms, q 3 terms."""
    B = qk.shape[0]
    q, k = qk[:, :Dq].reshape(B, Dq, -1), qk[:, Dq:].reshape(B, Dq, -1)
    cs = torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(Dq), dtype=torch.float32))
    kt, qt = split_bf16(k * cs, 3), split_bf16(q, 3)

    def dots(a, b):
        return torch.einsum("bdi,bdj->bij", a, b)
    return dots(qt[0] + qt[1] + qt[2], kt[0]) + dots(qt[0] + qt[1], kt[1]) + dots(qt[0], kt[2])


def s16_value(x32):
    """What an S16 tensor holds for x: (hi + lo) / 2^ASHIFT, and the pair (float64)."""
    hi = (x32 * ASC).half()
    lo = (x32 * ASC - hi.float()).half()
    return ((hi.double() + lo.double()) / ASC).float(), hi.double(), lo.double()


# ------------------------------------------------------------------------------------------------
# seeded inputs and the case table (shared with tests/test_gma_pos.py)


def make_qk(cls, B, h, w):
    """tests/test_gma_routes.py's make_qk at D = 128 (posdom, zero: plain randn of their std)."""
    P = h * w
    qk = torch.randn(B, 2 * D, P, generator=gen(_seed("qk", cls, B, D, h, w))) * QK_STD[cls]
    if cls == "peaked":                     # key (3 b + 1) % P lines up with query (5 b + 2) % P: that content logit is 40
        for b in range(B):
            q = qk[b, :D, (5 * b + 2) % P]
            qk[b, D:, (3 * b + 1) % P] = q * (40.0 * math.sqrt(D) / float((q * q).sum()))
    return qk.view(B, 2 * D, h, w).contiguous()


def make_emb(cls, B, h, w, M=MAXPOS):
    """(Eh, Ew) float32 (2M - 1, D)."""
    g = gen(_seed("emb", cls, h, w, M))
    Eh, Ew = torch.randn(2 * M - 1, D, generator=g), torch.randn(2 * M - 1, D, generator=g)
    if cls == "zero":
        return torch.zeros_like(Eh), torch.zeros_like(Ew)
    if cls == "posdom":
        q = make_qk(cls, B, h, w)[:, :D].double() * D ** -0.5
        s = 35.0 / float(pos_logits(*pos_tables(q, Eh.double(), Ew.double(), M)).abs().max())
        return (Eh * s).contiguous(), (Ew * s).contiguous()
    return Eh, Ew


def pos_route(entry, mode, P):
    if entry == "i":
        return "P1"
    split = mode != "f32" and P > 32            # (scale is D^-1/2 in every case)
    if entry == "s16":
        return "P4"
    return "P2" if split else "P3"


def design_of(entry, mode, P, content):
    return "bf16x6" if content and entry != "i" and mode != "f32" and P > 32 else None


ATT_CASES = []     # (route, entry, mode, content, B, h, w, cls)
_n = 0
for _entry, _mode in (("i", "f16x3"), ("t", "f16x3"), ("t", "bf16x6"), ("t", "f32"), ("s16", "f16x3")):
    for _content in (True, False):
        for _hw in SHAPES:                  # every shape, the classes in turn (diffuse needs more than 128 pixels)
            _ok = [c for c in CLASSES if c != "diffuse" or _hw[0] * _hw[1] > 128]
            ATT_CASES.append((pos_route(_entry, _mode, _hw[0] * _hw[1]), _entry, _mode, _content, 1 + _n % 2, _hw[0], _hw[1],
                              _ok[_n % len(_ok)]))
            _n += 1
        if _mode == "bf16x6":
            continue
        for _cls in CLASSES:                # every class at 130 pixels (two column blocks, the tail octet)
            _c = (pos_route(_entry, _mode, 130), _entry, _mode, _content, 1 + _n % 2, 13, 10, _cls)
            _n += 1
            if not any(x[:4] + x[5:] == _c[:4] + _c[5:] for x in ATT_CASES):
                ATT_CASES.append(_c)


def case_id(c):
    return "-".join(str(x) for x in c)


@functools.lru_cache(maxsize=None)
def att_model(case):
    route, entry, mode, content, B, h, w, cls = case
    qk = make_qk(cls, B, h, w)
    Eh, Ew = make_emb(cls, B, h, w)
    scale = D ** -0.5
    ref = attention(qk, Eh, Ew, MAXPOS, scale, content)
    # E32 is the float32 evaluation of the formula the route computes: the joint softmax, except for position_only on the
    # j-major routes, which multiply the two table softmaxes (three roundings more per element than the joint form has when
    # its logits happen to be exact - the zero class -, fewer bits lost in the exponent's argument when they are large)
    a32 = (attention(qk, Eh, Ew, MAXPOS, scale, content, torch.float32) if content or entry == "i"
           else attention_separable(qk, Eh, Ew, MAXPOS, scale, torch.float32))
    e32 = float((a32.double() - ref).abs().max())
    design = design_of(entry, mode, h * w, content)
    esplit = float((attention(qk, Eh, Ew, MAXPOS, scale, content, design=design) - ref).abs().max()) if design else 0.0
    gate = MARGIN * (e32 + esplit) + ((S16_REL * ref + S16_ABS) if entry == "s16" else 0.0)
    return {"ref": ref, "e32": e32, "esplit": esplit, "gate": gate, "scale": scale}


# ------------------------------------------------------------------------------------------------
# the restatement against the reference's attention


def test_restatement_reproduces_the_reference_attention(golden):
    """tests/test_oracle_golden.py::test_gma_attention_aggregate's gates on gma_c1: rows atol 1e-6 + rtol 1e-3, row sums 1e-5."""
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks.gma.gma import RAFTGMA, gma_args
    g, c1 = golden("gma_pos_c1"), golden("gma_c1")
    sd = make_state_dict(RAFTGMA(gma_args(position_and_content=True)))
    inp = torch.relu(torch.from_numpy(c1["cnet"])[:, 128:]).double()
    qk = torch.nn.functional.conv2d(inp, sd["att.to_qk.weight"].double())
    Eh, Ew = sd["att.pos_emb.rel_height.weight"], sd["att.pos_emb.rel_width.weight"]
    assert tuple(Eh.shape) == (2 * MAXPOS - 1, D)
    for tag, content in (("po", False), ("pc", True)):
        a = attention(qk, Eh, Ew, MAXPOS, D ** -0.5, content).numpy()
        assert np.abs(a.sum(-1) - g[tag + "_attn_rowsum"][:, 0]).max() <= 1e-5
        rows = g[tag + "_attn_rows"]
        err = np.abs(a[:, g["attn_rows_sel"]] - rows)
        print("%s: rows max err %.2e" % (tag, err.max()))
        assert (err <= 1e-6 + 1e-3 * np.abs(rows)).all(), (tag, err.max())
    assert np.abs(g["po_attn_rows"] - g["pc_attn_rows"]).max() > 1e-3          # (the two modes are different attentions)


def test_separable_form_of_position_only():
    """softmax_j(A[u] + Bw[v]) = softmax_u(A) softmax_v(Bw)."""
    qk, (Eh, Ew) = make_qk("mid", 1, 6, 11), make_emb("mid", 1, 6, 11)
    sep = attention_separable(qk, Eh, Ew, MAXPOS, D ** -0.5)
    assert float((sep - attention(qk, Eh, Ew, MAXPOS, D ** -0.5, False)).abs().max()) < 1e-15


# ------------------------------------------------------------------------------------------------
# input conditions, coverage, teeth


@pytest.mark.parametrize("case", [c for c in ATT_CASES if c[1] == "t" and c[2] == "f16x3"], ids=case_id)
def test_inputs_meet_the_conditions(case):
    route, entry, mode, content, B, h, w, cls = case
    qk, (Eh, Ew) = make_qk(cls, B, h, w), make_emb(cls, B, h, w)
    q = qk[:, :D].double() * D ** -0.5
    pos = pos_logits(*pos_tables(q, Eh.double(), Ew.double(), MAXPOS))
    con = content_logits(q, qk[:, D:].double())
    assert bool(torch.isfinite(att_model(case)["ref"]).all())
    if cls == "posdom":
        assert float(pos.abs().max()) > 30 and float(con.abs().max()) < 1
    elif cls == "zero":
        assert float(pos.abs().max()) == 0
        want = torch.softmax(con, 2) if content else torch.full_like(con, 1.0 / (h * w))
        assert float((att_model(case)["ref"] - want).abs().max()) < 1e-15
    elif cls == "peaked":
        assert float(con.abs().max()) > 30
    elif cls == "diffuse":
        assert h * w > 128 and float(con.abs().max()) < 0.2


def test_cases_cover_routes_modes_shapes_and_classes():
    for c in ATT_CASES:
        assert pos_route(c[1], c[2], c[5] * c[6]) == c[0]
    assert {c[0] for c in ATT_CASES} == {"P1", "P2", "P3", "P4"}
    for route in ("P1", "P2", "P3", "P4"):
        for content in (True, False):
            mine = [c for c in ATT_CASES if c[0] == route and c[3] == content]
            assert {c[7] for c in mine} == set(CLASSES), (route, content)
            assert {c[4] for c in mine} == {1, 2}, (route, content)
            want = set(SHAPES) - ({(3, 3)} if route == "P2" else set())          # (<= 32 pixels: the fp32 GEMM in every mode)
            assert {(c[5], c[6]) for c in mine} >= (want if route != "P3" else {(3, 3), (13, 10)}), (route, content)
    assert {(c[5], c[6]) for c in ATT_CASES if c[1:3] == ("t", "f32")} == set(SHAPES)
    assert ("P3", "t", "f16x3") in {c[:3] for c in ATT_CASES if (c[5], c[6]) == (3, 3)}
    assert ("P2", "t", "bf16x6") in {c[:3] for c in ATT_CASES}


MISTAKES = ("Ew for height", "delta x - u", "M - 2")


@pytest.mark.parametrize("case", [c for c in ATT_CASES if c[7] != "zero"], ids=case_id)
def test_index_mistakes_land_over_the_gate(case):
    """The embedding table swapped for the height term, the delta taken as x - u (and y - v), the offset M - 2 instead of
    M - 1: each moves some probability by at least TEETH gates, in both modes, on the inputs of every GPU attention case
    (the zero-embedding class cannot show an index).  Smallest ratio measured on the CPU: see the printed figures."""
    route, entry, mode, content, B, h, w, cls = case
    m = att_model(case)
    qk, (Eh, Ew) = make_qk(cls, B, h, w), make_emb(cls, B, h, w)
    for mistake in MISTAKES:
        bad = attention(qk, Eh, Ew, MAXPOS, m["scale"], content, mistake=mistake)
        r = float(((bad - m["ref"]).abs() / m["gate"]).max())
        print("TEETH %s %s %.1f" % (case_id(case), mistake, r))
        assert r >= TEETH, (mistake, r, m["e32"], m["esplit"])


# ------------------------------------------------------------------------------------------------
# the C entries refuse bad arguments before any launch (no device is needed: nothing may reach the runtime)


def test_c_entries_reject_bad_arguments():
    from accflow_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)       # never dereferenced: every call below must return before a launch
    nul = ctypes.c_void_p(0)
    sc = D ** -0.5
    tables = lib.accflow_gma_pos_tables_f32
    for args in ((nul, p, p, p), (p, nul, p, p), (p, p, nul, p), (p, p, p, nul)):
        assert tables(*args, 1, D, 8, 8, MAXPOS, sc, nul) != 0
    assert tables(p, p, p, p, 1, D, MAXPOS + 1, 8, MAXPOS, sc, nul) != 0          # H > max_pos
    assert tables(p, p, p, p, 1, D, 8, MAXPOS + 1, MAXPOS, sc, nul) != 0          # W > max_pos
    assert tables(p, p, p, p, 1, D, 9, 8, 8, sc, nul) != 0 and tables(p, p, p, p, 1, D, 8, 9, 8, sc, nul) != 0
    for bad in ((0, D, 8, 8, MAXPOS), (1, 0, 8, 8, MAXPOS), (1, D, 0, 8, MAXPOS), (1, D, 8, 0, MAXPOS), (1, D, 8, 8, 0)):
        assert tables(p, p, p, p, *bad, sc, nul) != 0
    rowmajor = lib.accflow_gma_attention_pos_f32
    for args in ((nul, p, p), (p, nul, p), (p, p, nul)):
        assert rowmajor(*args, 1, 1, D, 8, 8, sc, nul) != 0
    assert rowmajor(p, p, p, 2, 1, D, 8, 8, sc, nul) != 0 and rowmajor(p, p, p, 1, 0, D, 8, 8, sc, nul) != 0
    jmajor = lib.accflow_gma_attention_pos_t
    assert jmajor(nul, p, p, nul, p, 4, 1, 1, D, 8, 8, sc, nul) != 0
    assert jmajor(p, nul, p, nul, p, 4, 1, 1, D, 8, 8, sc, nul) != 0
    assert jmajor(p, p, nul, nul, p, 4, 1, 1, D, 8, 8, sc, nul) != 0              # no output
    assert jmajor(p, p, p, p, p, 4, 1, 1, D, 8, 8, sc, nul) != 0                  # two outputs
    assert jmajor(p, p, nul, p, nul, 4, 1, 1, D, 8, 8, sc, nul) != 0              # S16 with content needs the score workspace
    assert jmajor(p, p, p, nul, p, 4, 2, 1, D, 8, 8, sc, nul) != 0 and jmajor(p, p, p, nul, p, 4, 1, 1, D, 0, 8, sc, nul) != 0
    ws = lib.accflow_gma_attention_pos_ws_bytes
    assert ws(D, 8, 8, 0, 0) == ws(D, 8, 8, 0, 1) == 16 * 64 * 4                  # position_only: no scores, one item's tables
    assert jmajor(p, p, p, nul, nul, 4, 0, 1, D, 8, 8, sc, nul) != 0              # ... which need the workspace
    assert ws(D, 8, 8, 1, 1) - ws(D, 8, 8, 1, 0) == 64 * 64 * 4                   # S16: the fp32 scores of ONE item


def test_modules_refuse_what_is_not_built():
    import argparse
    from accflow_amd.networks.gma.gma import gma_args
    from accflow_amd.networks.gma.modules import Attention
    assert vars(gma_args()) == dict(num_heads=1, mixed_precision=True, position_only=False, position_and_content=False)
    assert gma_args(position_only=True).position_only and gma_args(position_and_content=True).position_and_content
    x = torch.zeros(1, 128, 161, 4)
    for flags in (dict(position_only=True), dict(position_and_content=True)):
        att = Attention(args=gma_args(**flags), dim=128, heads=1, max_pos_size=160, dim_head=128)
        for fn in (att.forward, att.forward_t):
            with pytest.raises(ValueError, match="161.*160"):
                fn(x)
            with pytest.raises(ValueError, match="161.*160"):
                fn(x.transpose(2, 3))
        with pytest.raises(NotImplementedError):
            att.forward_alt(x)
    many = Attention(args=argparse.Namespace(position_only=True, position_and_content=False), dim=128, heads=2, max_pos_size=160,
                     dim_head=64)
    with pytest.raises(NotImplementedError):
        many.forward(torch.zeros(1, 128, 4, 4))
