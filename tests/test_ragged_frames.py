"""The estimators and AccFlow end to end at RAGGED frame sizes, against a float64 run of the project's own oracle.

Every other end-to-end forward of the suite runs at a size whose 1/8 grid has an even width and a pixel count that is a
multiple of 64, so the Python glue between the kernels (padded 128-pixel query blocks, pair-group cuts, gathers over
frame-major features, descriptor caches) had only seen sizes where padded and unpadded extents agree, and the branch of
RAFT._estimate_encoded for an odd W8 (no operand packs: pair-major features, ops.corr_volume_disp) was never taken.

Cases (frame -> h8 x w8, P = h8 * w8):
  A  64x64    ->  8x8,    P = 64    the pyramid's minimum (level 3 is 1x1); less than one 128-pixel query block
  B  104x136  -> 13x17,   P = 221   both odd; one full and one ragged query block; pyramid 13x17, 6x8, 3x4, 1x2
  C  120x144  -> 15x18,   P = 270   H8 odd, W8 even, no multiple of 8, below 64
  D  72x1032  ->  9x129,  P = 1161  W8 odd and above 128 (three 64-column target tiles, the last of one column); ten query blocks
  E  64x72    ->  8x9,    P = 72    minimum height with an odd W8

Routes.  RAFT.estimate_pairs (AccFlow's entry) correlates from per-frame operand packs where ops.corr_packs_supported holds
(W8 even: A, C) and per pair through accflow_corr_volume_disp_f32 otherwise (W8 odd: B, D, E).  RAFT.forward(image1, image2)
has no frame-major features to pack: it takes accflow_corr_volume_disp_f32 at every size (with W8 even on its direct GEMM, with
W8 odd on the one that pools from level 0).  Each estimator case therefore runs through BOTH entries, and the library entry
points each run called are recorded and asserted (`routes`).

Gate.  For every output, on the CPU: d32 = EPE(fp32 oracle, float64 oracle), got = EPE(product, float64 oracle), mean and max;
required got_mean <= 8 * d32_mean, got_max <= 8 * d32_max and got_mean <= 1e-3 px (the project's gate).  The factor: the f16x3
operands carry 22 significant bits against fp32's 24 (each product up to 4x coarser), the accumulators are fp32 in both, and the
kernels sum in other orders (tiles, split-K) than the oracle's fp32 convolutions (another 2x).  The stage checks apply the same
factor to the max abs error of the encoders, the correlation pyramid and one update-block call at B and D, so that a failure
of the end-to-end gate is pinned to a stage without a rerun.  The CPU tests at the end show that the gate rejects four
injected glue faults (a wrong ragged-tail pixel, a dropped target column, a shifted pool, a wrong gather index).

Measured on an MI355X, every figure printed by the tests themselves (run with -s)
(of the two entries, forward / estimate_pairs, the one with the larger ratio):
  run                      case   got mean / max [px]     d32 mean / max [px]     ratio mean / max
  raft                     A      6.7e-06 / 2.5e-05       5.7e-06 / 2.6e-05       1.18 / 0.99
  raft                     B      8.6e-06 / 3.3e-05       6.9e-06 / 3.2e-05       1.24 / 1.02
  raft                     C      7.8e-06 / 3.3e-05       5.8e-06 / 2.3e-05       1.34 / 1.40
  raft                     D      1.4e-05 / 8.6e-05       1.2e-05 / 8.6e-05       1.14 / 1.00
  gma                      A      2.0e-05 / 9.5e-05       1.9e-05 / 9.3e-05       1.03 / 1.03
  gma                      B      2.1e-05 / 1.6e-04       3.1e-05 / 1.6e-04       0.68 / 1.00
  gma                      C      3.6e-05 / 1.5e-04       2.2e-05 / 8.7e-05       1.62 / 1.76
  gma                      D      6.6e-05 / 3.8e-04       4.8e-05 / 2.7e-04       1.39 / 1.42
  raft flow_init           B      9.7e-06 / 4.6e-05       7.6e-06 / 3.1e-05       1.28 / 1.46
  gma flow_init            B      2.4e-05 / 1.7e-04       3.9e-05 / 2.9e-04       0.62 / 0.57
  raft alternate_corr      B      8.3e-06 / 3.2e-05       6.9e-06 / 3.2e-05       1.21 / 0.99
  raft alternate_corr      C      7.9e-06 / 3.6e-05       5.8e-06 / 2.3e-05       1.36 / 1.54
  gma alternate_attention  B      2.2e-05 / 1.6e-04       3.1e-05 / 1.6e-04       0.69 / 1.00
  gma alternate_attention  C      3.6e-05 / 1.5e-04       2.2e-05 / 8.7e-05       1.62 / 1.77
  raft bf16x6              B      9.0e-06 / 3.4e-05       6.9e-06 / 3.2e-05       1.31 / 1.05
  acc|raft out0            B      5.8e-06 / 9.1e-05       5.5e-06 / 8.5e-05       1.05 / 1.06
  acc|raft out1            B      6.8e-06 / 7.5e-05       5.2e-06 / 8.4e-05       1.31 / 0.89
  acc|raft out0            C      7.2e-06 / 7.8e-05       5.4e-06 / 7.4e-05       1.33 / 1.05
  acc|raft out1            C      6.7e-06 / 5.6e-05       4.7e-06 / 6.8e-05       1.42 / 0.82
  acc|raft out0            E      3.7e-06 / 2.6e-05       3.1e-06 / 2.1e-05       1.19 / 1.20
  acc|gma out0             B      9.4e-06 / 1.5e-04       7.9e-06 / 1.1e-04       1.19 / 1.32
  acc|gma out1             B      1.0e-05 / 2.1e-04       1.0e-05 / 1.7e-04       1.02 / 1.25
  acc|gma out0             C      9.5e-06 / 9.4e-05       6.2e-06 / 6.7e-05       1.53 / 1.41
  acc|gma out1             C      7.2e-06 / 5.4e-05       6.6e-06 / 7.8e-05       1.09 / 0.69
  acc|gma out0             E      5.6e-06 / 6.1e-05       4.3e-06 / 3.6e-05       1.32 / 1.69
Stage ratios (max abs error / the fp32 oracle's): B at most 1.62 (pyramid level 0), D at most 2.20 (update block net).  No output
needed the occlusion-threshold exclusion, no stage was recomputed in bf16x6, and every run took the route listed above.
"""
import pytest
import torch

from oracle import accflow_oracle as O

gpu = pytest.mark.gpu

ITERS = 12
FACTOR = 8.0
CASES = {"A": (64, 64), "B": (104, 136), "C": (120, 144), "D": (72, 1032), "E": (64, 72)}
SEEDS = {"A": 2101, "B": 2102, "C": 2103, "D": 2104, "E": 2105}
# (tag, frames per sample batch N): the estimator runs; (tag, frames, N): the AccFlow runs
ESTIMATOR_RUNS = [("A", 2), ("B", 1), ("C", 1), ("D", 1)]
ACCFLOW_RUNS = [("B", 4, 2), ("C", 4, 1), ("E", 3, 1)]

PACKED = ("accflow_corr_pack_f32", "accflow_corr_volume_disp_packed_f32")
PER_PAIR = "accflow_corr_volume_disp_f32"
ROW_MAJOR = ("accflow_corr_volume_f32", "accflow_corr_volume_split_f32")
VOLUMES = PACKED + (PER_PAIR,) + ROW_MAJOR
FUSED_LOOKUP = "accflow_corr_lookup_convc1_s16"
ALT_PYRAMID = "accflow_corr_alt_pyramid_f32"
ALT_LOOKUPS = ("accflow_corr_lookup_alt_f32", "accflow_corr_lookup_alt_s16")


def grid(tag):
    H, W = CASES[tag]
    return H // 8, W // 8


def dev(t):
    return t.cuda()


def maxerr(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


# ------------------------------------------------------------------------------------------------
# inputs, weights and the two oracle runs of a case (computed once per module, never modified)

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def frames(tag, n, N=1):
    """n normalised frames (N, 3, H, W) of case `tag`; sample s moves the texture of seed + s."""
    from accflow_amd.data.synthetic import make_sequence, normalize
    H, W = CASES[tag]
    return cached(("frames", tag, n, N), lambda: [normalize(f) for f in make_sequence(SEEDS[tag], n, H, W, batch=N)])


def pair(tag, N=1):
    fr = frames(tag, 2, N)
    return fr[1], fr[0]


def flow_init(tag, N=1):
    h8, w8 = grid(tag)
    return cached(("init", tag, N), lambda: 2.0 * torch.randn(N, 2, h8, w8, generator=torch.Generator().manual_seed(77)))


def weights(name):
    """(fp32 state_dict, float64 state_dict) of "raft" / "gma" / "acc|raft" / "acc|gma"."""
    def make():
        from accflow_amd.data.synthetic import make_state_dict
        from accflow_amd.networks import build_flow_estimator
        m = build_flow_estimator(name)
        if name.startswith("acc"):
            from accflow_amd.networks.AccFlow_ import AccFlow
            m = AccFlow(m)
        sd = make_state_dict(m)
        return sd, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return cached(("sd", name), make)


def estimator_refs(name, tag, N=1, init=False):
    """(float64 oracle flow, fp32 oracle flow) of the pair of case `tag`."""
    def make():
        sd, sd64 = weights(name)
        i1, i2 = pair(tag, N)
        fi = flow_init(tag, N) if init else None
        with torch.no_grad():
            r64 = O.raft_forward(sd64, i1.double(), i2.double(), ITERS, flow_init=None if fi is None else fi.double(),
                                 gma=(name == "gma"))
            r32 = O.raft_forward(sd, i1, i2, ITERS, flow_init=fi, gma=(name == "gma"))
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32
        return r64, r32
    return cached(("est", name, tag, N, init), make)


def accflow_refs(name, tag, n, N):
    def make():
        sd, sd64 = weights(name)
        fr = frames(tag, n, N)
        with torch.no_grad():
            r64 = O.accflow_forward(sd64, [f.double() for f in fr], iters=ITERS, gma=name.endswith("gma"))
            r32 = O.accflow_forward(sd, fr, iters=ITERS, gma=name.endswith("gma"))
        assert all(r.dtype == torch.float64 for r in r64)
        return r64, r32
    return cached(("acc", name, tag, n, N), make)


# ------------------------------------------------------------------------------------------------
# the gate


def gate(what, got, r64, r32):
    """-> (passes, figures).  Prints got, d32 and their ratios."""
    d_mean, d_max = O.epe(r32.double(), r64)
    g_mean, g_max = O.epe(got.detach().cpu().double(), r64)
    fig = dict(got_mean=g_mean, got_max=g_max, d32_mean=d_mean, d32_max=d_max,
               ratio_mean=g_mean / d_mean if d_mean else float("inf"), ratio_max=g_max / d_max if d_max else float("inf"))
    print("RAGGED %-44s got %.3e / %.3e  d32 %.3e / %.3e  ratio %.2f / %.2f" % (
        what, g_mean, g_max, d_mean, d_max, fig["ratio_mean"], fig["ratio_max"]))
    finite = bool(torch.isfinite(got).all())
    ok = finite and g_mean <= FACTOR * d_mean and g_max <= FACTOR * d_max and g_mean <= 1e-3
    return ok, fig


def assert_gate(what, got, r64, r32):
    assert tuple(got.shape) == tuple(r64.shape), (what, tuple(got.shape), tuple(r64.shape))
    assert bool(torch.isfinite(got).all()), (what, "not finite")
    ok, fig = gate(what, got, r64, r32)
    assert ok, (what, fig)


# ------------------------------------------------------------------------------------------------
# models on the device and the record of library entry points


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def model(name):
    def make():
        from accflow_amd.networks import build_flow_estimator
        m = build_flow_estimator(name)
        if name.startswith("acc"):
            from accflow_amd.networks.AccFlow_ import AccFlow
            m = AccFlow(m)
        m.load_state_dict(weights(name)[0], strict=True)
        return m.cuda().eval()
    return cached(("model", name), make)


@pytest.fixture
def routes(monkeypatch):
    """Names of the correlation / attention entry points of the kernel library in the order they are called."""
    from accflow_amd import _lib as L
    lib = L.load()
    called = []
    for name in L.SIGNATURES:
        if not name.startswith(("accflow_corr_", "accflow_gma_")) or name.endswith(("_bytes", "_elems", "_supported", "_kpad")):
            continue

        def wrapper(*args, _real=getattr(lib, name), _name=name):
            called.append(_name)
            return _real(*args)
        monkeypatch.setattr(lib, name, wrapper)
    return called


def check_routes(called, tag, entry, alt=False, fused=True):
    """entry: "pairs" (estimate_pairs, AccFlow) or "forward" (RAFT.forward)."""
    seen = set(called)
    w8 = grid(tag)[1]
    if alt:
        assert ALT_PYRAMID in seen and seen & set(ALT_LOOKUPS), (tag, entry, sorted(seen))
        assert not seen & set(VOLUMES), (tag, entry, sorted(seen))
        return
    if fused:
        assert FUSED_LOOKUP in seen, (tag, entry, sorted(seen))
    assert not seen & set(ROW_MAJOR), (tag, entry, sorted(seen))
    if entry == "pairs" and w8 % 2 == 0:
        assert set(PACKED) <= seen and PER_PAIR not in seen, (tag, entry, sorted(seen))
    else:
        assert PER_PAIR in seen and not seen & set(PACKED), (tag, entry, sorted(seen))


def run_both_entries(ops, m, routes, what, tag, N, refs, init=False, alt=False, fused=True):
    """The pair of case `tag` through RAFT.forward and through estimate_pairs: gate, routes, no bf16x6 retry."""
    i1, i2 = pair(tag, N)
    fi = dev(flow_init(tag, N)) if init else None
    r64, r32 = refs
    for entry in ("forward", "pairs"):
        del routes[:]
        ops.guard_report()
        if entry == "forward":
            out = m(dev(i1), dev(i2), iters=ITERS, flow_init=fi)
        else:
            out = m.estimate_pairs([dev(i1), dev(i2)], [(0, 1)], iters=ITERS, flow_init=fi)
        out = out.cpu()
        assert ops.guard_report() == [], (what, entry, "a stage was recomputed in bf16x6")
        check_routes(routes, tag, entry, alt=alt, fused=fused)
        assert_gate("%s %s %s" % (what, tag, entry), out, r64, r32)


# ------------------------------------------------------------------------------------------------
# estimators


@gpu
@pytest.mark.parametrize("name", ["raft", "gma"])
@pytest.mark.parametrize("tag,N", ESTIMATOR_RUNS)
def test_estimator_ragged(ops, routes, name, tag, N):
    run_both_entries(ops, model(name), routes, name, tag, N, estimator_refs(name, tag, N))


@gpu
@pytest.mark.parametrize("name", ["raft", "gma"])
def test_estimator_ragged_flow_init(ops, routes, name):
    run_both_entries(ops, model(name), routes, name + " flow_init", "B", 1, estimator_refs(name, "B", 1, init=True), init=True)


@gpu
@pytest.mark.parametrize("name", ["raft", "gma"])
def test_estimator_ragged_batch_of_two_equals_single_calls(ops, name):
    """B with N = 2 (two different pairs) against two single calls: 1e-4 px, test_estimator_c1_vs_golden_and_oracle's bound."""
    m = model(name)
    i1, i2 = pair("B", 2)
    both = m(dev(i1), dev(i2), iters=ITERS).cpu()
    for n in range(2):
        solo = m(dev(i1[n:n + 1]), dev(i2[n:n + 1]), iters=ITERS).cpu()
        assert maxerr(both[n:n + 1], solo) <= 1e-4, (name, n, maxerr(both[n:n + 1], solo))
    both = m.estimate_pairs([dev(i1), dev(i2)], [(0, 1)], iters=ITERS).cpu()
    for n in range(2):
        solo = m.estimate_pairs([dev(i1[n:n + 1]), dev(i2[n:n + 1])], [(0, 1)], iters=ITERS).cpu()
        assert maxerr(both[n:n + 1], solo) <= 1e-4, (name, "pairs", n, maxerr(both[n:n + 1], solo))


@gpu
@pytest.mark.parametrize("tag", ["B", "C"])
def test_raft_alternate_corr_ragged(ops, routes, tag):
    m = model("raft")
    m.args.alternate_corr = True
    try:
        run_both_entries(ops, m, routes, "raft alternate_corr", tag, 1, estimator_refs("raft", tag, 1), alt=True)
    finally:
        m.args.alternate_corr = False


@gpu
@pytest.mark.parametrize("tag", ["B", "C"])
def test_gma_alternate_attention_ragged(ops, routes, tag):
    m = model("gma")
    m.args.alternate_attention = True
    try:
        run_both_entries(ops, m, routes, "gma alternate_attention", tag, 1, estimator_refs("gma", tag, 1))
        assert "accflow_gma_attention_alt" in routes and "accflow_gma_aggregate_alt" in routes, sorted(set(routes))
        assert "accflow_gma_attention_s16" not in routes and "accflow_gma_aggregate_s16" not in routes, sorted(set(routes))
    finally:
        m.args.alternate_attention = False


@gpu
def test_raft_bf16x6_ragged(ops, routes):
    """B in the mode a guard-tripped stage is recomputed in (fp32 activations: the lookup is a launch of its own there)."""
    with ops.conv_mode("bf16x6"):
        run_both_entries(ops, model("raft"), routes, "raft bf16x6", "B", 1, estimator_refs("raft", "B", 1), fused=False)
    assert FUSED_LOOKUP not in routes and "accflow_corr_lookup_disp_f32" in routes, sorted(set(routes))


# ------------------------------------------------------------------------------------------------
# AccFlow


@gpu
@pytest.mark.parametrize("name", ["acc|raft", "acc|gma"])
@pytest.mark.parametrize("tag,n,N", ACCFLOW_RUNS)
def test_accflow_ragged(ops, routes, name, tag, n, N):
    """B: 10 items (two stream groups), C: 5 items (a 2 / 3 cut), E: 3 items (one group)."""
    mdl = model(name)
    mdl.ofe_iters = ITERS
    r64, r32 = accflow_refs(name, tag, n, N)
    ops.guard_report()
    outs = [o.cpu() for o in mdl(images=[dev(f) for f in frames(tag, n, N)])]
    assert ops.guard_report() == [], (name, tag, "a stage was recomputed in bf16x6")
    check_routes(routes, tag, "pairs")
    assert len(outs) == n - 2
    for k, o in enumerate(outs):
        assert_gate("%s %s out%d" % (name, tag, k), o, r64[k], r32[k])


# ------------------------------------------------------------------------------------------------
# stage by stage (localises a failure of the gates above)


def stage_bound(what, got, want64, want32):
    """max abs error of a stage <= 8 x the fp32 oracle's."""
    e32 = maxerr(want32, want64)
    err = maxerr(got, want64)
    print("RAGGED stage %-36s err %.3e  fp32 oracle %.3e  ratio %.2f" % (what, err, e32, err / e32 if e32 else float("inf")))
    assert bool(torch.isfinite(got).all()), what
    assert err <= FACTOR * e32, (what, err, e32)


@gpu
@pytest.mark.parametrize("tag", ["B", "D"])
def test_stages_ragged(ops, tag):
    from accflow_amd.networks.raft.corr import CorrBlock
    m = model("raft")
    sd, sd64 = weights("raft")
    i1, i2 = pair(tag)
    fi = flow_init(tag)
    with torch.no_grad():
        both = torch.cat([i1, i2], 0)
        f64, f32 = O.basic_encoder(both.double(), sd64, "fnet", "instance"), O.basic_encoder(both, sd, "fnet", "instance")
        c64, c32 = O.basic_encoder(i1.double(), sd64, "cnet", "batch"), O.basic_encoder(i1, sd, "cnet", "batch")
    ops.guard_report()
    f1, f2 = m.fnet([dev(i1), dev(i2)])
    stage_bound(tag + " fnet fmap1", f1, f64[:1], f32[:1])
    stage_bound(tag + " fnet fmap2", f2, f64[1:], f32[1:])
    stage_bound(tag + " cnet", m.cnet(dev(i1)), c64, c32)
    # the later stages from the float64 oracle's state, rounded to fp32 once: product and fp32 oracle see the same inputs
    x1, x2 = f64[:1].float(), f64[1:].float()
    with torch.no_grad():
        p64, p32 = O.corr_pyramid(x1.double(), x2.double()), O.corr_pyramid(x1, x2)
    got = CorrBlock(dev(x1), dev(x2)).corr_pyramid
    assert len(got) == 4
    for l in range(4):
        assert tuple(got[l].shape) == tuple(p64[l].shape), (tag, l, tuple(got[l].shape))
        stage_bound("%s pyramid level %d" % (tag, l), got[l], p64[l], p32[l])
    net, inp = torch.tanh(c64[:, :128]).float(), torch.relu(c64[:, 128:]).float()
    h8, w8 = grid(tag)
    with torch.no_grad():
        corr = O.corr_lookup(p64, O.coords_grid(1, h8, w8, dtype=torch.float64) + fi.double()).float()
        u64 = O.update_block(net.double(), inp.double(), corr.double(), fi.double(), sd64)
        u32 = O.update_block(net, inp, corr, fi, sd)
    got = m.update_block(dev(net), dev(inp), dev(corr), dev(fi))
    for k, what in enumerate(("net", "mask", "delta_flow")):
        stage_bound("%s update block %s" % (tag, what), got[k], u64[k], u32[k])
    assert ops.guard_report() == [] and not ops.guard_tripped()


# ------------------------------------------------------------------------------------------------
# CPU: the case table covers what it claims, the float64 oracle runs, and the gate has teeth


def test_case_table_covers_what_it_claims():
    """ops.corr_packs_supported's conditions restated: C = 256 features (a multiple of 16), a split conv mode (the default),
    W8 even, and H8, W8 >= 8 (accflow_corr_disp_supported; the upper limits are far away)."""
    def packs(tag):
        h8, w8 = grid(tag)
        return 256 % 16 == 0 and w8 % 2 == 0 and h8 >= 8 and w8 >= 8

    for tag, (H, W) in CASES.items():
        h8, w8 = grid(tag)
        assert H % 8 == 0 and W % 8 == 0 and h8 >= 8 and w8 >= 8, tag      # level 3 of the pyramid is at least 1x1
    P = {tag: grid(tag)[0] * grid(tag)[1] for tag in CASES}
    assert P == {"A": 64, "B": 221, "C": 270, "D": 1161, "E": 72}
    assert P["A"] < 128 and P["E"] < 128
    assert all(P[t] % 128 for t in CASES)                                  # every case has a ragged last query block
    assert all(P[t] % 64 for t in "BCDE")
    assert [t for t in CASES if not packs(t)] == ["B", "D", "E"] and all(grid(t)[1] % 2 == 1 for t in "BDE")
    assert [t for t in CASES if packs(t)] == ["A", "C"]
    assert grid("D")[1] > 128 and (grid("D")[1] - 1) % 64 == 0             # the last 64-column target tile holds one column
    assert (P["D"] + 127) // 128 == 10 and (P["B"] + 127) // 128 == 2
    assert grid("C")[0] % 2 == 1 and grid("C")[1] % 2 == 0 and grid("C")[1] % 8 and grid("C")[1] < 64
    assert grid("B")[0] % 2 == 1 and grid("B")[1] % 2 == 1
    assert [(grid("B")[0] >> l, grid("B")[1] >> l) for l in range(4)] == [(13, 17), (6, 8), (3, 4), (1, 2)]
    assert (grid("A")[0] >> 3, grid("A")[1] >> 3) == (1, 1)
    # items of a call: estimator runs below the fork threshold of 4, AccFlow runs on both sides of it
    from accflow_amd.networks.AccFlow_ import AccFlow
    from accflow_amd.networks.raft.raft import RAFT
    items = {(tag, n, N): len(AccFlow.pair_schedule(n)) * N for tag, n, N in ACCFLOW_RUNS}
    assert items == {("B", 4, 2): 10, ("C", 4, 1): 5, ("E", 3, 1): 3}
    assert RAFT._group_cuts(5, 2) == [0, 2, 5] and RAFT._group_cuts(10, 2) == [0, 5, 10]
    assert all(N < 4 for _, N in ESTIMATOR_RUNS)
    assert {t for t, _ in ESTIMATOR_RUNS} | {t for t, _, _ in ACCFLOW_RUNS} == set(CASES)
    # every W8-odd case reaches the per-pair route through estimate_pairs somewhere, every W8-even one the packed route
    assert {"B", "D"} <= {t for t, _ in ESTIMATOR_RUNS} and {"B", "E"} <= {t for t, _, _ in ACCFLOW_RUNS}


@pytest.mark.parametrize("tag", sorted(CASES))
def test_float64_oracle_runs_every_size(tag):
    """RAFT in float64 at every case (2 iterations here; the GPU tests run 12): float64 out, close to the fp32 run."""
    sd, sd64 = weights("raft")
    i1, i2 = pair(tag)
    with torch.no_grad():
        r64 = O.raft_forward(sd64, i1.double(), i2.double(), 2)
        r32 = O.raft_forward(sd, i1, i2, 2)
    assert r64.dtype == torch.float64 and tuple(r64.shape) == (1, 2) + CASES[tag] and bool(torch.isfinite(r64).all())
    assert O.epe(r32.double(), r64)[1] <= 1e-3


def test_float64_accflow_oracle_runs():
    """AccFlow(GMA) in float64 at E, 3 frames (downflow8 follows its input's dtype)."""
    sd, sd64 = weights("acc|gma")
    fr = frames("E", 3)
    with torch.no_grad():
        r64 = O.accflow_forward(sd64, [f.double() for f in fr], iters=2, gma=True)
        r32 = O.accflow_forward(sd, fr, iters=2, gma=True)
    assert len(r64) == 1 and r64[0].dtype == torch.float64 and r32[0].dtype == torch.float32
    assert O.epe(r32[0].double(), r64[0])[1] <= 1e-3


def _mutant_last_query_pixel(monkeypatch):
    """(a) the lookup of query pixel P - 1 (the ragged tail of the last 128-pixel block) taken from pixel P - 2."""
    real = O.corr_lookup

    def lookup(pyramid, coords, radius=4):
        out = real(pyramid, coords, radius)
        out[:, :, -1, -1] = out[:, :, -1, -2]
        return out
    monkeypatch.setattr(O, "corr_lookup", lookup)


def _mutant_dropped_target_column(monkeypatch):
    """(b) the last column of every pyramid level zeroed."""
    real = O.corr_pyramid

    def pyramid(fmap1, fmap2, num_levels=4):
        pyr = [lvl.clone() for lvl in real(fmap1, fmap2, num_levels)]
        for lvl in pyr:
            lvl[..., -1] = 0
        return pyr
    monkeypatch.setattr(O, "corr_pyramid", pyramid)


def _mutant_shifted_pool(monkeypatch):
    """(c) level 1 pooled from level 0 shifted by one column (the other levels as they were)."""
    real = O.corr_pyramid

    def pyramid(fmap1, fmap2, num_levels=4):
        pyr = list(real(fmap1, fmap2, num_levels))
        h1, w1 = pyr[1].shape[2:]
        t = pyr[0][:, :, :2 * h1, 1:1 + 2 * w1]
        assert t.shape[3] == 2 * w1
        pyr[1] = (((t[:, :, 0::2, 0::2] + t[:, :, 0::2, 1::2]) + t[:, :, 1::2, 0::2]) + t[:, :, 1::2, 1::2]) * 0.25
        return pyr
    monkeypatch.setattr(O, "corr_pyramid", pyramid)


def _mutant_wrong_context_item(monkeypatch):
    """(d) the context features of item 1 used for item 0."""
    real = O.basic_encoder

    def encoder(x, sd, p, kind):
        out = real(x, sd, p, kind)
        if p == "cnet":
            out = out.clone()
            out[0] = out[1]
        return out
    monkeypatch.setattr(O, "basic_encoder", encoder)


MUTANTS = {"a": _mutant_last_query_pixel, "b": _mutant_dropped_target_column, "c": _mutant_shifted_pool,
           "d": _mutant_wrong_context_item}


def test_gate_accepts_the_fp32_oracle():
    r64, r32 = estimator_refs("raft", "B", 2)
    ok, fig = gate("fp32 oracle B N=2", r32, r64, r32)
    assert ok and fig["ratio_mean"] == 1.0 and fig["ratio_max"] == 1.0
    assert 0 < fig["d32_mean"] <= 1e-4 and fig["d32_max"] <= 1e-3, fig      # (the yardstick itself is fp32 rounding, no more)


@pytest.mark.parametrize("which", sorted(MUTANTS))
def test_gate_rejects_mutant(monkeypatch, which):
    """The fp32 oracle at B (N = 2) with one glue fault injected: the gate must see it."""
    r64, r32 = estimator_refs("raft", "B", 2)       # (before the fault goes in)
    sd, _ = weights("raft")
    i1, i2 = pair("B", 2)
    MUTANTS[which](monkeypatch)
    with torch.no_grad():
        bad = O.raft_forward(sd, i1, i2, ITERS)
    monkeypatch.undo()
    ok, fig = gate("mutant (%s) B N=2" % which, bad, r64, r32)
    assert not ok, (which, fig)
    assert fig["got_max"] > FACTOR * fig["d32_max"] and fig["got_mean"] > FACTOR * fig["d32_mean"], (which, fig)
