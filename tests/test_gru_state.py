"""The GRU state of the refinement loop against float64.

With ACCFLOW_H16_STATE=1 (the default) the ConvGRU state h lives only as the pre-split fp16 hi + lo tensor ws.h16 inside the
loop, and the GRU_Q epilogue re-rounds it in place once per half-step.  Error model (include/accflow_hip.h, ACCFLOW_CONV_F16X3):
the stored value carries 22 significant bits for |h| >= 2^-7 and an absolute resolution of 2^-29 below, i.e. one rounding moves
h by at most 2^-22 |h| + 2^-29.  Everything here runs through the product's code path (BasicUpdateBlock.gru_context /
gru_step on an UpdateWorkspace, descriptor replay from the second call on) and is compared with a float64 evaluation of the
same operation; the fp32-state form (rounds 3-5, USE_H16_STATE = False) runs next to it on the same inputs.

Per-element gate of one GRU iteration (two half-steps s), unit(h) = 2^-22 |h| + 2^-29:
    |h_gpu - h_64| <= K_STATE unit(h_64) + K_ACC 2^-22 sum_s z_s (M_q,s + 2 M_z,s)
  - the state term: one split rounds by at most 2^-23 |h| (lo carries the 11 bits below hi's half ulp) or 2^-29 below
    |h| = 2^-7, after the blend was formed in fp32 (2^-24 |h|): two half-steps give 2 unit at most (1.5 above 2^-7);
  - the arithmetic term: M_*,s = (|W| * |input|) + |b| is the absolute sum behind a gate's pre-activation (float64); an
    f16x3 product errs by about 2^-22 of |w x| and the fp32 sum of the products by less (a bound: the measured share is
    far below it); a pre-activation error reaches h through z (q's share) or z (1 - z) |q - h| <= 2 z (z's share).
  - where an update gate is closed (z <= 2^-30 in both half-steps, so that the exact iteration moves h by less than 1e-3
    unit and the fp32 blend (1 - z) h + z q gives h back) the state is CARRIED: it is representable and must come back
    unchanged, so the error there must stay below K_CARRY unit.  (With z of 1e-6 the fp32 blend alone can move h by one
    fp32 ulp, which the split may turn into one 22-bit step: measured at 3 of 10.8M elements at (11, 60, 128).)  That is
    the part that sees one lost bit of the state (a 21-bit state moves a carried value by up to one unit); the fp16-hi-only
    state fails both parts.  Both are asserted on float64 emulations of such states (test_host_logic.py runs the same
    check on the CPU).
Measured on the MI355X (gate ratio = max of error / tolerance; all elements / carried ones): packed state 0.49-0.97 / <= 0.002,
fp32 state 0.20-0.48 / <= 0.003 over the shapes below; the emulated intact split reaches 0.49-0.90 (the state term is the
binding one: two roundings of a state below 2^-7), one dropped lo bit 0.99-1.93 / 3.97-4.00, fp16 hi only ~1000 / ~3700."""
import pytest
import torch
import torch.nn.functional as F

from oracle import accflow_oracle as O

pytestmark = pytest.mark.gpu

K_STATE = 2.0           # two state roundings per iteration, each after an fp32 blend
K_CARRY = 0.5           # a carried (closed-gate) state: no rounding at all by the model, half a unit of headroom
K_ACC = 1.0             # the worst-case bound of the conv arithmetic (the measured share is far below it)
# packed-state error / fp32-state error over long recurrences, RMS and max (measured up to 1.56 and 2.29: test_recurrence_drift)
DRIFT_FACTOR, DRIFT_FACTOR_MAX = 2.0, 3.0
U22, A29 = 2.0 ** -22, 2.0 ** -29


def dev(t):
    return t.cuda()


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def ops():
    from accflow_amd import ops as o
    if o.conv_mode_name() != "f16x3":
        pytest.skip("the pre-split state belongs to the f16x3 mode")
    return o


# ---- float64 restatements -------------------------------------------------------------------------------------------

def round_sig(x, bits, min_ulp):
    """x rounded to nearest-even with `bits` significant bits, never finer than min_ulp (float64)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(1e-300)))
    ulp = torch.clamp(torch.pow(2.0, e - (bits - 1)), min=min_ulp)
    return torch.round(x / ulp) * ulp


def state_rounding(lo_bits=11, hi_only=False):
    """The kernels' split of the state, h * 2^4 = hi + lo with hi, lo fp16 (11 significant bits, subnormal step 2^-24),
    emulated in float64; lo_bits < 11 or hi_only emulate a state that lost bits."""
    def rnd(h):
        x = h * 16.0
        hi = round_sig(x, 11, 2.0 ** -24)
        if hi_only:
            return hi / 16.0
        return (hi + round_sig(x - hi, lo_bits, 2.0 ** (-24 + 11 - lo_bits))) / 16.0
    return rnd


def gru_ref(h, x, sd, p, rnd=None, mag=False):
    """SepConvGRU.forward (O.sep_conv_gru) with an optional rounding of the state after each half-step, and (mag) the
    per-element arithmetic term of the gate, sum over the half-steps of z (M_q + 2 M_z), and the larger z of the two.
    -> (h, acc, zmax) with mag, else (h, None, None)"""
    acc = zmax = torch.zeros_like(h) if mag else None
    for s, pad in (("1", (0, 2)), ("2", (2, 0))):
        hx = torch.cat([h, x], 1)
        wz, bz = sd[p + ".convz" + s + ".weight"], sd[p + ".convz" + s + ".bias"]
        wr, br = sd[p + ".convr" + s + ".weight"], sd[p + ".convr" + s + ".bias"]
        wq, bq = sd[p + ".convq" + s + ".weight"], sd[p + ".convq" + s + ".bias"]
        z = torch.sigmoid(F.conv2d(hx, wz, bz, padding=pad))
        r = torch.sigmoid(F.conv2d(hx, wr, br, padding=pad))
        qin = torch.cat([r * h, x], 1)
        q = torch.tanh(F.conv2d(qin, wq, bq, padding=pad))
        hn = (1 - z) * h + z * q
        if mag:
            mz = F.conv2d(hx.abs(), wz.abs(), bz.abs(), padding=pad)
            mq = F.conv2d(qin.abs(), wq.abs(), bq.abs(), padding=pad)
            acc = acc + z * (mq + 2 * mz)
            zmax = torch.maximum(zmax, z)
        h = rnd(hn) if rnd is not None else hn
    return h, acc, zmax


def gate_ratios(got, h0, h64, acc, zmax):
    """(max of error / tolerance over all elements, the same over the carried elements - update gate z <= 2^-30 in both
    half-steps, which the exact iteration moves by less than 1e-3 unit - with tolerance K_CARRY unit)"""
    err = (got.double() - h64).abs()
    unit = U22 * h64.abs() + A29
    r_all = float((err / (K_STATE * unit + K_ACC * U22 * acc)).max())
    carried = ((h64 - h0).abs() <= 1e-3 * unit) & (zmax <= 2.0 ** -30)
    assert int(carried.sum()) >= 4 * h64.shape[0] * h64.shape[2] * h64.shape[3] // 2    # (most of the closed z channels 4:8)
    return r_all, float((err[carried] / (K_CARRY * unit[carried])).max())


def gate_ok(r):
    return r[0] <= 1.0 and r[1] <= 1.0


def check_gate_discrimination(h0, x, sd64, p="update_block.gru"):
    """The gate of one iteration against float64 emulations of the state: rejects an fp16-hi-only state and a hi + lo state
    with one lo bit dropped, accepts the intact split.  -> {label: gate ratios}"""
    h64, acc, zmax = gru_ref(h0, x, sd64, p, mag=True)
    out = {}
    for label, rnd, ok in (("fp16 hi only", state_rounding(hi_only=True), False),
                           ("hi + lo, one lo bit dropped", state_rounding(10), False),
                           ("hi + lo (the kernels' split)", state_rounding(11), True)):
        emu = gru_ref(h0, x, sd64, p, rnd=rnd)[0]
        out[label] = gate_ratios(emu, h0, h64, acc, zmax)
        print("  emulated state %s: gate ratios %.3f / %.3f (all / carried)" % ((label,) + out[label]))
        assert gate_ok(out[label]) == ok, (label, out[label])
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------

def saturated_state_dict(name):
    """(estimator on the CPU, its state_dict) from make_state_dict, with a few output channels of convz1 / convz2 driven
    into z ~ 1 (0:4), z ~ 0 (4:8: the carried state) and into large pre-activations of both signs (8:12)."""
    from accflow_amd.data.synthetic import make_state_dict
    from accflow_amd.networks import build_flow_estimator
    m = build_flow_estimator(name)
    sd = make_state_dict(m)
    for s in ("1", "2"):
        w, b = sd["update_block.gru.convz%s.weight" % s], sd["update_block.gru.convz%s.bias" % s]
        b[0:4] = 30.0
        b[4:8] = -30.0
        w[8:12] *= 30.0
    m.load_state_dict(sd, strict=True)
    return m, sd


def gru_weights64(sd, device):
    return {k: v.double().to(device) for k, v in sd.items() if k.startswith("update_block.gru.")}


def gru_state_dict(name):
    m, sd = saturated_state_dict(name)
    return m.cuda().eval(), gru_weights64(sd, "cuda")


def gru_inputs(B, h, w, x_dim, seed, edges=True):
    """h (128 channels), inp (128), rest = x without inp (x_dim - 128): fp32 CPU tensors.  edges: h saturated
    (|h| = 1 - 1e-6), tiny (|h| < 2^-7), exact zeros, both signs; a pixel block with a large context addend."""
    g = gen(seed)
    hs = torch.tanh(torch.randn(B, 128, h, w, generator=g) * 1.5)
    inp = torch.relu(torch.randn(B, 128, h, w, generator=g))
    rest = torch.relu(torch.randn(B, x_dim - 128, h, w, generator=g))
    rest[:, 126:128] = torch.randn(B, 2, h, w, generator=g) * 4.0           # the flow channels of the motion features
    if edges:
        # (channels 0:16, which hold the saturated gates, keep spread values: a carried state of every magnitude)
        sign = torch.sign(torch.randn(B, 24, h, w, generator=g))
        hs[:, 16:40] = sign * (1.0 - 1e-6)                                   # saturated state
        hs[:, 40:64] = torch.randn(B, 24, h, w, generator=g) * 2.0 ** -10    # the absolute-resolution regime
        hs[:, 64:72] = 0.0
        hs[:, 72:80] = torch.randn(B, 8, h, w, generator=g) * 2.0 ** -20
        hs[:, 6:8] = torch.randn(B, 2, h, w, generator=g) * 2.0 ** -9        # tiny ones among the carried channels too
        inp[:, :, : max(1, h // 3), : max(1, w // 3)] *= 40.0                # gru_pre of large magnitude
    return hs, inp, rest


def make_ws(ops, ub, hs, inp, rest, monkeypatch, packed):
    """An UpdateWorkspace filled as RAFT._prepare_context does (net, inp, h16), with the motion channels pre-split into
    x16; packed = False runs the fp32-state form.  Returns (ws, h, x) where h, x are the values the kernels read."""
    import accflow_amd.networks.raft.update as U
    monkeypatch.setattr(U, "USE_H16_STATE", packed)
    B, _, h, w = hs.shape
    x_dim = 128 + rest.shape[1]
    ws = U.UpdateWorkspace(B, h, w, torch.device("cuda"), x_dim=x_dim)
    assert ws.s16 and ws.net_in_h16 == (packed and U.h16_state_supported())
    net = ops.to_s16(dev(hs)).to_float()                  # exactly representable by the pre-split state
    inp_k = ops.to_s16(dev(inp)).to_float()               # (gru_context splits the context features once)
    ops.copy_into(net, ws.net)
    ops.copy_into(inp_k, ws.inp)
    ops.copy_into(dev(rest), ws.hx[:, 256:])
    ops.to_s16(ws.net, ws.h16)
    ops.to_s16(ws.hx[:, 256:].contiguous(), ws.x16)
    assert torch.equal(ws.h16.to_float(), net)
    x = torch.cat([inp_k, ws.x16.to_float()], 1)          # the de-split motion features
    return ws, net.double(), x.double()


MODELS = {}


def model(name):
    if name not in MODELS:
        MODELS[name] = gru_state_dict(name)
    return MODELS[name]


# ---- 1 + 2: one iteration at the edges ------------------------------------------------------------------------------

SHAPES = [(1, 16, 32), (3, 13, 37),
          (2, 3, 20),      # smaller than one 4 x 32 direct tile (DIR_TH / DIR_TW, csrc/conv_common.h)
          (1, 5, 33),      # one past a tile in both directions
          (2, 2, 45), (2, 45, 2),   # below the 5-tap reach in one direction
          (11, 60, 128)]   # the 480x1024 pair batch


@pytest.mark.parametrize("name", ["raft", "gma"])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_iteration_vs_float64(ops, name, shape, monkeypatch):
    m, sd64 = model(name)
    ub = m.update_block
    B, h, w = shape
    x_dim = 384 if name == "gma" else 256
    hs, inp, rest = gru_inputs(B, h, w, x_dim, seed=100 + B * 7 + h + w)
    ratios = {}
    for packed in (True, False):
        ws, h0, x = make_ws(ops, ub, hs, inp, rest, monkeypatch, packed)
        try:
            ub.gru_step(ws)
        except RuntimeError as e:      # a shape the product routes to the packed path must be accepted by the library
            pytest.fail("gru_step refused %s at %s (packed=%s): %s" % (name, shape, packed, e))
        got = ws.net32()
        assert not ops.guard_tripped()
        h64, acc, zmax = gru_ref(h0, x, sd64, "update_block.gru", mag=True)
        ratios[packed] = gate_ratios(got, h0, h64, acc, zmax)
        print("GRU 1 iteration %s %s %s state: max err %.2e, gate ratios %.3f / %.3f (all / carried)"
              % ((name, shape, "packed" if packed else "fp32", float((got.double() - h64).abs().max())) + ratios[packed]))
    assert gate_ok(ratios[True]) and gate_ok(ratios[False]), ratios
    if B * h * w <= 2000:      # 2: the same gate rejects a state that lost bits (float64 emulations on the same inputs)
        check_gate_discrimination(h0, x, sd64)


# ---- 3: drift of the recurrence ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["raft", "gma"])
@pytest.mark.parametrize("shape", [(2, 13, 37), (11, 60, 128)])
def test_recurrence_drift(ops, name, shape, monkeypatch):
    """x fixed, 64 calls of gru_step on one workspace (calls 2.. replay the descriptors) against the float64 recurrence.
    Gate per iteration: packed-state error <= factor x fp32-state error + FLOOR, FLOOR = two roundings of a unit state
    (2 (2^-22 + 2^-29)), factor DRIFT_FACTOR for the RMS and DRIFT_FACTOR_MAX for the max (one element); after 64
    iterations the packed-state error <= DRIFT_BOUND (max, RMS).
    Measured on the MI355X: no growth of the packed state's error beyond the fp32 state's.  RMS packed / fp32 at iteration
    1 -> 64: RAFT (2, 13, 37) 1.37e-7 / 9.4e-8 -> 1.74e-7 / 1.22e-7, GMA 1.80e-7 -> 2.11e-7 / 1.39e-7, RAFT (11, 60, 128)
    1.56e-7 -> 1.93e-7 / 1.85e-7, GMA 1.84e-7 -> 2.20e-7 / 2.15e-7; the RMS ratio stays flat at <= 1.56 (the extra rounding
    of a 22-bit state), the max ratio reaches 2.29 (single elements of the small grid); max error at 64: <= 3.84e-5."""
    m, sd64 = model(name)
    ub = m.update_block
    B, h, w = shape
    x_dim = 384 if name == "gma" else 256
    hs, inp, rest = gru_inputs(B, h, w, x_dim, seed=7 + B + h, edges=False)
    n = 64
    curves = {}
    for packed in (True, False):
        ws, h64, x = make_ws(ops, ub, hs, inp, rest, monkeypatch, packed)
        cur = []
        for it in range(n):
            ub.gru_step(ws)
            h64 = gru_ref(h64, x, sd64, "update_block.gru")[0]
            d = ws.net32().double() - h64
            cur.append((float(d.abs().max()), float(d.pow(2).mean().sqrt())))
        assert "zr1" in ws.descs and not ops.guard_tripped()
        curves[packed] = cur
    print("\nGRU recurrence %s %s: iteration, max / RMS error of the packed state, of the fp32 state" % (name, shape))
    for it in range(n):
        (pm, pr), (fm, fr) = curves[True][it], curves[False][it]
        print("  %2d  packed %.3e / %.3e   fp32 %.3e / %.3e" % (it + 1, pm, pr, fm, fr))
    floor = 2 * (U22 + A29)
    for it in range(n):
        (pm, pr), (fm, fr) = curves[True][it], curves[False][it]
        assert pm <= DRIFT_FACTOR_MAX * fm + floor and pr <= DRIFT_FACTOR * fr + floor, (it + 1, curves[True][it], curves[False][it])
    assert curves[True][-1][0] <= DRIFT_BOUND[0] and curves[True][-1][1] <= DRIFT_BOUND[1], curves[True][-1]


DRIFT_BOUND = (1e-4, 5e-7)      # packed-state max / RMS error after 64 iterations (measured <= 3.84e-5 / 2.20e-7)


# ---- 4: end to end at long schedules ----------------------------------------------------------------------------------

def _both_states(monkeypatch, fn):
    import accflow_amd.networks.raft.update as U
    out = {}
    for packed in (True, False):
        monkeypatch.setattr(U, "USE_H16_STATE", packed)
        out[packed] = fn()
    return out


@pytest.mark.parametrize("name", ["raft", "gma"])
def test_estimator_iters32_vs_oracle(ops, name, monkeypatch):
    """RAFT / GMA at 128x256 with iters=32 (and 32 from a flow_init) against the CPU fp32 oracle, packed state on and off.
    Max-EPE gates about 4x the measured maxima (RAFT 2.82e-4, GMA 3.30e-3 px); the packed state's mean EPE stays within
    DRIFT_FACTOR of the fp32 state's (measured: within 1.3 %)."""
    from accflow_amd.data.synthetic import make_sequence, make_state_dict, normalize
    from accflow_amd.networks import build_flow_estimator
    m = build_flow_estimator(name)
    sd = make_state_dict(m)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    fr = [normalize(f) for f in make_sequence(1010, 2, 128, 256)]
    init = torch.randn(1, 2, 16, 32, generator=gen(23)) * 2.0
    refs = [O.raft_forward(sd, fr[1], fr[0], iters=32, gma=name == "gma"),
            O.raft_forward(sd, fr[1], fr[0], iters=32, flow_init=init, gma=name == "gma")]
    res = _both_states(monkeypatch, lambda: [m(dev(fr[1]), dev(fr[0]), iters=32).cpu(),
                                             m(dev(fr[1]), dev(fr[0]), iters=32, flow_init=dev(init)).cpu()])
    for k, ref in enumerate(refs):
        (pm, px), (fm, fx) = O.epe(res[True][k], ref), O.epe(res[False][k], ref)
        print("%s iters=32%s: EPE vs oracle mean / max: packed %.2e / %.2e, fp32 state %.2e / %.2e"
              % (name, " flow_init" if k else "", pm, px, fm, fx))
        for me, mx in ((pm, px), (fm, fx)):
            assert me <= 1e-3 and mx <= E2E_MAX[name], (name, k, me, mx)
        assert pm <= DRIFT_FACTOR * fm + 1e-5, (name, k, pm, fm)


def test_accflow_warm_iters_vs_oracle(ops, monkeypatch):
    """AccFlow(warm_start=True, warm_iters=24), ofe_iters=32, 4 frames at 128x256 against O.accflow_forward_warm.  Max-EPE
    gate about 4x the measured maximum (2.75e-3 px); packed-state mean EPE within DRIFT_FACTOR of the fp32 state's (1.18x)."""
    from accflow_amd.data.synthetic import make_sequence, make_state_dict, normalize
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.AccFlow_ import AccFlow
    model = AccFlow(build_flow_estimator("acc|raft"), warm_start=True, warm_iters=24)
    sd = make_state_dict(model)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    model.ofe_iters = 32
    frames = [normalize(f) for f in make_sequence(1011, 4, 128, 256)]
    refs = O.accflow_forward_warm(sd, frames, iters=32, warm_iters=24)
    res = _both_states(monkeypatch, lambda: [o.cpu() for o in model(images=[dev(f) for f in frames])])
    assert len(res[True]) == len(refs) == 2
    for k, ref in enumerate(refs):
        (pm, px), (fm, fx) = O.epe(res[True][k], ref), O.epe(res[False][k], ref)
        print("AccFlow warm 24 / 32 out%d: EPE vs oracle mean / max: packed %.2e / %.2e, fp32 state %.2e / %.2e"
              % (k, pm, px, fm, fx))
        for me, mx in ((pm, px), (fm, fx)):
            assert me <= 1e-3 and mx <= E2E_MAX["accflow"], (k, me, mx)
        assert pm <= DRIFT_FACTOR * fm + 1e-5, (k, pm, fm)


E2E_MAX = {"raft": 2e-3, "gma": 2e-2, "accflow": 2e-2}     # max EPE px at 32 iterations (measured 2.82e-4, 3.30e-3, 2.75e-3)
