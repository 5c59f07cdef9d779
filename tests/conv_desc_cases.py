"""The cases of tests/test_conv_desc.py and of tests/golden/make_conv_desc_golden.py, which records them: what accflow_amd.ops
hands to the library for a fixed list of convolution calls.

run_case(ops, name) runs one case with five entry points of the loaded library wrapped - accflow_conv2d_f32,
accflow_conv_stat_slots, accflow_conv_in_norm_supported, accflow_tap_sum_f32, accflow_tap_sum_parts_f32 - and returns a
JSON-able record: the ordered calls, what the op returned (type and shape), what it raised, whether the range guard tripped.

A descriptor is written "field=value field=value ..." over its non-zero fields (all of them: the four src[] entries as
src0.C=..., `reserved` included).  A pointer field is written as a LABEL, never an address:
    the name the case gave the tensor or pack attribute whose data_ptr() / ptr() it equals (in0, e0, pk.wpatch16,
    pk2.ztaps_acc.wscale16, ...; a test_conv_routes row: the names of its input dict, and pk#k.attr for the k-th pack built);
    guard, kws (this thread's range-guard flag and split-K scratch);
    tmp#k - the k-th distinct pointer not otherwise known, in order of first appearance in the case.
So a builder that swaps e0 and e1, or hands wpatch where wpatch16 belongs, differs from the record although every scalar agrees.

The forwards (one RAFT, GMA and AccFlow forward at tests/test_ragged_frames.py's 13x17-grid size, 2 refinement iterations) know
no tensor by name: weight-pack fields read `pack`, and tmp#k counts within ONE descriptor (first appearance in field order).
Across calls the caching allocator hands a freed temporary's address to a later one depending on what the process ran before,
so identity over a whole forward would not reproduce from one process to the next.  To keep the file small a forward stores,
per distinct descriptor, a summary and the first 16 hex digits of the SHA-256 of its text, and the order of the calls.
"""
import contextlib
import ctypes
import hashlib
import os
import zlib

import torch

import test_conv_routes as CR
import test_ragged_frames as RF

ENTRIES = ("accflow_conv2d_f32", "accflow_conv_stat_slots", "accflow_conv_in_norm_supported", "accflow_tap_sum_f32",
           "accflow_tap_sum_parts_f32")
PACK_ATTRS = ("wpack", "ktab", "bias", "wsplit", "wpatch", "wpatch16", "wscale16", "wsplit16")
PACK_FIELDS = PACK_ATTRS + ("tg_w16", "tg_scale")
# CONV_DESC_DRY=1: the three launching entry points are recorded and NOT forwarded (the two queries are host code and still
# are) - for trying a deliberately wrong builder against the record without launching what it built
DRY = os.environ.get("CONV_DESC_DRY", "0") == "1"
LAUNCHES = ("accflow_conv2d_f32", "accflow_tap_sum_f32", "accflow_tap_sum_parts_f32")
H16, W16 = 13, 37          # the ragged frame of test_conv_routes (4 x 32-pixel tiles, the last of a row 5 wide, the last row 1 high)


def _is_ptr(ctype):
    return ctype is ctypes.c_void_p


class Recorder:
    """Wraps the entry points on the library handle for the length of a `with`; names pointers."""

    def __init__(self, ops, forward=False, extra=()):
        from accflow_amd import _lib as L
        self.ops, self.L, self.lib, self.forward = ops, L, L.load(), forward
        self.entries = ENTRIES + tuple(extra)
        self.names, self.tmp, self.calls, self.packs = {}, {}, [], 0
        self.alive = []        # every named tensor lives as long as the record: a freed address would be handed out again

    # ---- names
    def name(self, label, t):
        if t is not None:
            self.alive.append(t)
            self.names.setdefault(t.ptr() if isinstance(t, self.ops.S16) else t.data_ptr(), label)
        return t

    def name_pack(self, label, pk):
        for a in PACK_ATTRS:
            if getattr(pk, a, None) is not None:
                self.name("%s.%s" % (label, a), getattr(pk, a))
        for sub in ("ztaps", "zcols", "ztaps_acc"):
            if getattr(pk, sub, None) is not None:
                self.name_pack("%s.%s" % (label, sub), getattr(pk, sub))
        return pk

    def label(self, field, ptr, local):
        if not ptr:
            return "null"
        if ptr in self.names:
            return self.names[ptr]
        tls = self.ops._tls
        flags = [getattr(tls, "guard_flag", None)] + list(getattr(tls, "guards", {}).values())
        if any(t is not None and ptr == t.data_ptr() for t in flags):
            return "guard"
        if any(ptr == t.data_ptr() for t in getattr(tls, "ksplit_ws", {}).values()):
            return "kws"
        if self.forward and field in PACK_FIELDS:
            return "pack"
        book = local if self.forward else self.tmp
        return "tmp#%d" % book.setdefault(ptr, len(book))

    # ---- records
    def describe(self, d):
        local, out = {}, []
        for f, ct in self.L.ConvDesc._fields_:
            v = getattr(d, f)
            if f == "src":
                for k in range(self.L.MAX_SRC):
                    for sf, sct in self.L.ConvSrc._fields_:
                        sv = getattr(v[k], sf)
                        if sv:
                            out.append("src%d.%s=%s" % (k, sf, self.label(sf, sv, local) if _is_ptr(sct) else sv))
            elif v:
                out.append("%s=%s" % (f, self.label(f, v, local) if _is_ptr(ct) else v))
        return " ".join(out)

    def _arg(self, a, ct, local):
        if _is_ptr(ct):
            return self.label("", a.value if isinstance(a, ctypes.c_void_p) else a, local)
        return a

    def __enter__(self):
        self._real = {n: getattr(self.lib, n) for n in self.entries}
        for n in self.entries:
            setattr(self.lib, n, self._wrapper(n, self._real[n]))
        return self

    def __exit__(self, *exc):
        for n, fn in self._real.items():
            setattr(self.lib, n, fn)

    def _wrapper(self, n, real):
        types = self.L.SIGNATURES[n]
        short = n[len("accflow_"):]
        if DRY and n == "accflow_conv2d_f32":      # refused as the launch would refuse it (validation and plan are host code)
            real = lambda dref, stream: self.lib.accflow_conv_plan_query(dref, (ctypes.c_int * 16)(), 16)  # noqa: E731
        elif DRY and n in LAUNCHES:
            real = lambda *a: 0  # noqa: E731

        def call(*args):
            if types and types[0] == ctypes.POINTER(self.L.ConvDesc):
                text = self.describe(args[0]._obj)
                rc = real(*args)
                self.calls.append([short, text] if n == "accflow_conv2d_f32" else [short, text, rc])
            else:
                local = {}
                self.calls.append([short] + [self._arg(a, ct, local) for a, ct in zip(args[:-1], types[:-1])])   # (not the stream)
                rc = real(*args)
            return rc
        return call


def shape_of(r, ops):
    """type and shape of what an op returned"""
    if isinstance(r, torch.Tensor):
        return ["tensor"] + list(r.shape)
    if isinstance(r, ops.S16):
        return ["S16"] + list(r.shape)
    if isinstance(r, ops.ConvStats):
        return ["ConvStats", r.slots] + list(r.partial.shape)
    if isinstance(r, (tuple, list)):
        return [shape_of(x, ops) for x in r]
    if isinstance(r, dict):
        return {k: shape_of(v, ops) for k, v in sorted(r.items())}
    return r if r is None or isinstance(r, (bool, int, float, str)) else type(r).__name__


@contextlib.contextmanager
def patched(obj, **kw):
    saved = {k: getattr(obj, k) for k in kw}
    for k, v in kw.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(obj, k, v)


class Kit:
    """Seeded inputs of a case, named for the recorder as they are made.  Values stay inside the fp16 split's range."""

    def __init__(self, ops, rec, name):
        self.ops, self.rec = ops, rec
        self.g = torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)

    def t(self, name, *shape, scale=1.0):
        return self.rec.name(name, (torch.randn(*shape, generator=self.g) * scale).cuda())

    def s16(self, name, *shape):
        return self.rec.name(name, self.ops.S16.from_float(torch.randn(*shape, generator=self.g).cuda()))

    def o16(self, name, *shape):
        return self.rec.name(name, self.ops.S16.empty(*shape, "cuda"))

    def weight(self, cout, cin, k):
        w = torch.randn(cout, cin, k[0], k[1], generator=self.g) * (2.0 / (cin * k[0] * k[1])) ** 0.5
        return w.cuda(), (torch.randn(cout, generator=self.g) * 0.1).cuda()

    def pk(self, name, cout, cin, k, **kw):
        w, b = self.weight(cout, cin, k)
        return self.rec.name_pack(name, self.ops.PackedConv(w, b, padding=(k[0] // 2, k[1] // 2), **kw))

    def multi(self, name, pk):
        for a in ("wpatch16", "wscale16", "bias"):
            self.rec.name("%s.%s" % (name, a), getattr(pk, a))
        return pk


# ------------------------------------------------------------------------------------------------
# the cases: name -> f(ops, kit) -> what the op returned


CASES = {}


def case(f):
    CASES[f.__name__] = f
    return f


def _row_case(row):
    def run(ops, K):
        # the row's tensors are made inside run_row: its input dict names what goes to the device, every pack built is pk#k
        I = CR.inputs(row)
        ids = {}
        for k, v in I.items():
            for j, t in enumerate(v if isinstance(v, list) else [v]):
                if t is not None:
                    ids[id(t)] = k + (str(j) if isinstance(v, list) else "")
        real_cuda, real_init, real_minit = torch.Tensor.cuda, ops.PackedConv.__init__, ops.PackedMulti.__init__

        def cuda(t, *a, **kw):
            r = real_cuda(t, *a, **kw)
            if id(t) in ids:
                K.rec.name(ids[id(t)], r)
            return r

        def init(pk, *a, **kw):
            real_init(pk, *a, **kw)
            K.rec.name_pack("pk#%d" % K.rec.packs, pk)
            K.rec.packs += 1

        def minit(pk, *a, **kw):
            real_minit(pk, *a, **kw)
            K.multi("pk#%d" % K.rec.packs, pk)
            K.rec.packs += 1
        with patched(torch.Tensor, cuda=cuda), patched(ops.PackedConv, __init__=init), patched(ops.PackedMulti, __init__=minit):
            out, out16, stats, intact = CR.run_row(ops, row)
        assert intact
        return out, out16, stats
    return run


for _row in CR.ROWS:
    CASES["row: " + _row.name] = _row_case(_row)


@case
def p32_out_128(ops, K):
    return ops.conv2d(K.pk("pk", 128, 128, (1, 5)), K.s16("in0", 1, 128, H16, W16), p32_out=True)


def _gru_packed(ops, K, which):
    hd = 128
    h16, x16 = K.s16("in0", 1, hd, H16, W16), K.s16("in1", 1, 128, H16, W16)
    if which == "zr":
        pk = K.pk("pk", 2 * hd, 256, (1, 5), C0=hd)
        pre = K.rec.name("pre", ops.to_p32(K.t("pre_nchw", 1, 2 * hd, H16, W16, scale=0.2)))
        K.rec.name("e0", h16)      # (the state is in0 and e0: in0 was named first and stays the label of both)
        return ops.conv2d(pk, h16, in1=x16, out=K.t("out", 1, hd, H16, W16), act=ops.ACT_SIGMOID, epi=ops.EPI_GRU_ZR, e0=h16,
                          out16=K.o16("out16", 1, hd, H16, W16), fp32_out=False, pre=pre)
    pk = K.pk("pk", hd, 256, (1, 5), C0=hd)
    pre = K.rec.name("pre", ops.to_p32(K.t("pre_nchw", 1, hd, H16, W16, scale=0.2)))
    state = K.s16("e0", 1, hd, H16, W16)
    return ops.conv2d(pk, h16, in1=x16, out=None, act=ops.ACT_TANH, epi=ops.EPI_GRU_Q, e0=state, e1=K.t("e1", 1, hd, H16, W16),
                      out16=state, fp32_out=False, pre=pre)


@case
def gru_packed_zr(ops, K):
    return _gru_packed(ops, K, "zr")


@case
def gru_packed_q(ops, K):
    return _gru_packed(ops, K, "q")


@case
def out16_only_store(ops, K):
    return ops.conv2d(K.pk("pk", 64, 32, (3, 3)), K.t("in0", 1, 32, H16, W16), act=ops.ACT_RELU,
                      out16=K.o16("out16", 1, 64, H16, W16), fp32_out=False)


@case
def out16_only_gru_zr(ops, K):
    h16 = K.s16("in0", 1, 64, H16, W16)
    return ops.conv2d(K.pk("pk", 128, 128, (1, 5), C0=64), h16, in1=K.s16("in1", 1, 64, H16, W16), act=ops.ACT_SIGMOID,
                      epi=ops.EPI_GRU_ZR, e0=K.rec.name("e0", h16.to_float()), out16=K.o16("out16", 1, 64, H16, W16), fp32_out=False)


def _tapsum(src, hw, f16):
    def run(ops, K):
        with patched(ops, TAPSUM_F16=f16):
            pk = K.pk("pk", 2, 32, (3, 3))
            x = (K.s16 if src == "s16" else K.t)("in0", 1, 32, *hw)
            return ops.conv2d(pk, x, out=K.t("out", 1, 2, *hw), epi=ops.EPI_ACCUM, e0=K.t("e0", 1, 2, *hw))
    return run


for _src in ("s16", "f32"):
    for _hw in ((64, 64), (63, 65)):           # B*H*W = TAPSUM_MIN_PIXELS exactly, and one less
        for _f16 in (True, False):
            CASES["tapsum_%s_%dpx%s" % (_src, _hw[0] * _hw[1], "" if _f16 else "_bf16x6")] = _tapsum(_src, _hw, _f16)


@case
def s16_to_float_fallback(ops, K):
    with patched(ops, USE_TAPSUM=False):
        pk = K.pk("pk", 2, 32, (3, 3))
    assert pk.ztaps is None
    return ops.conv2d(pk, K.s16("in0", 1, 32, H16, W16))


def _deform_inputs(K, C, H, W):
    return K.t("in0", 2, C, H, W), K.t("offset", 2, 18, H, W, scale=2.0), torch.sigmoid(K.t("logit", 2, 9, H, W))


@case
def deform_two_pass(ops, K):
    pk = K.pk("pk", 32, 32, (3, 3), tap_major=True)
    x, off, m = _deform_inputs(K, 32, 14, 22)
    return ops.conv2d(pk, x, offset=off, dmask=K.rec.name("dmask", m))


@case
def deform_single_kernel(ops, K):
    with patched(ops, USE_DEFORM_COLUMNS=False):
        pk = K.pk("pk", 32, 32, (3, 3), tap_major=True)
    assert pk.zcols is None
    x, off, m = _deform_inputs(K, 32, 14, 22)
    return ops.conv2d(pk, x, offset=off, dmask=K.rec.name("dmask", m))


def _deform_s16(C):
    def run(ops, K):
        pk = K.pk("pk", C, C, (3, 3), tap_major=True)
        x, off, m = _deform_inputs(K, C, 14, 22)
        return ops.deform_conv2d_s16(pk, x, off, K.rec.name("dmask", m), K.o16("out16", 2, C, 14, 22))
    return run


CASES["deform_s16_presplit_columns"] = _deform_s16(32)
CASES["deform_s16_fp32_columns"] = _deform_s16(8)         # 9 x 8 channels: no multiple of 32


def _via_multi(n):
    def run(ops, K):
        pk = K.pk("pk", 64, 32 * n, (3, 3), C0=32)
        with patched(ops, S16_VIA_MULTI=True):
            return ops.conv2d(pk, K.s16("in0", 1, 32, H16, W16), K.s16("in1", 1, 32, H16, W16) if n == 2 else None)
    return run


CASES["s16_via_multi_1"] = _via_multi(1)
CASES["s16_via_multi_2"] = _via_multi(2)


@case
def no_patch_fp32(ops, K):
    with patched(ops, USE_PATCH=False):
        return ops.conv2d(K.pk("pk", 64, 32, (3, 3)), K.t("in0", 1, 32, H16, W16))


@case
def no_patch_s16(ops, K):
    with patched(ops, USE_PATCH=False):
        return ops.conv2d(K.pk("pk", 64, 32, (3, 3)), K.s16("in0", 1, 32, H16, W16))


def _multi(variant):
    def run(ops, K):
        B, C, H, W = 1, 32, 14, 22
        x16 = K.s16("in0", B, C, H, W)
        kw, srcs = {}, None
        if variant in ("strided", "projection"):
            w, b = K.weight(64, C, (3, 3))
            if variant == "strided":
                pk = ops.PackedMulti.from_strided(w, b, 1)
            else:
                wp, bp = K.weight(64, C, (1, 1))
                pk = ops.PackedMulti.from_strided_with_projection(w, b, 1, wp, bp)
            srcs, kw = [x16] * len(pk.C), dict(out_hw=(7, 11))
        else:
            w, b = K.weight(64, C, (3, 3))
            pk = ops.PackedMulti.from_cat(w, b, [C], 1)
            srcs = [x16]
            if variant == "stats":
                kw = dict(want_stats=True)
            elif variant == "s16_e0":
                kw = dict(act=ops.ACT_RELU, epi=ops.EPI_RES_RELU, e0=K.s16("e0", B, 64, H, W), out16=K.o16("out16", B, 64, H, W),
                          fp32_out=False)
            elif variant == "lay":
                kw = dict(lay=2)
            elif variant == "out_hw":
                kw = dict(out_hw=(H, W))
        K.multi("pk", pk)
        return ops.conv2d_multi(pk, srcs, **kw)
    return run


for _v in ("stats", "strided", "projection", "s16_e0", "lay", "out_hw"):
    CASES["multi_" + _v] = _multi(_v)


@case
def multi_cout4_refused(ops, K):
    """The one place where `Cout > 4` of the split-K offer is not implied by the pack rules: a 4-channel PackedMulti.  The plan
    refuses the descriptor before anything is launched (conv_plan.cpp: s16m_eligible); it is recorded all the same, without a
    workspace."""
    w, b = K.weight(4, 32, (3, 3))
    return ops.conv2d_multi(K.multi("pk", ops.PackedMulti.from_cat(w, b, [32], 1)), [K.s16("in0", 1, 32, 14, 22)])


def _ksplit(hw, scope):
    def run(ops, K):
        pk = K.pk("pk", 8, 16, (1, 1))
        with ops.ksplit_scope(scope):
            return ops.conv2d(pk, K.t("in0", 1, 16, *hw))
    return run


CASES["ksplit_scope_off"] = _ksplit((H16, W16), False)
CASES["ksplit_max_pixels"] = _ksplit((120, 256), True)               # B*OH*OW = KSPLIT_MAX_PIXELS
CASES["ksplit_max_pixels_plus_1"] = _ksplit((31, 991), True)         # ... + 1


def _timer(ops, names=("conv2d",)):
    from accflow_amd import profiler
    return patched(profiler, ACTIVE=profiler.KernelTimer(names))


def _raises(f):
    try:
        f()
    except RuntimeError as e:
        return "RuntimeError: %s" % e
    return "no error"


def _replay_protocol(ops, call, replay):
    """call(cache) -> result with the real arguments, replay(cache) with none: the three promises of the cache."""
    D, empty, timed = {}, {}, {}
    first = call((D, "k"))
    again = replay((D, "k"))                                  # the identical launch (the calls of the record show it)
    res = {"first": shape_of(first, ops), "replay_returns_first": again is first, "stored": "k" in D,
           "empty_cache": _raises(lambda: replay((empty, "k")))}
    with _timer(ops):
        call((timed, "k"))
        res["timer_writes"] = len(timed)
        res["timer_reads"] = _raises(lambda: replay((D, "k")))       # the stored entry is not replayed: the call needs its arguments
    return res


@case
def replay_conv2d(ops, K):
    pk, x, o16 = K.pk("pk", 64, 32, (3, 3)), K.s16("in0", 1, 32, H16, W16), K.o16("out16", 1, 64, H16, W16)
    return _replay_protocol(ops, lambda c: ops.conv2d(pk, x, out16=o16, act=ops.ACT_RELU, fp32_out=False, cache=c),
                            lambda c: ops.conv2d(None, None, cache=c))


@case
def replay_tapgemm(ops, K):
    p1, p2 = K.pk("pk", 128, 128, (3, 3)), K.pk("pk2", 2, 128, (3, 3))
    x, out = K.s16("in0", 1, 128, 20, 64), K.t("out", 1, 2, 20, 64)
    with ops.ksplit_scope(False):
        assert ops.tapgemm_eligible(p1, p2, x)
        return _replay_protocol(ops, lambda c: ops.conv2d_tapgemm(p1, p2, x, out=out, epi=ops.EPI_ACCUM, e0=out, cache=c),
                                lambda c: ops.conv2d_tapgemm(None, None, None, cache=c))


@case
def replay_corr_lookup_s16(ops, K):
    pyr = ops.corr_volume_disp(K.t("fmap1", 1, 32, 8, 16), K.t("fmap2", 1, 32, 8, 16))
    for l, t in enumerate(pyr.levels):
        K.rec.name("lvl%d" % l, t)
    coords = K.rec.name("coords", ops.coords_grid(1, 8, 16, "cuda"))
    o16 = K.o16("out16", 1, ops.LOOKUP_S16_CHANNELS, 8, 16)
    return _replay_protocol(ops, lambda c: ops.corr_lookup_s16(pyr, coords, o16, cache=c),
                            lambda c: ops.corr_lookup_s16(None, None, None, cache=c))


REPLAY_EXTRA = {"replay_corr_lookup_s16": ("accflow_corr_lookup_disp_s16",)}


@case
def profiler_details(ops, K):
    """detail / work / work_exec of the five conv2d records: one launch per form, and tapgemm's two."""
    from accflow_amd import profiler
    p1, p2 = K.pk("pk", 128, 128, (3, 3)), K.pk("pk2", 2, 128, (3, 3))
    w, b = K.weight(64, 32, (3, 3))
    with _timer(ops), ops.ksplit_scope(False):
        K.rec.alive += [ops.conv2d(K.pk("pk3", 64, 32, (3, 3)), K.t("in0", 1, 32, H16, W16), algo_cin=7),
                        ops.conv2d(p1, K.s16("in1", 1, 128, 20, 64)),
                        ops.conv2d_multi(ops.PackedMulti.from_cat(w, b, [32], 1), [K.s16("in2", 1, 32, H16, W16)]),
                        ops.conv2d_tapgemm(p1, p2, K.s16("in3", 1, 128, 20, 64))]
        return [[n, work, detail, wexec] for n, _, _, work, detail, wexec in profiler.ACTIVE.records]


def _forward(name):
    def run(ops, K):
        m = RF.model(name)
        with torch.no_grad():
            if name.startswith("acc"):
                saved = m.__dict__.get("ofe_iters")
                m.ofe_iters = 2
                try:
                    return m(images=[f.cuda() for f in RF.frames("B", 3)])
                finally:
                    if saved is None:
                        del m.ofe_iters
                    else:
                        m.ofe_iters = saved
            i1, i2 = RF.pair("B")
            return m(i1.cuda(), i2.cuda(), iters=2)
    return run


FORWARDS = {"forward_raft": "raft", "forward_gma": "gma", "forward_accflow": "acc|raft"}
for _n, _m in FORWARDS.items():
    CASES[_n] = _forward(_m)


def digest(text):
    return hashlib.sha256(text.encode()).hexdigest()[:16]


def summary(text):
    f = dict(kv.split("=", 1) for kv in text.split())
    return "Cout%s B%s %sx%s epi%s nsrc%s" % (f.get("Cout"), f.get("B"), f.get("OH"), f.get("OW"), f.get("epi", 0), f.get("nsrc", 0))


def run_case(ops, name):
    """-> the record of one case (see the module docstring).  Starts from a fresh split-K scratch buffer and a quiet guard, so
    that a case's record does not depend on what ran before it."""
    assert ops.current_mode() == ops.CONV_F16X3
    ops._tls.__dict__.pop("ksplit_ws", None)
    ops.guard_tripped()
    forward = name in FORWARDS
    rec = Recorder(ops, forward=forward, extra=REPLAY_EXTRA.get(name, ()))
    res = {}
    with rec:
        try:
            ret = CASES[name](ops, Kit(ops, rec, name))
            res["returns"] = shape_of(ret, ops)
        except RuntimeError as e:
            res["raises"] = str(e)
    res["guard_tripped"] = ops.guard_tripped()
    if forward:        # distinct descriptors as (summary, digest), the calls as indices into them
        table, order = {}, []
        for c in rec.calls:
            key = (c[0], summary(c[1]), digest(c[1])) + tuple(c[2:]) if len(c) > 1 and isinstance(c[1], str) and "=" in c[1] else tuple(c)
            order.append(table.setdefault(key, len(table)))
        res["distinct"], res["calls"] = [list(k) for k in table], order
        res["_texts"] = {digest(c[1]): c[1] for c in rec.calls if len(c) > 1 and isinstance(c[1], str) and "=" in c[1]}
    else:
        res["calls"] = rec.calls
    return res
