"""Records what the library's two route queries - accflow_conv_stat_slots and accflow_conv_in_norm_supported - answer for a
fixed grid of convolution descriptors: tests/golden/conv_route_queries.json.

The recorded file was written by the library as it stood BEFORE the dispatch moved into csrc/conv_plan.cpp (the queries were
dry runs of the whole dispatcher then); tests/test_conv_plan.py holds every later library to those answers.  Neither query
reaches the HIP runtime, so no GPU is needed; the pointer fields are dummy non-null values that are never dereferenced.
The routing switches are read once per process, hence one child process per environment.

    python tests/golden/make_conv_route_golden.py            # rewrite the JSON (only ever from the commit it records)
    python tests/golden/make_conv_route_golden.py --child    # one environment: prints {"slots": [...], "norm": [...]}
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "conv_route_queries.json")

F32, BF16X3, BF16X6, F16X3 = 0, 2, 3, 4
ACT_NONE, ACT_RELU = 0, 1
EPI_STORE, EPI_RES_RELU, EPI_ACCUM = 0, 1, 4
ENVS = [{}, {"ACCFLOW_DIRECT_W4": "0"}, {"ACCFLOW_S16M": "1"}, {"ACCFLOW_CONV_STEM": "0"}, {"ACCFLOW_PATCH_MIN_BLOCKS": "0"}]
SWITCHES = ("ACCFLOW_DIRECT_W4", "ACCFLOW_DIRECT_KT", "ACCFLOW_DIRECT_KT9", "ACCFLOW_S16M", "ACCFLOW_S16M_KT9", "ACCFLOW_S16M_LAY",
            "ACCFLOW_CONV_STEM", "ACCFLOW_PATCH_MIN_BLOCKS", "ACCFLOW_DIRECT_KSPLIT", "ACCFLOW_IM2COL_KSPLIT")

COUTS = (2, 4, 8, 32, 64, 96, 128, 192, 256, 320)
KERNELS = ((1, 1), (3, 3), (1, 5), (5, 1), (5, 5), (7, 7))
SIZES = ((1, 8, 16), (2, 37, 53), (1, 60, 128), (11, 60, 128), (1, 240, 512))
INPUTS = ((64, 0), (64, 64), (48, 80))      # (C0, C1): one source; two with C0 a multiple of 32; two with C0 % 32 == 16
PTR = 0x1000                                # every pointer of a descriptor: never dereferenced by the queries


def kpad(cin, kh, kw):
    return (cin * kh * kw + 31) // 32 * 32


def coutpad(cout):
    return (cout + 127) // 128 * 128


def s16_words(c, h, w):
    return (c + 7) // 8 * 2 * h * w * 4


def plain(mode, c0, c1, cout, k, stride, size, kws=0, **kw):
    """A descriptor of the in0 / in1 form as a dict of fields (every pack its mode can use is present).
    kws: 0 = no split-K workspace, 1 = room for 8 parts, 2 = room for one part and a half."""
    B, H, W = size
    KH, KW = k
    OH, OW = (H + 2 * (KH // 2) - KH) // stride + 1, (W + 2 * (KW // 2) - KW) // stride + 1
    d = dict(in0=PTR, in0_bs=c0 * H * W, C0=c0, C1=c1, B=B, H=H, W=W, OH=OH, OW=OW, KH=KH, KW=KW, stride=stride, padH=KH // 2,
             padW=KW // 2, Cout=cout, wpack=PTR, ktab=PTR, Kpad=kpad(c0 + c1, KH, KW), CoutPad=coutpad(cout), bias=PTR, out=PTR,
             out_bs=cout * OH * OW, act=ACT_NONE, epi=EPI_STORE, mode=mode)
    if c1:
        d.update(in1=PTR, in1_bs=c1 * H * W)
    if mode != F32:
        d.update(wsplit=PTR, wpatch=PTR)
    if mode == F16X3:
        d.update(wpatch16=PTR, wsplit16=PTR, wscale16=PTR, guard=PTR)
    if kws:
        nout = B * cout * OH * OW
        d.update(kws=PTR, kws_elems=8 * nout if kws == 1 else nout * 3 // 2)
    d.update(kw)
    return d


def s16_inputs(d, fmt):
    d["in_fmt"] = fmt
    d["in0_bs"] = s16_words(d["C0"], d["H"], d["W"])
    if d.get("in1"):
        d["in1_bs"] = s16_words(d["C1"], d["H"], d["W"])
    return d


def multi(srcs, cout, size, kws=0, **kw):
    """A multi-source descriptor: srcs = [(C, step, oy, ox, KH, KW, padH, padW)], size = (B, OH, OW)."""
    B, OH, OW = size
    d = dict(B=B, OH=OH, OW=OW, H=OH, W=OW, Cout=cout, CoutPad=coutpad(cout), bias=PTR, out=PTR, out_bs=cout * OH * OW, act=ACT_NONE,
             epi=EPI_STORE, mode=F16X3, wpatch16=PTR, wscale16=PTR, guard=PTR, nsrc=len(srcs), src=[])
    for C, step, oy, ox, KH, KW, pH, pW in srcs:
        Hs, Ws = OH * step, OW * step
        d["src"].append(dict(ptr=PTR, bs=s16_words(C, Hs, Ws), C=C, Hs=Hs, Ws=Ws, step=step, oy=oy, ox=ox, KH=KH, KW=KW, padH=pH, padW=pW))
    if kws:
        nout = B * cout * OH * OW
        d.update(kws=PTR, kws_elems=8 * nout if kws == 1 else nout * 3 // 2)
    d.update(kw)
    return d


def parity_sources(C):
    """A 3x3, stride 2, pad 1 convolution as the four pixel-parity classes of its input (include/accflow_hip.h)."""
    return [(C, 2, 0, 0, 1, 1, 0, 0), (C, 2, 0, 1, 1, 2, 0, 1), (C, 2, 1, 0, 2, 1, 1, 0), (C, 2, 1, 1, 2, 2, 1, 1)]


STRIDE = 23   # (coprime with the length of every inner loop below: each value of each factor meets the others' in turn)


def grid():
    """The descriptors, in a fixed order: the stem's, and every STRIDE-th of the crossed factors."""
    g, stem = [], []
    # A: the four arithmetic modes x sources x Cout x kernel x stride x size, no workspace
    for mode in (F32, BF16X3, BF16X6, F16X3):
        for c0, c1 in INPUTS:
            for cout in COUTS:
                for k in KERNELS:
                    for stride in (1, 2):
                        if stride == 2 and k in ((1, 5), (5, 1), (5, 5)):
                            continue
                        for size in SIZES:
                            g.append(plain(mode, c0, c1, cout, k, stride, size))
    # B: a split-K workspace, ample and too small (stride 1: the direct kernel's shapes; 1x1 of 512 channels: the depth rule)
    for mode in (BF16X6, F16X3):
        for c0, c1 in INPUTS + ((512, 0),):
            for cout in COUTS:
                for k in KERNELS if c0 != 512 else ((1, 1),):
                    for size in SIZES:
                        for kws in (1, 2):
                            g.append(plain(mode, c0, c1, cout, k, 1, size, kws))
    # C: S16 inputs (in_fmt 1 and 3), the S16 copy of the output, the channel-block scatter
    for c0, c1, fmt in ((64, 0, 1), (64, 64, 3), (48, 80, 3), (64, 64, 1)):
        for cout in COUTS:
            for k in KERNELS:
                for size in SIZES:
                    for o16 in (0, 1):
                        for kws in (0, 1):
                            d = s16_inputs(plain(F16X3, c0, c1, cout, k, 1, size, kws), fmt)
                            if o16:
                                d.update(out16=PTR, out16_bs=s16_words(cout, d["OH"], d["OW"]))
                            g.append(d)
    for cout in (64, 128, 192, 256, 320):
        for cb in (32, 64, 48):
            for k in ((1, 1), (3, 3)):
                for size in SIZES:
                    for kws in (0, 1):
                        for o16 in (0, 1):
                            d = plain(F16X3, 64, 0, cout, k, 1, size, kws, cb=cb, out_cbs=cb * size[1] * size[2])
                            if o16:
                                d.update(out16=PTR, out16_bs=s16_words(cout, d["OH"], d["OW"]), out16_cbs=s16_words(cb, d["OH"], d["OW"]))
                            g.append(d)
    # D: fp32 input with out16 alone, activations / epilogues that bar the statistics, statistics already requested
    for cout in COUTS:
        for size in SIZES:
            g.append(plain(F16X3, 64, 0, cout, (3, 3), 1, size, out16=PTR, out16_bs=s16_words(cout, size[1], size[2])))
            g.append(plain(F16X3, 64, 0, cout, (3, 3), 1, size, act=ACT_RELU))
            g.append(plain(F16X3, 64, 0, cout, (3, 3), 1, size, epi=EPI_RES_RELU, e0=PTR, e0_bs=cout * size[1] * size[2]))
            g.append(plain(BF16X6, 64, 0, cout, (3, 3), 1, size, stats=PTR, stat_slots=4))
            g.append(plain(F16X3, 64, 0, cout, (3, 3), 1, size, in_norm=PTR))
            g.append(plain(F16X3, 320, 0, cout, (3, 3), 1, size))         # more channels than normalise-on-load takes
            g.append(plain(F16X3, 8, 0, cout, (3, 3), 1, size))           # fewer than the direct kernel takes
            g.append(plain(F16X3, 64, 0, cout, (3, 3), 1, size, wsplit16=0))
            g.append(plain(F16X3, 64, 0, cout, (7, 7), 2, size, wsplit16=0, wpatch=0, wpatch16=0, wscale16=0))
    # E: the encoders' stem (exact descriptor, and near misses), per-item weights, deformable
    for size in ((1, 16, 32), (2, 74, 106), (7, 480, 1024), (1, 120, 256)):
        B, H, W = size
        for mode in (F16X3, BF16X6):
            for cout in (64, 96, 32):
                for pad in (3, 2):
                    d = plain(mode, 3, 0, cout, (7, 7), 2, size, padH=pad, padW=pad)
                    d.update(OH=(H + 6 - 7) // 2 + 1, OW=(W + 6 - 7) // 2 + 1, Kpad=160 if pad == 3 else kpad(3, 7, 7))
                    d["out_bs"] = cout * d["OH"] * d["OW"]
                    stem.append(d)
                    stem.append(dict(d, out16=PTR, out16_bs=s16_words(cout, d["OH"], d["OW"]), act=ACT_RELU))
    for mode in (F32, BF16X3, BF16X6, F16X3):
        for cout in COUTS:
            for size in ((1, 8, 16), (2, 8, 16), (3, 37, 53), (1, 90, 160)):
                B, H, W = size
                P = H * W
                g.append(plain(mode, P, 0, cout, (1, 1), 1, size, kws=1 if B == 1 else 0, wpatch=0, wpatch16=0, wsplit_bs=3 * kpad(P, 1, 1) * coutpad(cout) * 2,
                               epi=EPI_ACCUM, e0=PTR, e0_bs=cout * P))
            for size in SIZES[:3]:
                g.append(plain(mode, 64, 64, cout, (3, 3), 1, size, offset=PTR, dmask=PTR, offset_bs=18 * size[1] * size[2],
                               dmask_bs=9 * size[1] * size[2]))
    # F: multi-source descriptors
    cats = ([(64, 1, 0, 0, 3, 3, 1, 1)], [(64, 1, 0, 0, 3, 3, 1, 1), (32, 1, 0, 0, 3, 3, 1, 1)],
            [(128, 1, 0, 0, 1, 5, 0, 2), (128, 1, 0, 0, 1, 5, 0, 2), (64, 1, 0, 0, 1, 5, 0, 2)],
            [(64, 1, 0, 0, 3, 3, 1, 1), (48, 1, 0, 0, 3, 3, 1, 1), (32, 1, 0, 0, 1, 1, 0, 0), (16, 1, 0, 0, 3, 3, 1, 1)],
            [(4096, 1, 0, 0, 1, 1, 0, 0)], [(64, 1, 0, 0, 7, 7, 3, 3)], [(64, 1, 0, 0, 1, 9, 0, 4)], parity_sources(64), parity_sources(96))
    for srcs in cats:
        for cout in COUTS:
            for size in SIZES:
                for kws in (0, 1, 2):
                    g.append(multi(srcs, cout, size, kws))
                g.append(multi(srcs, cout, size, 1, out16=PTR, out16_bs=s16_words(cout, size[1], size[2])))
                g.append(multi(srcs, cout, size, 1, e0_fmt=1, epi=EPI_RES_RELU, act=ACT_RELU, e0=PTR, e0_bs=s16_words(cout, size[1], size[2])))
                g.append(multi(srcs, cout, size, 0, act=ACT_RELU))
                for lay in (1, 2, 3, 4):
                    d = multi(srcs, cout, size, 1)
                    d["src"][0]["reserved"] = lay
                    g.append(d)
    for C in (64, 96):
        for c0 in (64, 96, 128):
            for c1 in (64, 96, 128, 192):
                for size in SIZES:
                    for act in (ACT_NONE, ACT_RELU):
                        g.append(multi(parity_sources(C), c0 + c1, size, 1, split_c0=c0, act=act))
    return g[::STRIDE] + stem


def grid_hash(g):
    return hashlib.sha256(json.dumps(g, sort_keys=True).encode()).hexdigest()


def to_desc(fields):
    from accflow_amd import _lib
    d = _lib.ConvDesc()
    for k, v in fields.items():
        if k == "src":
            for i, s in enumerate(v):
                for sk, sv in s.items():
                    setattr(d.src[i], sk, sv)
        else:
            setattr(d, k, v)
    return d


def query(g):
    """The two answers of the loaded library (ACCFLOW_HIP_LIB or the in-tree build) for every descriptor of g."""
    from accflow_amd import _lib
    lib = _lib.load()
    slots, norm = [], []
    for fields in g:
        d = to_desc(fields)
        slots.append(lib.accflow_conv_stat_slots(ctypes.byref(d)))
        norm.append(lib.accflow_conv_in_norm_supported(ctypes.byref(d)))
    return {"slots": slots, "norm": norm}


def query_in_child(env):
    """One fresh process per environment: the library reads its routing switches once."""
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=e, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("route query child failed (%d):\n%s" % (r.returncode, r.stderr[-4000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def dump(doc):
    """One array per line."""
    lines = ['{"grid_sha256":"%s","n":%d,"answers":{' % (doc["grid_sha256"], doc["n"])]
    for i, (k, v) in enumerate(doc["answers"].items()):
        lines.append('"%s":{"slots":%s,' % (k, json.dumps(v["slots"], separators=(",", ":"))))
        lines.append('"norm":%s}%s' % (json.dumps(v["norm"], separators=(",", ":")), "," if i + 1 < len(doc["answers"]) else ""))
    return "\n".join(lines) + "\n}}\n"


def env_key(env):
    return ",".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


if __name__ == "__main__":
    if "--child" in sys.argv:
        print(json.dumps(query(grid())))
    else:
        g = grid()
        doc = {"grid_sha256": grid_hash(g), "n": len(g), "answers": {env_key(e): query_in_child(e) for e in ENVS}}
        with open(OUT, "w") as f:
            f.write(dump(doc))
        print("%d descriptors x %d environments -> %s (%d bytes)" % (len(g), len(ENVS), OUT, os.path.getsize(OUT)))
