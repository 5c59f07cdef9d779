"""AccFlow backward accumulation on gfx950 kernels.

Mirrors the reference's networks/AccFlow_.py: `AccFlow(ofe).forward(images, test_mode=False)` returns
[F(2->0), F(3->0), ..., F(n-1->0)] (AccFlow_.py:157-175), `iter(I1, I2, In, F2n)` one accumulation step
(:177-201); sub-modules FlowDecoder (:13-45), FlowEncoder (:48-65), AccPlus (:68-109), Blending
(:112-124), functions getOcc (:127-135), downflow8 (:138-142); identical state_dict.

The deformable convolution (torchvision.ops.DeformConv2d in the reference, AccFlow_.py:83,104) is the
deformable mode of accflow_conv2d_f32; its parameters live in a plain container with the same names
(`dconv.weight`, `dconv.bias`).

Scheduling (exact): `forward` evaluates all estimator pairs of the sequence in ONE batched
call - they are independent because the reference never passes flow_init (AccFlow_.py:184,188) - with each
frame encoded once, and runs the context encoder once per frame; only the fusion chain is sequential.
"""
import contextlib
import functools
import itertools
import math
import os
import threading
import types

import torch
import torch.nn as nn

from .. import ops
from ..parallel import run_pair_sharded, run_pair_sharded_stream, world
from ._packs import PackCache, require_cuda, span
from .modules import ZeroConv2d
from .raft.extractor import BasicEncoder

USE_S16_CHAIN = os.environ.get("ACCFLOW_S16_CHAIN", "1") == "1"   # (0: the round-3 fusion chain on fp32 activations, A/B)
CONTEXT_SIDE_STREAM = os.environ.get("ACCFLOW_CONTEXT_STREAM", "1") == "1"   # (0: context encoder in the serial section, A/B)
# FlowEncoder of flow_ini / dflow, the occlusion / error maps and the blending mask of ALL fusion steps evaluated in one batch ahead
# of the sequential loop (_StepInputs over all steps; they do not depend on the accumulated flow).  Measured
# (profiles/r04_ab_chain_hoist.txt): -0.3 ms for one sequence at a time, nothing (+0.1 ms) when the chain runs underneath the
# next sequence's estimator, whose kernels fill the batch-1 steps' idle slots anyway.  "auto": on, except inside
# parallel.SequencePipeline; "1" / "0": always / never (A/B).
USE_CHAIN_HOIST = os.environ.get("ACCFLOW_CHAIN_HOIST", "auto")
_CHAIN_TLS = threading.local()


# The fusion chain of a PIPELINED sequence (another sequence's estimator fills the chip next to it) runs its batch-1
# convolutions without split-K: 21.66 -> 21.43 ms per step (profiles/r06_ab_chain_ksplit.txt); 1: split-K there too (rounds 2-5)
PIPELINE_CHAIN_KSPLIT = os.environ.get("ACCFLOW_PIPELINE_CHAIN_KSPLIT", "0") == "1"


@contextlib.contextmanager
def chain_in_pipeline():
    """Marks the enclosed fuse_chain call as running concurrently with another sequence's estimator (SequencePipeline)."""
    prev = (getattr(_CHAIN_TLS, "pipelined", False), getattr(_CHAIN_TLS, "no_ksplit", False))
    _CHAIN_TLS.pipelined, _CHAIN_TLS.no_ksplit = True, not PIPELINE_CHAIN_KSPLIT
    try:
        yield
    finally:
        _CHAIN_TLS.pipelined, _CHAIN_TLS.no_ksplit = prev


@contextlib.contextmanager
def pipeline_chain_arithmetic():
    """model(images) inside this scope computes the fusion chain with the arithmetic of the pipelined modes (no split-K in its
    batch-1 convolutions: another order of the same fp32 sums) - what SequencePipeline's outputs equal bit for bit."""
    prev = getattr(_CHAIN_TLS, "no_ksplit", False)
    _CHAIN_TLS.no_ksplit = not PIPELINE_CHAIN_KSPLIT
    try:
        yield
    finally:
        _CHAIN_TLS.no_ksplit = prev


def launch_chain_aside(model, images, by_pair, ready, flag, other_flags=None):
    """model.fuse_chain(images, by_pair) as a chain_in_pipeline on the device's side stream, behind the event `ready` of the
    estimator that made by_pair (parallel.SequencePipeline, AccFlow.forward_pair_sharded_stream).  flag: the device int32
    the chain's f16x3 kernels report range violations to, None in the other modes; other_flags: the other ranks' flags of
    the same sequence.  Their sum goes to pinned memory behind the chain: no host synchronisation.  -> (done event, pinned
    sum or None, outputs); the caller appends a tuple that starts with `images` and keeps alive what it allocated on its
    own stream and the chain reads: harvest_chain_aside's handle."""
    dev = images[0].device
    main = torch.cuda.current_stream(dev)
    side = _context_stream(dev)
    side.wait_event(ready)
    host = None
    with torch.cuda.stream(side), chain_in_pipeline(), (ops.guard_scope(flag) if flag is not None else contextlib.nullcontext()):
        outs = model.fuse_chain(images, by_pair)
        if flag is not None:
            tripped = flag
            if other_flags:
                tripped = flag + (torch.cat([f.reshape(-1) for f in other_flags]) != 0).sum().to(torch.int32)
            host = torch.empty(1, dtype=torch.int32, pin_memory=True)
            host.copy_(tripped, non_blocking=True)
        done = torch.cuda.Event()
        done.record(side)
    # the outputs live in blocks of the SIDE stream's allocator pool but are consumed by the caller on `main`
    # (whatever stream that is): tell the allocator, so that freeing them while the caller's kernels still read
    # them cannot hand the block to the next chain (the harvest only synchronises the HOST with the chain)
    for o in outs:
        o.record_stream(main)
    return done, host, outs


def harvest_chain_aside(model, handle, trip_name=None):
    """The outputs of a handle (see launch_chain_aside), once its chain has finished.  A value left the fp16 split's range:
    this sequence again in bf16x6, listed in ops.guard_report() as trip_name if one is given."""
    done, host, outs, keep = handle
    done.synchronize()
    if host is not None and int(host.item()):
        if trip_name is not None:
            ops.note_guard_trip(trip_name)
        with ops.conv_mode(ops.CONV_BF16X6), pipeline_chain_arithmetic():    # (every output of the pipelined modes: one arithmetic)
            outs = model(images=keep[0])
    return outs


def flows_by_pair(small, pairs):
    """estimate_small's pair-major (len(pairs) * N, 2, h, w) flows as {pair: (N, 2, h, w)}"""
    N = small.shape[0] // len(pairs)
    return {p: small[k * N:(k + 1) * N] for k, p in enumerate(pairs)}


def _hoist_now():
    if USE_CHAIN_HOIST == "auto":
        return not getattr(_CHAIN_TLS, "pipelined", False)
    return USE_CHAIN_HOIST == "1"


USE_CHAIN_DEFER_UP = os.environ.get("ACCFLOW_CHAIN_DEFER_UP", "1") == "1"   # (0: every fusion step upsamples its own flow, A/B)
_CTX_STREAMS = {}


def _context_stream(device):
    """ONE side stream per device for the context encoder / the fusion chain of the pipelined modes: with the caller's stream
    and the estimator's two pair-group streams that makes 4 - the number of hardware queues HIP maps streams onto.  Every
    further stream of the process shares a queue with one of these and serialises with it whenever both are busy (round 6:
    a second pair of group streams cost 6 ms per sequence, profiles/r06_ab_group_priority.txt), so parallel.SequencePipeline
    and forward_pair_sharded_stream use THIS stream for their chains instead of creating their own."""
    key = str(device)
    if key not in _CTX_STREAMS:
        _CTX_STREAMS[key] = torch.cuda.Stream(device=device)
    return _CTX_STREAMS[key]


class FlowDecoder(nn.Module):
    def __init__(self, cin=128):
        super().__init__()
        self.flow = nn.Sequential(nn.Conv2d(cin, cin * 2, 3, 1, 1), nn.ReLU(True), nn.Conv2d(cin * 2, 2, 3, 1, 1))
        self.mask = nn.Sequential(nn.Conv2d(cin, cin * 2, 3, 1, 1), nn.ReLU(True), nn.Conv2d(cin * 2, 64 * 9, 1, 1, 0))
        self._packs = PackCache()

    def upsample_flow(self, flow, mask):
        require_cuda(flow, mask)
        return ops.convex_upsample(flow.float(), mask.float())

    @torch.no_grad()
    @ops.range_guarded
    def forward(self, x):
        require_cuda(x)
        pk = self._packs
        if ops.s16_active() and USE_S16_CHAIN:
            return self._forward16(ops.to_s16(x.float()))
        t = ops.conv2d(pk.conv("f0", self.flow[0]), x, act=ops.ACT_RELU)
        flow_small = ops.conv2d(pk.conv("f2", self.flow[2]), t)
        t = ops.conv2d(pk.conv("m0", self.mask[0]), x, act=ops.ACT_RELU, out=t)
        mask = ops.conv2d(pk.conv("m2", self.mask[2]), t)  # no 0.25 factor here (AccFlow_.py:42-43)
        return flow_small, ops.convex_upsample(flow_small, mask)

    def _forward16(self, x16):
        """Pre-split form: the first convolutions of the flow and the mask head read the same tensor - ONE 128 -> 512
        convolution (multi-source kernel), its two halves feeding the 2-channel regression (all taps as a 1x1 on the matrix
        cores + tap sum) and the 1x1 mask convolution."""
        pk = self._packs
        B, _, h, w = x16.shape
        c2 = self.flow[0].out_channels
        t16 = ops.S16.empty(B, 2 * c2, h, w, x16.device)
        ops.conv2d_multi(pk.multi_cat("fm0", [self.flow[0], self.mask[0]]), [x16], act=ops.ACT_RELU, out16=t16, fp32_out=False)
        flow_small = ops.conv2d(pk.conv("f2", self.flow[2]), t16.channels(0, c2))
        mask = ops.conv2d_multi(pk.multi("m2m", self.mask[2]), [t16.channels(c2, 2 * c2)])   # no 0.25 factor (AccFlow_.py:42-43)
        return flow_small, ops.convex_upsample(flow_small, mask)

    def flow16(self, x16, out=None):
        """The flow head alone (AccFlow_.py:40): what the NEXT fusion step needs of this one."""
        pk = self._packs
        B, _, h, w = x16.shape
        t16 = ops.S16.empty(B, self.flow[0].out_channels, h, w, x16.device)
        ops.conv2d_multi(pk.multi("f0m", self.flow[0]), [x16], act=ops.ACT_RELU, out16=t16, fp32_out=False)
        return ops.conv2d(pk.conv("f2", self.flow[2]), t16, out=out)

    def upsample16(self, x16, flow_small):
        """The mask head and the convex upsampling (AccFlow_.py:41-45) of a batch of fused features - the part of the
        decoder no later fusion step depends on."""
        pk = self._packs
        B, _, h, w = x16.shape
        t16 = ops.S16.empty(B, self.mask[0].out_channels, h, w, x16.device)
        ops.conv2d_multi(pk.multi("m0m", self.mask[0]), [x16], act=ops.ACT_RELU, out16=t16, fp32_out=False)
        mask = ops.conv2d_multi(pk.multi("m2m", self.mask[2]), [t16])   # no 0.25 factor (AccFlow_.py:42-43)
        return ops.convex_upsample(flow_small, mask)


class FlowEncoder(nn.Module):
    def __init__(self, c=128):
        super().__init__()
        self.conv1 = nn.Conv2d(2, c, 7, stride=1, padding=3)
        self.conv2 = nn.Conv2d(c, c * 2, 3, stride=1, padding=1)
        self.conv3 = nn.Conv2d(c * 2, c, 1, stride=1, padding=0)
        self.relu = nn.ReLU(True)
        self._packs = PackCache()

    @torch.no_grad()
    @ops.range_guarded
    def forward(self, x):
        is_list = isinstance(x, (tuple, list))
        if is_list:
            batch_dim = x[0].shape[0]
            x = torch.cat(x, dim=0)
        require_cuda(x)
        pk = self._packs
        if ops.s16_active() and USE_S16_CHAIN:
            x = self.encode16(x.float().contiguous())[0]
        else:
            x = ops.conv2d(pk.conv("1", self.conv1), x.float().contiguous(), act=ops.ACT_RELU)
            x = ops.conv2d(pk.conv("2", self.conv2), x, act=ops.ACT_RELU)
            x = ops.conv2d(pk.conv("3", self.conv3), x)
        if is_list:
            x = torch.split(x, batch_dim, dim=0)
        return x

    def encode16(self, flows):
        """(B, 2, h, w) flows -> (fp32 features, ops.S16 features): the 7x7 convolution of the 2-channel flow as a 1x7 one
        over its row-shifted 16-channel stack (ops.flow_from_coords_s16, the form RAFT's convf1 takes), every conv -> conv
        tensor pre-split."""
        pk = self._packs
        B, _, h, w = flows.shape
        dev = flows.device
        c = self.conv1.out_channels
        stack16 = ops.S16.empty(B, 16, h, w, dev)
        ops.flow_from_coords_s16(flows, None, None, stack16, None, 0, is_flow=True)
        a16 = ops.S16.empty(B, c, h, w, dev)
        ops.conv2d(pk.conv("1s", self.conv1, rows_as_channels=True), stack16, act=ops.ACT_RELU, out16=a16, fp32_out=False)
        b16 = ops.S16.empty(B, 2 * c, h, w, dev)
        ops.conv2d_multi(pk.multi("2m", self.conv2), [a16], act=ops.ACT_RELU, out16=b16, fp32_out=False)
        o16 = ops.S16.empty(B, c, h, w, dev)
        out = ops.conv2d_multi(pk.multi("3m", self.conv3), [b16], out16=o16)
        return out, o16


class DeformConv2d(nn.Module):
    """Parameter container with torchvision.ops.DeformConv2d's names / shapes / default init
    (3x3, stride 1, pad 1, one offset group); evaluated by the deformable mode of the HIP conv."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1):
        super().__init__()
        if (kernel_size, stride, padding) != (3, 1, 1):
            raise NotImplementedError("AccPlus uses DeformConv2d(c, c, 3, 1, 1) (AccFlow_.py:83)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = (3, 3), (1, 1), (1, 1)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        self.bias = nn.Parameter(torch.empty(out_channels))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1 / math.sqrt(in_channels * 9)
        nn.init.uniform_(self.bias, -bound, bound)


class AccPlus(nn.Module):
    def __init__(self, c=128):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(c * 2 + 1, c * 2, 3, 1, 1), nn.ReLU(True), nn.Conv2d(c * 2, c, 3, 1, 1))
        self.conv2 = nn.Sequential(nn.Conv2d(c * 2, c * 2, 3, 1, 1), nn.ReLU(True), nn.Conv2d(c * 2, c, 3, 1, 1),
                                   nn.ReLU(True), ZeroConv2d(c, 3 ** 3))
        self.dconv = DeformConv2d(c, c, 3, 1, 1)
        self.conv3 = nn.Sequential(nn.Conv2d(c * 2 + 1, c * 2, 3, 1, 1), nn.ReLU(True), nn.Conv2d(c * 2, c, 3, 1, 1))
        self.conv4 = nn.Sequential(nn.Conv2d(c * 4, c * 2, 3, 1, 1), nn.ReLU(True), nn.Conv2d(c * 2, c, 3, 1, 1),
                                   nn.ReLU(True), nn.Conv2d(c, c, 1, 1, 0))
        self.c = c
        self._packs = PackCache()

    @torch.no_grad()
    @ops.range_guarded
    def forward(self, df, f, o, c):
        """AccFlow_.py:97-109.  Concats are laid out as channel slices of shared buffers:
        A = [df | f | o] (2c+1), G = [x | c | f_ | df] (4c), E = [f_ | df | o] (2c+1)."""
        require_cuda(df, f, o, c)
        if ops.s16_active() and USE_S16_CHAIN:
            return self.forward16(ops.to_s16(df.float()), f.float().contiguous(), ops.to_s16(f.float()), ops.to_s16(o.float()),
                                  ops.to_s16(c.float()))
        pk, C = self._packs, self.c
        B, _, h, w = df.shape
        dev = df.device

        def buf(ch):
            return torch.empty((B, ch, h, w), dtype=torch.float32, device=dev)

        A, E, G, X2 = buf(2 * C + 1), buf(2 * C + 1), buf(4 * C), buf(2 * C)
        ops.copy_into(df.float(), A[:, :C]); ops.copy_into(f.float(), A[:, C:2 * C]); ops.copy_into(o.float(), A[:, 2 * C:])
        ops.copy_into(c.float(), X2[:, C:]); ops.copy_into(c.float(), G[:, C:2 * C])
        ops.copy_into(df.float(), G[:, 3 * C:]); ops.copy_into(df.float(), E[:, C:2 * C]); ops.copy_into(o.float(), E[:, 2 * C:])
        t = ops.conv2d(pk.conv("1a", self.conv1[0]), A, act=ops.ACT_RELU)
        ops.conv2d(pk.conv("1b", self.conv1[2]), t, out=X2[:, :C])
        t = ops.conv2d(pk.conv("2a", self.conv2[0]), X2, act=ops.ACT_RELU, out=t)
        u = ops.conv2d(pk.conv("2b", self.conv2[2]), t, act=ops.ACT_RELU)
        zc = self.conv2[4]
        # ZeroConv2d (modules.py:94-96) with exp(3*scale) folded; sigmoid applies to the 9 mask channels only
        om = ops.conv2d(pk.conv("2z", zc.conv, scale=zc.out_scale, scale_dep=zc.scale), u)
        off, msk = om[:, :18], ops.activation_(om[:, 18:], ops.ACT_SIGMOID)  # split [18, 9] (:102-103)
        f_ = ops.conv2d(pk.conv("dc", self.dconv_as_conv(), tap_major=True), A[:, C:2 * C], out=E[:, :C],
                        offset=off, dmask=msk)
        ops.copy_into(f_, G[:, 2 * C:3 * C])
        t = ops.conv2d(pk.conv("3a", self.conv3[0]), E, act=ops.ACT_RELU, out=t)
        ops.conv2d(pk.conv("3b", self.conv3[2]), t, out=G[:, :C])
        t = ops.conv2d(pk.conv("4a", self.conv4[0]), G, act=ops.ACT_RELU, out=t)
        u = ops.conv2d(pk.conv("4b", self.conv4[2]), t, act=ops.ACT_RELU, out=u)
        return ops.conv2d(pk.conv("4c", self.conv4[4]), u)

    def forward16(self, df16, f, f16, o16, c16):
        """AccFlow_.py:97-109 on pre-split tensors: every torch.cat([...], 1) is the source list of ONE multi-source
        convolution (accflow_conv_desc.src: cat[df, f, o], cat[x, c], cat[f_, df, o], cat[x, c, f_, df] - nothing is
        copied), every conv -> conv tensor exists as ops.S16 only.  f is needed in fp32 as well: the deformable
        convolution samples it bilinearly."""
        pk, C = self._packs, self.c
        B, _, h, w = f.shape
        dev = f.device
        R = ops.ACT_RELU

        def s16(ch):
            return ops.S16.empty(B, ch, h, w, dev)

        t16, x16, u16, f_16, y16 = s16(2 * C), s16(C), s16(C), s16(C), s16(C)
        ops.conv2d_multi(pk.multi("1a", self.conv1[0], splits=[C, C, 1]), [df16, f16, o16], act=R, out16=t16, fp32_out=False)
        ops.conv2d_multi(pk.multi("1b", self.conv1[2]), [t16], out16=x16, fp32_out=False)
        ops.conv2d_multi(pk.multi("2a", self.conv2[0], splits=[C, C]), [x16, c16], act=R, out16=t16, fp32_out=False)
        ops.conv2d_multi(pk.multi("2b", self.conv2[2]), [t16], act=R, out16=u16, fp32_out=False)
        zc = self.conv2[4]
        # ZeroConv2d (modules.py:94-96) with exp(3*scale) folded; sigmoid applies to the 9 mask channels only
        om = ops.conv2d_multi(pk.multi("2z", zc.conv, scale=zc.out_scale, scale_dep=zc.scale), [u16])
        # split [18, 9] (:102-103); the sigmoid of the 9 modulation channels is applied by the columns kernel while sampling
        ops.deform_conv2d_s16(pk.conv("dc", self.dconv_as_conv(), tap_major=True), f, om[:, :18], om[:, 18:], f_16,
                              mask_is_logit=True)
        ops.conv2d_multi(pk.multi("3a", self.conv3[0], splits=[C, C, 1]), [f_16, df16, o16], act=R, out16=t16, fp32_out=False)
        ops.conv2d_multi(pk.multi("3b", self.conv3[2]), [t16], out16=y16, fp32_out=False)
        ops.conv2d_multi(pk.multi("4a", self.conv4[0], splits=[C, C, C, C]), [y16, c16, f_16, df16], act=R, out16=t16,
                         fp32_out=False)
        ops.conv2d_multi(pk.multi("4b", self.conv4[2]), [t16], act=R, out16=u16, fp32_out=False)
        return ops.conv2d_multi(pk.multi("4c", self.conv4[4]), [u16])

    def dconv_as_conv(self):
        return _ConvView(self.dconv)


class _ConvView:
    """Presents DeformConv2d's parameters with the attribute names PackCache.conv reads."""

    def __init__(self, d):
        self.weight, self.bias, self.stride, self.padding = d.weight, d.bias, d.stride, d.padding


class Blending(nn.Module):
    def __init__(self, c=128):
        super().__init__()
        self.mask = nn.Sequential(nn.Conv2d(c, c * 2, 1, 1, 0), nn.ReLU(True), nn.Conv2d(c * 2, 1, 3, 1, 1), nn.Sigmoid())
        self._packs = PackCache()

    def mask16(self, emap):
        """The blending mask alone (AccFlow_.py:119-121, S16 path): it depends on the error map only, so AccFlow.fuse_chain
        evaluates it for all steps of a sequence in one batch."""
        pk = self._packs
        e16 = emap if isinstance(emap, ops.S16) else ops.to_s16(emap.float())    # (the chain hands the map over pre-split)
        B, _, h, w = e16.shape
        t16 = ops.S16.empty(B, self.mask[0].out_channels, h, w, e16.device)
        ops.conv2d_multi(pk.multi("0m", self.mask[0]), [e16], act=ops.ACT_RELU, out16=t16, fp32_out=False)
        return ops.conv2d(pk.conv("2", self.mask[2]), t16, act=ops.ACT_SIGMOID)

    @torch.no_grad()
    @ops.range_guarded
    def forward(self, f1, f2, emap):
        require_cuda(f1, f2, emap)
        pk = self._packs
        if ops.s16_active() and USE_S16_CHAIN:
            m = self.mask16(emap)
        else:
            t = ops.conv2d(pk.conv("0", self.mask[0]), emap.float(), act=ops.ACT_RELU)
            m = ops.conv2d(pk.conv("2", self.mask[2]), t, act=ops.ACT_SIGMOID)
        return ops.blend(f1.float().contiguous(), f2.float().contiguous(), m)


def getOcc(F12, I1, I2, binary=True):
    """AccFlow_.py:127-135: 1 where mean_c |I1 - backwarp(I2, F12)| <= 1 (binary) or the per-channel
    absolute error map."""
    require_cuda(F12, I1, I2)
    return ops.get_occ(F12.float(), I1.float(), I2.float(), binary=binary)


def downflow8(flow, mode="bilinear"):
    """AccFlow_.py:138-142."""
    if mode != "bilinear":
        raise NotImplementedError("downflow8: bilinear only")
    require_cuda(flow)
    h, w = flow.shape[-2:]
    assert h % 8 == 0 and w % 8 == 0
    return ops.downflow8(flow.float().contiguous())


class _StepInputs:
    """What the pre-split fusion step (AccFlow._fuse16) reads that does not depend on the accumulated flow F2n
    (AccFlow_.py:191-200): f_ini, the FlowEncoder features of flow_ini (fp32); df16, those of dflow; o16, the occlusion map;
    mask, the blending mask.  The maps are read by convolutions only: their producers write them PRE-SPLIT (round 6).
    Each member is computed where it is first read.  The stepwise chain makes one holder per step: FlowEncoder takes
    [flow_ini, dflow, F2n] as one batch of 3N and every map is made right in front of its reader.  The hoisted chain makes
    ONE over the K = (n - 2) N items of all steps and reads every member ahead of the sequential loop - FlowEncoder, one batch
    of 2K, getOcc x 2, Blending.mask16 - and hands each step its items(); per step there remain FlowEncoder(F2n), AccPlus,
    the blend and the decoder.  Same operators on the same values, no added work.  (Convolving the df / o / c members of
    AccPlus's concatenations ahead of the loop as partial sums: built in round 4, no gain
    (profiles/r04_ab_chain_prefold.txt), removed in round 6.)"""

    def __init__(self, acc, flow_ini, dflow, c1, c2, cn):
        self.acc, self.c1, self.c2, self.cn = acc, c1, c2, cn
        self.flow_ini, self.dflow = flow_ini.float().contiguous(), dflow.float().contiguous()

    def encode(self, F2n=None):
        """FlowEncoder over flow_ini, dflow and - in the same batch - F2n -> F2n's features (fp32, pre-split)"""
        K = self.dflow.shape[0]
        flows = torch.cat([self.flow_ini, self.dflow] + ([] if F2n is None else [F2n]), dim=0)
        feats, feats16 = self.acc.flow_encoder.encode16(flows)
        self.f_ini, self.df16 = feats[:K], feats16.batch(K, 2 * K)
        return None if F2n is None else (feats[2 * K:], feats16.batch(2 * K, 3 * K))

    def _map16(self, flow, i2, binary):
        K, _, h, w = flow.shape
        out16 = ops.S16.empty(K, 1 if binary else self.c1.shape[1], h, w, flow.device)
        return ops.get_occ(flow, self.c1, i2, binary=binary, out16=out16)

    @functools.cached_property
    def o16(self):
        return self._map16(self.dflow, self.c2, True)

    @functools.cached_property
    def mask(self):
        return self.acc.blending.mask16(self._map16(self.flow_ini, self.cn, False))

    def items(self, k0, k1):
        """Items k0 .. k1 of a holder computed ahead: a step with these encodes F2n alone."""
        return types.SimpleNamespace(encode=self.acc.flow_encoder.encode16, f_ini=self.f_ini[k0:k1], df16=self.df16.batch(k0, k1),
                                     o16=self.o16.batch(k0, k1), mask=self.mask[k0:k1])


class AccFlow(nn.Module):
    """warm_start (build extension, default off = the reference's behaviour): SURVEY 8(f)#2 / the reference README's
    open TODO "Add warmstart mode" on top of RAFT's `flow_init` (raft.py:123-124).  The long-range estimate i -> 0 of
    step i is seeded with the composition of the adjacent flow i -> i-1 and the flow i-1 -> 0 accumulated so far
    (both at 1/8 resolution: seed = F(i->i-1) + backwarp(F(i-1->0), F(i->i-1))) and refined for `warm_iters`
    iterations (default: the estimator's 12).  The adjacent pairs stay one batched call; the long-range pairs become
    sequential with the fusion chain.  oracle.accflow_forward_warm is the CPU restatement."""

    def __init__(self, ofe: nn.Module, warm_start=False, warm_iters=None):
        super().__init__()
        self.warm_start = bool(warm_start)
        self.warm_iters = warm_iters
        self.ofe: nn.Module = ofe
        self.hidden_channel = 128
        self.flow_encoder = FlowEncoder(self.hidden_channel)
        self.flow_decoder = FlowDecoder(self.hidden_channel)
        self.context = BasicEncoder(3, output_dim=self.hidden_channel, norm_fn="none")
        self.accplus = AccPlus(self.hidden_channel)
        self.blending = Blending(self.hidden_channel)
        self.mixed_precision = True

    # ---- one fusion step given all its inputs (AccFlow_.py:191-201) -----------------------------
    def _fuse(self, dflow, flow_ini, F2n, c1, c2, cn):
        """The module-form step, the reference's iter body: iter(), the warm-start schedule and the chain on fp32 activations."""
        f_ini, df, f = self.flow_encoder([flow_ini, dflow, F2n])
        o = getOcc(dflow, c1, c2)
        f_acc = self.accplus(df, f, o, c1)
        emap = getOcc(flow_ini, c1, cn, binary=False)
        f_fuse = self.blending(f_ini, f_acc, emap)
        return self.flow_decoder(f_fuse)

    def _fuse16(self, inputs, F2n, c1_16, x16, small=None):
        """The pre-split step: every chain of the f16x3 mode.  inputs: _StepInputs, where the order of the launches in front
        of AccPlus and of the blend is decided; x16: where the fused features go.  small: the decoder's flow head alone
        writes the 1/8-resolution flow there, returns (small, None) - the caller upsamples all steps in one batch."""
        f, f16 = inputs.encode(F2n)
        f_acc = self.accplus.forward16(inputs.df16, f, f16, inputs.o16, c1_16)
        ops.blend(inputs.f_ini, f_acc, inputs.mask, out16=x16)
        if small is not None:
            return self.flow_decoder.flow16(x16, out=small), None
        return self.flow_decoder._forward16(x16)

    @torch.no_grad()
    @ops.range_guarded
    def iter(self, I1, I2, In, F2n):
        """input: I1, I2, IN; F2N (1/8 size) -> F1N_small (1/8 size), F1N   (AccFlow_.py:177-201)"""
        require_cuda(I1, I2, In)
        if F2n is None:
            flows = downflow8(self.ofe(torch.cat([I1, I1, I2]), torch.cat([I2, In, In])))
            dflow, flow_ini, F2n = flows.chunk(3)
        else:
            flows = downflow8(self.ofe(torch.cat([I1, I1]), torch.cat([I2, In])))
            dflow, flow_ini = flows.chunk(2)
        c1, c2, cn = self.context([I1, I2, In])
        out_small, out = self._fuse(dflow.contiguous(), flow_ini.contiguous(), F2n.float().contiguous(), c1, c2, cn)
        return out_small.float(), out.float()

    @staticmethod
    def pair_schedule(n_frames):
        """Estimator pairs (i -> j) the reference evaluates for an n-frame sequence, in its order
        (AccFlow_.py:167-190): step 2 -> (2,1),(2,0),(1,0); step i>2 -> (i,i-1),(i,0)."""
        pairs = []
        for i in range(2, n_frames):
            pairs += [(i, i - 1), (i, 0)]
            if i == 2:
                pairs.append((1, 0))
        return pairs

    @torch.no_grad()
    def estimate_small(self, images, pairs, flow_init=None, iters=None, features=None):
        """1/8-resolution estimator flows of `pairs`, (len(pairs)*N, 2, H/8, W/8), pair-major."""
        iters = getattr(self, "ofe_iters", 12) if iters is None else iters
        if hasattr(self.ofe, "estimate_pairs"):
            flows = self.ofe.estimate_pairs(images, pairs, iters=iters, flow_init=flow_init, features=features)
        else:  # any estimator with the reference signature
            flows = self.ofe(torch.cat([images[i] for i, _ in pairs]), torch.cat([images[j] for _, j in pairs]),
                             iters=iters, flow_init=flow_init)
        return downflow8(flows)

    def context_of(self, images, want16=True):
        """The context encoder's features per frame; want16: (fp32 features, pre-split features or None), what fuse_chain takes."""
        return self.context([im.float().contiguous() for im in images], want16=want16)

    # ---- the context encoder does not depend on any flow (AccFlow_.py:191: c1, c2, cn = self.context([I1, I2, In])): it runs
    # on a side stream UNDERNEATH the estimator of the same sequence instead of in the serial section behind it
    def context_async(self, images):
        """Start the per-frame context encoding on the side stream; returns a handle for context_join."""
        dev = images[0].device
        main = torch.cuda.current_stream(dev)
        side = _context_stream(dev)
        side.wait_stream(main)          # the images / the weights' packs, and every earlier reader of this pool's blocks
        # the encoder runs concurrently with the estimator's guarded stages, so it reports range violations of the f16x3
        # mode to a flag of its own (read at the join) instead of the thread's shared one
        guarded = ops.current_mode() == ops.CONV_F16X3 and not ops.inside_guard()
        with torch.cuda.stream(side):
            flag = torch.zeros(1, dtype=torch.int32, device=dev) if guarded else None
            with (ops.guard_scope(flag) if guarded else contextlib.nullcontext()):
                ctx = self.context_of(images)
        return (side, ctx, flag, images)

    def context_join(self, handle):
        side, ctx, flag, images = handle
        main = torch.cuda.current_stream(ctx[0][0].device)
        main.wait_stream(side)
        if flag is not None and int(flag.item()):        # the context stage alone falls back to bf16x6 (on this stream)
            ops.note_guard_trip("AccFlow.context")
            with ops.conv_mode(ops.CONV_BF16X6):
                return self.context_of(images)
        # the outputs live in blocks of the side stream's allocator pool and are read on `main`: tell the allocator, so that
        # freeing them cannot hand a block to another side-stream allocation while main's kernels still read it
        for t in list(ctx[0]) + [t.data for t in ctx[1] or ()]:
            t.record_stream(main)
        return ctx

    def estimate_with_context(self, images, pairs, ctx_images=None, **estimator):
        """estimate_small(images, pairs, **estimator) with the context encoder of ctx_images (default: all of them) underneath
        it on the side stream - behind it on this stream with CONTEXT_SIDE_STREAM off.  -> ({pair: flow}, context features)"""
        ctx_images = images if ctx_images is None else ctx_images
        handle = self.context_async(ctx_images) if CONTEXT_SIDE_STREAM else None
        small = self.estimate_small(images, pairs, **estimator)
        ctx = self.context_join(handle) if handle is not None else self.context_of(ctx_images)
        return flows_by_pair(small, pairs), ctx

    @torch.no_grad()
    @ops.range_guarded
    def fuse_chain(self, images, by_pair, ctx=None, return_small=False):
        """The sequential part of AccFlow.forward: by_pair[(i, j)] = (N,2,H/8,W/8) flow i -> j.  ctx: the context
        encoder's outputs if the caller computed them already (context_async / context_join).  return_small: (outputs, the
        decoder's 1/8-resolution flow of the LAST step) - what the next step of a longer chain starts from (AccFlowStream);
        the launches are the same either way."""
        if ctx is None:
            ctx = self.context_of(images)
        # (chain_in_pipeline / pipeline_chain_arithmetic: the chain proper only)
        with (ops.ksplit_scope(False) if getattr(_CHAIN_TLS, "no_ksplit", False) else contextlib.nullcontext()):
            return self._fuse_chain(images, by_pair, ctx, return_small)

    def _fuse_chain(self, images, by_pair, ctx, return_small=False):
        """One loop over the steps i = 2 .. n-1, each from the 1/8-resolution flow F2n of the one before.  In the f16x3 mode
        the steps are pre-split (_fuse16); with more than one step, what does not depend on F2n is hoisted out of the loop
        (_hoist_now: one _StepInputs over all steps) and what no later step reads is deferred behind it (USE_CHAIN_DEFER_UP)."""
        n = len(images)
        ctx, ctx16 = ctx
        outs, F2n = [], by_pair[(1, 0)]
        (N, _, h, w), dev = F2n.shape, F2n.device
        s16 = ctx16 is not None and ops.s16_active() and USE_S16_CHAIN
        hoist = s16 and n > 3 and _hoist_now()
        defer = s16 and n > 3 and USE_CHAIN_DEFER_UP
        steps = range(2, n)
        if hoist:
            # (views, not copies: the per-frame context features are consecutive slices of ONE encoder output)
            cn = ctx[0].expand(len(steps), -1, -1, -1) if N == 1 else ctx[0].repeat(len(steps), 1, 1, 1)
            ahead = _StepInputs(self, torch.cat([by_pair[(i, 0)] for i in steps], dim=0),
                                torch.cat([by_pair[(i, i - 1)] for i in steps], dim=0),
                                span([ctx[i] for i in steps]), span([ctx[i - 1] for i in steps]), cn)
            ahead.encode(), ahead.o16, ahead.mask         # (every member read here, in front of the loop)
        if defer:
            # Only the 1/8-resolution flow of step i enters step i+1 (AccFlow_.py:171-175): the mask head and the convex
            # upsampling of every step leave the sequential loop and run once, batched over the steps, behind it
            x16_all = ops.S16.empty(len(steps) * N, self.hidden_channel, h, w, dev)
            small_all = torch.empty((len(steps) * N, 2, h, w), dtype=torch.float32, device=dev)
        for k, i in enumerate(steps):
            k0, k1 = k * N, (k + 1) * N
            if s16:
                inputs = ahead.items(k0, k1) if hoist else _StepInputs(self, by_pair[(i, 0)], by_pair[(i, i - 1)], ctx[i],
                                                                       ctx[i - 1], ctx[0])
                x16 = x16_all.batch(k0, k1) if defer else ops.S16.empty(N, self.hidden_channel, h, w, dev)
                F2n, up = self._fuse16(inputs, F2n.float().contiguous(), ctx16[i], x16, small_all[k0:k1] if defer else None)
            else:
                F2n, up = self._fuse(by_pair[(i, i - 1)].contiguous(), by_pair[(i, 0)].contiguous(), F2n.contiguous(),
                                     ctx[i], ctx[i - 1], ctx[0])
            outs.append(up)
        if defer:
            outs = list(self.flow_decoder.upsample16(x16_all, small_all).split(N, dim=0))
        return (outs, F2n) if return_small else outs

    def _warm_chain(self, images, adj, ctx, F2n, feats, seed_iters):
        """The warm-start loop (see the class docstring): per frame i the seed by compose_flow, the seeded estimate i -> 0 of
        seed_iters iterations and the module-form step, starting from F2n = F(1 -> 0).  -> (outputs, the last step's F2n)"""
        outs = []
        for i in range(2, len(images)):
            dflow = adj[(i, i - 1)].contiguous()
            seed = ops.compose_flow(dflow, F2n.contiguous())
            flow_ini = self.estimate_small(images, [(i, 0)], flow_init=seed, iters=seed_iters, features=feats)
            F2n, up = self._fuse(dflow, flow_ini.contiguous(), F2n.contiguous(), ctx[i], ctx[i - 1], ctx[0])
            outs.append(up)
        return outs, F2n

    @torch.no_grad()
    @ops.range_guarded
    def forward_warm(self, images):
        """The warm-start schedule (see the class docstring): adjacent pairs in one batch, then per step i the seeded
        estimate i -> 0 followed by the fusion step."""
        images = list(images)
        require_cuda(*images)
        n = len(images)
        if n < 3:
            return []
        feats = {}
        adjacent = [(i, i - 1) for i in range(1, n)]
        adj = flows_by_pair(self.estimate_small(images, adjacent, features=feats), adjacent)
        ctx = self.context_of(images, want16=False)
        return self._warm_chain(images, adj, ctx, adj[(1, 0)], feats, self.warm_iters)[0]

    @staticmethod
    def stack_frames(images):
        """The frames as consecutive views of ONE tensor (a single copy): the three encoders then take their frame lists
        without a torch.cat each (_packs.span; 41 MB per 7-frame 480x1024 list)."""
        images = [im.float() for im in images]
        if len({tuple(im.shape) for im in images}) != 1:
            return images
        whole = span([im.contiguous() for im in images])      # (already adjacent: no copy at all)
        return list(whole.split(images[0].shape[0], dim=0))

    @torch.no_grad()
    def forward(self, images, test_mode=False):  # test_mode is ignored by the reference too (:157 FIXME)
        """f16x3 mode: the stages - estimator encoders, refinement, context encoder, fusion chain - are range-guarded one by
        one (ops.with_range_guard): a value outside the fp16 split's range re-runs only the stage that saw it in bf16x6."""
        images = list(images)
        require_cuda(*images)
        if len(images) < 3:
            return []
        if self.warm_start:
            return self.forward_warm(images)
        images = self.stack_frames(images)

        def run():
            flows, ctx = self.estimate_with_context(images, self.pair_schedule(len(images)))
            return self.fuse_chain(images, flows, ctx=ctx)

        # first without a host synchronisation per stage; only if some value left the fp16 split's range, stage by stage
        out, tripped = ops.optimistic(run, images[0].device)
        return run() if tripped else out

    def accumulate_video(self, frames, chunk=1, iters=None):
        """Generator over an iterable of frames (each (N,3,H,W), scaled as forward() expects): yields (i, F(i -> 0)) for
        i = 2, 3, ... as the frames come, `chunk` frames per AccFlowStream.push - memory does not grow with the video."""
        if int(chunk) != chunk or chunk < 1:
            raise ValueError("accumulate_video: chunk must be an integer >= 1 (got %r)" % (chunk,))
        stream = AccFlowStream(self, iters=iters)

        def gen():
            batch = []
            for f in frames:
                batch.append(f)
                if len(batch) == chunk:
                    yield from flush(batch)
                    batch = []
            if batch:
                yield from flush(batch)

        def flush(batch):
            outs = stream.push(batch)
            return zip(range(stream.n_frames - len(outs), stream.n_frames), outs)

        return gen()

    @torch.no_grad()
    def forward_pair_sharded_stream(self, sequences, group=None, on_result=None):
        """A stream of sequence batches, each spread over all ranks of `group`, with a ROTATING root
        (parallel.run_pair_sharded_stream): sequence k's fusion chain runs on rank k % world - on a side stream, underneath
        that rank's estimator pairs of the following sequences - so every rank does the same number of pairs and chains.
        Returns {k: outputs of sequence k} for the sequences this rank was the root of.  `sequences` may be any iterable (a
        data loader: it is consumed one sequence at a time); pending chains are resolved with a bounded lag, and with
        on_result(k, outputs) nothing is retained here - memory does not grow with the stream's length."""
        it = iter(sequences)
        first = list(next(it))
        sequences = itertools.chain([first], (list(s) for s in it))
        dev, n_frames = first[0].device, len(first)
        guarded = ops.current_mode() == ops.CONV_F16X3

        # f16x3 range guard without a host synchronisation: every rank's estimator pairs report to a device flag that rides
        # in the sequence's all_gather (parallel.run_pair_sharded_stream's aux); the root adds its chain's flag and copies
        # the sum to pinned memory behind the chain.  A tripped sequence (no real image has produced one) is recomputed
        # by its root alone, all pairs, in bf16x6, at the harvest.
        def est(images, my_pairs, is_root):
            N = images[0].shape[0]
            h, w = images[0].shape[2] // 8, images[0].shape[3] // 8
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            if not my_pairs:
                return torch.zeros((0, N, 2, h, w), dtype=torch.float32, device=dev), flag
            with (ops.guard_scope(flag) if guarded else contextlib.nullcontext()):
                small = self.estimate_small(images, my_pairs).view(len(my_pairs), N, 2, h, w)
            return small, flag

        def fuse(images, bp, flags):
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(dev))
            # (the chain on the ONE side stream per device of the process: hardware queues, see _context_stream)
            return launch_chain_aside(self, images, bp, ready, flag if guarded else None, flags) + ((images, bp, flag, flags),)

        shares = hasattr(getattr(self, "ofe", None), "att")
        return run_pair_sharded_stream(est, fuse, self.pair_schedule(n_frames), sequences, group=group,
                                       keep_together=shares, on_result=on_result,
                                       harvest=lambda h: harvest_chain_aside(self, h, "AccFlow.forward_pair_sharded_stream"))

    @torch.no_grad()
    def forward_pair_sharded(self, images, dst=0, group=None):
        """One sequence batch spread over the ranks of `group`: estimator pairs are dealt round-robin, one
        all_gather of the 1/8-res flows, fusion chain on `dst` (returns None on the other ranks)."""
        images = list(images)
        N = images[0].shape[0]
        h, w = images[0].shape[2] // 8, images[0].shape[3] // 8
        is_root = world(group)[1] == dst
        holder = []

        def est(my_pairs):
            # the root encodes the context features of all frames on its side stream WHILE it estimates its own pairs:
            # the serial section behind the all_gather is then the five fusion steps only
            if is_root and CONTEXT_SIDE_STREAM and images[0].is_cuda and not holder:
                holder.append(self.context_async(images))
            if not my_pairs:
                return torch.zeros((0, N, 2, h, w), dtype=torch.float32, device=images[0].device)
            return self.estimate_small(images, my_pairs).view(len(my_pairs), N, 2, h, w)

        def fuse(bp):
            if holder:
                return self.fuse_chain(images, bp, ctx=self.context_join(holder[0]))
            return self.fuse_chain(images, bp)

        # GMA: the pairs out of one image1 share its attention matrix - keep them on one rank (parallel.deal_pairs)
        shares = hasattr(getattr(self, "ofe", None), "att")
        return run_pair_sharded(est, fuse, len(images), self.pair_schedule(len(images)), dst=dst, group=group,
                                keep_together=shares)


def _own(t):
    """t without the rest of the allocation it is a view of (one frame's slice of a batched encoder output keeps the whole
    batch alive otherwise)."""
    if isinstance(t, ops.S16):
        return ops.S16(_own(t.data), t.C)
    return t if t.untyped_storage().nbytes() == t.numel() * t.element_size() else t.clone()


class _StreamState:
    """What AccFlowStream carries from one push to the next: frame 0 and the last frame - image, fnet features, context
    features (fp32, and pre-split where the mode has them) - the accumulated 1/8-resolution flow last -> 0, and the conv mode
    the features were made in.  Nothing here grows with the number of frames pushed."""
    __slots__ = ("images", "fmap", "ctx", "ctx16", "F2n", "mode")

    def __init__(self, images, fmap, ctx, ctx16, F2n, mode):
        self.images, self.fmap, self.ctx, self.ctx16 = list(images), list(fmap), list(ctx), ctx16
        self.F2n, self.mode = F2n, mode

    def features(self):
        """A fresh estimate_pairs feature dict (encode_frames clears one whose mode differs: never hand out the state's own)."""
        return {"fmap": dict(enumerate(self.fmap)), "cnet": {}, "mode": self.mode}


class AccFlowStream:
    """Backward accumulation over a frame stream: push frames as they come, get F(i -> 0) back, at constant memory.

        s = AccFlowStream(model)            # model: AccFlow, any estimator; iters: the estimator's iterations (None: forward's)
        flows = s.push(frames)              # one (N,3,H,W) tensor or a list of them -> [F(i -> 0) for each pushed i >= 2]

    A push of frames a..b is AccFlow.forward on [frame 0, frame a-1, frame a, ..., frame b] with pair (1, 0) of that list
    - F(a-1 -> 0) - not estimated: it is the flow carried from the previous push, the decoder's 1/8-resolution output of its
    last step (what the reference hands from step to step, AccFlow_.py:171-175,200).  Frames 0 and a-1 are not encoded again
    either (fnet and context features are kept; only image2 roles occur for them, so no cnet).  The launches are
    estimate_small's and fuse_chain's; with model.warm_start the push follows forward_warm's schedule instead.  The first
    push that brings the stream to three frames is forward() on all of them.  A push that raises leaves the stream as it was.
    With N > 1 the encoders run sample by sample (_encode_per_sample), everything else batched."""

    def __init__(self, model, iters=None):
        if not hasattr(model.ofe, "estimate_pairs"):
            raise TypeError("AccFlowStream: the estimator must take estimate_pairs(features=) - its encoder outputs of frame 0 "
                            "and of the last frame are kept from push to push")
        self.model, self.iters = model, iters
        self.reset()

    def reset(self):
        self._pending, self._state, self._like, self.n_frames = [], None, None, 0

    def _checked(self, frames):
        frames = [frames] if isinstance(frames, torch.Tensor) else list(frames)
        like = self._like
        for f in frames:
            if not (isinstance(f, torch.Tensor) and f.dim() == 4 and f.shape[1] == 3):
                raise ValueError("AccFlowStream.push: frames are (N,3,H,W) tensors")
            require_cuda(f)
            if like is None:
                like = (tuple(f.shape), f.device)
            if (tuple(f.shape), f.device) != like:
                raise ValueError("AccFlowStream.push: frame %s on %s in a stream of %s on %s" % (tuple(f.shape), f.device, *like))
        return frames, like

    @torch.no_grad()
    def push(self, frames):
        frames, like = self._checked(frames)
        if not frames:
            return []
        st = self._state
        if st is None and len(self._pending) + len(frames) < 3:      # frames 0 and 1 alone: nothing to accumulate yet
            self._pending = self._pending + [f.float().clone() for f in frames]
            self._like, self.n_frames = like, len(self._pending)
            return []
        run = self._push_warm if self.model.warm_start else self._push
        outs, state = run(st, list(st.images if st is not None else self._pending), frames)
        self._state, self._pending, self._like = state, [], like     # (the one commit, after the run whose result is returned)
        self.n_frames += len(frames)
        return outs

    def _push(self, st, kept, new):
        m = self.model
        new = m.stack_frames(new)
        L = kept + new
        N, dev = L[0].shape[0], L[0].device
        pairs = m.pair_schedule(len(L))
        if st is not None:
            pairs.remove((1, 0))

        def run():
            mode = ops.current_mode()
            cached = st is not None and st.mode == mode
            todo = new if cached else L        # (another conv mode than the cache's: frames 0 and a-1 again, from the images)
            feats = st.features() if st is not None else {}
            if N > 1:
                ctx, ctx16 = self._encode_per_sample(L, pairs, range(len(L) - len(todo), len(L)), feats, want16=True)
                by_pair = flows_by_pair(m.estimate_small(L, pairs, iters=self.iters, features=feats), pairs)
            else:
                by_pair, (ctx, ctx16) = m.estimate_with_context(L, pairs, ctx_images=todo, iters=self.iters, features=feats)
            ctx, ctx16 = list(ctx), list(ctx16) if ctx16 is not None else None
            if cached:
                ctx = st.ctx + ctx
                ctx16 = st.ctx16 + ctx16 if ctx16 is not None and st.ctx16 is not None else None
            if st is not None:
                by_pair[(1, 0)] = st.F2n
            outs, F2n = m.fuse_chain(L, by_pair, ctx=(ctx, ctx16), return_small=True)
            return outs, (feats["fmap"], ctx, ctx16, F2n, mode)

        # as forward(): first without a host synchronisation per stage; stage by stage only if a value left the fp16 range
        out, tripped = ops.optimistic(run, dev)
        outs, made = run() if tripped else out
        return outs, self._next_state(st, L, *made)

    def _push_warm(self, st, kept, new):
        """forward_warm's schedule: the adjacent pairs of the new frames in one batch, then per frame the compose_flow seed,
        the seeded estimate i -> 0 and the fusion step."""
        m = self.model
        L = kept + [f.float() for f in new]
        N, dev = L[0].shape[0], L[0].device
        adjacent = [(i, i - 1) for i in range(1 if st is None else 2, len(L))]
        warm_iters = m.warm_iters if m.warm_iters is not None else self.iters

        def run():
            mode = ops.current_mode()
            cached = st is not None and st.mode == mode
            feats = st.features() if st is not None else {}
            if N > 1:
                ctx = self._encode_per_sample(L, adjacent + [(i, 0) for i in range(2, len(L))],
                                              range(2 if cached else 0, len(L)), feats, want16=False)[0]
            adj = flows_by_pair(m.estimate_small(L, adjacent, iters=self.iters, features=feats), adjacent)
            if N == 1:
                ctx = list(m.context_of(L[2:] if cached else L, want16=False))
            if cached:
                ctx = st.ctx + ctx
            outs, F2n = m._warm_chain(L, adj, ctx, adj[(1, 0)] if st is None else st.F2n, feats, warm_iters)
            return outs, (feats["fmap"], ctx, None, F2n, mode)

        outs, made = ops.with_range_guard(run, dev, name="AccFlowStream.push")
        return outs, self._next_state(st, L, *made)

    def _encode_per_sample(self, L, pairs, ctx_ids, feats, want16):
        """N > 1: the three encoders sample by sample, so that a sample's flows do not depend on what else is in the batch.
        The convolution planner's schedule (split-K, tile shapes) is a function of the images per encoder call, and a
        last-bit difference in an encoder output grows past 1e-4 px over the refinement and the chain (measured: 1.5e-4 to
        2.3e-4 px between N = 2 and N = 1 with batched encoders, at most 6.3e-5 this way); the refinement and the chain stay
        batched.  Fills `feats` with what
        estimate_pairs needs for `pairs` (the samples' outputs joined per frame) and returns the context encoder's outputs of
        frames `ctx_ids` in context()'s two forms."""
        m = self.model
        fnet_ids, cnet_ids = {i for p in pairs for i in p}, {i for i, _ in pairs}
        per, ctx, ctx16 = [], [], []
        for n in range(L[0].shape[0]):
            frames = [f[n:n + 1] for f in L]
            fn = {k: ({i: t[n:n + 1] for i, t in v.items()} if isinstance(v, dict) else v) for k, v in feats.items()}
            per.append(m.ofe.encode_frames(frames, fnet_ids, cnet_ids, fn))
            c = m.context_of([frames[i] for i in ctx_ids], want16=want16)
            c, c16 = c if want16 else (c, None)
            ctx.append(c)
            ctx16.append(c16)
        feats.clear()
        feats.update({key: {i: torch.cat([p[key][i] for p in per]) for i in per[0][key]} for key in ("fmap", "cnet")})
        feats["mode"] = per[0]["mode"]
        joined = [torch.cat(cs) for cs in zip(*ctx)]
        if any(c is None for c in ctx16):
            return joined, None
        return joined, [ops.S16(torch.cat([c.data for c in cs]), cs[0].C) for cs in zip(*ctx16)]

    @staticmethod
    def _next_state(st, L, fmap, ctx, ctx16, F2n, mode):
        """Frame 0 and the last frame of L as the next push's cache; what the old state holds of frame 0 in this mode stays."""
        last = len(L) - 1
        if st is not None and st.mode == mode:
            fmap0, ctx0 = st.fmap[0], st.ctx[0]
        else:
            fmap0, ctx0 = _own(fmap[0]), _own(ctx[0])
        return _StreamState([L[0] if st is not None else L[0].clone(), L[last].clone()], [fmap0, _own(fmap[last])],
                            [ctx0, _own(ctx[last])], [_own(ctx16[0]), _own(ctx16[last])] if ctx16 is not None else None,
                            _own(F2n.float()), mode)
