// Direct (implicit-GEMM) fp32 convolution on the gfx950 fp32-input matrix cores: this unit is the dispatcher - validate,
// plan (conv_plan.cpp), hand descriptor + plan to the family's launcher (launchers.h).  The packs are conv_pack.hip's.
//
// Replaces every cuDNN conv the reference's inference path reaches through nn.Conv2d
// (raft/update.py:9-10,37-43,83-87,122-125; raft/extractor.py:9-15,52,140-158; AccFlow_.py:16-25,
// 51-53,71-95,115-120; gma/update.py:117-125) and torchvision.ops.deform_conv2d (AccFlow_.py:83,104).
//
// Formulation: D[ch x px] = Wp[k x ch]^T * X[k x px], k = (c, ky, kx) flattened, px = (b, oy, ox)
// flattened.  Output channels ride the MFMA A operand and pixels the B operand, so accumulator
// column = lane&31 = pixel and every store instruction writes two 128-B runs of consecutive pixels of
// an NCHW plane (coalesced without an LDS transpose).  Both operands are staged k-major in LDS
// ([k][ch], [k][px]): with the 32x32x2 fp32 MFMA each lane needs ONE float of each per instruction,
// read by conflict-free ds_read_b32.  fp32-in / fp32-acc MFMA is a bitwise fmaf chain, so the result
// matches an fp32 CPU convolution to summation-order rounding.
//
// Staging: the activation tile is an im2col gather.  Each thread owns one pixel of the tile for the
// whole kernel (its (b, oy, ox) is decoded once); the k row it loads is wave-uniform, so the per-k
// descriptor {channel, ky, kx, source} comes from a scalar load of a small table and the per-element
// work is two adds, two unsigned compares and one predicated dword load, coalesced along x.
// Registers double-buffer the next slab while the current one feeds the MFMAs (one barrier per slab).
#include "common.h"
#include "launchers.h"

extern "C" int accflow_conv_in_norm_supported(const accflow_conv_desc* desc) {
  if (!desc) return 0;
  accflow_conv_desc probe = *desc, d;   // (asked before in_norm and stats exist: neither decides the route)
  probe.in_norm = nullptr;
  probe.stats = nullptr;
  conv_plan p;
  return !conv_validate(&probe, d) && !conv_make_plan(d, false, p) && p.can_norm ? 1 : 0;
}

extern "C" int accflow_conv_stat_slots(const accflow_conv_desc* desc) {
  if (!desc || desc->epi != ACCFLOW_EPI_STORE || desc->act != ACCFLOW_ACT_NONE) return 0;
  accflow_conv_desc d;
  conv_plan p;
  return !conv_validate(desc, d) && !conv_make_plan(d, true, p) ? p.slots : 0;
}

// The plan accflow_conv2d_f32 would launch this descriptor with, and whether it would accept it (0) or refuse it (1):
// host only, launches nothing.  out[0..13]: family tc tp wc wp lay loop tapgemm norm w4 mode slots ch0 Z; with a tail split
// (ch0 > 0) out[14], out[15]: the split-K parts of the head and of the tail, 0 otherwise.
extern "C" int accflow_conv_plan_query(const accflow_conv_desc* desc, int* out, int n) {
  if (!out || n < 16) return 1;
  for (int i = 0; i < 16; ++i) out[i] = 0;
  accflow_conv_desc d;
  conv_plan p;
  if (conv_validate(desc, d) || conv_make_plan(d, d.stats != nullptr, p)) return 1;
  const int v[14] = {p.family, p.tc, p.tp, p.wc, p.wp, p.lay, p.loop, (int)p.tapgemm, (int)p.norm, (int)p.w4, p.mode, p.slots, p.ch0, p.Z};
  for (int i = 0; i < 14; ++i) out[i] = v[i];
  if (d.stats && p.slots != d.stat_slots) return 1;
  if (d.in_norm && !p.can_norm) return 1;
  if (p.ch0 > 0) {
    accflow_conv_desc head, tail;
    conv_plan ph, pt;
    conv_tail_split(d, p.ch0, head, tail);
    if (conv_plan_part(head, p, false, ph) || conv_plan_part(tail, p, true, pt)) return 1;
    out[14] = ph.Z;
    out[15] = pt.Z;
  }
  return 0;
}

extern "C" int accflow_conv2d_f32(const accflow_conv_desc* desc, void* stream) {
  accflow_conv_desc d;
  conv_plan p;
  if (conv_validate(desc, d) || conv_make_plan(d, d.stats != nullptr, p)) return 1;
  if (d.stats && p.slots != d.stat_slots) return 1;   // the route must be the one accflow_conv_stat_slots reported for
  if (d.in_norm && !p.can_norm) return 1;
  hipStream_t st = as_stream(stream);
  switch (p.family) {
    case CONV_FAM_SMALL:
    case CONV_FAM_SMALL_PATCH: return accflow_launch_conv_small(d, p, st);
    case CONV_FAM_STEM: return accflow_launch_conv_stem(d, st);
    case CONV_FAM_DIRECT: return accflow_launch_conv_direct(d, p, st);
    case CONV_FAM_S16M: return accflow_launch_conv_s16m(d, p, st);
    case CONV_FAM_IM2COL: return accflow_launch_conv_bf16s(d, p.tc, p.tp, p.Z, st);
    case CONV_FAM_F32: return accflow_launch_conv_f32(d, p.wc, p.wp, p.tc, p.tp, st);
  }
  return 1;
}
