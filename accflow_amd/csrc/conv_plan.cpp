// Convolution dispatch as a pure host function: descriptor -> conv_plan (conv_plan.h).  No device code, no hip* call.
#include "conv_plan.h"
#include <stdlib.h>

namespace {

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

long long env_ll(const char* name, long long dflt) {
  const char* e = getenv(name);
  return e ? atoll(e) : dflt;
}

// workgroups of a launch against the 768 slots of the chip (256 CUs x 3): the part count whose whole rounds are fullest
int fill_parts(long long nb) {
  int Z = 1;
  double best = 0.0;
  for (int z = 1; z <= 8; ++z) {
    const double fill = (double)(nb * z) / (double)(cdiv(nb * z, 768) * 768);
    if (fill > best + 0.03) { best = fill; Z = z; }
  }
  return Z;
}

// The split-K part count of every family.  nb: workgroups of the unsplit launch; deep: the reduction is deep enough for the
// fill rule (direct / multi-source: >= 256 chunks - the GMA aggregation, 14 400 channels at 720x1280; im2col: Kpad >= 2048),
// zenv its override; nchunk > 0: the family also splits small grids (the batch-1 fusion chain) in 2-4 parts of >= 2 chunks
// ((a fill-based part count up to 8 there, too, measured no gain on the chain: 30.9 vs 31.0 ms); im2col passes 0).
// One part when there is no workspace, with statistics (gathered in the conv kernel's epilogue), with an S16 residual
// (the reduce kernel reads an fp32 one), with split_c0 (two reduction lengths and activations: the reduce kernel knows
// one) and for a GRU_ZR S16 copy whose r*h half does not start on an octet.
int conv_split_k(const accflow_conv_desc& d, bool want_stats, long long nb, bool deep, int zenv, int nchunk) {
  if (!d.kws || want_stats || d.e0_fmt || d.split_c0) return 1;
  if (d.out16 && d.epi == ACCFLOW_EPI_GRU_ZR && ((d.Cout >> 1) & 7)) return 1;
  int Z = 1;
  if (deep && nb < 700) {
    Z = zenv > 0 ? zenv : fill_parts(nb);
  } else if (nchunk > 0 && nb < 320) {
    Z = (int)((512 + nb - 1) / nb);
    if (Z > 4) Z = 4;
    if (Z > nchunk / 2) Z = nchunk / 2;
  }
  const long long nout = (long long)d.B * d.Cout * d.OH * d.OW;
  if (Z > 1 && (long long)Z * nout > d.kws_elems) Z = (int)(d.kws_elems / nout);
  return Z < 1 ? 1 : Z;
}

// Cout = 128 m + (1..64) (convc2: 256 -> 192): with 128-channel workgroups only, the last channel block would run all its
// MFMAs with half of its rows on padding (25 % of the launch's matrix work wasted at 192).  Pointwise epilogues let the
// launch be cut in two along the channels: 128 m channels on 128-channel workgroups, the last 64 on 64-channel ones.
// nb128: 128-channel workgroups of the uncut launch (a small grid with a workspace is split along K instead).  Not with
// statistics: their slot count is that of ONE kernel, the one accflow_conv_stat_slots planned (want_stats).
int conv_tail_ch0(const accflow_conv_desc& d, bool want_stats, long long nb128) {
  const bool pointwise = d.epi == ACCFLOW_EPI_STORE || d.epi == ACCFLOW_EPI_RES_RELU || d.epi == ACCFLOW_EPI_ACCUM;
  if (d.Cout > 128 && d.Cout % 128 > 0 && d.Cout % 128 <= 64 && pointwise && !want_stats && !d.cb && !(d.kws && nb128 < 320))
    return d.Cout / 128 * 128;
  return 0;
}

void plan_init(conv_plan& p, int family, int mode) {
  p = conv_plan();
  p.family = family;
  p.mode = mode;
  p.Z = 1;
}

// ---- direct kernel: TC x 64 channels x (4 x 32) pixels ----
int plan_direct_tile(const accflow_conv_desc& d, int tc, bool want_stats, conv_plan& p) {
  const conv_switches& sw = conv_switches_get();
  plan_init(p, CONV_FAM_DIRECT, d.mode);
  p.tc = tc;
  p.w4 = tc == 2 && sw.direct_w4;
  const int tiles = cdiv(d.OW, DIR_TW) * cdiv(d.OH, DIR_TH);
  const long long nb = (long long)d.B * tiles * cdiv(d.Cout, 2 * tc * 32);
  // normalise-on-load: single-source input of <= 256 channels, the kernels instantiated for it
  p.can_norm = !d.in1 && d.C0 <= DIR_NORM_MAXC && (tc == 1 || sw.direct_w4);
  p.slots = tiles * (p.w4 ? 1 : 2);   // one slot per wave along the pixels
  const int nchunk = (d.C0 + d.C1 + 15) / 16;
  p.Z = conv_split_k(d, want_stats, nb, nchunk >= 256, sw.direct_ksplit, nchunk);
  const bool f16 = d.mode == ACCFLOW_CONV_F16X3 && d.wpatch16;
  const bool k3 = d.KH == 3 && d.KW == 3;
  if (d.epi == ACCFLOW_EPI_TAPGEMM) {   // (validated by conv_validate)
    if (tc != 2 || !f16 || !d.in_fmt || p.Z != 1 || !p.w4) return 1;
    p.tapgemm = true;
    if (sw.direct_kt9 && k3 && (d.C0 + d.C1) % 16 == 0) p.loop = CONV_LOOP_TAP9;
  } else if (d.in_fmt) {  // S16 sources: the fp16 kernel with the DMA loader (every source must be S16; no normalise-on-load)
    if (!f16 || d.in_norm || d.in_fmt != (d.in1 ? 3 : 1)) return 1;
    // the tap-specialised K loops: 5 taps (the GRU's 1x5 / 5x1) on the 128-channel kernel - 23.80 / 23.72 vs 23.91 / 23.98 ms
    // per step on one box - and 3x3 (round 6): 23.27-23.31 vs 23.44-23.54 ms per step
    if (sw.direct_kt && p.w4 && d.KH * d.KW == 5) p.loop = CONV_LOOP_TAP5;
    else if (sw.direct_kt9 && (tc == 1 || p.w4) && k3) p.loop = CONV_LOOP_TAP9;
  } else if (d.in_norm) {
    // (128-channel fp16 kernel only: 0.354 -> 0.314 and 0.161 -> 0.146 ms per step on the 96- / 128-channel layers; the 64-channel
    // kernel needs 129 registers in this form - 3 instead of 4 waves per SIMD - and was 4 % slower: profiles/r06_ab_kt9_norm.txt)
    p.norm = true;
    if (f16 && sw.direct_kt9 && tc == 2 && k3 && d.C0 % 16 == 0) p.loop = CONV_LOOP_TAP9;
  }
  return 0;
}

// ---- multi-source S16 kernel ----
bool s16m_fits(const accflow_conv_desc& d, int TH) {
  for (int s = 0; s < d.nsrc; ++s) {
    const accflow_conv_src& S = d.src[s];
    if ((TH + S.KH - 1) * (S16M_TW + S.KW - 1) > s16m_cap(TH) / 4) return false;
  }
  return true;
}

bool s16m_eligible(const accflow_conv_desc& d) {
  if (d.nsrc < 1 || d.nsrc > ACCFLOW_CONV_MAX_SRC || !d.wpatch16 || !d.wscale16 || d.mode != ACCFLOW_CONV_F16X3) return false;
  if (d.wsplit_bs || d.offset || d.in_norm || d.Cout <= 4) return false;
  // an S16 residual operand exists in the lean residual epilogue only (every wave's 32 * TCW rows present)
  if (d.e0_fmt && (d.epi != ACCFLOW_EPI_RES_RELU || d.act != ACCFLOW_ACT_RELU || d.cb || (d.Cout % 32) || !d.e0)) return false;
  for (int s = 0; s < d.nsrc; ++s) {
    const accflow_conv_src& S = d.src[s];
    if (!S.ptr || S.C <= 0 || S.Hs <= 0 || S.Ws <= 0 || (S.step != 1 && S.step != 2) || S.KH <= 0 || S.KW <= 0) return false;
    if (S.oy < 0 || S.ox < 0 || S.oy >= S.step || S.ox >= S.step) return false;
    if (S.padH < 0 || S.padW < 0 || S.padH >= S.KH || S.padW >= S.KW) return false;
    // 32-bit buffer offsets: each source must span < 4 GiB
    if ((((long long)(d.B - 1)) * S.bs + accflow_s16_item_words(S.C, S.Hs, S.Ws)) * 4 >= (1LL << 32)) return false;
  }
  return s16m_fits(d, 4);
}

int plan_s16m_lay(const accflow_conv_desc& d, int lay, bool want_stats, conv_plan& p) {
  plan_init(p, CONV_FAM_S16M, d.mode);
  const s16m_layout& L = S16M_LAYOUTS[lay];
  p.lay = lay;
  const int tiles = cdiv(d.OW, S16M_TW) * cdiv(d.OH, L.TH);
  const long long nb = (long long)d.B * tiles * cdiv(d.Cout, L.WC * L.TCW * 32);
  p.slots = tiles * L.WP;   // one statistics slot per wave along the pixels
  int nchunk = 0;
  for (int s = 0; s < d.nsrc; ++s) nchunk += (L.TH == 4 ? s16m_geometry<4>(d.src[s]) : s16m_geometry<8>(d.src[s])).nch;
  p.Z = conv_split_k(d, want_stats, nb, nchunk >= 256, 0, nchunk);
  if (d.e0_fmt && (d.Cout % (L.TCW * 32))) return 1;   // every wave's rows all present, or all absent
  // the tap-specialised loop when every source is 3x3 / step 1
  bool kt9 = conv_switches_get().s16m_kt9 && !d.split_c0;
  for (int s = 0; s < d.nsrc && kt9; ++s) kt9 = d.src[s].KH == 3 && d.src[s].KW == 3 && d.src[s].step == 1;
  if (kt9) p.loop = CONV_LOOP_TAP9;
  return 0;
}

int plan_s16m(const accflow_conv_desc& d, bool want_stats, conv_plan& p) {
  if (!s16m_eligible(d)) return 1;
  int lay = d.src[0].reserved > 0 ? d.src[0].reserved - 1 : -1;   // (tests / tuning: accflow_conv_src.reserved)
  if (lay < 0) lay = conv_switches_get().s16m_lay;
  const bool fits8 = s16m_fits(d, 8);
  const long long tiles8 = (long long)d.B * cdiv(d.OW, S16M_TW) * cdiv(d.OH, 8);
  if (d.split_c0) {
    // accflow_conv_desc.split_c0: the channel block must not straddle the two convolutions - 96 -> the 96-channel layout,
    // 128 -> the 128-channel one, 64 -> a 64-channel one; both halves whole blocks (the lean epilogue, or the general one
    // with act NONE for both: the InstanceNorm encoder's raw outputs + statistics)
    const int c0 = d.split_c0, c1 = d.Cout - d.split_c0;
    if (d.epi != ACCFLOW_EPI_STORE || d.cb || (d.act != ACCFLOW_ACT_NONE && (d.act != ACCFLOW_ACT_RELU || d.stats)) || c1 <= 0)
      return 1;
    int bc;
    if (c0 == 96 && fits8) { lay = 3; bc = 96; }
    else if (c0 == 128) { lay = 0; bc = 128; }
    else if (c0 == 64) { lay = (fits8 && tiles8 >= 1536) ? 1 : 2; bc = 64; }
    else return 1;
    if (c1 % bc) return 1;
    return plan_s16m_lay(d, lay, want_stats, p);
  }
  if ((lay == 1 || lay == 3) && !fits8) lay = -1;
  if (lay >= 0 && lay <= 3) return plan_s16m_lay(d, lay, want_stats, p);
  // enough workgroups to fill the chip at 3 per CU
  const bool big8 = fits8 && tiles8 >= 1536 && !(d.kws && tiles8 < 320);
  if (d.Cout <= 64) return plan_s16m_lay(d, big8 ? 1 : 2, want_stats, p);
  // 96-channel blocks: 96 -> 96 (encoder layer2) and 192 = 2 x 96 (convc2: 212 vs 227 us as 128 + 64, profiles/r04_s16m_bench.txt)
  if ((d.Cout <= 96 || d.Cout == 192) && fits8 && tiles8 >= 600 && !(d.kws && tiles8 < 320)) return plan_s16m_lay(d, 3, want_stats, p);
  const long long tiles4 = (long long)d.B * cdiv(d.OW, S16M_TW) * cdiv(d.OH, 4);
  const int rc = plan_s16m_lay(d, 0, want_stats, p);
  if (!rc) p.ch0 = conv_tail_ch0(d, want_stats, tiles4 * cdiv(d.Cout, 128));   // the head on layout 0, the tail on layout 2
  return rc;
}

// the in0 / in1 S16 form as sources (same pack: accflow_conv_pack_patch16's step order is (16-channel group, tap) over the
// concatenated channels, and a chunk never straddles the two sources - C0 % 16 == 0, % 32 for 1x1)
void s16m_from_legacy(accflow_conv_desc& e) {
  e.nsrc = e.in1 ? 2 : 1;
  for (int s = 0; s < e.nsrc; ++s) {
    accflow_conv_src& S = e.src[s];
    S.ptr = s ? (const void*)e.in1 : (const void*)e.in0;
    S.bs = s ? e.in1_bs : e.in0_bs;
    S.C = s ? e.C1 : e.C0;
    S.Hs = e.H; S.Ws = e.W;
    S.step = 1; S.oy = 0; S.ox = 0;
    S.KH = e.KH; S.KW = e.KW; S.padH = e.padH; S.padW = e.padW;
    S.reserved = 0;
  }
}

// the encoders' 7x7 stride-2 stem of the 3-channel image (conv_stem.hip)
bool stem_eligible(const accflow_conv_desc& d) {
  return d.mode == ACCFLOW_CONV_F16X3 && d.wsplit16 && d.wscale16 && !d.in1 && !d.in_fmt && !d.nsrc && d.C0 == 3 && d.KH == 7 &&
         d.KW == 7 && d.stride == 2 && d.padH == 3 && d.padW == 3 && d.Cout > 32 && d.Cout <= 64 && !d.offset && !d.in_norm &&
         !d.wsplit_bs && !d.cb && d.Kpad == 160 && d.OH == (d.H + 6 - 7) / 2 + 1 && d.OW == (d.W + 6 - 7) / 2 + 1;
}

// ---- im2col kernel: TC x 64 channels x TP x 64 pixels ----
int plan_im2col(const accflow_conv_desc& d, int tc, int tp, bool want_stats, bool per_item, conv_plan& p) {
  plan_init(p, CONV_FAM_IM2COL, d.mode);
  p.tc = tc; p.tp = tp;
  // statistics: a pixel tile must not straddle two batch items; 2 waves along the pixels = 2 slots per tile
  const int OHW = d.OH * d.OW, BP = 2 * tp * 32;
  p.slots = (!per_item && OHW % BP == 0) ? OHW / BP * 2 : 0;
  // split-K for deep reductions on grids that do not fill the 768 workgroup slots (3 per CU): the GMA aggregation
  // (K = h*w = 14 400 at 720x1280, 225 pixel tiles per item)
  const long long nb = (long long)cdiv((long long)d.B * OHW, BP) * cdiv(d.Cout, 2 * tc * 32);
  p.Z = conv_split_k(d, want_stats, nb, d.Kpad >= 2048, conv_switches_get().im2col_ksplit, 0);
  return 0;
}

// the largest tile that still yields >= 384 workgroups (256 CUs x ~1.5): the fusion chain runs at batch 1 (7 680 pixels),
// where 128 x 128 tiles would leave most CUs idle
int plan_im2col_auto(const accflow_conv_desc& d, bool want_stats, conv_plan& p) {
  const long long Ptot = (long long)d.B * d.OH * d.OW;
  auto nb = [&](int bc, int bp) { return (long long)cdiv(Ptot, bp) * cdiv(d.Cout, bc); };
  if (d.Cout <= 64) return plan_im2col(d, 1, nb(64, 128) >= 384 ? 2 : 1, want_stats, false, p);
  // (a 192-channel x 128-pixel tile existed for Cout % 192 == 0 until round 5: the only such convolution of the workload,
  // convc2, runs on the direct kernel; its instantiation group took 5.6 minutes to compile - the longest unit of the build)
  if (nb(128, 128) >= 384) return plan_im2col(d, 2, 2, want_stats, false, p);
  if (nb(128, 64) >= 384) return plan_im2col(d, 2, 1, want_stats, false, p);
  return plan_im2col(d, 1, 1, want_stats, false, p);
}

int plan_f32(const accflow_conv_desc& d, conv_plan& p) {   // (the fp32-MFMA kernels gather no statistics)
  plan_init(p, CONV_FAM_F32, d.mode);
  const long long Ptot = (long long)d.B * d.OH * d.OW;
  auto blocks = [&](int bc, int bp) { return (long long)cdiv(Ptot, bp) * cdiv(d.Cout, bc); };
  auto tile = [&](int wc, int wp, int tc, int tp) { p.wc = wc; p.wp = wp; p.tc = tc; p.tp = tp; return 0; };
  constexpr long long MIN_BLOCKS = 384;
  if (d.Cout <= 32) return tile(1, 4, 1, blocks(32, 256) >= MIN_BLOCKS ? 2 : 1);      // 32 ch x 256 / 128 px
  if (d.Cout <= 64) return tile(2, 2, 1, blocks(64, 128) >= MIN_BLOCKS ? 2 : 1);      // 64 ch x 128 / 64 px
  if (d.Cout % 96 == 0 && d.Cout % 128 != 0 && blocks(96, 128) >= MIN_BLOCKS) return tile(1, 4, 3, 1);   // 96 ch x 128 px
  if (blocks(128, 128) >= MIN_BLOCKS) return tile(2, 2, 2, 2);                        // 128 ch x 128 px
  if (blocks(128, 64) >= MIN_BLOCKS) return tile(2, 2, 2, 1);                         // 128 ch x 64 px
  return tile(2, 2, 1, 1);                                                            // 64 ch x 64 px
}

}  // namespace

const conv_switches& conv_switches_get() {
  static const conv_switches sw = [] {
    conv_switches s;
    s.direct_w4 = env_ll("ACCFLOW_DIRECT_W4", 1) != 0;
    s.direct_kt = env_ll("ACCFLOW_DIRECT_KT", 1) != 0;
    s.direct_kt9 = env_ll("ACCFLOW_DIRECT_KT9", 1) != 0;
    s.s16m = env_ll("ACCFLOW_S16M", 0) != 0;
    s.s16m_kt9 = env_ll("ACCFLOW_S16M_KT9", 1) != 0;
    s.s16m_lay = (int)env_ll("ACCFLOW_S16M_LAY", -1);
    s.stem = env_ll("ACCFLOW_CONV_STEM", 1) != 0;
    s.patch_min_blocks = env_ll("ACCFLOW_PATCH_MIN_BLOCKS", 300);
    s.direct_ksplit = (int)env_ll("ACCFLOW_DIRECT_KSPLIT", 0);
    s.im2col_ksplit = (int)env_ll("ACCFLOW_IM2COL_KSPLIT", 0);
    return s;
  }();
  return sw;
}

extern "C" long long accflow_s16_item_words(int C, int H, int W) {
  return (long long)((C + 7) / 8) * 2 * H * W * 4;   // octets x 2 terms x pixels x 16 bytes, in 4-byte words
}

extern "C" int accflow_conv_kpad(int Cin, int KH, int KW) {
  const int K = Cin * KH * KW;
  return (K + 31) / 32 * 32;  // multiple of every slab depth in use (16 and 32)
}

extern "C" int accflow_conv_coutpad(int Cout) { return (Cout + 127) / 128 * 128; }

// (the pre-split GRU state rides on the tap-specialised 5-tap instantiations: both A/B switches of that route must be on;
// Python asks this function instead of re-reading the switches, so the two cannot disagree)
extern "C" int accflow_conv_gru16_supported(void) {
  const conv_switches& sw = conv_switches_get();
  return sw.direct_kt && sw.direct_w4 && !sw.s16m ? 1 : 0;
}

bool accflow_conv_direct_eligible(const accflow_conv_desc& d) {
  if (!d.wpatch || d.wsplit_bs || d.mode == ACCFLOW_CONV_F32 || d.offset || d.stride != 1 || d.Cout <= 4) return false;
  if (d.OH != d.H || d.OW != d.W) return false;                                // "same" convolutions only
  if ((DIR_TH + d.KH - 1) * (DIR_TW + d.KW - 1) > DIR_NPMAX) return false;
  if (d.C0 + d.C1 < 16) return false;                                          // 2 / 3-channel stems: im2col kernel
  if (d.in1 && (d.C0 % (d.KH * d.KW == 1 ? 32 : 16))) return false;            // a chunk must not straddle the sources
  return true;
}

int conv_validate(const accflow_conv_desc* desc, accflow_conv_desc& dd) {
  if (!desc) return 1;
  dd = *desc;
  // the row / activation scales belong to the fp16 pack: every other kernel must not see them
  if (dd.mode == ACCFLOW_CONV_F16X3 && (dd.wpatch16 || dd.wsplit16) && !dd.wscale16) return 1;
  if (dd.mode != ACCFLOW_CONV_F16X3) { dd.wpatch16 = nullptr; dd.wsplit16 = nullptr; }
  if (!dd.wpatch16 && !dd.wsplit16) dd.wscale16 = nullptr;
  dd.acc_scale = 0.0f;
  if (dd.nsrc < 0 || dd.nsrc > ACCFLOW_CONV_MAX_SRC) return 1;
  // an S16 e0: the multi-source kernel's residual operand, or - round 6 - the GRU state of the 5-tap S16 direct convolutions on
  // PACKED operands (accflow_conv_desc.p32): GRU_ZR with p32 = 3, GRU_Q with p32 = 6, whole 128-channel blocks, no split-K
  const bool gru16 = !dd.nsrc && dd.e0_fmt;
  if (gru16 && !(dd.in_fmt == (dd.in1 ? 3 : 1) && dd.e0 && dd.pre && dd.out16 && dd.mode == ACCFLOW_CONV_F16X3 && !dd.cb && !dd.kws &&
                 dd.KH * dd.KW == 5 && dd.stride == 1 && accflow_conv_gru16_supported() && !dd.stats &&
                 ((dd.epi == ACCFLOW_EPI_GRU_ZR && dd.p32 == 3 && dd.out && dd.Cout == 256) ||
                  (dd.epi == ACCFLOW_EPI_GRU_Q && dd.p32 == 6 && dd.e1 && dd.Cout == 128))))
    return 1;
  // a pixel-major fp32 destination alone: a plain store of an S16-source direct convolution on whole 128-channel blocks
  if (!gru16 && dd.p32 && !(dd.p32 == 1 && !dd.nsrc && dd.in_fmt == (dd.in1 ? 3 : 1) && dd.mode == ACCFLOW_CONV_F16X3 && dd.out && !dd.out16 &&
                            dd.epi == ACCFLOW_EPI_STORE && (dd.act == ACCFLOW_ACT_NONE || dd.act == ACCFLOW_ACT_RELU) && !dd.cb &&
                            !dd.kws && !dd.stats && dd.stride == 1 && (dd.Cout % 128) == 0 && accflow_conv_gru16_supported()))
    return 1;
  const bool multi = dd.nsrc > 0;   // multi-source S16 form: src[] replaces in0 / in1 and the conv geometry fields
  if (multi) {
    if (dd.mode != ACCFLOW_CONV_F16X3 || !dd.wpatch16 || dd.in_norm || dd.offset || dd.wsplit_bs) return 1;
    dd.in_fmt = 0; dd.in0 = nullptr; dd.in1 = nullptr; dd.H = dd.OH; dd.W = dd.OW;
    dd.CoutPad = accflow_conv_coutpad(dd.Cout);
  }
  const accflow_conv_desc& d = dd;
  if ((!multi && (!d.in0 || !d.wpack || !d.ktab)) || d.B <= 0 || d.Cout <= 0 || d.OH <= 0 || d.OW <= 0) return 1;
  if (d.epi == ACCFLOW_EPI_TAPGEMM) {   // the result feeds the tap matrix of a following small-Cout conv inside the kernel
    if (multi || d.mode != ACCFLOW_CONV_F16X3 || !d.wpatch16 || !d.wscale16 || d.in_fmt != (d.in1 ? 3 : 1) || d.act != ACCFLOW_ACT_RELU ||
        (d.Cout & 127) || d.kws || d.stats || d.in_norm || d.cb || d.pre || d.offset || !d.tg_w16 || !d.tg_scale || !d.tg_out ||
        d.tg_rows < 1 || d.tg_rows > ACCFLOW_TAPGEMM_MAXROWS || d.tg_coutpad < 32 || (d.tg_coutpad & 31) ||
        d.tg_out_bs < (long long)d.tg_rows * d.OH * d.OW || (d.Cout > 128 && d.tg_out_ps <= 0) || !accflow_conv_direct_eligible(d) ||
        d.Kpad != accflow_conv_kpad(d.C0 + d.C1, d.KH, d.KW) || d.CoutPad != accflow_conv_coutpad(d.Cout))
      return 1;
    if ((((long long)(d.B - 1)) * d.in0_bs + accflow_s16_item_words(d.C0, d.H, d.W)) * 4 >= (1LL << 32)) return 1;
    if (d.in1 && (((long long)(d.B - 1)) * d.in1_bs + accflow_s16_item_words(d.C1, d.H, d.W)) * 4 >= (1LL << 32)) return 1;
    return 0;   // (`out` / `out16` are not written: the checks below do not apply)
  }
  // the fp32 destination may be omitted only when the S16 copy is requested (GRU_ZR: that concerns out2 = r*h; z stays)
  if (!d.out && (!d.out16 || d.epi == ACCFLOW_EPI_GRU_ZR)) return 1;
  if (d.epi == ACCFLOW_EPI_GRU_ZR && !d.out2 && !d.out16) return 1;
  if ((d.in_fmt || d.out16) && d.mode != ACCFLOW_CONV_F16X3) return 1;     // S16 tensors hold the fp16 split
  if (d.in_fmt & ~3) return 1;
  if (d.out16) {   // the S16 copy exists in the epilogue's specialised (epilogue, activation) forms only
    const int ea = d.epi * 8 + d.act;
    if (ea != ACCFLOW_EPI_STORE * 8 + ACCFLOW_ACT_NONE && ea != ACCFLOW_EPI_STORE * 8 + ACCFLOW_ACT_RELU &&
        ea != ACCFLOW_EPI_STORE * 8 + ACCFLOW_ACT_SIGMOID && ea != ACCFLOW_EPI_RES_RELU * 8 + ACCFLOW_ACT_RELU &&
        ea != ACCFLOW_EPI_RES_RELU * 8 + ACCFLOW_ACT_NONE &&
        ea != ACCFLOW_EPI_GRU_ZR * 8 + ACCFLOW_ACT_SIGMOID && ea != ACCFLOW_EPI_GRU_Q * 8 + ACCFLOW_ACT_TANH &&
        ea != ACCFLOW_EPI_ACCUM * 8 + ACCFLOW_ACT_NONE)
      return 1;
  }
  if (d.cb && ((d.cb & 31) || (d.epi != ACCFLOW_EPI_STORE && d.epi != ACCFLOW_EPI_ACCUM) || d.stats || d.Cout % d.cb)) return 1;
  if (!multi && (d.Kpad != accflow_conv_kpad(d.C0 + d.C1, d.KH, d.KW) || d.CoutPad != accflow_conv_coutpad(d.Cout))) return 1;
  if ((d.epi == ACCFLOW_EPI_RES_RELU || d.epi == ACCFLOW_EPI_ACCUM) && !d.e0) return 1;
  if (d.epi == ACCFLOW_EPI_GRU_ZR && (!d.e0 || (d.Cout & 1))) return 1;
  if (d.epi == ACCFLOW_EPI_GRU_ZR && d.out16 && ((d.Cout >> 1) & 7)) return 1;
  if (d.epi == ACCFLOW_EPI_GRU_Q && (!d.e0 || !d.e1)) return 1;
  if (d.pre && d.epi != ACCFLOW_EPI_GRU_ZR && d.epi != ACCFLOW_EPI_GRU_Q) return 1;
  if (d.offset && !d.dmask) return 1;
  if ((long long)d.B * d.OH * d.OW >= (1LL << 31)) return 1;
  // sources are addressed through 32-bit buffer offsets: each must span < 4 GiB (callers chunk the batch)
  if (!multi) {
    const long long w0 = (d.in_fmt & 1) ? accflow_s16_item_words(d.C0, d.H, d.W) : (long long)d.C0 * d.H * d.W;
    const long long w1 = (d.in_fmt & 2) ? accflow_s16_item_words(d.C1, d.H, d.W) : (long long)d.C1 * d.H * d.W;
    if ((((long long)(d.B - 1)) * d.in0_bs + w0) * 4 >= (1LL << 32)) return 1;
    if (d.in1 && (((long long)(d.B - 1)) * d.in1_bs + w1) * 4 >= (1LL << 32)) return 1;
  }
  if (d.out16 && (((long long)(d.B - 1)) * d.out16_bs + accflow_s16_item_words(d.Cout, d.OH, d.OW)) * 4 >= (1LL << 32)) return 1;
  if (d.stats && (d.epi != ACCFLOW_EPI_STORE || d.act != ACCFLOW_ACT_NONE || d.stat_slots <= 0)) return 1;
  return 0;
}

int conv_plan_direct(const accflow_conv_desc& d, int tc, bool want_stats, conv_plan& p) {
  if (!accflow_conv_direct_eligible(d)) return 1;
  const int rc = plan_direct_tile(d, tc, want_stats, p);
  if (!rc && tc == 2)   // the head on the 128-channel kernel, the tail on the 64-channel one
    p.ch0 = conv_tail_ch0(d, want_stats, (long long)d.B * cdiv(d.OW, DIR_TW) * cdiv(d.OH, DIR_TH) * cdiv(d.Cout, 128));
  return rc;
}

// the descriptors of channels [0, ch0) and [ch0, Cout): the channel-indexed pointers of the second advanced by ch0
void conv_tail_split(const accflow_conv_desc& d, int ch0, accflow_conv_desc& head, accflow_conv_desc& tail) {
  const long long OHW = (long long)d.OH * d.OW;
  head = d;
  tail = d;
  head.Cout = ch0;
  tail.Cout = d.Cout - ch0;
  tail.out = d.out ? d.out + ch0 * OHW : nullptr;
  if (d.bias) tail.bias = d.bias + ch0;
  if (d.wscale16) tail.wscale16 = d.wscale16 + ch0;
  if (d.e0) tail.e0 = d.e0 + ch0 * OHW;
  if (d.out16) tail.out16 = reinterpret_cast<char*>(d.out16) + (long long)(ch0 / 8) * 2 * OHW * 16;
  // packs are [term][step][octet][CoutPad][8]: the same CoutPad pitch, the channel origin moved by ch0 16-byte rows
  if (d.wpatch) tail.wpatch = reinterpret_cast<const char*>(d.wpatch) + (long long)ch0 * 16;
  if (d.wpatch16) tail.wpatch16 = reinterpret_cast<const char*>(d.wpatch16) + (long long)ch0 * 16;
}

int conv_plan_part(const accflow_conv_desc& part, const conv_plan& whole, bool tail, conv_plan& p) {
  if (whole.family == CONV_FAM_S16M) return plan_s16m_lay(part, tail ? 2 : 0, false, p);
  return plan_direct_tile(part, tail ? 1 : 2, false, p);
}

int conv_make_plan(accflow_conv_desc& d, bool want_stats, conv_plan& p) {
  const conv_switches& sw = conv_switches_get();
  if (d.epi == ACCFLOW_EPI_TAPGEMM) return conv_plan_direct(d, 2, want_stats, p);
  if (d.nsrc > 0) return plan_s16m(d, want_stats, p);
  // the encoders' stem (ACCFLOW_CONV_STEM=0: the im2col kernel, A/B)
  if (sw.stem && stem_eligible(d)) {
    plan_init(p, CONV_FAM_STEM, d.mode);
    p.slots = cdiv(d.OW, ST_TW) * cdiv(d.OH, ST_TH) * 2;   // one statistics slot per wave along the pixels (WP = 2)
    return 0;
  }
  // S16 sources of the in0 / in1 form: the direct kernel's S16 instantiations; ACCFLOW_S16M=1 sends them to the multi-source
  // kernel instead (same results bit for bit; in the refinement loop it measured 2 - 6 % slower per launch on one box,
  // profiles/r04_ab_s16m_vs_direct.txt, so the update block stays where it was)
  if (d.in_fmt && sw.s16m) {
    if (!accflow_conv_direct_eligible(d) || !d.wpatch16 || d.in_norm) return 1;
    if (d.in_fmt != (d.in1 ? 3 : 1)) return 1;
    s16m_from_legacy(d);
    return plan_s16m(d, want_stats, p);
  }
  if (d.in_fmt || d.out16 || d.cb) {
    // S16 tensors exist for the direct kernel only: its DMA loader reads them, its epilogue writes them.  No diversion
    // to another kernel whatever the grid size (the caller chose the format for this shape).
    if (!d.wpatch16 || d.stats || d.in_norm) return 1;
    if (d.in_fmt && d.in_fmt != (d.in1 ? 3 : 1)) return 1;
    return conv_plan_direct(d, d.Cout > 64 ? 2 : 1, want_stats, p);
  }
  if (d.Cout <= 4 && !d.offset && (d.epi == ACCFLOW_EPI_STORE || d.epi == ACCFLOW_EPI_ACCUM || d.epi == ACCFLOW_EPI_RES_RELU)) {
    const bool same = d.stride == 1 && d.OH == d.H && d.OW == d.W && d.KH * d.KW >= 2 && d.C0 + d.C1 >= 16 &&
                      (8 + d.KH - 1) * (16 + d.KW - 1) <= 192 && d.KH * d.KW <= 25 && (!d.in1 || d.C0 % 16 == 0);
    plan_init(p, same ? CONV_FAM_SMALL_PATCH : CONV_FAM_SMALL, d.mode);
    return 0;
  }
  if (accflow_conv_direct_eligible(d)) {
    const long long nb = (long long)d.B * cdiv(d.OW, DIR_TW) * cdiv(d.OH, DIR_TH);
    // with a split-K workspace small grids are split, not diverted (1x1 convolutions of < 512 channels: too few steps
    // per part to pay)
    const long long minb = (d.kws && (d.KH * d.KW >= 2 || d.C0 + d.C1 >= 512)) ? 0 : sw.patch_min_blocks;
    if (d.Cout > 64 && nb * cdiv(d.Cout, 128) >= minb) return conv_plan_direct(d, 2, want_stats, p);  // 128 ch
    if (nb * cdiv(d.Cout, 64) >= minb) return conv_plan_direct(d, 1, want_stats, p);                  //  64 ch
  }
  // the im2col kernel's fp16 form needs its own pack; without it (per-batch weights, <= 32 output channels, deformable
  // fp32 kernel, ...) the call runs bf16x6 arithmetic - and must not see the fp16 packs or the patch pack again
  if (d.mode == ACCFLOW_CONV_F16X3 && !(d.wsplit16 && !d.offset && d.Cout > 32)) {
    d.mode = ACCFLOW_CONV_BF16X6;
    d.wpatch = nullptr;
    d.wpatch16 = nullptr; d.wsplit16 = nullptr; d.wscale16 = nullptr;
  }
  if (d.wsplit_bs) {  // per-batch-item weights (GMA aggregation): 64-pixel tiles that never straddle items
    if ((d.OH * d.OW) % 64) return 1;
    if (d.mode != ACCFLOW_CONV_F16X3 && (d.mode == ACCFLOW_CONV_F32 || !d.wsplit || d.offset || d.Cout <= 32)) return 1;
    return plan_im2col(d, d.Cout > 64 ? 2 : 1, 1, want_stats, true, p);
  }
  if (d.mode == ACCFLOW_CONV_F16X3) {  // not direct-eligible (or too small a grid): im2col kernel on the fp16 pack
    d.wpatch16 = nullptr;
    return plan_im2col_auto(d, want_stats, p);
  }
  // split-bf16 matrix-core path (k order must be (c, tap): the tap-major pack is deformable-only)
  if (d.mode != ACCFLOW_CONV_F32 && d.wsplit && !d.offset && d.Cout > 32) return plan_im2col_auto(d, want_stats, p);
  return plan_f32(d, p);
}
