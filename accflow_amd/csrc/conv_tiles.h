// Tile constants of the convolution kernels that the host-side plan (conv_plan.cpp) needs as well: each has its one
// definition here.  No HIP header: the plan unit is built by the host compiler alone; the device headers include this file.
#pragma once
#include "accflow_hip.h"

#ifdef __HIP__
#define ACCFLOW_TILE_FN __host__ __device__ __forceinline__
#else
#define ACCFLOW_TILE_FN inline
#endif

// direct kernel: tile, max patch pixels (3x3: 204, 1x5: 144, 5x1: 256), most channels of a normalise-on-load source
constexpr int DIR_TH = 4, DIR_TW = 32, DIR_NPMAX = 256;
constexpr int DIR_NORM_MAXC = 256;
// stem kernel (conv_stem.hip): output tile
constexpr int ST_TH = 4, ST_TW = 32;

// multi-source S16 kernel (conv_s16m_kernel.h): wave layouts - WC x WP waves of TCW x TP 32 x 32 accumulator tiles, TH x 32 pixels
struct s16m_layout { int WC, WP, TCW, TP, TH; };
constexpr s16m_layout S16M_LAYOUTS[4] = {
    {4, 1, 1, 4, 4},   // 128 ch x 128 px
    {2, 2, 1, 4, 8},   //  64 ch x 256 px
    {2, 2, 1, 2, 4},   //  64 ch x 128 px
    {1, 4, 3, 2, 8},   //  96 ch x 256 px
};
// (A 128 ch x 256 px layout - WC 4, TP 8: every A fragment feeds 8 pixel tiles instead of 4 - was built after ablation
// builds, tools/s16m_ablation.sh / profiles/r04_s16m_ablation.txt, showed the A stream from L2 to be the second largest
// cost of the loop after the MFMAs: -19 % kernel time without it, -3 % with half the LDS reads.  Its 128 accumulator
// registers leave 2 waves per SIMD, and it measured 3 - 6 % SLOWER than layout 0 on every update-block shape
// (profiles/r04_s16m_bench.txt keeps the column); removed again.)
template <int LAY> struct s16m_lay {
  static constexpr int WC = S16M_LAYOUTS[LAY].WC, WP = S16M_LAYOUTS[LAY].WP, TCW = S16M_LAYOUTS[LAY].TCW, TP = S16M_LAYOUTS[LAY].TP,
                       TH = S16M_LAYOUTS[LAY].TH;
};

constexpr int S16M_TW = 32;
// 16-byte chunks of one LDS stage: [2 terms][oc octets][pitch] with oc * pitch = S16M_CAP / 2
constexpr int s16m_cap(int TH) { return TH == 4 ? 1024 : 1536; }

// per-source quantities both sides of the pipeline derive from the descriptor
struct s16m_geom {
  int PW, NP, T, KW, oc, NPS, nch, nq, n16;
};
template <int TH>
ACCFLOW_TILE_FN s16m_geom s16m_geometry(const accflow_conv_src& S) {
  s16m_geom g;
  g.PW = S16M_TW + S.KW - 1;
  g.NP = (TH + S.KH - 1) * g.PW;
  g.T = S.KH * S.KW;
  g.KW = S.KW;
  g.nq = (g.NP + 63) >> 6;
  // 1x1 sub-kernels stage 4 octets per chunk when the patch is small enough (two 16-deep steps per barrier)
  g.oc = (g.T == 1 && g.nq * 64 * 8 <= s16m_cap(TH)) ? 4 : 2;
  g.NPS = s16m_cap(TH) / (2 * g.oc);
  g.n16 = (S.C + 15) >> 4;                        // 16-channel groups = steps per tap (the pack's step count: n16 * T)
  g.nch = (g.n16 + (g.oc >> 1) - 1) / (g.oc >> 1);  // (the last chunk of a 4-octet source may hold one group only)
  return g;
}
