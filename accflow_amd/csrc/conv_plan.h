// The one home of the convolution dispatch: which kernel family, tile, wave layout, loop variant and split-K part count a
// descriptor gets.  Pure host code - no device code, no hip* call (conv_plan.cpp builds with the host compiler alone, and
// tests/test_conv_plan.py runs it under the sanitizers without a GPU).  accflow_conv2d_f32 validates, plans, checks the
// launch against the plan and hands descriptor + plan to the family's launcher; accflow_conv_stat_slots and
// accflow_conv_in_norm_supported validate, plan and return a field of the plan.
#pragma once
#include "conv_tiles.h"

constexpr int ACCFLOW_TAPGEMM_MAXROWS = 18;   // ACCFLOW_EPI_TAPGEMM: rows of the second product (3x3 taps x 2 channels)

// Routing switches of the environment (A/B measurements and tests), read once per process.
struct conv_switches {
  bool direct_w4;              // ACCFLOW_DIRECT_W4 (default 1; 0: the 2 x 2 wave layout of the 128-channel direct kernel)
  bool direct_kt;              // ACCFLOW_DIRECT_KT (1; 0: the generic loop for the GRU's 5-tap convolutions)
  bool direct_kt9;             // ACCFLOW_DIRECT_KT9 (1; 0: the generic loop for 3x3)
  bool s16m;                   // ACCFLOW_S16M (0; 1: S16 sources of the in0 / in1 form run on the multi-source kernel)
  bool s16m_kt9;               // ACCFLOW_S16M_KT9 (1; 0: the multi-source kernel's generic loop for 3x3)
  int s16m_lay;                // ACCFLOW_S16M_LAY (-1 = automatic wave layout)
  bool stem;                   // ACCFLOW_CONV_STEM (1; 0: the stem runs on the im2col kernel)
  long long patch_min_blocks;  // ACCFLOW_PATCH_MIN_BLOCKS (300; 0 forces the direct kernel on small grids)
  int direct_ksplit;           // ACCFLOW_DIRECT_KSPLIT, ACCFLOW_IM2COL_KSPLIT (0; > 0: the part count of deep reductions)
  int im2col_ksplit;
};
const conv_switches& conv_switches_get();

enum conv_family {
  CONV_FAM_SMALL,        // conv2d_small_cout_kernel (Cout <= 4)
  CONV_FAM_SMALL_PATCH,  // conv2d_small_cout_patch_kernel
  CONV_FAM_STEM,         // conv_stem.hip
  CONV_FAM_DIRECT,       // conv2d_direct_kernel.h
  CONV_FAM_S16M,         // conv_s16m_kernel.h (multi-source)
  CONV_FAM_IM2COL,       // conv2d_bf16s_kernel.h (split-bf16 / fp16 im2col)
  CONV_FAM_F32           // conv2d_f32_kernel.h (fp32 MFMA)
};
enum conv_loop { CONV_LOOP_GENERIC, CONV_LOOP_TAP5, CONV_LOOP_TAP9 };

struct conv_plan {
  int family;
  int tc, tp, wc, wp;   // tile arguments: direct tc; im2col tc, tp; fp32-MFMA wc, wp, tc, tp
  int lay;              // multi-source wave layout
  int loop;             // direct / multi-source K loop (conv_loop) ...
  bool tapgemm, norm, w4;   // ... in its ACCFLOW_EPI_TAPGEMM / normalise-on-load form, in the 4 x 1 wave layout
  int mode;             // arithmetic after the f16x3 -> bf16x6 fallback
  int Z;                // split-K parts
  int ch0;              // > 0: channels [0, ch0) and [ch0, Cout) run as two launches (conv_tail_split, conv_plan_part)
  int slots;            // statistic slots per plane the kernel writes (0: it gathers none)
  bool can_norm;        // the route can normalise on load (accflow_conv_desc.in_norm)
};

// desc -> the private copy d the launch works on (accflow_conv2d_f32's rejections and normalisations); 0 = valid
int conv_validate(const accflow_conv_desc* desc, accflow_conv_desc& d);
// The plan of a validated descriptor, 0 = ok.  want_stats: statistics are, or will be, gathered on this route - a launch
// passes d.stats != NULL, accflow_conv_stat_slots passes true - which rules out the tail split and split-K.  d is completed
// on the way: the bf16x6 fallback clears the packs it must not use, ACCFLOW_S16M=1 rewrites in0 / in1 as src[].
int conv_make_plan(accflow_conv_desc& d, bool want_stats, conv_plan& p);
// the same with the direct kernel forced (tc = 2: 128-channel workgroups, 1: 64), for the library's own descriptors
int conv_plan_direct(const accflow_conv_desc& d, int tc, bool want_stats, conv_plan& p);
// plan.ch0 > 0: the two sub-descriptors, and the plan of one of them
void conv_tail_split(const accflow_conv_desc& d, int ch0, accflow_conv_desc& head, accflow_conv_desc& tail);
int conv_plan_part(const accflow_conv_desc& part, const conv_plan& whole, bool tail, conv_plan& p);

bool accflow_conv_direct_eligible(const accflow_conv_desc& d);
