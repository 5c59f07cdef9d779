#include "conv2d_direct_kernel.h"

namespace {

// one launch of the direct kernel as planned (conv_plan.cpp: tile, wave layout, loop variant, split-K parts)
int launch_conv_direct(const accflow_conv_desc& d, const conv_plan& p, hipStream_t st) {
  const int tiles = cdiv(d.OW, DIR_TW) * cdiv(d.OH, DIR_TH);
  dim3 grid((unsigned)((long long)d.B * tiles), cdiv(d.Cout, 2 * p.tc * 32), p.Z);
  const bool f16 = p.mode == ACCFLOW_CONV_F16X3 && d.wpatch16;
  const int nt = p.mode == ACCFLOW_CONV_BF16X3 ? 2 : 3;
  int rc;
  if (p.tapgemm) {
    rc = p.loop == CONV_LOOP_TAP9 ? accflow_direct_launch_s16k9(d, 2, true, grid, st) : accflow_direct_launch_s16tg(d, grid, st);
  } else if (d.in_fmt) {  // S16 sources: the fp16 kernel with the DMA loader
    if (p.loop == CONV_LOOP_TAP5) rc = accflow_direct_launch_s16k(d, 5, grid, st);
    else if (p.loop == CONV_LOOP_TAP9) rc = accflow_direct_launch_s16k9(d, p.tc, false, grid, st);
    else rc = accflow_direct_launch_s16(d, p.tc, grid, st);
  } else if (p.norm) {
    rc = f16 ? accflow_direct_launch_f16_norm(d, p.tc, p.loop == CONV_LOOP_TAP9, grid, st) : accflow_direct_launch_bf16_norm(d, p.tc, nt, grid, st);
  } else {
    rc = f16 ? accflow_direct_launch_f16(d, p.tc, p.w4, grid, st) : accflow_direct_launch_bf16(d, p.tc, nt, p.w4, grid, st);
  }
  if (rc) return rc;
  if (p.Z > 1) return conv_ksplit_reduce_launch(d, p.Z, st);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

}  // namespace

int accflow_launch_conv_direct(const accflow_conv_desc& d, const conv_plan& p, hipStream_t st) {
  if (!p.ch0) return launch_conv_direct(d, p, st);
  // Cout = 128 m + 64: the 128 m channels on the 128-channel kernel, the last 64 on the 64-channel kernel (conv_tail_ch0)
  accflow_conv_desc part[2];
  conv_tail_split(d, p.ch0, part[0], part[1]);
  for (int i = 0; i < 2; ++i) {
    conv_plan pp;
    int rc = conv_plan_part(part[i], p, i == 1, pp);
    if (!rc) rc = launch_conv_direct(part[i], pp, st);
    if (rc) return rc;
  }
  return 0;
}

#ifdef ACCFLOW_KPROF
#define ACCFLOW_DIRECT_UNITY
#include "corr_gemm.hip"
#include "conv2d_direct_v_s16.hip"
#include "conv2d_direct_v_s16tg.hip"
#include "conv2d_direct_v_s16k.hip"
#include "conv2d_direct_v_s16k9.hip"
#include "conv2d_direct_v_f16.hip"
#include "conv2d_direct_v_f16n.hip"
#include "conv2d_direct_v_bf16x6.hip"
#include "conv2d_direct_v_bf16x3.hip"
#include "conv2d_direct_v_bf16n.hip"
extern "C" int accflow_debug_occupancy(int* out) {
  int n = 0;
  hipOccupancyMaxActiveBlocksPerMultiprocessor(&out[n++], conv2d_direct_bf16s_kernel<2, 3>, 256, 0);
  hipOccupancyMaxActiveBlocksPerMultiprocessor(&out[n++], conv2d_direct_bf16s_kernel<2, 2, true>, 256, 0);
  hipOccupancyMaxActiveBlocksPerMultiprocessor(&out[n++], conv2d_direct_bf16s_kernel<1, 3>, 256, 0);
  hipDeviceProp_t pr; hipGetDeviceProperties(&pr, 0);
  out[n++] = (int)(pr.maxSharedMemoryPerMultiProcessor / 1024); out[n++] = (int)(pr.sharedMemPerBlock / 1024);
  out[n++] = pr.regsPerMultiprocessor; out[n++] = pr.regsPerBlock;
  return n;
}
extern "C" int accflow_debug_kprof(unsigned long long* out, int reset) {
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(out, HIP_SYMBOL(g_kprof), 4096 * 16 * 8);
  if (reset) { void* p; hipGetSymbolAddress(&p, HIP_SYMBOL(g_kprof)); hipMemset(p, 0, 4096 * 16 * 8); }
  return (int)hipGetLastError();
}
#endif
