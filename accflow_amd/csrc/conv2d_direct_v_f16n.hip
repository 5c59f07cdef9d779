// (-DACCFLOW_KPROF builds compile this body inside conv2d_direct.hip instead: the in-kernel stamp buffer is per translation unit)
#if !defined(ACCFLOW_KPROF) || defined(ACCFLOW_DIRECT_UNITY)
#include "conv2d_direct_kernel.h"
// instantiation group: fp16 split with normalise-on-load
// (round 6: the 3x3 shapes - conv2 of the feature encoder's residual blocks, extractor.py:56-58 - on the tap-specialised 9-tap loop
// with the gather loader: the patch of the next chunk is gathered at tap 0 and normalised / split / stored behind tap 8)
// (128-channel kernel only - conv_plan.cpp keeps the measurements)
int accflow_direct_launch_f16_norm(const accflow_conv_desc& d, int tc, bool kt9, dim3 grid, hipStream_t st) {
  if (kt9) {
    if (tc != 2 || d.KH != 3 || d.KW != 3) return 1;
    hipLaunchKernelGGL((conv2d_direct_bf16s_kernel<2, 2, true, true, true, false, 7, false, 9, 3>), grid, dim3(256), 0, st, d);
    ACCFLOW_RETURN_LAUNCH_STATUS();
  }
  if (tc == 2) hipLaunchKernelGGL((conv2d_direct_bf16s_kernel<2, 2, true, true, true>), grid, dim3(256), 0, st, d);
  else hipLaunchKernelGGL((conv2d_direct_bf16s_kernel<1, 2, true, false, true>), grid, dim3(256), 0, st, d);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
#endif
