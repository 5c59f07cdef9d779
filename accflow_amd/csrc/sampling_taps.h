// The bilinear sampling rule every gather of the path shares (sampling.hip, flow_metrics.hip).
#pragma once
#include "common.h"

struct WarpTaps {
  int o00, o01, o10, o11;
  float w00, w01, w10, w11;
};

// taps of F.grid_sample(bilinear, zeros, align_corners=True) at pixel coords (sx, sy); weights of
// out-of-plane corners are zeroed and their offsets clamped to 0 so loads stay in bounds.
__device__ __forceinline__ WarpTaps make_taps(float sx, float sy, int H, int W) {
  sx = fminf(fmaxf(sx, -1.0e6f), 1.0e6f);
  sy = fminf(fmaxf(sy, -1.0e6f), 1.0e6f);
  const float fx0 = floorf(sx), fy0 = floorf(sy);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const float ax = sx - fx0, ay = sy - fy0;
  const bool xin0 = (unsigned)x0 < (unsigned)W, xin1 = (unsigned)(x0 + 1) < (unsigned)W;
  const bool yin0 = (unsigned)y0 < (unsigned)H, yin1 = (unsigned)(y0 + 1) < (unsigned)H;
  WarpTaps t;
  t.o00 = (xin0 && yin0) ? y0 * W + x0 : 0;
  t.o01 = (xin1 && yin0) ? y0 * W + x0 + 1 : 0;
  t.o10 = (xin0 && yin1) ? (y0 + 1) * W + x0 : 0;
  t.o11 = (xin1 && yin1) ? (y0 + 1) * W + x0 + 1 : 0;
  t.w00 = (xin0 && yin0) ? (1.0f - ax) * (1.0f - ay) : 0.0f;
  t.w01 = (xin1 && yin0) ? ax * (1.0f - ay) : 0.0f;
  t.w10 = (xin0 && yin1) ? (1.0f - ax) * ay : 0.0f;
  t.w11 = (xin1 && yin1) ? ax * ay : 0.0f;
  return t;
}
__device__ __forceinline__ float tap_sample(const float* __restrict__ plane, const WarpTaps& t) {
  return plane[t.o00] * t.w00 + plane[t.o01] * t.w01 + plane[t.o10] * t.w10 + plane[t.o11] * t.w11;
}
