// Judging a flow: the forward-backward occlusion masks (test_cvo.py:53-78) and the per-sample sums behind the end-point-error
// metrics (test_cvo.py:81-101, loss.py:37-45).  No float atomics: every reduction has one fixed order, so a sample's row of
// sums has the same bits whatever the batch size is and wherever in the batch the sample sits.
#include "common.h"
#include "sampling_taps.h"

namespace {

// The forward-backward decision of one pixel (x, y) for the flow (u, v) that starts there; (ou, ov) is the OTHER direction's
// flow at the same pixel and `other` its (2, H, W) block: 1 = occluded, i.e. |flow + other(p + flow)| > alpha (|flow| + |other|)
// + beta.  The sum of the two norms commutes, so both masks of a pixel compare against the same threshold.  Written with
// explicit FMAs: the bits must not depend on which kernel the function is inlined into.  A NaN compares false: 0.
__device__ __forceinline__ float fb_occ_bit(float u, float v, float ou, float ov, const float* __restrict__ other, int HW,
                                            int x, int y, int H, int W, float alpha, float beta) {
  const float mag = sqrtf(__builtin_fmaf(u, u, v * v)) + sqrtf(__builtin_fmaf(ou, ou, ov * ov));
  const float thr = __builtin_fmaf(alpha, mag, beta);
  const WarpTaps t = make_taps((float)x + u, (float)y + v, H, W);
  const float du = u + tap_sample(other, t), dv = v + tap_sample(other + HW, t);
  return sqrtf(__builtin_fmaf(du, du, dv * dv)) > thr ? 1.0f : 0.0f;
}

// calc_occ_mask: thread = pixel
template <bool BW, bool FW>
__global__ __launch_bounds__(256) void fb_occlusion_kernel(const float* __restrict__ bflow, long long b_bs,
                                                           const float* __restrict__ fflow, long long f_bs,
                                                           float* __restrict__ occ_bw, long long obw_bs,
                                                           float* __restrict__ occ_fw, long long ofw_bs, float alpha,
                                                           float beta, int B, int H, int W) {
  const int HW = H * W;
  const long long gp = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gp >= (long long)B * HW) return;
  const int b = (int)(gp / HW), pix = (int)(gp - (long long)b * HW);
  const int y = pix / W, x = pix - y * W;
  const float* bf = bflow + b * b_bs;
  const float* ff = fflow + b * f_bs;
  const float bu = bf[pix], bv = bf[HW + pix], fu = ff[pix], fv = ff[HW + pix];
  if constexpr (BW) occ_bw[b * obw_bs + pix] = fb_occ_bit(bu, bv, fu, fv, ff, HW, x, y, H, W, alpha, beta);
  if constexpr (FW) occ_fw[b * ofw_bs + pix] = fb_occ_bit(fu, fv, bu, bv, bf, HW, x, y, H, W, alpha, beta);
}

// Stage 1 of the sums: a workgroup owns METRICS_RUN consecutive pixels of ONE sample (a constant: the partition of a sample
// does not depend on B).  Thread t takes pixels run0 + t + 256 k; its METRICS_PER values go into 4 interleaved accumulators
// added as (a0 + a1) + (a2 + a3); then the xor butterfly over the 64 lanes, then the 4 waves through LDS as (w0 + w1) +
// (w2 + w3).  The counts are small integers in fp32 (<= METRICS_RUN), hence exact.
constexpr int METRICS_PER = 16;
constexpr int METRICS_RUN = 256 * METRICS_PER;

template <int MODE>
__global__ __launch_bounds__(256) void flow_metrics_partial_kernel(const float* __restrict__ pred, long long p_bs,
                                                                   const float* __restrict__ gt, long long g_bs,
                                                                   const float* __restrict__ mask, long long m_bs,
                                                                   const float* __restrict__ fflow, long long f_bs,
                                                                   float alpha, float beta, float* __restrict__ ws, int H,
                                                                   int W) {
  __shared__ float part[4][8];
  const int HW = H * W;
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* pr = pred + b * p_bs;
  const float* g = gt + b * g_bs;
  const float* ff = MODE == 2 ? fflow + b * f_bs : nullptr;
  const float* mk = MODE == 1 ? mask + b * m_bs : nullptr;
  float a[4][8];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) a[q][j] = 0.0f;
  const int run0 = blockIdx.x * METRICS_RUN;
#pragma unroll
  for (int k = 0; k < METRICS_PER; ++k) {
    const int pix = run0 + k * 256 + (int)threadIdx.x;
    if (pix < HW) {
      const float gu = g[pix], gv = g[HW + pix];
      const float dx = pr[pix] - gu, dy = pr[HW + pix] - gv;
      const float epe = sqrtf(__builtin_fmaf(dx, dx, dy * dy));
      float m = 0.0f;
      if constexpr (MODE == 1) m = mk[pix];
      if constexpr (MODE == 2) {
        const int y = pix / W, x = pix - y * W;
        m = fb_occ_bit(gu, gv, ff[pix], ff[HW + pix], ff, HW, x, y, H, W, alpha, beta);
      }
      float* s = a[k & 3];
      s[0] += epe;
      if constexpr (MODE != 0) {
        s[1] = __builtin_fmaf(epe, m, s[1]);
        s[2] += m;
      }
      s[3] += epe < 1.0f ? 1.0f : 0.0f;
      s[4] += epe < 3.0f ? 1.0f : 0.0f;
      s[5] += epe < 5.0f ? 1.0f : 0.0f;
      s[6] += fabsf(dx) + fabsf(dy);
      s[7] += 1.0f;
    }
  }
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = (a[0][j] + a[1][j]) + (a[2][j] + a[3][j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    r[j] = v;
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) part[wave][j] = r[j];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int j = threadIdx.x;
    ws[((long long)b * gridDim.x + blockIdx.x) * 8 + j] = (part[0][j] + part[1][j]) + (part[2][j] + part[3][j]);
  }
}

// Stage 2: one wave per sample.  The wave reads 8 partials (64 floats) at a time; column j = lane & 7 adds them in index
// order, in double.
__global__ __launch_bounds__(64) void flow_metrics_final_kernel(const float* __restrict__ ws, double* __restrict__ sums,
                                                                int nblk) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* p = ws + (long long)b * nblk * 8;
  const int n = nblk * 8;
  double acc = 0.0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const float v = i0 + lane < n ? p[i0 + lane] : 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float vk = __shfl(v, (lane & 7) + 8 * k, 64);
      if (i0 + 8 * k < n) acc += (double)vk;
    }
  }
  if (lane < 8) sums[(long long)b * 8 + lane] = acc;
}

inline bool metrics_dims_ok(int B, int H, int W) {
  // (one sample's pixels are indexed with an int; blockIdx.y carries the sample)
  return B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL - METRICS_RUN;
}

}  // namespace

extern "C" int accflow_fb_occlusion_f32(const float* bflow, long long b_bs, const float* fflow, long long f_bs, float* occ_bw,
                                        long long obw_bs, float* occ_fw, long long ofw_bs, float alpha, float beta, int B, int H,
                                        int W, void* stream) {
  if (!bflow || !fflow || (!occ_bw && !occ_fw) || B <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return 1;
  const long long np = (long long)B * H * W;
  if (np > 256LL * 0x7fffffffLL) return 1;   // (the grid's x extent)
  const dim3 grid(cdiv(np, 256)), block(256);
  if (occ_bw && occ_fw)
    hipLaunchKernelGGL((fb_occlusion_kernel<true, true>), grid, block, 0, as_stream(stream), bflow, b_bs, fflow, f_bs, occ_bw,
                       obw_bs, occ_fw, ofw_bs, alpha, beta, B, H, W);
  else if (occ_bw)
    hipLaunchKernelGGL((fb_occlusion_kernel<true, false>), grid, block, 0, as_stream(stream), bflow, b_bs, fflow, f_bs, occ_bw,
                       obw_bs, occ_fw, ofw_bs, alpha, beta, B, H, W);
  else
    hipLaunchKernelGGL((fb_occlusion_kernel<false, true>), grid, block, 0, as_stream(stream), bflow, b_bs, fflow, f_bs, occ_bw,
                       obw_bs, occ_fw, ofw_bs, alpha, beta, B, H, W);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" long long accflow_flow_metrics_ws_bytes(int B, int H, int W) {
  if (!metrics_dims_ok(B, H, W)) return 0;
  return (long long)B * cdiv((long long)H * W, METRICS_RUN) * 8 * (long long)sizeof(float);
}

extern "C" int accflow_flow_metrics_f32(const float* pred, long long p_bs, const float* gt, long long g_bs, const float* mask,
                                        long long m_bs, const float* fflow, long long f_bs, int mode, float alpha, float beta,
                                        double* sums, float* ws, int B, int H, int W, void* stream) {
  if (!pred || !gt || !sums || !ws || !metrics_dims_ok(B, H, W) || mode < 0 || mode > 2) return 1;
  if ((mode == 1 && !mask) || (mode == 2 && !fflow)) return 1;
  const int nblk = cdiv((long long)H * W, METRICS_RUN);
  const dim3 grid(nblk, B), block(256);
  if (mode == 0)
    hipLaunchKernelGGL((flow_metrics_partial_kernel<0>), grid, block, 0, as_stream(stream), pred, p_bs, gt, g_bs, mask, m_bs,
                       fflow, f_bs, alpha, beta, ws, H, W);
  else if (mode == 1)
    hipLaunchKernelGGL((flow_metrics_partial_kernel<1>), grid, block, 0, as_stream(stream), pred, p_bs, gt, g_bs, mask, m_bs,
                       fflow, f_bs, alpha, beta, ws, H, W);
  else
    hipLaunchKernelGGL((flow_metrics_partial_kernel<2>), grid, block, 0, as_stream(stream), pred, p_bs, gt, g_bs, mask, m_bs,
                       fflow, f_bs, alpha, beta, ws, H, W);
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(flow_metrics_final_kernel, dim3(B), dim3(64), 0, as_stream(stream), ws, sums, nblk);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
