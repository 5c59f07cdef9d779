// Showing a flow: the Middlebury colour coding (Baker et al., ICCV 2007) as two launches.  accflow_flow_maxrad_f32 finds the
// scale - the per-sample (or whole-batch) maximum of |flow| - and leaves it in device memory; accflow_flow_to_rgb_u8 reads it
// from there and paints uint8 pixels, packed (B,H,W,3) or planar (B,3,H,W).  Written from the definition:
//     (u, v) = flow / (max_rad + 1e-5),  rad = |(u, v)|,  fk = (atan2(-v, -u) / pi + 1) / 2 * 54,  k0 = floor(fk),  f = fk - k0,
//     col = wheel[k0] + f (wheel[k0 + 1 mod 55] - wheel[k0]),  col = rad <= 1 ? 1 - rad (1 - col) : 0.75 col,  out = floor(255 col).
// No atomics; a maximum of non-negative floats has one value in any order, so a sample's scale has the same bits in any batch.
#include "common.h"

namespace {

// The wheel: 55 hues in six segments, RY 15, YG 6, GC 4, CB 11, BM 13, MR 6.  Inside a segment one channel is 255, one is 0
// and one ramps as floor(255 k / n), up or down.  Held as value / 255 in fp32: 255 / 255 is exactly 1.
constexpr int WHEEL_N = 55;
struct Wheel { float c[WHEEL_N][3]; };
constexpr Wheel make_wheel() {
  //                     n   full  ramp  rising
  constexpr int seg[6][4] = {{15, 0, 1, 1}, {6, 1, 0, 0}, {4, 1, 2, 1}, {11, 2, 1, 0}, {13, 2, 0, 1}, {6, 0, 2, 0}};
  Wheel w{};
  int col = 0;
  for (int s = 0; s < 6; ++s) {
    const int n = seg[s][0];
    for (int k = 0; k < n; ++k, ++col) {
      const int ramp = 255 * k / n;
      for (int ch = 0; ch < 3; ++ch) w.c[col][ch] = 0.0f;
      w.c[col][seg[s][1]] = 1.0f;
      w.c[col][seg[s][2]] = (float)(seg[s][3] ? ramp : 255 - ramp) / 255.0f;
    }
  }
  return w;
}
static_assert(make_wheel().c[54][0] == 1.0f && make_wheel().c[54][1] == 0.0f && make_wheel().c[54][2] == 43.0f / 255.0f, "wheel[54]");
static_assert(make_wheel().c[15][0] == 1.0f && make_wheel().c[15][1] == 1.0f && make_wheel().c[14][1] == 238.0f / 255.0f, "RY -> YG");

constexpr float VIZ_UNKNOWN = 1.0e9f;   // Middlebury's "unknown flow" threshold
constexpr float VIZ_EPS = 1.0e-5f;

// np.clip(x, 0, clip) for clip >= 0 (a negative clip: none).  Comparisons, not min / max: -0.0 and NaN pass through as numpy
// passes them, and the sign of a zero decides the side of the colour seam.
__device__ __forceinline__ float viz_clip(float x, float clip) {
  if (clip >= 0.0f) {
    x = x < 0.0f ? 0.0f : x;
    x = x > clip ? clip : x;
  }
  return x;
}

// (true for NaN and +-inf as well)
__device__ __forceinline__ bool viz_unknown(float u, float v) { return !(fabsf(u) <= VIZ_UNKNOWN) || !(fabsf(v) <= VIZ_UNKNOWN); }

// sqrt(u*u + v*v) with every operation rounded on its own, as numpy's float32 does it: no contraction into an FMA.
__device__ __forceinline__ float viz_radius(float u, float v) {
#pragma clang fp contract(off)
  const float uu = u * u;
  const float vv = v * v;
  const float s = uu + vv;
  return sqrtf(s);
}

// Stage 1 of the scale: a workgroup owns VIZ_RUN consecutive pixels of ONE sample and writes their maximum radius.
constexpr int VIZ_PER = 16;
constexpr int VIZ_RUN = 256 * VIZ_PER;

__global__ __launch_bounds__(256) void flow_maxrad_partial_kernel(const float* __restrict__ flow, long long f_bs, float clip,
                                                                  float* __restrict__ ws, int HW) {
  __shared__ float part[4];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* fl = flow + b * f_bs;
  const int run0 = blockIdx.x * VIZ_RUN;
  float m = 0.0f;
#pragma unroll
  for (int k = 0; k < VIZ_PER; ++k) {
    const int pix = run0 + k * 256 + (int)threadIdx.x;
    if (pix < HW) {
      const float u = viz_clip(fl[pix], clip), v = viz_clip(fl[HW + pix], clip);
      if (!viz_unknown(u, v)) m = fmaxf(m, viz_radius(u, v));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) part[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    ws[(long long)b * gridDim.x + blockIdx.x] = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

// Stage 2: one wave takes the maximum of n partials starting at ws[blockIdx.x * n] and writes it to `count` entries.
// Per sample: grid B, n = partials per sample, count 1.  Shared scale: grid 1, n = all partials, count B.
__global__ __launch_bounds__(64) void flow_maxrad_final_kernel(const float* __restrict__ ws, float* __restrict__ maxrad,
                                                               long long n, int count) {
  const int lane = threadIdx.x;
  const float* p = ws + (long long)blockIdx.x * n;
  float m = 0.0f;
  for (long long i = lane; i < n; i += 64) m = fmaxf(m, p[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  for (int i = lane; i < count; i += 64) maxrad[(long long)blockIdx.x * count + i] = m;
}

// One pixel: the three channels as bytes in a dword, R (or B with `BGR`) in the low byte.
template <bool BGR>
__device__ __forceinline__ unsigned viz_pixel(float u, float v, float clip, float scale, const float (*wheel)[3]) {
  u = viz_clip(u, clip);
  v = viz_clip(v, clip);
  if (viz_unknown(u, v)) return 0u;
  u = u / scale;                           // (a zero keeps its sign through the division by a positive scale)
  v = v / scale;
  const float rad = viz_radius(u, v);      // from the normalised components, as the definition has it
  const float a = atan2f(-v, -u) / 3.14159274f;           // atan2f's +-pi is this very float: a = +-1 exactly on the seam
  float fk = (a + 1.0f) / 2.0f * (float)(WHEEL_N - 1);
  fk = fminf(fmaxf(fk, 0.0f), (float)(WHEEL_N - 1));      // (only a NaN scale gets here out of range; the index stays in the table)
  const float fl = floorf(fk);
  const int k0 = (int)fl;
  const int k1 = k0 + 1 == WHEEL_N ? 0 : k0 + 1;
  const float f = fk - fl;
  unsigned px = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float c0 = wheel[k0][ch], c1 = wheel[k1][ch];
    float col = c0 + f * (c1 - c0);        // c0 == c1 gives c0 exactly: the saturated channel stays 1.0
    col = rad <= 1.0f ? 1.0f - rad * (1.0f - col) : 0.75f * col;
    const unsigned byte = (unsigned)(int)fminf(fmaxf(floorf(255.0f * col), 0.0f), 255.0f);
    px |= byte << (8 * (BGR ? 2 - ch : ch));
  }
  return px;
}

// Thread = 4 consecutive pixels -> 12 bytes -> 3 dword stores.
//   packed: a sample of 3 HW bytes may start at any byte address inside the batch (HW = 15: 45 bytes).  4 pixels are 12
//           bytes, so every group of a sample has the misalignment of its first one: the first p0 = (address mod 4) pixels
//           go out as bytes (3 p0 = -p0 = -address mod 4), the groups behind them are dword-aligned, and so are their stores.
//   planar: the sample's base is dword-aligned (checked by the host), plane ch starts ch HW bytes behind it; a plane that
//           starts off a dword boundary (HW mod 4 != 0) goes out as bytes.
// The up to 3 head and 3 tail pixels of a sample are taken by the threads behind the last group, one pixel each.
template <bool PLANAR, bool BGR>
__global__ __launch_bounds__(256) void flow_to_rgb_kernel(const float* __restrict__ flow, long long f_bs,
                                                          const float* __restrict__ maxrad, float clip,
                                                          unsigned char* __restrict__ out, long long o_bs, int HW) {
  static constexpr Wheel WHEEL = make_wheel();            // (a constant of the device code object; the host side has no copy)
  __shared__ float wheel[WHEEL_N][3];
  for (int i = threadIdx.x; i < WHEEL_N * 3; i += 256) wheel[i / 3][i % 3] = WHEEL.c[i / 3][i % 3];
  __syncthreads();
  const int b = blockIdx.y;
  const float* fl = flow + b * f_bs;
  unsigned char* o = out + b * o_bs;
  const float scale = maxrad[b] + VIZ_EPS;
  int head = PLANAR ? 0 : (int)((uintptr_t)o & 3);
  head = head < HW ? head : HW;
  const int groups = (HW - head) >> 2;
  const int tail0 = head + 4 * groups;                    // first tail pixel
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i < groups) {
    const int p = head + 4 * i;
    const f4u u4 = *reinterpret_cast<const f4u*>(fl + p);
    const f4u v4 = *reinterpret_cast<const f4u*>(fl + HW + p);
    const unsigned q0 = viz_pixel<BGR>(u4.x, v4.x, clip, scale, wheel), q1 = viz_pixel<BGR>(u4.y, v4.y, clip, scale, wheel);
    const unsigned q2 = viz_pixel<BGR>(u4.z, v4.z, clip, scale, wheel), q3 = viz_pixel<BGR>(u4.w, v4.w, clip, scale, wheel);
    if constexpr (!PLANAR) {
      unsigned* d = reinterpret_cast<unsigned*>(o + 3 * (long long)p);
      d[0] = q0 | (q1 << 24);
      d[1] = (q1 >> 8) | (q2 << 16);
      d[2] = (q2 >> 16) | (q3 << 8);
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int s = 8 * ch;
        const unsigned w = ((q0 >> s) & 255u) | (((q1 >> s) & 255u) << 8) | (((q2 >> s) & 255u) << 16) | (((q3 >> s) & 255u) << 24);
        unsigned char* d = o + (long long)ch * HW + p;
        if ((((long long)ch * HW) & 3) == 0) {
          *reinterpret_cast<unsigned*>(d) = w;
        } else {
          d[0] = (unsigned char)w, d[1] = (unsigned char)(w >> 8), d[2] = (unsigned char)(w >> 16), d[3] = (unsigned char)(w >> 24);
        }
      }
    }
    return;
  }
  const int e = i - groups;                               // edge slot: head pixels first, then the tail
  const int p = e < head ? e : tail0 + (e - head);
  if (p >= HW) return;
  const unsigned q = viz_pixel<BGR>(fl[p], fl[HW + p], clip, scale, wheel);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    o[PLANAR ? (long long)ch * HW + p : 3 * (long long)p + ch] = (unsigned char)(q >> (8 * ch));
}

constexpr int VIZ_EDGE = 6;   // head + tail pixels of a sample, at most

inline bool viz_dims_ok(int B, int H, int W) {
  // (one sample's pixels, and 3 bytes for each, are indexed with an int; blockIdx.y carries the sample)
  return B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= (0x7fffffffLL - VIZ_RUN) / 3;
}

}  // namespace

extern "C" long long accflow_flow_maxrad_ws_bytes(int B, int H, int W) {
  if (!viz_dims_ok(B, H, W)) return 0;
  return (long long)B * cdiv((long long)H * W, VIZ_RUN) * (long long)sizeof(float);
}

extern "C" int accflow_flow_maxrad_f32(const float* flow, long long f_bs, float clip, int shared, float* maxrad, float* ws, int B,
                                       int H, int W, void* stream) {
  if (!flow || !maxrad || !ws || !viz_dims_ok(B, H, W)) return 1;
  const int HW = H * W, nblk = cdiv(HW, VIZ_RUN);
  hipLaunchKernelGGL(flow_maxrad_partial_kernel, dim3(nblk, B), dim3(256), 0, as_stream(stream), flow, f_bs, clip, ws, HW);
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  if (shared)
    hipLaunchKernelGGL(flow_maxrad_final_kernel, dim3(1), dim3(64), 0, as_stream(stream), ws, maxrad, (long long)B * nblk, B);
  else
    hipLaunchKernelGGL(flow_maxrad_final_kernel, dim3(B), dim3(64), 0, as_stream(stream), ws, maxrad, (long long)nblk, 1);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_flow_to_rgb_u8(const float* flow, long long f_bs, const float* maxrad, float clip, unsigned char* out,
                                      long long o_bs, int planar, int bgr, int B, int H, int W, void* stream) {
  if (!flow || !maxrad || !out || !viz_dims_ok(B, H, W)) return 1;
  if (planar && (((uintptr_t)out & 3) || (B > 1 && (o_bs & 3)))) return 1;
  const int HW = H * W;
  const dim3 grid(cdiv((long long)(HW >> 2) + VIZ_EDGE, 256), B), block(256);
#define VIZ_LAUNCH(P, G) \
  hipLaunchKernelGGL((flow_to_rgb_kernel<P, G>), grid, block, 0, as_stream(stream), flow, f_bs, maxrad, clip, out, o_bs, HW)
  if (planar) {
    if (bgr) VIZ_LAUNCH(true, true); else VIZ_LAUNCH(true, false);
  } else {
    if (bgr) VIZ_LAUNCH(false, true); else VIZ_LAUNCH(false, false);
  }
#undef VIZ_LAUNCH
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
