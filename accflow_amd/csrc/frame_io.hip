// The two ends of a video run, one launch each; both only move bytes (no LDS, no atomics).
//   accflow_frames_from_u8: 8-bit frames as a decoder hands them out - packed (N,H,W,3) or planar (N,3,H,W), RGB or BGR, any
//     base address and pitch - to the estimators' input: float32 (N,3,H+pt+pb,W+pl+pr), normalised to [-1, 1] and padded by
//     replication.      out[n,c,y,x] = g(src[n, clamp(y-pt,0,H-1), clamp(x-pl,0,W-1), c']),   c' = bgr ? 2-c : c,
//     g(v) = 2 (v / 255) - 1 with every step rounded to fp32 (a correctly rounded division: torch's 2 * (x / 255.0) - 1), or (float)v.
//   accflow_flow_export: a crop window of a flow (N,2,Hp,Wp) to the payload of a flow file: float32 (N,H,W,2) interleaved
//     (Middlebury .flo) or uint16 (N,H,W,3) = (code(u), code(v), valid) (KITTI / CVO 16-bit PNG), optionally byte-swapped.
// and the same two with a resampling inside the launch (run at a working size, hand the flow back at the source size):
//   accflow_frames_from_u8_resized: the frames resampled to (out_h, out_w) - bilinear with exact rational coordinates, or
//     integer area means - before the normalisation and the padding;
//   accflow_flow_resize: the crop window resampled bilinearly to (H, W), taps clamped inside the window, vectors rescaled,
//     in the two file codings or as a planar flow.
#include "common.h"

namespace {

struct __attribute__((packed, aligned(4))) u3u { unsigned x, y, z; };
struct __attribute__((packed, aligned(4))) u6u { unsigned w[6]; };
// 16 bytes as ONE vector access on a dword-aligned address.  (f4u, a struct, is taken apart into four scalar accesses first;
// the compiler then folds them into the scalar accesses of a tail path next to them and the 16 bytes go out as 12 + 4.)
typedef f32x4 f32x4u __attribute__((aligned(4)));

template <bool NORM>
__device__ __forceinline__ float frame_value(unsigned v) {
  const float f = (float)v;
  if constexpr (!NORM) return f;
  const float q = __fdiv_rn(f, 255.0f);
  return 2.0f * q - 1.0f;                  // 2 q is exact: contracted into an FMA or not, this is one rounding
}

// Thread = 4 consecutive output pixels of one row, all three channels: 12 source bytes in, 3 x 16 bytes out.
//   fast path: the 4 pixels are interior (no clamp in x) and their source bytes start on a dword - packed: 3 dword loads;
//              planar: one dword load per plane, decided plane by plane.
//   byte path: everything else - the pad columns, a misaligned base or pitch, the last group of a row with Wp % 4 != 0.
// The value of a byte does not depend on the path, so neither does the result.
template <bool PLANAR, bool NORM>
__global__ __launch_bounds__(256) void frames_from_u8_kernel(const unsigned char* __restrict__ src, long long s_bs, long long s_row,
                                                             long long s_plane, int bgr, float* __restrict__ out, long long o_bs,
                                                             int H, int W, int pl, int pt, int Hp, int Wp, int gpr) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= Hp * gpr) return;
  const int y = i / gpr, x0 = (i - y * gpr) * 4;
  const int n = blockIdx.y;
  int sy = y - pt;
  sy = sy < 0 ? 0 : (sy > H - 1 ? H - 1 : sy);
  const unsigned char* row = src + n * s_bs + sy * s_row;
  const int sx0 = x0 - pl;
  const bool interior = sx0 >= 0 && sx0 + 3 <= W - 1;      // (then x0 + 3 < Wp as well)
  unsigned v[3][4];                                        // [source channel][pixel]
  if (interior) {
    if constexpr (!PLANAR) {
      const unsigned char* p = row + 3 * (long long)sx0;
      if (((uintptr_t)p & 3) == 0) {
        const u3u w = *reinterpret_cast<const u3u*>(p);
        const unsigned d[3] = {w.x, w.y, w.z};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c][k] = (d[(3 * k + c) >> 2] >> (8 * ((3 * k + c) & 3))) & 255u;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c][k] = p[3 * k + c];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned char* p = row + c * s_plane + sx0;
        if (((uintptr_t)p & 3) == 0) {
          const unsigned d = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
          for (int k = 0; k < 4; ++k) v[c][k] = (d >> (8 * k)) & 255u;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[c][k] = p[k];
        }
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int sx = sx0 + k;                                    // (clamped: in the row even for a pixel beyond Wp, which is not stored)
      sx = sx < 0 ? 0 : (sx > W - 1 ? W - 1 : sx);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c][k] = PLANAR ? row[c * s_plane + sx] : row[3 * (long long)sx + c];
    }
  }
  float* o = out + n * o_bs + (long long)y * Wp + x0;
  const long long plane = (long long)Hp * Wp;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int cs = bgr ? 2 - c : c;
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned b = cs == 0 ? v[0][k] : (cs == 1 ? v[1][k] : v[2][k]);
      r[k] = frame_value<NORM>(b);
    }
    float* d = o + c * plane;
    if (x0 + 3 < Wp) {
      *reinterpret_cast<f32x4u*>(d) = f32x4{r[0], r[1], r[2], r[3]};
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (x0 + k < Wp) d[k] = r[k];
    }
  }
}

// code(f) = trunc(min(max(s f + 32768, 0), 65535)), the product and the sum rounded on their own as numpy's float32 does it.
__device__ __forceinline__ unsigned flow_code(float f, float s) {
#pragma clang fp contract(off)
  const float m = s * f;
  const float a = m + 32768.0f;
  return (unsigned)(int)fminf(fmaxf(a, 0.0f), 65535.0f);
}

__device__ __forceinline__ bool flow_finite(float f) { return fabsf(f) <= 3.402823466e38f; }   // (false for NaN and +-inf)

// A thread's 4 consecutive pixels (the first cnt of them) from pixel `pix` of the output sample at `o_n`, in one of the codings
//   0: float32 (H,W,2) interleaved, 2 x 16 bytes;   2: float32 (2,H,W) planar, the v plane `plane` elements behind u's;
//   1: uint16 (H,W,3): 12 samples = 24 bytes, as 6 dwords where the group starts on a dword (the sample base and the parity
//      of y W decide), as 12 halves otherwise.
template <int CODING>
__device__ __forceinline__ void flow_store(unsigned char* o_n, long long pix, long long plane, int cnt, const float (&u)[4],
                                           const float (&v)[4], float scale, int swap) {
  if constexpr (CODING == 0) {
    float* o = reinterpret_cast<float*>(o_n) + 2 * pix;
    if (cnt == 4) {
      *reinterpret_cast<f32x4u*>(o) = f32x4{u[0], v[0], u[1], v[1]};
      *reinterpret_cast<f32x4u*>(o + 4) = f32x4{u[2], v[2], u[3], v[3]};
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (k < cnt) o[2 * k] = u[k], o[2 * k + 1] = v[k];
    }
  } else if constexpr (CODING == 2) {
    float* o = reinterpret_cast<float*>(o_n) + pix;
    if (cnt == 4) {
      *reinterpret_cast<f32x4u*>(o) = f32x4{u[0], u[1], u[2], u[3]};
      *reinterpret_cast<f32x4u*>(o + plane) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (k < cnt) o[k] = u[k], o[plane + k] = v[k];
    }
  } else {
    unsigned s[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool fu = flow_finite(u[k]), fv = flow_finite(v[k]);
      s[3 * k] = fu ? flow_code(u[k], scale) : 0u;
      s[3 * k + 1] = fv ? flow_code(v[k], scale) : 0u;
      s[3 * k + 2] = fu && fv ? 1u : 0u;
    }
    if (swap) {
#pragma unroll
      for (int j = 0; j < 12; ++j) s[j] = ((s[j] >> 8) | (s[j] << 8)) & 0xffffu;
    }
    unsigned char* o = o_n + 6 * pix;
    if (cnt == 4 && ((uintptr_t)o & 3) == 0) {
      u6u w;
#pragma unroll
      for (int j = 0; j < 6; ++j) w.w[j] = s[2 * j] | (s[2 * j + 1] << 16);
      *reinterpret_cast<u6u*>(o) = w;
    } else {
      unsigned short* h = reinterpret_cast<unsigned short*>(o);
#pragma unroll
      for (int j = 0; j < 12; ++j)
        if (j < 3 * cnt) h[j] = (unsigned short)s[j];
    }
  }
}

// Thread = 4 consecutive pixels of one row of the crop window: loaded as 2 x 16 bytes, stored by flow_store.
template <bool U16>
__global__ __launch_bounds__(256) void flow_export_kernel(const float* __restrict__ flow, long long f_bs, int Hp, int Wp, int y0,
                                                          int x0, int H, int W, unsigned char* __restrict__ out, long long o_bs,
                                                          float scale, int swap, int gpr) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= H * gpr) return;
  const int y = i / gpr, x = (i - y * gpr) * 4;
  const int n = blockIdx.y;
  const float* pu = flow + n * f_bs + (long long)(y0 + y) * Wp + (x0 + x);
  const float* pv = pu + (long long)Hp * Wp;
  const int cnt = W - x < 4 ? W - x : 4;
  float u[4], v[4];
  if (cnt == 4) {
    const f32x4 a = *reinterpret_cast<const f32x4u*>(pu), b = *reinterpret_cast<const f32x4u*>(pv);
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = a[k], v[k] = b[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int kk = k < cnt ? k : 0;
      u[k] = pu[kk], v[k] = pv[kk];
    }
  }
  flow_store<U16 ? 1 : 0>(out + n * o_bs, (long long)y * W + x, 0, cnt, u, v, scale, swap);
}

// ---- resampling: the geometry both resizing kernels share ----
// Output index x of n_out over n_in source samples, pixel centres at half-integers (cv2.INTER_LINEAR, align_corners=False): the
// source coordinate is the rational ((2x+1) n_in - n_out) / (2 n_out).  i0 = its floor and f = the remainder over the
// denominator, ONE correctly rounded fp32 division of two integers below 2^17 - no float product of a coordinate anywhere.
// All sides <= RESIZE_MAX_SIDE, so that (2x+1) n_in < 2^31 and 32-bit integers are enough.  The numerator is negative only
// at the left / top border of an enlargement, and there above -2 n_out: its floor quotient is -1.
constexpr int RESIZE_MAX_SIDE = 32768;

struct resize_tap { int a, b; float f; };   // the taps clamp(i0), clamp(i0 + 1) into [0, n_in - 1] and the weight of b

__device__ __forceinline__ resize_tap make_tap(int x, int n_in, int n_out) {
  const int den = 2 * n_out, num = (2 * x + 1) * n_in - n_out;
  const int i0 = num >= 0 ? num / den : -1;
  resize_tap t;
  t.f = __fdiv_rn((float)(num - i0 * den), (float)den);
  t.a = i0 < 0 ? 0 : (i0 > n_in - 1 ? n_in - 1 : i0);
  t.b = i0 + 1 > n_in - 1 ? n_in - 1 : i0 + 1;
  return t;
}

// f == 0 selects a: a resize to the same size is the identity bit for bit, whatever stands in the neighbour (NaN, inf).
// The difference, the product and the sum are rounded one by one (no FMA): the result does not depend on the caller.
__device__ __forceinline__ float lerp_sel(float f, float a, float b) {
#pragma clang fp contract(off)
  const float d = b - a;
  const float m = f * d;
  return f == 0.0f ? a : a + m;
}

// horizontal first, then vertical
__device__ __forceinline__ float bilerp(float fx, float fy, float v00, float v01, float v10, float v11) {
  return lerp_sel(fy, lerp_sel(fx, v00, v01), lerp_sel(fx, v10, v11));
}

template <bool NORM>
__device__ __forceinline__ float frame_value_f(float f) {       // frame_value of a blended level; the same bits for a whole one
  if constexpr (!NORM) return f;
  const float q = __fdiv_rn(f, 255.0f);
  return 2.0f * q - 1.0f;
}

// frames_from_u8_kernel with a resampling in front: thread = 4 consecutive pixels of one row of the PADDED output, all
// three channels.  (y, x) is clamped into the resized frame first - replicate padding of the resized frame, the pad pixels
// computed as the border pixels are - then
//   AREA == false: the vertical tap pair from y, a horizontal pair per pixel from x, 2 x 2 x 3 bytes blended per pixel;
//   AREA == true : the window rows floor(y H / oh) .. ceil((y+1) H / oh) - 1, columns likewise (F.interpolate's "area"):
//                  an integer sum of bytes and one division float(sum) / float(count).
template <bool PLANAR, bool NORM, bool AREA>
__global__ __launch_bounds__(256) void frames_from_u8_resized_kernel(const unsigned char* __restrict__ src, long long s_bs,
                                                                     long long s_row, long long s_plane, int bgr,
                                                                     float* __restrict__ out, long long o_bs, int H, int W, int oh,
                                                                     int ow, int pl, int pt, int Hp, int Wp, int gpr) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= Hp * gpr) return;
  const int y = i / gpr, x0 = (i - y * gpr) * 4;
  const int n = blockIdx.y;
  int ry = y - pt;
  ry = ry < 0 ? 0 : (ry > oh - 1 ? oh - 1 : ry);
  const unsigned char* base = src + n * s_bs;
  float r[3][4];                                           // [source channel][pixel], in levels 0..255
  if constexpr (!AREA) {
    const resize_tap ty = make_tap(ry, H, oh);
    const unsigned char* row0 = base + ty.a * s_row;
    const unsigned char* row1 = base + ty.b * s_row;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int rx = x0 + k - pl;                                // (clamped: in the frame even for a pixel beyond Wp, which is not stored)
      rx = rx < 0 ? 0 : (rx > ow - 1 ? ow - 1 : rx);
      const resize_tap tx = make_tap(rx, W, ow);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const long long pa = PLANAR ? c * s_plane + tx.a : 3 * (long long)tx.a + c;
        const long long pb = PLANAR ? c * s_plane + tx.b : 3 * (long long)tx.b + c;
        r[c][k] = bilerp(tx.f, ty.f, (float)row0[pa], (float)row0[pb], (float)row1[pa], (float)row1[pb]);
      }
    }
  } else {
    const int r0 = (int)(((long long)ry * H) / oh), r1 = (int)(((long long)(ry + 1) * H + oh - 1) / oh);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int rx = x0 + k - pl;
      rx = rx < 0 ? 0 : (rx > ow - 1 ? ow - 1 : rx);
      const int c0 = (int)(((long long)rx * W) / ow), c1 = (int)(((long long)(rx + 1) * W + ow - 1) / ow);
      unsigned s[3] = {0u, 0u, 0u};                        // (a window holds fewer than 2^24 pixels: the sums fit)
      for (int sy = r0; sy < r1; ++sy) {
        const unsigned char* row = base + sy * s_row;
        for (int sx = c0; sx < c1; ++sx) {
#pragma unroll
          for (int c = 0; c < 3; ++c) s[c] += PLANAR ? row[c * s_plane + sx] : row[3 * (long long)sx + c];
        }
      }
      const float cnt = (float)((r1 - r0) * (c1 - c0));
#pragma unroll
      for (int c = 0; c < 3; ++c) r[c][k] = __fdiv_rn((float)s[c], cnt);
    }
  }
  float* o = out + n * o_bs + (long long)y * Wp + x0;
  const long long plane = (long long)Hp * Wp;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int cs = bgr ? 2 - c : c;
    float q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = frame_value_f<NORM>(cs == 0 ? r[0][k] : (cs == 1 ? r[1][k] : r[2][k]));
    float* d = o + c * plane;
    if (x0 + 3 < Wp) {
      *reinterpret_cast<f32x4u*>(d) = f32x4{q[0], q[1], q[2], q[3]};
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (x0 + k < Wp) d[k] = q[k];
    }
  }
}

// One component of the resized flow at output pixel (ty, tx) of the crop window whose first sample is `p`: what all three
// codings of flow_resize_kernel store.  The taps are clamped inside the window (make_tap), the vector is scaled to the new
// size with one multiplication.
__device__ __forceinline__ float flow_resized(const float* __restrict__ p, int Wp, const resize_tap& ty, const resize_tap& tx, float s) {
  const float* ra = p + (long long)ty.a * Wp;
  const float* rb = p + (long long)ty.b * Wp;
  return bilerp(tx.f, ty.f, ra[tx.a], ra[tx.b], rb[tx.a], rb[tx.b]) * s;
}

// Thread = 4 consecutive pixels of one output row; CODING as in flow_store.
template <int CODING>
__global__ __launch_bounds__(256) void flow_resize_kernel(const float* __restrict__ flow, long long f_bs, int Hp, int Wp, int y0, int x0,
                                                          int Hc, int Wc, int H, int W, float su, float sv,
                                                          unsigned char* __restrict__ out, long long o_bs, float scale, int swap,
                                                          int gpr) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= H * gpr) return;
  const int y = i / gpr, x = (i - y * gpr) * 4;
  const int n = blockIdx.y;
  const float* pu = flow + n * f_bs + (long long)y0 * Wp + x0;
  const float* pv = pu + (long long)Hp * Wp;
  const int cnt = W - x < 4 ? W - x : 4;
  const resize_tap ty = make_tap(y, Hc, H);
  float u[4], v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const resize_tap tx = make_tap(k < cnt ? x + k : x, Wc, W);
    u[k] = flow_resized(pu, Wp, ty, tx, su);
    v[k] = flow_resized(pv, Wp, ty, tx, sv);
  }
  flow_store<CODING>(out + n * o_bs, (long long)y * W + x, (long long)H * W, cnt, u, v, scale, swap);
}

inline bool io_dims_ok(int N, int H, int W) {
  // (a sample's elements, 3 per pixel, and the thread index are ints; blockIdx.y carries the sample)
  return N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W <= (0x7fffffffLL - 1024) / 3;
}

}  // namespace

extern "C" int accflow_frames_from_u8(const unsigned char* src, long long s_bs, long long s_row, long long s_plane, int planar,
                                      int bgr, int normalize, float* out, long long o_bs, int N, int H, int W, int pad_l,
                                      int pad_r, int pad_t, int pad_b, void* stream) {
  if (!src || !out || !io_dims_ok(N, H, W)) return 1;
  if (pad_l < 0 || pad_r < 0 || pad_t < 0 || pad_b < 0) return 1;
  const long long Hp = (long long)H + pad_t + pad_b, Wp = (long long)W + pad_l + pad_r;
  if (Hp > 0x7fffffffLL || Wp > 0x7fffffffLL || !io_dims_ok(N, (int)Hp, (int)Wp)) return 1;
  if (s_row < 0 || s_bs < 0 || (planar && s_plane < 0) || ((uintptr_t)out & 3)) return 1;
  const int gpr = cdiv(Wp, 4);
  const dim3 grid(cdiv(Hp * gpr, 256), N), block(256);
#define FIO_LAUNCH(P, G)                                                                                                      \
  hipLaunchKernelGGL((frames_from_u8_kernel<P, G>), grid, block, 0, as_stream(stream), src, s_bs, s_row, s_plane, bgr ? 1 : 0, \
                     out, o_bs, H, W, pad_l, pad_t, (int)Hp, (int)Wp, gpr)
  if (planar) {
    if (normalize) FIO_LAUNCH(true, true); else FIO_LAUNCH(true, false);
  } else {
    if (normalize) FIO_LAUNCH(false, true); else FIO_LAUNCH(false, false);
  }
#undef FIO_LAUNCH
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_frames_from_u8_resized(const unsigned char* src, long long s_bs, long long s_row, long long s_plane,
                                              int planar, int bgr, int normalize, float* out, long long o_bs, int N, int H, int W,
                                              int pad_l, int pad_r, int pad_t, int pad_b, int out_h, int out_w, int interp,
                                              void* stream) {
  if (!src || !out || !io_dims_ok(N, H, W) || out_h <= 0 || out_w <= 0 || (interp != 0 && interp != 1)) return 1;
  if (H > RESIZE_MAX_SIDE || W > RESIZE_MAX_SIDE || out_h > RESIZE_MAX_SIDE || out_w > RESIZE_MAX_SIDE) return 1;
  if (pad_l < 0 || pad_r < 0 || pad_t < 0 || pad_b < 0) return 1;
  const long long Hp = (long long)out_h + pad_t + pad_b, Wp = (long long)out_w + pad_l + pad_r;
  if (Hp > 0x7fffffffLL || Wp > 0x7fffffffLL || !io_dims_ok(N, (int)Hp, (int)Wp)) return 1;
  if (s_row < 0 || s_bs < 0 || (planar && s_plane < 0) || ((uintptr_t)out & 3)) return 1;
  // (an area window spans at most ceil(H / out_h) + 1 rows and as many columns in its direction)
  if (interp == 1 && (long long)(cdiv(H, out_h) + 1) * (cdiv(W, out_w) + 1) >= (1LL << 24)) return 1;
  const int gpr = cdiv(Wp, 4);
  const dim3 grid(cdiv(Hp * gpr, 256), N), block(256);
#define FIO_LAUNCH(P, G, A)                                                                                                 \
  hipLaunchKernelGGL((frames_from_u8_resized_kernel<P, G, A>), grid, block, 0, as_stream(stream), src, s_bs, s_row, s_plane, \
                     bgr ? 1 : 0, out, o_bs, H, W, out_h, out_w, pad_l, pad_t, (int)Hp, (int)Wp, gpr)
#define FIO_LAUNCH_PG(A)                                                           \
  if (planar) {                                                                    \
    if (normalize) FIO_LAUNCH(true, true, A); else FIO_LAUNCH(true, false, A);     \
  } else {                                                                         \
    if (normalize) FIO_LAUNCH(false, true, A); else FIO_LAUNCH(false, false, A);   \
  }
  if (interp) { FIO_LAUNCH_PG(true) } else { FIO_LAUNCH_PG(false) }
#undef FIO_LAUNCH_PG
#undef FIO_LAUNCH
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_flow_resize(const float* flow, long long f_bs, int Hp, int Wp, int y0, int x0, int Hc, int Wc, int H, int W,
                                   void* out, long long o_bs, int coding, float scale, int big_endian, int N, void* stream) {
  if (!flow || !out || !io_dims_ok(N, Hp, Wp) || !io_dims_ok(N, H, W) || coding < 0 || coding > 2) return 1;
  if (y0 < 0 || x0 < 0 || Hc <= 0 || Wc <= 0 || (long long)y0 + Hc > Hp || (long long)x0 + Wc > Wp) return 1;
  if (Hc > RESIZE_MAX_SIDE || Wc > RESIZE_MAX_SIDE || H > RESIZE_MAX_SIDE || W > RESIZE_MAX_SIDE) return 1;
  const int amask = coding == 1 ? 1 : 3;
  if (((uintptr_t)out & amask) || (N > 1 && (o_bs & amask)) || o_bs < 0) return 1;
  const float su = (float)W / (float)Wc, sv = (float)H / (float)Hc;    // (sides <= 2^15: exact operands, one rounding each)
  const int gpr = cdiv(W, 4);
  const dim3 grid(cdiv((long long)H * gpr, 256), N), block(256);
  unsigned char* o = static_cast<unsigned char*>(out);
#define FIO_LAUNCH(C, S, E)                                                                                                      \
  hipLaunchKernelGGL(flow_resize_kernel<C>, grid, block, 0, as_stream(stream), flow, f_bs, Hp, Wp, y0, x0, Hc, Wc, H, W, su, sv, \
                     o, o_bs, S, E, gpr)
  if (coding == 1) FIO_LAUNCH(1, scale, big_endian ? 1 : 0);
  else if (coding == 2) FIO_LAUNCH(2, 0.0f, 0);
  else FIO_LAUNCH(0, 0.0f, 0);
#undef FIO_LAUNCH
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_flow_export(const float* flow, long long f_bs, int Hp, int Wp, int y0, int x0, int H, int W, void* out,
                                   long long o_bs, int coding, float scale, int big_endian, int N, void* stream) {
  if (!flow || !out || !io_dims_ok(N, Hp, Wp) || (coding != 0 && coding != 1)) return 1;
  if (y0 < 0 || x0 < 0 || H <= 0 || W <= 0 || (long long)y0 + H > Hp || (long long)x0 + W > Wp) return 1;
  if (((uintptr_t)out & (coding ? 1 : 3)) || (N > 1 && (o_bs & (coding ? 1 : 3))) || o_bs < 0) return 1;
  const int gpr = cdiv(W, 4);
  const dim3 grid(cdiv((long long)H * gpr, 256), N), block(256);
  unsigned char* o = static_cast<unsigned char*>(out);
  if (coding)
    hipLaunchKernelGGL(flow_export_kernel<true>, grid, block, 0, as_stream(stream), flow, f_bs, Hp, Wp, y0, x0, H, W, o, o_bs, scale,
                       big_endian ? 1 : 0, gpr);
  else
    hipLaunchKernelGGL(flow_export_kernel<false>, grid, block, 0, as_stream(stream), flow, f_bs, Hp, Wp, y0, x0, H, W, o, o_bs, scale,
                       0, gpr);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
