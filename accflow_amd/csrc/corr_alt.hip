// alternate_corr: the CorrBlock lookup computed on the fly from the feature maps, without the all-pairs volume.
//
// Level l of the reference pyramid is V_l = avg_pool2d^l over the target axes of (f1 . f2) / sqrt(C).  Pooling is
// linear and floors odd sizes the same way for a plane and for a feature map, so V_l[p][y'][x'] = f1[p] . pool_l(f2)[y'][x']
// / sqrt(C): the lookup only needs f1 and the pooled target pyramid of f2, O(P) memory where the volume needs O(P^2).
//
// Pyramid (accflow_corr_alt_pyramid_f32): per FRAME, once - level l of all F frames is an (F, Hl, Wl, C) channel-last block
// (pooled ((a+b)+c)+d then * 0.25 from level l-1, as F.avg_pool2d(2, 2)); level 0 is also the query operand.  The blocks
// follow each other, level 0 first (accflow_corr_alt_pyramid_elems floats per frame in all).
//
// Lookup (accflow_corr_lookup_alt_f32 / _s16): one 256-thread workgroup = a 4 x 16 tile of query pixels of one item at one
// level.  All 64 pixels take their integer 10x10 window origins (the coordinate arithmetic of corr_lookup.hip); the union of
// the windows that touch the plane is a box of target cells.  For coherent flow that box is ~13x25 cells at level 0 and
// smaller below, so each target feature is read once per tile and shared by the windows of the 64 pixels: the box is
// staged through LDS 16 channels at a time (cell stride 20 floats: the ds_read_b128 of neighbouring cells hit different
// banks), the query chunk next to it.  Wave w forms window cells 25w .. 25w+24 of every pixel (lane = pixel) as fp32 FMA
// dot products - exact fp32, no operand split, so no range guard is involved; a box larger than ALT_MAXBOX cells (noise-like
// flow) makes the tile read its targets straight from global memory instead, summing in the same order (same bits).
// The 100 window sums go through LDS to the blend, which is corr_disp.hip's fma chain: fp32 out in the reference channel order
// l*81 + i*9 + j, or the pre-split S16 form of accflow_corr_lookup_disp_s16 (88 channels per level, compute order + 7 zeros).
#include "common.h"

namespace {

constexpr int R = 4, WIN = 2 * R + 2;
constexpr int TH = 4, TW = 16;            // query tile (64 pixels)
constexpr int CK = 16, CS = 20;           // channels per LDS chunk, floats per staged cell
constexpr int ALT_MAXBOX = 512;           // box cells staged per chunk (+1 zero cell)
constexpr int NCELL = 25;                 // window cells per thread (100 over the 4 waves)
constexpr int WSTRIDE = WIN * WIN + 1;    // LDS window row of one pixel (odd: conflict-free ds_read_b32)
constexpr int LDS_T = (ALT_MAXBOX + 1) * CS;
constexpr int LDS_W = 64 * WSTRIDE;
constexpr int LDS_MAIN = LDS_T > LDS_W ? LDS_T : LDS_W;

__host__ __device__ inline long long level_offset(int F, int C, int H8, int W8, int l) {
  long long off = 0;
  for (int k = 0; k < l; ++k) off += (long long)F * (H8 >> k) * (W8 >> k) * C;
  return off;
}

// (F, C, H8, W8) -> (F, H8, W8, C): 64 channels x 64 pixels per workgroup through LDS
__global__ __launch_bounds__(256) void alt_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int P) {
  __shared__ float t[64][65];
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, f = blockIdx.z;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const float* src = in + (long long)f * C * P;
  for (int c = ty; c < 64; c += 4)
    t[c][tx] = (p0 + tx < P && c0 + c < C) ? src[(long long)(c0 + c) * P + p0 + tx] : 0.0f;
  __syncthreads();
  float* dst = out + (long long)f * P * C;
  for (int p = ty; p < 64; p += 4)
    if (p0 + p < P && c0 + tx < C) dst[(long long)(p0 + p) * C + c0 + tx] = t[tx][p];
}

// level l+1 from level l, channel-last: thread = (output cell, 4 channels)
__global__ __launch_bounds__(256) void alt_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int F, int C,
                                                      int Hi, int Wi) {
  const int Ho = Hi >> 1, Wo = Wi >> 1, C4 = C >> 2;
  const long long n = (long long)F * Ho * Wo * C4;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int c4 = (int)(t % C4);
  const long long cell = t / C4;
  const int xo = (int)(cell % Wo);
  const long long r = cell / Wo;
  const int yo = (int)(r % Ho);
  const int f = (int)(r / Ho);
  const float* s = in + (((long long)f * Hi + 2 * yo) * Wi + 2 * xo) * C + 4 * c4;
  const float4 a = *reinterpret_cast<const float4*>(s), b = *reinterpret_cast<const float4*>(s + C);
  const float4 c = *reinterpret_cast<const float4*>(s + (long long)Wi * C), d = *reinterpret_cast<const float4*>(s + (long long)Wi * C + C);
  float4 o;
  o.x = (((a.x + b.x) + c.x) + d.x) * 0.25f;
  o.y = (((a.y + b.y) + c.y) + d.y) * 0.25f;
  o.z = (((a.z + b.z) + c.z) + d.z) * 0.25f;
  o.w = (((a.w + b.w) + c.w) + d.w) * 0.25f;
  *reinterpret_cast<float4*>(out + cell * C + 4 * c4) = o;
}

__device__ __forceinline__ float dot4(float acc, const float4 q, const float4 t) {
  acc = __builtin_fmaf(q.x, t.x, acc);
  acc = __builtin_fmaf(q.y, t.y, acc);
  acc = __builtin_fmaf(q.z, t.z, acc);
  return __builtin_fmaf(q.w, t.w, acc);
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = min(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = max(v, __shfl_xor(v, m));
  return v;
}

typedef unsigned lu32x4 __attribute__((ext_vector_type(4)));

template <bool OUT16>
__global__ __launch_bounds__(256) void corr_lookup_alt_kernel(const float* __restrict__ pyr, int F, const int* __restrict__ idx,
                                                             const float* __restrict__ coords, float* __restrict__ out,
                                                             long long out_bs, int B, int C, int H8, int W8, int* guard) {
  __shared__ __attribute__((aligned(16))) float lds_main[LDS_MAIN];   // staged box cells / afterwards the 64 windows
  __shared__ __attribute__((aligned(16))) float lds_q[64 * CS];        // query chunk
  const int P = H8 * W8;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lvl = blockIdx.z, b = blockIdx.y;
  const int ntx = (W8 + TW - 1) / TW;
  const int y = (blockIdx.x / ntx) * TH + (lane >> 4), x = (blockIdx.x % ntx) * TW + (lane & 15);
  const bool active = y < H8 && x < W8;
  const int pix = active ? y * W8 + x : 0;
  const int f1 = idx[b], f2 = idx[B + b];
  if ((unsigned)f1 >= (unsigned)F || (unsigned)f2 >= (unsigned)F) return;   // (host-checked; never index outside the pyramid)

  const int Hl = H8 >> lvl, Wl = W8 >> lvl;
  const float* __restrict__ qsrc = pyr + ((long long)f1 * P + pix) * C;
  const float* __restrict__ tgt = pyr + level_offset(F, C, H8, W8, lvl) + (long long)f2 * Hl * Wl * C;

  const float inv = 1.0f / (float)(1 << lvl);
  float cx = coords[((long long)b * 2 + 0) * P + pix] * inv;
  float cy = coords[((long long)b * 2 + 1) * P + pix] * inv;
  cx = fminf(fmaxf(cx, -1.0e6f), 1.0e6f);
  cy = fminf(fmaxf(cy, -1.0e6f), 1.0e6f);
  const float fx0 = floorf(cx), fy0 = floorf(cy);
  const float ax = cx - fx0, ay = cy - fy0;
  const int xs = (int)fx0 - R, ys = (int)fy0 - R;

  // box of target cells that some window of the tile covers inside the plane
  const int lx = max(xs, 0), hx = min(xs + WIN - 1, Wl - 1), ly = max(ys, 0), hy = min(ys + WIN - 1, Hl - 1);
  const bool needy = active && lx <= hx && ly <= hy;
  const int bx0 = wave_min(needy ? lx : 0x7fffffff), by0 = wave_min(needy ? ly : 0x7fffffff);
  const int bx1 = wave_max(needy ? hx : -1), by1 = wave_max(needy ? hy : -1);
  const bool any = bx0 <= bx1;
  const int bw = any ? bx1 - bx0 + 1 : 0, bh = any ? by1 - by0 + 1 : 0;
  const int nb = bw * bh;
  const bool staged = nb <= ALT_MAXBOX;

  float acc[NCELL];
#pragma unroll
  for (int k = 0; k < NCELL; ++k) acc[k] = 0.0f;

  if (staged && nb > 0) {
    int off[NCELL];
#pragma unroll
    for (int k = 0; k < NCELL; ++k) {
      const int cidx = wv * NCELL + k, r = cidx / WIN, s = cidx - r * WIN;
      const int yy = ys + r, xx = xs + s;
      const bool in = active && (unsigned)yy < (unsigned)Hl && (unsigned)xx < (unsigned)Wl;
      off[k] = (in ? (yy - by0) * bw + (xx - bx0) : nb) * CS;
    }
    if (tid < CK / 4) *reinterpret_cast<float4*>(lds_main + nb * CS + 4 * tid) = make_float4(0.f, 0.f, 0.f, 0.f);
    const int npass = (nb + 63) >> 6;   // 64 cells x 4 float4 per pass of 256 threads
    const int sub = tid & 3;
    for (int c0 = 0; c0 < C; c0 += CK) {
      __syncthreads();   // (previous chunk consumed)
      for (int ps = 0; ps < npass; ++ps) {
        const int cell = ps * 64 + (tid >> 2);
        if (cell < nb) {
          const int cy_ = cell / bw, cx_ = cell - cy_ * bw;
          const float4 v = *reinterpret_cast<const float4*>(tgt + ((long long)(by0 + cy_) * Wl + (bx0 + cx_)) * C + c0 + 4 * sub);
          *reinterpret_cast<float4*>(lds_main + cell * CS + 4 * sub) = v;
        }
      }
      {
        const int p = tid >> 2;   // the query chunk: 64 pixels x 4 float4
        const int qy = (blockIdx.x / ntx) * TH + (p >> 4), qx = (blockIdx.x % ntx) * TW + (p & 15);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (qy < H8 && qx < W8) v = *reinterpret_cast<const float4*>(pyr + ((long long)f1 * P + qy * W8 + qx) * C + c0 + 4 * sub);
        *reinterpret_cast<float4*>(lds_q + p * CS + 4 * sub) = v;
      }
      __syncthreads();
#pragma unroll 1
      for (int c4 = 0; c4 < CK / 4; ++c4) {
        const float4 q = *reinterpret_cast<const float4*>(lds_q + lane * CS + 4 * c4);
#pragma unroll
        for (int k = 0; k < NCELL; ++k)
          acc[k] = dot4(acc[k], q, *reinterpret_cast<const float4*>(lds_main + off[k] + 4 * c4));
      }
    }
  } else if (nb > 0) {
    // box beyond the LDS budget: this tile's windows read their targets from global memory (same summation order)
#pragma unroll
    for (int k = 0; k < NCELL; ++k) {
      const int cidx = wv * NCELL + k, r = cidx / WIN, s = cidx - r * WIN;
      const int yy = ys + r, xx = xs + s;
      if (active && (unsigned)yy < (unsigned)Hl && (unsigned)xx < (unsigned)Wl) {
        const float* tp = tgt + ((long long)yy * Wl + xx) * C;
        float a = 0.0f;
        for (int c = 0; c < C; c += 4)
          a = dot4(a, *reinterpret_cast<const float4*>(qsrc + c), *reinterpret_cast<const float4*>(tp + c));
        acc[k] = a;
      }
    }
  }

  // windows -> LDS (scaled by 1/sqrt(C)), then the blend of corr_disp.hip
  const float scale = 1.0f / sqrtf((float)C);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NCELL; ++k) lds_main[lane * WSTRIDE + wv * NCELL + k] = acc[k] * scale;
  __syncthreads();
  if (!active) return;
  const float* wn = lds_main + lane * WSTRIDE;
  const float w00 = (1.0f - ax) * (1.0f - ay), w01 = ax * (1.0f - ay), w10 = (1.0f - ax) * ay, w11 = ax * ay;
  auto tap = [&](int i, int j) {
    const float* r0 = wn + j * WIN + i;
    const float* r1 = r0 + WIN;
    return __builtin_fmaf(r1[1], w11, __builtin_fmaf(r1[0], w10, __builtin_fmaf(r0[1], w01, r0[0] * w00)));
  };
  if constexpr (!OUT16) {
    float* o = out + (long long)b * out_bs + (long long)(lvl * 81) * P + pix;
    for (int j = wv; j < 2 * R + 1; j += 4)
#pragma unroll
      for (int i = 0; i < 2 * R + 1; ++i) o[(long long)(i * 9 + j) * P] = tap(i, j);
  } else {
    lu32x4* o16 = reinterpret_cast<lu32x4*>(out + (long long)b * out_bs) + pix;
    bool bad = false;
    for (int oct = wv; oct < 11; oct += 4) {
      float buf[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int n = oct * 8 + t;
        buf[t] = n < 81 ? tap(n % 9, n / 9) : 0.0f;
      }
      lu32x4 hi, lo;
      s16_split8(buf, hi, lo, bad);
      o16[(long long)((lvl * 11 + oct) * 2 + 0) * P] = hi;
      o16[(long long)((lvl * 11 + oct) * 2 + 1) * P] = lo;
    }
    if (bad && guard) atomicOr(guard, 1);
  }
}

bool alt_shape_ok(int F, int C, int H8, int W8) {
  return F > 0 && C >= CK && C % CK == 0 && H8 >= 8 && W8 >= 8 && (long long)H8 * W8 < (1LL << 30);
}

}  // namespace

extern "C" long long accflow_corr_alt_pyramid_elems(int C, int H8, int W8) {
  if (C <= 0 || H8 <= 0 || W8 <= 0) return 0;
  return level_offset(1, C, H8, W8, 4);
}

extern "C" int accflow_corr_alt_pyramid_f32(const float* fmaps, float* pyr, int F, int C, int H8, int W8, void* stream) {
  if (!fmaps || !pyr || !alt_shape_ok(F, C, H8, W8)) return 1;
  hipStream_t st = as_stream(stream);
  const int P = H8 * W8;
  hipLaunchKernelGGL(alt_transpose_kernel, dim3(cdiv(P, 64), cdiv(C, 64), F), dim3(256), 0, st, fmaps, pyr, C, P);
  for (int l = 0; l < 3; ++l) {
    const int Hi = H8 >> l, Wi = W8 >> l;
    const long long n = (long long)F * (Hi >> 1) * (Wi >> 1) * (C / 4);
    hipLaunchKernelGGL(alt_pool_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, pyr + level_offset(F, C, H8, W8, l),
                       pyr + level_offset(F, C, H8, W8, l + 1), F, C, Hi, Wi);
  }
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_corr_lookup_alt_f32(const float* pyr, int F, const int* idx, const float* coords, float* out,
                                           long long out_bs, int B, int C, int H8, int W8, void* stream) {
  if (!pyr || !idx || !coords || !out || B <= 0 || B > 65535 || !alt_shape_ok(F, C, H8, W8)) return 1;
  const int tiles = cdiv(H8, TH) * cdiv(W8, TW);
  hipLaunchKernelGGL(corr_lookup_alt_kernel<false>, dim3(tiles, B, 4), dim3(256), 0, as_stream(stream), pyr, F, idx, coords,
                     out, out_bs, B, C, H8, W8, nullptr);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_corr_lookup_alt_s16(const float* pyr, int F, const int* idx, const float* coords, void* out16,
                                           long long out16_bs, int* guard, int B, int C, int H8, int W8, void* stream) {
  if (!pyr || !idx || !coords || !out16 || B <= 0 || B > 65535 || !alt_shape_ok(F, C, H8, W8)) return 1;
  const int tiles = cdiv(H8, TH) * cdiv(W8, TW);
  hipLaunchKernelGGL(corr_lookup_alt_kernel<true>, dim3(tiles, B, 4), dim3(256), 0, as_stream(stream), pyr, F, idx, coords,
                     reinterpret_cast<float*>(out16), out16_bs, B, C, H8, W8, guard);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
