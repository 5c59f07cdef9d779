// forward_interpolate (raft/utils/utils.py:31-63): RAFT's warm start for video.  Every cell s = (ys, xs) of a 1/8-resolution
// flow is pushed to (x1, y1) = (xs + dx[s], ys + dy[s]); sources that stay strictly inside (0, W8) x (0, H8) are kept, and
// every grid cell (x0, y0) takes BOTH flow components of the kept source nearest to it (scipy's griddata(method="nearest")
// twice over the same points).  Brute force: P = H8 W8 is 7 680 at 480x1024, P^2 = 59 M distance tests per item.
//
// Arithmetic: positions and squared distances in double, as the reference's (int64 grid + float32 flow -> float64); the
// squared distance is (x1 - x0)^2 + (y1 - y0)^2 as two roundings of two products and one of their sum - NOT contracted into an
// FMA (fp contract off for this unit), so that a float64 restatement on the host reproduces every comparison bit for bit.
// Exact ties go to the lowest row-major source index: every thread scans its sources in ascending order with a strict
// `<`, and partial results are merged as the lexicographic minimum of (d^2, index) - the result does not depend on how the
// sources are dealt to threads.  An item without a valid source (the reference raises inside scipy) gives zeros.
//
// Launch shape: one 256-thread workgroup owns FI_TT = 32 targets and all sources; thread t serves target t % 32 and the
// sources s = t / 32 (mod 8) - eight interleaved shares, merged through LDS at the end.  P / 32 workgroups of four waves =
// 240 on 256 CUs at B = 1, P = 7 680 (one target per thread and no split: 30).  The sources pass through LDS in chunks of
// FI_CHUNK as (x1, y1) doubles, invalid ones as +inf, whose distance is +inf and never below the
// running best; all 32 lanes of a half-wave read the SAME 16 bytes per step (a broadcast, conflict-free), the two halves
// adjacent ones.  No atomics, no workspace, loops bounded by P.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int FI_THREADS = 256;
constexpr int FI_TT = 32;                       // targets per workgroup
constexpr int FI_SPLIT = FI_THREADS / FI_TT;    // interleaved source shares per target
constexpr int FI_CHUNK = 1024;                  // sources per LDS chunk (16 KiB)

struct __attribute__((aligned(16))) fi_pos { double x, y; };

__global__ __launch_bounds__(FI_THREADS) void forward_interpolate_kernel(const float* __restrict__ flow, float* __restrict__ out,
                                                                         int H8, int W8, int tiles) {
  __shared__ fi_pos src[FI_CHUNK];
  __shared__ double best_d[FI_SPLIT][FI_TT];
  __shared__ int best_i[FI_SPLIT][FI_TT];
  const int P = H8 * W8;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const float* __restrict__ fx = flow + (long long)b * 2 * P;
  const float* __restrict__ fy = fx + P;
  const int tid = threadIdx.x, tl = tid % FI_TT, share = tid / FI_TT;
  const int t = tile * FI_TT + tl;
  const int tc = t < P ? t : P - 1;             // (threads past the end scan like the last target and write nothing)
  const int ty = tc / W8;
  const double x0 = (double)(tc - ty * W8), y0 = (double)ty;
  const double inf = __builtin_inf();
  double bd = inf;
  int bi = -1;
  for (int c0 = 0; c0 < P; c0 += FI_CHUNK) {
    const int n = min(FI_CHUNK, P - c0);
    for (int i = tid; i < n; i += FI_THREADS) {
      const int s = c0 + i, ys = s / W8;
      const double x1 = (double)(s - ys * W8) + (double)fx[s];
      const double y1 = (double)ys + (double)fy[s];
      const bool valid = x1 > 0.0 && x1 < (double)W8 && y1 > 0.0 && y1 < (double)H8;   // (NaN, +-inf: false)
      src[i] = valid ? fi_pos{x1, y1} : fi_pos{inf, inf};
    }
    __syncthreads();
#pragma unroll 4
    for (int j = share; j < n; j += FI_SPLIT) {
      const fi_pos p = src[j];
      const double ex = p.x - x0, ey = p.y - y0;
      const double d = ex * ex + ey * ey;
      if (d < bd) {
        bd = d;
        bi = c0 + j;
      }
    }
    __syncthreads();
  }
  best_d[share][tl] = bd;
  best_i[share][tl] = bi;
  __syncthreads();
  if (share != 0 || t >= P) return;
#pragma unroll
  for (int k = 1; k < FI_SPLIT; ++k) {
    const double d = best_d[k][tl];
    const int i = best_i[k][tl];
    if (i >= 0 && (bi < 0 || d < bd || (d == bd && i < bi))) {
      bd = d;
      bi = i;
    }
  }
  float* __restrict__ o = out + (long long)b * 2 * P;
  o[t] = bi >= 0 ? fx[bi] : 0.0f;
  o[P + t] = bi >= 0 ? fy[bi] : 0.0f;
}

}  // namespace

extern "C" int accflow_forward_interpolate_f32(const float* flow, float* out, int B, int H8, int W8, void* stream) {
  if (!flow || !out || flow == out || B <= 0 || H8 <= 0 || W8 <= 0) return 1;
  const long long P = (long long)H8 * W8;
  if (P > (1 << 24)) return 1;                  // (brute force: far beyond any 1/8-resolution frame; keeps every index in int)
  const long long tiles = (P + FI_TT - 1) / FI_TT;
  if (tiles * B * FI_THREADS >= (1LL << 32)) return 1;   // (HIP launches fewer than 2^32 threads)
  hipLaunchKernelGGL(forward_interpolate_kernel, dim3((unsigned)(tiles * B)), dim3(FI_THREADS), 0, as_stream(stream), flow, out,
                     H8, W8, (int)tiles);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
