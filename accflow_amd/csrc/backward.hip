// Backward kernels of the fusion heads (the slice of the training path that carries gradients: train_acc.py
// freezes the estimator - `ofe` - and AccFlow_.py:172,182,195,198 detach flows / occlusion / error maps, so the loss reaches
// only the convolution stacks of FlowEncoder / AccPlus / Blending / FlowDecoder, the modulated deformable convolution, the
// blend and the convex upsampling).  fp32 arithmetic throughout (gradients are compared with the reference's autograd at 1e-4
// relative); the input-gradient of a stride-1 convolution is the forward convolution kernel run with the transposed, flipped
// weights and needs no kernel of its own.
#include "conv_common.h"
#include <stdlib.h>

namespace {

// dx = dy * act'(y) from the activation's OUTPUT y: relu -> [y > 0], sigmoid -> y (1 - y), tanh -> 1 - y^2.  Operands are
// (B, CHW) planes with their own batch strides (channel slices of wider tensors).
__global__ __launch_bounds__(256) void act_backward_kernel(const float* __restrict__ dy, long long dy_bs, const float* __restrict__ y,
                                                           long long y_bs, float* __restrict__ dx, long long dx_bs, int B,
                                                           long long CHW, int act) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= CHW) return;
  for (int b = 0; b < B; ++b) {
    const float v = y[b * y_bs + i], g = dy[b * dy_bs + i];
    float r = g;
    if (act == ACCFLOW_ACT_RELU) r = v > 0.0f ? g : 0.0f;
    else if (act == ACCFLOW_ACT_SIGMOID) r = g * v * (1.0f - v);
    else if (act == ACCFLOW_ACT_TANH) r = g * (1.0f - v * v);
    dx[b * dx_bs + i] = r;
  }
}

// dst += src over (B, CHW) planes with batch strides (gradient accumulation where a tensor feeds several consumers)
__global__ __launch_bounds__(256) void add_kernel(float* __restrict__ dst, long long dst_bs, const float* __restrict__ src,
                                                  long long src_bs, int B, long long CHW) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= CHW) return;
  for (int b = 0; b < B; ++b) dst[b * dst_bs + i] += src[b * src_bs + i];
}

// d/dpred of scale * sum |pred - gt| (loss.py:34-36, the mean folded into `scale`): scale * sign(pred - gt), 0 at equality
// (torch's abs backward)
__global__ __launch_bounds__(256) void l1_grad_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                      float* __restrict__ dpred, long long n, float scale) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float d = pred[i] - gt[i];
  dpred[i] = d > 0.0f ? scale : (d < 0.0f ? -scale : 0.0f);
}

// Zero insertion: dst (B, C, Hd, Wd; zeroed by the launcher) [y * s, x * s] = src (B, C, OH, OW) [y, x] - the gradient of a
// stride-s convolution's output laid out so that its input gradient is a stride-1 convolution with the flipped weights.
__global__ __launch_bounds__(256) void dilate_kernel(const float* __restrict__ src, long long src_bs, float* __restrict__ dst, int B,
                                                     int C, int OH, int OW, int Hd, int Wd, int s) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * C * OH * OW) return;
  const int x = (int)(i % OW), y = (int)((i / OW) % OH), c = (int)((i / ((long long)OW * OH)) % C);
  const int b = (int)(i / ((long long)OW * OH * C));
  dst[(((long long)b * C + c) * Hd + (long long)y * s) * Wd + (long long)x * s] = src[b * src_bs + ((long long)c * OH + y) * OW + x];
}

// Blending (AccFlow_.py:122-124) out = f1 m + (1 - m) f2:  df1 = dy m, df2 = dy (1 - m), dm = sum_c dy (f1 - f2)
__global__ __launch_bounds__(256) void blend_backward_kernel(const float* __restrict__ dy, const float* __restrict__ f1,
                                                             const float* __restrict__ f2, const float* __restrict__ m,
                                                             float* __restrict__ df1, float* __restrict__ df2,
                                                             float* __restrict__ dm, int B, int C, int HW) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * HW) return;
  const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
  const float mm = m[i];
  float acc = 0.0f;
  for (int c = 0; c < C; ++c) {
    const long long e = ((long long)b * C + c) * HW + p;
    const float g = dy[e];
    df1[e] = g * mm;
    df2[e] = g * (1.0f - mm);
    acc += g * (f1[e] - f2[e]);
  }
  dm[i] = acc;
}

// Convex upsampling (raft.py:81-92) backward.  Thread = (n, coarse pixel, sub-pixel a*8+b): softmax s_k of the 9 mask logits,
// t_k = sum_c g_c * 8 flow_zp[c, h+k/3-1, w+k%3-1];  dmask_k = s_k (t_k - sum_j s_j t_j);  dflow[c, neighbour k] += 8 s_k g_c
// (float atomics: 64 sub-pixels x up to 9 coarse pixels add into one element).
__global__ __launch_bounds__(256) void convex_upsample_backward_kernel(const float* __restrict__ dup, const float* __restrict__ flow,
                                                                       const float* __restrict__ mask, float* __restrict__ dflow,
                                                                       float* __restrict__ dmask, int B, int H8, int W8) {
  const int P = H8 * W8;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * 64 * P) return;
  const int pix = (int)(i % P), ab = (int)((i / P) % 64), n = (int)(i / ((long long)P * 64));
  const int h = pix / W8, w = pix - h * W8, a = ab >> 3, b = ab & 7;
  const int W = 8 * W8;
  float g[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) g[c] = dup[((long long)(n * 2 + c) * (8 * H8) + 8 * h + a) * W + 8 * w + b];
  // softmax, t and d mask in double: near one-hot weights make d mask heavy-tailed (largest element 37 x its RMS with logits of
  // +-100) and s_k (t_k - sum_j s_j t_j) a difference of nearly equal numbers - fp32 left it 1.3e-5 of the RMS from float64; the
  // kernel moves 2 x 576 values per coarse pixel through memory, the 9 exponentials do not show
  double m[9], mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    m[k] = (double)mask[((long long)n * 576 + k * 64 + ab) * P + pix];
    mx = fmax(mx, m[k]);
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) { m[k] = exp(m[k] - mx); s += m[k]; }
  double t[9], dot = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    m[k] /= s;
    const int yy = h + k / 3 - 1, xx = w + k % 3 - 1;
    const bool ok = (unsigned)yy < (unsigned)H8 && (unsigned)xx < (unsigned)W8;
    t[k] = 0.0;
    if (ok) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        t[k] += (double)g[c] * 8.0 * (double)flow[((long long)n * 2 + c) * P + yy * W8 + xx];
        atomicAdd(&dflow[((long long)n * 2 + c) * P + yy * W8 + xx], (float)(8.0 * m[k] * (double)g[c]));
      }
    }
    dot += m[k] * t[k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) dmask[((long long)n * 576 + k * 64 + ab) * P + pix] = (float)(m[k] * (t[k] - dot));
}

// Weight gradient of a convolution: dw[co][ci][ky][kx] = sum_{b,y,x} dy[b,co,y,x] * x[b,ci,y*stride+ky-padH,x*stride+kx-padW]
// (zero padding), db[co] = sum dy - the GEMM  D[co][j] = sum_p dY[co][p] * Xcol[j][p],  j = (ci, tap), p = (b, y, x), on the
// matrix cores with split-bf16 operands (NT = 3 terms, 6 products: fp32-equivalent - gradients span the whole fp32 exponent
// range, which rules the scaled fp16 split out).  A workgroup owns a 128 (co) x 128 (j) tile, 4 waves of 64 x 64; the
// reduction runs over the pixels in steps of 16: thread (row = tid / 2, half = tid % 2) gathers 8 consecutive pixels of its dY
// row and of its im2col row (two 16-byte loads each when they are contiguous and inside the image, per-element otherwise),
// splits them into bf16 terms and writes them to LDS as the MFMA fragments [term][k-half][row] (16-byte chunks, conflict-free
// ds_read_b128); the next step's gathers are in flight under the current step's MFMAs; one barrier per step (two LDS stages).
// blockIdx.z splits the pixel axis, the parts are added with float atomics (dw / db zeroed by the launcher).
template <int NT>
__global__ __launch_bounds__(256, 2) void conv_wgrad_mfma_kernel(const float* __restrict__ x, long long x_bs,
                                                                 const float* __restrict__ dy, long long dy_bs,
                                                                 float* __restrict__ dw, float* __restrict__ db, int B, int Cin,
                                                                 int Cout, int H, int W, int OH, int OW, int KH, int KW, int stride,
                                                                 int padH, int padW) {
  constexpr int TC = 2, TP = 2;
  constexpr int OPC = NT * 2 * 128;                        // chunks of one operand of one stage
  __shared__ u32x4 S[2 * 2 * OPC];                         // [stage][A | B][term][k-half][row]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wave >> 1, wp = wave & 1, l31 = lane & 31, kh = lane >> 5;
  const int HWo = OH * OW, HWi = H * W, T = KH * KW, J = Cin * T;
  const long long Ptot = (long long)B * HWo;
  const int co0 = blockIdx.y * 128, j0 = blockIdx.x * 128;
  const long long nsteps = (Ptot + 15) >> 4;
  const long long per = (nsteps + gridDim.z - 1) / gridDim.z;
  const long long s_begin = (long long)blockIdx.z * per, s_end = s_begin + per < nsteps ? s_begin + per : nsteps;
  if (s_begin >= s_end) return;

  const int srow = tid >> 1, skg = tid & 1;
  const int co = co0 + srow, j = j0 + srow;
  const bool a_ok = co < Cout, b_ok = j < J;
  const int ci = b_ok ? j / T : 0, tap = b_ok ? j - ci * T : 0, ky = tap / KW, kx = tap - ky * KW;
  const float* arow = dy + (long long)(a_ok ? co : 0) * HWo;
  const float* brow = x + (long long)ci * HWi;
  float xa0[8], xb0[8], xa1[8], xb1[8];      // two register sets: the gathers run TWO steps ahead of the MFMAs that use them
  auto gather = [&](long long step, float (&xa)[8], float (&xb)[8]) {
    const long long p = step * 16 + skg * 8;
    int b = (int)(p / HWo), pix = (int)(p - (long long)b * HWo);
    int oy = pix / OW, ox = pix - oy * OW;
    // ---- A: 8 consecutive pixels of dY row co ----
    if (a_ok && b < B && pix + 8 <= HWo) {
      const f4u* q = reinterpret_cast<const f4u*>(arow + (long long)b * dy_bs + pix);
      const f4u v0 = q[0], v1 = q[1];
      xa[0] = v0.x; xa[1] = v0.y; xa[2] = v0.z; xa[3] = v0.w; xa[4] = v1.x; xa[5] = v1.y; xa[6] = v1.z; xa[7] = v1.w;
    } else {
      int bb = b, pp = pix;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        xa[q] = (a_ok && bb < B) ? arow[(long long)bb * dy_bs + pp] : 0.0f;
        if (++pp == HWo) { pp = 0; ++bb; }
      }
    }
    // ---- B: the im2col row j at the same 8 pixels ----
    const int iy = oy * stride + ky - padH, ix = ox * stride + kx - padW;
    if (b_ok && b < B && stride == 1 && ox + 8 <= OW && (unsigned)iy < (unsigned)H && ix >= 0 && ix + 8 <= W) {
      const f4u* q = reinterpret_cast<const f4u*>(brow + (long long)b * x_bs + (long long)iy * W + ix);
      const f4u v0 = q[0], v1 = q[1];
      xb[0] = v0.x; xb[1] = v0.y; xb[2] = v0.z; xb[3] = v0.w; xb[4] = v1.x; xb[5] = v1.y; xb[6] = v1.z; xb[7] = v1.w;
    } else {
      int bb = b, yy = oy, xx = ox;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int sy = yy * stride + ky - padH, sx = xx * stride + kx - padW;
        const bool ok = b_ok && bb < B && (unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W;
        xb[q] = ok ? brow[(long long)bb * x_bs + (long long)sy * W + sx] : 0.0f;
        if (++xx == OW) { xx = 0; if (++yy == OH) { yy = 0; ++bb; } }
      }
    }
  };
  f32x16 acc[TC][TP];
#pragma unroll
  for (int tc = 0; tc < TC; ++tc)
#pragma unroll
    for (int tp = 0; tp < TP; ++tp)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tc][tp][r] = 0.0f;
  float bsum = 0.0f;
  const bool want_b = db != nullptr && blockIdx.x == 0;
  // one step: split + store the registers gathered two steps ago, barrier, request step + 2 into the set just freed, MFMAs
#define WGRAD_STEP(STEP, XA, XB)                                                                                         \
  do {                                                                                                                   \
    u32x4* st = S + (((STEP) - s_begin) & 1) * 2 * OPC;                                                                  \
    {                                                                                                                    \
      u32x4 ta[NT], tb[NT];                                                                                              \
      split8_bf16<NT, 0>(XA, ta);                                                                                        \
      split8_bf16<NT, 0>(XB, tb);                                                                                        \
      _Pragma("unroll") for (int t = 0; t < NT; ++t) {                                                                   \
        st[(t * 2 + skg) * 128 + srow] = ta[t];                                                                          \
        st[OPC + (t * 2 + skg) * 128 + srow] = tb[t];                                                                    \
      }                                                                                                                  \
      if (want_b) bsum += ((XA[0] + XA[1]) + (XA[2] + XA[3])) + ((XA[4] + XA[5]) + (XA[6] + XA[7]));                     \
    }                                                                                                                    \
    __syncthreads();                                                                                                     \
    if ((STEP) + 2 < s_end) gather((STEP) + 2, XA, XB);                                                                  \
    bf16x8 A[NT][TC], Bf[NT][TP];                                                                                        \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) _Pragma("unroll") for (int i = 0; i < 2; ++i) {                       \
      A[t][i] = __builtin_bit_cast(bf16x8, st[(t * 2 + kh) * 128 + wc * 64 + i * 32 + l31]);                             \
      Bf[t][i] = __builtin_bit_cast(bf16x8, st[OPC + (t * 2 + kh) * 128 + wp * 64 + i * 32 + l31]);                      \
    }                                                                                                                    \
    constexpr int NPAIR = NT == 3 ? 6 : 3;                                                                               \
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0}; /* smallest products first */                  \
    _Pragma("unroll") for (int pr = 6 - NPAIR; pr < 6; ++pr) _Pragma("unroll") for (int tc = 0; tc < TC; ++tc)           \
        _Pragma("unroll") for (int tp = 0; tp < TP; ++tp) if (PA[pr] < NT && PB[pr] < NT)                                \
            acc[tc][tp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[PA[pr] < NT ? PA[pr] : 0][tc],                       \
                                                                  Bf[PB[pr] < NT ? PB[pr] : 0][tp], acc[tc][tp], 0, 0, 0); \
  } while (0)
  gather(s_begin, xa0, xb0);
  if (s_begin + 1 < s_end) gather(s_begin + 1, xa1, xb1);
  for (long long step = s_begin; step < s_end; step += 2) {
    WGRAD_STEP(step, xa0, xb0);
    if (step + 1 < s_end) WGRAD_STEP(step + 1, xa1, xb1);
  }
#undef WGRAD_STEP
#pragma unroll
  for (int tc = 0; tc < TC; ++tc)
#pragma unroll
    for (int tp = 0; tp < TP; ++tp)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = co0 + wc * 64 + tc * 32 + (r >> 2) * 8 + kh * 4 + (r & 3), col = j0 + wp * 64 + tp * 32 + l31;
        if (row < Cout && col < J) atomicAdd(&dw[(long long)row * J + col], acc[tc][tp][r]);
      }
  if (want_b && a_ok) atomicAdd(&db[co], bsum);
}

// The same GEMM for the shapes the fusion heads train on - stride 1, "same" width (OW == W), OW % 8 == 0, |kx - padW| <= 1 (3x3, 1x1,
// 3x1 ...) - with a BRANCH-FREE operand gather.  The general kernel above spends ~570 VALU instructions per 16-pixel step and wave
// next to 24 MFMAs (ISA count: a 64-bit division per step to find the batch item, and - because the 64 lanes of a wave hold
// im2col rows of different taps - both the contiguous and the per-element gather path in every step: at ox = 0 the kx = 0 rows
// overhang the image row, at ox = OW - 8 the kx = 2 rows): ~2 300 VALU cycles against 768 matrix cycles.  Here
//   * the pixel position (item, oy, ox) of a thread's 8-pixel chunk is carried from step to step (no division in the loop);
//   * every load is a range-checked buffer load: a chunk of a padding row, of a row past the last item or of a tile row past
//     Cout / J gets an offset outside the descriptor and arrives as zeros - no branch, no per-element bounds code;
//   * the im2col chunk [ox + d, ox + d + 8), d = kx - padW in {-1, 0, 1}, is the aligned chunk [ox, ox + 8) of the input row (two
//     16-byte loads) plus its left and right neighbour pixels (two 4-byte loads, zero outside the row), and the shift is a
//     register select when the values are consumed, two steps later.
// 1: the gather's loads as inline assembly with hand-counted waits (the compiler-managed form waits vmcnt(0) at the top of the
// loop - also for the set requested ONE step ago).  Measured on one box, alternating: 43.09 / 43.00 vs 43.36 / 42.99 ms per
// training step - no difference, so the product build keeps the compiler-managed loads (nothing for the scheduler to get wrong).
#ifndef ACCFLOW_WGRAD_ASMLOADS
#define ACCFLOW_WGRAD_ASMLOADS 0
#endif
typedef int wg_i32x4 __attribute__((ext_vector_type(4)));
typedef float wg_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wg_rsrc(wg_i32x4 desc) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)((((unsigned long long)(unsigned)desc[1]) << 32) | (unsigned)desc[0]), 0, desc[2], desc[3]);
}
__device__ __forceinline__ void wg_load4(wg_f32x4& dst, unsigned voff, wg_i32x4 desc, int soff) {
#if ACCFLOW_WGRAD_ASMLOADS
  asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(dst) : "v"(voff), "s"(desc), "s"(soff) : "memory");
#else
  dst = __builtin_bit_cast(wg_f32x4, __builtin_amdgcn_raw_buffer_load_b128(wg_rsrc(desc), (int)voff, soff, 0));
#endif
}
__device__ __forceinline__ void wg_load1(float& dst, unsigned voff, wg_i32x4 desc) {
#if ACCFLOW_WGRAD_ASMLOADS
  asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(dst) : "v"(voff), "s"(desc) : "memory");
#else
  dst = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wg_rsrc(desc), (int)voff, 0, 0));
#endif
}
template <int N>
__device__ __forceinline__ void wg_wait_vm() {
#if ACCFLOW_WGRAD_ASMLOADS
  asm volatile("s_waitcnt vmcnt(%0)" : : "n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
#endif
}

// R64 (round 6): a 64 x 256 tile (rows = output channels, 4 waves side by side along the im2col rows) for layers of <= 64 output
// channels - the 128 x 128 tile ran half of its matrix work and half of its A staging on padding there (the context encoder's
// 64 -> 64 3x3 layers at 128 x 128: a quarter of the step's weight-gradient time).  A thread then stages two B rows per step.
template <int NT, bool R64 = false>
__global__ __launch_bounds__(256, 2) void conv_wgrad_mfma_fast_kernel(const float* __restrict__ x, long long x_bs,
                                                                      const float* __restrict__ dy, long long dy_bs,
                                                                      float* __restrict__ dw, float* __restrict__ db, int B, int Cin,
                                                                      int Cout, int H, int W, int OH, int OW, int KH, int KW,
                                                                      int padH, int padW) {
  constexpr int TC = 2, TP = 2;
  constexpr int AR = R64 ? 64 : 128, BR = R64 ? 256 : 128, NB = R64 ? 2 : 1;   // tile rows of dY / of the im2col matrix; B rows per thread
  constexpr int OPA = NT * 2 * AR, OPB = NT * 2 * BR, STG = OPA + OPB;
  constexpr unsigned SENT = 0x80000000u;                   // (descriptors span < 2^31 bytes: checked by the launcher)
  __shared__ u32x4 S[2 * STG];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = R64 ? 0 : wave >> 1, wp = R64 ? wave : wave & 1, l31 = lane & 31, kh = lane >> 5;
  const int HWo = OH * OW, HWi = H * W, T = KH * KW, J = Cin * T;
  const long long Ptot = (long long)B * HWo;
  const int co0 = blockIdx.y * AR, j0 = blockIdx.x * BR;
  const long long nsteps = (Ptot + 15) >> 4;
  const long long per = (nsteps + gridDim.z - 1) / gridDim.z;
  const long long s_begin = (long long)blockIdx.z * per, s_end = s_begin + per < nsteps ? s_begin + per : nsteps;
  if (s_begin >= s_end) return;

  const int srow = tid >> 1, skg = tid & 1;
  const int co = co0 + srow;
  const bool a_row_live = srow < AR, a_ok = a_row_live && co < Cout;
  bool b_ok[NB];
  int ky[NB], dsh[NB], b_row[NB];                           // (dsh = kx - padW: -1 / 0 / +1)
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int j = j0 + srow + 128 * n;
    b_ok[n] = j < J;
    const int ci = b_ok[n] ? j / T : 0, tap = b_ok[n] ? j - ci * T : 0;
    ky[n] = tap / KW;
    dsh[n] = tap - ky[n] * KW - padW;
    b_row[n] = ci * HWi;
  }
  // this thread's chunk position, carried along: item sb, output row soy, column sox (a multiple of 8)
  int sb, soy, sox;
  {
    const long long p = s_begin * 16 + skg * 8;
    sb = (int)(p / HWo);
    const int pix = (int)(p - (long long)sb * HWo);
    soy = pix / OW;
    sox = pix - soy * OW;
  }
  typedef wg_f32x4 f32x4_;
  auto mkdesc = [](const void* base, long long bytes) {
    const unsigned long long bp = (unsigned long long)base;
    wg_i32x4 v;
    v[0] = (int)(unsigned)bp; v[1] = (int)(unsigned)((bp >> 32) & 0xFFFFu); v[2] = (int)(unsigned)bytes; v[3] = 0x00020000;
    return v;
  };
  const wg_i32x4 ra4 = mkdesc(dy, (((long long)(B - 1)) * dy_bs + (long long)Cout * HWo) * 4);
  const wg_i32x4 rb4 = mkdesc(x, (((long long)(B - 1)) * x_bs + (long long)Cin * HWi) * 4);
  // raw registers of one gathered step: A chunk (2 x 4), per B row its chunk (2 x 4) and the chunk's two neighbour pixels
  struct Raw { f32x4_ a0, a1, b0[NB], b1[NB]; float bl[NB], br[NB]; };
  constexpr int NLD = 2 + 4 * NB;                           // loads per gathered step
  // (32-bit element offsets: both tensors are < 2^31 bytes; everything is computed unconditionally and SELECTED, so that the
  // compiler keeps the gather straight-line - its if-converted form put an s_waitcnt vmcnt(0) inside a branch)
  const int dy_bs32 = (int)dy_bs, x_bs32 = (int)x_bs, a_row = co * HWo;
  auto sel = [](bool c, unsigned a) { const unsigned m = 0u - (unsigned)c; return (a & m) | (SENT & ~m); };
  auto gather = [&](Raw& g) {
    const bool live = sb < B;
    const unsigned aoff = sel(a_ok && live, (unsigned)(sb * dy_bs32 + a_row + soy * OW + sox) << 2);
    // (wg_load*: compiler-managed buffer loads in the product build; ACCFLOW_WGRAD_ASMLOADS=1: hand-placed, see above)
    wg_load4(g.a0, aoff, ra4, 0);
    wg_load4(g.a1, aoff, ra4, 16);
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const int iy = soy + ky[n] - padH;
      const bool rowok = b_ok[n] && live && (unsigned)iy < (unsigned)H;
      const unsigned braw = (unsigned)(sb * x_bs32 + b_row[n] + iy * W + sox) << 2;
      const unsigned boff = sel(rowok, braw);
      const unsigned loff = sel(rowok && sox > 0, braw - 4u), roff = sel(rowok && sox + 8 < W, braw + 32u);
      wg_load4(g.b0[n], boff, rb4, 0);
      wg_load4(g.b1[n], boff, rb4, 16);
      wg_load1(g.bl[n], loff, rb4);
      wg_load1(g.br[n], roff, rb4);
    }
    // the same half of the next step: 16 pixels on
    sox += 16;
    while (sox >= OW) { sox -= OW; ++soy; }
    while (soy >= OH) { soy -= OH; ++sb; }
  };
  f32x16 acc[TC][TP];
#pragma unroll
  for (int tc = 0; tc < TC; ++tc)
#pragma unroll
    for (int tp = 0; tp < TP; ++tp)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tc][tp][r] = 0.0f;
  float bsum = 0.0f;
  const bool want_b = db != nullptr && blockIdx.x == 0;
#define WGRAD_FSTEP(STEP, G)                                                                                             \
  do {                                                                                                                   \
    u32x4* st = S + (((STEP) - s_begin) & 1) * STG;                                                                      \
    if ((STEP) + 1 < s_end) wg_wait_vm<NLD>(); else wg_wait_vm<0>();   /* the loads of the OTHER set may stay in flight */ \
    if (!R64 || a_row_live) {                                                                                            \
      const float XA[8] = {G.a0.x, G.a0.y, G.a0.z, G.a0.w, G.a1.x, G.a1.y, G.a1.z, G.a1.w};                              \
      u32x4 ta[NT];                                                                                                      \
      split8_bf16<NT, 0>(XA, ta);                                                                                        \
      _Pragma("unroll") for (int t = 0; t < NT; ++t) st[(t * 2 + skg) * AR + srow] = ta[t];                              \
      if (want_b) bsum += ((XA[0] + XA[1]) + (XA[2] + XA[3])) + ((XA[4] + XA[5]) + (XA[6] + XA[7]));                     \
    }                                                                                                                    \
    _Pragma("unroll") for (int n = 0; n < NB; ++n) {                                                                     \
      const float E[10] = {G.bl[n], G.b0[n].x, G.b0[n].y, G.b0[n].z, G.b0[n].w, G.b1[n].x, G.b1[n].y, G.b1[n].z, G.b1[n].w, G.br[n]}; \
      float XB[8];                                                                                                       \
      _Pragma("unroll") for (int q = 0; q < 8; ++q) XB[q] = dsh[n] < 0 ? E[q] : (dsh[n] > 0 ? E[q + 2] : E[q + 1]);     \
      u32x4 tb[NT];                                                                                                      \
      split8_bf16<NT, 0>(XB, tb);                                                                                        \
      _Pragma("unroll") for (int t = 0; t < NT; ++t) st[OPA + (t * 2 + skg) * BR + srow + 128 * n] = tb[t];              \
    }                                                                                                                    \
    __syncthreads();                                                                                                     \
    if ((STEP) + 2 < s_end) gather(G);                                                                                   \
    bf16x8 A[NT][TC], Bf[NT][TP];                                                                                        \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) _Pragma("unroll") for (int i = 0; i < 2; ++i) {                       \
      A[t][i] = __builtin_bit_cast(bf16x8, st[(t * 2 + kh) * AR + wc * 64 + i * 32 + l31]);                              \
      Bf[t][i] = __builtin_bit_cast(bf16x8, st[OPA + (t * 2 + kh) * BR + wp * 64 + i * 32 + l31]);                       \
    }                                                                                                                    \
    constexpr int NPAIR = NT == 3 ? 6 : 3;                                                                               \
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};                                                \
    _Pragma("unroll") for (int pr = 6 - NPAIR; pr < 6; ++pr) _Pragma("unroll") for (int tc = 0; tc < TC; ++tc)           \
        _Pragma("unroll") for (int tp = 0; tp < TP; ++tp) if (PA[pr] < NT && PB[pr] < NT)                                \
            acc[tc][tp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[PA[pr] < NT ? PA[pr] : 0][tc],                       \
                                                                  Bf[PB[pr] < NT ? PB[pr] : 0][tp], acc[tc][tp], 0, 0, 0); \
  } while (0)
  Raw g0, g1;
  gather(g0);
  if (s_begin + 1 < s_end) gather(g1);
  for (long long step = s_begin; step < s_end; step += 2) {
    WGRAD_FSTEP(step, g0);
    if (step + 1 < s_end) WGRAD_FSTEP(step + 1, g1);
  }
#undef WGRAD_FSTEP
#pragma unroll
  for (int tc = 0; tc < TC; ++tc)
#pragma unroll
    for (int tp = 0; tp < TP; ++tp)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = co0 + wc * 64 + tc * 32 + (r >> 2) * 8 + kh * 4 + (r & 3), col = j0 + wp * 64 + tp * 32 + l31;
        if (row < Cout && col < J) atomicAdd(&dw[(long long)row * J + col], acc[tc][tp][r]);
      }
  if (want_b && a_ok) atomicAdd(&db[co], bsum);
}

// Modulated deformable convolution (torchvision.ops.deform_conv2d, AccFlow_.py:104) backward, second half: from the gradient of
// the deformed columns dcols[b][tap*C + c][p] (= W^T dY, a 1x1 convolution) to the gradients of the input (bilinear scatter,
// float atomics), of the offsets (dy first, then dx: d sample / d h, d w with the floor cell held fixed - what autograd of the
// bilinear formula gives) and of the modulation mask.  Thread = (b, tap, pixel), loop over the channels.
constexpr int DEFORM_CG = 16;
// One coordinate of a sample, position = tap position `base` (an integer) + offset, as the cell below it and the fraction inside
// the cell: cell = base + floor(offset), frac = offset - floor(offset) - exact to 2^-24 px wherever the sample lies.  The sum
// (float)base + offset instead is a multiple of 2^-16 px at coordinates of 128 .. 256 (of 2^-14 at 512 ..): its rounding moved
// d offset of a 241-pixel-wide plane by 1.1e-4 of its RMS against float64 (d mask 6.7e-5, d x 4.6e-5).
// Returns whether -1 < position < size (torchvision's condition for a sample to count); a NaN or huge offset is outside.
__device__ __forceinline__ bool deform_cell(int base, float offset, int size, int& cell, float& frac) {
  const float fo = floorf(offset);
  cell = base + (int)fminf(fmaxf(fo, -1.0e9f), 1.0e9f);
  frac = offset - fo;
  return cell <= size - 1 && (cell >= 0 || (cell == -1 && frac > 0.0f));
}
__global__ __launch_bounds__(256) void deform_backward_kernel(const float* __restrict__ x, long long x_bs,
                                                              const float* __restrict__ off, long long off_bs,
                                                              const float* __restrict__ msk, long long msk_bs,
                                                              const float* __restrict__ dcols, float* __restrict__ dx,
                                                              long long dx_bs, float* __restrict__ doff, float* __restrict__ dmsk,
                                                              int B, int C, int H, int W, int KH, int KW, int padH, int padW) {
  const int HW = H * W, T = KH * KW;
  // blockIdx.y = channel group: the thread sums its DEFORM_CG channels; the groups' shares of d offset / d mask are added with
  // float atomics (outputs zeroed by the launcher) - a thread per (b, tap, pixel) looping over all 128 channels was 574 us
  const int c_begin = blockIdx.y * DEFORM_CG, c_end = c_begin + DEFORM_CG < C ? c_begin + DEFORM_CG : C;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * T * HW) return;
  const int p = (int)(i % HW), tap = (int)((i / HW) % T), b = (int)(i / ((long long)HW * T));
  const int y = p / W, xx = p - y * W, ky = tap / KW, kx = tap - ky * KW;
  const float dyo = off[b * off_bs + (long long)(2 * tap) * HW + p], dxo = off[b * off_bs + (long long)(2 * tap + 1) * HW + p];
  const float m = msk[b * msk_bs + (long long)tap * HW + p];
  int hl, wl;
  float lh, lw;
  const bool inside_h = deform_cell(y - padH + ky, dyo, H, hl, lh), inside_w = deform_cell(xx - padW + kx, dxo, W, wl, lw);
  float g_h = 0.0f, g_w = 0.0f, g_m = 0.0f;
  if (inside_h && inside_w) {
    const int hh = hl + 1, wh = wl + 1;
    const float uh = 1.0f - lh, uw = 1.0f - lw;
    const bool o1 = hl >= 0 && wl >= 0, o2 = hl >= 0 && wh <= W - 1, o3 = hh <= H - 1 && wl >= 0, o4 = hh <= H - 1 && wh <= W - 1;
    const int i1 = o1 ? hl * W + wl : 0, i2 = o2 ? hl * W + wh : 0, i3 = o3 ? hh * W + wl : 0, i4 = o4 ? hh * W + wh : 0;
    const float* src = x + b * x_bs;
    float* dsrc = dx + b * dx_bs;
    const float* dc = dcols + ((long long)b * T * C + (long long)tap * C) * HW + p;
    for (int c = c_begin; c < c_end; ++c) {
      const float* plane = src + (long long)c * HW;
      const float v1 = o1 ? plane[i1] : 0.0f, v2 = o2 ? plane[i2] : 0.0f, v3 = o3 ? plane[i3] : 0.0f, v4 = o4 ? plane[i4] : 0.0f;
      const float g = dc[(long long)c * HW];
      g_m += g * (uh * uw * v1 + uh * lw * v2 + lh * uw * v3 + lh * lw * v4);
      g_h += g * m * (uw * (v3 - v1) + lw * (v4 - v2));
      g_w += g * m * (uh * (v2 - v1) + lh * (v4 - v3));
      float* dplane = dsrc + (long long)c * HW;
      const float gm = g * m;
      if (o1) atomicAdd(&dplane[i1], gm * uh * uw);
      if (o2) atomicAdd(&dplane[i2], gm * uh * lw);
      if (o3) atomicAdd(&dplane[i3], gm * lh * uw);
      if (o4) atomicAdd(&dplane[i4], gm * lh * lw);
    }
  }
  atomicAdd(&doff[((long long)b * 2 * T + 2 * tap) * HW + p], g_h);
  atomicAdd(&doff[((long long)b * 2 * T + 2 * tap + 1) * HW + p], g_w);
  atomicAdd(&dmsk[((long long)b * T + tap) * HW + p], g_m);
}

// The same for images whose plane fits LDS (H * W <= DEFORM_LDS_PX, e.g. the 32 x 32 feature maps of the 256 x 256 training crops):
// a workgroup owns the planes of CG channels of one batch item ENTIRELY - it walks all (tap, pixel) samples, scatters into LDS
// (ds_add_f32) and writes its planes with plain stores.  The global-atomic form above spends 141 M float atomics on a 3.9 M element
// tensor at batch 30 (36 per element: 2.7 ms); here none are left for d x.  d offset / d mask: the channel groups' shares by
// global float atomics as above (outputs zeroed by the launcher).
constexpr int DEFORM_LDS_PX = 4096;
template <int CG>
__global__ __launch_bounds__(256) void deform_backward_lds_kernel(const float* __restrict__ x, long long x_bs,
                                                                  const float* __restrict__ off, long long off_bs,
                                                                  const float* __restrict__ msk, long long msk_bs,
                                                                  const float* __restrict__ dcols, float* __restrict__ dx,
                                                                  long long dx_bs, float* __restrict__ doff,
                                                                  float* __restrict__ dmsk, int B, int C, int H, int W, int KH,
                                                                  int KW, int padH, int padW) {
  extern __shared__ float acc_lds[];                     // [CG][HW]
  const int HW = H * W, T = KH * KW;
  const int b = blockIdx.x, c_begin = blockIdx.y * CG;
  const int nc = C - c_begin < CG ? C - c_begin : CG;
  for (int i = threadIdx.x; i < CG * HW; i += 256) acc_lds[i] = 0.0f;
  __syncthreads();
  const float* src = x + b * x_bs + (long long)c_begin * HW;
  for (int it = threadIdx.x; it < T * HW; it += 256) {
    const int tap = it / HW, p = it - tap * HW;
    const int y = p / W, xx = p - y * W, ky = tap / KW, kx = tap - ky * KW;
    const float dyo = off[b * off_bs + (long long)(2 * tap) * HW + p], dxo = off[b * off_bs + (long long)(2 * tap + 1) * HW + p];
    const float m = msk[b * msk_bs + (long long)tap * HW + p];
    int hl, wl;
    float lh, lw;
    if (!deform_cell(y - padH + ky, dyo, H, hl, lh) || !deform_cell(xx - padW + kx, dxo, W, wl, lw)) continue;
    const int hh = hl + 1, wh = wl + 1;
    const float uh = 1.0f - lh, uw = 1.0f - lw;
    const bool o1 = hl >= 0 && wl >= 0, o2 = hl >= 0 && wh <= W - 1, o3 = hh <= H - 1 && wl >= 0, o4 = hh <= H - 1 && wh <= W - 1;
    const int i1 = o1 ? hl * W + wl : 0, i2 = o2 ? hl * W + wh : 0, i3 = o3 ? hh * W + wl : 0, i4 = o4 ? hh * W + wh : 0;
    const float* dc = dcols + ((long long)b * T * C + (long long)tap * C + c_begin) * HW + p;
    float g_h = 0.0f, g_w = 0.0f, g_m = 0.0f;
    for (int c = 0; c < nc; ++c) {
      const float* plane = src + (long long)c * HW;
      const float v1 = o1 ? plane[i1] : 0.0f, v2 = o2 ? plane[i2] : 0.0f, v3 = o3 ? plane[i3] : 0.0f, v4 = o4 ? plane[i4] : 0.0f;
      const float g = dc[(long long)c * HW];
      g_m += g * (uh * uw * v1 + uh * lw * v2 + lh * uw * v3 + lh * lw * v4);
      g_h += g * m * (uw * (v3 - v1) + lw * (v4 - v2));
      g_w += g * m * (uh * (v2 - v1) + lh * (v4 - v3));
      float* a = acc_lds + c * HW;
      const float gm = g * m;
      if (o1) atomicAdd(&a[i1], gm * uh * uw);
      if (o2) atomicAdd(&a[i2], gm * uh * lw);
      if (o3) atomicAdd(&a[i3], gm * lh * uw);
      if (o4) atomicAdd(&a[i4], gm * lh * lw);
    }
    atomicAdd(&doff[((long long)b * 2 * T + 2 * tap) * HW + p], g_h);
    atomicAdd(&doff[((long long)b * 2 * T + 2 * tap + 1) * HW + p], g_w);
    atomicAdd(&dmsk[((long long)b * T + tap) * HW + p], g_m);
  }
  __syncthreads();
  float* dst = dx + b * dx_bs + (long long)c_begin * HW;
  for (int i = threadIdx.x; i < nc * HW; i += 256) dst[i] = acc_lds[i];
}

}  // namespace

extern "C" int accflow_act_backward_f32(const float* dy, long long dy_bs, const float* y, long long y_bs, float* dx, long long dx_bs,
                                        int B, long long CHW, int act, void* stream) {
  if (!dy || !y || !dx || B <= 0 || CHW <= 0) return 1;
  hipLaunchKernelGGL(act_backward_kernel, dim3(cdiv(CHW, 256)), dim3(256), 0, as_stream(stream), dy, dy_bs, y, y_bs, dx, dx_bs, B,
                     CHW, act);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_add_f32(float* dst, long long dst_bs, const float* src, long long src_bs, int B, long long CHW, void* stream) {
  if (!dst || !src || B <= 0 || CHW <= 0) return 1;
  hipLaunchKernelGGL(add_kernel, dim3(cdiv(CHW, 256)), dim3(256), 0, as_stream(stream), dst, dst_bs, src, src_bs, B, CHW);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_l1_grad_f32(const float* pred, const float* gt, float* dpred, long long n, float scale, void* stream) {
  if (!pred || !gt || !dpred || n <= 0) return 1;
  hipLaunchKernelGGL(l1_grad_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), pred, gt, dpred, n, scale);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_dilate_f32(const float* src, long long src_bs, float* dst, int B, int C, int OH, int OW, int Hd, int Wd,
                                  int stride, void* stream) {
  if (!src || !dst || B <= 0 || C <= 0 || OH <= 0 || OW <= 0 || stride <= 0 || Hd < (OH - 1) * stride + 1 ||
      Wd < (OW - 1) * stride + 1)
    return 1;
  hipMemsetAsync(dst, 0, (size_t)B * C * Hd * Wd * sizeof(float), as_stream(stream));
  hipLaunchKernelGGL(dilate_kernel, dim3(cdiv((long long)B * C * OH * OW, 256)), dim3(256), 0, as_stream(stream), src, src_bs, dst,
                     B, C, OH, OW, Hd, Wd, stride);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_blend_backward_f32(const float* dy, const float* f1, const float* f2, const float* m, float* df1,
                                          float* df2, float* dm, int B, int C, int HW, void* stream) {
  if (!dy || !f1 || !f2 || !m || !df1 || !df2 || !dm || B <= 0 || C <= 0 || HW <= 0) return 1;
  hipLaunchKernelGGL(blend_backward_kernel, dim3(cdiv((long long)B * HW, 256)), dim3(256), 0, as_stream(stream), dy, f1, f2, m,
                     df1, df2, dm, B, C, HW);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_convex_upsample_backward_f32(const float* dup, const float* flow, const float* mask, float* dflow,
                                                    float* dmask, int B, int H8, int W8, void* stream) {
  if (!dup || !flow || !mask || !dflow || !dmask || B <= 0 || H8 <= 0 || W8 <= 0) return 1;
  hipMemsetAsync(dflow, 0, (size_t)B * 2 * H8 * W8 * sizeof(float), as_stream(stream));
  hipLaunchKernelGGL(convex_upsample_backward_kernel, dim3(cdiv((long long)B * 64 * H8 * W8, 256)), dim3(256), 0, as_stream(stream),
                     dup, flow, mask, dflow, dmask, B, H8, W8);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

// Every decision of the weight-gradient launch - kernel, operand terms, grid, pixel parts - as ONE host function: the launcher
// below runs what it returns, accflow_conv_wgrad_plan reports it (tests pin their cases to a route through it).  No device call.
struct wgrad_plan {
  int kernel, terms, OH, OW;          // kernel: ACCFLOW_WGRAD_GENERAL / _FAST128 / _FAST64
  unsigned gx, gy, gz;
  long long per, nsteps;              // steps of 16 pixels per part (as the kernels derive it from gridDim.z) / in all
};
static int conv_wgrad_plan(int B, int Cin, int Cout, int H, int W, int KH, int KW, int stride, int padH, int padW, long long x_bs,
                           long long dy_bs, wgrad_plan* pl) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0 || stride <= 0) return 1;
  const int OH = (H + 2 * padH - KH) / stride + 1, OW = (W + 2 * padW - KW) / stride + 1;
  if (OH <= 0 || OW <= 0) return 1;
  const int J = Cin * KH * KW;
  const long long Ptot = (long long)B * OH * OW, nsteps = (Ptot + 15) / 16;
  // (layers of <= 64 output channels on the fast kernel's 64 x 256 tile, ACCFLOW_WGRAD_R64=0: the 128 x 128 tile everywhere)
  static const bool r64_on = [] { const char* e = getenv("ACCFLOW_WGRAD_R64"); return !e || atoi(e) != 0; }();
  static const bool fast_on = [] { const char* e = getenv("ACCFLOW_WGRAD_FAST"); return !e || atoi(e) != 0; }();
  // the branch-free gather (conv_wgrad_mfma_fast_kernel): stride 1, "same" width, rows of whole 8-pixel chunks, |kx - padW| <= 1,
  // both tensors below 2^31 bytes; ACCFLOW_WGRAD_FAST=0: the general kernel everywhere (A/B runs, tests)
  const bool fast = fast_on && stride == 1 && OW == W && (OW & 7) == 0 && padW <= 1 && KW - 1 - padW <= 1 && padW >= 0 && padH >= 0 &&
                    (((long long)(B - 1)) * x_bs + (long long)Cin * H * W) * 4 < (1LL << 31) &&
                    (((long long)(B - 1)) * dy_bs + (long long)Cout * OH * OW) * 4 < (1LL << 31);
  const bool r64 = fast && r64_on && Cout <= 64;
  const int tiles = r64 ? cdiv(J, 256) : cdiv(J, 128) * cdiv(Cout, 128);
  // Parts along the pixel axis (blockIdx.z; added with float atomics).  Two costs pull against each other: a part runs
  // nsteps / Z steps, and every part adds its 128 x 128 tile to the SAME addresses as the other parts of that tile - Z
  // serialised atomic rounds (~0.4 us each: a single-tile 1x1 shape cut into 240 parts spent 100 of its 105 us there).
  // Z = what fills `target` workgroup slots (rounded DOWN: one more part than fits starts a second, nearly empty round of
  // workgroups), capped where the atomic rounds would outweigh the shortened loop, Z <= sqrt(catom * nsteps).
  static const int target = [] { const char* e = getenv("ACCFLOW_WGRAD_WGS"); return e ? atoi(e) : 512; }();
  static const int zfloor = [] { const char* e = getenv("ACCFLOW_WGRAD_FLOOR"); return e ? atoi(e) : 1; }();
  static const double catom = [] { const char* e = getenv("ACCFLOW_WGRAD_CATOM"); return e ? atof(e) : 2.4; }();
  long long Z = tiles >= target ? 1 : (zfloor ? target / tiles : cdiv(target, tiles));
  if (catom > 0.0) {
    long long zc = (long long)sqrt(catom * (double)nsteps);
    if (zc < 1) zc = 1;
    if (Z > zc) Z = zc;
  }
  if (Z * 8 > nsteps) Z = nsteps / 8 > 0 ? nsteps / 8 : 1;   // at least 8 steps of 16 pixels per part
  // operand split: 3 bf16 terms / 6 products (fp32-equivalent; default) or, ACCFLOW_WGRAD_TERMS=2, 2 terms / 3 products (16
  // mantissa bits per operand: passes the same gradient tests - 1e-5 of the gradient's RMS - but measured no shorter step:
  // the training step is not bound by this kernel's matrix work)
  static const int terms = [] { const char* e = getenv("ACCFLOW_WGRAD_TERMS"); return e ? atoi(e) : 3; }();
  pl->kernel = r64 ? ACCFLOW_WGRAD_FAST64 : (fast ? ACCFLOW_WGRAD_FAST128 : ACCFLOW_WGRAD_GENERAL);
  pl->terms = terms >= 3 ? 3 : 2;
  pl->OH = OH;
  pl->OW = OW;
  pl->gx = r64 ? cdiv(J, 256) : cdiv(J, 128);
  pl->gy = r64 ? 1 : cdiv(Cout, 128);
  pl->gz = (unsigned)Z;
  pl->per = (nsteps + Z - 1) / Z;
  pl->nsteps = nsteps;
  return 0;
}

extern "C" int accflow_conv_wgrad_plan(int B, int Cin, int Cout, int H, int W, int KH, int KW, int stride, int padH, int padW,
                                       long long x_bs, long long dy_bs, int* out, int n) {
  wgrad_plan pl;
  if (!out || n < 7 || conv_wgrad_plan(B, Cin, Cout, H, W, KH, KW, stride, padH, padW, x_bs, dy_bs, &pl)) return 1;
  const long long imax = 0x7fffffff;
  out[0] = pl.kernel;
  out[1] = pl.terms;
  out[2] = (int)pl.gx;
  out[3] = (int)pl.gy;
  out[4] = (int)pl.gz;
  out[5] = (int)(pl.per < imax ? pl.per : imax);
  out[6] = (int)(pl.nsteps < imax ? pl.nsteps : imax);
  return 0;
}

extern "C" int accflow_conv_wgrad_f32(const float* x, long long x_bs, const float* dy, long long dy_bs, float* dw, float* db, int B,
                                      int Cin, int Cout, int H, int W, int KH, int KW, int stride, int padH, int padW,
                                      void* stream) {
  wgrad_plan pl;
  if (!x || !dy || !dw || conv_wgrad_plan(B, Cin, Cout, H, W, KH, KW, stride, padH, padW, x_bs, dy_bs, &pl)) return 1;
  const int OH = pl.OH, OW = pl.OW;
  hipMemsetAsync(dw, 0, (size_t)Cout * Cin * KH * KW * sizeof(float), as_stream(stream));
  if (db) hipMemsetAsync(db, 0, (size_t)Cout * sizeof(float), as_stream(stream));
  const dim3 grid(pl.gx, pl.gy, pl.gz);
  if (pl.kernel == ACCFLOW_WGRAD_FAST64) {
    if (pl.terms >= 3)
      hipLaunchKernelGGL((conv_wgrad_mfma_fast_kernel<3, true>), grid, dim3(256), 0, as_stream(stream), x, x_bs, dy, dy_bs, dw, db, B,
                         Cin, Cout, H, W, OH, OW, KH, KW, padH, padW);
    else
      hipLaunchKernelGGL((conv_wgrad_mfma_fast_kernel<2, true>), grid, dim3(256), 0, as_stream(stream), x, x_bs, dy, dy_bs, dw, db, B,
                         Cin, Cout, H, W, OH, OW, KH, KW, padH, padW);
    ACCFLOW_RETURN_LAUNCH_STATUS();
  }
  if (pl.kernel == ACCFLOW_WGRAD_FAST128) {
    if (pl.terms >= 3)
      hipLaunchKernelGGL((conv_wgrad_mfma_fast_kernel<3>), grid, dim3(256), 0, as_stream(stream), x, x_bs, dy, dy_bs, dw, db, B, Cin,
                         Cout, H, W, OH, OW, KH, KW, padH, padW);
    else
      hipLaunchKernelGGL((conv_wgrad_mfma_fast_kernel<2>), grid, dim3(256), 0, as_stream(stream), x, x_bs, dy, dy_bs, dw, db, B, Cin,
                         Cout, H, W, OH, OW, KH, KW, padH, padW);
    ACCFLOW_RETURN_LAUNCH_STATUS();
  }
  if (pl.terms >= 3)
    hipLaunchKernelGGL((conv_wgrad_mfma_kernel<3>), grid, dim3(256), 0, as_stream(stream), x, x_bs, dy, dy_bs, dw, db, B, Cin, Cout, H,
                       W, OH, OW, KH, KW, stride, padH, padW);
  else
    hipLaunchKernelGGL((conv_wgrad_mfma_kernel<2>), grid, dim3(256), 0, as_stream(stream), x, x_bs, dy, dy_bs, dw, db, B, Cin, Cout, H,
                       W, OH, OW, KH, KW, stride, padH, padW);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_deform_conv_backward_f32(const float* x, long long x_bs, const float* offset, long long offset_bs,
                                                const float* dmask_in, long long dmask_bs, const float* dcols, float* dx,
                                                long long dx_bs, float* doffset, float* ddmask, int B, int C, int H, int W, int KH,
                                                int KW, int padH, int padW, void* stream) {
  if (!x || !offset || !dmask_in || !dcols || !dx || !doffset || !ddmask || B <= 0 || C <= 0 || H <= 0 || W <= 0) return 1;
  hipMemsetAsync(doffset, 0, (size_t)B * 2 * KH * KW * H * W * sizeof(float), as_stream(stream));
  hipMemsetAsync(ddmask, 0, (size_t)B * KH * KW * H * W * sizeof(float), as_stream(stream));
  if (H * W <= DEFORM_LDS_PX) {   // the plane fits LDS: no global atomics for d x (deform_backward_lds_kernel)
    // channels per workgroup: as many as 64 KB of LDS hold (the per-sample offset / weight arithmetic is shared by them)
#define DEFORM_LDS_LAUNCH(CG)                                                                                                   \
  hipLaunchKernelGGL((deform_backward_lds_kernel<CG>), dim3(B, cdiv(C, CG)), dim3(256), (size_t)CG * H * W * sizeof(float),        \
                     as_stream(stream), x, x_bs, offset, offset_bs, dmask_in, dmask_bs, dcols, dx, dx_bs, doffset, ddmask, B, C, H, \
                     W, KH, KW, padH, padW)
    if (H * W <= 1024) DEFORM_LDS_LAUNCH(16);
    else if (H * W <= 2048) DEFORM_LDS_LAUNCH(8);
    else DEFORM_LDS_LAUNCH(4);
#undef DEFORM_LDS_LAUNCH
    ACCFLOW_RETURN_LAUNCH_STATUS();
  }
  for (int b = 0; b < B; ++b) hipMemsetAsync(dx + (long long)b * dx_bs, 0, (size_t)C * H * W * sizeof(float), as_stream(stream));
  const long long n = (long long)B * KH * KW * H * W;
  hipLaunchKernelGGL(deform_backward_kernel, dim3(cdiv(n, 256), cdiv(C, DEFORM_CG)), dim3(256), 0, as_stream(stream), x, x_bs, offset, offset_bs,
                     dmask_in, dmask_bs, dcols, dx, dx_bs, doffset, ddmask, B, C, H, W, KH, KW, padH, padW);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
