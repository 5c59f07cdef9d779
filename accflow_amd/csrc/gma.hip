// GMA attention (gma/modules.py:54-76, content-only branch, heads = 1) and aggregation
// (gma/modules.py:102-115).  The P x P attention matrix is materialised once per image1 (fp32, as the
// reference does) and re-read every GRU iteration by the aggregation GEMM, which is the HBM-bound part.
// The matrix-core routes are 1x1 convolutions built here: v * gamma (q, k) packed per call (conv_pack.hip), the descriptor
// planned and launched on the direct or the im2col kernel.
#include "common.h"
#include "launchers.h"

namespace {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum2(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// in-place softmax over each row of a (rows, n) matrix; one workgroup per row.
__global__ __launch_bounds__(256) void row_softmax_kernel(float* __restrict__ a, int n) {
  __shared__ float red[4];
  float* row = a + (long long)blockIdx.x * n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float mx = -INFINITY;
  for (int i = threadIdx.x; i < n; i += 256) mx = fmaxf(mx, row[i]);
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float s = 0.0f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float e = expf(row[i] - mx);
    row[i] = e;
    s += e;
  }
  s = wave_sum2(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  s = (red[0] + red[1]) + (red[2] + red[3]);
  for (int i = threadIdx.x; i < n; i += 256) row[i] = row[i] / s;
}

// out[b][d][i] = fmap[b][d][i] + gamma * sum_j V[b][d][j] * attn[b][i][j]   (both operands k-contiguous)
// Tile: all 128 rows d  x  128 columns i; operands are transposed into the k-major LDS layout of
// mma_slab while staging (global float4 along k, four conflict-free ds_write_b32).
__global__ __launch_bounds__(256) void gma_aggregate_kernel(const float* __restrict__ attn, const float* __restrict__ v,
                                                            const float* __restrict__ fmap,
                                                            const float* __restrict__ gamma, float* __restrict__ out,
                                                            long long out_bs, int D, int P) {
  constexpr int BC = 128, BP = 128, BK = MMA_BK;
  __shared__ __attribute__((aligned(16))) float Vs[2][BK * BC];
  __shared__ __attribute__((aligned(16))) float As[2][BK * BP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wc = wave >> 1, wp = wave & 1;
  const int b = blockIdx.z, i0 = blockIdx.x * BP, d0 = blockIdx.y * BC;
  const float* vb = v + (long long)b * D * P;
  const float* ab = attn + (long long)b * P * P;
  const int row = tid & 127, kq = tid >> 7;  // each thread: one row, 8 consecutive k
  const bool vec = (P & 3) == 0;
  float vr[8], ar[8];
  auto load = [&](int kbase) {
    const int k0 = kbase + kq * 8;
    const int d = d0 + row, i = i0 + row;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = k0 + h * 4;
      if (vec && k + 3 < P) {
        const float4 t = d < D ? *reinterpret_cast<const float4*>(vb + (long long)d * P + k) : make_float4(0, 0, 0, 0);
        const float4 u = i < P ? *reinterpret_cast<const float4*>(ab + (long long)i * P + k) : make_float4(0, 0, 0, 0);
        vr[h * 4 + 0] = t.x; vr[h * 4 + 1] = t.y; vr[h * 4 + 2] = t.z; vr[h * 4 + 3] = t.w;
        ar[h * 4 + 0] = u.x; ar[h * 4 + 1] = u.y; ar[h * 4 + 2] = u.z; ar[h * 4 + 3] = u.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          vr[h * 4 + q] = (d < D && k + q < P) ? vb[(long long)d * P + k + q] : 0.0f;
          ar[h * 4 + q] = (i < P && k + q < P) ? ab[(long long)i * P + k + q] : 0.0f;
        }
      }
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      Vs[buf][(kq * 8 + q) * BC + row] = vr[q];
      As[buf][(kq * 8 + q) * BP + row] = ar[q];
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int tc = 0; tc < 2; ++tc)
#pragma unroll
    for (int tp = 0; tp < 2; ++tp)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tc][tp][r] = 0.0f;
  const int nslab = (P + BK - 1) / BK;
  load(0);
  store(0);
  __syncthreads();
  for (int s = 0; s < nslab; ++s) {
    const int cur = s & 1;
    if (s + 1 < nslab) load((s + 1) * BK);
    mma_slab<2, 2, BC, BP>(Vs[cur], As[cur], acc, wc * 64, wp * 64, lane);
    if (s + 1 < nslab) store(cur ^ 1);
    __syncthreads();
  }
  const float g = gamma[0];
  const int l31 = lane & 31;
#pragma unroll
  for (int tp = 0; tp < 2; ++tp) {
    const int i = i0 + wp * 64 + tp * 32 + l31;
    if (i >= P) continue;
#pragma unroll
    for (int tc = 0; tc < 2; ++tc)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int d = d0 + wc * 64 + tc * 32 + acc_row(r, lane);
        if (d < D) out[b * out_bs + (long long)d * P + i] = fmap[((long long)b * D + d) * P + i] + g * acc[tc][tp][r];
      }
  }
}

// In-place softmax over the ROWS index j of a (P x P) matrix stored j-major.  (One thread per column walking all P rows
// left 342 workgroups on the chip at 720x1280: 10.6 ms per call.)
// Column softmax with the rows dealt to 16 waves per 64 columns (wave w takes rows w, w + 16, ...), TWO sweeps: an online
// (max, sum of exponentials) pass - the 16 partial pairs of a column meet in LDS and are combined in a fixed order -
// and one read-normalise-write pass.  2 reads + 1 write of the matrix instead of the 3 + 2 of max / exp / scale sweeps.
__global__ __launch_bounds__(1024) void col_softmax16_kernel(float* __restrict__ a, int P) {
  __shared__ float redm[16][64], reds[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  const bool live = i < P;
  float* col = a + (long long)blockIdx.y * P * P + (live ? i : 0);
  constexpr int U = 8;
  float mx = -INFINITY, s = 0.0f;
  for (int j = wave; j < P; j += 16 * U) {
    float x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = (live && j + 16 * u < P) ? col[(long long)(j + 16 * u) * P] : -INFINITY;
    float m2 = mx;
#pragma unroll
    for (int u = 0; u < U; ++u) m2 = fmaxf(m2, x[u]);
    if (m2 > -INFINITY) {   // (a dead lane or an all -inf column keeps s = 0)
      float t = 0.0f;
#pragma unroll
      for (int u = 0; u < U; ++u) t += expf(x[u] - m2);
      s = s * expf(mx - m2) + t;
      mx = m2;
    }
  }
  redm[wave][lane] = mx;
  reds[wave][lane] = s;
  __syncthreads();
  float m = -INFINITY;
#pragma unroll
  for (int w = 0; w < 16; ++w) m = fmaxf(m, redm[w][lane]);
  float tot = 0.0f;
#pragma unroll
  for (int w = 0; w < 16; ++w) tot += redm[w][lane] > -INFINITY ? reds[w][lane] * expf(redm[w][lane] - m) : 0.0f;
  const float inv = 1.0f / tot;
  for (int j = wave; j < P; j += 16 * U) {
    float x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = (live && j + 16 * u < P) ? col[(long long)(j + 16 * u) * P] : -INFINITY;
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (live && j + 16 * u < P) col[(long long)(j + 16 * u) * P] = expf(x[u] - m) * inv;
  }
}

}  // namespace

// Transposed-attention pair used by the estimator's hot path (same numbers, j-major storage):
//   attnT[b][j][i] = softmax_j(scale * <q_i, k_j>)
extern "C" long long accflow_gma_attention_ws_bytes(int D, int H, int W) { return accflow_corr_volume_ws_bytes(D, H, W); }

extern "C" int accflow_gma_attention_t_f32(const float* qk, float* attnT, void* ws, int mode, int B, int D, int H, int W,
                                           float scale, void* stream) {
  if (!qk || !attnT || B <= 0 || D <= 0 || H <= 0 || W <= 0) return 1;
  const int P = H * W;
  hipStream_t st = as_stream(stream);
  static const bool split_ok = [] { const char* e = getenv("ACCFLOW_GMA_QK_SPLIT"); return !e || atoi(e) != 0; }();
  // C[j][i] = scale * sum_d k[d][j] * q[d][i]: with scale = D^-1/2 (GMA's, modules.py:42) this is the correlation
  // volume of (k, q), so the split modes reuse its matrix-core GEMM (bf16x6: fp32-equivalent) pair by pair.
  // P > 32: that GEMM is a convolution with P output rows, and accflow_conv2d_f32 gives <= 32 rows to the fp32 kernels, which
  // read the weight pack as fp32 - level 0 writes only the split pack (the correlation volume never has fewer than 64 pixels)
  if (split_ok && mode != ACCFLOW_CONV_F32 && ws && P > 32 && fabsf(scale * sqrtf((float)D) - 1.0f) < 1e-6f) {
    for (int b = 0; b < B; ++b) {
      const float* q = qk + (long long)b * 2 * D * P;
      const int rc = accflow_corr_level0_bf16s(q + (long long)D * P, q, attnT + (long long)b * P * P, ws, 1, D, H, W,
                                               ACCFLOW_CONV_BF16X6, 0, nullptr, st, nullptr, nullptr);
      if (rc) return rc;
    }
  } else {
    const int rc = accflow_gemm_atb_f32(qk + (long long)D * P, qk, attnT, P, P, D, 2LL * D * P, 2LL * D * P,
                                        (long long)P * P, B, scale, st);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(col_softmax16_kernel, dim3(cdiv(P, 64), B), dim3(1024), 0, st, attnT, P);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" long long accflow_gma_aggregate_ws_bytes(int B, int D, int P) {
  const long long Kpad = (P + 31) / 32 * 32, CoutPad = (D + 127) / 128 * 128;
  // im2col route: split v and row scales per item, one k-table, and (single-item calls) up to 8 split-K partial outputs
  const long long a = B * (3 * Kpad * CoutPad * 2 + CoutPad * 4) + Kpad * 16 + 16 + (B == 1 ? 8LL * D * P * 4 : 0);
  // LDS-patch route (B == 1, f16x3): v in the patch layout, row scales, split-K partials
  const long long b = B == 1 ? accflow_conv_patch_elems(D, P, 1, 1) * 2 + CoutPad * 4 + 8LL * D * P * 4 : 0;
  return a > b ? a : b;
}

// GMA aggregation (gma/modules.py:102-115) as B independent 1x1 convolutions on the split-bf16 matrix cores:
// out[b][d][i] = fmap[b][d][i] + gamma * sum_j v[b][d][j] * attnT[b][j][i].  The TRANSPOSED attention (j-major) is
// exactly a (1, P channels, h, w) activation tensor, v[b] the (D x P) weight matrix (re-split every call, gamma folded
// in), and the residual add is the conv's accumulate epilogue.  ws as accflow_corr_volume_ws_bytes-style scratch:
// 3*Kpad*CoutPad uint16 + Kpad int4.
static int gma_aggregate_conv(const float* attnT, const float* v, const float* fmap, const float* gamma, float* out,
                              long long out_bs, void* ws, int mode, int* guard, int B, int D, int H, int W, hipStream_t st) {
  const int P = H * W;
  const int Kpad = accflow_conv_kpad(P, 1, 1), CoutPad = accflow_conv_coutpad(D);
  if (mode == ACCFLOW_CONV_F16X3 && B == 1 && P >= 16) {
    // one item (or a stacked run of items that share the attention): the LDS-patch kernel (about twice the im2col
    // kernel's rate) with v * gamma packed as its fp16 weights; split-K fills the chip (115 pixel tiles at 720x1280)
    unsigned short* wpatch16 = reinterpret_cast<unsigned short*>(ws);
    float* wscale16 = reinterpret_cast<float*>(wpatch16 + accflow_conv_patch_elems(D, P, 1, 1));
    float* kws = wscale16 + CoutPad;
    accflow_pack_row_scale16(v, nullptr, D, P, CoutPad, 1, wscale16, gamma, st);
    accflow_pack_patch(v, nullptr, D, P, 1, CoutPad, wpatch16, 1, wscale16, 2, gamma, st);
    accflow_conv_desc d = {};
    d.in0 = attnT; d.in0_bs = (long long)P * P; d.C0 = P;
    d.B = 1; d.H = H; d.W = W; d.OH = H; d.OW = W; d.KH = 1; d.KW = 1; d.stride = 1;
    d.Cout = D; d.Kpad = Kpad; d.CoutPad = CoutPad;
    d.out = out; d.out_bs = out_bs;
    d.act = ACCFLOW_ACT_NONE; d.epi = ACCFLOW_EPI_ACCUM; d.e0 = fmap; d.e0_bs = (long long)D * P;
    d.wpatch = wpatch16; d.wpatch16 = wpatch16; d.wscale16 = wscale16; d.mode = mode; d.guard = guard;
    d.kws = kws; d.kws_elems = 8LL * D * P;
    conv_plan p;
    if (conv_plan_direct(d, D > 64 ? 2 : 1, false, p)) return 1;
    return accflow_launch_conv_direct(d, p, st);
  }
  // the im2col route packs v as split terms only: accflow_conv2d_f32 would hand <= 32 rows to the fp32 kernels, which read
  // the pack as fp32 (the estimator's D is 128)
  if (D <= 32) return 1;
  unsigned short* wsplit = reinterpret_cast<unsigned short*>(ws);
  int* ktab = reinterpret_cast<int*>(wsplit + 3LL * Kpad * CoutPad * B);
  float* wscale16 = reinterpret_cast<float*>(reinterpret_cast<char*>(ktab) + (long long)Kpad * 16);  // [B][CoutPad]
  float* kws = wscale16 + (((long long)B * CoutPad + 3) & ~3LL);   // B == 1: 8 * D * P floats of split-K partials
  accflow_pack_ktab_1x1(P, Kpad, ktab, st);
  // f16x3: v[b] * gamma as fp16 hi + lo with per-row (and per-pair) power-of-two scales; the attention (values in
  // [0, 1]) is split by the kernel with the usual 2^ACCFLOW_F16_ASHIFT.  Half the MFMAs of the bf16x6 form.
  const bool f16 = mode == ACCFLOW_CONV_F16X3 && (P % 64) == 0;
  if (mode == ACCFLOW_CONV_F16X3 && !f16) mode = ACCFLOW_CONV_BF16X6;
  if (f16) accflow_pack_row_scale16(v, nullptr, D, P, CoutPad, B, wscale16, gamma, st);
  accflow_pack_bf16s(v, nullptr, D, P, 1, 1, Kpad, CoutPad, B, wsplit, 0, 1.0f, gamma, f16 ? wscale16 : nullptr, st);
  accflow_conv_desc d = {};
  d.in0 = attnT; d.in0_bs = (long long)P * P; d.C0 = P; d.C1 = 0;
  d.B = B; d.H = H; d.W = W; d.OH = H; d.OW = W; d.KH = 1; d.KW = 1; d.stride = 1;
  d.Cout = D; d.wpack = reinterpret_cast<const float*>(wsplit); d.ktab = ktab; d.Kpad = Kpad; d.CoutPad = CoutPad;
  d.out = out; d.out_bs = out_bs;
  d.act = ACCFLOW_ACT_NONE; d.epi = ACCFLOW_EPI_ACCUM; d.e0 = fmap; d.e0_bs = (long long)D * P;
  d.wsplit = wsplit; d.wsplit_bs = 3LL * Kpad * CoutPad * 2; d.mode = mode;
  if (f16) { d.wsplit16 = wsplit; d.wscale16 = wscale16; d.guard = guard; }
  if (B == 1) { d.kws = kws; d.kws_elems = 8LL * D * P; }
  if (P % 64 == 0) {  // 64-pixel tiles never straddle two pairs: as few launches as 32-bit buffer offsets allow
    const long long per_pair = (long long)P * P * 4;
    const int chunk = (int)(((1LL << 32) - 1) / per_pair);
    if (chunk < 1) return 1;
    for (int b0 = 0; b0 < B; b0 += chunk) {
      accflow_conv_desc e = d;
      e.B = B - b0 < chunk ? B - b0 : chunk;
      e.in0 = attnT + (long long)b0 * P * P; e.out = out + (long long)b0 * out_bs; e.e0 = fmap + (long long)b0 * D * P;
      e.wsplit = wsplit + 3LL * Kpad * CoutPad * b0;
      if (f16) { e.wsplit16 = e.wsplit; e.wscale16 = wscale16 + (long long)b0 * CoutPad; }
      const int rc = accflow_conv2d_f32(&e, st);
      if (rc) return rc;
    }
    return 0;
  }
  for (int b = 0; b < B; ++b) {                           // ragged sizes: one launch per pair
    accflow_conv_desc e = d;
    e.B = 1; e.in0 = attnT + (long long)b * P * P; e.out = out + (long long)b * out_bs; e.e0 = fmap + (long long)b * D * P;
    e.wsplit = wsplit + 3LL * Kpad * CoutPad * b; e.wsplit_bs = 0;
    const int rc = accflow_conv2d_f32(&e, st);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int accflow_gma_aggregate_t_f32(const float* attnT, const float* v, const float* fmap, const float* gamma,
                                           float* out, long long out_bs, void* ws, int mode, int* guard, int B, int D,
                                           int H, int W, void* stream) {
  if (!attnT || !v || !fmap || !gamma || !out || !ws || B <= 0 || D <= 0 || H <= 0 || W <= 0) return 1;
  if (mode == ACCFLOW_CONV_F32) return 1;  // the fp32 path is accflow_gma_aggregate_f32 on the i-major attention
  return gma_aggregate_conv(attnT, v, fmap, gamma, out, out_bs, ws, mode, guard, B, D, H, W, as_stream(stream));
}

extern "C" long long accflow_gma_aggregate_s16_ws_bytes(int n, int D, int P) {
  const long long CoutPad = ((long long)n * D + 127) / 128 * 128;
  return accflow_conv_patch_elems(n * D, P, 1, 1) * 2 + CoutPad * 4 + 8LL * n * D * P * 4;
}

// GMA aggregation on the pre-split attention (accflow_gma_attention_s16): ONE GEMM for the n batch items that share an
// attention matrix - rows = the n x D channels of v * gamma (packed per call as fp16 weights with their row scales), the
// S16 attention as the activation operand through the direct kernel's DMA loader (no split in the K loop: the matrix is
// constant over the refinement iterations), split-K over the P = h*w deep reduction - whose epilogue reads each item's
// residual and writes each item's slice (fp32 and / or S16) through the channel-block scatter: no copies around it.
static int gma_aggregate_s16_impl(const void* attn16, const float* v, const float* fmap, long long fmap_bs, const float* gamma,
                                  float* out, long long out_bs, void* out16, long long out16_bs, void* ws, int* guard, int n,
                                  int D, int H, int W, hipStream_t st) {
  const int P = H * W, Cout = n * D;
  const int Kpad = accflow_conv_kpad(P, 1, 1), CoutPad = accflow_conv_coutpad(Cout);
  unsigned short* wpatch16 = reinterpret_cast<unsigned short*>(ws);
  float* wscale16 = reinterpret_cast<float*>(wpatch16 + accflow_conv_patch_elems(Cout, P, 1, 1));
  float* kws = wscale16 + CoutPad;
  accflow_pack_rows16(v, Cout, P, CoutPad, wpatch16, wscale16, gamma, st);
  accflow_conv_desc d = {};
  d.in0 = reinterpret_cast<const float*>(attn16); d.in0_bs = accflow_s16_item_words(P, H, W); d.C0 = P; d.in_fmt = 1;
  d.B = 1; d.H = H; d.W = W; d.OH = H; d.OW = W; d.KH = 1; d.KW = 1; d.stride = 1;
  d.Cout = Cout; d.Kpad = Kpad; d.CoutPad = CoutPad;
  d.out = out; d.out_bs = (long long)n * out_bs;
  d.out16 = out16; d.out16_bs = (long long)n * out16_bs;
  d.act = ACCFLOW_ACT_NONE; d.epi = ACCFLOW_EPI_ACCUM; d.e0 = fmap; d.e0_bs = (long long)n * fmap_bs;
  d.cb = D; d.out_cbs = out_bs; d.e0_cbs = fmap_bs; d.out16_cbs = out16_bs;
  d.wpatch = wpatch16; d.wpatch16 = wpatch16; d.wscale16 = wscale16; d.mode = ACCFLOW_CONV_F16X3; d.guard = guard;
  d.kws = kws; d.kws_elems = 8LL * Cout * P;
  conv_plan p;
  if (conv_plan_direct(d, Cout > 64 ? 2 : 1, false, p)) return 1;
  return accflow_launch_conv_direct(d, p, st);
}

extern "C" int accflow_gma_aggregate_s16(const void* attn16, const float* v, const float* fmap, long long fmap_bs,
                                         const float* gamma, float* out, long long out_bs, void* out16, long long out16_bs,
                                         void* ws, int* guard, int n, int D, int H, int W, void* stream) {
  if (!attn16 || !v || !fmap || !gamma || (!out && !out16) || !ws || n <= 0 || D <= 0 || (D & 31) || H <= 0 || W <= 0) return 1;
  return gma_aggregate_s16_impl(attn16, v, fmap, fmap_bs, gamma, out, out_bs, out16, out16_bs, ws, guard, n, D, H, W,
                                as_stream(stream));
}

// GMA attention -> S16 (gma_attn_gemm_kernel, gma_attn.hip): q and k are packed as fp16 hi / lo of x * 2^ASHIFT (k
// carries GMA's scale dim_head^-1/2), two passes of the register-only GEMM per item.
// ws: accflow_gma_attention_s16_ws_bytes(D, H, W) = two packs + partial / final column statistics.
extern "C" long long accflow_gma_attention_s16_ws_bytes(int D, int H, int W) {
  const long long P = (long long)H * W, Ppad = accflow_conv_coutpad((int)P), nb = (P + 127) / 128;
  return 2 * (2LL * (D / 8) * Ppad * 16) + (nb * P * 2 + P * 2) * 4 + 256;
}

extern "C" int accflow_gma_attention_s16(const float* qk, void* attn16, void* ws, int* guard, int B, int D, int H, int W,
                                         float scale, void* stream) {
  if (!qk || !attn16 || !ws || B <= 0 || D < 16 || (D % 16) || H <= 0 || W <= 0) return 1;
  const int P = H * W, Ppad = accflow_conv_coutpad(P), Kpad = accflow_conv_kpad(D, 1, 1);
  if (Kpad != D) return 1;
  hipStream_t st = as_stream(stream);
  const long long pack_bytes = 2LL * (D / 8) * Ppad * 16;
  char* kp = reinterpret_cast<char*>(ws);
  char* qp = kp + pack_bytes;
  float* part = reinterpret_cast<float*>(qp + pack_bytes);
  float* stats = part + (long long)cdiv(P, 128) * P * 2;
  const float fs = ldexpf(1.0f, ACCFLOW_F16_ASHIFT);
  const long long item = accflow_s16_item_words(P, H, W);
  for (int b = 0; b < B; ++b) {
    const float* q = qk + (long long)b * 2 * D * P;   // q = qk[:, :D], k = qk[:, D:] (modules.py:63)
    accflow_pack_kmajor(q + (long long)D * P, P, D, Kpad, Ppad, kp, scale * fs, 1, guard, st);
    accflow_pack_kmajor(q, P, D, Kpad, Ppad, qp, fs, 1, guard, st);
    const int rc = accflow_launch_gma_attn(kp, qp, part, stats, reinterpret_cast<unsigned*>(attn16) + b * item, 1.0f / (fs * fs),
                                           P, D, Ppad, st);
    if (rc) return rc;
  }
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_gma_attention_f32(const float* qk, float* attn, int B, int D, int P, float scale,
                                         void* stream) {
  if (!qk || !attn || B <= 0 || D <= 0 || P <= 0) return 1;
  hipStream_t st = as_stream(stream);
  // sim[b][i][j] = scale * <q[b][:, i], k[b][:, j]>, q = qk[:, :D], k = qk[:, D:]
  int rc = accflow_gemm_atb_f32(qk, qk + (long long)D * P, attn, P, P, D, 2LL * D * P, 2LL * D * P, (long long)P * P, B,
                                scale, st);
  if (rc) return rc;
  hipLaunchKernelGGL(row_softmax_kernel, dim3((unsigned)((long long)B * P)), dim3(256), 0, st, attn, P);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_gma_aggregate_f32(const float* attn, const float* v, const float* fmap, const float* gamma,
                                         float* out, long long out_bs, int B, int D, int P, void* stream) {
  if (!attn || !v || !fmap || !gamma || !out || B <= 0 || D <= 0 || P <= 0) return 1;
  dim3 grid(cdiv(P, 128), cdiv(D, 128), B);
  hipLaunchKernelGGL(gma_aggregate_kernel, grid, dim3(256), 0, as_stream(stream), attn, v, fmap, gamma, out, out_bs, D,
                     P);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
