// GMA attention with relative position embeddings (gma/modules.py:6-31, 62-68; heads = 1): args.position_only and
// args.position_and_content.  For query pixel i = (x, y) and key pixel j = (u, v) of the h x w grid, M = max_pos_size,
// q already multiplied by scale, Eh / Ew the embedding tables (2M-1, D):
//     sim_pos[i][j] = A[i][u] + Bw[i][v],   A[i][u] = <q_i, Eh[u - x + M - 1]>,   Bw[i][v] = <q_i, Ew[v - y + M - 1]>
// so the positional term is h + w dot products per query, not h * w.  pos_tables_kernel builds them once per image1
// (tab[b][u][i] = A, tab[b][h + v][i] = Bw: stored by query, the j-major softmax reads them coalesced), the softmax
// kernels add tab[u][i] + tab[h + v][i] to the content logit - or, position_only, take it as the whole logit: no score
// matrix and no QK GEMM (j-major: the separable form, softmax_u(A) softmax_v(Bw); row-major: the joint form).  The content
// scores come from the GEMMs accflow_gma_attention_t_f32 / _f32 use (gma.hip).
#include "common.h"
#include "launchers.h"

namespace {

__device__ __forceinline__ float pos_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float pos_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Tables, fp32 FMA on fp32 operands.  Workgroup = (item b, query row x, 64 queries y0.. of that row, 32 table rows r0.. of
// ONE table); thread = one query y and 8 table rows.  Height table: the 32 rows Eh[r - x + M - 1] are the same for every
// query of the row (a (D x w) by (D x 32) GEMM; the LDS reads of E are wave-wide broadcasts).  Width table: query y takes
// Ew[r - y + M - 1] - Toeplitz in (r, y) - so the tile stages the 32 + 63 embedding rows it touches and lane y reads row
// (r - r0) + 63 - y of them: neighbouring lanes are one padded row (33 words) apart, conflict-free.  Each dot product is
// computed once (no band of 2w - 1 rows is materialised).  The embedding rows are read from the weight as it is.
constexpr int PT_Y = 64, PT_R = 32, PT_D = 32, PT_E = PT_R + PT_Y - 1, PT_LD = PT_D + 1;

__global__ __launch_bounds__(256) void pos_tables_kernel(const float* __restrict__ qk, const float* __restrict__ rel_h,
                                                         const float* __restrict__ rel_w, float* __restrict__ tab, int D,
                                                         int H, int W, int M, float scale) {
  __shared__ float qs[PT_D][PT_Y];
  __shared__ float es[PT_E * PT_LD];
  const int tid = threadIdx.x, ly = tid & 63, rg = tid >> 6;
  const int P = H * W, ytiles = (W + PT_Y - 1) / PT_Y, nth = (H + PT_R - 1) / PT_R;
  const int x = blockIdx.x / ytiles, y0 = (blockIdx.x - x * ytiles) * PT_Y, b = blockIdx.z;
  const bool width = (int)blockIdx.y >= nth;
  const int r0 = (width ? (int)blockIdx.y - nth : (int)blockIdx.y) * PT_R, R = width ? W : H;
  const float* __restrict__ E = width ? rel_w : rel_h;
  // LDS row e holds embedding row ebase + e (rows outside the table - dead queries / dead table rows only - are zero)
  const int ne = width ? PT_E : PT_R;
  const int ebase = width ? r0 - (y0 + PT_Y - 1) + M - 1 : r0 - x + M - 1;
  const int eoff = (rg * 8 + (width ? PT_Y - 1 - ly : 0)) * PT_LD;
  const float* __restrict__ q = qk + (long long)b * 2 * D * P + (long long)x * W;
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.0f;
  for (int d0 = 0; d0 < D; d0 += PT_D) {
    for (int t = tid; t < PT_D * PT_Y; t += 256) {
      const int dd = t >> 6, yy = t & 63;
      qs[dd][yy] = (d0 + dd < D && y0 + yy < W) ? q[(long long)(d0 + dd) * P + y0 + yy] * scale : 0.0f;
    }
    for (int t = tid; t < ne * PT_D; t += 256) {
      const int e = t >> 5, dd = t & 31, row = ebase + e;
      es[e * PT_LD + dd] = (row >= 0 && row < 2 * M - 1 && d0 + dd < D) ? E[(long long)row * D + d0 + dd] : 0.0f;
    }
    __syncthreads();
    float part[8];      // (one partial sum per 32-deep chunk: the rounding error grows with the chunk, not with D)
#pragma unroll
    for (int k = 0; k < 8; ++k) part[k] = 0.0f;
#pragma unroll 8
    for (int dd = 0; dd < PT_D; ++dd) {
      const float qv = qs[dd][ly];
#pragma unroll
      for (int k = 0; k < 8; ++k) part[k] = fmaf(qv, es[eoff + k * PT_LD + dd], part[k]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] += part[k];
    __syncthreads();
  }
  if (y0 + ly >= W) return;
  float* __restrict__ t = tab + ((long long)b * (H + W) + (width ? H : 0)) * P + (long long)x * W + y0 + ly;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int r = r0 + rg * 8 + k;
    if (r < R) t[(long long)r * P] = acc[k];
  }
}

// Row-major softmax over j of score[i][j] + A[i][u] + Bw[i][v] (CONTENT; in place on the score matrix) or of the
// positional logit alone; one workgroup per query i, its h + w table entries staged in LDS (row_softmax_kernel's passes).
template <bool CONTENT>
__global__ __launch_bounds__(256) void row_softmax_pos_kernel(float* __restrict__ a, const float* __restrict__ tab, int H,
                                                              int W) {
  extern __shared__ __attribute__((aligned(16))) float ts[];   // h + w table entries, then 4 partials
  const int P = H * W, R = H + W;
  float* red = ts + R;
  const int b = blockIdx.x / P, i = blockIdx.x - b * P;
  float* row = a + (long long)blockIdx.x * P;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = threadIdx.x; r < R; r += 256) ts[r] = tab[((long long)b * R + r) * P + i];
  __syncthreads();
  auto logit = [&](int j) {
    const int u = j / W;
    return (CONTENT ? row[j] : 0.0f) + (ts[u] + ts[H + j - u * W]);
  };
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < P; j += 256) mx = fmaxf(mx, logit(j));
  mx = pos_wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float s = 0.0f;
  for (int j = threadIdx.x; j < P; j += 256) {
    const float e = expf(logit(j) - mx);
    row[j] = e;
    s += e;
  }
  s = pos_wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  s = (red[0] + red[1]) + (red[2] + red[3]);
  for (int j = threadIdx.x; j < P; j += 256) row[j] = row[j] / s;
}

// j-major softmax of position_and_content (col_softmax16_kernel's two sweeps: online max / sum with the 16 partial pairs
// of a column combined in a fixed order, then read-normalise-write) over score[j][i] + tab[u][i] + tab[h + v][i].  A wave
// takes whole octets of j (rows 8 o .. 8 o + 7, octets o = wave, wave + 16, ...), so that the normalising sweep can write
// the pre-split S16 layout directly (OUT16: per lane one 16-byte hi and one 16-byte lo store per octet, p *
// 2^ACCFLOW_F16_ASHIFT split as accflow_to_s16_f32 splits it, rows >= P of the last octet zero) - or fp32, j-major (out32:
// may be the score matrix itself, every element is read and written by the same lane).
template <bool OUT16>
__global__ __launch_bounds__(1024) void col_softmax_pos_kernel(const float* score, long long score_bs,
                                                               const float* __restrict__ tab, float* out32,
                                                               long long out32_bs, mu32x4* __restrict__ out16,
                                                               long long out16_bs, int H, int W) {
  __shared__ float redm[16][64], reds[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int P = H * W, NO = (P + 7) >> 3;
  const int i = blockIdx.x * 64 + lane;
  const bool live = i < P;
  const int b = blockIdx.y;
  const float* col = score + b * score_bs + (live ? i : 0);
  const float* th = tab + (long long)b * (H + W) * P + (live ? i : 0);
  const float* tw = th + (long long)H * P;
  auto logits = [&](int o, float (&x)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = o * 8 + u;
      if (live && j < P) {
        const int ju = j / W, jv = j - ju * W;
        x[u] = col[(long long)j * P] + (th[(long long)ju * P] + tw[(long long)jv * P]);
      } else {
        x[u] = -INFINITY;
      }
    }
  };
  float mx = -INFINITY, s = 0.0f;
  for (int o = wave; o < NO; o += 16) {
    float x[8];
    logits(o, x);
    float m2 = mx;
#pragma unroll
    for (int u = 0; u < 8; ++u) m2 = fmaxf(m2, x[u]);
    if (m2 > -INFINITY) {   // (a dead lane keeps s = 0)
      float t = 0.0f;
#pragma unroll
      for (int u = 0; u < 8; ++u) t += expf(x[u] - m2);
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
  if (!live) return;
  for (int o = wave; o < NO; o += 16) {
    float x[8];
    logits(o, x);
    float p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = o * 8 + u < P ? expf(x[u] - m) * inv : 0.0f;
    if (OUT16) {
      mu32x4 hi, lo;
      bool bad = false;   // (probabilities are <= 1: no range guard)
      s16_split8(p, hi, lo, bad);
      mu32x4* d = out16 + b * out16_bs + i;
      d[(long long)(o * 2 + 0) * P] = hi;
      d[(long long)(o * 2 + 1) * P] = lo;
    } else {
      float* d = out32 + b * out32_bs + i;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (o * 8 + u < P) d[(long long)(o * 8 + u) * P] = p[u];
    }
  }
}

// position_only, j-major: the softmax factorises, softmax_j(A[u] + Bw[v]) = softmax_u(A) softmax_v(Bw).
// tab_softmax_kernel normalises the two tables of ONE item over their rows (per query i; h + w values each) into the
// workspace - 16 waves per 64 queries, wave w takes rows w, w + 16, ..., the 16 partial maxima / sums meet in LDS in a
// fixed order -, pos_only_kernel writes the P x P products: one multiply per element, no exponential, store-bound.
__global__ __launch_bounds__(1024) void tab_softmax_kernel(const float* __restrict__ tab, float* __restrict__ nt, int H,
                                                           int W) {
  __shared__ float red[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int P = H * W, R = blockIdx.y ? W : H;
  const int i = blockIdx.x * 64 + lane;
  const bool live = i < P;
  const long long off = (long long)(blockIdx.y ? H : 0) * P + (live ? i : 0);
  const float* src = tab + off;
  float* dst = nt + off;
  float mx = -INFINITY;
  for (int r = wave; r < R; r += 16) mx = fmaxf(mx, live ? src[(long long)r * P] : 0.0f);
  red[wave][lane] = mx;
  __syncthreads();
  float m = -INFINITY;
#pragma unroll
  for (int w = 0; w < 16; ++w) m = fmaxf(m, red[w][lane]);     // (R >= 1: wave 0 always holds a finite maximum)
  __syncthreads();
  float s = 0.0f;
  for (int r = wave; r < R; r += 16) s += live ? expf(src[(long long)r * P] - m) : 0.0f;
  red[wave][lane] = s;
  __syncthreads();
  float tot = 0.0f;
#pragma unroll
  for (int w = 0; w < 16; ++w) tot += red[w][lane];
  const float inv = 1.0f / tot;
  if (!live) return;
  for (int r = wave; r < R; r += 16) dst[(long long)r * P] = expf(src[(long long)r * P] - m) * inv;
}

template <bool OUT16>
__global__ __launch_bounds__(1024) void pos_only_kernel(const float* __restrict__ nt, float* __restrict__ out32,
                                                        mu32x4* __restrict__ out16, int H, int W) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int P = H * W, NO = (P + 7) >> 3;
  const int i = blockIdx.x * 64 + lane;
  if (i >= P) return;
  const float* nh = nt + i;
  const float* nw = nh + (long long)H * P;
  for (int o = wave; o < NO; o += 16) {
    float p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = o * 8 + u;
      if (j < P) {
        const int ju = j / W, jv = j - ju * W;
        p[u] = nh[(long long)ju * P] * nw[(long long)jv * P];
      } else {
        p[u] = 0.0f;
      }
    }
    if (OUT16) {
      mu32x4 hi, lo;
      bool bad = false;
      s16_split8(p, hi, lo, bad);
      out16[(long long)(o * 2 + 0) * P + i] = hi;
      out16[(long long)(o * 2 + 1) * P + i] = lo;
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (o * 8 + u < P) out32[(long long)(o * 8 + u) * P + i] = p[u];
    }
  }
}

// scores, j-major: C[j][i] = scale * <k_j, q_i> for nb items - accflow_gma_attention_t_f32's two GEMM routes
int pos_scores_t(const float* qk, float* dst, void* ws, int mode, int nb, int D, int H, int W, float scale, hipStream_t st) {
  const int P = H * W;
  static const bool split_ok = [] { const char* e = getenv("ACCFLOW_GMA_QK_SPLIT"); return !e || atoi(e) != 0; }();
  if (split_ok && mode != ACCFLOW_CONV_F32 && ws && P > 32 && fabsf(scale * sqrtf((float)D) - 1.0f) < 1e-6f) {
    for (int b = 0; b < nb; ++b) {
      const float* q = qk + (long long)b * 2 * D * P;
      const int rc = accflow_corr_level0_bf16s(q + (long long)D * P, q, dst + (long long)b * P * P, ws, 1, D, H, W,
                                               ACCFLOW_CONV_BF16X6, 0, nullptr, st, nullptr, nullptr);
      if (rc) return rc;
    }
    return 0;
  }
  return accflow_gemm_atb_f32(qk + (long long)D * P, qk, dst, P, P, D, 2LL * D * P, 2LL * D * P, (long long)P * P, nb, scale,
                              st);
}

long long pos_split_ws_bytes(int D, int H, int W) { return (accflow_corr_volume_ws_bytes(D, H, W) + 255) & ~255LL; }

}  // namespace

extern "C" int accflow_gma_pos_tables_f32(const float* qk, const float* rel_height, const float* rel_width, float* tab,
                                          int B, int D, int H, int W, int max_pos, float scale, void* stream) {
  if (!qk || !rel_height || !rel_width || !tab || B <= 0 || D <= 0 || H <= 0 || W <= 0 || max_pos <= 0) return 1;
  if (H > max_pos || W > max_pos || B > 65535) return 1;   // (the embedding row u - x + max_pos - 1 would leave the table)
  const dim3 grid(H * cdiv(W, PT_Y), cdiv(H, PT_R) + cdiv(W, PT_R), B);
  hipLaunchKernelGGL(pos_tables_kernel, grid, dim3(256), 0, as_stream(stream), qk, rel_height, rel_width, tab, D, H, W,
                     max_pos, scale);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_gma_attention_pos_f32(const float* qk, const float* tab, float* attn, int content, int B, int D,
                                             int H, int W, float scale, void* stream) {
  if (!qk || !tab || !attn || (content != 0 && content != 1) || B <= 0 || D <= 0 || H <= 0 || W <= 0) return 1;
  const long long P = (long long)H * W, rows = (long long)B * P;
  const size_t lds = (size_t)(H + W + 4) * sizeof(float);
  if (rows > 0x7fffffffLL || lds > 60000) return 1;
  hipStream_t st = as_stream(stream);
  if (content) {
    const int rc = accflow_gemm_atb_f32(qk, qk + (long long)D * P, attn, (int)P, (int)P, D, 2LL * D * P, 2LL * D * P, P * P, B,
                                        scale, st);
    if (rc) return rc;
    hipLaunchKernelGGL(row_softmax_pos_kernel<true>, dim3((unsigned)rows), dim3(256), lds, st, attn, tab, H, W);
  } else {
    hipLaunchKernelGGL(row_softmax_pos_kernel<false>, dim3((unsigned)rows), dim3(256), lds, st, attn, tab, H, W);
  }
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" long long accflow_gma_attention_pos_ws_bytes(int D, int H, int W, int content, int s16) {
  if (D <= 0 || H <= 0 || W <= 0) return 0;
  if (!content) return (long long)(H + W) * H * W * 4;   // the normalised tables of one item
  return pos_split_ws_bytes(D, H, W) + (s16 ? (long long)H * W * H * W * 4 : 0);
}

extern "C" int accflow_gma_attention_pos_t(const float* qk, const float* tab, float* attnT, void* attn16, void* ws, int mode,
                                           int content, int B, int D, int H, int W, float scale, void* stream) {
  if (!qk || !tab || (!attnT) == (!attn16) || (content != 0 && content != 1) || B <= 0 || D <= 0 || H <= 0 || W <= 0) return 1;
  if (B > 65535 || ((attn16 || !content) && !ws)) return 1;
  const int P = H * W;
  hipStream_t st = as_stream(stream);
  const dim3 blocks(cdiv(P, 64), B), one(cdiv(P, 64), 1);
  const long long tab_bs = (long long)(H + W) * P, pp = (long long)P * P;
  const long long item16 = accflow_s16_item_words(P, H, W) / 4;     // 16-byte chunks per S16 item
  mu32x4* o16 = reinterpret_cast<mu32x4*>(attn16);
  if (!content) {   // the two tables of one item, normalised, live in the workspace (reused item after item)
    float* nt = reinterpret_cast<float*>(ws);
    for (int b = 0; b < B; ++b) {
      hipLaunchKernelGGL(tab_softmax_kernel, dim3(cdiv(P, 64), 2), dim3(1024), 0, st, tab + b * tab_bs, nt, H, W);
      if (attn16)
        hipLaunchKernelGGL(pos_only_kernel<true>, one, dim3(1024), 0, st, nt, nullptr, o16 + b * item16, H, W);
      else
        hipLaunchKernelGGL(pos_only_kernel<false>, one, dim3(1024), 0, st, nt, attnT + b * pp, nullptr, H, W);
    }
    ACCFLOW_RETURN_LAUNCH_STATUS();
  }
  if (!attn16) {
    const int rc = pos_scores_t(qk, attnT, ws, mode, B, D, H, W, scale, st);
    if (rc) return rc;
    hipLaunchKernelGGL(col_softmax_pos_kernel<false>, blocks, dim3(1024), 0, st, attnT, pp, tab, attnT, pp, nullptr, 0LL,
                       H, W);
    ACCFLOW_RETURN_LAUNCH_STATUS();
  }
  // S16 output: the fp32 scores of ONE item live in the workspace (behind the split GEMM's own), reused item after item
  float* sc = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + pos_split_ws_bytes(D, H, W));
  for (int b = 0; b < B; ++b) {
    const int rc = pos_scores_t(qk + (long long)b * 2 * D * P, sc, ws, mode, 1, D, H, W, scale, st);
    if (rc) return rc;
    hipLaunchKernelGGL(col_softmax_pos_kernel<true>, one, dim3(1024), 0, st, sc, 0LL, tab + b * tab_bs, nullptr, 0LL,
                       o16 + b * item16, 0LL, H, W);
  }
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
