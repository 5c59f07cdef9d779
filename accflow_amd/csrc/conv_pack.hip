// Every weight and operand pack of the convolution kernels: the kernels, their C entry points (accflow_conv_pack_*) and the
// launch functions the other units pack through (launchers.h).  The numeric rules - row scale, term splits, k-table
// entry - are pack_terms.h's.
#include "conv_common.h"
#include "pack_terms.h"

namespace {

// weights for the patch kernel: [3 terms][nchunk*T steps][2 octets][CoutPad][8] bf16, element (t, step = cc*T + tap,
// o, ch, q) = term t of w[ch][cc*16 + o*8 + q][tap] (* scale[ch]), zero beyond Cin / Cout
// f16: two fp16 terms of val * 2^k[ch], the row scale recovered from wscale16[ch] = 2^-(k[ch] + ACCFLOW_F16_ASHIFT)
// octs: octets per channel chunk (2 = the direct kernel's 16-channel chunks)
__global__ void conv_pack_patch_kernel(const float* __restrict__ w, const float* __restrict__ scale, int Cout, int Cin,
                                       int T, int CoutPad, unsigned short* __restrict__ wp, int f16,
                                       const float* __restrict__ wscale16, int octs, const float* __restrict__ gptr) {
  const int nstep = (Cin + 8 * octs - 1) / (8 * octs) * T;
  const long long per_term = (long long)nstep * octs * CoutPad * 8;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= per_term) return;
  const int q = (int)(idx & 7);
  long long r = idx >> 3;
  const int ch = (int)(r % CoutPad); r /= CoutPad;
  const int o = (int)(r % octs); r /= octs;
  const int step = (int)r, cc = step / T, tap = step % T;
  const int c = cc * 8 * octs + o * 8 + q;
  float val = 0.0f;
  if (c < Cin && ch < Cout) {
    val = w[((long long)ch * Cin + c) * T + tap];
    if (scale) val *= scale[ch];
    if (gptr) val *= gptr[0];
  }
  if (f16) pack_store_f16x2z(wp + idx, per_term, val * pack_row_mul16(wscale16[ch]));
  else pack_store_bf16x3(wp + idx, per_term, val);
}

// w (OIHW fp32, optional per-channel scale) -> three bf16 terms [3][Kpad/8][CoutPad][8], k ordered (c, tap)
__global__ void conv_pack_bf16s_kernel(const float* __restrict__ w, const float* __restrict__ scale, int Cout, int Cin,
                                       int KH, int KW, int Kpad, int CoutPad, unsigned short* __restrict__ ws,
                                       int kmajor, float cscale, const float* __restrict__ gptr,
                                       const float* __restrict__ wscale16) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)Kpad * CoutPad) return;
  w += (long long)blockIdx.y * Cout * Cin * KH * KW;          // batched use: one weight matrix per blockIdx.y
  ws += (long long)blockIdx.y * 3 * Kpad * CoutPad;
  if (wscale16) wscale16 += (long long)blockIdx.y * CoutPad;
  const int k = (int)(idx / CoutPad), o = (int)(idx % CoutPad);
  const int T = KH * KW, K = Cin * T;
  float val = 0.0f;
  if (k < K && o < Cout) {
    const int c = k / T, t = k % T;
    val = kmajor ? w[(long long)k * Cout + o] : w[((long long)o * Cin + c) * T + t];
    if (scale) val *= scale[o];
    val *= cscale;
    if (gptr) val *= gptr[0];
  }
  const long long per_term = (long long)Kpad * CoutPad;
  const long long dst = ((long long)(k / 8) * CoutPad + o) * 8 + (k % 8);
  // wscale16: fp16 hi + lo of the row-scaled weight (third slot zero), see conv_pack_patch_kernel
  if (wscale16) pack_store_f16x2z(ws + dst, per_term, val * pack_row_mul16(wscale16[o]));
  else pack_store_bf16x3(ws + dst, per_term, val);
}

// The same pack for a K-MAJOR matrix (a feature map (C, P) used as weights: correlation level 0), one thread per
// (8 consecutive k, output column): coalesced reads along the columns and ONE 16-byte store per term (the generic
// kernel above writes 2-byte elements 16 bytes apart).  f16 != 0: fp16 hi + lo, the third slot is not written.
__global__ __launch_bounds__(256) void conv_pack_kmajor_kernel(const float* __restrict__ w, int Cout, int K, int Kpad,
                                                               int CoutPad, u32x4* __restrict__ ws, float cscale, int f16,
                                                               int* guard) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)(Kpad / 8) * CoutPad) return;
  const int k8 = (int)(idx / CoutPad), o = (int)(idx % CoutPad);
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = k8 * 8 + j;
    x[j] = (k < K && o < Cout) ? w[(long long)k * Cout + o] * cscale : 0.0f;
  }
  const long long per_term = (long long)(Kpad / 8) * CoutPad;
  if (f16) {
    u32x4 t2[2];
    bool bad = false;
    s16_split8(x, t2[0], t2[1], bad, 1.0f);  // (cscale already carries 2^ACCFLOW_F16_ASHIFT)
    if (bad && guard) atomicOr(guard, 1);
    ws[idx] = t2[0];
    ws[per_term + idx] = t2[1];
  } else {
    u32x4 t3[3];
    split8_bf16<3, 0>(x, t3);
#pragma unroll
    for (int t = 0; t < 3; ++t) ws[t * per_term + idx] = t3[t];
  }
}

// wscale16[ch] = 2^-(k + ACCFLOW_F16_ASHIFT) with k such that max_j |w[ch][j] * scale[ch]| * 2^k lies in [2^10, 2^11)
// (k = 0 for an all-zero / non-finite row, 0 for the padding channels): one workgroup per output channel
// (blockIdx.y: one weight matrix per batch item, gptr: a device scalar factor - the GMA aggregation's per-pair v * gamma)
__global__ __launch_bounds__(256) void conv_row_scale16_kernel(const float* __restrict__ w, const float* __restrict__ scale,
                                                               int Cout, int rowlen, float* __restrict__ wscale16,
                                                               const float* __restrict__ gptr) {
  const int ch = blockIdx.x;
  w += (long long)blockIdx.y * Cout * rowlen;
  wscale16 += (long long)blockIdx.y * gridDim.x;
  float m = 0.0f;
  if (ch < Cout)
    for (int j = threadIdx.x; j < rowlen; j += 256) m = fmaxf(m, fabsf(w[(long long)ch * rowlen + j]));
  m = pack_block_max256(m);
  if (threadIdx.x) return;
  if (ch < Cout && scale) m *= fabsf(scale[ch]);
  if (gptr) m *= fabsf(gptr[0]);
  wscale16[ch] = pack_row_scale16(m);
}

// conv_row_scale16_kernel + conv_pack_patch_kernel in ONE launch for 1x1 weight matrices that change every call (the GMA
// aggregation's v * gamma: 72 packs per sequence): one workgroup per output row - the row maximum, then that row's fp16
// hi / lo chunks in the patch layout [term][step][octet][CoutPad][8] (T = 1, 2 octets per step).
// Rows of up to ROWS16_REG * 2048 elements are read ONCE: every thread keeps its 8-element chunks (c8 = tid + 256 i) in
// registers between the maximum and the pack (the two-pass form read the 22 MB of a 3-item v twice: 31 us per launch, 72
// launches per C5 sequence); longer rows take the two-pass loop.
constexpr int ROWS16_REG = 8;
__global__ __launch_bounds__(256) void conv_pack_rows16_kernel(const float* __restrict__ w, int Cout, int Cin, int CoutPad,
                                                               unsigned short* __restrict__ wp, float* __restrict__ wscale16,
                                                               const float* __restrict__ gptr) {
  const int ch = blockIdx.x;
  const float gmul = gptr ? gptr[0] : 1.0f;
  const int nstep = (Cin + 15) / 16, nchunk = nstep * 2;
  const bool inreg = nchunk <= ROWS16_REG * 256 && !(Cin & 3);       // (rows start 16-byte aligned when Cin % 4 == 0)
  const float* row = w + (long long)ch * Cin;
  float keep[ROWS16_REG][8];
  float m = 0.0f;
  if (inreg) {
#pragma unroll
    for (int i = 0; i < ROWS16_REG; ++i) {
      const int c0 = (threadIdx.x + 256 * i) * 8;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = c0 + 4 * h;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (ch < Cout && c + 4 <= Cin) v = *reinterpret_cast<const f32x4*>(row + c);
        else if (ch < Cout) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = c + q < Cin ? row[c + q] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) { keep[i][4 * h + q] = v[q]; m = fmaxf(m, fabsf(v[q])); }
      }
    }
  } else if (ch < Cout) {
    for (int j = threadIdx.x; j < Cin; j += 256) m = fmaxf(m, fabsf(row[j]));
  }
  m = pack_block_max256(m) * fabsf(gmul);
  const float sc = pack_row_scale16(m);                        // the same value conv_row_scale16_kernel stores
  if (threadIdx.x == 0) wscale16[ch] = sc;
  const float mul = pack_row_mul16(sc);
  const long long per_term = (long long)nstep * 2 * CoutPad * 8;
  auto emit = [&](int c8, const float (&x)[8]) {              // one 8-channel chunk (step, octet) of this row
    u32x4 hv, lv;
    pack_hilo8(x, gmul, mul, hv, lv);
    const long long base = ((long long)c8 * CoutPad + ch) * 8;   // (16-byte aligned: one vector store per term)
    *reinterpret_cast<u32x4*>(wp + base) = hv;
    *reinterpret_cast<u32x4*>(wp + per_term + base) = lv;
  };
  if (inreg) {
#pragma unroll
    for (int i = 0; i < ROWS16_REG; ++i) {
      const int c8 = threadIdx.x + 256 * i;
      if (c8 < nchunk) emit(c8, keep[i]);
    }
    return;
  }
  for (int c8 = threadIdx.x; c8 < nchunk; c8 += 256) {
    float x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int c = c8 * 8 + q;
      x[q] = (c < Cin && ch < Cout) ? row[c] : 0.0f;
    }
    emit(c8, x);
  }
}

__global__ void conv_pack_kernel(const float* __restrict__ w, const float* __restrict__ scale, int Cout,
                                 int Cin, int KH, int KW, int C0, int tap_major, int Kpad, int CoutPad,
                                 float* __restrict__ wpack, int4* __restrict__ ktab) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)Kpad * CoutPad) return;
  const int k = (int)(idx / CoutPad), o = (int)(idx % CoutPad);
  const int T = KH * KW, K = Cin * T;
  int c = 0, t = 0;
  if (k < K) {
    if (tap_major) { t = k / Cin; c = k % Cin; } else { c = k / T; t = k % T; }
  }
  const int ky = t / KW, kx = t % KW;
  float val = 0.0f;
  if (k < K && o < Cout) {
    val = w[(((long long)o * Cin + c) * KH + ky) * KW + kx];
    if (scale) val *= scale[o];
  }
  wpack[idx] = val;
  if (o == 0) ktab[k] = pack_ktab_entry(k < K, c, ky, kx, C0);
}

// Every pack of one convolution in ONE launch (accflow_conv_pack_all_f32): what accflow_conv_pack_f32, _pack_bf16s, _pack_patch,
// _pack_patch16 and _pack_split16 write with up to seven launches - a training step rebuilds the packs of ~40 trainable
// convolutions and of their transposed forms after every optimizer step, 570 launches of ~5 us inside the step's graph.  One
// workgroup per output row: the row's largest magnitude (the fp16 packs' power-of-two scale, conv_row_scale16_kernel's value),
// then the row's elements in the im2col order (wpack, ktab, wsplit, wsplit16) and in the patch order (wpatch, wpatch16); every
// value goes through the functions the single-purpose kernels above use, so the packs are bit-identical to theirs.
// tflip: `w` is the (Cin, Cout, KH, KW) weight of the FORWARD convolution and the logical weight is its transposed, flipped
// form  W[o][c][ky][kx] = w[c][o][KH-1-ky][KW-1-kx]  - the input-gradient convolution's weights without materialising them.
__global__ __launch_bounds__(256) void conv_pack_all_kernel(const float* __restrict__ w, const float* __restrict__ scale, int Cout,
                                                            int Cin, int KH, int KW, int C0, int tap_major, int tflip, int Kpad,
                                                            int CoutPad, float* __restrict__ wpack, int4* __restrict__ ktab,
                                                            unsigned short* __restrict__ wsplit, unsigned short* __restrict__ wpatch,
                                                            unsigned short* __restrict__ wpatch16, float* __restrict__ wscale16,
                                                            unsigned short* __restrict__ wsplit16) {
  const int ch = blockIdx.x, T = KH * KW, K = Cin * T;
  auto wat = [&](int c, int t) -> float {     // logical w[ch][c][tap t]
    if (!tflip) return w[((long long)ch * Cin + c) * T + t];
    const int ky = t / KW, kx = t - ky * KW;
    return w[(((long long)c * Cout + ch) * KH + (KH - 1 - ky)) * KW + (KW - 1 - kx)];
  };
  float rscale = 1.0f;    // 2^-ASHIFT / wscale16[ch]
  if (wscale16) {
    float m = 0.0f;
    if (ch < Cout)
      for (int j = threadIdx.x; j < K; j += 256) m = fmaxf(m, fabsf(wat(j / T, j % T)));
    m = pack_block_max256(m);
    if (ch < Cout && scale) m *= fabsf(scale[ch]);
    const float ws = pack_row_scale16(m);
    if (threadIdx.x == 0) wscale16[ch] = ws;
    rscale = pack_row_mul16(ws);
  }
  const float sc = (scale && ch < Cout) ? scale[ch] : 1.0f;
  const bool has_sc = scale != nullptr;
  // ---- im2col order: k = (c, tap) (tap_major: (tap, c)), Kpad entries ----
  const long long per_term = (long long)Kpad * CoutPad;
  for (int k = threadIdx.x; k < Kpad; k += 256) {
    int c = 0, t = 0;
    if (k < K) {
      if (tap_major) { t = k / Cin; c = k % Cin; } else { c = k / T; t = k % T; }
    }
    float val = 0.0f;
    if (k < K && ch < Cout) {
      val = wat(c, t);
      if (has_sc) val *= sc;
    }
    wpack[(long long)k * CoutPad + ch] = val;
    if (ch == 0) ktab[k] = pack_ktab_entry(k < K, c, t / KW, t % KW, C0);
    if (wsplit || wsplit16) {     // (never tap_major: k = c * T + t) - conv_pack_bf16s_kernel's value: * scale, * cscale (= 1)
      float v2 = 0.0f;
      if (k < K && ch < Cout) {
        v2 = wat(k / T, k % T);
        if (has_sc) v2 *= sc;
        v2 *= 1.0f;
      }
      const long long dst = ((long long)(k / 8) * CoutPad + ch) * 8 + (k % 8);
      if (wsplit) pack_store_bf16x3(wsplit + dst, per_term, v2);
      if (wsplit16) pack_store_f16x2z(wsplit16 + dst, per_term, v2 * rscale);
    }
  }
  // ---- patch order: (16-channel chunk, tap) steps, 2 octets ----
  if (wpatch || wpatch16) {
    const int nstep = (Cin + 15) / 16 * T;
    const long long pterm = (long long)nstep * 2 * CoutPad * 8;
    for (int i = threadIdx.x; i < nstep * 16; i += 256) {
      const int q = i & 7, o = (i >> 3) & 1, step = i >> 4;
      const int cc = step / T, tap = step % T;
      const int c = cc * 16 + o * 8 + q;
      float val = 0.0f;
      if (c < Cin && ch < Cout) {
        val = wat(c, tap);
        if (has_sc) val *= sc;
      }
      const long long idx = (((long long)step * 2 + o) * CoutPad + ch) * 8 + q;
      if (wpatch) pack_store_bf16x3(wpatch + idx, pterm, val);
      if (wpatch16) pack_store_f16x2z(wpatch16 + idx, pterm, val * rscale);
    }
  }
}

// k-table of a 1x1, single-source conv: entry k = {channel k, 0, 0, source 0}; padding entries never in range
__global__ void conv_ktab_kernel(int Cin, int Kpad, int4* __restrict__ ktab) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= Kpad) return;
  ktab[k] = pack_ktab_entry(k < Cin, k, 0, 0, Cin);
}

}  // namespace

void accflow_pack_kmajor(const float* w, int Cout, int K, int Kpad, int CoutPad, void* ws, float cscale, int f16, int* guard,
                         hipStream_t st) {
  const long long n8 = (long long)(Kpad / 8) * CoutPad;
  hipLaunchKernelGGL(conv_pack_kmajor_kernel, dim3(cdiv(n8, 256)), dim3(256), 0, st, w, Cout, K, Kpad, CoutPad,
                     reinterpret_cast<u32x4*>(ws), cscale, f16, guard);
}

void accflow_pack_row_scale16(const float* w, const float* scale, int Cout, int rowlen, int CoutPad, int B, float* wscale16,
                              const float* gptr, hipStream_t st) {
  hipLaunchKernelGGL(conv_row_scale16_kernel, dim3(CoutPad, B), dim3(256), 0, st, w, scale, Cout, rowlen, wscale16, gptr);
}

void accflow_pack_patch(const float* w, const float* scale, int Cout, int Cin, int T, int CoutPad, unsigned short* wp, int f16,
                        const float* wscale16, int octs, const float* gptr, hipStream_t st) {
  const long long n = (long long)((Cin + 8 * octs - 1) / (8 * octs)) * T * octs * CoutPad * 8;
  hipLaunchKernelGGL(conv_pack_patch_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, w, scale, Cout, Cin, T, CoutPad, wp, f16,
                     wscale16, octs, gptr);
}

void accflow_pack_bf16s(const float* w, const float* scale, int Cout, int Cin, int KH, int KW, int Kpad, int CoutPad, int B,
                        unsigned short* ws, int kmajor, float cscale, const float* gptr, const float* wscale16, hipStream_t st) {
  const long long n = (long long)Kpad * CoutPad;
  hipLaunchKernelGGL(conv_pack_bf16s_kernel, dim3(cdiv(n, 256), B), dim3(256), 0, st, w, scale, Cout, Cin, KH, KW, Kpad,
                     CoutPad, ws, kmajor, cscale, gptr, wscale16);
}

void accflow_pack_rows16(const float* w, int Cout, int Cin, int CoutPad, unsigned short* wp, float* wscale16, const float* gptr,
                         hipStream_t st) {
  hipLaunchKernelGGL(conv_pack_rows16_kernel, dim3(CoutPad), dim3(256), 0, st, w, Cout, Cin, CoutPad, wp, wscale16, gptr);
}

void accflow_pack_ktab_1x1(int Cin, int Kpad, int* ktab, hipStream_t st) {
  hipLaunchKernelGGL(conv_ktab_kernel, dim3(cdiv(Kpad, 256)), dim3(256), 0, st, Cin, Kpad, reinterpret_cast<int4*>(ktab));
}

extern "C" long long accflow_conv_patch_elems(int Cout, int Cin, int KH, int KW) {
  return 3LL * ((Cin + 15) / 16) * KH * KW * 2 * accflow_conv_coutpad(Cout) * 8;
}

extern "C" int accflow_conv_pack_patch(const float* w, const float* scale, int Cout, int Cin, int KH, int KW,
                                       void* wpatch, void* stream) {
  if (!w || !wpatch || Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0) return 1;
  accflow_pack_patch(w, scale, Cout, Cin, KH * KW, accflow_conv_coutpad(Cout), reinterpret_cast<unsigned short*>(wpatch), 0,
                     nullptr, 2, nullptr, as_stream(stream));
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_conv_pack_patch16(const float* w, const float* scale, int Cout, int Cin, int KH, int KW,
                                         void* wpatch16, float* wscale16, void* stream) {
  if (!w || !wpatch16 || !wscale16 || Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0) return 1;
  const int CoutPad = accflow_conv_coutpad(Cout);
  accflow_pack_row_scale16(w, scale, Cout, Cin * KH * KW, CoutPad, 1, wscale16, nullptr, as_stream(stream));
  accflow_pack_patch(w, scale, Cout, Cin, KH * KW, CoutPad, reinterpret_cast<unsigned short*>(wpatch16), 1, wscale16, 2,
                     nullptr, as_stream(stream));
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_conv_pack_split16(const float* w, const float* scale, int Cout, int Cin, int KH, int KW,
                                         void* wsplit16, float* wscale16, void* stream) {
  if (!w || !wsplit16 || !wscale16 || Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0) return 1;
  const int Kpad = accflow_conv_kpad(Cin, KH, KW), CoutPad = accflow_conv_coutpad(Cout);
  accflow_pack_row_scale16(w, scale, Cout, Cin * KH * KW, CoutPad, 1, wscale16, nullptr, as_stream(stream));
  accflow_pack_bf16s(w, scale, Cout, Cin, KH, KW, Kpad, CoutPad, 1, reinterpret_cast<unsigned short*>(wsplit16), 0, 1.0f,
                     nullptr, wscale16, as_stream(stream));
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_conv_pack_bf16s(const float* w, const float* scale, int Cout, int Cin, int KH, int KW,
                                       void* wsplit, void* stream) {
  if (!w || !wsplit || Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0) return 1;
  const int Kpad = accflow_conv_kpad(Cin, KH, KW), CoutPad = accflow_conv_coutpad(Cout);
  accflow_pack_bf16s(w, scale, Cout, Cin, KH, KW, Kpad, CoutPad, 1, reinterpret_cast<unsigned short*>(wsplit), 0, 1.0f, nullptr,
                     nullptr, as_stream(stream));
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_conv_pack_f32(const float* w, const float* scale, int Cout, int Cin, int KH, int KW,
                                     int C0, int tap_major, float* wpack, int* ktab, void* stream) {
  if (!w || !wpack || !ktab || Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0) return 1;
  const int Kpad = accflow_conv_kpad(Cin, KH, KW), CoutPad = accflow_conv_coutpad(Cout);
  const long long n = (long long)Kpad * CoutPad;
  hipLaunchKernelGGL(conv_pack_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), w, scale, Cout,
                     Cin, KH, KW, C0, tap_major, Kpad, CoutPad, wpack, reinterpret_cast<int4*>(ktab));
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_conv_pack_all_f32(const float* w, const float* scale, int Cout, int Cin, int KH, int KW, int C0, int tap_major,
                                         int transpose_flip, float* wpack, int* ktab, void* wsplit, void* wpatch, void* wpatch16,
                                         float* wscale16, void* wsplit16, void* stream) {
  if (!w || !wpack || !ktab || Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0) return 1;
  if ((wpatch16 || wsplit16) && !wscale16) return 1;
  if (tap_major && (wsplit || wpatch || wpatch16 || wsplit16)) return 1;      // (the matrix-core packs are (c, tap)-ordered)
  const int Kpad = accflow_conv_kpad(Cin, KH, KW), CoutPad = accflow_conv_coutpad(Cout);
  hipLaunchKernelGGL(conv_pack_all_kernel, dim3(CoutPad), dim3(256), 0, as_stream(stream), w, scale, Cout, Cin, KH, KW, C0, tap_major,
                     transpose_flip, Kpad, CoutPad, wpack, reinterpret_cast<int4*>(ktab), reinterpret_cast<unsigned short*>(wsplit),
                     reinterpret_cast<unsigned short*>(wpatch), reinterpret_cast<unsigned short*>(wpatch16), wscale16,
                     reinterpret_cast<unsigned short*>(wsplit16));
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
