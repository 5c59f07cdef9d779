// Host side of the multi-source S16 convolution kernel (conv_s16m_kernel.h): the launch of a plan (validation, wave-layout
// choice and split-K: conv_plan.cpp) and its weight pack (accflow_conv_pack_multi16).
#include "conv_s16m_kernel.h"
#include "pack_terms.h"

namespace {

struct multi_pack_args {
  const float* w[ACCFLOW_CONV_MAX_SRC];
  int rowlen[ACCFLOW_CONV_MAX_SRC];
  int nsrc;
};

// wscale16[ch] = 2^-(k + ACCFLOW_F16_ASHIFT), k such that the row's largest |w * scale| over ALL sources * 2^k lies in
// [2^10, 2^11) (the packs' one row-scale rule, pack_terms.h): one workgroup per output channel
__global__ __launch_bounds__(256) void conv_row_scale_multi_kernel(const multi_pack_args a, const float* __restrict__ scale, int Cout,
                                                                   float* __restrict__ wscale16) {
  const int ch = blockIdx.x;
  float m = 0.0f;
  if (ch < Cout)
    for (int s = 0; s < a.nsrc; ++s)
      for (int j = threadIdx.x; j < a.rowlen[s]; j += 256) m = fmaxf(m, fabsf(a.w[s][(long long)ch * a.rowlen[s] + j]));
  m = pack_block_max256(m);
  if (threadIdx.x) return;
  if (ch < Cout && scale) m *= fabsf(scale[ch]);
  wscale16[ch] = pack_row_scale16(m);
}

// one source's steps [step0, step0 + ceil(C/16) * T) of the pack [term][step][2 octets][CoutPad][8]
__global__ __launch_bounds__(256) void conv_pack_multi16_kernel(const float* __restrict__ w, const float* __restrict__ scale, int Cout,
                                                                int C, int T, int CoutPad, long long per_term, long long step0,
                                                                unsigned short* __restrict__ wp,
                                                                const float* __restrict__ wscale16) {
  const long long n = (long long)((C + 15) / 16) * T * 2 * CoutPad * 8;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const int q = (int)(idx & 7);
  long long r = idx >> 3;
  const int ch = (int)(r % CoutPad); r /= CoutPad;
  const int o = (int)(r & 1); r >>= 1;
  const int step = (int)r, g = step / T, tap = step - g * T;
  const int c = g * 16 + o * 8 + q;
  float val = 0.0f;
  if (c < C && ch < Cout) {
    val = w[((long long)ch * C + c) * T + tap];
    if (scale) val *= scale[ch];
  }
  const long long dst = step0 * 2 * CoutPad * 8 + idx;
  pack_store_f16x2z(wp + dst, per_term, val * pack_row_mul16(wscale16[ch]));
}

long long multi_steps(int nsrc, const int* C, const int* KH, const int* KW) {
  long long n = 0;
  for (int s = 0; s < nsrc; ++s) n += (long long)((C[s] + 15) / 16) * KH[s] * KW[s];
  return n;
}

// one launch of wave layout p.lay as planned (conv_plan.cpp)
int s16m_launch(const accflow_conv_desc& d, const conv_plan& p, hipStream_t st) {
  const s16m_layout& L = S16M_LAYOUTS[p.lay];
  const int tiles = cdiv(d.OW, S16M_TW) * cdiv(d.OH, L.TH);
  dim3 grid((unsigned)((long long)d.B * tiles), cdiv(d.Cout, L.WC * L.TCW * 32), p.Z);
  const bool kt9 = p.loop == CONV_LOOP_TAP9;
  int rc;
  if (p.lay == 0) rc = accflow_s16m_launch_0(d, grid, st, kt9);
  else if (p.lay == 1) rc = accflow_s16m_launch_1(d, grid, st, kt9);
  else if (p.lay == 2) rc = accflow_s16m_launch_2(d, grid, st, kt9);
  else rc = accflow_s16m_launch_3(d, grid, st, kt9);
  if (rc) return rc;
  if (p.Z > 1) return conv_ksplit_reduce_launch(d, p.Z, st);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

}  // namespace

extern "C" long long accflow_conv_multi_pack_elems(int Cout, int nsrc, const int* C, const int* KH, const int* KW) {
  if (nsrc < 1 || nsrc > ACCFLOW_CONV_MAX_SRC || !C || !KH || !KW) return 0;
  return 3LL * multi_steps(nsrc, C, KH, KW) * 2 * accflow_conv_coutpad(Cout) * 8;
}

extern "C" int accflow_conv_pack_multi16(const float* const* w, const float* scale, int Cout, int nsrc, const int* C,
                                         const int* KH, const int* KW, void* wpatch16, float* wscale16, void* stream) {
  if (!w || !C || !KH || !KW || !wpatch16 || !wscale16 || Cout <= 0 || nsrc < 1 || nsrc > ACCFLOW_CONV_MAX_SRC) return 1;
  multi_pack_args a;
  a.nsrc = nsrc;
  for (int s = 0; s < ACCFLOW_CONV_MAX_SRC; ++s) { a.w[s] = nullptr; a.rowlen[s] = 0; }
  for (int s = 0; s < nsrc; ++s) {
    if (!w[s] || C[s] <= 0 || KH[s] <= 0 || KW[s] <= 0) return 1;
    a.w[s] = w[s];
    a.rowlen[s] = C[s] * KH[s] * KW[s];
  }
  const int CoutPad = accflow_conv_coutpad(Cout);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(conv_row_scale_multi_kernel, dim3(CoutPad), dim3(256), 0, st, a, scale, Cout, wscale16);
  const long long per_term = multi_steps(nsrc, C, KH, KW) * 2 * CoutPad * 8;
  long long step0 = 0;
  for (int s = 0; s < nsrc; ++s) {
    const int T = KH[s] * KW[s];
    const long long n = (long long)((C[s] + 15) / 16) * T * 2 * CoutPad * 8;
    hipLaunchKernelGGL(conv_pack_multi16_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, w[s], scale, Cout, C[s], T, CoutPad,
                       per_term, step0, reinterpret_cast<unsigned short*>(wpatch16), wscale16);
    step0 += (long long)((C[s] + 15) / 16) * T;
  }
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

int accflow_launch_conv_s16m(const accflow_conv_desc& d, const conv_plan& p, hipStream_t st) {
  if (!p.ch0) return s16m_launch(d, p, st);
  // Cout = 128 m + 64: the 128 m channels on the 128-channel layout, the last 64 on a 64-channel one (conv_tail_ch0)
  accflow_conv_desc part[2];
  conv_tail_split(d, p.ch0, part[0], part[1]);
  for (int i = 0; i < 2; ++i) {
    conv_plan pp;
    int rc = conv_plan_part(part[i], p, i == 1, pp);
    if (!rc) rc = s16m_launch(part[i], pp, st);
    if (rc) return rc;
  }
  return 0;
}
