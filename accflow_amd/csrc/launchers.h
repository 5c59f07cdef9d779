// Host-only prototypes of every function one translation unit defines and another calls (C++ linkage; the C ABI is
// include/accflow_hip.h).  No device code: gma.hip, gma_alt.hip, corr_volume.hip and corr_disp.hip include this without
// the convolution kernels' device header.  No .hip file declares a function of another unit itself.
#pragma once
#include <hip/hip_runtime.h>
#include "accflow_hip.h"
#include "conv_plan.h"

// ---- kernel families: conv_plan.cpp turns a validated descriptor into a conv_plan; these execute it (they keep the grid
// arithmetic and the choice of the instantiation).  One translation unit each, so that they compile in parallel.
int accflow_launch_conv_f32(const accflow_conv_desc& d, int wc, int wp, int tc, int tp, hipStream_t st);   // conv2d_f32.hip
int accflow_launch_conv_bf16s(const accflow_conv_desc& d, int tc, int tp, int Z, hipStream_t st);          // conv2d_bf16s.hip
int accflow_launch_corr_disp_bf16s(const accflow_conv_desc& d, hipStream_t st);
int accflow_launch_conv_direct(const accflow_conv_desc& d, const conv_plan& p, hipStream_t st);            // conv2d_direct.hip
int conv_ksplit_reduce_launch(const accflow_conv_desc& d, int Z, hipStream_t st);                          // conv_ksplit.hip
int accflow_launch_corr_disp_direct(const accflow_conv_desc& d, hipStream_t st);                           // corr_gemm.hip
// gma_attn.hip
int accflow_launch_gma_attn(const void* kpack, const void* qpack, float* part, float* stats, void* out16, float acc_scale, int P,
                            int D, int Ppad, hipStream_t st);
int accflow_launch_gma_attn_stats(const void* kpack, const void* qpack, float* part, float* stats, float acc_scale, int P, int D,
                                  int Ppad, hipStream_t st);
int accflow_launch_conv_s16m(const accflow_conv_desc& d, const conv_plan& p, hipStream_t st);   // multi-source S16 kernel (conv2d_s16m.hip)
int accflow_launch_conv_stem(const accflow_conv_desc& d, hipStream_t st);                        // conv_stem.hip
int accflow_launch_conv_small(const accflow_conv_desc& d, const conv_plan& p, hipStream_t st);   // <= 4 output channels (conv_small.hip)

// ---- operand packs (conv_pack.hip): one launch each, the arguments are the kernel's
// K-major (K x Cout) matrix -> [term][Kpad/8][CoutPad][8]: three bf16 terms, or (f16) fp16 hi + lo with the range check
void accflow_pack_kmajor(const float* w, int Cout, int K, int Kpad, int CoutPad, void* ws, float cscale, int f16, int* guard,
                         hipStream_t st);
// wscale16 of B weight matrices (Cout x rowlen each, CoutPad scales each); gptr: a device scalar factor
void accflow_pack_row_scale16(const float* w, const float* scale, int Cout, int rowlen, int CoutPad, int B, float* wscale16,
                              const float* gptr, hipStream_t st);
// the LDS-patch layout [term][step][octet][CoutPad][8] (f16: row-scaled fp16 hi + lo by wscale16)
void accflow_pack_patch(const float* w, const float* scale, int Cout, int Cin, int T, int CoutPad, unsigned short* wp, int f16,
                        const float* wscale16, int octs, const float* gptr, hipStream_t st);
// B weight matrices -> the im2col layout [3][Kpad/8][CoutPad][8] each (wscale16: fp16 hi + lo instead of three bf16 terms)
void accflow_pack_bf16s(const float* w, const float* scale, int Cout, int Cin, int KH, int KW, int Kpad, int CoutPad, int B,
                        unsigned short* ws, int kmajor, float cscale, const float* gptr, const float* wscale16, hipStream_t st);
// row scale + patch pack of a 1x1 weight matrix in one launch
void accflow_pack_rows16(const float* w, int Cout, int Cin, int CoutPad, unsigned short* wp, float* wscale16, const float* gptr,
                         hipStream_t st);
// k-table of a 1x1 single-source convolution (Kpad int4 entries)
void accflow_pack_ktab_1x1(int Cin, int Kpad, int* ktab, hipStream_t st);

// ---- correlation and GEMM helpers
int accflow_gemm_atb_f32(const float* A, const float* Bm, float* C, int M, int N, int K, long long a_bs, long long b_bs,
                         long long c_bs, int batch, float scale, hipStream_t st);                            // corr_volume.hip
int accflow_corr_level0_bf16s(const float* fmap1, const float* fmap2, float* lvl0, void* ws, int B, int C, int H8, int W8,
                              int mode, int disp, int* guard, hipStream_t st, float* lvl1, int* lvl1_done);  // corr_volume.hip
int accflow_corr_disp_pool_from(const float* lvl0, float* lvl1, float* lvl2, float* lvl3, int B, int H8, int W8, int first,
                                hipStream_t st);                                                             // corr_disp.hip
