// (-DACCFLOW_KPROF builds compile this body inside conv2d_direct.hip instead: the in-kernel stamp buffer is per translation unit)
#if !defined(ACCFLOW_KPROF) || defined(ACCFLOW_DIRECT_UNITY)
#include "conv2d_direct_kernel.h"

// Level 0 of the displaced correlation pyramid for one pair: E_0 = shear(F1^T F2 / sqrt(C)) with BOTH feature maps
// pre-split into [term][k/8][pixel][8] packs (d.wpatch / d.wpatch16 = fmap1 incl. the 1/sqrt(C) scale, d.in0 reused as
// the pack of fmap2), so that every MFMA fragment is one 16-byte buffer load straight from L2: no LDS, no barrier and no
// operand split in the K loop (the 1x1-convolution form of the direct kernel re-split the same fmap2 tile in each of
// the P/128 workgroups of a tile column and spent 2300 cycles per 16-deep step, 384 of them in its 12 MFMAs).
// Workgroup = 128 query pixels (rows) x 128 target pixels (columns): TWO image rows (2*yo, 2*yo + 1) x 64 columns
// (xc*64 ..), so that the tile holds whole 2x2 pooling cells and level 1 is emitted with level 0 (corr_disp_store2;
// d.out2 = this pair's level 1); LDS only for the displaced store.
template <int NT, bool F16>
__global__ __launch_bounds__(256, 2) void corr_disp_gemm_kernel(const accflow_conv_desc d) {
  constexpr int TC = 2, TP = 2;
  __shared__ __attribute__((aligned(16))) unsigned char smem[DISP2_LDS_BYTES];
#ifdef ACCFLOW_KPROF
  const unsigned long long tL0 = __builtin_amdgcn_s_memrealtime();
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wave >> 1, wp = wave & 1;
  const int l31 = lane & 31, kh = lane >> 5;
  const int P = d.OH * d.OW;
  // XCD-aware tile order.  Workgroups b and b + 8 share an XCD (and its 4 MB L2): XCD j owns the query-pixel blocks
  // j, j + 8, ... and walks the target tiles with its own query blocks innermost, so the ~96 workgroups an XCD runs
  // at a time share <= 8 A tiles and ~12 B tiles (128 KB each).  In plain row-major order every workgroup streamed
  // its 256 KB of operands from beyond L2: 920 MB of reads per pair for 236 MB of output, 178 us per pair.
  const int npb = (P + 127) >> 7, percol = (npb + 7) >> 3;
  const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
  const int pb = xcd + 8 * (seq % percol), qt = seq / percol;
  if (pb >= npb) return;
  const int ncx = (d.OW + 63) >> 6;
  const int yo = qt / ncx, xc = qt - yo * ncx;
  const int cblk0 = pb * 128;
  const int nstep = d.Kpad / 16;
  const long long step_bytes = 2LL * d.CoutPad * 16, term_bytes = (long long)(d.Kpad / 8) * d.CoutPad * 16;
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(F16 ? d.wpatch16 : d.wpatch), 0, (int)(unsigned)(3 * term_bytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(d.in0), 0, (int)(unsigned)(3 * term_bytes), 0x00020000);
  const unsigned avoff = (unsigned)((kh * d.CoutPad + cblk0 + wc * 64 + l31) * 16);
  // this wave's target pixels: row 2*yo + wp, columns xc*64 + i*32 + l31 (outside the image: masked, reads 0)
  unsigned bvoff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int y2 = 2 * yo + wp, x2 = xc * 64 + i * 32 + l31;
    bvoff[i] = (y2 < d.OH && x2 < d.OW) ? (unsigned)((kh * d.CoutPad + y2 * d.OW + x2) * 16) : 0xFFFFFFFFu;
  }
#define CG_LOAD(STEP, A, Bf)                                                                                     \
  _Pragma("unroll") for (int t = 0; t < NT; ++t) _Pragma("unroll") for (int i = 0; i < 2; ++i) {                 \
    const int so = (int)(unsigned)(t * term_bytes + (STEP) * step_bytes);                                        \
    A[t][i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(ra, (int)(avoff + i * 512), so, 0)); \
    Bf[t][i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rb, (int)bvoff[i], so, 0));      \
  }
  f32x16 acc[TC][TP];
#pragma unroll
  for (int tc = 0; tc < TC; ++tc)
#pragma unroll
    for (int tp = 0; tp < TP; ++tp)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tc][tp][r] = 0.0f;
  // fragments are requested PD steps ahead (an L2 round trip is longer than one 12-MFMA step): 2 with two terms
  // (three register sets, still 3 workgroups per CU), 1 with three terms
  constexpr int PD = NT == 2 ? 2 : 1;
  bf16x8 aA[NT][TC], bA[NT][TP], aB[NT][TC], bB[NT][TP], aC[NT][TC], bC[NT][TP];
  CG_LOAD(0, aA, bA);
  if (PD == 2 && nstep > 1) { CG_LOAD(1, aB, bB); }
#define CG_STEP(STEP, AC, BC, AN, BN)                                                                            \
  do {                                                                                                           \
    if ((STEP) + PD < nstep) { CG_LOAD((STEP) + PD, AN, BN); }                                                   \
    constexpr int NPAIR = NT == 3 ? 6 : 3;                                                                       \
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};                                        \
    _Pragma("unroll") for (int pr = 6 - NPAIR; pr < 6; ++pr) _Pragma("unroll") for (int tc = 0; tc < TC; ++tc)   \
        _Pragma("unroll") for (int tp = 0; tp < TP; ++tp) acc[tc][tp] =                                          \
            dir_mfma<F16>(AC[PA[pr]][tc], BC[PB[pr]][tp], acc[tc][tp]);                                          \
  } while (0)
  if constexpr (PD == 2) {
    for (int step = 0; step < nstep; step += 3) {
      CG_STEP(step, aA, bA, aC, bC);
      if (step + 1 < nstep) CG_STEP(step + 1, aB, bB, aA, bA);
      if (step + 2 < nstep) CG_STEP(step + 2, aC, bC, aB, bB);
    }
  } else {
    for (int step = 0; step < nstep; step += 2) {
      CG_STEP(step, aA, bA, aB, bB);
      if (step + 1 < nstep) CG_STEP(step + 1, aB, bB, aA, bA);
    }
  }
#undef CG_STEP
#undef CG_LOAD
#ifdef ACCFLOW_KPROF
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long tL1 = __builtin_amdgcn_s_memrealtime();
#endif
  corr_disp_store2(d, acc, reinterpret_cast<float*>(smem), reinterpret_cast<int*>(smem) + 64 * DISP_PITCH,
                   reinterpret_cast<float*>(smem + DISP_LDS_BYTES), d.out2, cblk0, yo, xc, wc, wp, lane, wave, tid);
#ifdef ACCFLOW_KPROF
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (tid == 0) {
    const int slot = (blockIdx.x & 4095) * 16;
    g_kprof[slot + 8] = tL1 - tL0;
    g_kprof[slot + 11] = __builtin_amdgcn_s_memrealtime() - tL0;
    g_kprof[slot + 10] = 1;
    g_kprof[slot + 14] = 0;
  }
#endif
}

// LDS-ring form of corr_disp_gemm_kernel (fp16 split, two terms).  The register-only loop above lets every wave pull its
// own A and B fragments from L2 - 8 KB per 12 MFMAs - and is bound by the vector memory pipe, not by the matrix cores or
// the stores (profiles/r03_corr_gemm_store_ab.txt).  Here each operand byte enters the CU once per WORKGROUP: a 16-deep
// step's A tile (128 query pixels) and B tile (2 image rows x 64 target pixels), 2 terms x 2 octets x 128 x 16 B = 8 KB
// each, are DMA'd (buffer_load_dwordx4 ... lds, 16 one-KB pieces per step, 4 per wave) into a 3-slot LDS ring two steps
// ahead; the waves read their fragments with conflict-free ds_read_b128 (32 lanes = 512 contiguous bytes).  Half the
// vector-memory traffic, none of it through VGPRs.  One barrier per step: it publishes step s (every wave has waited for
// ITS pieces with a counted vmcnt) and retires step s-1's reads, whose slot the DMA of step s+2 then overwrites.
// The ring memory is reused by the displaced store afterwards.
// (A 16-byte-store epilogue with a 2-slot ring and 4 workgroups per CU was built, measured and removed again: no faster -
// profiles/r03_corr_gemm_store_ab.txt; in-kernel stamps, tools/kprof_corr.py: K loop 13.8 us, store phase 8.5 us.)
constexpr int CRING_SLOT_CHUNKS = 2 * 2 * 2 * 128;   // [A|B][term][octet][128] 16-byte chunks
// measurement builds only (tools/corr_ablation.sh, -DACCFLOW_CORR_ABL=bits): 1 no B-fragment reads (A's registers reused),
// 2 no MFMAs, 4 no operand DMA (stale LDS), 8 no displaced store, 16 no A-fragment reads either
#ifndef ACCFLOW_CORR_ABL
#define ACCFLOW_CORR_ABL 0
#endif
__global__ __launch_bounds__(256, 2) void corr_disp_ring_kernel(const accflow_conv_desc d) {
  constexpr int TC = 2, TP = 2;
  constexpr int CRING_SLOTS = 3;
  constexpr int RING_BYTES = CRING_SLOTS * CRING_SLOT_CHUNKS * 16;
  constexpr int ST_BYTES = DISP2_LDS_BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char smem[RING_BYTES > ST_BYTES ? RING_BYTES : ST_BYTES];
  u32x4* ring = reinterpret_cast<u32x4*>(smem);
#ifdef ACCFLOW_KPROF
  const unsigned long long tL0 = __builtin_amdgcn_s_memrealtime();
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wave >> 1, wp = wave & 1;
  const int l31 = lane & 31, kh = lane >> 5;
  const int P = d.OH * d.OW;
  const int npb = (P + 127) >> 7, percol = (npb + 7) >> 3;
  const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
  const int pb = xcd + 8 * (seq % percol), qt = seq / percol;
  if (pb >= npb) return;
  const int ncx = (d.OW + 63) >> 6;
  const int yo = qt / ncx, xc = qt - yo * ncx;
  const int cblk0 = pb * 128;
  const int nstep = d.Kpad / 16;
  const unsigned oct_bytes = (unsigned)d.CoutPad * 16u, term_bytes = (unsigned)(d.Kpad / 8) * oct_bytes;
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(d.wpatch16), 0, (int)(2 * term_bytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.in0), 0, (int)(2 * term_bytes), 0x00020000);
  // DMA piece i of this wave: piece id = wave*4 + i -> operand (A: 0-7, B: 8-15), (term, octet) row, half of the 128 items
  unsigned pvoff[4];
  int prow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = wave * 4 + i;
    const int isb = id >> 3, row = (id >> 1) & 3, half = id & 1;
    prow[i] = row;
    if (!isb) {
      pvoff[i] = (unsigned)(cblk0 + half * 64 + lane) * 16u;       // (rows beyond P are zero in the pack)
    } else {
      const int y2 = 2 * yo + half, x2 = xc * 64 + lane;           // B: image row `half` of the tile
      pvoff[i] = (y2 < d.OH && x2 < d.OW) ? (unsigned)(y2 * d.OW + x2) * 16u : 0xFFFFFFFFu;
    }
  }
  auto issue = [&](int step) {
    const int slot = step % CRING_SLOTS;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = wave * 4 + i;
      const int isb = id >> 3, row = prow[i], half = id & 1;
      const int t = row >> 1, o = row & 1;
      const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)t * term_bytes + (unsigned)(2 * step + o) * oct_bytes));
      const int dst = __builtin_amdgcn_readfirstlane(slot * CRING_SLOT_CHUNKS + isb * 512 + row * 128 + half * 64);
      if (isb)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (__attribute__((address_space(3))) void*)&ring[dst], 16, (int)pvoff[i], (int)soff, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (__attribute__((address_space(3))) void*)&ring[dst], 16, (int)pvoff[i], (int)soff, 0, 0);
    }
  };
  f32x16 acc[TC][TP];
#pragma unroll
  for (int tc = 0; tc < TC; ++tc)
#pragma unroll
    for (int tp = 0; tp < TP; ++tp)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tc][tp][r] = 0.0f;
  constexpr int AHEAD = CRING_SLOTS - 1;        // steps of DMA in flight beyond the one being consumed
  issue(0);
  if (AHEAD > 1 && nstep > 1) issue(1);
  bf16x8 A[2][TC], Bf[2][TP];
  for (int step = 0; step < nstep; ++step) {
    // this wave's 4 pieces of `step` have landed once at most the pieces of the later steps are still in flight
    if (AHEAD > 1 && step + 1 < nstep) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (step + AHEAD < nstep && !(ACCFLOW_CORR_ABL & 4)) issue(step + AHEAD);   // into the slot whose reads (step - 1) every wave finished before the barrier
    const u32x4* sl = ring + (step % CRING_SLOTS) * CRING_SLOT_CHUNKS;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (!(ACCFLOW_CORR_ABL & 16) || step == 0) A[t][i] = __builtin_bit_cast(bf16x8, sl[(t * 2 + kh) * 128 + wc * 64 + i * 32 + l31]);
        if (ACCFLOW_CORR_ABL & 1) Bf[t][i] = A[t][i];
        else Bf[t][i] = __builtin_bit_cast(bf16x8, sl[512 + (t * 2 + kh) * 128 + wp * 64 + i * 32 + l31]);
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};
#pragma unroll
    for (int pr = 0; pr < 3; ++pr)
#pragma unroll
      for (int tc = 0; tc < TC; ++tc)
#pragma unroll
        for (int tp = 0; tp < TP; ++tp) {
          if (ACCFLOW_CORR_ABL & 2) acc[tc][tp][pr] += __builtin_bit_cast(float, __builtin_bit_cast(u32x4, A[PA[pr]][tc])[0] ^ __builtin_bit_cast(u32x4, Bf[PB[pr]][tp])[1]);
          else acc[tc][tp] = dir_mfma<true>(A[PA[pr]][tc], Bf[PB[pr]][tp], acc[tc][tp]);
        }
  }
  __syncthreads();   // the ring is dead: its memory becomes the displaced store's staging tile
  if ((ACCFLOW_CORR_ABL & 8) && acc[0][0][0] != 12345.678f) return;
#ifdef ACCFLOW_KPROF
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long tL1 = __builtin_amdgcn_s_memrealtime();
#endif
  corr_disp_store2(d, acc, reinterpret_cast<float*>(smem), reinterpret_cast<int*>(smem) + 64 * DISP_PITCH,
                   reinterpret_cast<float*>(smem + DISP_LDS_BYTES), d.out2, cblk0, yo, xc, wc, wp, lane, wave, tid);
#ifdef ACCFLOW_KPROF
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long tL2 = __builtin_amdgcn_s_memrealtime();   // store instructions issued
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (tid == 0) {
    const int slot = (blockIdx.x & 4095) * 16;
    g_kprof[slot + 8] = tL1 - tL0;
    g_kprof[slot + 9] = tL2 - tL1;
    g_kprof[slot + 11] = __builtin_amdgcn_s_memrealtime() - tL0;
    g_kprof[slot + 10] = 1;
  }
#endif
}

int accflow_launch_corr_disp_direct(const accflow_conv_desc& d, hipStream_t st) {
  const int P = d.OH * d.OW, npb = cdiv(P, 128);
  if (!d.out2) return 1;
  const int nqt = cdiv(d.OH, 2) * cdiv(d.OW, 64);  // target tiles: 2 rows x 64 columns
  dim3 grid(8 * ((npb + 7) / 8) * nqt);  // (XCD, its query blocks, target tiles): see the kernel
  // ACCFLOW_CORR_GEMM=regs: the register-only operand loop (A/B); default: the LDS-ring form
  static const bool ringk = [] { const char* e = getenv("ACCFLOW_CORR_GEMM"); return !(e && e[0] == 'r'); }();
  if (d.mode == ACCFLOW_CONV_F16X3 && d.wpatch16 && ringk) {
    hipLaunchKernelGGL(corr_disp_ring_kernel, grid, dim3(256), 0, st, d);
  } else if (d.mode == ACCFLOW_CONV_F16X3 && d.wpatch16) hipLaunchKernelGGL((corr_disp_gemm_kernel<2, true>), grid, dim3(256), 0, st, d);
  else if (d.mode == ACCFLOW_CONV_BF16X3) hipLaunchKernelGGL((corr_disp_gemm_kernel<2, false>), grid, dim3(256), 0, st, d);
  else hipLaunchKernelGGL((corr_disp_gemm_kernel<3, false>), grid, dim3(256), 0, st, d);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
#endif
