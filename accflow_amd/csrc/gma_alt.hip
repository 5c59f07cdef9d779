// alternate_attention: GMA's aggregation fmap + gamma * softmax_j(scale q_i . k_j) @ v WITHOUT the P x P attention matrix
// (gma/modules.py:54-76, 102-115; heads = 1, D = 128, content branch).  The stored route (accflow_gma_attention_s16 ->
// accflow_gma_aggregate_s16) keeps 4 P^2 bytes per distinct image1 and re-reads them in every refinement iteration; here
// the kept state is what the softmax of a query needs to be evaluated anywhere, at any time:
//     the fp16 hi / lo packs of q 2^ASHIFT and fp32(k scale) 2^ASHIFT (accflow_pack_kmajor, 512 Ppad bytes each) and
//     the FINAL statistics {max_i, 1 / sum_i} per query (pass 0 of gma_attn_gemm_kernel + gma_attn_stats_kernel, 8 P bytes)
// - accflow_gma_attention_alt (below) stops there.  Every iteration then recomputes the probabilities tile by tile
// and feeds them to the second product from registers.
//
// gma_alt_aggregate_kernel<NI>: 4 waves, wave w owns the 32 queries i0 + 32 w .. + 31 of a 128-query tile for the whole
// kernel - no LDS, no barrier, no exchange between waves.  Per tile of 128 keys j:
//   1. logits S[j][i] = k_j . q_i: four 32 x 32 accumulator tiles (64 registers), D / 16 = 8 steps of the three products
//      lo.hi, hi.lo, hi.hi that pass 1 of gma_attn_gemm_kernel keeps (rows j = A operand from the k pack, columns i = B
//      operand from the q pack);
//   2. p = exp(S acc_scale - max_i) inv_i 2^ASHIFT in fp32 - the statistics are final, so nothing is rescaled later -, zero
//      for j >= P, split into fp16 hi + lo in registers (the values pass 1 stores as the S16 pair);
//   3. out[d][i] += sum_j w[d][j] p[j][i]: the accumulator tile has the query on the lane and 16 keys in registers
//      8 s .. 8 s + 7 (s = 0, 1), which IS the B fragment of a 32x32x16 product whose k slot (lane half h, element e) is key
//      16 s + 8 (e >> 2) + 4 h + (e & 3) - so v * gamma is packed per call (gma_alt_pack_v_kernel) with its keys in that
//      order, rows scaled by the packs' one rule (pack_terms.h: row maximum into [2^10, 2^11)), fp16 hi + lo, and the
//      products lo.hi, hi.lo, hi.hi accumulate into four 32 (d) x 32 (i) tiles per item (64 registers per item).
// A wave therefore holds 32 KT + 64 NI accumulator registers for KT 32-key logit tiles and NI items: NI <= 2 items per
// pass (one item: 128 keys at a time; two items: 64, so that two waves per SIMD still fit - at 128 keys and one wave per SIMD
// the pair ran 2.1x slower); longer runs are cut into chunks of two and the logits recomputed per chunk.  The keys are
// split over Z workgroups per query tile (a pair at 90 x 160 has 113
// query tiles for 256 CUs); each writes its unscaled partial sums to part[z][item][d][i] and gma_alt_epilogue_kernel adds
// them in the fixed order z = 0 .. Z - 1, applies the row scale and the stored route's epilogue out = fmap + acc per item
// (fp32 and / or the S16 pair, arbitrary batch strides).  No atomics on floats: results are bit-identical call to call.
//
// Addressing: the k, q packs and each item's v pack go through their own buffer descriptor (512 Ppad bytes each, the
// host refuses >= 2^31); partial sums, residual and outputs through 64-bit pointers.  Nothing here is O(P^2) in memory.
//
// Compiler report (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage):
//   gma_alt_aggregate_kernel<1, 4>: 210 VGPRs, 0 AGPRs, scratch 0 bytes, 2 waves / SIMD
//   gma_alt_aggregate_kernel<2, 2>: 216 VGPRs, 0 AGPRs, scratch 0 bytes, 2 waves / SIMD
#include "conv_common.h"
#include "pack_terms.h"

namespace {

constexpr int ALT_D = 128;         // dim_head of the estimator (the only one on the AccFlow path)
constexpr int ALT_MAXZ = 8;

__device__ __forceinline__ f32x16 alt_mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

struct gma_alt_args {
  const void* kpack; const void* qpack;   // [2 terms][D/8][Ppad][8] fp16 (accflow_pack_kmajor)
  const float* stats;                     // [P][2] = {max, 1 / sum}
  const void* vpack;                      // this chunk's first item: [item][2 terms][Ppad/16][2 halves][128 rows][8] fp16
  float* part;                            // this chunk's first item of [Z][n][128][P]
  long long part_zs;                      // floats between two key splits (n * 128 * P)
  float acc_scale;                        // logits = acc * acc_scale
  int P, Ppad, Z;
};

// v (n, 128, P) * gamma -> the second product's A fragments, one workgroup per row (item, d): the row maximum, then the
// fp16 hi / lo of fp32(v gamma) 2^k with k from the packs' row-scale rule (pack_terms.h); wscale[row] = 2^-(k + ASHIFT).
// Chunk (16-key group g, lane half h) of row d holds keys 16 g + 8 (e >> 2) + 4 h + (e & 3), e = 0..7; zero past P.
__global__ __launch_bounds__(256) void gma_alt_pack_v_kernel(const float* __restrict__ v, int P, int Ppad,
                                                             unsigned short* __restrict__ vp, float* __restrict__ wscale,
                                                             const float* __restrict__ gptr) {
  const int row = blockIdx.x, item = row / ALT_D, d = row - item * ALT_D;
  const float gmul = gptr[0];
  const float* src = v + (long long)row * P;
  float m = 0.0f;
  for (int j = threadIdx.x; j < P; j += 256) m = fmaxf(m, fabsf(src[j]));
  m = pack_block_max256(m) * fabsf(gmul);
  const float sc = pack_row_scale16(m);
  if (threadIdx.x == 0) wscale[row] = sc;
  const float mul = pack_row_mul16(sc);
  const long long term_elems = (long long)Ppad * ALT_D;         // (Ppad / 16 groups x 2 halves x 128 rows x 8)
  unsigned short* dst = vp + (long long)item * 2 * term_elems;
  const int nchunk = Ppad / 8;
  for (int c = threadIdx.x; c < nchunk; c += 256) {
    const int g = c >> 1, h = c & 1;
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = 16 * g + 8 * (e >> 2) + 4 * h + (e & 3);
      x[e] = j < P ? src[j] : 0.0f;
    }
    u32x4 hv, lv;
    pack_hilo8(x, gmul, mul, hv, lv);
    const long long base = ((long long)c * ALT_D + d) * 8;
    *reinterpret_cast<u32x4*>(dst + base) = hv;
    *reinterpret_cast<u32x4*>(dst + term_elems + base) = lv;
  }
}

// KT: 32-key accumulator tiles per pass of the logits (4: 128 keys at a time, 2: 64 - what lets two items' output tiles and
// two waves per SIMD fit the register file)
template <int NI, int KT>
__global__ __launch_bounds__(256, 2) void gma_alt_aggregate_kernel(const gma_alt_args a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, kh = lane >> 5, lh4 = kh * 4;
  const int i = blockIdx.x * 128 + wave * 32 + l31;              // this lane's query (< Ppad: the packs are padded)
  const int z = blockIdx.y;
  const int T = a.Ppad >> 7;                                     // key tiles
  const int jt0 = (int)((long long)z * T / a.Z), jt1 = (int)((long long)(z + 1) * T / a.Z);
  constexpr int nstep = ALT_D / 16;
  const int step_bytes = 2 * a.Ppad * 16, term_bytes = (ALT_D / 8) * a.Ppad * 16;   // (host: 2 * term_bytes < 2^31)
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.kpack), 0, 2 * term_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.qpack), 0, 2 * term_bytes, 0x00020000);
  const int vterm_bytes = a.Ppad * ALT_D * 2;                    // one term of one item's v pack (= term_bytes at D = 128)
  __amdgpu_buffer_rsrc_t rv[NI];
#pragma unroll
  for (int n = 0; n < NI; ++n)
    rv[n] = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(a.vpack) + (long long)n * 2 * vterm_bytes),
                                              0, 2 * vterm_bytes, 0x00020000);
  const bool iok = i < a.P;
  const float m_i = iok ? a.stats[2 * i] : 0.0f;
  const float inv_i = iok ? a.stats[2 * i + 1] * S16_SCALE : 0.0f;
  const int qvoff = (kh * a.Ppad + i) * 16;
  f32x16 out[NI][4];
#pragma unroll
  for (int n = 0; n < NI; ++n)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) out[n][dt][r] = 0.0f;

  for (int jt = jt0 * (4 / KT); jt < jt1 * (4 / KT); ++jt) {
    const int j0 = jt * (32 * KT);
    f32x16 acc[KT];
#pragma unroll
    for (int tc = 0; tc < KT; ++tc)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tc][r] = 0.0f;
    const int kvoff = (kh * a.Ppad + j0 + l31) * 16;
#pragma unroll 2
    for (int step = 0; step < nstep; ++step) {
      bf16x8 A[2][KT], Bq[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int so = t * term_bytes + step * step_bytes;
        Bq[t] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rq, qvoff, so, 0));
#pragma unroll
        for (int tc = 0; tc < KT; ++tc)
          A[t][tc] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rk, kvoff + tc * 512, so, 0));
      }
      constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};        // gma_attn_gemm_kernel's three products, in its order
#pragma unroll
      for (int pr = 0; pr < 3; ++pr)
#pragma unroll
        for (int tc = 0; tc < KT; ++tc) acc[tc] = alt_mfma(A[PA[pr]][tc], Bq[PB[pr]], acc[tc]);
    }
#pragma unroll
    for (int tc = 0; tc < KT; ++tc)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int jg = j0 + tc * 32 + 16 * s;                    // first key of this 16-key group (wave-uniform)
        unsigned hi[4], lo[4];
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {                          // k slots 2 e2, 2 e2 + 1 = registers 8 s + 2 e2, + 1
          const int r = 8 * s + 2 * e2;
          const int j = jg + 8 * (e2 >> 1) + lh4 + ((2 * e2) & 3);
          const float pa = j < a.P ? expf(acc[tc][r] * a.acc_scale - m_i) * inv_i : 0.0f;
          const float pb = j + 1 < a.P ? expf(acc[tc][r + 1] * a.acc_scale - m_i) * inv_i : 0.0f;
          s16_split2(pa, pb, hi[e2], lo[e2]);                     // values in [0, 16]: no range check
        }
        const u32x4 hv = {hi[0], hi[1], hi[2], hi[3]}, lv = {lo[0], lo[1], lo[2], lo[3]};
        const bf16x8 ph = __builtin_bit_cast(bf16x8, hv), pl = __builtin_bit_cast(bf16x8, lv);
        const int vvoff = (((jg >> 4) * 2 + kh) * ALT_D + l31) * 16;
#pragma unroll
        for (int n = 0; n < NI; ++n)
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            const bf16x8 wh = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rv[n], vvoff + dt * 512, 0, 0));
            const bf16x8 wl = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rv[n], vvoff + dt * 512, vterm_bytes, 0));
            out[n][dt] = alt_mfma(wl, ph, out[n][dt]);     // w_lo p_hi, w_hi p_lo, w_hi p_hi: the stored route's order
            out[n][dt] = alt_mfma(wh, pl, out[n][dt]);
            out[n][dt] = alt_mfma(wh, ph, out[n][dt]);
          }
      }
  }
  if (!iok) return;
#pragma unroll
  for (int n = 0; n < NI; ++n) {
    float* p = a.part + (long long)z * a.part_zs + (long long)n * ALT_D * a.P + i;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) p[(long long)(dt * 32 + 8 * (r >> 2) + lh4 + (r & 3)) * a.P] = out[n][dt][r];
  }
}

// out = fmap + wscale[row] * (part[0] + part[1] + ... in that order) per item: one thread per (item, channel octet, pixel),
// fp32 planes and / or the S16 chunk pair of the octet.
__global__ __launch_bounds__(256) void gma_alt_epilogue_kernel(const float* __restrict__ part, long long part_zs, int Z,
                                                               const float* __restrict__ wscale, const float* __restrict__ fmap,
                                                               long long fmap_bs, float* __restrict__ out, long long out_bs,
                                                               unsigned* __restrict__ out16, long long out16_bs, int* guard, int P) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int item = blockIdx.y / (ALT_D / 8), o = blockIdx.y - item * (ALT_D / 8);
  float x[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int d = 8 * o + c;
    const float* p = part + ((long long)item * ALT_D + d) * P + i;
    float s = p[0];
    for (int zz = 1; zz < Z; ++zz) s += p[zz * part_zs];
    x[c] = fmaf(s, wscale[item * ALT_D + d], fmap[item * fmap_bs + (long long)d * P + i]);
    if (out) out[item * out_bs + (long long)d * P + i] = x[c];
  }
  if (out16) {
    mu32x4 hi, lo;
    bool bad = false;
    s16_split8(x, hi, lo, bad);
    if (bad && guard) atomicOr(guard, 1);
    unsigned* q = out16 + item * out16_bs + ((long long)o * 2 * P + i) * 4;
    *reinterpret_cast<mu32x4*>(q) = hi;
    *reinterpret_cast<mu32x4*>(q + (long long)P * 4) = lo;
  }
}

inline long long align256(long long x) { return (x + 255) / 256 * 256; }

// key splits per query tile: enough workgroups for two per CU, at most one per key tile
inline int alt_key_splits(int P) {
  const int nb = cdiv(P, 128);
  int Z = 512 / nb;
  if (Z > ALT_MAXZ) Z = ALT_MAXZ;
  if (Z > nb) Z = nb;
  return Z < 1 ? 1 : Z;
}

}  // namespace

// ws of accflow_gma_attention_alt: the partial statistics of pass 0 ([ceil(P / 128)][P][2] floats), transient
extern "C" long long accflow_gma_attention_alt_ws_bytes(int D, int H, int W) {
  (void)D;
  const long long P = (long long)H * W, nb = (P + 127) / 128;
  return nb * P * 2 * 4 + 256;
}

// The kept state: the two packs of accflow_gma_attention_s16 per item, pass 0 and the final statistics - and no matrix.  kpack /
// qpack: B packs of 2 * (D / 8) * coutpad(P) * 16 bytes each, stats: (B, P, 2) = {max_i, 1 / sum_i}; ws (partial
// statistics, accflow_gma_attention_alt_ws_bytes) is free again when the call's kernels have run.
extern "C" int accflow_gma_attention_alt(const float* qk, void* kpack, void* qpack, float* stats, void* ws, int* guard, int B,
                                         int D, int H, int W, float scale, void* stream) {
  if (!qk || !kpack || !qpack || !stats || !ws || B <= 0 || D != 128 || H <= 0 || W <= 0) return 1;
  if ((long long)H * W * 512 >= (1LL << 31) - 65536) return 1;   // 32-bit offsets inside one pack (gma_alt_aggregate_kernel)
  const int P = H * W, Ppad = accflow_conv_coutpad(P), Kpad = accflow_conv_kpad(D, 1, 1);
  hipStream_t st = as_stream(stream);
  const long long pack_bytes = 2LL * (D / 8) * Ppad * 16;
  const float fs = ldexpf(1.0f, ACCFLOW_F16_ASHIFT);
  for (int b = 0; b < B; ++b) {
    const float* q = qk + (long long)b * 2 * D * P;
    char* kp = reinterpret_cast<char*>(kpack) + b * pack_bytes;
    char* qp = reinterpret_cast<char*>(qpack) + b * pack_bytes;
    accflow_pack_kmajor(q + (long long)D * P, P, D, Kpad, Ppad, kp, scale * fs, 1, guard, st);
    accflow_pack_kmajor(q, P, D, Kpad, Ppad, qp, fs, 1, guard, st);
    const int rc = accflow_launch_gma_attn_stats(kp, qp, reinterpret_cast<float*>(ws), stats + (long long)b * 2 * P,
                                                 1.0f / (fs * fs), P, D, Ppad, st);
    if (rc) return rc;
  }
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

// ws of accflow_gma_aggregate_alt: the v pack, its row scales, the partial sums of the key splits
extern "C" long long accflow_gma_aggregate_alt_ws_bytes(int n, int D, int P) {
  if (n <= 0 || D != ALT_D || P <= 0) return 0;
  const long long Ppad = accflow_conv_coutpad(P);
  return align256(2LL * n * Ppad * ALT_D * 2) + align256(4LL * n * ALT_D) + 4LL * alt_key_splits(P) * n * ALT_D * P + 256;
}

extern "C" int accflow_gma_aggregate_alt(const void* kpack, const void* qpack, const float* stats, const float* v,
                                         const float* fmap, long long fmap_bs, const float* gamma, float* out, long long out_bs,
                                         void* out16, long long out16_bs, void* ws, int* guard, int n, int D, int H, int W,
                                         void* stream) {
  if (!kpack || !qpack || !stats || !v || !fmap || !gamma || (!out && !out16) || !ws || n <= 0 || D != ALT_D || H <= 0 || W <= 0)
    return 1;
  const long long P64 = (long long)H * W;
  if (P64 * 512 >= (1LL << 31) - 65536) return 1;               // 32-bit offsets inside one pack
  const int P = (int)P64, Ppad = accflow_conv_coutpad(P), Z = alt_key_splits(P);
  hipStream_t st = as_stream(stream);
  char* base = reinterpret_cast<char*>(ws);
  unsigned short* vp = reinterpret_cast<unsigned short*>(base);
  float* wscale = reinterpret_cast<float*>(base + align256(2LL * n * Ppad * ALT_D * 2));
  float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(wscale) + align256(4LL * n * ALT_D));
  hipLaunchKernelGGL(gma_alt_pack_v_kernel, dim3(n * ALT_D), dim3(256), 0, st, v, P, Ppad, vp, wscale, gamma);
  const float fs = ldexpf(1.0f, ACCFLOW_F16_ASHIFT);
  gma_alt_args a;
  a.kpack = kpack; a.qpack = qpack; a.stats = stats;
  a.part_zs = (long long)n * ALT_D * P; a.acc_scale = 1.0f / (fs * fs); a.P = P; a.Ppad = Ppad; a.Z = Z;
  const dim3 grid(Ppad / 128, Z);
  for (int b0 = 0; b0 < n; b0 += 2) {                           // chunks of <= 2 items: the logits are recomputed per chunk
    a.vpack = vp + (long long)b0 * 2 * Ppad * ALT_D;
    a.part = part + (long long)b0 * ALT_D * P;
    if (n - b0 >= 2) hipLaunchKernelGGL((gma_alt_aggregate_kernel<2, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((gma_alt_aggregate_kernel<1, 4>), grid, dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(gma_alt_epilogue_kernel, dim3(cdiv(P, 256), n * (ALT_D / 8)), dim3(256), 0, st, part, a.part_zs, Z, wscale,
                     fmap, fmap_bs, out, out_bs, reinterpret_cast<unsigned*>(out16), out16_bs, guard, P);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
