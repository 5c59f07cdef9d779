// Kernels of the update-block fine-tuning step (accflow_amd/train_raft.py; reference: fine_tune.py:203-243, loss.py:4-25,
// raft/update.py:45-60): the two gate products of a SepConvGRU half-step with their backward passes, and one term of
// sequence_loss_raft with its gradient.  Everything else of that step - convolutions, their input / weight gradients, relu,
// the convex upsampling - are the kernels the fusion heads' training step already runs (csrc/backward.hip).
//
// The gate kernels are elementwise over (B, CHW) fp32 planes, every operand with its own batch stride: z, r, r*h, h and the
// pre-activation gradients are channel slices of the [h | x], [r*h | x] and [z | r] buffers the convolutions read and write,
// so nothing is copied in or out of a slice.  One thread handles 4 consecutive elements (16-byte accesses on dword-aligned
// addresses, common.h f4u) when CHW is a multiple of 4 - then no group straddles the end of a plane - and 1 otherwise.
// Plain vector stores, no atomics.
#include "common.h"

namespace {

template <int V>
__device__ __forceinline__ void ldv(const float* __restrict__ p, float (&r)[V]) {
  if constexpr (V == 4) {
    const f4u v = *reinterpret_cast<const f4u*>(p);
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
  } else {
    r[0] = p[0];
  }
}

template <int V>
__device__ __forceinline__ void stv(float* __restrict__ p, const float (&r)[V]) {
  if constexpr (V == 4) {
    f4u v;
    v.x = r[0]; v.y = r[1]; v.z = r[2]; v.w = r[3];
    *reinterpret_cast<f4u*>(p) = v;
  } else {
    p[0] = r[0];
  }
}

// element offset of this thread's group inside a plane, or -1 past the end (grid: x over groups of V, y = batch item)
template <int V>
__device__ __forceinline__ long long group_offset(long long CHW) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
  return i + V <= CHW ? i : -1;
}

// rh = r * h   (update.py:50, the first operand of convq's input cat[r*h, x])
template <int V>
__global__ __launch_bounds__(256) void gru_reset_forward_kernel(const float* __restrict__ r, long long r_bs,
                                                                const float* __restrict__ h, long long h_bs,
                                                                float* __restrict__ rh, long long rh_bs, long long CHW) {
  const long long i = group_offset<V>(CHW);
  if (i < 0) return;
  const long long b = blockIdx.y;
  float vr[V], vh[V], o[V];
  ldv<V>(r + b * r_bs + i, vr);
  ldv<V>(h + b * h_bs + i, vh);
#pragma unroll
  for (int k = 0; k < V; ++k) o[k] = vr[k] * vh[k];
  stv<V>(rh + b * rh_bs + i, o);
}

// h_new = (1 - z) h + z q   (update.py:51 / :59); h_new may be another channel slice than h (the next half-step's [h | x])
template <int V>
__global__ __launch_bounds__(256) void gru_update_forward_kernel(const float* __restrict__ z, long long z_bs,
                                                                 const float* __restrict__ h, long long h_bs,
                                                                 const float* __restrict__ q, long long q_bs,
                                                                 float* __restrict__ hn, long long hn_bs, long long CHW) {
  const long long i = group_offset<V>(CHW);
  if (i < 0) return;
  const long long b = blockIdx.y;
  float vz[V], vh[V], vq[V], o[V];
  ldv<V>(z + b * z_bs + i, vz);
  ldv<V>(h + b * h_bs + i, vh);
  ldv<V>(q + b * q_bs + i, vq);
#pragma unroll
  for (int k = 0; k < V; ++k) o[k] = __builtin_fmaf(1.0f - vz[k], vh[k], vz[k] * vq[k]);
  stv<V>(hn + b * hn_bs + i, o);
}

// Backward of h_new = (1 - z) h + z q with z = sigmoid(az), q = tanh(aq), from the activations' OUTPUTS:
//   daz = dh_new (q - h) z (1 - z)     daq = dh_new z (1 - q^2)     dh = dh_new (1 - z)
// (dh is written, not added to: it is the first contribution to the half-step's input state)
template <int V>
__global__ __launch_bounds__(256) void gru_update_backward_kernel(const float* __restrict__ g, long long g_bs,
                                                                  const float* __restrict__ z, long long z_bs,
                                                                  const float* __restrict__ h, long long h_bs,
                                                                  const float* __restrict__ q, long long q_bs,
                                                                  float* __restrict__ daz, long long daz_bs,
                                                                  float* __restrict__ daq, long long daq_bs,
                                                                  float* __restrict__ dh, long long dh_bs, long long CHW) {
  const long long i = group_offset<V>(CHW);
  if (i < 0) return;
  const long long b = blockIdx.y;
  float vg[V], vz[V], vh[V], vq[V], oz[V], oq[V], oh[V];
  ldv<V>(g + b * g_bs + i, vg);
  ldv<V>(z + b * z_bs + i, vz);
  ldv<V>(h + b * h_bs + i, vh);
  ldv<V>(q + b * q_bs + i, vq);
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const float omz = 1.0f - vz[k];
    oz[k] = vg[k] * (vq[k] - vh[k]) * (vz[k] * omz);
    oq[k] = vg[k] * vz[k] * (1.0f - vq[k] * vq[k]);
    oh[k] = vg[k] * omz;
  }
  stv<V>(daz + b * daz_bs + i, oz);
  stv<V>(daq + b * daq_bs + i, oq);
  stv<V>(dh + b * dh_bs + i, oh);
}

// Backward of rh = r h with r = sigmoid(ar):  dar = drh h r (1 - r),  dh += drh r
template <int V>
__global__ __launch_bounds__(256) void gru_reset_backward_kernel(const float* __restrict__ drh, long long drh_bs,
                                                                 const float* __restrict__ r, long long r_bs,
                                                                 const float* __restrict__ h, long long h_bs,
                                                                 float* __restrict__ dar, long long dar_bs,
                                                                 float* __restrict__ dh, long long dh_bs, long long CHW) {
  const long long i = group_offset<V>(CHW);
  if (i < 0) return;
  const long long b = blockIdx.y;
  float vg[V], vr[V], vh[V], acc[V], oa[V];
  ldv<V>(drh + b * drh_bs + i, vg);
  ldv<V>(r + b * r_bs + i, vr);
  ldv<V>(h + b * h_bs + i, vh);
  ldv<V>(dh + b * dh_bs + i, acc);
#pragma unroll
  for (int k = 0; k < V; ++k) {
    oa[k] = vg[k] * vh[k] * (vr[k] * (1.0f - vr[k]));
    acc[k] = __builtin_fmaf(vg[k], vr[k], acc[k]);
  }
  stv<V>(dar + b * dar_bs + i, oa);
  stv<V>(dh + b * dh_bs + i, acc);
}

// One term of sequence_loss_raft (loss.py:10-13): dpred = scale sign(pred - gt) (0 at equality: torch's abs backward) and
// sum |pred - gt| in a FIXED order.  Stage 1: a workgroup owns SEQ_RUN consecutive elements; thread t adds its SEQ_PER groups
// in index order in double, then the xor butterfly over the 64 lanes, then the 4 waves through LDS as (w0 + w1) + (w2 + w3).
// Stage 2: one wave adds the workgroups' partials - lane l takes l, l + 64, ... in index order - then the same butterfly, and
// lane 0 adds weight * sum / n to the loss.  No atomics: the value does not depend on the schedule.
constexpr int SEQ_PER = 4;

template <int V>
__global__ __launch_bounds__(256) void seq_l1_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                             float* __restrict__ dpred, long long n, float scale,
                                                             double* __restrict__ ws) {
  __shared__ double part[4];
  const long long run0 = (long long)blockIdx.x * (256 * SEQ_PER * V);
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < SEQ_PER; ++k) {
    const long long i = run0 + ((long long)k * 256 + threadIdx.x) * V;
    if (i + V <= n) {
      float vp[V], vg[V], o[V];
      ldv<V>(pred + i, vp);
      ldv<V>(gt + i, vg);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float d = vp[j] - vg[j];
        o[j] = d > 0.0f ? scale : (d < 0.0f ? -scale : 0.0f);
        acc += (double)fabsf(d);
      }
      stv<V>(dpred + i, o);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) ws[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(64) void seq_l1_final_kernel(const double* __restrict__ ws, int nblk, double weight, long long n,
                                                          double* __restrict__ loss) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) acc += ws[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (threadIdx.x == 0) loss[0] += weight * (acc / (double)n);
}

inline bool planes_ok(int B, long long CHW) { return B > 0 && B <= 65535 && CHW > 0 && CHW < (1LL << 38); }

// the widest group every operand allows: 4 elements when no group straddles the end of a plane
inline int group_width(long long CHW) { return (CHW & 3) == 0 ? 4 : 1; }

inline long long seq_blocks(long long n) {
  const long long run = 256LL * SEQ_PER * group_width(n);
  return (n + run - 1) / run;
}

}  // namespace

#define GATE_LAUNCH(kernel, ...)                                                                                         \
  do {                                                                                                                   \
    if (group_width(CHW) == 4)                                                                                           \
      hipLaunchKernelGGL((kernel<4>), dim3(cdiv(CHW / 4, 256), B), dim3(256), 0, as_stream(stream), __VA_ARGS__, CHW);      \
    else                                                                                                                 \
      hipLaunchKernelGGL((kernel<1>), dim3(cdiv(CHW, 256), B), dim3(256), 0, as_stream(stream), __VA_ARGS__, CHW);          \
  } while (0)

extern "C" int accflow_gru_reset_forward_f32(const float* r, long long r_bs, const float* h, long long h_bs, float* rh,
                                             long long rh_bs, int B, long long CHW, void* stream) {
  if (!r || !h || !rh || !planes_ok(B, CHW)) return 1;
  GATE_LAUNCH(gru_reset_forward_kernel, r, r_bs, h, h_bs, rh, rh_bs);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_gru_update_forward_f32(const float* z, long long z_bs, const float* h, long long h_bs, const float* q,
                                              long long q_bs, float* h_new, long long hn_bs, int B, long long CHW, void* stream) {
  if (!z || !h || !q || !h_new || !planes_ok(B, CHW)) return 1;
  GATE_LAUNCH(gru_update_forward_kernel, z, z_bs, h, h_bs, q, q_bs, h_new, hn_bs);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_gru_update_backward_f32(const float* dh_new, long long dhn_bs, const float* z, long long z_bs, const float* h,
                                               long long h_bs, const float* q, long long q_bs, float* daz, long long daz_bs,
                                               float* daq, long long daq_bs, float* dh, long long dh_bs, int B, long long CHW,
                                               void* stream) {
  if (!dh_new || !z || !h || !q || !daz || !daq || !dh || !planes_ok(B, CHW)) return 1;
  GATE_LAUNCH(gru_update_backward_kernel, dh_new, dhn_bs, z, z_bs, h, h_bs, q, q_bs, daz, daz_bs, daq, daq_bs, dh, dh_bs);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

extern "C" int accflow_gru_reset_backward_f32(const float* drh, long long drh_bs, const float* r, long long r_bs, const float* h,
                                              long long h_bs, float* dar, long long dar_bs, float* dh, long long dh_bs, int B,
                                              long long CHW, void* stream) {
  if (!drh || !r || !h || !dar || !dh || !planes_ok(B, CHW)) return 1;
  GATE_LAUNCH(gru_reset_backward_kernel, drh, drh_bs, r, r_bs, h, h_bs, dar, dar_bs, dh, dh_bs);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}

#undef GATE_LAUNCH

extern "C" long long accflow_seq_l1_ws_bytes(long long n) {
  if (n <= 0 || n >= (1LL << 40)) return 0;
  return seq_blocks(n) * (long long)sizeof(double);
}

extern "C" int accflow_seq_l1_f32(const float* pred, const float* gt, float* dpred, long long n, double weight, double* loss,
                                  void* ws, void* stream) {
  if (!pred || !gt || !dpred || !loss || !ws || n <= 0 || n >= (1LL << 40)) return 1;
  const int nblk = (int)seq_blocks(n);
  const float scale = (float)(weight / (double)n);
  if (group_width(n) == 4)
    hipLaunchKernelGGL((seq_l1_partial_kernel<4>), dim3(nblk), dim3(256), 0, as_stream(stream), pred, gt, dpred, n, scale,
                       static_cast<double*>(ws));
  else
    hipLaunchKernelGGL((seq_l1_partial_kernel<1>), dim3(nblk), dim3(256), 0, as_stream(stream), pred, gt, dpred, n, scale,
                       static_cast<double*>(ws));
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(seq_l1_final_kernel, dim3(1), dim3(64), 0, as_stream(stream), static_cast<const double*>(ws), nblk, weight, n,
                     loss);
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
