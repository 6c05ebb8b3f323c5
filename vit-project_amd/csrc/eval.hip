// On-device validation metrics (the reference's validate(), VIT:167-204): per batch the cross-entropy
// mean, the row-loss sum and the top-1 / top-k hit counts are added into six double accumulators on the
// device, so an evaluation loop synchronises once, at the end, instead of once per batch.
#include "common.hpp"

// One wave per row (ce_fwd_kernel's layout), one pass over the row's C logits: an online log-sum-exp
// (running maximum and rescaled sum per lane, merged across the wave) and, against the target's logit
// xt, the count of classes that rank in front of the target -- a larger logit, or an equal one at a
// smaller index -- so rank 0 is torch's first-maximum argmax == target.
//   row_ws[row]     = row loss (lse - xt)
//   row_ws[B + row] = 1 * (rank == 0) + 2 * (rank < topk); 0 when the log-sum-exp is not finite
__global__ void eval_rows_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ target,
                                 int B, int C, int topk, float* __restrict__ row_ws) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B) return;
  const float* x = logits + (int64_t)row * ld;
  const int64_t t = target[row];
  const bool t_ok = t >= 0 && t < C;  // the contract; a target outside it reads nothing and counts as wrong
  const float xt = t_ok ? x[t] : __builtin_nanf("");
  float m = -INFINITY, s = 0.f;
  int ahead = 0;
  for (int c = lane; c < C; c += 64) {
    const float v = x[c];
    if (v > m) {
      s = s * __expf(m - v) + 1.0f;  // m == -inf: s is 0 and stays 0 * 0
      m = v;
    } else if (!(v == -INFINITY)) {  // a masked (-inf) logit adds nothing; a NaN one still poisons the sum
      s += __expf(v - m);
    }
    ahead += (v > xt || (v == xt && c < t)) ? 1 : 0;
  }
  const float mx = wave_max(m);
  s = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - mx));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ahead += __shfl_xor(ahead, o, 64);
  if (lane == 0) {
    const float lse = mx + logf(s);
    const bool fin = t_ok && isfinite(lse);
    row_ws[row] = lse - xt;
    row_ws[B + row] = fin ? (float)((ahead == 0 ? 1 : 0) + (ahead < topk ? 2 : 0)) : 0.f;
  }
}

// One workgroup sums the per-row results in a fixed order (thread-strided partials, then an LDS tree):
// the same inputs give the same bits on every run.  acc += {mean loss, loss sum, top-1, top-k, B, 1}.
__global__ __launch_bounds__(256) void eval_reduce_kernel(const float* __restrict__ row_ws, int B,
                                                          double* __restrict__ acc) {
  __shared__ double ls[256];
  __shared__ int c1[256], ck[256];
  const int tid = threadIdx.x;
  double l = 0.0;
  int n1 = 0, nk = 0;
  for (int i = tid; i < B; i += 256) {
    l += (double)row_ws[i];
    const int f = (int)row_ws[B + i];
    n1 += f & 1;
    nk += (f >> 1) & 1;
  }
  ls[tid] = l;
  c1[tid] = n1;
  ck[tid] = nk;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      ls[tid] += ls[tid + o];
      c1[tid] += c1[tid + o];
      ck[tid] += ck[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    acc[0] += ls[0] / (double)B;
    acc[1] += ls[0];
    acc[2] += (double)c1[0];
    acc[3] += (double)ck[0];
    acc[4] += (double)B;
    acc[5] += 1.0;
  }
}

extern "C" {

// Validation metrics of one batch of f32 logits [B, C] (row stride ld) against int64 targets in [0, C),
// added into acc[6] (f64, zeroed by the caller with vit_zero):
//   acc[0] += mean row loss (what F.cross_entropy returns)   acc[1] += sum of row losses
//   acc[2] += rows whose target has rank 0 (top-1)            acc[3] += rows whose target has rank < topk
//   acc[4] += B                                               acc[5] += 1
// rank = classes with a larger logit + classes with an equal logit and a smaller index.  A row whose
// log-sum-exp is not finite adds its non-finite loss and counts as wrong.  row_ws: >= 2 * B floats of
// scratch.  No allocation, no synchronisation, no atomics: capture safe, and run-to-run bitwise stable.
int vit_eval_metrics(int B, int C, const float* logits, int64_t ld, const int64_t* target, int topk, float* row_ws,
                     double* acc, void* stream) {
  if (B <= 0 || C <= 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(eval_rows_kernel, dim3((B + 3) / 4), dim3(256), 0, s, logits, ld, target, B, C, topk, row_ws);
  VIT_CHECK_LAUNCH();
  hipLaunchKernelGGL(eval_reduce_kernel, dim3(1), dim3(256), 0, s, (const float*)row_ws, B, acc);
  VIT_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
