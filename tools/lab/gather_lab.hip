// Lab: shapes of the token-block gather (csrc/clip.hip gather_blocks_kernel): threads per workgroup, 16-byte
// vectors per lane, non-temporal loads (NT & 1) and stores (NT & 2).  Built and driven by tools/lab/gather_lab.py;
// not product code.  Records: profiles/r13/gather_lab.json.
#include <hip/hip_runtime.h>
#include <stdint.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int THREADS, int PER, int NT>
__global__ __launch_bounds__(THREADS) void k(const f32x4* __restrict__ src, const int64_t* __restrict__ idx,
                                             f32x4* __restrict__ dst, int64_t row_vecs) {
  const int64_t r = idx[blockIdx.y];
  const f32x4* s = src + r * row_vecs;
  f32x4* o = dst + (int64_t)blockIdx.y * row_vecs;
  const int64_t v0 = (int64_t)blockIdx.x * (THREADS * PER) + threadIdx.x;
  f32x4 t[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int64_t v = v0 + j * THREADS;
    if (v < row_vecs) t[j] = (NT & 1) ? __builtin_nontemporal_load(s + v) : s[v];
  }
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int64_t v = v0 + j * THREADS;
    if (v < row_vecs) {
      if (NT & 2) __builtin_nontemporal_store(t[j], o + v); else o[v] = t[j];
    }
  }
}
template <int THREADS, int PER, int NT>
static int go(int n, int64_t row_vecs, const float* src, const int64_t* idx, float* dst, hipStream_t st) {
  const int64_t chunk = THREADS * PER, chunks = (row_vecs + chunk - 1) / chunk;
  hipLaunchKernelGGL((k<THREADS, PER, NT>), dim3((unsigned)chunks, (unsigned)n), dim3(THREADS), 0, st,
                     (const f32x4*)src, idx, (f32x4*)dst, row_vecs);
  return (int)hipGetLastError();
}
extern "C" int gb_lab(int variant, int n, int64_t row_elems, const float* src, const int64_t* idx, float* dst, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int64_t rv = row_elems / 4;
  switch (variant) {
    case 0: return go<256, 8, 0>(n, rv, src, idx, dst, st);
    case 1: return go<256, 4, 0>(n, rv, src, idx, dst, st);
    case 2: return go<256, 2, 0>(n, rv, src, idx, dst, st);
    case 3: return go<256, 1, 0>(n, rv, src, idx, dst, st);
    case 4: return go<256, 4, 1>(n, rv, src, idx, dst, st);
    case 5: return go<256, 4, 3>(n, rv, src, idx, dst, st);
    case 6: return go<512, 4, 0>(n, rv, src, idx, dst, st);
    case 7: return go<1024, 2, 0>(n, rv, src, idx, dst, st);
    case 8: return go<1024, 4, 0>(n, rv, src, idx, dst, st);
    case 9: return go<256, 2, 1>(n, rv, src, idx, dst, st);
    case 10: return go<512, 2, 0>(n, rv, src, idx, dst, st);
    case 11: return go<256, 16, 0>(n, rv, src, idx, dst, st);
  }
  return -1;
}
