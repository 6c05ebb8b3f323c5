// LoRA adapter weight (NEWP:307-336) and its backward.
//
//   W[i][j] = W0[i][j] + s * sum_k B[i][k] A[k][j]        W0, W [n, n], B [n, r], A [r, n], f32
//
// This is LoRALayer.weight as the reference writes it: B @ A ([in, out]) is added to W0 ([out, in])
// without a transpose, so it exists only for in == out and is not the weight LoRALayer.forward applies.
// nn.MultiheadAttention reads out_proj.weight (quirk Q5), so on the CLIP-HBA path this is what trains.
//
// Forward: one launch.  A workgroup owns a 32 x 128 tile of W; its [r, 128] slice of A and [32, r] slice
// of B sit in LDS, a thread keeps 4 rows x 4 columns in registers and reads / writes W0 / W as 16-byte
// vectors along j (scalar when n % 4 != 0 or a pointer is not 16-byte aligned).
// Backward (gW = dL/dW):
//   dA[k][j] = s * sum_i B[i][k] gW[i][j]      dB[i][k] = s * sum_j gW[i][j] A[k][j]
// gW is read once: a workgroup stages a 64 x 64 tile of it in LDS and forms the tile's share of dA (reduced
// over its 64 rows) and of dB (reduced over its 64 columns) from it; a second launch sums the ceil(n / 64)
// shares of each element in tile order and scales by s.  No atomics: the same bits on every run.
#include "common.hpp"

namespace {

constexpr int KP = 68;  // LDS row pitch in floats: 16-byte aligned rows, consecutive rows 4 banks apart
constexpr int FI = 32, FJ = 128;
constexpr int BT = 64;
constexpr int LORA_MAX_R = 64;
constexpr int LORA_BWD_MAX_N = 16384;  // 2 * ceil(n / 64) * r * n workspace floats stay below 2^31

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

template <bool VEC>
__global__ __launch_bounds__(256) void lora_weight_fwd_kernel(int n, int r, const float* __restrict__ W0,
                                                              const float* __restrict__ A,
                                                              const float* __restrict__ Bm, float s,
                                                              float* __restrict__ W) {
  __shared__ __attribute__((aligned(16))) float As[LORA_MAX_R][FJ];
  __shared__ __attribute__((aligned(16))) float Bs[FI][KP];
  const int t = threadIdx.x, i0 = blockIdx.y * FI, j0 = blockIdx.x * FJ;
  const int r4 = (r + 3) & ~3;
  const int jq = t & 31, ig = t >> 5, j = j0 + 4 * jq;

  // this thread's W0 values first, so their latency runs under the LDS fill
  f32x4 w[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = i0 + ig + 8 * u;
    w[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i < n) {
      const float* p = W0 + (int64_t)i * n + j;
      if (VEC) {
        if (j < n) w[u] = ld4(p);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (j + c < n) w[u][c] = p[c];
      }
    }
  }
  if (VEC) {
    for (int idx = t; idx < r4 * (FJ / 4); idx += 256) {
      const int k = idx / (FJ / 4), q = idx % (FJ / 4), jj = j0 + 4 * q;
      st4(&As[k][4 * q], (k < r && jj < n) ? ld4(A + (int64_t)k * n + jj) : f32x4{0.f, 0.f, 0.f, 0.f});
    }
  } else {
    for (int idx = t; idx < r4 * FJ; idx += 256) {
      const int k = idx / FJ, jl = idx % FJ;
      As[k][jl] = (k < r && j0 + jl < n) ? A[(int64_t)k * n + j0 + jl] : 0.f;
    }
  }
  for (int idx = t; idx < FI * r4; idx += 256) {
    const int il = idx / r4, k = idx % r4;
    Bs[il][k] = (i0 + il < n && k < r) ? Bm[(int64_t)(i0 + il) * r + k] : 0.f;
  }
  __syncthreads();

  f32x4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < r4; k += 4) {
    f32x4 a[4], b[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = ld4(&As[k + c][4 * jq]);
#pragma unroll
    for (int u = 0; u < 4; ++u) b[u] = ld4(&Bs[ig + 8 * u][k]);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[u][e] = fmaf(b[u][c], a[c][e], acc[u][e]);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = i0 + ig + 8 * u;
    if (i >= n) continue;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fmaf(s, acc[u][e], w[u][e]);
    float* p = W + (int64_t)i * n + j;
    if (VEC) {
      if (j < n) st4(p, o);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (j + c < n) p[c] = o[c];
    }
  }
}

// One 64 x 64 tile of gW -> PA[blockIdx.y][k][j0..] (the tile's rows reduced) and PB[blockIdx.x][i0..][k]
// (its columns reduced).  A thread covers k = kq + 16 u, u < KT: KT = ceil(r / 16) rounded up to 1, 2 or 4.
template <int KT, bool VEC>
__global__ __launch_bounds__(256) void lora_weight_bwd_tile_kernel(int n, int r, const float* __restrict__ A,
                                                                   const float* __restrict__ Bm,
                                                                   const float* __restrict__ gW,
                                                                   float* __restrict__ PA, float* __restrict__ PB) {
  constexpr int RP = 16 * KT;
  __shared__ __attribute__((aligned(16))) float Gs[BT][KP];
  __shared__ __attribute__((aligned(16))) float As[RP][KP];
  __shared__ __attribute__((aligned(16))) float Bs[BT][KP];
  const int t = threadIdx.x, i0 = blockIdx.y * BT, j0 = blockIdx.x * BT;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    for (int idx = t; idx < BT * (BT / 4); idx += 256) {
      const int il = idx >> 4, q = idx & 15, i = i0 + il, j = j0 + 4 * q;
      st4(&Gs[il][4 * q], (i < n && j < n) ? ld4(gW + (int64_t)i * n + j) : zero);
    }
    for (int idx = t; idx < RP * (BT / 4); idx += 256) {
      const int k = idx >> 4, q = idx & 15, j = j0 + 4 * q;
      st4(&As[k][4 * q], (k < r && j < n) ? ld4(A + (int64_t)k * n + j) : zero);
    }
  } else {
    for (int idx = t; idx < BT * BT; idx += 256) {
      const int il = idx >> 6, jl = idx & 63, i = i0 + il, j = j0 + jl;
      Gs[il][jl] = (i < n && j < n) ? gW[(int64_t)i * n + j] : 0.f;
    }
    for (int idx = t; idx < RP * BT; idx += 256) {
      const int k = idx >> 6, jl = idx & 63, j = j0 + jl;
      As[k][jl] = (k < r && j < n) ? A[(int64_t)k * n + j] : 0.f;
    }
  }
  for (int idx = t; idx < BT * RP; idx += 256) {
    const int il = idx / RP, k = idx % RP;
    Bs[il][k] = (i0 + il < n && k < r) ? Bm[(int64_t)(i0 + il) * r + k] : 0.f;
  }
  __syncthreads();

  {  // dA share: rows of the tile reduced; thread = (k group kq, 4 columns jq)
    const int jq = t & 15, kq = t >> 4, j = j0 + 4 * jq;
    f32x4 acc[KT];
#pragma unroll
    for (int u = 0; u < KT; ++u) acc[u] = zero;
#pragma unroll 8
    for (int i = 0; i < BT; ++i) {
      const f32x4 g = ld4(&Gs[i][4 * jq]);
#pragma unroll
      for (int u = 0; u < KT; ++u) {
        const float b = Bs[i][kq + 16 * u];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[u][e] = fmaf(b, g[e], acc[u][e]);
      }
    }
#pragma unroll
    for (int u = 0; u < KT; ++u) {
      const int k = kq + 16 * u;
      if (k >= r) continue;
      float* p = PA + ((int64_t)blockIdx.y * r + k) * n + j;
      if (VEC) {
        if (j < n) st4(p, acc[u]);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (j + c < n) p[c] = acc[u][c];
      }
    }
  }
  {  // dB share: columns of the tile reduced; thread = (rows iq + 16 v, k group kq)
    const int kq = t & 15, iq = t >> 4;
    float acc[4][KT];
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int u = 0; u < KT; ++u) acc[v][u] = 0.f;
#pragma unroll 4
    for (int j4 = 0; j4 < BT; j4 += 4) {
      f32x4 g[4], a[KT];
#pragma unroll
      for (int v = 0; v < 4; ++v) g[v] = ld4(&Gs[iq + 16 * v][j4]);
#pragma unroll
      for (int u = 0; u < KT; ++u) a[u] = ld4(&As[kq + 16 * u][j4]);
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int u = 0; u < KT; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[v][u] = fmaf(g[v][e], a[u][e], acc[v][u]);
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = i0 + iq + 16 * v;
      if (i >= n) continue;
#pragma unroll
      for (int u = 0; u < KT; ++u) {
        const int k = kq + 16 * u;
        if (k < r) PB[((int64_t)blockIdx.x * n + i) * r + k] = acc[v][u];
      }
    }
  }
}

// dA and dB are both r * n floats and so is every share: out[e] = s * sum_t part[t][e], t ascending.
// blockIdx.y = 0: dA from PA, 1: dB from PB.
template <bool VEC>
__global__ __launch_bounds__(256) void lora_weight_bwd_sum_kernel(int64_t rn, int tiles, const float* __restrict__ PA,
                                                                  const float* __restrict__ PB, float s,
                                                                  float* __restrict__ dA, float* __restrict__ dB) {
  const float* part = blockIdx.y ? PB : PA;
  float* out = blockIdx.y ? dB : dA;
  if (VEC) {
    const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= rn) return;
    f32x4 acc = ld4(part + e);
    for (int z = 1; z < tiles; ++z) acc += ld4(part + (int64_t)z * rn + e);
    st4(out + e, acc * s);
  } else {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= rn) return;
    float acc = part[e];
    for (int z = 1; z < tiles; ++z) acc += part[(int64_t)z * rn + e];
    out[e] = acc * s;
  }
}

template <bool VEC>
void lora_bwd_tiles(int kt, dim3 grid, hipStream_t s, int n, int r, const float* A, const float* Bm,
                           const float* gW, float* PA, float* PB) {
  if (kt == 1)
    hipLaunchKernelGGL((lora_weight_bwd_tile_kernel<1, VEC>), grid, dim3(256), 0, s, n, r, A, Bm, gW, PA, PB);
  else if (kt == 2)
    hipLaunchKernelGGL((lora_weight_bwd_tile_kernel<2, VEC>), grid, dim3(256), 0, s, n, r, A, Bm, gW, PA, PB);
  else
    hipLaunchKernelGGL((lora_weight_bwd_tile_kernel<4, VEC>), grid, dim3(256), 0, s, n, r, A, Bm, gW, PA, PB);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

// W [n, n] = W0 + s * (B @ A); 1 <= r <= 64, n >= 1.
int vit_lora_weight_fwd(int n, int r, const float* W0, const float* A, const float* Bm, float scaling, float* W,
                        void* stream) {
  if (n < 1 || r < 1 || r > LORA_MAX_R) return (int)hipErrorInvalidValue;
  const int64_t gy = ((int64_t)n + FI - 1) / FI;
  if (gy > 65535) return (int)hipErrorInvalidValue;
  const dim3 grid((n + FJ - 1) / FJ, (unsigned)gy);
  hipStream_t s = (hipStream_t)stream;
  if (n % 4 == 0 && aligned16(W0) && aligned16(A) && aligned16(W))
    hipLaunchKernelGGL(lora_weight_fwd_kernel<true>, grid, dim3(256), 0, s, n, r, W0, A, Bm, scaling, W);
  else
    hipLaunchKernelGGL(lora_weight_fwd_kernel<false>, grid, dim3(256), 0, s, n, r, W0, A, Bm, scaling, W);
  VIT_CHECK_LAUNCH();
  return 0;
}

// Floats of workspace vit_lora_weight_bwd needs: the ceil(n / 64) shares of dA and of dB, r * n floats each.
// 0 for arguments the backward rejects.  Host only.
int vit_lora_weight_bwd_ws_floats(int n, int r) {
  if (n < 1 || n > LORA_BWD_MAX_N || r < 1 || r > LORA_MAX_R) return 0;
  const int64_t tiles = (n + BT - 1) / BT;
  return (int)(2 * tiles * r * n);
}

// dA [r, n] and dB [n, r] (overwritten) from gW = dL/dW [n, n]; ws >= vit_lora_weight_bwd_ws_floats(n, r)
// floats, 16-byte aligned.  1 <= r <= 64, 1 <= n <= 16384.
int vit_lora_weight_bwd(int n, int r, const float* A, const float* Bm, const float* gW, float scaling, float* dA,
                        float* dB, float* ws, void* stream) {
  if (n < 1 || n > LORA_BWD_MAX_N || r < 1 || r > LORA_MAX_R || ws == nullptr) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (n + BT - 1) / BT;
  const int64_t rn = (int64_t)r * n;
  float* PA = ws;
  float* PB = ws + tiles * rn;
  const int kt = r <= 16 ? 1 : r <= 32 ? 2 : 4;
  const dim3 grid(tiles, tiles);
  // PA rows start at multiples of n floats from ws: 16-byte aligned when n % 4 == 0 and ws is
  if (n % 4 == 0 && aligned16(gW) && aligned16(A) && aligned16(ws))
    lora_bwd_tiles<true>(kt, grid, s, n, r, A, Bm, gW, PA, PB);
  else
    lora_bwd_tiles<false>(kt, grid, s, n, r, A, Bm, gW, PA, PB);
  VIT_CHECK_LAUNCH();
  if (rn % 4 == 0 && aligned16(ws) && aligned16(dA) && aligned16(dB))
    hipLaunchKernelGGL(lora_weight_bwd_sum_kernel<true>, dim3((unsigned)((rn / 4 + 255) / 256), 2), dim3(256), 0, s,
                       rn, tiles, PA, PB, scaling, dA, dB);
  else
    hipLaunchKernelGGL(lora_weight_bwd_sum_kernel<false>, dim3((unsigned)((rn + 255) / 256), 2), dim3(256), 0, s, rn,
                       tiles, PA, PB, scaling, dA, dB);
  VIT_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
