// Scaled-dot-product attention for timm Attention: per (batch, head)
// softmax(q k^T * hd^-0.5) v, head_dim 64, any token count; unmasked or causal (the
// text tower's build_attention_mask: key > query gets -inf).  Up to 288 tokens (197
// for ViT-B/16, 257 for CLIP ViT-L/14, 77 for the CLIP text tower) the resident
// kernels below run; past 288 (384-pixel fine-tuning: 577, patch 8: 785) the
// streamed kernels (bf16 attn_*_stream, f32 attn_*_stream_f32), and for causal or
// misaligned operands the generic scalar kernels -- a causal streamed form is out of scope.
//
// q/k/v are read in place from the fused qkv GEMM output [B*N, 3*D] (row stride
// ld_qkv), the output o is written as [B*N, D] (the proj GEMM operand), and the
// backward writes dq/dk/dv into a [B*N, 3*D] buffer laid out like qkv so the
// qkv dgrad/wgrad GEMMs consume it directly.
//
// resident bf16 path: one workgroup (4 waves) per (b, h); the whole K and V of the head
// live in LDS (<= 2 x 36 KiB); S^T = K Q^T with v_mfma_f32_16x16x32_bf16 so each
// lane owns one query column and the softmax row-max/row-sum are in-lane plus two
// cross-lane shuffles; P stays in registers and feeds the PV MFMA as its
// B-operand (k-slot permutation pi), V^T comes from ds_read_b64_tr_b16.
// f32 path (parity mode): scalar-FMA online softmax.
// resident f32 path, "high" (vit_sdpa_f32_precision(1), opt-in): the bf16 path's algebra on hi / lo bf16 splits of the
// f32 operands, three MFMA products a product (attn_*_f32x3; see the block in front of F32X3).
// streamed f32 path, "high" + long (vit_sdpa_f32_long_precision(1) as well, opt-in): the same split on the streamed
// schedule (attn_*_stream_x3; see the block in front of SX_BUF).
// one-query path (attn_cls1_*, the CLIP visual tower's class-token tail): query row 0 of every image alone,
// K / V straight from HBM to registers, no MFMA -- see the block in front of attn_cls1_fwd; attn_row1_fwd is the
// same forward at a row per sequence, causal or not (the CLIP text tower's EOT tail).
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <type_traits>

#include "bf16_split.hpp"
#include "common.hpp"
#include "reduce.hpp"

extern "C" int vit_colsum(int dtype, int M, int N, const void* X, int64_t ld, float* out, float* partial,
                          int64_t partial_floats, int accumulate, void* stream);

// 128-B row image with XOR swizzle (row & 6) on 16-B chunks: conflict-free for
// the 16x16x32 ds_read_b128 fragment reads and for the ds_read_b64_tr_b16 reads
// of 8 consecutive rows (LDS images).
__device__ __forceinline__ int at_off(int row, int c) { return row * 128 + ((c ^ (row & 6)) << 4); }

// Load rows [0, N) of NM head slices (64 wide) into LDS images of ROWS rows,
// zero-filling rows >= N.  All global loads of the thread are issued before the
// first LDS write (one latency, not one per chunk); rows >= N load a clamped
// valid row and are zeroed in registers.
template <int ROWS, int NTHR, int NM>
__device__ __forceinline__ void at_load(char* const (&img)[NM], const bf16* const (&src)[NM],
                                        const int64_t (&ld)[NM], int N) {
  constexpr int TOTAL = ROWS * 8, PER = (TOTAL + NTHR - 1) / NTHR;
  bf16x8 v[NM][PER];
#pragma unroll
  for (int mtx = 0; mtx < NM; ++mtx)
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = threadIdx.x + u * NTHR;
      const int row = min(idx >> 3, N - 1), c = idx & 7;
      if (idx < TOTAL) v[mtx][u] = *reinterpret_cast<const bf16x8*>(src[mtx] + (int64_t)row * ld[mtx] + c * 8);
    }
#pragma unroll
  for (int mtx = 0; mtx < NM; ++mtx)
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = threadIdx.x + u * NTHR;
      const int row = idx >> 3, c = idx & 7;
      if (idx < TOTAL) {
        bf16x8 w = v[mtx][u];
        if (row >= N) {
#pragma unroll
          for (int t = 0; t < 8; ++t) w[t] = (bf16)0.f;
        }
        *reinterpret_cast<bf16x8*>(img[mtx] + at_off(row, c)) = w;
      }
    }
}

constexpr int AT_THREADS = 512;  // 8 waves per (batch, head)
constexpr int AT_WAVES = AT_THREADS / 64;

__device__ __forceinline__ bf16x8 pack8(const f32x4& a, const f32x4& b) {
  return bf16x8{(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
}

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

// ---------------------------------------------------------------------------
// Per-lane LDS offsets.  Tiles start at multiples of 16 (row fragments) or 32
// (transposed fragments) rows, which leaves (row & 6) -- the swizzle -- a
// function of the lane only, so every fragment address is a lane constant plus
// a wave-uniform tile offset (row0 * 128).
// ---------------------------------------------------------------------------
struct AtOffsets {
  int row[2];   // row fragment, k-substep kk (d 0..31 / 32..63)
  int tr[4];    // transposed fragment, d-tile dt, rows 4g+q (+16 rows: + 2048)
  __device__ __forceinline__ AtOffsets(int lane) {
    const int l15 = lane & 15, g = lane >> 4, q = l15 >> 2, p = l15 & 3;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) row[kk] = l15 * 128 + (((kk * 4 + g) ^ (l15 & 6)) << 4);
    const int ra = 4 * g + q;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) tr[dt] = ra * 128 + (((2 * dt + (p >> 1)) ^ (ra & 6)) << 4) + (p & 1) * 8;
  }
};
__device__ __forceinline__ bf16x8 rowf(const char* img, int row0, int off) {
  return *reinterpret_cast<const bf16x8*>(img + row0 * 128 + off);
}
__device__ __forceinline__ bf16x8 trf(const char* img, int row0, int off) {
  const char* b = img + row0 * 128 + off;
  return cat4(lds_read_tr(b), lds_read_tr(b + 16 * 128));
}
// Operand policies of the resident tile steps (at_dq_step, at_dkv_step): how a head image is named, what an MFMA
// operand is, how an f32 accumulator pair becomes one, and how a product is issued.
struct AtBf16 {  // bf16 operands, one product
  static constexpr bool SPLIT = false;
  using Img = const char*;
  using Frag = bf16x8;
  static __device__ __forceinline__ Frag row(Img m, int row0, int off) { return rowf(m, row0, off); }
  static __device__ __forceinline__ Frag tr(Img m, int row0, int off) { return trf(m, row0, off); }
  static __device__ __forceinline__ Frag pack(const f32x4& a, const f32x4& b) { return pack8(a, b); }
  static __device__ __forceinline__ f32x4 mma(const Frag& a, const Frag& b, f32x4 c) { return mfma16(a, b, c); }
};
struct AtBf16x3 {  // f32 operands as hi / lo bf16 splits (bf16_split.hpp), three products: hi lo, lo hi, hi hi
  static constexpr bool SPLIT = true;
  struct Img { const char *hi, *lo; };
  struct Frag { bf16x8 hi, lo; };
  static __device__ __forceinline__ Frag row(Img m, int row0, int off) {
    return {rowf(m.hi, row0, off), rowf(m.lo, row0, off)};
  }
  static __device__ __forceinline__ Frag tr(Img m, int row0, int off) {
    return {trf(m.hi, row0, off), trf(m.lo, row0, off)};
  }
  static __device__ __forceinline__ Frag pack(const f32x4& a, const f32x4& b) {
    Frag f;
    split8<1>(a, b, f.hi, f.lo);
    return f;
  }
  static __device__ __forceinline__ f32x4 mma(const Frag& a, const Frag& b, f32x4 c) {
    c = mfma16(a.hi, b.lo, c);
    c = mfma16(a.lo, b.hi, c);
    return mfma16(a.hi, b.hi, c);
  }
};
__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// Diagnostic phase stamps (tools/attn_stamps.py): a separate template instance, launched only
// while vit_debug_attn_stamps() has set a buffer.  Thread 0 of a workgroup records s_memtime at
// phase boundaries and s_memrealtime at start / end into stamps[blockIdx.x * 8 + i].
static unsigned long long* g_attn_stamps = nullptr;
#define AT_STAMP(i)                                                   \
  if constexpr (STAMP) { if (threadIdx.x == 0) st[i] = __builtin_amdgcn_s_memtime(); }
#define AT_STAMP_BEGIN()                                                                          \
  unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                            \
  if constexpr (STAMP) { if (threadIdx.x == 0) st[5] = __builtin_amdgcn_s_memrealtime(); }        \
  AT_STAMP(0)
#define AT_STAMP_FLUSH()                                                                         \
  if constexpr (STAMP) if (threadIdx.x == 0) {                                                   \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                             \
    st[6] = __builtin_amdgcn_s_memtime();                                                        \
    st[7] = __builtin_amdgcn_s_memrealtime();                                                    \
    unsigned long long* d = stamps + (int64_t)blockIdx.x * 8;                                    \
    for (int i_ = 0; i_ < 8; ++i_) d[i_] = st[i_];                                               \
  }

// ---------------------------------------------------------------------------
// bf16 forward
// ---------------------------------------------------------------------------
// CLS (the class-token tail's last block: only query 0 of each head is read): query tile 0 alone, on the
// same arithmetic, so o and lse of rows 0..15 keep their bits; the rows that are not computed get o = 0 and
// lse = +inf, so a backward over them sees p = exp(s - inf) = 0 and delta = 0 exactly.
template <int NT, bool STAMP = false, bool CAUSAL = false, bool CLS = false>  // key/query tiles of 16: NT = ceil(N/16)
__global__ __launch_bounds__(AT_THREADS, NT <= 14 ? 4 : 2) void attn_fwd_mfma(const bf16* __restrict__ qkv, int64_t ld_qkv, int D,
                                                     int H, int N, float scale, bf16* __restrict__ o,
                                                     int64_t ld_o, float* __restrict__ lse, int causal,
                                                     unsigned long long* __restrict__ stamps) {
  AT_STAMP_BEGIN()
  constexpr int NT2 = (NT + 1) / 2, ROWS = NT2 * 32;
  __shared__ __attribute__((aligned(16))) char smem[2 * ROWS * 128];
  char* Kimg = smem;
  char* Vimg = smem + ROWS * 128;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  const bf16* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  {
    char* const imgs[2] = {Kimg, Vimg};
    const bf16* const srcs[2] = {base + D, base + 2 * D};
    const int64_t lds_[2] = {ld_qkv, ld_qkv};
    at_load<ROWS, AT_THREADS, 2>(imgs, srcs, lds_, N);
  }
  const AtOffsets off(lane);
  __syncthreads();
  AT_STAMP(1)
  const float c2 = scale * LOG2E;
  if constexpr (CLS) {
    for (int i = 16 * 16 + threadIdx.x; i < N * 16; i += AT_THREADS)  // rows 16 .. N - 1: 16 pieces of 4
      *reinterpret_cast<bf16x4*>(o + ((int64_t)b * N + (i >> 4)) * ld_o + h * 64 + (i & 15) * 4) =
          bf16x4{(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
    for (int r = 16 + threadIdx.x; r < N; r += AT_THREADS) lse[(int64_t)bh * N + r] = INFINITY;
  }
  for (int qt = wave; qt < (CLS ? 1 : NT); qt += AT_WAVES) {
    const int q = qt * 16 + (lane & 15);
    bf16x8 qf[2];
    {
      const int qq = min(q, N - 1);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) qf[kk] = *reinterpret_cast<const bf16x8*>(base + (int64_t)qq * ld_qkv + kk * 32 + g * 8);
    }
    f32x4 s[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) s[kt] = mfma16(rowf(Kimg, kt * 16, off.row[kk]), qf[kk], s[kt]);
      if (kt % 4 == 3) __builtin_amdgcn_sched_barrier(0);  // bound K-fragment hoisting (VGPRs)
    }
    // keys >= N exist only in the last tile
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if ((NT - 1) * 16 + 4 * g + r >= N) s[NT - 1][r] = -INFINITY;
    if constexpr (CAUSAL) {  // key > query masked (CLIP text tower attn_mask); key 0 always survives
#pragma unroll
      for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kt * 16 + 4 * g + r > q) s[kt][r] = -INFINITY;
    }
    // row max / sum as 4 independent chains (one per accumulator slot r): a single chain over
    // the 4*NT scores is a 52-deep dependent VALU sequence at N = 197
    float mr[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) mr[r] = fmaxf(mr[r], s[kt][r]);
    float m = fmaxf(fmaxf(mr[0], mr[1]), fmaxf(mr[2], mr[3]));
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float mc = m * c2;
    float lr[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) { float p = fexp2(fmaf(s[kt][r], c2, -mc)); s[kt][r] = p; lr[r] += p; }
    float l = (lr[0] + lr[1]) + (lr[2] + lr[3]);
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    f32x4 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NT2; ++ks) {
      f32x4 hi = (2 * ks + 1 < NT) ? s[2 * ks + 1 < NT ? 2 * ks + 1 : 0] : f32x4{0.f, 0.f, 0.f, 0.f};
      bf16x8 pf = pack8(s[2 * ks], hi);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) oacc[dt] = mfma16(trf(Vimg, ks * 32, off.tr[dt]), pf, oacc[dt]);
      if (ks % 2 == 1) __builtin_amdgcn_sched_barrier(0);  // bound V-fragment hoisting (VGPRs)
    }
    if (q < N) {
      const float inv = 1.0f / l;
      bf16* orow = o + ((int64_t)b * N + q) * ld_o + h * 64;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        bf16x4 ov = {(bf16)(oacc[dt][0] * inv), (bf16)(oacc[dt][1] * inv), (bf16)(oacc[dt][2] * inv),
                     (bf16)(oacc[dt][3] * inv)};
        *reinterpret_cast<bf16x4*>(orow + dt * 16 + 4 * g) = ov;
      }
      if (g == 0) lse[(int64_t)bh * N + q] = (mc + __log2f(l)) * LN2;
    }
  }
  AT_STAMP(2)
  AT_STAMP_FLUSH()
}


// ---------------------------------------------------------------------------
// fp8 forward (BASELINE configs[4]: the perturbation sweep's frozen-tower attention and the RSA
// evaluation forward).  Block-scaled OCP e4m3 operands on v_mfma_scale_f32_32x32x64_f8f6f4
// (twice the bf16 MFMA rate per clock), operand layouts probed with exact one-hot data
// (tools/probe/mfma_scale_probe.hip): lane l holds A[row l%32][k = 32(l/32) + byte] and
// B[k = 32(l/32) + byte][col l%32]; its E8M0 scale byte covers those 32 k values.
//
//   S^T = K Q^T: A = K (rows = keys, k = d), B = Q^T; one MFMA per 32-key tile (hd = 64 = K).
//     Q and K are quantised per row (all 64 d): e = the smallest exponent with
//     max|x| <= 448 * 2^e, byte = x * 2^-e rounded to e4m3, E8M0 scale 127 + e in both lane halves
//     of the row.  (One scale per row, not per 32 values: the hardware's 32-value scale blocks
//     interleave the two lane halves' bytes -- tools/probe/mfma_scale_probe.hip, test 6.)
//   P = exp(S - rowmax) in (0, 1], quantised as P * 2^8 (scale 2^-8): no block max needed.
//   O^T = V^T P^T: A = V^T (rows = d, k = keys), B = P^T straight from the S^T accumulators:
//     lane half h holds keys 4h + (r&3) + 8(r>>2) of each 32-key tile (the 32x32 C layout), so
//     the MFMA's k slots are permuted the same way for both operands; V is quantised per
//     (d, 64-key tile) into a transposed [d][keys] LDS image read 4 keys at a time.
// One workgroup (8 waves) per (b, h); each wave takes 32-query tiles.  Softmax statistics, the
// row sum and the output scaling stay f32; o is written bf16, lse f32 (natural log).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int e8m0_exp(float amax) {
  // smallest e with amax <= 448 * 2^e (448 = 1.75 * 2^8), clamped to the E8M0 range
  const uint32_t bits = __float_as_uint(amax);
  const int E = (int)((bits >> 23) & 255) - 127;
  if (((bits >> 23) & 255) == 0) return -127;  // 0 / denormal
  const int e = (bits & 0x7fffff) <= 0x600000 ? E - 8 : E - 7;
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}
__device__ __forceinline__ float inv_exp2i(int e) {  // 2^-e, exact for e in [-127, 126]
  return e >= 127 ? 0.f : __uint_as_float((uint32_t)(e == -127 ? 254 : 127 - e) << 23);
}
// 4 floats -> 4 e4m3 bytes (round to nearest even; |x| <= 448 by construction)
__device__ __forceinline__ int pack_fp8x4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
}
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int F8_THREADS = 512, F8_WAVES = 8;
__device__ __forceinline__ int f8_koff(int key, int c) { return key * 64 + ((c ^ ((key >> 2) & 1)) << 4); }

template <typename T> __device__ __forceinline__ void load8f(const T* p, float* x);
template <> __device__ __forceinline__ void load8f<bf16>(const bf16* p, float* x) {
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int u = 0; u < 8; ++u) x[u] = (float)v[u];
}
template <> __device__ __forceinline__ void load8f<float>(const float* p, float* x) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int u = 0; u < 4; ++u) { x[u] = a[u]; x[4 + u] = b[u]; }
}

// One 64-key tile of the fp8 online softmax, stated once for attn_fwd_fp8 (the tile inside the head's resident
// images) and attn_fwd_fp8_stream (the chunk in the ring buffer): the two S^T MFMAs, the mask, the max / alpha /
// exp2 update, the P pack and the two PV MFMAs.  Kt: the tile's 64 K rows (f8_koff layout), ksc: its 128 row-scale
// bytes; Vt: the V^T image at the tile's key 0, rows vrow bytes apart; vsc[d * vsc_ld]: the tile's V scale bytes.
// key0: the tile's first key, counted from key 0 of the head (mask only).  This lane: query q, lane half h.
__device__ __forceinline__ void f8_tile_step(const unsigned char* Kt, const unsigned char* ksc, const unsigned char* Vt,
                                             int vrow, const unsigned char* vsc, int vsc_ld, int key0, int N, int q,
                                             int causal, const i32x8& qf, int qsc, float c2, int h, int l31, float& m,
                                             float& l, f32x16 (&oacc)[2]) {
  f32x16 s[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int key = u * 32 + l31;
    typedef int i32x4_ __attribute__((ext_vector_type(4)));
    const i32x4_ lo = *reinterpret_cast<const i32x4_*>(Kt + f8_koff(key, 2 * h));
    const i32x4_ hi = *reinterpret_cast<const i32x4_*>(Kt + f8_koff(key, 2 * h + 1));
    const i32x8 kf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    f32x16 z = {};
    s[u] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf, qf, z, 0, 0, 0, ksc[key * 2 + h], 0, qsc);
  }
  // rows of s[u]: key key0 + u*32 + 4h + (r&3) + 8(r>>2); column: query q.  The mask (key >= N, causal: key > q)
  // compares each row's constant part with two per-tile limits, so no per-row key lives in a register
  const int lim_n = N - key0 - 4 * h, lim_q = causal ? q - key0 - 4 * h : 64;
  float mt = -INFINITY;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kr = u * 32 + (r & 3) + 8 * (r >> 2);
      if (kr >= lim_n || kr > lim_q) s[u][r] = -INFINITY;
      mt = fmaxf(mt, s[u][r]);
    }
  mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
  const float mn = fmaxf(m, mt);  // finite from the first tile on: key 0 is never masked
  const float alpha = fexp2((m - mn) * c2);  // first tile: m = -inf -> 0
  m = mn;
  const float mc = m * c2;
  l *= alpha;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) oacc[dt] *= alpha;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = fexp2(fmaf(s[u][r], c2, -mc));
      s[u][r] = p;
      l += p;
    }
  i32x8 pf;  // P^T fragment: byte j = tile (j/16), register j%16, times 2^8
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    const f32x16& t = s[w >> 2];
    const int r = 4 * (w & 3);
    pf[w] = pack_fp8x4(t[r] * 256.f, t[r + 1] * 256.f, t[r + 2] * 256.f, t[r + 3] * 256.f);
  }
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    const int d = dt * 32 + l31;
    const unsigned char* row = Vt + d * vrow + 4 * h;
    i32x8 vf;
#pragma unroll
    for (int w = 0; w < 8; ++w) vf[w] = *reinterpret_cast<const int*>(row + (w >> 2) * 32 + 8 * (w & 3));
    oacc[dt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf, pf, oacc[dt], 0, 0, 0, vsc[d * vsc_ld], 0, 127 - 8);
  }
}

// The Q^T fragment of query row qrow (its 64 head dims at src0): this lane's 32 d values (block h), one E8M0
// scale for the row across both lane halves.
template <typename T>
__device__ __forceinline__ void f8_q_frag(const T* src0, int h, i32x8& qf, int& qsc) {
  const T* src = src0 + h * 32;
  float x[32];
#pragma unroll
  for (int c = 0; c < 4; ++c) load8f<T>(src + c * 8, x + c * 8);
  float amax = 0.f;
#pragma unroll
  for (int u = 0; u < 32; ++u) amax = fmaxf(amax, fabsf(x[u]));
  amax = fmaxf(amax, __shfl_xor(amax, 32, 64));  // the query's other lane half: one scale per row
  const int e = e8m0_exp(amax);
  const float inv = inv_exp2i(e);
#pragma unroll
  for (int u = 0; u < 8; ++u) qf[u] = pack_fp8x4(x[4 * u] * inv, x[4 * u + 1] * inv, x[4 * u + 2] * inv, x[4 * u + 3] * inv);
  qsc = e + 127;
}

// Writing o and lse of one 32-query tile, for both fp8 kernels: oacc holds O^T (rows d, column query q).
template <typename T>
__device__ __forceinline__ void f8_store(T* orow, float* lse_q, const f32x16 (&oacc)[2], float l, float mc, int h) {
  const float inv = 1.0f / l;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int mq = 0; mq < 4; ++mq) {
      const int d = dt * 32 + 4 * h + 8 * mq;
      const f32x4 ov = {oacc[dt][4 * mq] * inv, oacc[dt][4 * mq + 1] * inv, oacc[dt][4 * mq + 2] * inv,
                        oacc[dt][4 * mq + 3] * inv};
      if constexpr (sizeof(T) == 2) *reinterpret_cast<bf16x4*>(orow + d) = bf16x4{(bf16)ov[0], (bf16)ov[1], (bf16)ov[2], (bf16)ov[3]};
      else *reinterpret_cast<f32x4*>(orow + d) = ov;
    }
  if (h == 0 && lse_q) *lse_q = (mc + __log2f(l)) * LN2;
}

template <int NKT, typename T>  // 64-key tiles: keys padded to NKT * 64; T = the qkv / o dtype
__global__ __launch_bounds__(F8_THREADS, 2) void attn_fwd_fp8(const T* __restrict__ qkv, int64_t ld_qkv, int D,
                                                             int H, int N, float scale, T* __restrict__ o,
                                                             int64_t ld_o, float* __restrict__ lse, int causal) {
  constexpr int KEYS = NKT * 64, VROW = KEYS + 4;  // V^T rows padded: conflict-free transposed writes
  __shared__ __attribute__((aligned(16))) unsigned char Kimg[KEYS * 64];
  __shared__ __attribute__((aligned(16))) unsigned char Vt[64 * VROW];
  __shared__ unsigned char Ksc[KEYS * 2];
  __shared__ unsigned char Vsc[64 * NKT];
  const int bh = blockIdx.x, b = bh / H, hh = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* base = qkv + (int64_t)b * N * ld_qkv + hh * 64;

  // K: two adjacent lanes per key (one 32-wide d half each), one scale per key row
  for (int t = threadIdx.x; t < KEYS * 2; t += F8_THREADS) {
    const int key = t >> 1, half = t & 1;
    float x[32];
    if (key < N) {
      const T* src = base + (int64_t)key * ld_qkv + D + half * 32;
#pragma unroll
      for (int c = 0; c < 4; ++c) load8f<T>(src + c * 8, x + c * 8);
    } else {
#pragma unroll
      for (int u = 0; u < 32; ++u) x[u] = 0.f;
    }
    float amax = 0.f;
#pragma unroll
    for (int u = 0; u < 32; ++u) amax = fmaxf(amax, fabsf(x[u]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));  // the row's other half (KEYS * 2 is a multiple of 64)
    const int e = e8m0_exp(amax);
    const float inv = inv_exp2i(e);
    int w[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) w[u] = pack_fp8x4(x[4 * u] * inv, x[4 * u + 1] * inv, x[4 * u + 2] * inv, x[4 * u + 3] * inv);
    typedef int i32x4_ __attribute__((ext_vector_type(4)));
    *reinterpret_cast<i32x4_*>(Kimg + f8_koff(key, 2 * half)) = i32x4_{w[0], w[1], w[2], w[3]};
    *reinterpret_cast<i32x4_*>(Kimg + f8_koff(key, 2 * half + 1)) = i32x4_{w[4], w[5], w[6], w[7]};
    Ksc[key * 2 + half] = (unsigned char)(e + 127);
  }
  // V: wave per 64-key tile, lane = d
  for (int kt = wave; kt < NKT; kt += F8_WAVES) {
    float x[64];
    const T* src = base + 2 * D + lane;
#pragma unroll
    for (int u = 0; u < 64; ++u) {
      const int key = kt * 64 + u;
      x[u] = key < N ? (float)src[(int64_t)key * ld_qkv] : 0.f;
    }
    float amax = 0.f;
#pragma unroll
    for (int u = 0; u < 64; ++u) amax = fmaxf(amax, fabsf(x[u]));
    const int e = e8m0_exp(amax);
    const float inv = inv_exp2i(e);
#pragma unroll
    for (int u = 0; u < 16; ++u)
      *reinterpret_cast<int*>(Vt + lane * VROW + kt * 64 + 4 * u) =
          pack_fp8x4(x[4 * u] * inv, x[4 * u + 1] * inv, x[4 * u + 2] * inv, x[4 * u + 3] * inv);
    Vsc[lane * NKT + kt] = (unsigned char)(e + 127);
  }
  __syncthreads();

  const float c2 = scale * LOG2E;
  const int h = lane >> 5, l31 = lane & 31;
  const int nqt = (N + 31) / 32;
  for (int qt = wave; qt < nqt; qt += F8_WAVES) {
    const int q = qt * 32 + l31;
    // Q^T fragment: this lane's 32 d values (block h) of query q
    i32x8 qf;
    int qsc;
    f8_q_frag<T>(base + (int64_t)min(q, N - 1) * ld_qkv, h, qf, qsc);
    // online softmax over 64-key tiles (two S^T MFMAs each): only one tile's scores are live
    float m = -INFINITY, l = 0.f;
    f32x16 oacc[2] = {};
#pragma unroll 1
    for (int kt = 0; kt < NKT; ++kt)
      f8_tile_step(Kimg + kt * 64 * 64, Ksc + kt * 128, Vt + kt * 64, VROW, Vsc + kt, NKT, kt * 64, N, q, causal, qf, qsc,
                   c2, h, l31, m, l, oacc);
    l += __shfl_xor(l, 32, 64);
    const float mc = m * c2;
    if (q < N)
      f8_store<T>(o + ((int64_t)b * N + q) * ld_o + hh * 64, lse ? lse + (int64_t)bh * N + q : nullptr, oacc, l, mc, h);
  }
}

// ---------------------------------------------------------------------------
// Streamed fp8 forward: attn_fwd_fp8's quantisation, MFMAs and online softmax (f8_tile_step) with no bound on
// N.  K and V pass through a two-buffer LDS ring of 64-key chunks instead of living there whole.
//   grid (B*H, ceil(N / 256)), 8 waves: a wave owns one 32-query tile, its Q fragment quantised once and kept in
//   registers.  Per chunk (attn_fwd_stream's schedule): the next chunk's global loads are issued first, the
//   tile step on the current chunk runs under their latency, then all 512 threads quantise the loaded pieces
//   into the other buffer; one barrier per chunk.  The f32 form requests only K's piece before the step and V's
//   after it, ahead of K's quantisation: with 16 loaded registers in flight over the step it spilled at the 128
//   VGPRs that two workgroups per CU allow (launch bound 4 waves per SIMD); bf16's pieces are 8 registers.
//   The step sits in its own `live` branch on purpose: as straight-line code the scheduler interleaved it with
//   the quantisation and the kernel needed 156 (bf16) / 164 (f32) VGPRs instead of 125.
//   A chunk is 64 keys, not 128: it is then exactly one of V's scale blocks (counted from key 0 of the head, as
//   the resident kernel counts them) and one 16-B (bf16) piece of K and of V per thread, so both quantisations
//   finish inside a wave -- K's row maximum over the 8 adjacent lanes of a key, V's block maximum over the 64
//   lanes (keys) of the wave that holds 8 head dims -- and the buffer that is being written needs no second barrier.
//   Buffer: Kimg (f8_koff) 4 KiB | V^T 64 rows of 64 + 4 bytes | 128 K scale bytes | 64 V scale bytes = 8640 B.
// Keys past N: loaded from row N - 1 and zeroed in registers (at_load's rule), masked to -inf in the step.
// Every wave runs every chunk and every barrier; a wave whose 32 queries all lie past N skips only the tile
// steps and the stores (`live` is wave-uniform, `more` workgroup-uniform, no barrier sits under either).
// The max is exact in any order and every other operation is the resident kernel's, in its order: up to 320
// tokens o and lse are bit for bit attn_fwd_fp8's.
// ---------------------------------------------------------------------------
constexpr int F8S_CH = 64;                // keys per chunk = V's scale block
constexpr int F8S_QB = F8_WAVES * 32;     // queries per workgroup
constexpr int F8S_VROW = F8S_CH + 4;      // V^T row pitch: the resident kernel's +4 padding
constexpr int F8S_VT = F8S_CH * 64;       // buffer offsets: V^T image, K scales, V scales
constexpr int F8S_KSC = F8S_VT + 64 * F8S_VROW;
constexpr int F8S_VSC = F8S_KSC + F8S_CH * 2;
constexpr int F8S_BUF = (F8S_VSC + 64 + 15) / 16 * 16;
static_assert(F8S_CH * 8 == F8_THREADS, "one 8-value piece of a chunk's K and of its V per thread");
static_assert(F8_WAVES * 8 == 64, "a wave quantises 8 head dims of V");

template <typename T> struct F8Raw;  // 8 values of a row as loaded, converted only when they are quantised
template <> struct F8Raw<bf16> {
  bf16x8 v;
  __device__ __forceinline__ void load(const bf16* p) { v = *reinterpret_cast<const bf16x8*>(p); }
  __device__ __forceinline__ void get(float* x, bool zero) const {
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = zero ? 0.f : (float)v[u];
  }
};
template <> struct F8Raw<float> {
  f32x4 a, b;
  __device__ __forceinline__ void load(const float* p) {
    a = *reinterpret_cast<const f32x4*>(p);
    b = *reinterpret_cast<const f32x4*>(p + 4);
  }
  __device__ __forceinline__ void get(float* x, bool zero) const {
#pragma unroll
    for (int u = 0; u < 4; ++u) { x[u] = zero ? 0.f : a[u]; x[4 + u] = zero ? 0.f : b[u]; }
  }
};
template <typename T> struct F8Piece { F8Raw<T> k, v; };

// this thread's pieces of keys [j0, j0 + 64), rows clamped to N - 1.  K: key j0 + tid / 8, head dims 8 (tid % 8) ..;
// V: key j0 + lane, head dims 8 wave ..
template <typename T>
__device__ __forceinline__ void f8s_fetch_k(F8Piece<T>& p, const T* base, int64_t ld_qkv, int D, int j0, int N) {
  const int tid = threadIdx.x;
  p.k.load(base + (int64_t)min(j0 + (tid >> 3), N - 1) * ld_qkv + D + (tid & 7) * 8);
}
template <typename T>
__device__ __forceinline__ void f8s_fetch_v(F8Piece<T>& p, const T* base, int64_t ld_qkv, int D, int j0, int N) {
  const int tid = threadIdx.x;
  p.v.load(base + (int64_t)min(j0 + (tid & 63), N - 1) * ld_qkv + 2 * D + (tid >> 6) * 8);
}
// quantise the pieces into buffer buf: attn_fwd_fp8's bytes and scale bytes for these keys
template <typename T>
__device__ __forceinline__ void f8s_commit(unsigned char* buf, const F8Piece<T>& p, int j0, int N) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float x[8];
  {  // K: 8 adjacent lanes hold a key's row
    const int key = tid >> 3, c = tid & 7;
    p.k.get(x, j0 + key >= N);
    float amax = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) amax = fmaxf(amax, fabsf(x[u]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 4, 64));
    const int e = e8m0_exp(amax);
    const float inv = inv_exp2i(e);
    typedef int i32x2_ __attribute__((ext_vector_type(2)));
    *reinterpret_cast<i32x2_*>(buf + f8_koff(key, c >> 1) + (c & 1) * 8) =
        i32x2_{pack_fp8x4(x[0] * inv, x[1] * inv, x[2] * inv, x[3] * inv),
               pack_fp8x4(x[4] * inv, x[5] * inv, x[6] * inv, x[7] * inv)};
    if ((c & 3) == 0) buf[F8S_KSC + key * 2 + (c >> 2)] = (unsigned char)(e + 127);
  }
  {  // V: this lane's key, head dims 8 wave + i; the block maximum of each d over the wave's 64 keys
    p.v.get(x, j0 + lane >= N);
    // halve the values in flight at each of the first three exchanges: 7 shuffles, after which this lane holds
    // the maximum of d = lane / 8 over the lanes that differ from it in bits 3..5; 3 more finish it
    const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
    float w4[4], w2[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float keep = fabsf(b5 ? x[4 + i] : x[i]), send = fabsf(b5 ? x[i] : x[4 + i]);
      w4[i] = fmaxf(keep, __shfl_xor(send, 32, 64));
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float keep = b4 ? w4[2 + i] : w4[i], send = b4 ? w4[i] : w4[2 + i];
      w2[i] = fmaxf(keep, __shfl_xor(send, 16, 64));
    }
    float t = fmaxf(b3 ? w2[1] : w2[0], __shfl_xor(b3 ? w2[0] : w2[1], 8, 64));
    t = fmaxf(t, __shfl_xor(t, 4, 64));
    t = fmaxf(t, __shfl_xor(t, 2, 64));
    t = fmaxf(t, __shfl_xor(t, 1, 64));
    const int e = e8m0_exp(t);
    if ((lane & 7) == 0) buf[F8S_VSC + wave * 8 + (lane >> 3)] = (unsigned char)(e + 127);
    const int inv_bits = __float_as_int(inv_exp2i(e));  // of d = lane / 8: lane 8 i holds head dim i's
    float y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = x[i] * __int_as_float(__builtin_amdgcn_readlane(inv_bits, 8 * i));
    const int w0 = pack_fp8x4(y[0], y[1], y[2], y[3]), w1 = pack_fp8x4(y[4], y[5], y[6], y[7]);
    unsigned char* col = buf + F8S_VT + (wave * 8) * F8S_VROW + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      col[i * F8S_VROW] = (unsigned char)(w0 >> (8 * i));
      col[(4 + i) * F8S_VROW] = (unsigned char)(w1 >> (8 * i));
    }
  }
}

template <typename T>
__global__ __launch_bounds__(F8_THREADS, 4) void attn_fwd_fp8_stream(const T* __restrict__ qkv, int64_t ld_qkv, int D,
                                                                    int H, int N, float scale, T* __restrict__ o,
                                                                    int64_t ld_o, float* __restrict__ lse,
                                                                    int causal) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][F8S_BUF];
  const int bh = blockIdx.x, b = bh / H, hh = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* base = qkv + (int64_t)b * N * ld_qkv + hh * 64;
  const int h = lane >> 5, l31 = lane & 31;
  const int q0 = blockIdx.y * F8S_QB + wave * 32, q = q0 + l31;
  i32x8 qf;
  int qsc;
  f8_q_frag<T>(base + (int64_t)min(q, N - 1) * ld_qkv, h, qf, qsc);
  const int nc = (N + F8S_CH - 1) / F8S_CH;
  F8Piece<T> pc;
  f8s_fetch_k<T>(pc, base, ld_qkv, D, 0, N);
  f8s_fetch_v<T>(pc, base, ld_qkv, D, 0, N);
  f8s_commit<T>(smem[0], pc, 0, N);
  __syncthreads();
  const float c2 = scale * LOG2E;
  float m = -INFINITY, l = 0.f;
  f32x16 oacc[2] = {};
  const bool live = q0 < N;  // wave-uniform; the trip count below does not depend on it
  constexpr bool V_EARLY = sizeof(T) == 2;
#pragma unroll 1
  for (int c = 0; c < nc; ++c) {
    const unsigned char* buf = smem[c & 1];
    const int j0 = c * F8S_CH;
    const bool more = c + 1 < nc;  // the same in every wave of the workgroup
    if (more) {
      f8s_fetch_k<T>(pc, base, ld_qkv, D, j0 + F8S_CH, N);
      if constexpr (V_EARLY) f8s_fetch_v<T>(pc, base, ld_qkv, D, j0 + F8S_CH, N);
    }
    if (live)
      f8_tile_step(buf, buf + F8S_KSC, buf + F8S_VT, F8S_VROW, buf + F8S_VSC, 1, j0, N, q, causal, qf, qsc, c2, h, l31,
                   m, l, oacc);
    if (more) {
      if constexpr (!V_EARLY) f8s_fetch_v<T>(pc, base, ld_qkv, D, j0 + F8S_CH, N);
      f8s_commit<T>(smem[(c + 1) & 1], pc, j0 + F8S_CH, N);
    }
    __syncthreads();
  }
  if (!live) return;
  l += __shfl_xor(l, 32, 64);
  if (q < N)
    f8_store<T>(o + ((int64_t)b * N + q) * ld_o + hh * 64, lse ? lse + (int64_t)bh * N + q : nullptr, oacc, l, m * c2, h);
}

// ---------------------------------------------------------------------------
// Quantise-once form of the streamed fp8 forward (opt-in).  attn_fwd_fp8_stream quantises a head's K and V once
// per 256-query block; here attn_fp8_quant_kv does it once per head into a workspace and attn_fwd_fp8_pre streams
// the ready-made chunk images through the same ring.
//   workspace: [B*H][ceil(N / 64)] chunk images of F8S_BUF bytes, each byte for byte the ring buffer that
//   f8s_commit builds (Kimg | V^T | K scales | V scales), so the consumer's copy into LDS is lane-linear: 540
//   16-B pieces for 512 threads.  V^T's 4 pad bytes per row, which nothing reads, are written as zero: the
//   workspace is a pure function of K and V.
//   attn_fp8_quant_kv: grid (B*H, ceil(N / 64)), one chunk per workgroup: f8s_fetch_k / f8s_fetch_v / f8s_commit
//   into LDS, one barrier, coalesced 16-B stores.  Keys past N: the streamed kernel's rule (row N - 1, zeroed).
//   attn_fwd_fp8_pre: attn_fwd_fp8_stream's grid, wave-to-query mapping, ring, loop and barriers; the fetch is
//   this thread's pieces of the next image (requested before the tile step, 4 or 8 registers in flight over it),
//   the commit their LDS write.  Q is still quantised here, once per wave.  The bytes in LDS and every operation
//   on them are the streamed kernel's: o and lse are its bits at every N.
// ---------------------------------------------------------------------------
constexpr int F8P_PIECES = F8S_BUF / 16;            // 16-B pieces of a chunk image
constexpr int F8P_TAIL = F8P_PIECES - F8_THREADS;   // threads that move a second piece
static_assert(F8S_BUF % 16 == 0 && F8P_TAIL >= 0 && F8P_TAIL <= F8_THREADS, "one or two pieces per thread");
static_assert(F8S_VROW % 4 == 0 && F8S_VT % 4 == 0 && F8S_VROW - F8S_CH == 4, "V^T's pad is one aligned word per row");
typedef int f8p_piece __attribute__((ext_vector_type(4)));

template <typename T>
__global__ __launch_bounds__(F8_THREADS) void attn_fp8_quant_kv(const T* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                                int N, unsigned char* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) unsigned char buf[F8S_BUF];
  const int bh = blockIdx.x, b = bh / H, hh = bh - b * H;
  const int tid = threadIdx.x, j0 = blockIdx.y * F8S_CH;
  const T* base = qkv + (int64_t)b * N * ld_qkv + hh * 64;
  F8Piece<T> pc;
  f8s_fetch_k<T>(pc, base, ld_qkv, D, j0, N);
  f8s_fetch_v<T>(pc, base, ld_qkv, D, j0, N);
  if (tid < 64) *reinterpret_cast<int*>(buf + F8S_VT + tid * F8S_VROW + F8S_CH) = 0;  // the pad f8s_commit leaves
  f8s_commit<T>(buf, pc, j0, N);
  __syncthreads();
  f8p_piece* dst = reinterpret_cast<f8p_piece*>(ws + ((int64_t)bh * gridDim.y + blockIdx.y) * F8S_BUF);
  const f8p_piece* src = reinterpret_cast<const f8p_piece*>(buf);
  dst[tid] = src[tid];
  if (tid < F8P_TAIL) dst[F8_THREADS + tid] = src[F8_THREADS + tid];
}

struct F8PrePiece { f8p_piece a, b; };
__device__ __forceinline__ void f8p_fetch(F8PrePiece& p, const unsigned char* img) {
  const int tid = threadIdx.x;
  const f8p_piece* src = reinterpret_cast<const f8p_piece*>(img);
  p.a = src[tid];
  if (tid < F8P_TAIL) p.b = src[F8_THREADS + tid];
}
__device__ __forceinline__ void f8p_commit(unsigned char* buf, const F8PrePiece& p) {
  const int tid = threadIdx.x;
  f8p_piece* dst = reinterpret_cast<f8p_piece*>(buf);
  dst[tid] = p.a;
  if (tid < F8P_TAIL) dst[F8_THREADS + tid] = p.b;
}

template <typename T>
__global__ __launch_bounds__(F8_THREADS, 4) void attn_fwd_fp8_pre(const T* __restrict__ qkv, int64_t ld_qkv, int H,
                                                                 int N, const unsigned char* __restrict__ ws,
                                                                 float scale, T* __restrict__ o, int64_t ld_o,
                                                                 float* __restrict__ lse, int causal) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][F8S_BUF];
  const int bh = blockIdx.x, b = bh / H, hh = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* base = qkv + (int64_t)b * N * ld_qkv + hh * 64;
  const int h = lane >> 5, l31 = lane & 31;
  const int q0 = blockIdx.y * F8S_QB + wave * 32, q = q0 + l31;
  i32x8 qf;
  int qsc;
  f8_q_frag<T>(base + (int64_t)min(q, N - 1) * ld_qkv, h, qf, qsc);
  const int nc = (N + F8S_CH - 1) / F8S_CH;
  const unsigned char* img = ws + (int64_t)bh * nc * F8S_BUF;  // this head's chunk images
  F8PrePiece pc = {};
  f8p_fetch(pc, img);
  f8p_commit(smem[0], pc);
  __syncthreads();
  const float c2 = scale * LOG2E;
  float m = -INFINITY, l = 0.f;
  f32x16 oacc[2] = {};
  const bool live = q0 < N;  // wave-uniform; the trip count below does not depend on it
#pragma unroll 1
  for (int c = 0; c < nc; ++c) {
    const unsigned char* buf = smem[c & 1];
    const int j0 = c * F8S_CH;
    const bool more = c + 1 < nc;  // the same in every wave of the workgroup
    if (more) f8p_fetch(pc, img + (int64_t)(c + 1) * F8S_BUF);
    if (live)
      f8_tile_step(buf, buf + F8S_KSC, buf + F8S_VT, F8S_VROW, buf + F8S_VSC, 1, j0, N, q, causal, qf, qsc, c2, h, l31,
                   m, l, oacc);
    if (more) f8p_commit(smem[(c + 1) & 1], pc);
    __syncthreads();
  }
  if (!live) return;
  l += __shfl_xor(l, 32, 64);
  if (q < N)
    f8_store<T>(o + ((int64_t)b * N + q) * ld_o + hh * 64, lse ? lse + (int64_t)bh * N + q : nullptr, oacc, l, m * c2, h);
}

// qkv-bias gradient partials of one (b, h): sum this workgroup's rows of dq (or dk, dv)
// -- per lane over its rows, across the 16 lanes of a row group, across the 8 waves
// through LDS (reused after the main loop) -- into out[0..63] (and out[D..] for dk,
// out[2D..] for dv when NOUT = 2).
template <int NOUT>
__device__ __forceinline__ void bias_flush(f32x4 (&c0)[4], f32x4 (*c1)[4], char* smem, float* out, int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  float* red = reinterpret_cast<float*>(smem);  // [NOUT][AT_WAVES][64]
  __syncthreads();                              // every wave is done reading the LDS images
#pragma unroll
  for (int o = 0; o < NOUT; ++o) {
    f32x4 (&c)[4] = o == 0 ? c0 : *c1;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float v = c[dt][t];
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 4, 64);
        v += __shfl_xor(v, 8, 64);
        if ((lane & 15) == 0) red[(o * AT_WAVES + wave) * 64 + dt * 16 + 4 * g + t] = v;
      }
  }
  __syncthreads();
  if (threadIdx.x < 64 * NOUT) {
    const int o = threadIdx.x >> 6, d = threadIdx.x & 63;
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < AT_WAVES; ++w) sum += red[(o * AT_WAVES + w) * 64 + d];
    out[(NOUT == 1 ? 0 : (o + 1) * D) + d] = sum;
  }
}

// Column sums of a 16-row fragment set c[dt][t] (rows = lane & 15, column dt*16 + 4g + t),
// reduced over the 16 rows and kept compressed: lane l ends up owning column
// (l15 >> 2) * 16 + 4g + (l15 & 3), one register instead of sixteen.
__device__ __forceinline__ float colsum16(const f32x4 (&c)[4], int lane) {
  const int l15 = lane & 15;
  float own = 0.f;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float v = c[dt][t];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64);
      if (l15 == dt * 4 + t) own = v;
    }
  return own;
}
__device__ __forceinline__ int colsum16_col(int lane) {
  const int l15 = lane & 15;
  return (l15 >> 2) * 16 + 4 * (lane >> 4) + (l15 & 3);
}
// Flush per-lane compressed column sums (own[o] for output o) of the 8 waves into out.
template <int NOUT>
__device__ __forceinline__ void bias_flush_c(const float (&own)[NOUT], char* smem, float* out, int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* red = reinterpret_cast<float*>(smem);  // [NOUT][AT_WAVES][64]
  __syncthreads();                              // every wave is done reading the LDS images
#pragma unroll
  for (int o = 0; o < NOUT; ++o) red[(o * AT_WAVES + wave) * 64 + colsum16_col(lane)] = own[o];
  __syncthreads();
  if (threadIdx.x < 64 * NOUT) {
    const int o = threadIdx.x >> 6, d = threadIdx.x & 63;
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < AT_WAVES; ++w) sum += red[(o * AT_WAVES + w) * 64 + d];
    out[(NOUT == 1 ? 0 : (o + 1) * D) + d] = sum;
  }
}

// ---------------------------------------------------------------------------
// Pieces of the bf16 backward shared by the resident kernels (attn_bwd_dq, attn_bwd_dkv: whole-head
// images) and the streamed ones (attn_bwd_dq_stream, attn_bwd_dkv_stream: 64-row chunk images).  A tile
// is named twice: row0, its first row inside the LDS image, and key0 / q0, its absolute index (the same
// for a resident image, j0 + row0 for a chunk).
// ---------------------------------------------------------------------------
// Query row q of one head (clamped to N - 1): the q and dO fragments, delta = rowsum(dO * O) (written for
// the dkv kernel) and lse * log2(e).  base / dob / ob: the head's q, dO, O columns of row 0.
__device__ __forceinline__ void at_qrow(const bf16* base, int64_t ld_qkv, const bf16* dob, int64_t ld_do,
                                        const bf16* ob, int64_t ld_o, const float* lse_bh, float* delta_bh, int q,
                                        int N, int g, bf16x8 (&qf)[2], bf16x8 (&of)[2], float& dl, float& l2) {
  const int qc = min(q, N - 1);
  dl = 0.f;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    qf[kk] = *reinterpret_cast<const bf16x8*>(base + (int64_t)qc * ld_qkv + kk * 32 + g * 8);
    of[kk] = *reinterpret_cast<const bf16x8*>(dob + (int64_t)qc * ld_do + kk * 32 + g * 8);
    const bf16x8 ov = *reinterpret_cast<const bf16x8*>(ob + (int64_t)qc * ld_o + kk * 32 + g * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) dl = fmaf((float)of[kk][e], (float)ov[e], dl);
  }
  dl += __shfl_xor(dl, 16, 64);
  dl += __shfl_xor(dl, 32, 64);
  l2 = lse_bh[qc] * LOG2E;
  if (g == 0 && q < N) delta_bh[q] = dl;
}
// Key row kc of one head: the k and v fragments.
__device__ __forceinline__ void at_krow(const bf16* base, int64_t ld_qkv, int D, int kc, int g, bf16x8 (&kf)[2],
                                        bf16x8 (&vf)[2]) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    kf[kk] = *reinterpret_cast<const bf16x8*>(base + (int64_t)kc * ld_qkv + D + kk * 32 + g * 8);
    vf[kk] = *reinterpret_cast<const bf16x8*>(base + (int64_t)kc * ld_qkv + 2 * D + kk * 32 + g * 8);
  }
}
// A 16-row fragment set x[dt][t] (this lane: columns dt*16 + 4g + t of its row) as bf16 to the row at p.
__device__ __forceinline__ void at_store_row(bf16* p, const f32x4 (&x)[4], int g) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    *reinterpret_cast<bf16x4*>(p + dt * 16 + 4 * g) =
        bf16x4{(bf16)x[dt][0], (bf16)x[dt][1], (bf16)x[dt][2], (bf16)x[dt][3]};
}
// dk (already scaled) and dv of one key row; row = the key's dq column of this head.
__device__ __forceinline__ void at_store_dkv(bf16* row, int D, const f32x4 (&dk)[4], const f32x4 (&dv)[4], int g) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    bf16x4 kv = {(bf16)dk[dt][0], (bf16)dk[dt][1], (bf16)dk[dt][2], (bf16)dk[dt][3]};
    bf16x4 vv = {(bf16)dv[dt][0], (bf16)dv[dt][1], (bf16)dv[dt][2], (bf16)dv[dt][3]};
    *reinterpret_cast<bf16x4*>(row + D + dt * 16 + 4 * g) = kv;
    *reinterpret_cast<bf16x4*>(row + 2 * D + dt * 16 + 4 * g) = vv;
  }
}
// The two resident backward steps, stated once for both operand policies P (AtBf16: the bf16 kernels, resident and
// streamed; AtBf16x3: the f32 "high" kernels).
// dq half, one pair of key tiles (32 keys): S^T and dP^T of the lane's query against the K / V images,
// p = exp2(c2 S - l2) (0 on keys >= N and, causal, on keys > q), dS = p (dP - dl), dQ += dS K.
// edge: the caller's wave-uniform "this pair (chunk) may hold keys >= N".
template <typename P = AtBf16>
__device__ __forceinline__ void at_dq_step(typename P::Img Kimg, typename P::Img Vimg, int row0, int key0, int N,
                                           bool edge, const AtOffsets& off, int g, const typename P::Frag (&qf)[2],
                                           const typename P::Frag (&of)[2], float c2, float l2, float dl, int q,
                                           int causal, f32x4 (&dq)[4]) {
  f32x4 ds[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, dpacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      sacc = P::mma(P::row(Kimg, row0 + u * 16, off.row[kk]), qf[kk], sacc);
      dpacc = P::mma(P::row(Vimg, row0 + u * 16, off.row[kk]), of[kk], dpacc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = key0 + u * 16 + 4 * g + r;
      float pv = fexp2(fmaf(sacc[r], c2, -l2));
      if (edge && key >= N) pv = 0.f;
      if (causal && key > q) pv = 0.f;
      ds[u][r] = pv * (dpacc[r] - dl);
    }
    // split operands: bound fragment hoisting -- both tiles' 16 fragments spill at 128 VGPRs
    if constexpr (P::SPLIT) if (u == 0) __builtin_amdgcn_sched_barrier(0);
  }
  const typename P::Frag dsf = P::pack(ds[0], ds[1]);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dq[dt] = P::mma(P::tr(Kimg, row0, off.tr[dt]), dsf, dq[dt]);
}
// dkv half, one pair of query tiles (32 queries): S and dP of the lane's key against the Q / dO images,
// row constants from the lse * log2(e) / delta strips (indexed like the image), dV += P^T dO, dK += dS^T Q.
template <typename P = AtBf16>
__device__ __forceinline__ void at_dkv_step(typename P::Img Qimg, typename P::Img Oimg, const float* lse2,
                                            const float* delta, int row0, int q0, const AtOffsets& off, int g,
                                            const typename P::Frag (&kf)[2], const typename P::Frag (&vf)[2], float c2,
                                            bool kvalid, int key, int causal, f32x4 (&dk)[4], f32x4 (&dv)[4]) {
  f32x4 p[2], ds[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    f32x4 sacc = {0.f, 0.f, 0.f, 0.f}, dpacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      sacc = P::mma(P::row(Qimg, row0 + u * 16, off.row[kk]), kf[kk], sacc);
      dpacc = P::mma(P::row(Oimg, row0 + u * 16, off.row[kk]), vf[kk], dpacc);
    }
    const f32x4 l2 = *reinterpret_cast<const f32x4*>(lse2 + row0 + u * 16 + 4 * g);
    const f32x4 dl = *reinterpret_cast<const f32x4*>(delta + row0 + u * 16 + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float pv = kvalid ? fexp2(fmaf(sacc[r], c2, -l2[r])) : 0.f;
      if (causal && key > q0 + u * 16 + 4 * g + r) pv = 0.f;
      p[u][r] = pv;
      ds[u][r] = pv * (dpacc[r] - dl[r]);
    }
  }
  const typename P::Frag pf = P::pack(p[0], p[1]), dsf = P::pack(ds[0], ds[1]);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    dv[dt] = P::mma(P::tr(Oimg, row0, off.tr[dt]), pf, dv[dt]);
    dk[dt] = P::mma(P::tr(Qimg, row0, off.tr[dt]), dsf, dk[dt]);
  }
}

// ---------------------------------------------------------------------------
// bf16 backward, two kernels per (b, h) so each holds only half the head in LDS
// (57 KiB -> two workgroups per CU); N > 224 (CLIP ViT-L/14's 257 tokens), else attn_bwd_fused:
//   attn_bwd_dq  : LDS K, V; each wave owns query tiles (Q, dO, O from global),
//                  computes delta = rowsum(dO*O) (written for the other kernel),
//                  recomputes S^T, dP^T over all keys, accumulates dQ.
//   attn_bwd_dkv : LDS Q, dO (+ lse, delta); each wave owns key tiles (K, V from
//                  global), recomputes S, dP over all queries, accumulates dK, dV.
// ---------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(AT_THREADS, 4) void attn_bwd_dq(const bf16* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                            int N, float scale, const bf16* __restrict__ o,
                                                            int64_t ld_o, const bf16* __restrict__ dout, int64_t ld_do,
                                                            const float* __restrict__ lse, float* __restrict__ delta_out,
                                                            bf16* __restrict__ dqkv, int64_t ld_dqkv,
                                                            float* __restrict__ bias_part, int causal) {
  constexpr int NT2 = (NT + 1) / 2, ROWS = NT2 * 32;
  __shared__ __attribute__((aligned(16))) char smem[2 * ROWS * 128];
  char* Kimg = smem;
  char* Vimg = Kimg + ROWS * 128;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  const bf16* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  {
    char* const imgs[2] = {Kimg, Vimg};
    const bf16* const srcs[2] = {base + D, base + 2 * D};
    const int64_t lds_[2] = {ld_qkv, ld_qkv};
    at_load<ROWS, AT_THREADS, 2>(imgs, srcs, lds_, N);
  }
  const AtOffsets off(lane);
  __syncthreads();
  const float c2 = scale * LOG2E;
  f32x4 cs[4];  // column sums of dq (qkv-bias gradient), this lane's rows
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) cs[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int qt = wave; qt < NT; qt += AT_WAVES) {
    const int q = qt * 16 + (lane & 15);
    bf16x8 qf[2], of[2];
    float dl, l2;
    at_qrow(base, ld_qkv, dout + (int64_t)b * N * ld_do + h * 64, ld_do, o + (int64_t)b * N * ld_o + h * 64, ld_o,
            lse + (int64_t)bh * N, delta_out + (int64_t)bh * N, q, N, g, qf, of, dl, l2);
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kp = 0; kp < NT2; ++kp)  // edge, wave-uniform: only the last pair holds padded keys
      at_dq_step(Kimg, Vimg, kp * 32, kp * 32, N, (kp + 1) * 32 > N, off, g, qf, of, c2, l2, dl, q, causal, dq);
    if (q < N) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        dq[dt] *= scale;
        cs[dt] += dq[dt];
      }
      at_store_row(dqkv + ((int64_t)b * N + q) * ld_dqkv + h * 64, dq, g);
    }
  }
  if (bias_part) bias_flush<1>(cs, nullptr, smem, bias_part + (int64_t)b * 3 * D + h * 64, D);
}

template <int NT>
__global__ __launch_bounds__(AT_THREADS, 4) void attn_bwd_dkv(const bf16* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                             int N, float scale, const bf16* __restrict__ dout,
                                                             int64_t ld_do, const float* __restrict__ lse,
                                                             const float* __restrict__ delta_in, bf16* __restrict__ dqkv,
                                                             int64_t ld_dqkv, float* __restrict__ bias_part,
                                                             int causal) {
  constexpr int NT2 = (NT + 1) / 2, ROWS = NT2 * 32;
  __shared__ __attribute__((aligned(16))) char smem[2 * ROWS * 128 + 2 * ROWS * 4];
  char* Qimg = smem;
  char* Oimg = Qimg + ROWS * 128;  // dO
  float* lse2 = reinterpret_cast<float*>(Oimg + ROWS * 128);
  float* delta = lse2 + ROWS;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  const bf16* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const bf16* dob = dout + (int64_t)b * N * ld_do + h * 64;
  {
    char* const imgs[2] = {Qimg, Oimg};
    const bf16* const srcs[2] = {base, dob};
    const int64_t lds_[2] = {ld_qkv, ld_do};
    at_load<ROWS, AT_THREADS, 2>(imgs, srcs, lds_, N);
  }
  for (int q = threadIdx.x; q < ROWS; q += AT_THREADS) {
    delta[q] = (q < N) ? delta_in[(int64_t)bh * N + q] : 0.f;
    lse2[q] = (q < N) ? lse[(int64_t)bh * N + q] * LOG2E : INFINITY;
  }
  const AtOffsets off(lane);
  __syncthreads();
  const float c2 = scale * LOG2E;
  float cs[2] = {0.f, 0.f};  // compressed column sums of dk, dv (qkv-bias gradient), colsum16 layout
  for (int kt = wave; kt < NT; kt += AT_WAVES) {
    const int key = kt * 16 + (lane & 15);
    const bool kvalid = key < N;
    bf16x8 kf[2], vf[2];
    at_krow(base, ld_qkv, D, min(key, N - 1), g, kf, vf);
    f32x4 dv[4], dk[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dk[dt] = dv[dt]; }
#pragma unroll 1  // unroll 2 spills ~300 VGPRs at the 128-register budget
    for (int qp = 0; qp < NT2; ++qp)
      at_dkv_step(Qimg, Oimg, lse2, delta, qp * 32, qp * 32, off, g, kf, vf, c2, kvalid, key, causal, dk, dv);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dk[dt] = kvalid ? dk[dt] * scale : f32x4{0.f, 0.f, 0.f, 0.f};
      if (!kvalid) dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (kvalid) at_store_dkv(dqkv + ((int64_t)b * N + key) * ld_dqkv + h * 64, D, dk, dv, g);
    if (bias_part) {  // wave-uniform
      cs[0] += colsum16(dk, lane);
      cs[1] += colsum16(dv, lane);
    }
  }
  if (bias_part) bias_flush_c<2>(cs, smem, bias_part + (int64_t)b * 3 * D + h * 64, D);
}

// ---------------------------------------------------------------------------
// bf16 backward fused into one kernel per (b, h) for N <= 224 (NT <= 14 tiles of 16): one
// workgroup of NT waves, so each wave owns exactly one key tile in phase 1 and one query tile
// in phase 2.  q, k, v, o, dO are read once and S, dP computed once (the two-kernel form
// recomputes both and reads q, k, v, dO twice).
//   prologue: Q, dO -> LDS images; delta = rowsum(dO * O) (O straight from global) and lse -> LDS;
//             wave w holds key tile w's K, V rows in registers.
//   phase 1 : wave w: S, dP of its 16 keys against every query (the attn_bwd_dkv loop) ->
//             dK, dV; dS^T goes to LDS as NT column tiles [key row][16 queries] bf16, the layout
//             the transposed read of phase 2 takes conflict-free (16 rows x 32 B per group).
//   phase 2 : the K tiles replace the Q image; wave w: dQ of its 16 queries = dS K over all keys
//             (A = K^T and B = dS^T from the same transposed-read pattern: same k-slot order).
// LDS at N = 197: 2 x 28 KiB images + 13 x 7 KiB dS^T tiles + lse/delta = 149 KiB (1 WG/CU).
// ---------------------------------------------------------------------------
template <int NT> struct BwdF {
  static constexpr int NT2 = (NT + 1) / 2, ROWS = NT2 * 32, THREADS = NT * 64;
  static constexpr int IMG = ROWS * 128, DST = ROWS * 32;
  static constexpr int LDS = 2 * IMG + NT * DST + 2 * ROWS * 4;
};

template <int NT, bool CAUSAL = false, bool STAMP = false>
__global__ __launch_bounds__(NT * 64, (NT + 3) / 4) void attn_bwd_fused(
    const bf16* __restrict__ qkv, int64_t ld_qkv, int D, int H, int N, float scale, const bf16* __restrict__ o,
    int64_t ld_o, const bf16* __restrict__ dout, int64_t ld_do, const float* __restrict__ lse,
    float* __restrict__ delta_out, bf16* __restrict__ dqkv, int64_t ld_dqkv, float* __restrict__ bias_part,
    unsigned long long* __restrict__ stamps) {
  AT_STAMP_BEGIN()
  using F = BwdF<NT>;
  constexpr int NT2 = F::NT2, ROWS = F::ROWS, NTHR = F::THREADS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qimg = smem;  // Q in phase 1, K in phase 2
  char* Oimg = smem + F::IMG;  // dO
  char* dST = smem + 2 * F::IMG;
  float* lse2 = reinterpret_cast<float*>(dST + NT * F::DST);
  float* delta = lse2 + ROWS;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const bf16* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const bf16* dob = dout + (int64_t)b * N * ld_do + h * 64;
  const bf16* obase = o + (int64_t)b * N * ld_o + h * 64;

  // ---- prologue: this wave's key tile (registers), Q / dO images, delta, lse
  const int key = wave * 16 + l15;
  const bool kvalid = key < N;
  bf16x8 kf[2], vf[2];
  {
    const int kc = min(key, N - 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      kf[kk] = *reinterpret_cast<const bf16x8*>(base + (int64_t)kc * ld_qkv + D + kk * 32 + g * 8);
      vf[kk] = *reinterpret_cast<const bf16x8*>(base + (int64_t)kc * ld_qkv + 2 * D + kk * 32 + g * 8);
    }
  }
  {
    constexpr int TOTAL = ROWS * 8, PER = (TOTAL + NTHR - 1) / NTHR;
    bf16x8 qv[PER], dv8[PER], ov[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = tid + u * NTHR;
      const int row = min(idx >> 3, N - 1), c = idx & 7;
      if (idx < TOTAL) {
        qv[u] = *reinterpret_cast<const bf16x8*>(base + (int64_t)row * ld_qkv + c * 8);
        dv8[u] = *reinterpret_cast<const bf16x8*>(dob + (int64_t)row * ld_do + c * 8);
        ov[u] = *reinterpret_cast<const bf16x8*>(obase + (int64_t)row * ld_o + c * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = tid + u * NTHR;
      const int row = idx >> 3, c = idx & 7;
      const bool in = idx < TOTAL, live = in && row < N;
      float dl = 0.f;
      if (live) {
#pragma unroll
        for (int e = 0; e < 8; ++e) dl = fmaf((float)dv8[u][e], (float)ov[u][e], dl);
      }
      // the 8 chunks of a row sit in 8 consecutive lanes (NTHR % 8 == 0): reduce outside the branch
      dl += __shfl_xor(dl, 1, 64);
      dl += __shfl_xor(dl, 2, 64);
      dl += __shfl_xor(dl, 4, 64);
      if (in) {
        bf16x8 qw = qv[u], dw = dv8[u];
        if (!live) {
#pragma unroll
          for (int t = 0; t < 8; ++t) { qw[t] = (bf16)0.f; dw[t] = (bf16)0.f; }
        }
        *reinterpret_cast<bf16x8*>(Qimg + at_off(row, c)) = qw;
        *reinterpret_cast<bf16x8*>(Oimg + at_off(row, c)) = dw;
        if (c == 0) {
          // negated row constants: the initial S / dP accumulators of phase 1
          delta[row] = -dl;
          lse2[row] = live ? -lse[(int64_t)bh * N + row] / scale : -INFINITY;
          if (live) delta_out[(int64_t)bh * N + row] = dl;
        }
      }
    }
    // dS^T rows of the padded keys [NT*16, ROWS) are read by phase 2's last key pair: zero them
    constexpr int PAD = (ROWS - NT * 16) * 32 / 16;  // 16-B chunks per column tile
    if constexpr (PAD > 0) {
      for (int i = tid; i < NT * PAD; i += NTHR) {
        const int t = i / PAD, r = i - t * PAD;
        *reinterpret_cast<f32x4*>(dST + t * F::DST + NT * 16 * 32 + r * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
  const AtOffsets off(lane);
  __syncthreads();
  AT_STAMP(1)
  const float c2 = scale * LOG2E;

  // ---- phase 1: wave = key tile
  f32x4 dv[4], dk[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) { dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dk[dt] = dv[dt]; }
  char* dsw = dST + key * 32 + g * 8;  // this lane's dS^T slot (queries 4g..4g+3 of a column tile)
#pragma unroll
  for (int qp = 0; qp < NT2; ++qp) {
    f32x4 p[2], ds[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int qt = 2 * qp + u;
      // row constants as the initial accumulators: S' = QK^T - lse/scale (-inf on padded keys),
      // dP' = dO V^T - delta, so p = exp2(c2 S') and dS = p dP' (two VALU ops per element)
      const f32x4 nl = *reinterpret_cast<const f32x4*>(lse2 + qt * 16 + 4 * g);
      f32x4 sacc = kvalid ? nl : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      f32x4 dpacc = *reinterpret_cast<const f32x4*>(delta + qt * 16 + 4 * g);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        sacc = mfma16(rowf(Qimg, qt * 16, off.row[kk]), kf[kk], sacc);
        dpacc = mfma16(rowf(Oimg, qt * 16, off.row[kk]), vf[kk], dpacc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pv = fexp2(sacc[r] * c2);
        if constexpr (CAUSAL) { if (key > qt * 16 + 4 * g + r) pv = 0.f; }
        p[u][r] = pv;
        ds[u][r] = pv * dpacc[r];
      }
      if (qt < NT) {  // wave-uniform (the padded tile of an odd NT has no column tile)
        const bf16x4 w = {(bf16)ds[u][0], (bf16)ds[u][1], (bf16)ds[u][2], (bf16)ds[u][3]};
        *reinterpret_cast<bf16x4*>(dsw + qt * F::DST) = w;
      }
    }
    const bf16x8 pf = pack8(p[0], p[1]), dsf = pack8(ds[0], ds[1]);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dv[dt] = mfma16(trf(Oimg, qp * 32, off.tr[dt]), pf, dv[dt]);
      dk[dt] = mfma16(trf(Qimg, qp * 32, off.tr[dt]), dsf, dk[dt]);
    }
  }
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    dk[dt] = kvalid ? dk[dt] * scale : f32x4{0.f, 0.f, 0.f, 0.f};
    if (!kvalid) dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (kvalid) {
    bf16* row = dqkv + ((int64_t)b * N + key) * ld_dqkv + h * 64;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      bf16x4 kv = {(bf16)dk[dt][0], (bf16)dk[dt][1], (bf16)dk[dt][2], (bf16)dk[dt][3]};
      bf16x4 vv = {(bf16)dv[dt][0], (bf16)dv[dt][1], (bf16)dv[dt][2], (bf16)dv[dt][3]};
      *reinterpret_cast<bf16x4*>(row + D + dt * 16 + 4 * g) = kv;
      *reinterpret_cast<bf16x4*>(row + 2 * D + dt * 16 + 4 * g) = vv;
    }
  }
  float cs[3] = {0.f, 0.f, 0.f};  // compressed column sums of dq, dk, dv (qkv-bias gradient)
  if (bias_part) {
    cs[1] = colsum16(dk, lane);
    cs[2] = colsum16(dv, lane);
  }
  __syncthreads();  // every wave is done with Q, dO and has written its dS^T rows
  AT_STAMP(2)

  // ---- phase 2: K tiles over the Q image (padded rows: zeros), wave = query tile
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    bf16x8 w = kf[kk];
    if (!kvalid) {
#pragma unroll
      for (int t = 0; t < 8; ++t) w[t] = (bf16)0.f;
    }
    *reinterpret_cast<bf16x8*>(Qimg + at_off(key, kk * 4 + g)) = w;
  }
  __syncthreads();
  AT_STAMP(3)
  {
    const int q = wave * 16 + l15;
    const char* dsr = dST + wave * F::DST + (4 * g + (l15 >> 2)) * 32 + (l15 & 3) * 8;
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kp = 0; kp < NT2; ++kp) {
      const bf16x8 sf = cat4(lds_read_tr(dsr + kp * 32 * 32), lds_read_tr(dsr + kp * 32 * 32 + 16 * 32));
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) dq[dt] = mfma16(trf(Qimg, kp * 32, off.tr[dt]), sf, dq[dt]);
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = q < N ? dq[dt] * scale : f32x4{0.f, 0.f, 0.f, 0.f};
    if (q < N) {
      bf16* row = dqkv + ((int64_t)b * N + q) * ld_dqkv + h * 64;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        bf16x4 qv4 = {(bf16)dq[dt][0], (bf16)dq[dt][1], (bf16)dq[dt][2], (bf16)dq[dt][3]};
        *reinterpret_cast<bf16x4*>(row + dt * 16 + 4 * g) = qv4;
      }
    }
    if (bias_part) cs[0] = colsum16(dq, lane);
  }
  if (bias_part) {  // [3][NT][64] partials through LDS, then one 64-column row per output
    float* red = reinterpret_cast<float*>(smem);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 3; ++t) red[(t * NT + wave) * 64 + colsum16_col(lane)] = cs[t];
    __syncthreads();
    for (int i = tid; i < 3 * 64; i += NTHR) {
      const int t = i >> 6, d = i & 63;
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < NT; ++w) sum += red[(t * NT + w) * 64 + d];
      bias_part[(int64_t)b * 3 * D + t * D + h * 64 + d] = sum;
    }
  }
  AT_STAMP(4)
  AT_STAMP_FLUSH()
}

// ---------------------------------------------------------------------------
// f32 forward on v_mfma_f32_16x16x4_f32 (CLIP-HBA at the reference's fp32 precision, NEWP:274;
// config C3): one workgroup (8 waves) per (b, h), K and V of the head in LDS as f32 (<= 2 x 72 KiB,
// N <= 288), wave = query tile of 16.  Products are exact f32 (the MFMA's f32 form), accumulation f32.
//   S^T = K Q^T: A = K (row = key), B = Q^T; the 4 k-slots of lane group g take head dims 16g + ks, so a
//     lane reads 16 consecutive floats of its key row (4 x ds_read_b128) and holds Q[query][16g..16g+15]
//     in registers.  Output: lane (l15, g) holds S[query l15][key 4g + r] -- the bf16 kernel's layout.
//   O^T = V^T P^T: B = P^T straight from the softmax registers (k-slot g at step (kt, r) is key
//     kt*16 + 4g + r, the key the lane already holds); A row m of d-tile dt is head dim 4m + dt, so one
//     ds_read_b128 of V[key][4*l15 .. 4*l15+3] feeds the 4 d-tiles, and a lane ends with
//     O[query l15][16g .. 16g+15].
// K image: 16-B chunk c of row r at chunk position c ^ kswz(r) -- conflict-free for the four
// ds_read_b128 of a key tile (each 16-lane group covers 16 rows and two chunk columns); V image plain
// row-major (a group reads one row and its 4th-next, disjoint banks).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int kswz(int r) {
  const int x = r & 15;
  return x ^ ((((x >> 2) ^ (x >> 3)) & 1) << 2);
}

// Rows [0, rows) of a head slice into a swizzled image (rows >= N zero).
__device__ __forceinline__ void f32_img_load(float* img, const float* src, int64_t ld, int N, int rows, int tid,
                                             int nthr) {
  for (int i = tid; i < rows * 16; i += nthr) {
    const int r = i >> 4, c = i & 15;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < N) v = *reinterpret_cast<const f32x4*>(src + (int64_t)r * ld + c * 4);
    *reinterpret_cast<f32x4*>(img + r * 64 + ((c ^ kswz(r)) << 2)) = v;
  }
}
// row r of a swizzled image: the 16 floats [16g, 16g + 16) (4 chunks)
__device__ __forceinline__ void f32_row16(const float* img, int r, int g, float (&x)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(img + r * 64 + (((4 * g + j) ^ kswz(r)) << 2));
    x[4 * j] = v[0]; x[4 * j + 1] = v[1]; x[4 * j + 2] = v[2]; x[4 * j + 3] = v[3];
  }
}
// chunk c of row r; SWZ = false: a plain row-major image (the resident forward's V)
template <bool SWZ = true>
__device__ __forceinline__ f32x4 f32_chunk(const float* img, int r, int c) {
  return *reinterpret_cast<const f32x4*>(img + r * 64 + ((SWZ ? c ^ kswz(r) : c) << 2));
}
__device__ __forceinline__ void f32_glob16(const float* p, float (&x)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * j);
    x[4 * j] = v[0]; x[4 * j + 1] = v[1]; x[4 * j + 2] = v[2]; x[4 * j + 3] = v[3];
  }
}
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// x[dt][rr] * mul = element 4 rr + dt of the lane's 16 floats at p (the O^T / dQ^T / dK^T / dV^T accumulators:
// row m of d-tile dt is head dim 4m + dt); mul = 1.f folds away.
__device__ __forceinline__ void f32_store_row(float* p, const f32x4 (&x)[4], float mul) {
#pragma unroll
  for (int rr = 0; rr < 4; ++rr)
    *reinterpret_cast<f32x4*>(p + 4 * rr) = f32x4{x[0][rr] * mul, x[1][rr] * mul, x[2][rr] * mul, x[3][rr] * mul};
}
// dk * scale and dv of one key row; row = the lane's 16 floats of the key's dq column.
__device__ __forceinline__ void f32_store_dkv(float* row, int D, const f32x4 (&dk)[4], const f32x4 (&dv)[4],
                                              float scale) {
  f32_store_row(row + D, dk, scale);
  f32_store_row(row + 2 * D, dv, 1.f);
}
// o = oacc / l and lse[at] = (mc + log2 l) ln 2 of one query (mc = max * c2, l = the row sum); lse may be null.
__device__ __forceinline__ void f32_store_o(float* orow, float* lse, int64_t at, const f32x4 (&oacc)[4], float l,
                                            float mc, int g) {
  f32_store_row(orow, oacc, 1.0f / l);
  if (g == 0 && lse) lse[at] = (mc + __log2f(l)) * LN2;
}

template <int NT>
__global__ __launch_bounds__(512) void attn_fwd_f32mfma(const float* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                        int N, float scale, float* __restrict__ o, int64_t ld_o,
                                                        float* __restrict__ lse, int causal) {
  constexpr int ROWS = NT * 16, KG = 4;  // key tiles per K-register group
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Kimg = reinterpret_cast<float*>(smem);
  float* Vimg = Kimg + ROWS * 64;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const float* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  // K, V -> LDS (rows >= N zero) in one loop, both loads of a piece in flight together: two f32_img_load
  // passes measured 4 % slower at 257 tokens (profiles/r12/README.md)
  for (int i = tid; i < ROWS * 16; i += 512) {
    const int r = i >> 4, c = i & 15;
    f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = kv;
    if (r < N) {
      kv = *reinterpret_cast<const f32x4*>(base + (int64_t)r * ld_qkv + D + c * 4);
      vv = *reinterpret_cast<const f32x4*>(base + (int64_t)r * ld_qkv + 2 * D + c * 4);
    }
    *reinterpret_cast<f32x4*>(Kimg + r * 64 + ((c ^ kswz(r)) << 2)) = kv;
    *reinterpret_cast<f32x4*>(Vimg + r * 64 + c * 4) = vv;
  }
  __syncthreads();
  const float c2 = scale * LOG2E;
  for (int qt = wave; qt < NT; qt += 8) {
    const int q = qt * 16 + l15;
    float qf[16];
    f32_glob16(base + (int64_t)min(q, N - 1) * ld_qkv + 16 * g, qf);
    f32x4 s[NT];
#pragma unroll
    for (int k0 = 0; k0 < NT; k0 += KG) {
      float kf[KG][16];
#pragma unroll
      for (int u = 0; u < KG; ++u) {
        if (k0 + u < NT) {
          f32_row16(Kimg, (k0 + u) * 16 + l15, g, kf[u]);
          s[k0 + u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
#pragma unroll
      for (int ks = 0; ks < 16; ++ks)
#pragma unroll
        for (int u = 0; u < KG; ++u)
          if (k0 + u < NT) s[k0 + u] = mfma4(kf[u][ks], qf[ks], s[k0 + u]);
    }
    // keys >= N exist only in the last tile
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if ((NT - 1) * 16 + 4 * g + r >= N) s[NT - 1][r] = -INFINITY;
    if (causal) {
#pragma unroll
      for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kt * 16 + 4 * g + r > q) s[kt][r] = -INFINITY;
    }
    float mr[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) mr[r] = fmaxf(mr[r], s[kt][r]);
    float m = fmaxf(fmaxf(mr[0], mr[1]), fmaxf(mr[2], mr[3]));
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float mc = m * c2;
    float lr[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) { const float p = fexp2(fmaf(s[kt][r], c2, -mc)); s[kt][r] = p; lr[r] += p; }
    float l = (lr[0] + lr[1]) + (lr[2] + lr[3]);
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    f32x4 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const f32x4 v = f32_chunk<false>(Vimg, kt * 16 + 4 * g + r, l15);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) oacc[dt] = mfma4(v[dt], s[kt][r], oacc[dt]);
      }
      if (kt % 4 == 3) __builtin_amdgcn_sched_barrier(0);  // bound V-read hoisting (VGPRs)
    }
    if (q < N) f32_store_o(o + ((int64_t)b * N + q) * ld_o + h * 64 + 16 * g, lse, (int64_t)bh * N + q, oacc, l, mc, g);
  }
}

// ---------------------------------------------------------------------------
// f32 backward on v_mfma_f32_16x16x4_f32 (N <= 288, head_dim 64), the same operand algebra as the f32
// forward: two kernels, each with two head images in LDS (kswz chunk swizzle, read both by rows -- 4
// ds_read_b128 of 16 consecutive floats -- and by columns -- one ds_read_b128 of chunk l15 of row
// 4g + r, the A operand of the 4 d-tiles whose row m is head dim 4m + dt).
//   dq : wave = query tile, K and V images; S^T and dP^T with the lane's query in registers, so a lane
//        holds keys 4g + r of query l15; dQ^T += K^T dS^T, B = dS^T from registers.  Writes delta.
//   dkv: wave = key tile, Q and dO images; S and dP with the wave's key tile in registers (a lane
//        holds queries 4g + r of key l15); dV^T += dO^T P, dK^T += Q^T dS, B from registers.
// The row I/O and the two tile steps below are shared with the streamed f32 kernels (attn_bwd_dq_stream_f32,
// attn_bwd_dkv_stream_f32), whose images are 64-row chunks.
// ---------------------------------------------------------------------------
// Query row q of one head (clamped to N - 1): q and dO in registers, delta = rowsum(dO * O) (written for the
// dkv kernel) and lse * log2(e).  base / dob / ob: the head's q, dO, O columns of row 0.
__device__ __forceinline__ void f32_qrow(const float* base, int64_t ld_qkv, const float* dob, int64_t ld_do,
                                         const float* ob, int64_t ld_o, const float* lse_bh, float* delta_bh, int q,
                                         int N, int g, float (&qf)[16], float (&df)[16], float& dl, float& l2) {
  const int qc = min(q, N - 1);
  float of[16];
  f32_glob16(base + (int64_t)qc * ld_qkv + 16 * g, qf);
  f32_glob16(dob + (int64_t)qc * ld_do + 16 * g, df);
  f32_glob16(ob + (int64_t)qc * ld_o + 16 * g, of);
  dl = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) dl = fmaf(df[j], of[j], dl);
  dl += __shfl_xor(dl, 16, 64);
  dl += __shfl_xor(dl, 32, 64);
  if (q < N && g == 0) delta_bh[q] = dl;
  l2 = lse_bh[qc] * LOG2E;
}
// Key row kc of one head: k and v in registers.
__device__ __forceinline__ void f32_krow(const float* base, int64_t ld_qkv, int D, int kc, int g, float (&kf)[16],
                                         float (&vf)[16]) {
  f32_glob16(base + (int64_t)kc * ld_qkv + D + 16 * g, kf);
  f32_glob16(base + (int64_t)kc * ld_qkv + 2 * D + 16 * g, vf);
}
// dq half, one key tile: S^T and dP^T of the lane's query (a lane holds keys 4g + r), p = exp2(c2 S - l2)
// (0 on keys >= N and, causal, on keys > q), dS = p (dP - dl), dQ^T += K^T dS^T.  row0: the tile's first row in
// the image; key0: its first key (the same for a resident image, j0 + row0 for a streamed chunk).
__device__ __forceinline__ void f32_dq_step(const float* Kimg, const float* Vimg, int row0, int key0, int N, int l15,
                                            int g, const float (&qf)[16], const float (&df)[16], float c2, float l2,
                                            float dl, int q, int causal, f32x4 (&dq)[4]) {
  float kf[16], vf[16];
  f32_row16(Kimg, row0 + l15, g, kf);
  f32_row16(Vimg, row0 + l15, g, vf);
  f32x4 st = {0.f, 0.f, 0.f, 0.f}, dpt = st;
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
    st = mfma4(kf[ks], qf[ks], st);   // S^T[key 4g + r][query l15]
    dpt = mfma4(vf[ks], df[ks], dpt);
  }
  f32x4 ds;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int key = key0 + 4 * g + r;
    float p = key < N ? fexp2(fmaf(st[r], c2, -l2)) : 0.f;
    if (causal && key > q) p = 0.f;
    ds[r] = p * (dpt[r] - dl);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const f32x4 a = f32_chunk(Kimg, row0 + 4 * g + r, l15);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = mfma4(a[dt], ds[r], dq[dt]);
  }
}
// dkv half, one query tile: S and dP of the lane's key (a lane holds queries 4g + r), row constants from the
// lse * log2(e) / delta strips (indexed like the image), dV^T += dO^T P, dK^T += Q^T dS.  q0: the tile's first query.
__device__ __forceinline__ void f32_dkv_step(const float* Qimg, const float* Oimg, const float* l2s, const float* dls,
                                             int row0, int q0, int l15, int g, const float (&kf)[16],
                                             const float (&vf)[16], float c2, bool kvalid, int key, int causal,
                                             f32x4 (&dk)[4], f32x4 (&dv)[4]) {
  float qf[16], df[16];
  f32_row16(Qimg, row0 + l15, g, qf);
  f32_row16(Oimg, row0 + l15, g, df);
  f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dpc = sc;
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
    sc = mfma4(qf[ks], kf[ks], sc);   // S[query 4g + r][key l15]
    dpc = mfma4(df[ks], vf[ks], dpc);
  }
  const f32x4 l2 = *reinterpret_cast<const f32x4*>(l2s + row0 + 4 * g);
  const f32x4 dl = *reinterpret_cast<const f32x4*>(dls + row0 + 4 * g);
  f32x4 p, ds;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float pv = kvalid ? fexp2(fmaf(sc[r], c2, -l2[r])) : 0.f;
    if (causal && key > q0 + 4 * g + r) pv = 0.f;
    p[r] = pv;
    ds[r] = pv * (dpc[r] - dl[r]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const f32x4 ao = f32_chunk(Oimg, row0 + 4 * g + r, l15), aq = f32_chunk(Qimg, row0 + 4 * g + r, l15);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dv[dt] = mfma4(ao[dt], p[r], dv[dt]);
      dk[dt] = mfma4(aq[dt], ds[r], dk[dt]);
    }
  }
}

template <int NT>
__global__ __launch_bounds__(512) void attn_bwd_dq_f32mfma(const float* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                           int N, float scale, const float* __restrict__ o, int64_t ld_o,
                                                           const float* __restrict__ dout, int64_t ld_do,
                                                           const float* __restrict__ lse, float* __restrict__ delta_out,
                                                           float* __restrict__ dqkv, int64_t ld_dqkv, int causal) {
  constexpr int ROWS = NT * 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Kimg = reinterpret_cast<float*>(smem);
  float* Vimg = Kimg + ROWS * 64;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const float* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  f32_img_load(Kimg, base + D, ld_qkv, N, ROWS, tid, 512);
  f32_img_load(Vimg, base + 2 * D, ld_qkv, N, ROWS, tid, 512);
  __syncthreads();
  const float c2 = scale * LOG2E;
  for (int qt = wave; qt < NT; qt += 8) {
    const int q = qt * 16 + l15;
    float qf[16], df[16], dl, l2;
    f32_qrow(base, ld_qkv, dout + (int64_t)b * N * ld_do + h * 64, ld_do, o + (int64_t)b * N * ld_o + h * 64, ld_o,
             lse + (int64_t)bh * N, delta_out + (int64_t)bh * N, q, N, g, qf, df, dl, l2);
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kt = 0; kt < NT; ++kt)
      f32_dq_step(Kimg, Vimg, kt * 16, kt * 16, N, l15, g, qf, df, c2, l2, dl, q, causal, dq);
    if (q < N) f32_store_row(dqkv + ((int64_t)b * N + q) * ld_dqkv + h * 64 + 16 * g, dq, scale);
  }
}

template <int NT>
__global__ __launch_bounds__(512) void attn_bwd_dkv_f32mfma(const float* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                            int N, float scale, const float* __restrict__ dout,
                                                            int64_t ld_do, const float* __restrict__ lse,
                                                            const float* __restrict__ delta, float* __restrict__ dqkv,
                                                            int64_t ld_dqkv, int causal) {
  constexpr int ROWS = NT * 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Qimg = reinterpret_cast<float*>(smem);
  float* Oimg = Qimg + ROWS * 64;  // dO
  float* l2s = Oimg + ROWS * 64;   // lse * log2(e) per query (+inf past N)
  float* dls = l2s + ROWS;         // delta per query
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const float* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  f32_img_load(Qimg, base, ld_qkv, N, ROWS, tid, 512);
  f32_img_load(Oimg, dout + (int64_t)b * N * ld_do + h * 64, ld_do, N, ROWS, tid, 512);
  for (int i = tid; i < ROWS; i += 512) {
    l2s[i] = i < N ? lse[(int64_t)bh * N + i] * LOG2E : INFINITY;
    dls[i] = i < N ? delta[(int64_t)bh * N + i] : 0.f;
  }
  __syncthreads();
  const float c2 = scale * LOG2E;
  for (int kt = wave; kt < NT; kt += 8) {
    const int key = kt * 16 + l15;
    const bool kvalid = key < N;
    float kf[16], vf[16];
    f32_krow(base, ld_qkv, D, min(key, N - 1), g, kf, vf);
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[dt] = dk[dt]; }
#pragma unroll 1
    for (int qt = 0; qt < NT; ++qt)
      f32_dkv_step(Qimg, Oimg, l2s, dls, qt * 16, qt * 16, l15, g, kf, vf, c2, kvalid, key, causal, dk, dv);
    if (kvalid) f32_store_dkv(dqkv + ((int64_t)b * N + key) * ld_dqkv + h * 64 + 16 * g, D, dk, dv, scale);
  }
}

// ---------------------------------------------------------------------------
// Resident f32 attention as three bf16 MFMA products ("high", vit_sdpa_f32_precision(1)): the
// operand algebra of the resident bf16 kernels (attn_fwd_mfma, at_dq_step, at_dkv_step -- rowf / trf fragments,
// the AtOffsets swizzle, 16-row tiles in 32-row pairs) fed from f32 global memory.  Every f32 value x is split
// with the GEMM's helper (bf16_split.hpp) into hi = bf16_rne(x), lo = bf16_rne(x - hi), and every matrix product
// runs as  acc += A_hi B_lo;  acc += A_lo B_hi;  acc += A_hi B_hi  on v_mfma_f32_16x16x32_bf16 (A, B: the MFMA's
// operands; lo lo is dropped).  That is the operand policy AtBf16x3: the backward kernels call the bf16 kernels' own
// at_dq_step / at_dkv_step with it, the forward restates attn_fwd_mfma's query-tile body on it (a shared body or
// softmax block reschedules every attn_fwd_mfma instance).
//   head images : loaded as f32, split once while the LDS image is written -- a hi and a lo image per matrix in
//                 the bf16 layout, 4 x ROWS x 128 B, the bytes of the two f32 images they replace
//   row operands: the wave's own rows (q; q and dO; k and v) from global memory as f32, split once per tile
//   P, dS       : split from the f32 accumulators into a hi and a lo pack (4 values per lane and tile)
// The masking, the row max / sum of the unsplit p, exp2, delta = rowsum(dO O), 1 / l, lse, the scale factors and
// the stores are f32 as in the f32 MFMA kernels above.  Dynamic LDS; two workgroups per CU while four images fit
// twice (<= 80 KiB), one beyond -- the launch bound follows.
// ---------------------------------------------------------------------------
template <int NT>
struct F32X3 {
  static constexpr int NT2 = (NT + 1) / 2, ROWS = NT2 * 32, IMG = ROWS * 128;
  static constexpr int LDS = 4 * IMG, LDS_DKV = 4 * IMG + 2 * ROWS * 4;
  static constexpr int CU_LDS = 163840;
  // waves per SIMD (8 waves per workgroup on 4 SIMDs): 4 = two workgroups per CU (128 VGPRs), 2 = one (256)
  static constexpr int WPS = 2 * LDS <= CU_LDS ? 4 : 2, WPS_DKV = 2 * LDS_DKV <= CU_LDS ? 4 : 2;
  static_assert(LDS_DKV <= CU_LDS, "one workgroup per CU");
};

// Image forms (IMAGE = true): the head slices are read from, and o is written as, the pre-split
// activation image of DESIGN 4.26 in place of the f32 values -- the same addresses and row pitch.  A row's head slice
// is two 128-byte k-blocks m; hi chunk g of a block is at byte 128m + 16g, lo chunk g at 128m + 64 + 16g, and element j
// of a chunk is column 16 (j >> 2) + 4g + (j & 3) of the block: the bytes split8 gives for those columns.  The LDS
// images, the fragments and every MFMA are the f32 forms'; only the operand bits' origin and the o store differ.
typedef uint32_t u32x2_ __attribute__((ext_vector_type(2)));
// hi / lo chunk g = c & 3 of k-block m = c >> 2 of an image row -> row r of a hi and a lo LDS image.  A chunk's low
// 8 bytes are head dims 32m + 4g .. + 3 and its high 8 bytes 32m + 16 + 4g .. + 3: half g & 1 of the granules
// 4m + (g >> 1) and 4m + 2 + (g >> 1).
__device__ __forceinline__ void x3_put_chunk(char* hi, char* lo, int r, int c, const u32x4_& h, const u32x4_& l) {
  const int c0 = (c & 4) + ((c & 3) >> 1), half = (c & 1) * 8;
  const int o0 = at_off(r, c0) + half, o1 = at_off(r, c0 + 2) + half;
  *reinterpret_cast<u32x2_*>(hi + o0) = u32x2_{h[0], h[1]};
  *reinterpret_cast<u32x2_*>(hi + o1) = u32x2_{h[2], h[3]};
  *reinterpret_cast<u32x2_*>(lo + o0) = u32x2_{l[0], l[1]};
  *reinterpret_cast<u32x2_*>(lo + o1) = u32x2_{l[2], l[3]};
}
// the hi (u = 0) / lo (u = 1) chunk c of the image row whose head slice starts at p
__device__ __forceinline__ u32x4_ x3_chunk(const float* p, int c, int u) {
  return *reinterpret_cast<const u32x4_*>(reinterpret_cast<const char*>(p) + (c >> 2) * 128 + u * 64 + (c & 3) * 16);
}

// Rows [0, N) of two f32 head slices -> a hi and a lo bf16 image each (at_off layout, rows >= N zero).
// IMAGE: the slices are image rows, copied chunk by chunk.
template <int ROWS, bool IMAGE = false>
__device__ __forceinline__ void x3_load2(char* ahi, char* alo, const float* sa, int64_t lda, char* bhi, char* blo,
                                         const float* sb, int64_t ldb, int N) {
  for (int i = threadIdx.x; i < ROWS * 8; i += AT_THREADS) {
    const int r = i >> 3, c = i & 7;
    if constexpr (IMAGE) {
      u32x4_ ah = {0u, 0u, 0u, 0u}, al = ah, bh = ah, bl = ah;
      if (r < N) {
        ah = x3_chunk(sa + (int64_t)r * lda, c, 0);
        al = x3_chunk(sa + (int64_t)r * lda, c, 1);
        bh = x3_chunk(sb + (int64_t)r * ldb, c, 0);
        bl = x3_chunk(sb + (int64_t)r * ldb, c, 1);
      }
      x3_put_chunk(ahi, alo, r, c, ah, al);
      x3_put_chunk(bhi, blo, r, c, bh, bl);
      continue;
    }
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, b0 = a0, b1 = a0;
    if (r < N) {
      a0 = *reinterpret_cast<const f32x4*>(sa + (int64_t)r * lda + c * 8);
      a1 = *reinterpret_cast<const f32x4*>(sa + (int64_t)r * lda + c * 8 + 4);
      b0 = *reinterpret_cast<const f32x4*>(sb + (int64_t)r * ldb + c * 8);
      b1 = *reinterpret_cast<const f32x4*>(sb + (int64_t)r * ldb + c * 8 + 4);
    }
    bf16x8 h, l;
    split8<1>(a0, a1, h, l);
    *reinterpret_cast<bf16x8*>(ahi + at_off(r, c)) = h;
    *reinterpret_cast<bf16x8*>(alo + at_off(r, c)) = l;
    split8<1>(b0, b1, h, l);
    *reinterpret_cast<bf16x8*>(bhi + at_off(r, c)) = h;
    *reinterpret_cast<bf16x8*>(blo + at_off(r, c)) = l;
  }
}
// The lane's row fragments (head dims kk * 32 + 8g .. + 8) of the f32 row at p, split; x: the f32 values.
__device__ __forceinline__ void x3_row(const float* p, int g, AtBf16x3::Frag (&f)[2], f32x4 (&x)[4]) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    x[2 * kk] = *reinterpret_cast<const f32x4*>(p + kk * 32 + g * 8);
    x[2 * kk + 1] = *reinterpret_cast<const f32x4*>(p + kk * 32 + g * 8 + 4);
    f[kk] = AtBf16x3::pack(x[2 * kk], x[2 * kk + 1]);
  }
}
// x[dt] * mul = columns dt * 16 + 4g .. + 4 of the lane's row at p (the accumulator layout of the bf16 kernels)
__device__ __forceinline__ void x3_store_row(float* p, const f32x4 (&x)[4], float mul, int g) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    *reinterpret_cast<f32x4*>(p + dt * 16 + 4 * g) = f32x4{x[dt][0] * mul, x[dt][1] * mul, x[dt][2] * mul, x[dt][3] * mul};
}

// x3_row from an image row: the lane's fragment kk is granule c = 4 kk + g of the head slice -- k0 = 8g, half
// hh = g >> 1 of the chunks ga = 2 (g & 1) and ga + 1 of k-block kk, 8 bytes each, hi then (+ 64) lo.
__device__ __forceinline__ void x3_row_image(const float* p, int g, AtBf16x3::Frag (&f)[2]) {
  const char* b = reinterpret_cast<const char*>(p) + (g & 1) * 32 + (g >> 1) * 8;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    u32x2_ w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = *reinterpret_cast<const u32x2_*>(b + kk * 128 + (u >> 1) * 64 + (u & 1) * 16);
    f[kk].hi = __builtin_bit_cast(bf16x8, u32x4_{w[0][0], w[0][1], w[1][0], w[1][1]});
    f[kk].lo = __builtin_bit_cast(bf16x8, u32x4_{w[2][0], w[2][1], w[3][0], w[3][1]});
  }
}
// x3_store_row as an image row: x[2m], x[2m + 1] are the two halves of chunk g of k-block m.  The products are
// x3_store_row's; split8<1> because mul ends a reciprocal and the asm's operands are not modelled.
__device__ __forceinline__ void x3_store_row_image(float* p, const f32x4 (&x)[4], float mul, int g) {
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const f32x4 a = {x[2 * m][0] * mul, x[2 * m][1] * mul, x[2 * m][2] * mul, x[2 * m][3] * mul};
    const f32x4 b = {x[2 * m + 1][0] * mul, x[2 * m + 1][1] * mul, x[2 * m + 1][2] * mul, x[2 * m + 1][3] * mul};
    bf16x8 h, l;
    split8<1>(a, b, h, l);
    char* d = reinterpret_cast<char*>(p) + m * 128 + g * 16;
    *reinterpret_cast<bf16x8*>(d) = h;
    *reinterpret_cast<bf16x8*>(d + 64) = l;
  }
}

// The resident "high" forward, stated once in attn_x3_fwd.inc: attn_fwd_f32x3 (f32 qkv and o) and
// attn_fwd_image_x3 (qkv and o hold pre-split images; o and lse are attn_fwd_f32x3's bit for bit, o as
// its image).
#define X3_FWD_KERNEL attn_fwd_f32x3
#define X3_IMAGE 0
#include "attn_x3_fwd.inc"
#undef X3_FWD_KERNEL
#undef X3_IMAGE
#define X3_FWD_KERNEL attn_fwd_image_x3
#define X3_IMAGE 1
#include "attn_x3_fwd.inc"
#undef X3_FWD_KERNEL
#undef X3_IMAGE

template <int NT>
__global__ __launch_bounds__(AT_THREADS, F32X3<NT>::WPS) void attn_bwd_dq_f32x3(
    const float* __restrict__ qkv, int64_t ld_qkv, int D, int H, int N, float scale, const float* __restrict__ o,
    int64_t ld_o, const float* __restrict__ dout, int64_t ld_do, const float* __restrict__ lse,
    float* __restrict__ delta_out, float* __restrict__ dqkv, int64_t ld_dqkv, int causal) {
  using X = AtBf16x3;
  constexpr int NT2 = F32X3<NT>::NT2, ROWS = F32X3<NT>::ROWS, IMG = F32X3<NT>::IMG;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *Khi = smem, *Klo = smem + IMG, *Vhi = smem + 2 * IMG, *Vlo = smem + 3 * IMG;
  const X::Img Kimg = {Khi, Klo}, Vimg = {Vhi, Vlo};
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  const float* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const float* dob = dout + (int64_t)b * N * ld_do + h * 64;
  const float* ob = o + (int64_t)b * N * ld_o + h * 64;
  x3_load2<ROWS>(Khi, Klo, base + D, ld_qkv, Vhi, Vlo, base + 2 * D, ld_qkv, N);
  const AtOffsets off(lane);
  __syncthreads();
  const float c2 = scale * LOG2E;
  for (int qt = wave; qt < NT; qt += AT_WAVES) {
    const int q = qt * 16 + (lane & 15), qc = min(q, N - 1);
    X::Frag qf[2], of[2];
    float dl = 0.f;
    {
      f32x4 x[4], df[4];
      x3_row(base + (int64_t)qc * ld_qkv, g, qf, x);
      x3_row(dob + (int64_t)qc * ld_do, g, of, df);
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // delta = rowsum(dO * O) on the unsplit f32 values
        const f32x4 ov = *reinterpret_cast<const f32x4*>(ob + (int64_t)qc * ld_o + (j >> 1) * 32 + g * 8 + (j & 1) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) dl = fmaf(df[j][e], ov[e], dl);
      }
    }
    dl += __shfl_xor(dl, 16, 64);
    dl += __shfl_xor(dl, 32, 64);
    if (q < N && g == 0) delta_out[(int64_t)bh * N + q] = dl;
    const float l2 = lse[(int64_t)bh * N + qc] * LOG2E;
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kp = 0; kp < NT2; ++kp)  // edge, wave-uniform: only the last pair holds padded keys
      at_dq_step<X>(Kimg, Vimg, kp * 32, kp * 32, N, (kp + 1) * 32 > N, off, g, qf, of, c2, l2, dl, q, causal, dq);
    if (q < N) x3_store_row(dqkv + ((int64_t)b * N + q) * ld_dqkv + h * 64, dq, scale, g);
  }
}

template <int NT>
__global__ __launch_bounds__(AT_THREADS, F32X3<NT>::WPS_DKV) void attn_bwd_dkv_f32x3(
    const float* __restrict__ qkv, int64_t ld_qkv, int D, int H, int N, float scale, const float* __restrict__ dout,
    int64_t ld_do, const float* __restrict__ lse, const float* __restrict__ delta_in, float* __restrict__ dqkv,
    int64_t ld_dqkv, int causal) {
  using X = AtBf16x3;
  constexpr int NT2 = F32X3<NT>::NT2, ROWS = F32X3<NT>::ROWS, IMG = F32X3<NT>::IMG;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *Qhi = smem, *Qlo = smem + IMG, *Ohi = smem + 2 * IMG, *Olo = smem + 3 * IMG;  // O: dO
  const X::Img Qimg = {Qhi, Qlo}, Oimg = {Ohi, Olo};
  float* lse2 = reinterpret_cast<float*>(smem + 4 * IMG);  // lse * log2(e) per query (+inf past N)
  float* delta = lse2 + ROWS;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  const float* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  x3_load2<ROWS>(Qhi, Qlo, base, ld_qkv, Ohi, Olo, dout + (int64_t)b * N * ld_do + h * 64, ld_do, N);
  for (int i = threadIdx.x; i < ROWS; i += AT_THREADS) {
    lse2[i] = i < N ? lse[(int64_t)bh * N + i] * LOG2E : INFINITY;
    delta[i] = i < N ? delta_in[(int64_t)bh * N + i] : 0.f;
  }
  const AtOffsets off(lane);
  __syncthreads();
  const float c2 = scale * LOG2E;
  for (int kt = wave; kt < NT; kt += AT_WAVES) {
    const int key = kt * 16 + (lane & 15), kc = min(key, N - 1);
    const bool kvalid = key < N;
    X::Frag kf[2], vf[2];
    {
      f32x4 x[4];
      x3_row(base + (int64_t)kc * ld_qkv + D, g, kf, x);
      x3_row(base + (int64_t)kc * ld_qkv + 2 * D, g, vf, x);
    }
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[dt] = dk[dt]; }
#pragma unroll 1
    for (int qp = 0; qp < NT2; ++qp)
      at_dkv_step<X>(Qimg, Oimg, lse2, delta, qp * 32, qp * 32, off, g, kf, vf, c2, kvalid, key, causal, dk, dv);
    if (kvalid) {
      float* row = dqkv + ((int64_t)b * N + key) * ld_dqkv + h * 64;
      x3_store_row(row + D, dk, scale, g);
      x3_store_row(row + 2 * D, dv, 1.f, g);
    }
  }
}

// ---------------------------------------------------------------------------
// generic (f32 compute, f32 or bf16 storage) path: 4 lanes per query / key,
// each owning 16 of the 64 head dims; keys / queries streamed through LDS.
// ---------------------------------------------------------------------------
constexpr int GCH = 64;  // rows per LDS chunk

template <typename T>
__global__ __launch_bounds__(256) void attn_fwd_generic(const T* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                        int N, float scale, T* __restrict__ o, int64_t ld_o,
                                                        float* __restrict__ lse, int causal) {
  __shared__ float Ks[GCH][65], Vs[GCH][65];
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int t = threadIdx.x, qi = blockIdx.x * 64 + (t >> 2), u = t & 3;
  const T* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  float qv[16], acc[16];
  const bool valid = qi < N;
#pragma unroll
  for (int d = 0; d < 16; ++d) { qv[d] = valid ? (float)base[(int64_t)qi * ld_qkv + u * 16 + d] * scale : 0.f; acc[d] = 0.f; }
  float m = -INFINITY, l = 0.f;
  for (int j0 = 0; j0 < N; j0 += GCH) {
    __syncthreads();
    for (int idx = t; idx < GCH * 64; idx += 256) {
      int r = idx >> 6, d = idx & 63, j = j0 + r;
      Ks[r][d] = j < N ? (float)base[(int64_t)j * ld_qkv + D + d] : 0.f;
      Vs[r][d] = j < N ? (float)base[(int64_t)j * ld_qkv + 2 * D + d] : 0.f;
    }
    __syncthreads();
    const int jn = min(GCH, N - j0);
    for (int r = 0; r < jn; ++r) {
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < 16; ++d) s = fmaf(qv[d], Ks[r][u * 16 + d], s);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      if (causal && j0 + r > qi) s = -INFINITY;  // key 0 comes first, so m is finite from then on
      float mn = fmaxf(m, s);
      float corr = __expf(m - mn), p = __expf(s - mn);
      l = l * corr + p;
#pragma unroll
      for (int d = 0; d < 16; ++d) acc[d] = acc[d] * corr + p * Vs[r][u * 16 + d];
      m = mn;
    }
  }
  if (!valid) return;
  const float inv = 1.f / l;
  T* orow = o + ((int64_t)b * N + qi) * ld_o + h * 64 + u * 16;
#pragma unroll
  for (int d = 0; d < 16; ++d) orow[d] = (T)(acc[d] * inv);
  if (u == 0) lse[(int64_t)bh * N + qi] = m + logf(l);
}

// q-parallel: delta_i = dO_i . O_i ; dQ_i = scale * sum_j p_ij (dO_i.v_j - delta_i) k_j
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_dq_generic(const T* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                           int N, float scale, const T* __restrict__ o,
                                                           int64_t ld_o, const T* __restrict__ dout, int64_t ld_do,
                                                           const float* __restrict__ lse, float* __restrict__ delta_out,
                                                           T* __restrict__ dqkv, int64_t ld_dqkv, int causal) {
  __shared__ float Ks[GCH][65], Vs[GCH][65];
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int t = threadIdx.x, qi = blockIdx.x * 64 + (t >> 2), u = t & 3;
  const T* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const bool valid = qi < N;
  float qv[16], dov[16], acc[16];
  float dl = 0.f;
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    qv[d] = valid ? (float)base[(int64_t)qi * ld_qkv + u * 16 + d] * scale : 0.f;
    dov[d] = valid ? (float)dout[((int64_t)b * N + qi) * ld_do + h * 64 + u * 16 + d] : 0.f;
    float ov = valid ? (float)o[((int64_t)b * N + qi) * ld_o + h * 64 + u * 16 + d] : 0.f;
    dl = fmaf(dov[d], ov, dl);
    acc[d] = 0.f;
  }
  dl += __shfl_xor(dl, 1, 64);
  dl += __shfl_xor(dl, 2, 64);
  const float L = valid ? lse[(int64_t)bh * N + qi] : 0.f;
  for (int j0 = 0; j0 < N; j0 += GCH) {
    __syncthreads();
    for (int idx = t; idx < GCH * 64; idx += 256) {
      int r = idx >> 6, d = idx & 63, j = j0 + r;
      Ks[r][d] = j < N ? (float)base[(int64_t)j * ld_qkv + D + d] : 0.f;
      Vs[r][d] = j < N ? (float)base[(int64_t)j * ld_qkv + 2 * D + d] : 0.f;
    }
    __syncthreads();
    const int jn = min(GCH, N - j0);
    for (int r = 0; r < jn; ++r) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < 16; ++d) { s = fmaf(qv[d], Ks[r][u * 16 + d], s); dp = fmaf(dov[d], Vs[r][u * 16 + d], dp); }
      s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64);
      dp += __shfl_xor(dp, 1, 64); dp += __shfl_xor(dp, 2, 64);
      float ds = (causal && j0 + r > qi) ? 0.f : __expf(s - L) * (dp - dl);
#pragma unroll
      for (int d = 0; d < 16; ++d) acc[d] = fmaf(ds, Ks[r][u * 16 + d], acc[d]);
    }
  }
  if (!valid) return;
  if (u == 0) delta_out[(int64_t)bh * N + qi] = dl;
  T* row = dqkv + ((int64_t)b * N + qi) * ld_dqkv + h * 64 + u * 16;
#pragma unroll
  for (int d = 0; d < 16; ++d) row[d] = (T)(acc[d] * scale);
}

// key-parallel: dV_j = sum_i p_ij dO_i ; dK_j = scale * sum_i ds_ij q_i
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_dkv_generic(const T* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                            int N, float scale, const T* __restrict__ dout,
                                                            int64_t ld_do, const float* __restrict__ lse,
                                                            const float* __restrict__ delta, T* __restrict__ dqkv,
                                                            int64_t ld_dqkv, int causal) {
  __shared__ float Qs[GCH][65], Os[GCH][65];
  __shared__ float Ls[GCH], Dl[GCH];
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int t = threadIdx.x, kj = blockIdx.x * 64 + (t >> 2), u = t & 3;
  const T* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const bool valid = kj < N;
  float kv[16], vv[16], dk[16], dv[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    kv[d] = valid ? (float)base[(int64_t)kj * ld_qkv + D + u * 16 + d] : 0.f;
    vv[d] = valid ? (float)base[(int64_t)kj * ld_qkv + 2 * D + u * 16 + d] : 0.f;
    dk[d] = 0.f; dv[d] = 0.f;
  }
  for (int i0 = 0; i0 < N; i0 += GCH) {
    __syncthreads();
    for (int idx = t; idx < GCH * 64; idx += 256) {
      int r = idx >> 6, d = idx & 63, i = i0 + r;
      Qs[r][d] = i < N ? (float)base[(int64_t)i * ld_qkv + d] : 0.f;
      Os[r][d] = i < N ? (float)dout[((int64_t)b * N + i) * ld_do + h * 64 + d] : 0.f;
    }
    if (t < GCH) {
      int i = i0 + t;
      Ls[t] = i < N ? lse[(int64_t)bh * N + i] : 0.f;
      Dl[t] = i < N ? delta[(int64_t)bh * N + i] : 0.f;
    }
    __syncthreads();
    const int in = min(GCH, N - i0);
    for (int r = 0; r < in; ++r) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < 16; ++d) { s = fmaf(Qs[r][u * 16 + d], kv[d], s); dp = fmaf(Os[r][u * 16 + d], vv[d], dp); }
      s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64);
      dp += __shfl_xor(dp, 1, 64); dp += __shfl_xor(dp, 2, 64);
      float p = (causal && kj > i0 + r) ? 0.f : __expf(s * scale - Ls[r]);
      float ds = p * (dp - Dl[r]);
#pragma unroll
      for (int d = 0; d < 16; ++d) { dv[d] = fmaf(p, Os[r][u * 16 + d], dv[d]); dk[d] = fmaf(ds, Qs[r][u * 16 + d], dk[d]); }
    }
  }
  if (!valid) return;
  T* row = dqkv + ((int64_t)b * N + kj) * ld_dqkv + h * 64 + u * 16;
#pragma unroll
  for (int d = 0; d < 16; ++d) { row[D + d] = (T)(dk[d] * scale); row[2 * D + d] = (T)dv[d]; }
}

// delta[(b*H + h)*N + n] = sum_d dO[b*N+n][h*64+d] * O[b*N+n][h*64+d]; 16 lanes
// per (row, head), 4 dims per lane (8-B loads), shuffle-reduced.
template <typename T>
__global__ __launch_bounds__(256) void attn_delta_kernel(const T* __restrict__ o, int64_t ld_o,
                                                         const T* __restrict__ dout, int64_t ld_do, int B, int H,
                                                         int N, float* __restrict__ delta) {
  const int64_t pair = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int l = threadIdx.x & 15;
  const bool ok = pair < (int64_t)B * N * H;
  float s = 0.f;
  int64_t row = 0;
  int h = 0;
  if (ok) {
    row = pair / H;
    h = (int)(pair - row * H);
    const T* op = o + row * ld_o + h * 64 + l * 4;
    const T* dp = dout + row * ld_do + h * 64 + l * 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) s = fmaf((float)op[t], (float)dp[t], s);
  }
#pragma unroll
  for (int m = 8; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
  if (ok && l == 0) {
    const int b = (int)(row / N), n = (int)(row - (int64_t)b * N);
    delta[((int64_t)b * H + h) * N + n] = s;
  }
}

// ---------------------------------------------------------------------------
// Streamed bf16 attention: no compile-time bound on N (the path for N > 288).  The resident kernels'
// operand algebra -- S^T = K Q^T with a lane per query column, P / dS in registers as the B operand,
// the swizzled 128-B row image read by rowf / trf -- with the streamed operand passing through a
// double-buffered LDS ring of 64-row chunks instead of living there whole.
//   grid (B*H, ceil(N / 128)): a workgroup owns 128 queries (keys in the dkv kernel), a wave 16 of them,
//   held in registers for the whole kernel.  Per chunk: the next chunk's global loads are issued first
//   (one 16-B piece of each of the two images per thread), the MFMA work on the current chunk runs
//   under their latency, then the pieces go to the other buffer; one barrier per chunk.
//   fwd : K, V chunks; online softmax (running max m, per-lane partial sum l, o rescaled per chunk).
//   dq  : K, V chunks; writes delta and dq.          dkv : Q, dO chunks + lse / delta; writes dk, dv.
// Rows past N: loads are clamped to row N - 1 and the piece is zeroed in registers (at_load's rule);
// a key past N gets score -inf (p = 0 exactly), a query past N gets lse = +inf (p = 0 exactly).
// Every output element has one owner and every sum a fixed order: runs are bitwise repeatable.
// LDS: 2 x 16 KiB (+ 1 KiB lse / delta in dkv); 128-VGPR budget, so two workgroups share a CU.
// Out of scope: a causal streamed form (it takes the generic kernels past 288 tokens); f32: attn_*_stream_f32.
// ---------------------------------------------------------------------------
constexpr int ST_CH = 64;             // rows per streamed chunk
constexpr int ST_QB = AT_WAVES * 16;  // queries (keys) per workgroup
constexpr int ST_IMG = ST_CH * 128;   // bytes per chunk image
static_assert(ST_CH * 8 == AT_THREADS, "one 16-B piece of a chunk image per thread");

struct StPiece { bf16x8 a, b; };
// this thread's piece of rows [j0, j0 + 64) of two head slices (clamped to row N - 1)
__device__ __forceinline__ StPiece st_fetch(const bf16* sa, int64_t lda, const bf16* sb, int64_t ldb, int j0, int N) {
  const int row = min(j0 + (int)(threadIdx.x >> 3), N - 1), c = threadIdx.x & 7;
  StPiece p;
  p.a = *reinterpret_cast<const bf16x8*>(sa + (int64_t)row * lda + c * 8);
  p.b = *reinterpret_cast<const bf16x8*>(sb + (int64_t)row * ldb + c * 8);
  return p;
}
__device__ __forceinline__ void st_commit(char* buf, StPiece p, int j0, int N) {
  const int r = threadIdx.x >> 3, c = threadIdx.x & 7;
  if (j0 + r >= N) {
#pragma unroll
    for (int t = 0; t < 8; ++t) { p.a[t] = (bf16)0.f; p.b[t] = (bf16)0.f; }
  }
  *reinterpret_cast<bf16x8*>(buf + at_off(r, c)) = p.a;
  *reinterpret_cast<bf16x8*>(buf + ST_IMG + at_off(r, c)) = p.b;
}
// Online-softmax update for one chunk's raw scores s (this lane: keys j0 + kt*16 + 4g + r of its query, in both
// dtypes): -inf on keys >= N, the running max m (raw scores, all 4 lanes of a query agree), this lane's part l of
// the sum and oacc rescaled by alpha; s becomes p = exp2((s - m) c2).
__device__ __forceinline__ void st_softmax_chunk(f32x4 (&s)[4], int j0, int N, int g, float c2, float& m, float& l,
                                                 f32x4 (&oacc)[4]) {
  if (j0 + ST_CH > N) {  // wave-uniform: only the last chunk holds keys >= N
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (j0 + kt * 16 + 4 * g + r >= N) s[kt][r] = -INFINITY;
  }
  float mt = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) mt = fmaxf(mt, s[kt][r]);
  mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
  mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
  const float mn = fmaxf(m, mt);             // finite from the first chunk on: key 0 is never masked
  const float alpha = fexp2((m - mn) * c2);  // first chunk: m = -inf -> 0
  m = mn;
  const float mc = m * c2;
  float lt = 0.f;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) { const float p = fexp2(fmaf(s[kt][r], c2, -mc)); s[kt][r] = p; lt += p; }
  l = fmaf(l, alpha, lt);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oacc[dt] *= alpha;
}
// Row constants of a chunk for the dkv kernels, a strip of 2 x 64 floats behind the chunk's two images: threads
// 0..63 carry lse * log2(e) (+inf past N: p = 0), 64..127 delta (0 past N).
__device__ __forceinline__ float st_stat_fetch(const float* lse_bh, const float* delta_bh, int j0, int N) {
  const int tid = threadIdx.x;
  if (tid >= 2 * ST_CH) return 0.f;
  const int i = j0 + (tid & (ST_CH - 1));
  if (tid < ST_CH) return i < N ? lse_bh[i] * LOG2E : INFINITY;
  return i < N ? delta_bh[i] : 0.f;
}
__device__ __forceinline__ void st_stat_commit(void* strip, float v) {
  if (threadIdx.x < 2 * ST_CH) static_cast<float*>(strip)[threadIdx.x] = v;
}

__global__ __launch_bounds__(AT_THREADS, 2) void attn_fwd_stream(const bf16* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                                int N, float scale, bf16* __restrict__ o, int64_t ld_o,
                                                                float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) char smem[2][2 * ST_IMG];  // [buffer][K | V]
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  const bf16* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const int q = blockIdx.y * ST_QB + wave * 16 + (lane & 15);
  bf16x8 qf[2];
  {
    const int qq = min(q, N - 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) qf[kk] = *reinterpret_cast<const bf16x8*>(base + (int64_t)qq * ld_qkv + kk * 32 + g * 8);
  }
  const AtOffsets off(lane);
  const int nc = (N + ST_CH - 1) / ST_CH;
  StPiece pc = st_fetch(base + D, ld_qkv, base + 2 * D, ld_qkv, 0, N);
  st_commit(smem[0], pc, 0, N);
  __syncthreads();
  const float c2 = scale * LOG2E;
  float m = -INFINITY, l = 0.f;  // running max (raw scores, all 4 lanes of a query agree); this lane's part of the sum
  f32x4 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int c = 0; c < nc; ++c) {
    const char* Kc = smem[c & 1];
    const char* Vc = Kc + ST_IMG;
    const int j0 = c * ST_CH;
    const bool more = c + 1 < nc;
    if (more) pc = st_fetch(base + D, ld_qkv, base + 2 * D, ld_qkv, j0 + ST_CH, N);
    f32x4 s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) s[kt] = mfma16(rowf(Kc, kt * 16, off.row[kk]), qf[kk], s[kt]);
    }
    st_softmax_chunk(s, j0, N, g, c2, m, l, oacc);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 pf = pack8(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) oacc[dt] = mfma16(trf(Vc, ks * 32, off.tr[dt]), pf, oacc[dt]);
    }
    if (more) st_commit(smem[(c + 1) & 1], pc, j0 + ST_CH, N);
    __syncthreads();
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (q < N) {
    const float inv = 1.0f / l;
    bf16* orow = o + ((int64_t)b * N + q) * ld_o + h * 64;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      bf16x4 ov = {(bf16)(oacc[dt][0] * inv), (bf16)(oacc[dt][1] * inv), (bf16)(oacc[dt][2] * inv),
                   (bf16)(oacc[dt][3] * inv)};
      *reinterpret_cast<bf16x4*>(orow + dt * 16 + 4 * g) = ov;
    }
    if (g == 0) lse[(int64_t)bh * N + q] = (m * c2 + __log2f(l)) * LN2;
  }
}

// query-parallel half of the streamed backward: delta = rowsum(dO * O) and dQ (attn_bwd_dq's at_qrow and, per
// chunk, at_dq_step)
__global__ __launch_bounds__(AT_THREADS, 2) void attn_bwd_dq_stream(const bf16* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                                   int N, float scale, const bf16* __restrict__ o,
                                                                   int64_t ld_o, const bf16* __restrict__ dout,
                                                                   int64_t ld_do, const float* __restrict__ lse,
                                                                   float* __restrict__ delta_out, bf16* __restrict__ dqkv,
                                                                   int64_t ld_dqkv) {
  __shared__ __attribute__((aligned(16))) char smem[2][2 * ST_IMG];  // [buffer][K | V]
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  const bf16* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const int q = blockIdx.y * ST_QB + wave * 16 + (lane & 15);
  bf16x8 qf[2], of[2];
  float dl, l2;
  at_qrow(base, ld_qkv, dout + (int64_t)b * N * ld_do + h * 64, ld_do, o + (int64_t)b * N * ld_o + h * 64, ld_o,
          lse + (int64_t)bh * N, delta_out + (int64_t)bh * N, q, N, g, qf, of, dl, l2);
  const AtOffsets off(lane);
  const int nc = (N + ST_CH - 1) / ST_CH;
  StPiece pc = st_fetch(base + D, ld_qkv, base + 2 * D, ld_qkv, 0, N);
  st_commit(smem[0], pc, 0, N);
  __syncthreads();
  const float c2 = scale * LOG2E;
  f32x4 dq[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int c = 0; c < nc; ++c) {
    const char* Kc = smem[c & 1];
    const char* Vc = Kc + ST_IMG;
    const int j0 = c * ST_CH;
    const bool more = c + 1 < nc;
    if (more) pc = st_fetch(base + D, ld_qkv, base + 2 * D, ld_qkv, j0 + ST_CH, N);
    const bool edge = j0 + ST_CH > N;  // wave-uniform: only the last chunk holds keys >= N
#pragma unroll
    for (int kp = 0; kp < 2; ++kp)
      at_dq_step(Kc, Vc, kp * 32, j0 + kp * 32, N, edge, off, g, qf, of, c2, l2, dl, q, 0, dq);
    if (more) st_commit(smem[(c + 1) & 1], pc, j0 + ST_CH, N);
    __syncthreads();
  }
  if (q < N) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] *= scale;
    at_store_row(dqkv + ((int64_t)b * N + q) * ld_dqkv + h * 64, dq, g);
  }
}

// key-parallel half: dK, dV of the workgroup's 128 keys (K, V rows in registers) over streamed Q / dO chunks
__global__ __launch_bounds__(AT_THREADS, 2) void attn_bwd_dkv_stream(const bf16* __restrict__ qkv, int64_t ld_qkv, int D,
                                                                    int H, int N, float scale,
                                                                    const bf16* __restrict__ dout, int64_t ld_do,
                                                                    const float* __restrict__ lse,
                                                                    const float* __restrict__ delta_in,
                                                                    bf16* __restrict__ dqkv, int64_t ld_dqkv) {
  constexpr int BUF = 2 * ST_IMG + 2 * ST_CH * 4;  // Q | dO | lse * log2(e) | delta
  __shared__ __attribute__((aligned(16))) char smem[2][BUF];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const bf16* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const bf16* dob = dout + (int64_t)b * N * ld_do + h * 64;
  const int key = blockIdx.y * ST_QB + wave * 16 + (lane & 15);
  const bool kvalid = key < N;
  bf16x8 kf[2], vf[2];
  at_krow(base, ld_qkv, D, min(key, N - 1), g, kf, vf);
  const float* lse_bh = lse + (int64_t)bh * N;
  const float* delta_bh = delta_in + (int64_t)bh * N;
  const AtOffsets off(lane);
  const int nc = (N + ST_CH - 1) / ST_CH;
  StPiece pc = st_fetch(base, ld_qkv, dob, ld_do, 0, N);
  float sv = st_stat_fetch(lse_bh, delta_bh, 0, N);
  st_commit(smem[0], pc, 0, N);
  st_stat_commit(smem[0] + 2 * ST_IMG, sv);
  __syncthreads();
  const float c2 = scale * LOG2E;
  f32x4 dv[4], dk[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) { dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dk[dt] = dv[dt]; }
#pragma unroll 1
  for (int c = 0; c < nc; ++c) {
    const char* Qc = smem[c & 1];
    const char* Oc = Qc + ST_IMG;  // dO
    const float* lse2 = reinterpret_cast<const float*>(Qc + 2 * ST_IMG);
    const float* delta = lse2 + ST_CH;
    const int j0 = c * ST_CH;
    const bool more = c + 1 < nc;
    if (more) {
      pc = st_fetch(base, ld_qkv, dob, ld_do, j0 + ST_CH, N);
      sv = st_stat_fetch(lse_bh, delta_bh, j0 + ST_CH, N);
    }
#pragma unroll 1
    for (int qp = 0; qp < 2; ++qp)
      at_dkv_step(Qc, Oc, lse2, delta, qp * 32, j0 + qp * 32, off, g, kf, vf, c2, kvalid, key, 0, dk, dv);
    if (more) {
      st_commit(smem[(c + 1) & 1], pc, j0 + ST_CH, N);
      st_stat_commit(smem[(c + 1) & 1] + 2 * ST_IMG, sv);
    }
    __syncthreads();
  }
  if (kvalid) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dk[dt] *= scale;
    at_store_dkv(dqkv + ((int64_t)b * N + key) * ld_dqkv + h * 64, D, dk, dv, g);
  }
}

// ---------------------------------------------------------------------------
// Streamed f32 attention (N > 288 at the reference's fp32 precision: CLIP ViT-L/14@336px, 577 tokens): the
// resident f32 kernels' operand algebra -- v_mfma_f32_16x16x4_f32, a lane holding the 16 head dims
// [16g, 16g + 16) of its query (key), P / dS fed from registers, the kswz row image read by rows
// (f32_row16) and by columns (f32_chunk) -- on the streamed kernels' schedule: grid (B*H, ceil(N / 128)),
// a two-buffer LDS ring of 64-row chunks, the next chunk's global loads issued before the MFMA work on
// the current one and committed after it, one barrier per chunk.  An f32 chunk image is 64 x 256 B =
// 16 KiB, so a thread moves two 16-B pieces of each of the two images per chunk and the ring takes
// 64 KiB (+ 1 KiB of lse * log2(e) / delta strips in dkv).  Ragged ends, ownership and summation order
// follow the bf16 streamed kernels: one owner per output element, no atomics, bitwise repeatable.
// ---------------------------------------------------------------------------
constexpr int SF_IMG = ST_CH * 64;  // floats per f32 chunk image
static_assert(ST_CH * 16 == 2 * AT_THREADS, "two 16-B pieces of an f32 chunk image per thread");

struct SfPiece { f32x4 a[2], b[2]; };
// this thread's two pieces (rows r and r + 32 of the chunk) of rows [j0, j0 + 64) of two head slices
__device__ __forceinline__ SfPiece sf_fetch(const float* sa, int64_t lda, const float* sb, int64_t ldb, int j0, int N) {
  const int c = threadIdx.x & 15;
  SfPiece p;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = min(j0 + u * 32 + (int)(threadIdx.x >> 4), N - 1);
    p.a[u] = *reinterpret_cast<const f32x4*>(sa + (int64_t)row * lda + c * 4);
    p.b[u] = *reinterpret_cast<const f32x4*>(sb + (int64_t)row * ldb + c * 4);
  }
  return p;
}
__device__ __forceinline__ void sf_commit(float* buf, SfPiece p, int j0, int N) {
  const int c = threadIdx.x & 15;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int r = u * 32 + (int)(threadIdx.x >> 4);
    if (j0 + r >= N) { p.a[u] = f32x4{0.f, 0.f, 0.f, 0.f}; p.b[u] = p.a[u]; }
    const int at = r * 64 + ((c ^ kswz(r)) << 2);
    *reinterpret_cast<f32x4*>(buf + at) = p.a[u];
    *reinterpret_cast<f32x4*>(buf + SF_IMG + at) = p.b[u];
  }
}
constexpr int SF_LDS = 2 * 2 * SF_IMG * 4;                      // fwd, dq: [buffer][K | V]
constexpr int SF_BUF_DKV = 2 * SF_IMG + 2 * ST_CH;              // floats: Q | dO | lse * log2(e) | delta
constexpr int SF_LDS_DKV = 2 * SF_BUF_DKV * 4;

__global__ __launch_bounds__(AT_THREADS, 4) void attn_fwd_stream_f32(const float* __restrict__ qkv, int64_t ld_qkv, int D,
                                                                    int H, int N, float scale, float* __restrict__ o,
                                                                    int64_t ld_o, float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* ring = reinterpret_cast<float*>(smem);
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
  const float* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const int q = blockIdx.y * ST_QB + wave * 16 + l15;
  float qf[16];
  f32_glob16(base + (int64_t)min(q, N - 1) * ld_qkv + 16 * g, qf);
  const int nc = (N + ST_CH - 1) / ST_CH;
  SfPiece pc = sf_fetch(base + D, ld_qkv, base + 2 * D, ld_qkv, 0, N);
  sf_commit(ring, pc, 0, N);
  __syncthreads();
  const float c2 = scale * LOG2E;
  float m = -INFINITY, l = 0.f;  // running max (raw scores, all 4 lanes of a query agree); this lane's part of the sum
  f32x4 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int c = 0; c < nc; ++c) {
    const float* Kc = ring + (c & 1) * 2 * SF_IMG;
    const float* Vc = Kc + SF_IMG;
    const int j0 = c * ST_CH;
    const bool more = c + 1 < nc;
    if (more) pc = sf_fetch(base + D, ld_qkv, base + 2 * D, ld_qkv, j0 + ST_CH, N);
    f32x4 s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {  // one key tile's K rows live at a time: the 128-register budget
      float kf[16];
      f32_row16(Kc, kt * 16 + l15, g, kf);
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) s[kt] = mfma4(kf[ks], qf[ks], s[kt]);  // S^T[key 4g + r][query l15]
      if (kt % 2 == 1) __builtin_amdgcn_sched_barrier(0);  // bound K-row hoisting (VGPRs)
    }
    st_softmax_chunk(s, j0, N, g, c2, m, l, oacc);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const f32x4 v = f32_chunk(Vc, kt * 16 + 4 * g + r, l15);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) oacc[dt] = mfma4(v[dt], s[kt][r], oacc[dt]);
      }
    if (more) sf_commit(ring + ((c + 1) & 1) * 2 * SF_IMG, pc, j0 + ST_CH, N);
    __syncthreads();
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (q < N)
    f32_store_o(o + ((int64_t)b * N + q) * ld_o + h * 64 + 16 * g, lse, (int64_t)bh * N + q, oacc, l, m * c2, g);
}

// query-parallel half of the streamed f32 backward: delta = rowsum(dO * O) and dQ (f32_qrow, f32_dq_step per chunk)
__global__ __launch_bounds__(AT_THREADS, 4) void attn_bwd_dq_stream_f32(
    const float* __restrict__ qkv, int64_t ld_qkv, int D, int H, int N, float scale, const float* __restrict__ o,
    int64_t ld_o, const float* __restrict__ dout, int64_t ld_do, const float* __restrict__ lse,
    float* __restrict__ delta_out, float* __restrict__ dqkv, int64_t ld_dqkv) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* ring = reinterpret_cast<float*>(smem);
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
  const float* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const int q = blockIdx.y * ST_QB + wave * 16 + l15;
  float qf[16], df[16], dl, l2;
  f32_qrow(base, ld_qkv, dout + (int64_t)b * N * ld_do + h * 64, ld_do, o + (int64_t)b * N * ld_o + h * 64, ld_o,
           lse + (int64_t)bh * N, delta_out + (int64_t)bh * N, q, N, g, qf, df, dl, l2);
  const int nc = (N + ST_CH - 1) / ST_CH;
  SfPiece pc = sf_fetch(base + D, ld_qkv, base + 2 * D, ld_qkv, 0, N);
  sf_commit(ring, pc, 0, N);
  __syncthreads();
  const float c2 = scale * LOG2E;
  f32x4 dq[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int c = 0; c < nc; ++c) {
    const float* Kc = ring + (c & 1) * 2 * SF_IMG;
    const float* Vc = Kc + SF_IMG;
    const int j0 = c * ST_CH;
    const bool more = c + 1 < nc;
    if (more) pc = sf_fetch(base + D, ld_qkv, base + 2 * D, ld_qkv, j0 + ST_CH, N);
#pragma unroll 1
    for (int kt = 0; kt < 4; ++kt)
      f32_dq_step(Kc, Vc, kt * 16, j0 + kt * 16, N, l15, g, qf, df, c2, l2, dl, q, 0, dq);
    if (more) sf_commit(ring + ((c + 1) & 1) * 2 * SF_IMG, pc, j0 + ST_CH, N);
    __syncthreads();
  }
  if (q < N) f32_store_row(dqkv + ((int64_t)b * N + q) * ld_dqkv + h * 64 + 16 * g, dq, scale);
}

// key-parallel half: dK, dV of the workgroup's 128 keys (K, V rows in registers) over streamed Q / dO chunks.
// kf, vf, dk, dv are 64 live values per lane before the chunk's own operands: one workgroup per CU
// (256-register budget), where the other two kernels keep the 128-register budget of two.
__global__ __launch_bounds__(AT_THREADS, 2) void attn_bwd_dkv_stream_f32(
    const float* __restrict__ qkv, int64_t ld_qkv, int D, int H, int N, float scale, const float* __restrict__ dout,
    int64_t ld_do, const float* __restrict__ lse, const float* __restrict__ delta_in, float* __restrict__ dqkv,
    int64_t ld_dqkv) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* ring = reinterpret_cast<float*>(smem);
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const float* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const float* dob = dout + (int64_t)b * N * ld_do + h * 64;
  const int key = blockIdx.y * ST_QB + wave * 16 + l15;
  const bool kvalid = key < N;
  float kf[16], vf[16];
  f32_krow(base, ld_qkv, D, min(key, N - 1), g, kf, vf);
  const float* lse_bh = lse + (int64_t)bh * N;
  const float* delta_bh = delta_in + (int64_t)bh * N;
  const int nc = (N + ST_CH - 1) / ST_CH;
  SfPiece pc = sf_fetch(base, ld_qkv, dob, ld_do, 0, N);
  float sv = st_stat_fetch(lse_bh, delta_bh, 0, N);
  sf_commit(ring, pc, 0, N);
  st_stat_commit(ring + 2 * SF_IMG, sv);
  __syncthreads();
  const float c2 = scale * LOG2E;
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) { dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[dt] = dk[dt]; }
#pragma unroll 1
  for (int c = 0; c < nc; ++c) {
    const float* Qc = ring + (c & 1) * SF_BUF_DKV;
    const float* Oc = Qc + SF_IMG;  // dO
    const float* l2s = Qc + 2 * SF_IMG;
    const float* dls = l2s + ST_CH;
    const int j0 = c * ST_CH;
    const bool more = c + 1 < nc;
    if (more) {
      pc = sf_fetch(base, ld_qkv, dob, ld_do, j0 + ST_CH, N);
      sv = st_stat_fetch(lse_bh, delta_bh, j0 + ST_CH, N);
    }
#pragma unroll 1
    for (int qt = 0; qt < 4; ++qt)
      f32_dkv_step(Qc, Oc, l2s, dls, qt * 16, j0 + qt * 16, l15, g, kf, vf, c2, kvalid, key, 0, dk, dv);
    if (more) {
      float* nb = ring + ((c + 1) & 1) * SF_BUF_DKV;
      sf_commit(nb, pc, j0 + ST_CH, N);
      st_stat_commit(nb + 2 * SF_IMG, sv);
    }
    __syncthreads();
  }
  if (kvalid) f32_store_dkv(dqkv + ((int64_t)b * N + key) * ld_dqkv + h * 64 + 16 * g, D, dk, dv, scale);
}

// ---------------------------------------------------------------------------
// Streamed f32 attention as three bf16 MFMA products ("high" + long, vit_sdpa_f32_long_precision(1)):
// the operand policy AtBf16x3 of the resident "high" kernels on the streamed schedule above -- the loop of
// attn_fwd_stream with st_softmax_chunk, at_dq_step / at_dkv_step per 32-row pair, x3_row for the wave's own rows.
// A ring buffer holds a hi and a lo bf16 image (64 rows x 128 B, at_off layout) of each of the two streamed
// matrices: 32 KiB a buffer, 64 KiB a ring, the bytes of the f32 ring (+ the lse * log2(e) / delta strip in dkv).
// A thread fetches one 8-float piece of each matrix as f32, holds it across the chunk's MFMA work and splits it at
// commit (x3_load2's rule, a chunk at a time: rows are clamped to N - 1 and pieces of rows >= N zeroed first).
// Ragged ends, ownership and summation order are the streamed kernels': one owner per output element, no atomics,
// bitwise repeatable.
// ---------------------------------------------------------------------------
constexpr int SX_BUF = 4 * ST_IMG;                   // bytes: A hi | A lo | B hi | B lo
constexpr int SX_LDS = 2 * SX_BUF;                   // fwd, dq: K, V
constexpr int SX_BUF_DKV = SX_BUF + 2 * ST_CH * 4;   // Q, dO | lse * log2(e) | delta
constexpr int SX_LDS_DKV = 2 * SX_BUF_DKV;
static_assert(SX_BUF_DKV % 16 == 0, "the second buffer's images stay 16-B aligned");

struct SxPiece { f32x4 a[2], b[2]; };
// this thread's 8-float piece of rows [j0, j0 + 64) of two f32 head slices (clamped to row N - 1)
__device__ __forceinline__ SxPiece sx_fetch(const float* sa, int64_t lda, const float* sb, int64_t ldb, int j0, int N) {
  const int row = min(j0 + (int)(threadIdx.x >> 3), N - 1), c = threadIdx.x & 7;
  SxPiece p;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    p.a[u] = *reinterpret_cast<const f32x4*>(sa + (int64_t)row * lda + c * 8 + u * 4);
    p.b[u] = *reinterpret_cast<const f32x4*>(sb + (int64_t)row * ldb + c * 8 + u * 4);
  }
  return p;
}
// The same from image rows: this thread's hi (a[0] / b[0]) and lo (a[1] / b[1]) chunk c
struct SxChunk { u32x4_ a[2], b[2]; };
__device__ __forceinline__ SxChunk sx_fetch_image(const float* sa, int64_t lda, const float* sb, int64_t ldb, int j0,
                                                  int N) {
  const int row = min(j0 + (int)(threadIdx.x >> 3), N - 1), c = threadIdx.x & 7;
  SxChunk p;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    p.a[u] = x3_chunk(sa + (int64_t)row * lda, c, u);
    p.b[u] = x3_chunk(sb + (int64_t)row * ldb, c, u);
  }
  return p;
}
__device__ __forceinline__ void sx_commit(char* buf, SxChunk p, int j0, int N) {
  const int r = threadIdx.x >> 3, c = threadIdx.x & 7;
  if (j0 + r >= N) {
    p.a[0] = u32x4_{0u, 0u, 0u, 0u};
    p.a[1] = p.a[0]; p.b[0] = p.a[0]; p.b[1] = p.a[0];
  }
  x3_put_chunk(buf, buf + ST_IMG, r, c, p.a[0], p.a[1]);
  x3_put_chunk(buf + 2 * ST_IMG, buf + 3 * ST_IMG, r, c, p.b[0], p.b[1]);
}
__device__ __forceinline__ void sx_commit(char* buf, SxPiece p, int j0, int N) {
  const int r = threadIdx.x >> 3, c = threadIdx.x & 7;
  if (j0 + r >= N) {
    p.a[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    p.a[1] = p.a[0]; p.b[0] = p.a[0]; p.b[1] = p.a[0];
  }
  bf16x8 h, l;
  split8<1>(p.a[0], p.a[1], h, l);
  *reinterpret_cast<bf16x8*>(buf + at_off(r, c)) = h;
  *reinterpret_cast<bf16x8*>(buf + ST_IMG + at_off(r, c)) = l;
  split8<1>(p.b[0], p.b[1], h, l);
  *reinterpret_cast<bf16x8*>(buf + 2 * ST_IMG + at_off(r, c)) = h;
  *reinterpret_cast<bf16x8*>(buf + 3 * ST_IMG + at_off(r, c)) = l;
}
// The streamed kernels' name for the policy: at_dq_step / at_dkv_step instantiated on it are functions of their own,
// so the resident attn_bwd_*_f32x3 kernels keep the instruction streams they had before these kernels shared the
// steps (tools/isa_digest.sh --compare).
struct AtBf16x3St : AtBf16x3 {};
// matrix mtx (0: A, 1: B) of a ring buffer
__device__ __forceinline__ AtBf16x3::Img sx_img(const char* buf, int mtx) {
  return {buf + 2 * mtx * ST_IMG, buf + (2 * mtx + 1) * ST_IMG};
}

// The streamed "high" forward, for attn_fwd_stream_x3 (f32 qkv and o) and attn_fwd_image_stream (both as images).
template <bool IMAGE>
__device__ __forceinline__ auto sx_fetch_kv(const float* base, int64_t ld_qkv, int D, int j0, int N) {
  if constexpr (IMAGE)
    return sx_fetch_image(base + D, ld_qkv, base + 2 * D, ld_qkv, j0, N);
  else
    return sx_fetch(base + D, ld_qkv, base + 2 * D, ld_qkv, j0, N);
}
template <bool IMAGE>
__device__ __forceinline__ void sx_fwd(const float* qkv, int64_t ld_qkv, int D, int H, int N, float scale, float* o,
                                       int64_t ld_o, float* lse) {
  using X = AtBf16x3;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  const float* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const int q = blockIdx.y * ST_QB + wave * 16 + (lane & 15);
  X::Frag qf[2];
  if constexpr (IMAGE) {
    x3_row_image(base + (int64_t)min(q, N - 1) * ld_qkv, g, qf);
  } else {
    f32x4 x[4];
    x3_row(base + (int64_t)min(q, N - 1) * ld_qkv, g, qf, x);
  }
  const AtOffsets off(lane);
  const int nc = (N + ST_CH - 1) / ST_CH;
  auto pc = sx_fetch_kv<IMAGE>(base, ld_qkv, D, 0, N);
  sx_commit(smem, pc, 0, N);
  __syncthreads();
  const float c2 = scale * LOG2E;
  float m = -INFINITY, l = 0.f;  // running max (raw scores, all 4 lanes of a query agree); this lane's part of the sum
  f32x4 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int c = 0; c < nc; ++c) {
    const char* buf = smem + (c & 1) * SX_BUF;
    const X::Img Kimg = sx_img(buf, 0), Vimg = sx_img(buf, 1);
    const int j0 = c * ST_CH;
    const bool more = c + 1 < nc;
    if (more) pc = sx_fetch_kv<IMAGE>(base, ld_qkv, D, j0 + ST_CH, N);
    f32x4 s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) s[kt] = X::mma(X::row(Kimg, kt * 16, off.row[kk]), qf[kk], s[kt]);
      if (kt % 2 == 1) __builtin_amdgcn_sched_barrier(0);  // bound K-fragment hoisting (VGPRs)
    }
    st_softmax_chunk(s, j0, N, g, c2, m, l, oacc);  // on the f32 scores; the row sum is of the unsplit p
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const X::Frag pf = X::pack(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) oacc[dt] = X::mma(X::tr(Vimg, ks * 32, off.tr[dt]), pf, oacc[dt]);
    }
    if (more) sx_commit(smem + ((c + 1) & 1) * SX_BUF, pc, j0 + ST_CH, N);
    __syncthreads();
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (q < N) {
    if constexpr (IMAGE)
      x3_store_row_image(o + ((int64_t)b * N + q) * ld_o + h * 64, oacc, 1.0f / l, g);
    else
      x3_store_row(o + ((int64_t)b * N + q) * ld_o + h * 64, oacc, 1.0f / l, g);
    if (g == 0) lse[(int64_t)bh * N + q] = (m * c2 + __log2f(l)) * LN2;
  }
}
__global__ __launch_bounds__(AT_THREADS, 4) void attn_fwd_stream_x3(const float* __restrict__ qkv, int64_t ld_qkv, int D,
                                                                   int H, int N, float scale, float* __restrict__ o,
                                                                   int64_t ld_o, float* __restrict__ lse) {
  sx_fwd<false>(qkv, ld_qkv, D, H, N, scale, o, ld_o, lse);
}
// qkv and o hold pre-split images; o and lse are attn_fwd_stream_x3's bit for bit (o as its image)
__global__ __launch_bounds__(AT_THREADS, 4) void attn_fwd_image_stream(const float* __restrict__ qkv, int64_t ld_qkv,
                                                                         int D, int H, int N, float scale,
                                                                         float* __restrict__ o, int64_t ld_o,
                                                                         float* __restrict__ lse) {
  sx_fwd<true>(qkv, ld_qkv, D, H, N, scale, o, ld_o, lse);
}

// query-parallel half of the streamed "high" backward: delta = rowsum(dO * O) on the unsplit f32 values (as in
// attn_bwd_dq_f32x3) and dQ (at_dq_step<AtBf16x3> per 32-key pair of a chunk)
__global__ __launch_bounds__(AT_THREADS, 4) void attn_bwd_dq_stream_x3(
    const float* __restrict__ qkv, int64_t ld_qkv, int D, int H, int N, float scale, const float* __restrict__ o,
    int64_t ld_o, const float* __restrict__ dout, int64_t ld_do, const float* __restrict__ lse,
    float* __restrict__ delta_out, float* __restrict__ dqkv, int64_t ld_dqkv) {
  using X = AtBf16x3;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  const float* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const int q = blockIdx.y * ST_QB + wave * 16 + (lane & 15), qc = min(q, N - 1);
  X::Frag qf[2], of[2];
  float dl = 0.f;
  {
    const float* dorow = dout + ((int64_t)b * N + qc) * ld_do + h * 64;
    const float* orow = o + ((int64_t)b * N + qc) * ld_o + h * 64;
    f32x4 x[4], df[4];
    x3_row(base + (int64_t)qc * ld_qkv, g, qf, x);
    x3_row(dorow, g, of, df);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 ov = *reinterpret_cast<const f32x4*>(orow + (j >> 1) * 32 + g * 8 + (j & 1) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) dl = fmaf(df[j][e], ov[e], dl);
    }
  }
  dl += __shfl_xor(dl, 16, 64);
  dl += __shfl_xor(dl, 32, 64);
  if (q < N && g == 0) delta_out[(int64_t)bh * N + q] = dl;
  const float l2 = lse[(int64_t)bh * N + qc] * LOG2E;
  const AtOffsets off(lane);
  const int nc = (N + ST_CH - 1) / ST_CH;
  SxPiece pc = sx_fetch(base + D, ld_qkv, base + 2 * D, ld_qkv, 0, N);
  sx_commit(smem, pc, 0, N);
  __syncthreads();
  const float c2 = scale * LOG2E;
  f32x4 dq[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int c = 0; c < nc; ++c) {
    const char* buf = smem + (c & 1) * SX_BUF;
    const X::Img Kimg = sx_img(buf, 0), Vimg = sx_img(buf, 1);
    const int j0 = c * ST_CH;
    const bool more = c + 1 < nc;
    if (more) pc = sx_fetch(base + D, ld_qkv, base + 2 * D, ld_qkv, j0 + ST_CH, N);
    const bool edge = j0 + ST_CH > N;  // wave-uniform: only the last chunk holds keys >= N
#pragma unroll 1
    for (int kp = 0; kp < 2; ++kp)
      at_dq_step<AtBf16x3St>(Kimg, Vimg, kp * 32, j0 + kp * 32, N, edge, off, g, qf, of, c2, l2, dl, q, 0, dq);
    if (more) sx_commit(smem + ((c + 1) & 1) * SX_BUF, pc, j0 + ST_CH, N);
    __syncthreads();
  }
  if (q < N) x3_store_row(dqkv + ((int64_t)b * N + q) * ld_dqkv + h * 64, dq, scale, g);
}

// key-parallel half: dK, dV of the workgroup's 128 keys (K, V rows split in registers) over streamed Q / dO chunks.
// kf, vf (hi and lo), dk and dv are 64 live registers before the chunk's own operands: the 256-register budget, as
// attn_bwd_dkv_stream_f32.
__global__ __launch_bounds__(AT_THREADS, 2) void attn_bwd_dkv_stream_x3(
    const float* __restrict__ qkv, int64_t ld_qkv, int D, int H, int N, float scale, const float* __restrict__ dout,
    int64_t ld_do, const float* __restrict__ lse, const float* __restrict__ delta_in, float* __restrict__ dqkv,
    int64_t ld_dqkv) {
  using X = AtBf16x3;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  const float* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  const float* dob = dout + (int64_t)b * N * ld_do + h * 64;
  const int key = blockIdx.y * ST_QB + wave * 16 + (lane & 15), kc = min(key, N - 1);
  const bool kvalid = key < N;
  X::Frag kf[2], vf[2];
  {
    f32x4 x[4];
    x3_row(base + (int64_t)kc * ld_qkv + D, g, kf, x);
    x3_row(base + (int64_t)kc * ld_qkv + 2 * D, g, vf, x);
  }
  const float* lse_bh = lse + (int64_t)bh * N;
  const float* delta_bh = delta_in + (int64_t)bh * N;
  const AtOffsets off(lane);
  const int nc = (N + ST_CH - 1) / ST_CH;
  SxPiece pc = sx_fetch(base, ld_qkv, dob, ld_do, 0, N);
  float sv = st_stat_fetch(lse_bh, delta_bh, 0, N);
  sx_commit(smem, pc, 0, N);
  st_stat_commit(smem + SX_BUF, sv);
  __syncthreads();
  const float c2 = scale * LOG2E;
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) { dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[dt] = dk[dt]; }
#pragma unroll 1
  for (int c = 0; c < nc; ++c) {
    const char* buf = smem + (c & 1) * SX_BUF_DKV;
    const X::Img Qimg = sx_img(buf, 0), Oimg = sx_img(buf, 1);  // O: dO
    const float* lse2 = reinterpret_cast<const float*>(buf + SX_BUF);
    const float* delta = lse2 + ST_CH;
    const int j0 = c * ST_CH;
    const bool more = c + 1 < nc;
    if (more) {
      pc = sx_fetch(base, ld_qkv, dob, ld_do, j0 + ST_CH, N);
      sv = st_stat_fetch(lse_bh, delta_bh, j0 + ST_CH, N);
    }
#pragma unroll 1
    for (int qp = 0; qp < 2; ++qp)
      at_dkv_step<AtBf16x3St>(Qimg, Oimg, lse2, delta, qp * 32, j0 + qp * 32, off, g, kf, vf, c2, kvalid, key, 0, dk, dv);
    if (more) {
      char* nb = smem + ((c + 1) & 1) * SX_BUF_DKV;
      sx_commit(nb, pc, j0 + ST_CH, N);
      st_stat_commit(nb + SX_BUF, sv);
    }
    __syncthreads();
  }
  if (kvalid) {
    float* row = dqkv + ((int64_t)b * N + key) * ld_dqkv + h * 64;
    x3_store_row(row + D, dk, scale, g);
    x3_store_row(row + 2 * D, dv, 1.f, g);
  }
}

// qkv-bias gradient partials past 288 tokens: part[b][c] = sum over the image's N rows of dqkv[.][c], one
// thread per column, rows in a fixed order (8 interleaved chains) -- the [B][3D] layout the resident
// kernels leave.  It reads dqkv once, a few percent of the bytes the two backward kernels move.
__global__ __launch_bounds__(256) void attn_bias_image(const bf16* __restrict__ dqkv, int64_t ld, int N, int C,
                                                       float* __restrict__ part) {
  const int b = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (c >= C) return;
  const bf16* p = dqkv + (int64_t)b * N * ld + c;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int n = 0;
  for (; n + 8 <= N; n += 8)
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] += (float)p[(int64_t)(n + u) * ld];
  for (; n < N; ++n) a[0] += (float)p[(int64_t)n * ld];
  part[(int64_t)b * C + c] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// Past 288 tokens (vit_sdpa_long_config / VIT_ATTN_LONG): 1 = the streamed MFMA kernels (default),
// 0 = the generic kernels.  g_long_count: vit_sdpa_fwd / vit_sdpa_bwd calls that took the streamed kernels.
static int g_long_mode = -1;
static int g_long_count = 0;      // bf16 streamed calls
static int g_long_f32_count = 0;  // f32 streamed calls
static int g_fp8_stream_count = 0;  // vit_sdpa_fwd_fp8_stream calls
static int g_fp8_pre_count = 0;     // vit_sdpa_fwd_fp8_pre calls
static bool attn_long_stream() {
  if (g_long_mode >= 0) return g_long_mode != 0;
  static const int v = [] { const char* e = getenv("VIT_ATTN_LONG"); return e && *e == '0' ? 0 : 1; }();
  return v != 0;
}
constexpr int AT_RESIDENT_MAX = 288;  // the resident kernels' token limit (by_tiles)
// VIT_ATTN_F32_GENERIC=1: the scalar-FMA f32 kernels instead of the f32 MFMA ones (A/B runs); f32 only
static bool attn_f32_generic() {
  static const int v = [] { const char* e = getenv("VIT_ATTN_F32_GENERIC"); return e && *e == '1' ? 1 : 0; }();
  return v != 0;
}

// Which kernel family a vit_sdpa_fwd / vit_sdpa_bwd call takes (attention dispatch table).
// aligned: every row stride of the call meets the family's vector width -- bf16 forward ld_qkv % 8, ld_o % 4,
// backward also ld_do % 8, ld_dqkv % 4; f32 every stride % 4.
enum AttnPath { AP_RESIDENT_BF16, AP_RESIDENT_F32, AP_STREAM_BF16, AP_STREAM_F32, AP_GENERIC };
static AttnPath attn_path(int dtype, int N, int causal, bool aligned) {
  const bool resident = N <= AT_RESIDENT_MAX;
  if (aligned && (dtype == VIT_BF16 || (dtype == VIT_F32 && !attn_f32_generic()))) {
    if (resident) return dtype == VIT_BF16 ? AP_RESIDENT_BF16 : AP_RESIDENT_F32;
    // a causal streamed form is out of scope: it takes the generic kernels
    if (!causal && attn_long_stream()) return dtype == VIT_BF16 ? AP_STREAM_BF16 : AP_STREAM_F32;
  }
  return AP_GENERIC;
}

// Kernels whose LDS is past the 64 KiB static limit take it as dynamic LDS; each family raises the
// attribute once, behind a static flag.
template <typename K>
static void raise_lds(K* kernel, int bytes) {
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}
static void stream_f32_attrs() {
  static bool attr = false;
  if (attr) return;
  raise_lds(attn_fwd_stream_f32, SF_LDS);
  raise_lds(attn_bwd_dq_stream_f32, SF_LDS);
  raise_lds(attn_bwd_dkv_stream_f32, SF_LDS_DKV);
  attr = true;
}
static void stream_x3_attrs() {
  static bool attr = false;
  if (attr) return;
  raise_lds(attn_fwd_stream_x3, SX_LDS);
  raise_lds(attn_bwd_dq_stream_x3, SX_LDS);
  raise_lds(attn_bwd_dkv_stream_x3, SX_LDS_DKV);
  attr = true;
}
// The two resident f32 kernel families behind one interface, for fwd_f32 / bwd_f32 below: SPLIT, THREADS, the
// dynamic LDS sizes LDS / LDS_DKV and the kernels fwd(causal), dq(), dkv().
template <int NT>
struct F32Res {  // f32 MFMA: two head images of NT * 16 rows (+ lse / delta strips in dkv)
  static constexpr bool SPLIT = false;
  static constexpr int THREADS = 512;
  static constexpr int IMG = NT * 16 * 64 * 4, LDS = 2 * IMG, LDS_DKV = 2 * IMG + 2 * NT * 16 * 4;
  static auto fwd(int) { return attn_fwd_f32mfma<NT>; }  // the mask is a kernel argument
  static auto dq() { return attn_bwd_dq_f32mfma<NT>; }
  static auto dkv() { return attn_bwd_dkv_f32mfma<NT>; }
};
template <int NT>
struct F32X3Res : F32X3<NT> {  // bf16x3: F32X3's layout constants and the kernels defined behind them
  static constexpr bool SPLIT = true;
  static constexpr int THREADS = AT_THREADS;
  // the mask is a template argument, as in fwd_mfma
  static auto fwd(int causal) { return causal ? attn_fwd_f32x3<NT, true> : attn_fwd_f32x3<NT, false>; }
  static auto fwd_image(int causal) { return causal ? attn_fwd_image_x3<NT, true> : attn_fwd_image_x3<NT, false>; }
  static auto dq() { return attn_bwd_dq_f32x3<NT>; }
  static auto dkv() { return attn_bwd_dkv_f32x3<NT>; }
};
template <typename F>
static void f32_attrs() {
  static bool attr = false;
  if (attr) return;
  raise_lds(F::fwd(0), F::LDS);
  raise_lds(F::fwd(1), F::LDS);
  raise_lds(F::dq(), F::LDS);
  raise_lds(F::dkv(), F::LDS_DKV);
  attr = true;
}
// fp32 arithmetic of the resident f32 kernels (vit_sdpa_f32_precision): 0 = v_mfma_f32_16x16x4_f32, 1 = bf16x3
// (the attn_*_f32x3 kernels).  Process-wide, read at launch time; the initial value comes from VIT_F32_ATTENTION
// (highest | high, default highest).  g_f32_split_count: vit_sdpa_fwd / vit_sdpa_bwd calls that took them.
static int f32_attention_env() {
  const char* s = getenv("VIT_F32_ATTENTION");
  return s && !strcmp(s, "high") ? 1 : 0;
}
static int g_f32_split = f32_attention_env();
static int g_f32_split_count = 0;
// The same choice for the streamed f32 kernels past 288 tokens (vit_sdpa_f32_long_precision): 1 = bf16x3 (the
// attn_*_stream_x3 kernels), honoured only while g_f32_split is 1 too.  Initial value from VIT_F32_ATTENTION_LONG=1.
// g_long_f32_split_count: vit_sdpa_fwd / vit_sdpa_bwd calls that took them (g_long_f32_count counts those too).
static int f32_attention_long_env() {
  const char* s = getenv("VIT_F32_ATTENTION_LONG");
  return s && !strcmp(s, "1") ? 1 : 0;
}
static int g_f32_long = f32_attention_long_env();
static int g_long_f32_split_count = 0;
static bool stream_f32_split() { return g_f32_split && g_f32_long; }

// ---------------------------------------------------------------------------
template <int NT>
static int fwd_mfma(const void* qkv, int64_t ld_qkv, int D, int B, int H, int N, float scale, int causal, void* o,
                    int64_t ld_o, float* lse, hipStream_t s) {
  // the causal mask is a compile-time choice: as a runtime flag its per-score compares and selects
  // stayed in the unmasked kernel's softmax loop (≈130 of ≈400 VALU instructions per query tile)
  if (causal)
    hipLaunchKernelGGL((attn_fwd_mfma<NT, false, true>), dim3(B * H), dim3(AT_THREADS), 0, s, (const bf16*)qkv, ld_qkv,
                       D, H, N, scale, (bf16*)o, ld_o, lse, causal, nullptr);
  else if (g_attn_stamps)
    hipLaunchKernelGGL((attn_fwd_mfma<NT, true>), dim3(B * H), dim3(AT_THREADS), 0, s, (const bf16*)qkv, ld_qkv, D, H,
                       N, scale, (bf16*)o, ld_o, lse, causal, g_attn_stamps);
  else
    hipLaunchKernelGGL((attn_fwd_mfma<NT>), dim3(B * H), dim3(AT_THREADS), 0, s, (const bf16*)qkv, ld_qkv, D, H, N,
                       scale, (bf16*)o, ld_o, lse, causal, nullptr);
  VIT_CHECK_LAUNCH();
  return 0;
}
// The resident f32 forward and backward of either family F (F32Res<NT> or F32X3Res<NT>; the callers choose by
// g_f32_split).
template <typename F>
static int fwd_f32(const void* qkv, int64_t ld_qkv, int D, int B, int H, int N, float scale, int causal, void* o,
                   int64_t ld_o, float* lse, hipStream_t s) {
  f32_attrs<F>();
  if constexpr (F::SPLIT)
    hipLaunchKernelGGL(F::fwd(causal), dim3(B * H), dim3(F::THREADS), F::LDS, s, (const float*)qkv, ld_qkv, D, H, N,
                       scale, (float*)o, ld_o, lse);
  else
    hipLaunchKernelGGL(F::fwd(causal), dim3(B * H), dim3(F::THREADS), F::LDS, s, (const float*)qkv, ld_qkv, D, H, N,
                       scale, (float*)o, ld_o, lse, causal);
  VIT_CHECK_LAUNCH();
  g_f32_split_count += F::SPLIT;
  return 0;
}
template <typename F>
static int bwd_f32(const void* qkv, int64_t ld_qkv, int D, int B, int H, int N, float scale, int causal, const void* o,
                   int64_t ld_o, const void* dout, int64_t ld_do, const float* lse, float* delta, void* dqkv,
                   int64_t ld_dqkv, hipStream_t s) {
  f32_attrs<F>();
  hipLaunchKernelGGL(F::dq(), dim3(B * H), dim3(F::THREADS), F::LDS, s, (const float*)qkv, ld_qkv, D, H, N, scale,
                     (const float*)o, ld_o, (const float*)dout, ld_do, lse, delta, (float*)dqkv, ld_dqkv, causal);
  VIT_CHECK_LAUNCH();
  hipLaunchKernelGGL(F::dkv(), dim3(B * H), dim3(F::THREADS), F::LDS_DKV, s, (const float*)qkv, ld_qkv, D, H, N, scale,
                     (const float*)dout, ld_do, lse, (const float*)delta, (float*)dqkv, ld_dqkv, causal);
  VIT_CHECK_LAUNCH();
  g_f32_split_count += F::SPLIT;
  return 0;
}
// The image form of the resident "high" forward: fwd_f32<F32X3Res<NT>> with qkv and o as pre-split
// images.  g_f32_image_count: vit_sdpa_fwd_image calls that launched (they count in g_f32_split_count or
// g_long_f32_split_count too, as the f32 forms do).
static int g_f32_image_count = 0;
template <int NT>
static int fwd_f32_image(const void* qkv, int64_t ld_qkv, int D, int B, int H, int N, float scale, int causal, void* o,
                         int64_t ld_o, float* lse, hipStream_t s) {
  using F = F32X3Res<NT>;
  static bool attr = false;
  if (!attr) {
    raise_lds(F::fwd_image(0), F::LDS);
    raise_lds(F::fwd_image(1), F::LDS);
    attr = true;
  }
  hipLaunchKernelGGL(F::fwd_image(causal), dim3(B * H), dim3(F::THREADS), F::LDS, s, (const float*)qkv, ld_qkv, D, H, N,
                     scale, (float*)o, ld_o, lse);
  VIT_CHECK_LAUNCH();
  ++g_f32_split_count;
  ++g_f32_image_count;
  return 0;
}
// The generic backward: any token count and alignment, causal or not.
template <typename T>
static int bwd_generic(const void* qkv, int64_t ld_qkv, int D, int B, int H, int N, float scale, int causal,
                       const void* o, int64_t ld_o, const void* dout, int64_t ld_do, const float* lse, float* delta,
                       void* dqkv, int64_t ld_dqkv, hipStream_t s) {
  if ((int64_t)B * H > 65535) return (int)hipErrorInvalidValue;  // the generic kernels put b*h on grid.y
  const dim3 grid((N + 63) / 64, B * H);
  hipLaunchKernelGGL(attn_bwd_dq_generic<T>, grid, dim3(256), 0, s, (const T*)qkv, ld_qkv, D, H, N, scale, (const T*)o,
                     ld_o, (const T*)dout, ld_do, lse, delta, (T*)dqkv, ld_dqkv, causal);
  VIT_CHECK_LAUNCH();
  hipLaunchKernelGGL(attn_bwd_dkv_generic<T>, grid, dim3(256), 0, s, (const T*)qkv, ld_qkv, D, H, N, scale,
                     (const T*)dout, ld_do, lse, delta, (T*)dqkv, ld_dqkv, causal);
  VIT_CHECK_LAUNCH();
  return 0;
}
// bf16 backward form for N <= 224 (vit_sdpa_bwd_variant / VIT_ATTN_BWD_SPLIT=1, A/B): 1 = whole-head fused
// (the default), 2 = the two kernels for every N.  (Round 4's banded-query form measured 0.276 vs 0.248 ms
// standalone and -0.8 % in the step, profiles/r04/ab_attn_bwd_band.txt, and was removed in round 5.)
static int g_bwd_variant = -1;
static bool attn_bwd_split() {
  if (g_bwd_variant == 2) return true;
  static const int v = [] { const char* e = getenv("VIT_ATTN_BWD_SPLIT"); return e && *e == '1' ? 1 : 0; }();
  return v != 0;
}

template <int NT>
static int bwd_mfma(const void* qkv, int64_t ld_qkv, int D, int B, int H, int N, float scale, int causal, const void* o,
                    int64_t ld_o, const void* dout, int64_t ld_do, const float* lse, float* delta,
                    void* dqkv, int64_t ld_dqkv, float* bias_part, hipStream_t s) {
  if constexpr (NT <= 14) {
    if (!attn_bwd_split()) {
      static bool attr = false;
      if (!attr) {
        raise_lds(attn_bwd_fused<NT>, BwdF<NT>::LDS);
        raise_lds(attn_bwd_fused<NT, true>, BwdF<NT>::LDS);
        raise_lds(attn_bwd_fused<NT, false, true>, BwdF<NT>::LDS);
        attr = true;
      }
#define BWD_FUSED(C, S, ST)                                                                                    \
  hipLaunchKernelGGL((attn_bwd_fused<NT, C, S>), dim3(B * H), dim3(BwdF<NT>::THREADS), BwdF<NT>::LDS, s,         \
                     (const bf16*)qkv, ld_qkv, D, H, N, scale, (const bf16*)o, ld_o, (const bf16*)dout, ld_do, lse, \
                     delta, (bf16*)dqkv, ld_dqkv, bias_part, ST)
      if (causal)
        BWD_FUSED(true, false, nullptr);
      else if (g_attn_stamps)
        BWD_FUSED(false, true, g_attn_stamps);
      else
        BWD_FUSED(false, false, nullptr);
#undef BWD_FUSED
      VIT_CHECK_LAUNCH();
      return 0;
    }
  }
  hipLaunchKernelGGL((attn_bwd_dq<NT>), dim3(B * H), dim3(AT_THREADS), 0, s, (const bf16*)qkv, ld_qkv, D, H, N, scale,
                     (const bf16*)o, ld_o, (const bf16*)dout, ld_do, lse, delta, (bf16*)dqkv, ld_dqkv, bias_part, causal);
  VIT_CHECK_LAUNCH();
  hipLaunchKernelGGL((attn_bwd_dkv<NT>), dim3(B * H), dim3(AT_THREADS), 0, s, (const bf16*)qkv, ld_qkv, D, H, N, scale,
                     (const bf16*)dout, ld_do, lse, (const float*)delta, (bf16*)dqkv, ld_dqkv, bias_part, causal);
  VIT_CHECK_LAUNCH();
  return 0;
}

template <int NT>
static int fwd_mfma_cls(const void* qkv, int64_t ld_qkv, int D, int B, int H, int N, float scale, void* o, int64_t ld_o,
                        float* lse, hipStream_t s) {
  hipLaunchKernelGGL((attn_fwd_mfma<NT, false, false, true>), dim3(B * H), dim3(AT_THREADS), 0, s, (const bf16*)qkv,
                     ld_qkv, D, H, N, scale, (bf16*)o, ld_o, lse, 0, nullptr);
  VIT_CHECK_LAUNCH();
  return 0;
}
static int g_cls_count = 0;

// ---------------------------------------------------------------------------
// One-query attention (the class-token tail of the CLIP visual tower): query row 0 of every
// image against all N keys and values, T = bf16 or float.  Memory-bound K / V reads with no reuse, so nothing
// is staged in LDS: one workgroup per (b, h), 8 lanes per key, each lane holding 8 of the 64 head dims (one 16-B
// load in bf16, two in f32), a wave 8 keys and the workgroup C1_GROUPS = 32 keys per step; f32 arithmetic
// throughout.  Every sum has a fixed order -- 8 FMAs in the lane, three xor-shuffles across the key's 8 lanes,
// keys g, g + 32, ... in sequence inside a lane group, then the 32 groups in index order through LDS -- so two
// calls give the same bits.  No atomics, no workspace.
// ---------------------------------------------------------------------------
constexpr int C1_THREADS = 256, C1_GROUPS = C1_THREADS / 8;
constexpr int C1_MAX_TOKENS = 2048;  // the entry points' bound: the backward keeps two floats a key in LDS

template <typename T> __device__ __forceinline__ void store8f(T* p, const float* x);
template <> __device__ __forceinline__ void store8f<bf16>(bf16* p, const float* x) {
  *reinterpret_cast<bf16x8*>(p) = bf16x8{(bf16)x[0], (bf16)x[1], (bf16)x[2], (bf16)x[3],
                                         (bf16)x[4], (bf16)x[5], (bf16)x[6], (bf16)x[7]};
}
template <> __device__ __forceinline__ void store8f<float>(float* p, const float* x) {
  *reinterpret_cast<f32x4*>(p) = f32x4{x[0], x[1], x[2], x[3]};
  *reinterpret_cast<f32x4*>(p + 4) = f32x4{x[4], x[5], x[6], x[7]};
}
// a . b over the 64 head dims of which this lane holds 8: the same value in all 8 lanes of the key's group
__device__ __forceinline__ float c1_dot(const float* a, const float* b) {
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 8; ++u) s = fmaf(a[u], b[u], s);
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  return s;
}

// The one-query forward of one (b, h), shared by attn_cls1_fwd (query row 0, all N keys) and attn_row1_fwd (a
// query row per sequence, causal or not): s_j = scale * (q . k_j) over keys j < nk, lse = logsumexp_j s_j,
// o = sum_j softmax(s)_j v_j -- an online softmax per lane group over its keys g, g + 32, ..., the groups merged
// in index order.  seq: the sequence's row 0 at this head's column plus this lane's 8 dims; the query is row qr.
// 1 <= nk: group 0 holds key 0, so the merged maximum is finite.  No row >= nk of K / V is read; the only stores
// are the head's 64 columns at o_head and one float at lse_dst.
template <typename T>
__device__ __forceinline__ void c1_fwd_body(const T* __restrict__ seq, int64_t ld_qkv, int D, int qr, int nk,
                                            float scale, T* __restrict__ o_head, float* __restrict__ lse_dst) {
  __shared__ float gm[C1_GROUPS], gl[C1_GROUPS], gacc[C1_GROUPS][64];
  const int g = threadIdx.x >> 3, c = threadIdx.x & 7;
  float q[8], acc[8];
  load8f<T>(seq + (int64_t)qr * ld_qkv, q);
#pragma unroll
  for (int u = 0; u < 8; ++u) acc[u] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int j = g; j < nk; j += C1_GROUPS) {
    float k[8], v[8];
    load8f<T>(seq + (int64_t)j * ld_qkv + D, k);
    load8f<T>(seq + (int64_t)j * ld_qkv + 2 * D, v);
    const float s = c1_dot(q, k) * scale;
    const float mn = fmaxf(m, s);
    const float corr = __expf(m - mn), p = __expf(s - mn);  // the group's first key: corr = exp(-inf) = 0
    l = l * corr + p;
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = acc[u] * corr + p * v[u];
    m = mn;
  }
  if (c == 0) { gm[g] = m; gl[g] = l; }
#pragma unroll
  for (int u = 0; u < 8; ++u) gacc[g][c * 8 + u] = acc[u];
  __syncthreads();
  if (threadIdx.x < 64) {
    // group 0 holds key 0, so M is finite; a group without keys (nk < 32) has m = -inf, l = 0 and weight 0
    float M = gm[0];
    for (int i = 1; i < C1_GROUPS; ++i) M = fmaxf(M, gm[i]);
    float Lsum = 0.f, od = 0.f;
    for (int i = 0; i < C1_GROUPS; ++i) {
      const float w = __expf(gm[i] - M);
      Lsum = fmaf(gl[i], w, Lsum);
      od = fmaf(gacc[i][threadIdx.x], w, od);
    }
    o_head[threadIdx.x] = (T)(od / Lsum);
    if (threadIdx.x == 0) *lse_dst = M + logf(Lsum);
  }
}

// Query row 0 of every image against all N keys.  o_cls row b at b * ld_o (column h * 64), lse_cls[b * H + h].
template <typename T>
__global__ __launch_bounds__(C1_THREADS) void attn_cls1_fwd(const T* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                            int N, float scale, T* __restrict__ o_cls, int64_t ld_o,
                                                            float* __restrict__ lse_cls) {
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  c1_fwd_body<T>(qkv + (int64_t)b * N * ld_qkv + h * 64 + (threadIdx.x & 7) * 8, ld_qkv, D, 0, N, scale,
                 o_cls + (int64_t)b * ld_o + h * 64, lse_cls + bh);
}

// Query row qrow[b] of sequence b (clamped to [0, N - 1]: the host never sees the values) against keys
// 0 .. nk - 1, nk = qrow[b] + 1 under the causal mask and N without it (the CLIP text tower's EOT rows, DESIGN
// §4.21).  o_row row b at b * ld_o (column h * 64), lse_row[b * H + h].  No backward: the caller takes this route
// only where no attention backward follows.
template <typename T>
__global__ __launch_bounds__(C1_THREADS) void attn_row1_fwd(const T* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                            int N, const int64_t* __restrict__ qrow, int causal,
                                                            float scale, T* __restrict__ o_row, int64_t ld_o,
                                                            float* __restrict__ lse_row) {
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  int64_t r = qrow[b];
  r = r < 0 ? 0 : (r > N - 1 ? N - 1 : r);
  const int qr = (int)r;
  c1_fwd_body<T>(qkv + (int64_t)b * N * ld_qkv + h * 64 + (threadIdx.x & 7) * 8, ld_qkv, D, qr, causal ? qr + 1 : N,
                 scale, o_row + (int64_t)b * ld_o + h * 64, lse_row + bh);
}

// p_j = exp(s_j - lse), delta = dO0 . o0, ds_j = p_j (dO0 . v_j - delta); dk_j = scale ds_j q0 and dv_j = p_j dO0 for
// every row, dq row 0 = scale sum_j ds_j k_j (k_j still in registers), dq rows 1 .. N-1 = 0: the whole 64-column
// slice of this head in dqkv [B*N, 3D] is written, by the lane group that read the row (row 0's dq after the merge).
//
// Consistency step.  In exact arithmetic sum_j ds_j = 0, and dq is the sum of ds_j (k_j - kbar): what a common
// offset of the keys contributes cancels.  o0 arrives rounded to T, so delta is off by e = dO0 . (o0 - o) and the
// sum by -e: in bf16, on keys with a large common offset, that alone puts dq 5e-2 of its largest magnitude off
// (17 tokens, q, k += 6).  The kernel knows r = sum_j ds_j and den = sum_j p_j when the keys are through, so it
// takes e = r / den back out: ds_j -= p_j r / den, that is dq -= scale (r / den) sum_j p_j k_j, and dk_j is written
// from the corrected ds_j, kept per key in LDS (two floats a key) until then.  K and V are still read once.
template <typename T>
__global__ __launch_bounds__(C1_THREADS) void attn_cls1_bwd(const T* __restrict__ qkv, int64_t ld_qkv, int D, int H,
                                                            int N, float scale, const T* __restrict__ o_cls,
                                                            int64_t ld_o, const T* __restrict__ do_cls, int64_t ld_do,
                                                            const float* __restrict__ lse_cls, T* __restrict__ dqkv,
                                                            int64_t ld_dqkv) {
  __shared__ float gacc[C1_GROUPS][64], gpk[C1_GROUPS][64], gr[C1_GROUPS], gden[C1_GROUPS];
  __shared__ float sds[C1_MAX_TOKENS], sp[C1_MAX_TOKENS];
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int g = threadIdx.x >> 3, c = threadIdx.x & 7;
  const T* base = qkv + (int64_t)b * N * ld_qkv + h * 64 + c * 8;
  T* dbase = dqkv + (int64_t)b * N * ld_dqkv + h * 64 + c * 8;
  float q[8], d0[8], o0[8], acc[8], pk[8], zero[8];
  load8f<T>(base, q);
  load8f<T>(do_cls + (int64_t)b * ld_do + h * 64 + c * 8, d0);
  load8f<T>(o_cls + (int64_t)b * ld_o + h * 64 + c * 8, o0);
  const float delta = c1_dot(d0, o0), lse = lse_cls[bh];
#pragma unroll
  for (int u = 0; u < 8; ++u) { acc[u] = 0.f; pk[u] = 0.f; zero[u] = 0.f; }
  float r = 0.f, den = 0.f;
  for (int j = g; j < N; j += C1_GROUPS) {
    float k[8], v[8], dv[8];
    load8f<T>(base + (int64_t)j * ld_qkv + D, k);
    load8f<T>(base + (int64_t)j * ld_qkv + 2 * D, v);
    const float p = __expf(c1_dot(q, k) * scale - lse);
    const float ds = p * (c1_dot(d0, v) - delta);  // the same value in the key's 8 lanes
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc[u] = fmaf(ds, k[u], acc[u]);
      pk[u] = fmaf(p, k[u], pk[u]);
      dv[u] = p * d0[u];
    }
    r += ds;
    den += p;
    if (c == 0) { sds[j] = ds; sp[j] = p; }  // j < N <= C1_MAX_TOKENS (the entry point's bound)
    T* row = dbase + (int64_t)j * ld_dqkv;
    if (j > 0) store8f<T>(row, zero);
    store8f<T>(row + 2 * D, dv);
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) {  // a group without keys: zeros
    gacc[g][c * 8 + u] = acc[u];
    gpk[g][c * 8 + u] = pk[u];
  }
  if (c == 0) { gr[g] = r; gden[g] = den; }
  __syncthreads();
  float R = 0.f, Den = 0.f;  // every thread, the groups in index order: the same bits everywhere
  for (int i = 0; i < C1_GROUPS; ++i) { R += gr[i]; Den += gden[i]; }
  const float corr = Den > 0.f ? R / Den : 0.f;
  if (threadIdx.x < 64) {
    float s = 0.f, t = 0.f;
    for (int i = 0; i < C1_GROUPS; ++i) { s += gacc[i][threadIdx.x]; t += gpk[i][threadIdx.x]; }
    dqkv[(int64_t)b * N * ld_dqkv + h * 64 + threadIdx.x] = (T)((s - corr * t) * scale);
  }
  for (int j = g; j < N; j += C1_GROUPS) {  // the keys this group stashed itself
    const float dss = (sds[j] - sp[j] * corr) * scale;
    float dk[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) dk[u] = dss * q[u];
    store8f<T>(dbase + (int64_t)j * ld_dqkv + D, dk);
  }
}
static int g_cls1_count = 0;
static int g_row1_count = 0;

// what both one-query entry points refuse before anything is queued: head_dim, N, row strides and addresses
// that the 16-B loads and stores cannot take
static bool cls1_args_ok(int dtype, int B, int H, int N, int head_dim, std::initializer_list<int64_t> lds,
                         std::initializer_list<const void*> ptrs) {
  if ((dtype != VIT_BF16 && dtype != VIT_F32) || head_dim != 64 || B <= 0 || H <= 0 || N <= 0 || N > C1_MAX_TOKENS)
    return false;
  const int64_t per16 = dtype == VIT_BF16 ? 8 : 4;  // elements in 16 bytes
  for (int64_t ld : lds)
    if (ld < 0 || ld % per16) return false;
  for (const void* p : ptrs)
    if (p == nullptr || ((uintptr_t)p & 15)) return false;
  return true;
}

// f(integral_constant<int, NT>) at NT = ceil(N / 16) = 1 .. 18, the resident kernels' tile counts
template <typename F>
static int by_tiles(int N, F&& f) {
  switch ((N + 15) / 16) {
#define CASE(n) case n: return f(std::integral_constant<int, n>{});
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13)
    CASE(14) CASE(15) CASE(16) CASE(17) CASE(18)
#undef CASE
  }
  return (int)hipErrorInvalidValue;
}
// f(T{}) with T = bf16 or float, after dtype
template <typename F>
static int by_dtype(int dtype, F&& f) {
  return dtype == VIT_BF16 ? f(bf16{}) : f(float{});
}
// a call counter, read and zeroed on request: the body of every vit_sdpa_*_count export
static int take_count(int& counter, int reset) {
  const int c = counter;
  if (reset) counter = 0;
  return c;
}

extern "C" {

// diagnostic only (tools/attn_stamps.py): phase stamps of the bf16 forward / fused backward
// kernels go to buf ([B*H][8] u64) until called again with null; not part of include/vit_hip.h
int vit_debug_attn_stamps(void* buf) {
  g_attn_stamps = (unsigned long long*)buf;
  return 0;
}

// Tuning hook: the bf16 backward form (-1 = from the environment, 1 = whole-head fused (the default),
// 2 = two kernels; they agree to bf16 rounding).  0 (round 4's banded form) is gone.
int vit_sdpa_bwd_variant(int v) {
  if (v == 0 || v > 2) return (int)hipErrorInvalidValue;
  g_bwd_variant = v < 0 ? -1 : v;
  return 0;
}

// Kernel choice past 288 tokens (bf16 or f32, non-causal, aligned): -1 = from the environment
// (VIT_ATTN_LONG=0|1, default 1), 0 = the generic kernels, 1 = the streamed MFMA kernels of the dtype
// (f32 also stays generic under VIT_ATTN_F32_GENERIC=1).  Returns the previous mode.
int vit_sdpa_long_config(int mode) {
  const int prev = g_long_mode;
  g_long_mode = mode < 0 ? -1 : (mode != 0);
  return prev;
}
// Host-side count of vit_sdpa_fwd / vit_sdpa_bwd calls that took the streamed bf16 kernels (one per call:
// the backward's two kernels count once); reset != 0 zeroes it after reading.
int vit_sdpa_long_count(int reset) { return take_count(g_long_count, reset); }
// The same count for the streamed f32 kernels.
int vit_sdpa_long_f32_count(int reset) { return take_count(g_long_f32_count, reset); }

// fp32 arithmetic of the resident f32 kernels (f32, N <= 288, aligned rows, causal or not): 0 = f32 MFMA,
// 1 = bf16x3, -1 keeps; other values are ignored.  Returns the previous setting.  "At most bf16x3": the generic and
// the one-query kernels and vit_sdpa_fwd_cls stay exact f32, and so do the streamed f32 kernels past 288 tokens
// unless vit_sdpa_f32_long_precision(1) is set as well.
int vit_sdpa_f32_precision(int mode) {
  const int prev = g_f32_split;
  if (mode == 0 || mode == 1) g_f32_split = mode;
  return prev;
}
// Host-side count of vit_sdpa_fwd / vit_sdpa_bwd calls that took the bf16x3 kernels; reset != 0 zeroes it.
int vit_sdpa_f32_split_count(int reset) { return take_count(g_f32_split_count, reset); }
// fp32 arithmetic of the streamed f32 kernels (f32, N > 288, aligned rows, not causal): 0 = f32 MFMA (exact, the
// default), 1 = bf16x3 while vit_sdpa_f32_precision is 1 as well, -1 keeps; other values are ignored.  Returns the
// previous setting.  The generic kernels past 288 tokens (causal, misaligned, vit_sdpa_long_config(0),
// VIT_ATTN_F32_GENERIC=1) stay exact f32.
int vit_sdpa_f32_long_precision(int mode) {
  const int prev = g_f32_long;
  if (mode == 0 || mode == 1) g_f32_long = mode;
  return prev;
}
// Host-side count of vit_sdpa_fwd / vit_sdpa_bwd calls that took the streamed bf16x3 kernels (they count in
// vit_sdpa_long_f32_count too, never in vit_sdpa_f32_split_count); reset != 0 zeroes it.
int vit_sdpa_long_f32_split_count(int reset) { return take_count(g_long_f32_split_count, reset); }

// F.scaled_dot_product_attention(q, k, v) (no dropout) for head_dim 64; causal = 1
// masks key > query (OpenAI CLIP text tower attn_mask, additive -inf above the diagonal).
// qkv: [B*N, ld_qkv] with q at column h*64, k at D + h*64, v at 2D + h*64.
// o: [B*N, ld_o] (column h*64); lse: [B*H*N] f32 (natural-log, scaled scores).
int vit_sdpa_fwd(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, void* o,
                 int64_t ld_o, float* lse, float scale, int causal, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (head_dim != 64 || N <= 0) return (int)hipErrorInvalidValue;
  const int D = H * 64;
  const bool aligned = (ld_qkv % (dtype == VIT_BF16 ? 8 : 4) == 0) && (ld_o % 4 == 0);
  const dim3 sgrid(B * H, (N + ST_QB - 1) / ST_QB);  // streamed kernels
  switch (attn_path(dtype, N, causal, aligned)) {
    case AP_STREAM_BF16:
      hipLaunchKernelGGL(attn_fwd_stream, sgrid, dim3(AT_THREADS), 0, s, (const bf16*)qkv, ld_qkv, D, H, N, scale,
                         (bf16*)o, ld_o, lse);
      VIT_CHECK_LAUNCH();
      ++g_long_count;
      return 0;
    case AP_STREAM_F32:
      if (stream_f32_split()) {
        stream_x3_attrs();
        hipLaunchKernelGGL(attn_fwd_stream_x3, sgrid, dim3(AT_THREADS), SX_LDS, s, (const float*)qkv, ld_qkv, D, H, N,
                           scale, (float*)o, ld_o, lse);
        VIT_CHECK_LAUNCH();
        ++g_long_f32_count;
        ++g_long_f32_split_count;
        return 0;
      }
      stream_f32_attrs();
      hipLaunchKernelGGL(attn_fwd_stream_f32, sgrid, dim3(AT_THREADS), SF_LDS, s, (const float*)qkv, ld_qkv, D, H, N,
                         scale, (float*)o, ld_o, lse);
      VIT_CHECK_LAUNCH();
      ++g_long_f32_count;
      return 0;
    case AP_RESIDENT_BF16:
      return by_tiles(N, [&](auto nt) {
        return fwd_mfma<nt()>(qkv, ld_qkv, D, B, H, N, scale, causal, o, ld_o, lse, s);
      });
    case AP_RESIDENT_F32:
      return by_tiles(N, [&](auto nt) {
        return g_f32_split ? fwd_f32<F32X3Res<nt()>>(qkv, ld_qkv, D, B, H, N, scale, causal, o, ld_o, lse, s)
                           : fwd_f32<F32Res<nt()>>(qkv, ld_qkv, D, B, H, N, scale, causal, o, ld_o, lse, s);
      });
    case AP_GENERIC:
      break;
  }
  if ((int64_t)B * H > 65535) return (int)hipErrorInvalidValue;  // the generic kernels put b*h on grid.y
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(attn_fwd_generic<T>, dim3((N + 63) / 64, B * H), dim3(256), 0, s, (const T*)qkv, ld_qkv, D, H, N,
                       scale, (T*)o, ld_o, lse, causal);
    VIT_CHECK_LAUNCH();
    return 0;
  });
}

// Whether vit_sdpa_fwd_image launches: where vit_sdpa_fwd with f32 tensors of this geometry takes the bf16x3
// kernels -- mode "high", head_dim 64, every row pitch a multiple of 4 floats, up to 288 tokens (causal or not) or,
// past them, not causal with the streamed kernels on and the long switch set -- and, one thing more than vit_sdpa_fwd
// looks at (it takes 16-byte aligned rows on trust), qkv_img and o_img 16-byte aligned.  lse is stored a float at a
// time and may sit anywhere.
static bool sdpa_image_ok(int B, int H, int N, int head_dim, int causal, int64_t strides_or, uint64_t ptrs_or) {
  if (head_dim != 64 || N <= 0 || B <= 0 || H <= 0 || !g_f32_split) return false;
  const bool aligned = strides_or % 4 == 0 && ptrs_or % 16 == 0;
  switch (attn_path(VIT_F32, N, causal, aligned)) {
    case AP_RESIDENT_F32: return true;
    case AP_STREAM_F32: return stream_f32_split();
    default: return false;
  }
}
// Host-only query (no GPU call): 1 when vit_sdpa_fwd_image would launch for this geometry, strides_or = ld_qkv | ld_o,
// ptrs_or = the OR of the addresses of qkv_img and o_img; else 0.
int vit_sdpa_fwd_takes_image(int B, int H, int N, int head_dim, int causal, int64_t strides_or, uint64_t ptrs_or) {
  return sdpa_image_ok(B, H, N, head_dim, causal, strides_or, ptrs_or) ? 1 : 0;
}
// vit_sdpa_fwd for f32 "high" with qkv and o as pre-split activation images (the f32 row
// pitches): the bf16x3 kernels' image forms, o the image of vit_sdpa_fwd's o and lse its lse, bit for bit.  Anything
// else is hipErrorInvalidValue with nothing launched and nothing written: an image is never read as floats.
int vit_sdpa_fwd_image(int B, int H, int N, int head_dim, const void* qkv_img, int64_t ld_qkv, void* o_img,
                       int64_t ld_o, float* lse, float scale, int causal, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!qkv_img || !o_img || !lse) return (int)hipErrorInvalidValue;
  if (!sdpa_image_ok(B, H, N, head_dim, causal, ld_qkv | ld_o, (uint64_t)qkv_img | (uint64_t)o_img))
    return (int)hipErrorInvalidValue;
  const int D = H * 64;
  if (N > AT_RESIDENT_MAX) {
    static bool attr = false;
    if (!attr) {
      raise_lds(attn_fwd_image_stream, SX_LDS);
      attr = true;
    }
    hipLaunchKernelGGL(attn_fwd_image_stream, dim3(B * H, (N + ST_QB - 1) / ST_QB), dim3(AT_THREADS), SX_LDS, s,
                       (const float*)qkv_img, ld_qkv, D, H, N, scale, (float*)o_img, ld_o, lse);
    VIT_CHECK_LAUNCH();
    ++g_long_f32_count;
    ++g_long_f32_split_count;
    ++g_f32_image_count;
    return 0;
  }
  return by_tiles(N, [&](auto nt) {
    return fwd_f32_image<nt()>(qkv_img, ld_qkv, D, B, H, N, scale, causal, o_img, ld_o, lse, s);
  });
}
// Host-side count of vit_sdpa_fwd_image calls that launched; reset != 0 zeroes it.
int vit_sdpa_f32_image_count(int reset) { return take_count(g_f32_image_count, reset); }

// Query-limited forward: only query 0 of every (b, h) will be read.  bf16, N <= 288, aligned rows: the
// resident kernel on query tile 0 (rows 0..15 of each image bit for bit vit_sdpa_fwd's; every other row
// o = 0, lse = +inf).  Anything else: vit_sdpa_fwd, unmasked (all rows).
int vit_sdpa_fwd_cls(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, void* o,
                     int64_t ld_o, float* lse, float scale, void* stream) {
  if (head_dim != 64 || N <= 0) return (int)hipErrorInvalidValue;
  if (N <= AT_RESIDENT_MAX && dtype == VIT_BF16 && (ld_qkv % 8 == 0) && (ld_o % 4 == 0) && lse && !g_attn_stamps) {
    ++g_cls_count;
    return by_tiles(N, [&](auto nt) {
      return fwd_mfma_cls<nt()>(qkv, ld_qkv, H * 64, B, H, N, scale, o, ld_o, lse, (hipStream_t)stream);
    });
  }
  return vit_sdpa_fwd(dtype, B, H, N, head_dim, qkv, ld_qkv, o, ld_o, lse, scale, 0, stream);
}
// Host-side count of vit_sdpa_fwd_cls calls that took the query-limited kernel (reset != 0 zeroes it).
int vit_sdpa_cls_count(int reset) { return take_count(g_cls_count, reset); }

// One-query forward (attn_cls1_fwd): query row 0 of every image, all N keys and values; bf16 or f32, any N up to
// 2048.  o_cls [B, D] with row b at b * ld_o (the dense o with ld_o = N * D is a valid argument), lse_cls [B * H]
// f32 (natural log).  head_dim != 64, N <= 0 or > 2048, a row stride or an address that is not a multiple of 16
// bytes: hipErrorInvalidValue, nothing queued.
int vit_sdpa_cls1_fwd(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, void* o_cls,
                      int64_t ld_o, float* lse_cls, float scale, void* stream) {
  if (!cls1_args_ok(dtype, B, H, N, head_dim, {ld_qkv, ld_o}, {qkv, o_cls}) || lse_cls == nullptr ||
      ld_qkv < 3 * (int64_t)H * 64)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int D = H * 64;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(attn_cls1_fwd<T>, dim3(B * H), dim3(C1_THREADS), 0, s, (const T*)qkv, ld_qkv, D, H, N, scale,
                       (T*)o_cls, ld_o, lse_cls);
    VIT_CHECK_LAUNCH();
    ++g_cls1_count;
    return 0;
  });
}

// One-query backward (attn_cls1_bwd) from the class rows' dO (do_cls [B, D], row b at b * ld_do), the forward's
// o_cls and lse_cls: writes every element of dqkv [B*N, 3D] (dq rows 1 .. N-1 exact zeros); delta is computed
// in the kernel, no workspace, no bias partials.  Refusals as vit_sdpa_cls1_fwd.
int vit_sdpa_cls1_bwd(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv,
                      const void* o_cls, int64_t ld_o, const void* do_cls, int64_t ld_do, const float* lse_cls,
                      void* dqkv, int64_t ld_dqkv, float scale, void* stream) {
  if (!cls1_args_ok(dtype, B, H, N, head_dim, {ld_qkv, ld_o, ld_do, ld_dqkv}, {qkv, o_cls, do_cls, dqkv}) ||
      lse_cls == nullptr || ld_qkv < 3 * (int64_t)H * 64 || ld_dqkv < 3 * (int64_t)H * 64)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int D = H * 64;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(attn_cls1_bwd<T>, dim3(B * H), dim3(C1_THREADS), 0, s, (const T*)qkv, ld_qkv, D, H, N, scale,
                       (const T*)o_cls, ld_o, (const T*)do_cls, ld_do, lse_cls, (T*)dqkv, ld_dqkv);
    VIT_CHECK_LAUNCH();
    ++g_cls1_count;
    return 0;
  });
}
// Host-side count of launches of either one-query kernel (reset != 0 zeroes it after reading).
int vit_sdpa_cls1_count(int reset) { return take_count(g_cls1_count, reset); }

// One-query forward at a row per sequence (attn_row1_fwd): query row qrow[b] (int64 on the device, clamped to
// [0, N - 1] in the kernel) against keys 0 .. qrow[b] (causal != 0) or all N keys; bf16 or f32, any N up to 2048.
// o_row [B, D] with row b at b * ld_o, lse_row [B * H] f32 (natural log).  qrow[b] = 0 without the mask is
// vit_sdpa_cls1_fwd bit for bit.  Refusals as vit_sdpa_cls1_fwd, a null qrow among them.
int vit_sdpa_row1_fwd(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv,
                      const int64_t* qrow, int causal, void* o_row, int64_t ld_o, float* lse_row, float scale,
                      void* stream) {
  if (!cls1_args_ok(dtype, B, H, N, head_dim, {ld_qkv, ld_o}, {qkv, o_row}) || lse_row == nullptr ||
      qrow == nullptr || ld_qkv < 3 * (int64_t)H * 64)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int D = H * 64;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(attn_row1_fwd<T>, dim3(B * H), dim3(C1_THREADS), 0, s, (const T*)qkv, ld_qkv, D, H, N, qrow,
                       causal != 0, scale, (T*)o_row, ld_o, lse_row);
    VIT_CHECK_LAUNCH();
    ++g_row1_count;
    return 0;
  });
}
// Host-side count of attn_row1_fwd launches (reset != 0 zeroes it after reading).
int vit_sdpa_row1_count(int reset) { return take_count(g_row1_count, reset); }

// fp8 (block-scaled OCP e4m3) forward, head_dim 64, N <= 320: see attn_fwd_fp8.  qkv / o bf16
// or f32 (dtype; quantised to e4m3 inside the kernel either way); lse f32 or null.
int vit_sdpa_fwd_fp8(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, void* o,
                     int64_t ld_o, float* lse, float scale, int causal, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (head_dim != 64 || N <= 0 || N > 320 || (ld_qkv % 8) || (ld_o % 4)) return (int)hipErrorInvalidValue;
  const int D = H * 64;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    switch ((N + 63) / 64) {
#define F8(n)                                                                                                       \
  case n:                                                                                                           \
    hipLaunchKernelGGL((attn_fwd_fp8<n, T>), dim3(B * H), dim3(F8_THREADS), 0, s, (const T*)qkv, ld_qkv, D, H, N, scale, \
                       (T*)o, ld_o, lse, causal);                                                                   \
    break;
      F8(1) F8(2) F8(3) F8(4) F8(5)
#undef F8
    }
    VIT_CHECK_LAUNCH();
    return 0;
  });
}

// The streamed form of vit_sdpa_fwd_fp8 (attn_fwd_fp8_stream): any N >= 1, the same refusals otherwise; up to
// 320 tokens the same bits.  Callers choose it (ops.sdpa_fwd's fp8_long past 320 tokens); nothing falls into it.
int vit_sdpa_fwd_fp8_stream(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, void* o,
                            int64_t ld_o, float* lse, float scale, int causal, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (head_dim != 64 || N <= 0 || (ld_qkv % 8) || (ld_o % 4)) return (int)hipErrorInvalidValue;
  if (dtype != VIT_BF16 && dtype != VIT_F32) return (int)hipErrorInvalidValue;
  const int D = H * 64;
  const dim3 grid(B * H, (N + F8S_QB - 1) / F8S_QB);
  if (grid.y > 65535) return (int)hipErrorInvalidValue;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(attn_fwd_fp8_stream<T>, grid, dim3(F8_THREADS), 0, s, (const T*)qkv, ld_qkv, D, H, N, scale,
                       (T*)o, ld_o, lse, causal);
    VIT_CHECK_LAUNCH();
    ++g_fp8_stream_count;
    return 0;
  });
}
// Host-side count of vit_sdpa_fwd_fp8_stream calls that launched (reset != 0 zeroes it after reading).
int vit_sdpa_fp8_stream_count(int reset) { return take_count(g_fp8_stream_count, reset); }

// The quantise-once pair (attn_fp8_quant_kv, attn_fwd_fp8_pre).  The workspace layout is private to this file:
// callers size it with vit_sdpa_fp8_kv_bytes.
static int64_t fp8_kv_bytes(int B, int H, int N) {
  return (int64_t)B * H * ((N + F8S_CH - 1) / F8S_CH) * F8S_BUF;
}
static bool fp8_pre_args_ok(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv,
                            const void* ws, int64_t ws_bytes) {
  if (head_dim != 64 || B < 1 || H < 1 || N < 1 || (ld_qkv % 8) || qkv == nullptr) return false;
  if (dtype != VIT_BF16 && dtype != VIT_F32) return false;
  if (ws == nullptr || ((uintptr_t)ws % 16) || ws_bytes < fp8_kv_bytes(B, H, N)) return false;
  return (N + F8S_CH - 1) / F8S_CH <= 65535;  // grid.y of the pre-pass; the consumer's is smaller
}
int vit_sdpa_fp8_kv_bytes(int B, int H, int N, int64_t* bytes) {
  if (B < 1 || H < 1 || N < 1 || bytes == nullptr) return (int)hipErrorInvalidValue;
  *bytes = fp8_kv_bytes(B, H, N);
  return 0;
}
// The pre-pass: K and V of qkv, quantised as vit_sdpa_fwd_fp8_stream quantises them, into ws (every byte of the
// first vit_sdpa_fp8_kv_bytes bytes is written).
int vit_sdpa_fp8_quant_kv(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, void* ws,
                          int64_t ws_bytes, void* stream) {
  if (!fp8_pre_args_ok(dtype, B, H, N, head_dim, qkv, ld_qkv, ws, ws_bytes)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int D = H * 64;
  const dim3 grid(B * H, (N + F8S_CH - 1) / F8S_CH);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(attn_fp8_quant_kv<T>, grid, dim3(F8_THREADS), 0, s, (const T*)qkv, ld_qkv, D, H, N,
                       (unsigned char*)ws);
    VIT_CHECK_LAUNCH();
    return 0;
  });
}
// The consumer: vit_sdpa_fwd_fp8_stream's o and lse, bit for bit, with K and V taken from ws alone (qkv is read
// for Q).  Same refusals, and ws as in vit_sdpa_fp8_quant_kv.
int vit_sdpa_fwd_fp8_pre(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, const void* ws,
                         int64_t ws_bytes, void* o, int64_t ld_o, float* lse, float scale, int causal, void* stream) {
  if (!fp8_pre_args_ok(dtype, B, H, N, head_dim, qkv, ld_qkv, ws, ws_bytes) || (ld_o % 4) || o == nullptr)
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(B * H, (N + F8S_QB - 1) / F8S_QB);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(attn_fwd_fp8_pre<T>, grid, dim3(F8_THREADS), 0, s, (const T*)qkv, ld_qkv, H, N,
                       (const unsigned char*)ws, scale, (T*)o, ld_o, lse, causal);
    VIT_CHECK_LAUNCH();
    ++g_fp8_pre_count;
    return 0;
  });
}
// Host-side count of vit_sdpa_fwd_fp8_pre calls that launched (reset != 0 zeroes it after reading).
int vit_sdpa_fp8_pre_count(int reset) { return take_count(g_fp8_pre_count, reset); }

// SDPA backward: writes dq/dk/dv into dqkv (same column layout as qkv).
// `delta_ws` (>= B*H*N floats) receives rowsum(dO*O) per (b, h, n).
// dbias (optional, [3D] f32) = column sums of dqkv (the qkv Linear's bias gradient);
// needs `partial` >= vit_sdpa_bwd_partial_floats(B, N, D) floats.
int vit_sdpa_bwd_partial_floats(int B, int N, int D) {
  const int64_t C = 3 * (int64_t)D;
  const int64_t mfma = B * C + (B > 64 ? (int64_t)((B + 63) / 64) * C : 0);
  const int64_t gen = 256 * C + 4 * C;  // vit_colsum on the generic path
  return (int)(mfma > gen ? mfma : gen);
}

int vit_sdpa_bwd(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, const void* o,
                 int64_t ld_o, const void* dout, int64_t ld_do, const float* lse, void* dqkv, int64_t ld_dqkv,
                 float* delta_ws, float scale, int causal, float* dbias, float* partial, int64_t partial_floats,
                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (head_dim != 64 || N <= 0) return (int)hipErrorInvalidValue;
  const int D = H * 64;
  if (!delta_ws) return (int)hipErrorInvalidValue;
  // dbias == null with a partial buffer: leave the per-image [B][3D] partials for the caller (bf16 path)
  const bool part_only = !dbias && partial;
  if ((dbias || part_only) && (partial == nullptr || partial_floats < vit_sdpa_bwd_partial_floats(B, N, D)))
    return (int)hipErrorInvalidValue;
  const bool aligned = (ld_qkv % (dtype == VIT_BF16 ? 8 : 4) == 0) && (ld_do % (dtype == VIT_BF16 ? 8 : 4) == 0) &&
                       (ld_dqkv % 4 == 0) && (ld_o % 4 == 0);
  const AttnPath path = attn_path(dtype, N, causal, aligned);
  // bf16 past 288 tokens, streamed or generic kernels alike: the bias partials come from a per-image
  // column-sum pass over dqkv, so partial-only mode works there; elsewhere it needs the resident bf16 kernels
  const bool long_bf16 = N > AT_RESIDENT_MAX && dtype == VIT_BF16;
  if (part_only && !long_bf16 && path != AP_RESIDENT_BF16) return (int)hipErrorInvalidValue;
  const dim3 sgrid(B * H, (N + ST_QB - 1) / ST_QB);  // streamed kernels
  int rc = (int)hipErrorInvalidValue;
  switch (path) {
    case AP_RESIDENT_BF16:
      rc = by_tiles(N, [&](auto nt) {
        return bwd_mfma<nt()>(qkv, ld_qkv, D, B, H, N, scale, causal, o, ld_o, dout, ld_do, lse, delta_ws, dqkv, ld_dqkv,
                              (dbias || part_only) ? partial : nullptr, s);
      });
      if (rc || !dbias) return rc;
      launch_colreduce(partial, B, 3 * D, dbias, 0, s, partial + (int64_t)B * 3 * D);
      VIT_CHECK_LAUNCH();
      return 0;
    case AP_RESIDENT_F32:
      rc = by_tiles(N, [&](auto nt) {
        return g_f32_split ? bwd_f32<F32X3Res<nt()>>(qkv, ld_qkv, D, B, H, N, scale, causal, o, ld_o, dout, ld_do, lse,
                                                     delta_ws, dqkv, ld_dqkv, s)
                           : bwd_f32<F32Res<nt()>>(qkv, ld_qkv, D, B, H, N, scale, causal, o, ld_o, dout, ld_do, lse,
                                                   delta_ws, dqkv, ld_dqkv, s);
      });
      break;
    case AP_STREAM_BF16:
      hipLaunchKernelGGL(attn_bwd_dq_stream, sgrid, dim3(AT_THREADS), 0, s, (const bf16*)qkv, ld_qkv, D, H, N, scale,
                         (const bf16*)o, ld_o, (const bf16*)dout, ld_do, lse, delta_ws, (bf16*)dqkv, ld_dqkv);
      VIT_CHECK_LAUNCH();
      hipLaunchKernelGGL(attn_bwd_dkv_stream, sgrid, dim3(AT_THREADS), 0, s, (const bf16*)qkv, ld_qkv, D, H, N, scale,
                         (const bf16*)dout, ld_do, lse, (const float*)delta_ws, (bf16*)dqkv, ld_dqkv);
      VIT_CHECK_LAUNCH();
      ++g_long_count;
      rc = 0;
      break;
    case AP_STREAM_F32:
      if (stream_f32_split()) {
        stream_x3_attrs();
        hipLaunchKernelGGL(attn_bwd_dq_stream_x3, sgrid, dim3(AT_THREADS), SX_LDS, s, (const float*)qkv, ld_qkv, D, H, N,
                           scale, (const float*)o, ld_o, (const float*)dout, ld_do, lse, delta_ws, (float*)dqkv, ld_dqkv);
        VIT_CHECK_LAUNCH();
        hipLaunchKernelGGL(attn_bwd_dkv_stream_x3, sgrid, dim3(AT_THREADS), SX_LDS_DKV, s, (const float*)qkv, ld_qkv, D,
                           H, N, scale, (const float*)dout, ld_do, lse, (const float*)delta_ws, (float*)dqkv, ld_dqkv);
        VIT_CHECK_LAUNCH();
        ++g_long_f32_count;
        ++g_long_f32_split_count;
        rc = 0;
        break;
      }
      stream_f32_attrs();
      hipLaunchKernelGGL(attn_bwd_dq_stream_f32, sgrid, dim3(AT_THREADS), SF_LDS, s, (const float*)qkv, ld_qkv, D, H, N,
                         scale, (const float*)o, ld_o, (const float*)dout, ld_do, lse, delta_ws, (float*)dqkv, ld_dqkv);
      VIT_CHECK_LAUNCH();
      hipLaunchKernelGGL(attn_bwd_dkv_stream_f32, sgrid, dim3(AT_THREADS), SF_LDS_DKV, s, (const float*)qkv, ld_qkv, D,
                         H, N, scale, (const float*)dout, ld_do, lse, (const float*)delta_ws, (float*)dqkv, ld_dqkv);
      VIT_CHECK_LAUNCH();
      ++g_long_f32_count;
      rc = 0;
      break;
    case AP_GENERIC:
      rc = by_dtype(dtype, [&](auto t) {
        return bwd_generic<decltype(t)>(qkv, ld_qkv, D, B, H, N, scale, causal, o, ld_o, dout, ld_do, lse, delta_ws, dqkv,
                                        ld_dqkv, s);
      });
      break;
  }
  if (rc) return rc;
  if (!long_bf16)
    return dbias ? vit_colsum(dtype, B * N, 3 * D, dqkv, ld_dqkv, dbias, partial, partial_floats, 0, stream) : 0;
  if (!dbias && !part_only) return 0;
  hipLaunchKernelGGL(attn_bias_image, dim3(B, (3 * D + 255) / 256), dim3(256), 0, s, (const bf16*)dqkv, ld_dqkv, N,
                     3 * D, partial);
  VIT_CHECK_LAUNCH();
  if (dbias) {
    launch_colreduce(partial, B, 3 * D, dbias, 0, s, partial + (int64_t)B * 3 * D);
    VIT_CHECK_LAUNCH();
  }
  return 0;
}

}  // extern "C"
