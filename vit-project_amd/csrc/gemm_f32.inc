// Included by gemm.hip (after namespace big).  fp32 MFMA GEMM: the parity / reference-precision
// path (compute_dtype=float32, CLIP-HBA as the reference runs it: clip_model.float(), NEWP:274).
//
//   v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulate; 64 FLOP/clk/SIMD = 157 TF/s chip
//   peak, MI355X_MICROARCH.md) on 128x128x32 tiles, 4 waves (2x2, 64x64 each), a 2-deep LDS ring
//   filled by global_load_lds (16 B/lane), 64 KiB -> 2 workgroups per CU.
//
// As in the bf16 kernels the MFMA computes C^T (Q is the A operand) so a lane owns C[i][j..j+3]
// (i = lane&15, j = 4*(lane>>4)) and the epilogue stores 16 B per lane (epi_vec, V = 4).  The reduction
// order inside a 16-deep k block is permuted identically for both operands: lane group
// g = lane>>4 feeds k = 16h + 4g + t to MFMA t (t = 0..3), so an r-contiguous (RC) operand row
// gives a lane its four k values with one ds_read_b128; an r-strided (CR) operand takes four
// ds_read_b32.
//
// LDS images (both conflict-free for those reads):
//   RC [rows][32 f32]: 128-B rows, 16-B chunk c of row r at r*128 + ((c ^ (r & 7)) << 4)
//   CR [32 k][cols f32]: 512-B k-rows, chunk c of k-row r at r*512 + ((c ^ (((r >> 2) & 3) << 2)) << 4)
// global_load_lds writes lane L's 16 B at piece + 16 L, so each lane loads the global chunk that
// belongs in its slot (the swizzle is an involution).
//
// SPLIT = 1 ("high", vit_gemm_f32_precision(1), DESIGN 4.22): the same staging, LDS images, fragment
// reads, ring, epilogue and stream-K code, but the products run as bf16x3.  Per k-step a wave reads the
// fragments of both 16-deep halves, splits every f32 value x in registers into
//   hi = bf16_rne(x),  lo = bf16_rne(x - float(hi))     (the subtraction is exact in f32)
// with v_cvt_pk_bf16_f32, packs the value of k = 16h + 4g + t as element j = 4h + t of a bf16x8 operand
// (the same rule for P and Q, so their reduction slots line up) and issues, per fragment pair,
//   acc += P_hi Q_lo;  acc += P_lo Q_hi;  acc += P_hi Q_hi       (v_mfma_f32_16x16x32_bf16, this order)
// P_lo Q_lo is dropped: tested to |C - C64| <= (3 * 2^-18 + (R + 3) * 2^-24) |P| |Q|^T on random normal-range
// data (DESIGN 4.22 for what a worst case adds), and the exact sum when both operands are bf16 values (lo = 0).  The C/D lane map of 16x16x32_bf16 is that
// of 16x16x4_f32, so the epilogue and the stream-K fragment images are unchanged.  48 MFMA-pipe cycles x
// 16 fragment pairs per k-step against 256 x 16; the split is 3 VALU per value (half a cvt, an unpack, a
// subtract, half a cvt), 64 values per lane per k-step.  The subtracts are single v_sub_f32 on purpose:
// packed f32 VALU beside MFMAs is an anti-lever (MI355X_MICROARCH.md, "price of one filler").
// Non-finite in, non-finite out: x = +-inf gives hi = +-inf, lo = NaN, and a finite |x| that rounds past the
// bf16 range gives hi = +-inf, lo = -+inf; either way the element is NaN where the f32 form gives +-inf.
// The setting is "at most bf16x3": GEMMs that do not take this path run the generic scalar-FMA kernel
// and are exact f32 in either mode.
//
// SPLIT = 2 (namespace f32w below, DESIGN 4.25): SPLIT = 1 with Q read from a pre-split image of a weight,
// built once per weight version by f32w::weight_image_kernel.  A row's 128-byte k-block holds four hi chunks,
// then four lo chunks; hi chunk g holds the bf16 hi of k = 16 (j >> 2) + 4 g + (j & 3) as element j = 0..7 --
// what split8 packs from the two fragment reads (h = 0, 1) of lane group g -- and lo chunk g the lo values in
// the same order.  The image has the f32 matrix's row pitch and size, stage<LAY_RC> copies it unchanged, and
// the reads frag<LAY_RC>(.., h = 0) / (.., h = 1) (chunks g and 4 + g) ARE Q's hi / lo packs: no VALU work
// for Q, P split as in SPLIT = 1, the same three MFMAs on the same operand bits in the same order, so the
// result is SPLIT = 1's bit for bit.
//
// SPLIT = 3 (namespace f32a below, DESIGN 4.26): SPLIT = 2 with P read from the same kind of image, written by the
// kernel that produced the activation (a LayerNorm forward, or the image epilogue below of the GEMM in front).  The
// image rule is Q's: P is row-contiguous too, staged by the same stage<LAY_RC> and read by the same frag<LAY_RC>.
// No split8 is left in the k-step: 16 ds_read_b128 and 48 MFMAs on the operand bits of SPLIT = 1, in its order.
namespace f32m {

constexpr int BM = 128, BN = 128, BK = 32, THREADS = 256, WAVES = 4, S = 2;
constexpr int PIMG = BM * BK * 4, QIMG = BN * BK * 4, STAGE = PIMG + QIMG, LDS = S * STAGE;
constexpr int GP = PIMG / 1024 / WAVES, GQ = QIMG / 1024 / WAVES, G = GP + GQ;
constexpr int AI = 4, AJ = 4;  // 16x16 fragments per wave (64 x 64)
static_assert(LDS <= 163840 / 2, "two workgroups per CU");

__device__ __forceinline__ int cr_sw(int r) { return ((r >> 2) & 3) << 2; }

// stage a ROWS x BK (RC) or BK x ROWS (CR) f32 tile; rows / columns past `lim` are clamped
template <int LAY, int ROWS, int GOP>
__device__ __forceinline__ void stage(char* img, const float* __restrict__ base, int64_t ld, int row0, int r0, int lim,
                                      int wave, int lane) {
#pragma unroll
  for (int u = 0; u < GOP; ++u) {
    const int t = wave * GOP + u;  // 1-KiB piece
    const float* src;
    if constexpr (LAY == LAY_RC) {  // piece = 8 rows x 8 chunks
      const int row = t * 8 + lane / 8, slot = lane % 8;
      const int c = slot ^ (row & 7);
      src = base + (int64_t)min(row0 + row, lim - 1) * ld + r0 + c * 4;
    } else {  // piece = 2 k-rows x 32 chunks
      const int r = t * 2 + lane / 32, slot = lane % 32;
      const int c = slot ^ cr_sw(r);
      src = base + (int64_t)(r0 + r) * ld + min(row0 + c * 4, lim - 4);
    }
    __builtin_amdgcn_global_load_lds((const void*)src, LDS_PTR(img + t * 1024), 16, 0, 0);
  }
}

typedef float f32x4_ __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 asm_read_f128(uint32_t a) {
  f32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(a));
  return v;
}
__device__ __forceinline__ float asm_read_f32(uint32_t a) {
  float v;
  asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(a));
  return v;
}

// the four k values (t = 0..3) lane `lane` feeds for fragment s (rows s*16..s*16+15) in k half h
template <int LAY, int ROWS>
__device__ __forceinline__ f32x4 frag(uint32_t img, int s, int h, int lane) {
  const int g = lane >> 4, i = s * 16 + (lane & 15);
  if constexpr (LAY == LAY_RC) {
    const int c = h * 4 + g;
    return asm_read_f128(img + i * 128 + ((c ^ (i & 7)) << 4));
  } else {
    f32x4 v;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int r = 16 * h + 4 * g + t;
      v[t] = asm_read_f32(img + r * (ROWS * 4) + (((i >> 2) ^ cr_sw(r)) << 4) + (i & 3) * 4);
    }
    return v;
  }
}

// SPLIT = 1: split8 (bf16_split.hpp) turns the 8 values of a lane's fragment (x0: k half 0, x1: k half 1) into
// hi / lo bf16x8 operands, element j = 4h + t

// acc += P(i0.., rb + kb*BK ..) Q(j0.., ...)^T over k-steps [kb, ke) of one tile (the LDS ring restarts
// per call; a __syncthreads before the first issue protects a previous call's reads)
template <int PL, int QL, int SPLIT>
__device__ __forceinline__ void mainloop(const float* __restrict__ P, int64_t ldp, const float* __restrict__ Q,
                                         int64_t ldq, int M, int N, int i0, int j0, int rb, int kb, int ke,
                                         f32x4 (&acc)[AI][AJ], char* smem, int wave, int lane) {
  const int wi = wave >> 1, wj = wave & 1;
  auto issue = [&](int k, int part) {  // part 1: P pieces, 2: Q pieces, 3: both
    char* buf = smem + (k % S) * STAGE;
    if (part & 1) stage<PL, BM, GP>(buf, P, ldp, i0, rb + k * BK, M, wave, lane);
    if (part & 2) stage<QL, BN, GQ>(buf + PIMG, Q, ldq, j0, rb + k * BK, N, wave, lane);
  };
  if (ke <= kb) return;
  issue(kb, 3);
  for (int kt = kb; kt < ke; ++kt) {
    big::wait_vm<0>();
    big::lds_barrier();
    const bool more = kt + 1 < ke;
    const uint32_t cur = big::lds_addr(smem + (kt % S) * STAGE);
    if constexpr (SPLIT == 2 || SPLIT == 3) {
      static_assert(QL == LAY_RC && (SPLIT == 2 || PL == LAY_RC), "the pre-split image is row-contiguous");
      // Q is a pre-split image: its h = 0 / h = 1 reads are the hi / lo packs.  Issue and read order as below.
      // SPLIT = 3: P is one too (an activation image), so the k-step has no split8 at all.
      f32x4 pf[2][AI], qf[2][AJ];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (more) issue(kt + 1, h + 1);
#pragma unroll
        for (int b = 0; b < AJ; ++b) qf[h][b] = frag<QL, BN>(cur + PIMG, wj * AJ + b, h, lane);
#pragma unroll
        for (int a = 0; a < AI; ++a) pf[h][a] = frag<PL, BM>(cur, wi * AI + a, h, lane);
      }
      big::lgkm_wait0();
#pragma unroll
      for (int a = 0; a < AI; ++a) {
        bf16x8 ph, pl;
        if constexpr (SPLIT == 3) {
          ph = __builtin_bit_cast(bf16x8, pf[0][a]);
          pl = __builtin_bit_cast(bf16x8, pf[1][a]);
        } else {
          split8(pf[0][a], pf[1][a], ph, pl);
        }
#pragma unroll
        for (int b = 0; b < AJ; ++b) {
          const bf16x8 qh = __builtin_bit_cast(bf16x8, qf[0][b]), ql = __builtin_bit_cast(bf16x8, qf[1][b]);
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ql, ph, acc[a][b], 0, 0, 0);  // P_hi Q_lo
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qh, pl, acc[a][b], 0, 0, 0);  // P_lo Q_hi
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qh, ph, acc[a][b], 0, 0, 0);  // P_hi Q_hi
        }
      }
    } else if constexpr (SPLIT) {
      // both halves' fragments before any MFMA; the next stage's P pieces before the first half's reads,
      // its Q pieces before the second's (the same split issue)
      f32x4 pf[2][AI], qf[2][AJ];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (more) issue(kt + 1, h + 1);
#pragma unroll
        for (int b = 0; b < AJ; ++b) qf[h][b] = frag<QL, BN>(cur + PIMG, wj * AJ + b, h, lane);
#pragma unroll
        for (int a = 0; a < AI; ++a) pf[h][a] = frag<PL, BM>(cur, wi * AI + a, h, lane);
      }
      big::lgkm_wait0();
      bf16x8 qh[AJ], ql[AJ];
#pragma unroll
      for (int b = 0; b < AJ; ++b) split8(qf[0][b], qf[1][b], qh[b], ql[b]);
#pragma unroll
      for (int a = 0; a < AI; ++a) {  // one P fragment's packs at a time (8 VGPRs live, not 32)
        bf16x8 ph, pl;
        split8(pf[0][a], pf[1][a], ph, pl);
#pragma unroll
        for (int b = 0; b < AJ; ++b) {
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ql[b], ph, acc[a][b], 0, 0, 0);  // P_hi Q_lo
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qh[b], pl, acc[a][b], 0, 0, 0);  // P_lo Q_hi
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qh[b], ph, acc[a][b], 0, 0, 0);  // P_hi Q_hi
        }
      }
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // the next stage's P pieces before the first half's fragment reads, its Q pieces before the
        // second's (as gemm_tile's split issue: not one burst behind the barrier)
        if (more) issue(kt + 1, h + 1);
        f32x4 pf[AI], qf[AJ];
#pragma unroll
        for (int b = 0; b < AJ; ++b) qf[b] = frag<QL, BN>(cur + PIMG, wj * AJ + b, h, lane);
#pragma unroll
        for (int a = 0; a < AI; ++a) pf[a] = frag<PL, BM>(cur, wi * AI + a, h, lane);
        big::lgkm_wait0();
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
          for (int a = 0; a < AI; ++a)
#pragma unroll
            for (int b = 0; b < AJ; ++b)
              acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[b][tt], pf[a][tt], acc[a][b], 0, 0, 0);
      }
    }
    // every wave's reads of this slot retire (lgkm_wait0) before the next barrier, so the
    // slot can be refilled after it (WAR)
  }
}

template <int EPI, typename TO, typename TA>
__device__ __forceinline__ void epilogue(const Epi& e, const f32x4 (&acc)[AI][AJ], int M, int N, int i0, int j0,
                                         int z, int wave, int lane) {
  const int wi = wave >> 1, wj = wave & 1;
  VIT_EPI_FRAG(AI, AJ, i0 + wi * 64, j0 + wj * 64, )
}

#include "gemm_f32_kernels.inc"

}  // namespace f32m

// The kernels that read a pre-split weight image as Q (instantiated with PL = QL = LAY_RC, SPLIT = 2 only), and the
// pass that writes one.  A namespace of their own: the f32m kernels are the SPLIT = 0 / 1 pairs and nothing else.
namespace f32w {

using namespace f32m;

#include "gemm_f32_kernels.inc"

// img (rows x red cells of 4 bytes, contiguous) = the pre-split image of A, where A = W [rows][red] (row stride
// ldw) or, TRANSPOSE, A = W^T of W [red][rows].  red % 32 == 0.  One lane per (row, 32-deep k-block, lane group
// g): the two f32x4 the GEMM's lane group g would read (k = 4g.. and 16 + 4g..) through split8 into hi chunk g
// and lo chunk g.  Memory-bound, run once per weight version.
__global__ __launch_bounds__(256) void weight_image_kernel(const float* __restrict__ W, int64_t ldw, int rows,
                                                           int red, char* __restrict__ img) {
  const int kbs = red / 32;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int g = (int)(id & 3);
  const int64_t blk = id >> 2;
  if (blk >= (int64_t)rows * kbs) return;
  const int row = (int)(blk / kbs), kb = (int)(blk - (int64_t)row * kbs);
  const float* src = W + (int64_t)row * ldw + kb * 32 + 4 * g;
  const f32x4 x0 = *reinterpret_cast<const f32x4*>(src), x1 = *reinterpret_cast<const f32x4*>(src + 16);
  bf16x8 hi, lo;
  split8(x0, x1, hi, lo);
  char* dst = img + ((int64_t)row * red + kb * 32) * 4 + 16 * g;
  *reinterpret_cast<bf16x8*>(dst) = hi;
  *reinterpret_cast<bf16x8*>(dst + 64) = lo;
}

// the transposed form through an LDS tile of 64 reduction rows (n) x 32 image rows (k): 128-byte row pieces
// in, 256-byte image-row pieces out
__global__ __launch_bounds__(256) void weight_image_t_kernel(const float* __restrict__ W, int64_t ldw, int red,
                                                             int rows, char* __restrict__ img) {
  __shared__ float tile[64][33];
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * 64, k0 = blockIdx.y * 32;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int n = (tid >> 5) + 8 * u, k = tid & 31;
    tile[n][k] = (n0 + n < red && k0 + k < rows) ? W[(int64_t)(n0 + n) * ldw + k0 + k] : 0.f;
  }
  __syncthreads();
  const int k = tid >> 3, nb = (tid >> 2) & 1, g = tid & 3;
  if (k0 + k >= rows || n0 + nb * 32 >= red) return;  // red % 32 == 0: a k-block is whole or absent
  f32x4 x0, x1;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    x0[t] = tile[nb * 32 + 4 * g + t][k];
    x1[t] = tile[nb * 32 + 16 + 4 * g + t][k];
  }
  bf16x8 hi, lo;
  split8(x0, x1, hi, lo);
  char* dst = img + ((int64_t)(k0 + k) * red + n0 + nb * 32) * 4 + 16 * g;
  *reinterpret_cast<bf16x8*>(dst) = hi;
  *reinterpret_cast<bf16x8*>(dst + 64) = lo;
}

}  // namespace f32w

// The kernels that read or write an activation image (DESIGN 4.26), a namespace of their own again: SPLIT = 3 reads
// P and Q as images; TO = img_t writes C as the image of the f32 matrix the plain epilogue would have stored, for
// the GEMM behind it to read as its P (SPLIT = 2 or 3 in front of it).
namespace f32a {

using namespace f32m;

struct img_t { float cell; };  // output type tag: 4-byte cells at the f32 matrix's row pitch

// The image-writing epilogue (EPI_STORE and the two act-only codes; N % 32 == 0).  A lane holds both inputs of the
// split8 of lane group g = lane >> 4 in the 32-column k-block m of its wave: acc[a][2m] is columns 32m + 4g .. + 3
// (the h = 0 half), acc[a][2m + 1] columns 32m + 16 + 4g .. + 3 (h = 1).  Bias, activation and rounding are
// epi_vec's for an f32 output; then hi chunk g and lo chunk g of that row's k-block, 16 bytes each.
template <int EPI>
__device__ __forceinline__ void epilogue_image(const Epi& e, const f32x4 (&acc)[AI][AJ], int M, int N, int i0, int j0,
                                               int wave, int lane) {
  static_assert(EPI == EPI_STORE || epi_act_only(EPI), "image outputs: the plain store and the act-only forms");
  static_assert(AJ % 2 == 0, "fragment pairs");
  const int wi = wave >> 1, wj = wave & 1, g = lane >> 4;
#pragma unroll
  for (int a = 0; a < AI; ++a) {
    const int i = i0 + wi * 64 + a * 16 + (lane & 15);
#pragma unroll
    for (int m = 0; m < AJ / 2; ++m) {
      const int jb = j0 + wj * 64 + 32 * m;  // first column of the k-block
      if (i < M && jb < N) {
        f32x4 x[2] = {acc[a][2 * m], acc[a][2 * m + 1]};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (e.bias) x[h] += *reinterpret_cast<const f32x4*>(e.bias + jb + 16 * h + 4 * g);
          if constexpr (epi_act_only(EPI)) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              float ga, gd;
              epi_act_pair<EPI>(x[h][t], ga, gd);
              x[h][t] = ga;
            }
          }
        }
        bf16x8 hi, lo;
        split8(x[0], x[1], hi, lo);
        char* dst = (char*)e.C + ((int64_t)i * e.ldc + jb) * 4 + 16 * g;
        *reinterpret_cast<bf16x8*>(dst) = hi;
        *reinterpret_cast<bf16x8*>(dst + 64) = lo;
      }
    }
  }
}

// what the kernels below call: the image epilogue for TO = img_t, f32m's own for every other output
template <int EPI, typename TO, typename TA>
__device__ __forceinline__ void epilogue(const Epi& e, const f32x4 (&acc)[AI][AJ], int M, int N, int i0, int j0,
                                         int z, int wave, int lane) {
  if constexpr (std::is_same<TO, img_t>::value) epilogue_image<EPI>(e, acc, M, N, i0, j0, wave, lane);
  else f32m::epilogue<EPI, TO, TA>(e, acc, M, N, i0, j0, z, wave, lane);
}

#include "gemm_f32_kernels.inc"

}  // namespace f32a
