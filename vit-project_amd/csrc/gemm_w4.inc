// ----------------------------------------------------------------------------
// Wide-wave bf16 GEMM tile (round 5): 256x256 output tile on FOUR waves, one per SIMD, each wave owning a
// 128x128 block -- 64 16x16 accumulators = 256 fp32 registers per lane, pinned to AGPRs by inline-asm MFMAs
// (the one-wave-per-SIMD budget is 512 registers).  Per 32-deep k-step a wave reads 16 fragments for 64
// MFMAs (the 8-wave 128x64 tiles of V5 / the ping-pong kernel read 12 for 32: on the transposed CR images
// of the weight gradient that loop was bound by LDS instruction issue, DESIGN.md §4.9), and the next
// k-step's fragment reads are interleaved with this k-step's MFMAs (register double buffer), so no LDS
// read sits between a barrier and the MFMAs.  Operands stream through an S-deep ring of 32-KiB stages (P
// image 16 KiB, Q image 16 KiB; RC rows with the BK = 32 swizzle or half-blocked CR images, gemm_lds.hpp)
// filled by global_load_lds, S - 1 stages ahead, one s_barrier per k-step.
//
// Inline asm (MFMA, fragment reads) is invisible to the compiler's hazard recognizer and waitcnt pass:
//  - the fragment reads write "=v" outputs the compiler believes are ready at once; every destination is
//    named "+v" by the statements right after the k-step's s_waitcnt lgkmcnt(0), so the compiler's
//    own uses of them come after the data lands (a lab build without this copied fragments early: wrong
//    rows, profiles/r05/w4_lab_diag.jsonl); tools/w4_audit.sh checks the loop for copies between a read and
//    that wait (a CR fragment's two 8-B halves must be allocated adjacent, no concatenation move);
//  - accumulators are zeroed by the compiler (v_accvgpr_write), named "+a" by empty statements, then an
//    s_nop 4 precedes the first MFMA; each accumulator is re-used 64 MFMAs later; 24 wait states separate
//    the last MFMA from the epilogue's accumulator reads.
// ----------------------------------------------------------------------------
namespace w4 {

constexpr int BK = 32, PIMG = 256 * BK * 2, STAGE = 2 * PIMG;

__device__ __forceinline__ void mfma_acc(f32x4& c, const bf16x8& a, const bf16x8& b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}

template <int S_, int LD_> struct Cfg {
  static constexpr int S = S_, LD = LD_, LDS = S * STAGE, THREADS = 256;
  static_assert(LDS <= 163840, "LDS");
};

// unit w of the (split, tile) space; PL / QL: operand layouts (weight gradient: CR x CR)
template <class C, int PL, int QL, int EPI, typename TO, typename TA>
__device__ __forceinline__ void tile(const bf16* __restrict__ P, int64_t ldp, const bf16* __restrict__ Q,
                                     int64_t ldq, int M, int N, int R, int r_chunk, const Epi& e, int w,
                                     char* smem) {
  constexpr int S = C::S, LD = C::LD;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave >> 1, wj = wave & 1;
  const int tiles_j = (N + 255) / 256, tiles_i = (M + 255) / 256;
  const int tiles = tiles_i * tiles_j;
  const int z = w / tiles, t0 = w - z * tiles;
  // walk along the longer tile dimension (an XCD's consecutive units cover all short-side blocks)
  int ti, tj;
  if (tiles_j > tiles_i) {
    tj = t0 / tiles_i;
    ti = t0 - tj * tiles_i;
  } else {
    ti = t0 / tiles_j;
    tj = t0 - ti * tiles_j;
  }
  const int i0 = ti * 256, j0 = tj * 256;
  const int rb = z * r_chunk;
  const int re = min(R, rb + r_chunk);
  const int nk = (re - rb) / BK;

  f32x4 acc[8][8];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // staging: 16 1-KiB pieces per operand image, 4 per wave; per-lane source pointers advanced per stage
  const bf16* srcP[4];
  const bf16* srcQ[4];
  int64_t stepP, stepQ;
  {
    auto init = [&](auto lay_tag, const bf16* base, int64_t ld, int row0, int lim, const bf16* (&src)[4],
                    int64_t& step) {
      constexpr int LAY = decltype(lay_tag)::value;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = wave * 4 + u;
        if constexpr (LAY == LAY_RC) {
          const int row = t * 16 + lane / 4;
          const int c = (lane % 4) ^ big::rc_sw<32>(row);
          src[u] = base + (int64_t)min(row0 + row, lim - 1) * ld + rb + c * 8;
          step = BK;
        } else {
          src[u] = base + (int64_t)rb * ld + big::crh_src<256>(t, lane, ld, row0, lim);
          step = BK * ld;
        }
      }
    };
    init(std::integral_constant<int, PL>{}, P, ldp, i0, M, srcP, stepP);
    init(std::integral_constant<int, QL>{}, Q, ldq, j0, N, srcQ, stepQ);
  }
  // piece u (0..7) of stage k: 0-3 of P, 4-7 of Q
  auto piece = [&](int k, int u) {
    char* buf = smem + (k % S) * STAGE;
    if (u < 4) {
      __builtin_amdgcn_global_load_lds((const void*)srcP[u], LDS_PTR(buf + (wave * 4 + u) * 1024), 16, 0, 0);
      srcP[u] += stepP;
    } else {
      __builtin_amdgcn_global_load_lds((const void*)srcQ[u - 4], LDS_PTR(buf + PIMG + (wave * 4 + u - 4) * 1024), 16, 0,
                                       0);
      srcQ[u - 4] += stepQ;
    }
  };
  const bool noload = e.dbg & 1;

  // fragment read bases (lane part + the wave's first fragment)
  uint32_t crh_p[2][2], crh_q[2][2];
#pragma unroll
  for (int lh = 0; lh < 2; ++lh)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      crh_p[lh][h] = big::crh_lane<256>(lane, lh, h) + (uint32_t)(wi * 4 * 1024);
      crh_q[lh][h] = PIMG + big::crh_lane<256>(lane, lh, h) + (uint32_t)(wj * 4 * 1024);
    }
  const uint32_t rc_p = (uint32_t)(wi * 128 * 64 + big::rc_off<32>(lane & 15, lane >> 4));
  const uint32_t rc_q = (uint32_t)(PIMG + wj * 128 * 64 + big::rc_off<32>(lane & 15, lane >> 4));
  // fragment f (0..15): 0-7 Q (columns), 8-15 P (rows); a CR fragment is two 8-B transposed reads
  auto read_frag = [&](auto fI, uint32_t cur, bf16x8 (&pf)[8], bf16x8 (&qf)[8]) {
    constexpr int f = decltype(fI)::value;
    if constexpr (f < 8) {
      if constexpr (QL == LAY_RC) qf[f] = big::asm_read128_off<f * 16 * 64>(cur + rc_q);
      else qf[f] = big::frag_crh<256, 0, f>(crh_q, cur);
    } else {
      constexpr int a = f - 8;
      if constexpr (PL == LAY_RC) pf[a] = big::asm_read128_off<a * 16 * 64>(cur + rc_p);
      else pf[a] = big::frag_crh<256, 0, a>(crh_p, cur);
    }
  };
  // after a k-step's reads: wait for them, then name every destination "+v" (audit: no compiler copy of a
  // destination between its read and this wait -- tools/w4_audit.sh), then 2 wait states before any MFMA
  auto settle = [&](bf16x8 (&pf)[8], bf16x8 (&qf)[8]) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int a = 0; a < 8; ++a) asm volatile("" : "+v"(pf[a]), "+v"(qf[a]));
    asm volatile("s_nop 1" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  // one k-step: 64 MFMAs on (pc, qc) with the next k-step's 16 fragment reads (from `nxt`) after MFMAs
  // 3f+1 -- unconditionally: past the last k-step they read a stale ring slot nothing uses, so the loop
  // body has no data-dependent register definitions -- and the pieces of stage t + S per LD (0: all after
  // the barrier, 1: one after every 8 MFMAs, 2: one after every 4 of the first 32)
  auto kstep = [&](int t, uint32_t nxt, const bf16x8 (&pc)[8], const bf16x8 (&qc)[8], bf16x8 (&pn)[8], bf16x8 (&qn)[8]) {
    const bool more = t + S < nk && !noload;
    if constexpr (LD == 0) {
      if (more) {
#pragma unroll
        for (int u = 0; u < 8; ++u) piece(t + S, u);
      }
    }
    big::Unroll<64>::run([&](auto mI) {
      constexpr int m = decltype(mI)::value;
      constexpr int a = m / 8, b = m % 8;
      mfma_acc(acc[a][b], qc[b], pc[a]);
      if constexpr (m % 3 == 1 && m / 3 < 16) read_frag(std::integral_constant<int, m / 3>{}, nxt, pn, qn);
      if constexpr (LD == 1 && m % 8 == 4) {
        if (more) piece(t + S, m / 8);
      }
      if constexpr (LD == 2 && m % 4 == 2 && m < 32) {
        if (more) piece(t + S, m / 4);
      }
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  // prologue: stages 0..S-1 in flight; stage 0 landed (S-1 stages of 8 pieces may stay in flight)
  if (!noload) {
#pragma unroll
    for (int k = 0; k < S; ++k)
      if (k < nk)
#pragma unroll
        for (int u = 0; u < 8; ++u) piece(k, u);
    big::wait_stages<8, S>(min(S - 1, nk - 1));
  }
  big::lds_barrier();
  bf16x8 pA[8], qA[8], pB[8], qB[8];
  {
    const uint32_t cur = big::lds_addr(smem);
    big::Unroll<16>::run([&](auto fI) { read_frag(fI, cur, pA, qA); });
    settle(pA, qA);
  }
#pragma unroll
  for (int a = 0; a < 8; ++a)
    asm volatile("" : "+a"(acc[a][0]), "+a"(acc[a][1]), "+a"(acc[a][2]), "+a"(acc[a][3]), "+a"(acc[a][4]),
                      "+a"(acc[a][5]), "+a"(acc[a][6]), "+a"(acc[a][7]));
  asm volatile("s_nop 4" ::: "memory");  // accumulator zeroing (VALU) -> first MFMA's SrcC
  __builtin_amdgcn_sched_barrier(0);
  // iteration t: stage t+1 must be visible before its fragment reads (own pieces waited + barrier);
  // after the barrier every wave has retired its reads of stage t (iteration t-1), so slot t % S takes
  // stage t + S
  auto iter = [&](int t, const bf16x8 (&pc)[8], const bf16x8 (&qc)[8], bf16x8 (&pf)[8], bf16x8 (&qf)[8]) {
    if (t + 1 < nk) {
      if (!noload) big::wait_stages<8, S>(min(S - 2, nk - 2 - t));
      big::lds_barrier();
    }
    kstep(t, big::lds_addr(smem + ((t + 1) % S) * STAGE), pc, qc, pf, qf);
    settle(pf, qf);
  };
  int t = 0;
  for (; t + 2 <= nk; t += 2) {
    iter(t, pA, qA, pB, qB);
    iter(t + 1, pB, qB, pA, qA);
  }
  if (t < nk) iter(t, pA, qA, pB, qB);  // odd nk: the last k-step
  asm volatile("s_nop 7\n s_nop 7\n s_nop 7" ::: "memory");  // last MFMA -> accumulator reads
  __builtin_amdgcn_sched_barrier(0);
  if (e.dbg & 4) {  // timing experiment: keep the accumulators live, skip the epilogue
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < 8; ++b) asm volatile("" ::"a"(acc[a][b]));
    return;
  }
  // epilogue straight from the fragments: acc[a][b] holds C[i][j..j+3], i = 16a + lane%16, j = 16b + 4*(lane/16)
  // accumulator row a is re-defined in front of its stores, so its AGPR -> VGPR copies are made at this row
  // and not all 256 at once after the loop (which spilled)
  VIT_EPI_FRAG(8, 8, i0 + wi * 128, j0 + wj * 128,
               asm volatile("" : "+a"(acc[a][0]), "+a"(acc[a][1]), "+a"(acc[a][2]), "+a"(acc[a][3]),
                                 "+a"(acc[a][4]), "+a"(acc[a][5]), "+a"(acc[a][6]), "+a"(acc[a][7])))
}

template <class C, int PL, int QL, int EPI, typename TO, typename TA>
__global__ __launch_bounds__(256, 1) void kernel(const bf16* __restrict__ P, int64_t ldp, const bf16* __restrict__ Q,
                                                 int64_t ldq, int M, int N, int R, int r_chunk, Epi e) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  tile<C, PL, QL, EPI, TO, TA>(P, ldp, Q, ldq, M, N, R, r_chunk, e, big::xcd_remap(blockIdx.x, gridDim.x), smem);
}

// two weight gradients over the same token rows in one launch (units [0, a.nwg) are a's)
template <class C, int PL, int QL, int EPI, typename TO, typename TA>
__global__ __launch_bounds__(256, 1) void kernel2(big::PPProb a, big::PPProb b) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int w = big::xcd_remap(blockIdx.x, gridDim.x);
  if (w < a.nwg)
    tile<C, PL, QL, EPI, TO, TA>(a.P, a.ldp, a.Q, a.ldq, a.M, a.N, a.R, a.r_chunk, a.e, w, smem);
  else
    tile<C, PL, QL, EPI, TO, TA>(b.P, b.ldp, b.Q, b.ldq, b.M, b.N, b.R, b.r_chunk, b.e, w - a.nwg, smem);
}

using Default = Cfg<4, 1>;
}  // namespace w4
