// Included by gemm_f32.inc, once inside namespace f32m (SPLIT = 0 / 1: f32 operands), once inside namespace
// f32w (SPLIT = 2: Q is a pre-split weight image) and once inside namespace f32a (SPLIT = 3: P is an activation
// image too; TO = img_t: C is written as one): the tile kernel and the stream-K kernel of the fp32 MFMA GEMM,
// one text for all.  mainloop and the constants are f32m's; epilogue is f32m's, wrapped in f32a.

template <int PL, int QL, int EPI, typename TO, typename TA, int SPLIT>
__global__ __launch_bounds__(THREADS, 2) void gemm_kernel(const float* __restrict__ P, int64_t ldp,
                                                          const float* __restrict__ Q, int64_t ldq, int M, int N,
                                                          int R, int r_chunk, Epi e) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_j = (N + BN - 1) / BN;
  const int tiles = ((M + BM - 1) / BM) * tiles_j;
  const int w = big::xcd_remap(blockIdx.x, gridDim.x);
  const int z = w / tiles, t = w - z * tiles;
  const int ti = t / tiles_j, tj = t - ti * tiles_j;
  const int i0 = ti * BM, j0 = tj * BN;
  const int rb = z * r_chunk;
  const int re = min(R, rb + r_chunk);
  const int nk = (re - rb) / BK;
  f32x4 acc[AI][AJ];
#pragma unroll
  for (int a = 0; a < AI; ++a)
#pragma unroll
    for (int b = 0; b < AJ; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  mainloop<PL, QL, SPLIT>(P, ldp, Q, ldq, M, N, i0, j0, rb, 0, nk, acc, smem, wave, lane);
  epilogue<EPI, TO, TA>(e, acc, M, N, i0, j0, z, wave, lane);
}

// Stream-K form (one split, R % BK == 0) for tile counts that leave a ragged last round (C3's
// 64 x 257 = 16 448 rows are 128.5 row tiles: 1032 / 3096 / 4128 tiles on 512 workgroup slots).
// G persistent workgroups first run `dp_rounds` tile-aligned rounds (tile r*G + w: every workgroup
// starts its tile at k = 0 together with the workgroups that share its operand blocks, so they hit in
// L2 as a plain launch does), then share the remaining tiles x nk k-steps equally.  That remainder is
// at least G tiles, so each workgroup holds at least nk k-steps and a tile is cut at most once, at the
// start of workgroup b (boundary b): its piece 0 (k < cut, from workgroup b-1) and piece 1 (from b)
// are published as f32 fragment images in part[b][piece]; the workgroup that draws the boundary's
// second ticket adds them in piece order (agent-scope release / acquire, cdna_hip_programming.md §5
// "In-launch split-K reduction") and runs the tile's epilogue.  Sums in a fixed order: the result does
// not depend on arrival order.  (Sharing all k-steps from the start measured 2-7 % slower on the tall
// forwards: co-resident workgroups sat at different k offsets of the blocks they share.)
template <int PL, int QL, int EPI, typename TO, typename TA, int SPLIT>
__global__ __launch_bounds__(THREADS, 2) void gemm_sk_kernel(const float* __restrict__ P, int64_t ldp,
                                                             const float* __restrict__ Q, int64_t ldq, int M, int N,
                                                             int R, int dp_rounds, Epi e,
                                                             float* __restrict__ part, int* __restrict__ cnt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_j = (N + BN - 1) / BN;
  const int tiles = ((M + BM - 1) / BM) * tiles_j;
  const int nk = R / BK;
  const int G = gridDim.x, w = big::xcd_remap(blockIdx.x, G);
  for (int r = 0; r < dp_rounds; ++r) {  // tile-aligned rounds
    const int t = r * G + w;
    const int ti = t / tiles_j, tj = t - ti * tiles_j;
    f32x4 acc[AI][AJ];
#pragma unroll
    for (int a = 0; a < AI; ++a)
#pragma unroll
      for (int b = 0; b < AJ; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();  // the previous tile's LDS reads are done before the ring restarts
    mainloop<PL, QL, SPLIT>(P, ldp, Q, ldq, M, N, ti * BM, tj * BN, 0, 0, nk, acc, smem, wave, lane);
    epilogue<EPI, TO, TA>(e, acc, M, N, ti * BM, tj * BN, 0, wave, lane);
  }
  const int tbase = dp_rounds * G;
  const int64_t W = (int64_t)(tiles - tbase) * nk;
  const int64_t s0 = (int64_t)w * W / G, s1 = (int64_t)(w + 1) * W / G;
  constexpr int PIECE = BM * BN;  // floats of one fragment image
  int* flag = reinterpret_cast<int*>(smem + LDS);  // one int past the ring (dynamic LDS holds it)
  for (int64_t s = s0; s < s1;) {
    const int tl = (int)(s / nk), k0 = (int)(s - (int64_t)tl * nk);
    const int t = tbase + tl;
    const int k1 = (int)min((int64_t)nk, k0 + (s1 - s));
    const int ti = t / tiles_j, tj = t - ti * tiles_j;
    const int i0 = ti * BM, j0 = tj * BN;
    f32x4 acc[AI][AJ];
#pragma unroll
    for (int a = 0; a < AI; ++a)
#pragma unroll
      for (int b = 0; b < AJ; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();  // the previous segment's LDS reads are done before the ring restarts
    mainloop<PL, QL, SPLIT>(P, ldp, Q, ldq, M, N, i0, j0, 0, k0, k1, acc, smem, wave, lane);
    s += k1 - k0;
    if (k0 == 0 && k1 == nk) {
      epilogue<EPI, TO, TA>(e, acc, M, N, i0, j0, 0, wave, lane);
      continue;
    }
    // a cut tile: piece 0 ends at the start of workgroup w + 1, piece 1 starts at the start of w
    const int b = k0 == 0 ? w + 1 : w, piece = k0 == 0 ? 0 : 1;
    float* mine = part + ((int64_t)b * 2 + piece) * PIECE + tid * 4;
#pragma unroll
    for (int a = 0; a < AI; ++a)
#pragma unroll
      for (int c = 0; c < AJ; ++c)
        *reinterpret_cast<f32x4*>(mine + (a * AJ + c) * THREADS * 4) = acc[a][c];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      *flag = __hip_atomic_fetch_add(cnt + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (*flag != 1) continue;  // the other piece finishes the tile
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(cnt + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const float* other = part + ((int64_t)b * 2 + (1 - piece)) * PIECE + tid * 4;
#pragma unroll
    for (int a = 0; a < AI; ++a)
#pragma unroll
      for (int c = 0; c < AJ; ++c) {
        const f32x4 o = *reinterpret_cast<const f32x4*>(other + (a * AJ + c) * THREADS * 4);
        acc[a][c] = piece == 0 ? acc[a][c] + o : o + acc[a][c];  // piece 0 + piece 1
      }
    epilogue<EPI, TO, TA>(e, acc, M, N, i0, j0, 0, wave, lane);
  }
}
