// The resident "high" forward (DESIGN 4.23, 4.27), included by attention.hip once per form with
//   X3_FWD_KERNEL  the kernel's name
//   X3_IMAGE       0: qkv and o are f32 (attn_fwd_f32x3); 1: both hold pre-split images (attn_fwd_image_x3) -- the
//                  operand bits come from the image and o is stored as one; everything between is the same text.
// A file, not a shared device function: inlined from one, the f32 form's instances lose an instruction at their end
// (tools/isa_digest.sh --compare), and they are to stay the code they were.
template <int NT, bool CAUSAL>
__global__ __launch_bounds__(AT_THREADS, F32X3<NT>::WPS) void X3_FWD_KERNEL(const float* __restrict__ qkv,
                                                                            int64_t ld_qkv, int D, int H, int N,
                                                                            float scale, float* __restrict__ o,
                                                                            int64_t ld_o, float* __restrict__ lse) {
  using X = AtBf16x3;
  constexpr int NT2 = F32X3<NT>::NT2, ROWS = F32X3<NT>::ROWS, IMG = F32X3<NT>::IMG;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *Khi = smem, *Klo = smem + IMG, *Vhi = smem + 2 * IMG, *Vlo = smem + 3 * IMG;
  const X::Img Kimg = {Khi, Klo}, Vimg = {Vhi, Vlo};
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  const float* base = qkv + (int64_t)b * N * ld_qkv + h * 64;
  x3_load2<ROWS, X3_IMAGE>(Khi, Klo, base + D, ld_qkv, Vhi, Vlo, base + 2 * D, ld_qkv, N);
  const AtOffsets off(lane);
  __syncthreads();
  const float c2 = scale * LOG2E;
  for (int qt = wave; qt < NT; qt += AT_WAVES) {
    const int q = qt * 16 + (lane & 15);
    X::Frag qf[2];
    if constexpr (X3_IMAGE) {
      x3_row_image(base + (int64_t)min(q, N - 1) * ld_qkv, g, qf);
    } else {
      f32x4 x[4];
      x3_row(base + (int64_t)min(q, N - 1) * ld_qkv, g, qf, x);
    }
    f32x4 s[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) s[kt] = X::mma(X::row(Kimg, kt * 16, off.row[kk]), qf[kk], s[kt]);
      if (kt % 4 == 3) __builtin_amdgcn_sched_barrier(0);  // bound K-fragment hoisting (VGPRs)
    }
    // keys >= N exist only in the last tile
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if ((NT - 1) * 16 + 4 * g + r >= N) s[NT - 1][r] = -INFINITY;
    if constexpr (CAUSAL) {
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
    for (int ks = 0; ks < NT2; ++ks) {
      const f32x4 hi = (2 * ks + 1 < NT) ? s[2 * ks + 1 < NT ? 2 * ks + 1 : 0] : f32x4{0.f, 0.f, 0.f, 0.f};
      const X::Frag pf = X::pack(s[2 * ks], hi);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) oacc[dt] = X::mma(X::tr(Vimg, ks * 32, off.tr[dt]), pf, oacc[dt]);
      if (ks % 2 == 1) __builtin_amdgcn_sched_barrier(0);  // bound V-fragment hoisting (VGPRs)
    }
    if (q < N) {
      if constexpr (X3_IMAGE)
        x3_store_row_image(o + ((int64_t)b * N + q) * ld_o + h * 64, oacc, 1.0f / l, g);
      else
        x3_store_row(o + ((int64_t)b * N + q) * ld_o + h * 64, oacc, 1.0f / l, g);
      if (g == 0) lse[(int64_t)bh * N + q] = (mc + __log2f(l)) * LN2;
    }
  }
}
