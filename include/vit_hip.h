/*
 * vit_hip.h -- C ABI of libvit_hip.so, the MI355X (gfx950) kernels behind the
 * ViT training step of seemadhungana/ViT-Project.
 *
 * The reference is pure Python: its hot path reaches GPU code only through
 * torch ops called from timm's VisionTransformer (external) and from its own
 * training loops.  Each entry point below replaces one of those ops; the
 * reference call site it serves is cited as FILE:LINE with
 *   VIT  = Training/vit_training/baseline/train_vit_sgd.py
 *   MEAS = Training/vit_training/single_epoch/measure_single_epoch_perturbation_effect.py
 *   NEWP = Training/functions/new_cvpr_train_behavior_things_pipeline.py
 *
 * Conventions: plain device pointers and sizes; `stream` is a hipStream_t;
 * every function returns 0 or a hipError_t code and never allocates, frees or
 * synchronises (graph-capture safe).  dtype codes: 0 = f32, 1 = bf16.
 * Row strides (ld*) are in elements.
 */
#ifndef VIT_HIP_H
#define VIT_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { VIT_DTYPE_F32 = 0, VIT_DTYPE_BF16 = 1 };
enum { VIT_LAYOUT_RC = 0, VIT_LAYOUT_CR = 1 };
enum {
  VIT_EPI_STORE = 0,      /* C = acc (+bias)                                   */
  VIT_EPI_BIAS_GELU = 1,  /* pre = acc+bias: C = gelu_erf'(pre), aux_out = gelu_erf(pre) */
  VIT_EPI_RESID = 2,      /* C (f32) = resid + acc + bias                      */
  VIT_EPI_GELU_BWD = 3,   /* C = acc * aux (aux = the gelu'(pre) BIAS_GELU saved) */
  VIT_EPI_PATCH = 4,      /* patch-embed row remap + pos_embed                 */
  VIT_EPI_BIAS_QGELU = 5, /* QuickGELU variant (OpenAI CLIP towers): C = qgelu'(pre) */
  VIT_EPI_QGELU_BWD = 6,
  /* 7 is taken inside the library (accumulate into C).  Additive to ABI 10, forward (RC x RC) layout only: */
  VIT_EPI_BIAS_GELU_FWD = 8,  /* pre = acc+bias: C = gelu_erf(pre); nothing else written, aux_out ignored */
  VIT_EPI_BIAS_QGELU_FWD = 9  /* the same with QuickGELU */
};

int vit_abi_version(void); /* 10 (round 6): vit_blaslt_workspace / vit_gemm_lib removed -- the plain bf16
                              * forward / input-gradient GEMMs run the hand-written 4-wave kernel (csrc/
                              * gemm_g4.hip), the library links no vendor BLAS; 9: those two hooks (hipBLASLt);
                              * 8: vit_gemm_ms / vit_gemm_ms_config and the banded attention backward removed.
                              * Additive to 10 (no entry point or argument changed): the act-only epilogue codes
                              * VIT_EPI_BIAS_GELU_FWD / VIT_EPI_BIAS_QGELU_FWD, vit_eval_metrics, and the LoRA weight
                              * build vit_lora_weight_fwd / _bwd / _bwd_ws_floats */

/* Generic MFMA GEMM C[i][j] = epi(sum_r P(i,r) Q(j,r)); layouts RC (r contiguous)
 * or CR (i/j contiguous).  Backs every nn.Linear of timm's ViT reached from
 * VIT:139 (forward) and VIT:142 (backward).
 * Kernel choice (every GEMM entry point below goes through it).  The MFMA kernels need, for bf16: a reduction
 * R % 32 == 0, N % 4 == 0, a CR operand's extent % 8, ldp / ldq % 8 and 16-byte-aligned P and Q (g4 for the plain
 * bf16 store: R % 64, N % 8); for f32: R % 32, N % 4, a CR extent % 4, ldp / ldq % 4, aligned P and Q and at least
 * 64 output tiles of 128 x 128 (times the split).  Their epilogues move 16 bytes at a time, so they also need C,
 * aux_out, bias, aux (the residual / saved act'), pos_embed and the column-sum partial rows 16-byte aligned and
 * ldc (shared by aux_out) and ld_aux multiples of 16 bytes (% 8 in bf16, % 4 in f32).  Anything else runs the
 * generic kernel (one element at a time, any alignment and stride), with the same result on exact data. */
int vit_gemm(int dtype, int out_dtype, int p_layout, int q_layout, int epi, int M, int N, int R,
             const void* P, int64_t ldp, const void* Q, int64_t ldq, void* C, int64_t ldc,
             const float* bias, const void* aux, int64_t ld_aux, void* aux_out, int allow_fast, void* stream);

/* Tuning hook: force GEMM tile configuration v (see csrc/gemm.hip big::V*; 20 = the 4-wave g4 kernel of
 * csrc/gemm_g4.hip for the plain bf16 store classes), -1 = per-shape choice (g4 for the plain bf16
 * forward / input gradient unless VIT_GEMM_G4=0). */
int vit_gemm_variant(int v);

/* Tuning hook: the forward / input-gradient GEMMs walk their tiles in bands of `fwd` / `dgrad`
 * row tiles, column-major inside a band (L2 reuse of the operand blocks); 0 = row-major (the forward
 * default), -1 = the per-shape rule (bands of 8 for wide outputs with >= 4 MiB weights).  The input
 * gradients default to bands of 4 (round 5: the fc2 GELU' one, 3.9x less operand FETCH, +0.65 %);
 * -2 restores a class's default (VIT_GEMM_GROUP_FWD / _DGRAD, else the defaults above). */
int vit_gemm_group(int fwd, int dgrad);

/* The plain bf16 forward (+ f32 bias) and input-gradient GEMMs run the 4-wave g4 kernel (csrc/gemm_g4.hip,
 * VIT:139 / VIT:142 through timm's qkv / proj / fc1 / fc2).  Tuning / test hook: its tile walk for the forward
 * and the input-gradient class (0 = stride over the tiles with min(tiles, CUs or `wgs`) persistent workgroups,
 * 1 = one workgroup per 256-row band walking the column tiles, 2 = stride over the tiles with one workgroup per
 * 256-row band, so the workgroups running together share a band's rows in L2 (the input gradients' default,
 * round 6: +1.1 / +1.3 % over 1), -1 = keep), the stride walk's workgroup cap
 * (0 = the CU count, -1 = keep) and its tiles per workgroup (grid >= ceil(tiles / tpw); 0 = no limit, -1 = keep). */
int vit_gemm_g4_config(int fwd_mode, int dgrad_mode, int wgs, int tpw);

/* Host-side count of g4 launches since the last reset (reset != 0 zeroes it); no GPU call. */
int vit_gemm_g4_count(int reset);

/* Tuning / test hook: the fc2 GELU' input gradient (vit_linear_dgrad with EPI_GELU_BWD / EPI_QGELU_BWD, bf16)
 * on g4 (1: the act' tile arrives by LDS-DMA in the two stage slots past the stream's end, products in place,
 * column partials for the fc1 bias gradient; needs a reduction of at least 128) or on the 8-wave V1 kernel (0);
 * bit 1 (2, 3) also puts the fc1 GELU pair forward on g4; -1 keeps.  Returns the previous setting (default
 * VIT_G4_GELU, else 1). */
int vit_gemm_g4_gelu(int on);

/* Stream-K workspace for the fp32 MFMA GEMMs launched on `stream` (the reference-precision C3 path,
 * NEWP:274): part >= 4 * CUs * 128*128 floats, counters >= 2 * CUs ints, zero-filled before first use
 * (kernels leave them zero).  With it, an f32 GEMM whose tile count would leave a ragged last round
 * (C3's 128.5 row tiles) runs as 2 * CUs persistent workgroups sharing the k-steps equally; cut
 * tiles combine in-launch in a fixed order.  part == NULL removes the stream's entry (host-only); past
 * 32 registered streams a new stream keeps the plain launch. */
int vit_gemm_streamk_workspace(void* stream, float* part, int64_t part_bytes, int* counters, int ncounters);

/* fp32 GEMM arithmetic on the MFMA path (clip_model.float(), NEWP:274; compute_dtype float32):
 * 0 = v_mfma_f32_16x16x4_f32, exact f32 products (default); 1 = each operand as hi + lo bf16
 * (hi = bf16_rne(x), lo = bf16_rne(x - hi)), three bf16 MFMA products (hi*lo, lo*hi, hi*hi), f32
 * accumulate: held to |C - C64| <= (3 * 2^-18 + (R + 3) * 2^-24) |P| |Q|^T on random normal-range data (4.4e-6
 * rms relative error; every rounding at its limit at once would be 3 * 2^-16), exact where both operands are
 * bf16 values; -1 keeps.  Returns the previous setting (default VIT_F32_MATMUL = highest |
 * high, else 0).  The setting is "at most bf16x3": f32 GEMMs that do not take the MFMA path (under 64
 * output tiles, misaligned operands, allow_fast = 0) run the generic kernel and are exact f32 in either
 * mode.  Non-finite in, non-finite out: an infinite (or past-bf16-range) operand gives NaN in mode 1 where
 * mode 0 gives +-inf.  Process-wide, read at launch time.  Additive to ABI 10.  Host-only, no GPU call. */
int vit_gemm_f32_precision(int mode);
/* Host-side launch counts since the last reset: every launch of the f32 MFMA path / those in mode 1. */
int vit_gemm_f32_count(int reset);
int vit_gemm_f32_split_count(int reset);

/* Pre-split weight images for mode 1 (additive to ABI 10).  In mode 1 both operands are split into hi / lo bf16 in
 * registers, by every wave in every k-step; a frozen weight's split can be done once.  The image of an f32 matrix
 * A [rows][red] has A's size and a row pitch of red * 4 bytes: each 128-byte block of 32 reduction values holds
 * four 16-byte hi chunks, then four lo chunks, and hi chunk g holds as its bf16 element j = 0..7 the hi of
 * k = 16 (j >> 2) + 4 g + (j & 3); lo chunk g the lo values in the same order.  That is the operand pack the
 * kernel forms in registers, so a GEMM that reads the image issues the same MFMAs on the same bits: its result is
 * mode 1's bit for bit.
 * vit_gemm_f32_weight_image writes the image of W [N][K] (row stride ldw; transpose == 0: N rows x K cells, the
 * forward's operand) or of W^T (transpose != 0: K rows x N cells, the input gradient's operand).  The reduction
 * extent (K, or N transposed) must be a multiple of 32, W and img 16-byte aligned, ldw a multiple of 4 and >= K;
 * otherwise hipErrorInvalidValue with nothing launched.  img holds N * K * 4 bytes and may not overlap W. */
int vit_gemm_f32_weight_image(int N, int K, const float* W, int64_t ldw, int transpose, void* img, void* stream);
/* Launches of the f32 MFMA path that read a weight image since the last reset (they also count in
 * vit_gemm_f32_count and vit_gemm_f32_split_count). */
int vit_gemm_f32_presplit_count(int reset);

/* Pre-split activation images for mode 1 (additive to ABI 10).  With a weight image the activation is
 * the one operand still split in every k-step.  In a forward-only chain an activation is read by one GEMM and
 * nothing else, so the kernel that produces it can write its image instead: the same bytes, the same row pitch.
 * VIT_DTYPE_F32_SPLIT names such a buffer: f32-sized, holding the image (rule above) of the f32 matrix with that
 * row pitch, row by row -- what vit_gemm_f32_weight_image(rows, K, X, ldx, 0, ..) writes for a contiguous one.
 *   - dtype_y of vit_layer_norm_fwd (f32 x) and vit_add_layer_norm_fwd: y is written as the image of the f32 y;
 *     mean, rstd and xs are unchanged.  Vector kernels only: D % 256 == 0 with the alignment they ask for (ldy % 4,
 *     y 16-byte aligned); anything else is hipErrorInvalidValue with nothing launched.
 *   - out_dtype of vit_linear_fwd_wimg with VIT_EPI_STORE, VIT_EPI_BIAS_GELU_FWD or VIT_EPI_BIAS_QGELU_FWD: Y is
 *     written as the image of the f32 Y of the same call.  Needs N % 32 == 0.
 *   - dtype of vit_linear_fwd_wimg (X is an image; K % 32 == 0) with those three epilogues or VIT_EPI_RESID: the
 *     result is the f32-X call's bit for bit.  W must still be given the way that call gets it (it is not read).
 * In both linear forms act_out must be NULL (none of those epilogues writes one).  The LayerNorm entries take the code when
 * vit_layer_norm_fwd_image_ok says so (host-only: add = 0 / 1 for vit_layer_norm_fwd / vit_add_layer_norm_fwd, D, the
 * OR of every row stride and the OR of every address of the call): D % 256 == 0 up to 2048 -- but not 1280 or 1792
 * for vit_layer_norm_fwd, whose f32 form runs the element-wise kernel there -- strides % 4 == 0, 16-byte alignment.
 * A linear call that names the code in either place runs only on the pre-split MFMA kernels: when Wimg is NULL, the
 * mode is not 1, or the same call with f32 X and Y would not take the f32 MFMA path (vit_linear_fwd_f32_mfma below,
 * and 16-byte aligned Y, bias, resid with ldy % 4 == 0), it returns hipErrorInvalidValue with nothing launched.
 * Image bytes are never read as floats there (vit_linear_fwd, which has no Wimg, refuses the code too).  The three
 * entry points above are the only ones that know the code: pass it to no other.
 * vit_linear_fwd_f32_mfma (host-only, no GPU call): 1 when an f32 forward of these M, N, K with X (row pitch ldx)
 * and W at these addresses takes the f32 MFMA path in either mode -- at least 64 output tiles of 128 x 128,
 * K % 32 == 0, N % 4 == 0, ldx % 4 == 0, X and W 16-byte aligned -- else 0.  Only the addresses' alignment is
 * looked at.  Ask before asking a producer for an image.
 * vit_gemm_f32_presplit_act_count: launches that read an activation image since the last reset (they count in
 * the three counters above as well). */
enum { VIT_DTYPE_F32_SPLIT = 2 };
int vit_linear_fwd_f32_mfma(int M, int N, int K, const void* X, int64_t ldx, const void* W);
int vit_gemm_f32_presplit_act_count(int reset);
int vit_layer_norm_fwd_image_ok(int add, int D, int64_t strides_or, uint64_t ptrs_or);

/* Host-only query (no GPU call): rows per launch the bf16 MFMA path uses for a row-contiguous
 * operand of M rows x ld elements (its staging offsets are 32-bit: larger operands are split
 * into row chunks, a multiple of 256 rows each); M when one launch fits, 0 if none does. */
int vit_gemm_rc_chunk_rows(int M, int64_t ld);

/* F.linear forward, Y = X W^T + b with fused epilogue (timm Attention.qkv/proj,
 * Mlp.fc1+GELU / fc2 + residual, head; under VIT:138-139 autocast).  With VIT_EPI_BIAS_GELU_FWD /
 * VIT_EPI_BIAS_QGELU_FWD (passes no backward follows: VIT:167-204's validate, frozen CLIP blocks) Y is the
 * activation itself, bit for bit what the pair code stores into act_out on the same kernel path, and
 * act_out may be NULL. */
int vit_linear_fwd(int dtype, int out_dtype, int epi, int M, int N, int K, const void* X, int64_t ldx,
                   const void* W, const float* bias, void* Y, int64_t ldy, const void* resid,
                   void* act_out, void* stream);
/* The same, with Wimg = the image of W (vit_gemm_f32_weight_image(N, K, W, K, 0, ..) of W's current values).  When
 * the mode is 1, Wimg is not NULL, dtype is f32 and the call takes the f32 MFMA path, the image alone is read and W
 * is never dereferenced; the result is vit_linear_fwd's bit for bit.  In every other case this is vit_linear_fwd. */
int vit_linear_fwd_wimg(int dtype, int out_dtype, int epi, int M, int N, int K, const void* X, int64_t ldx,
                        const void* W, const float* bias, void* Y, int64_t ldy, const void* resid,
                        void* act_out, const void* Wimg, void* stream);

/* F.linear input gradient dX = dY W (+ GELU' epilogue) -- autograd of VIT:142.  dbias (optional) =
 * column sums of dX (bias gradient of the Linear that produced dX's forward value, e.g. fc1.bias from
 * fc2's dgrad); partial >= vit_linear_dgrad_partial_floats, else hipErrorInvalidValue with nothing launched.
 * What is summed depends on the path.  On the MFMA kernels the sums are fused into the epilogue and take its f32
 * values BEFORE they are rounded to dX's type: with the GELU' epilogue, the column sums of the f32 products
 * acc * act'.  On the generic path (and when only `partial` is not 16-byte aligned) a second kernel reads dX
 * back: the column sums of dX AS STORED.  The two agree for an f32 dX and differ by the bf16 roundings
 * otherwise; each is a fixed-order sum. */
int vit_linear_dgrad(int dtype, int out_dtype, int epi, int M, int N, int K, const void* dY, int64_t lddy,
                     const void* W, void* dX, int64_t lddx, const void* pre, float* dbias, float* partial,
                     int64_t partial_floats, int defer_reduce, void* stream);
/* The same, with Wimg = the image of W^T (vit_gemm_f32_weight_image(N, K, W, K, 1, ..)), read in place of W under
 * the rule of vit_linear_fwd_wimg; dX and the fused column sums are vit_linear_dgrad's bit for bit. */
int vit_linear_dgrad_wimg(int dtype, int out_dtype, int epi, int M, int N, int K, const void* dY, int64_t lddy,
                          const void* W, void* dX, int64_t lddx, const void* pre, float* dbias, float* partial,
                          int64_t partial_floats, int defer_reduce, const void* Wimg, void* stream);
/* defer_reduce = 1: dbias is not written; `partial` keeps its [ceil(M/64)][K] column-sum
 * partials for the caller to reduce with vit_colreduce (e.g. on another stream, off the
 * input-gradient chain). */
int vit_linear_dgrad_partial_floats(int M, int K);

/* F.linear weight gradient dW (f32) = dY^T X, split-K over rows with fp32 slabs
 * in `workspace` (>= split*N*K*4 bytes, else hipErrorInvalidValue with nothing launched) -- autograd of
 * VIT:142.  The slab sum moves 16 bytes at a time: with N*K % 4 != 0, or a workspace or dW that is not 16-byte
 * aligned, the call runs unsplit (the same sum in one pass); a misaligned dW also keeps the generic kernel.
 * A split call adds the ragged M % 32 rows into the last slab before it sums the slabs (slab 0, then += slab z),
 * as vit_linear_wgrad_partials does: with at most 8 slabs dW is bit for bit what vit_colreduce_batch makes of
 * that call's slabs. */
int vit_linear_wgrad(int dtype, int M, int N, int K, const void* dY, int64_t lddy, const void* X,
                     int64_t ldx, float* dW, int split, void* workspace, int64_t ws_bytes, void* stream);
/* The same weight gradient as split-K partials only: slabs[z][N*K] f32 for
 * z < vit_linear_wgrad_nslabs(...), dW = sum_z slabs[z] (ragged M % 32 rows folded into the last
 * slab); the caller reduces them -- the block backward's single vit_colreduce_batch launch
 * (S = nslabs, N = N*K).  bf16, or f32 on the MFMA path. */
int vit_linear_wgrad_nslabs(int dtype, int M, int N, int K, int split);
int vit_linear_wgrad_partials(int dtype, int M, int N, int K, const void* dY, int64_t lddy, const void* X,
                              int64_t ldx, int split, float* slabs, int64_t slab_bytes, void* stream);
/* Two weight gradients of one block over the same M token rows (fc2 + fc1, or proj + qkv, from
 * the autograd of VIT:142) as ONE launch of split-K partials: slabs_a / slabs_b as
 * vit_linear_wgrad_partials for (Na, Ka) / (Nb, Kb) with the same split.  bf16, M % 32 == 0;
 * otherwise hipErrorInvalidValue and nothing is launched. */
int vit_linear_wgrad_partials2(int M, int split, int Na, int Ka, const void* dYa, int64_t lddya, const void* Xa,
                               int64_t ldxa, float* slabs_a, int64_t bytes_a, int Nb, int Kb, const void* dYb,
                               int64_t lddyb, const void* Xb, int64_t ldxb, float* slabs_b, int64_t bytes_b,
                               void* stream);

/* Column sums (bias gradients): out[N] = sum_i X[i][:] -- autograd of VIT:142. */
int vit_colsum(int dtype, int M, int N, const void* X, int64_t ld, float* out, float* partial,
               int64_t partial_floats, int accumulate, void* stream);
/* out[N] (+)= sum_z part[z][:] over S partial rows (second stage of fused bias gradients);
 * scratch optional (>= ceil(S/64)*N floats, faster for S > 64). */
int vit_colreduce(const float* part, int S, int N, float* out, int accumulate, float* scratch, void* stream);
/* nq (1..3) stacked [S][N] partial matrices (part + q*S*N) reduced into out0..out2 with one
 * launch per stage (the LayerNorm backward's dgamma | dbeta | dsum partials); scratch optional
 * (>= nq*ceil(S/64)*N floats). */
int vit_colreduce_multi(const float* part, int nq, int S, int N, float* out0, float* out1, float* out2,
                        int accumulate, float* scratch, void* stream);

/* Every deferred column reduction of one transformer block's backward (the bias gradients of
 * qkv / proj / fc1 / fc2 and the norm1 / norm2 affine gradients, autograd of VIT:142) in ONE
 * launch: jobs = njobs x {part, out, S, N, accumulate} as int64 in host memory, each
 * out[N] (+)= sum of the S rows of part [S][N].  Sums run in a fixed order (bitwise reproducible);
 * jobs with more than 64 partial rows combine 64-row chunk partials in-launch (agent-scope
 * release/acquire + a ticket counter per 256-column strip).  scratch / counters sized by
 * vit_colreduce_batch_sizes; counters zero-filled before first use (the kernel leaves them zero).
 * scratch must be 16-byte aligned; each job that takes scratch gets a slice of it whose size is rounded up to a
 * multiple of 4 floats (in both functions), so every slice starts on 16 bytes whatever jobs stand in front of it. */
int vit_colreduce_batch_sizes(const int64_t* jobs, int njobs, int64_t* scratch_floats, int* counters);
int vit_colreduce_batch(const int64_t* jobs, int njobs, float* scratch, int64_t scratch_floats, int* counters,
                        int ncounters, void* stream);

/* timm PatchEmbed Conv2d(3,768,16,16) as GEMM over unfolded patches, writing
 * rows b*(np+1)+1+p of the f32 token stream with pos_embed added (VIT:139). */
int vit_patch_embed_fwd(int dtype, int B, int np, int D, int K, const void* U, const void* W,
                        const float* bias, const float* pos, float* x, void* stream);
/* Conv2d 16/16 unfold: img f32 [B,C,H,W] -> U [B*np, C*ps*ps] (column = c*ps*ps+ky*ps+kx). */
int vit_patch_unfold(int dtype, int B, int C, int Hi, int Wi, int ps, const float* img, void* U, void* stream);
/* ABI 7: the same with U rows ldu >= C*ps*ps elements apart, columns [C*ps*ps, ldu) zero-filled, and the
 * patch embedding over such rows (K = the padded reduction length, W [D][ldw] zero past the real
 * columns): CLIP ViT-L/14's 3*14*14 = 588 columns padded to 608 run on the MFMA GEMM instead of the
 * scalar-FMA kernel (NEWP:274's visual conv1).  vit_copy_rows_padded builds such a W: dst[r][c] =
 * src[r][c] for c < cols, 0 up to ld_dst. */
int vit_patch_unfold_ld(int dtype, int B, int C, int Hi, int Wi, int ps, int ldu, const float* img, void* U,
                        void* stream);
int vit_patch_embed_fwd_ld(int dtype, int B, int np, int D, int K, const void* U, int64_t ldu, const void* W,
                           int64_t ldw, const float* bias, const float* pos, float* x, void* stream);
int vit_copy_rows_padded(int dtype, int rows, int cols, const void* src, int64_t ld_src, void* dst, int64_t ld_dst,
                         void* stream);
/* cat(cls_token) + pos_embed[0] into row 0 of every image (timm _pos_embed). */
int vit_cls_pos_fill(int B, int S, int D, float* x, const float* cls, const float* pos, void* stream);
/* d pos_embed [S,D] = sum_b dx[b]; d cls_token = d pos_embed[0]. */
int vit_pos_grad(int B, int S, int D, const float* dx, float* dpos, float* dcls, void* stream);

/* Tuning hook: LayerNorm backward form for D % 256 == 0 -- 1 = software-pipelined (next row's loads
 * issued before this row's stores; default), 0 = the plain row loop.  Equal to rounding. */
int vit_layer_norm_bwd_variant(int v);

/* F.layer_norm forward (timm norm1/norm2/norm, eps 1e-6), one wave per row; saves mean/rstd.
 * D <= 2048.  16-byte accesses when D % 256 == 0, strides % 4 == 0 and x, y, w, b are aligned to 4 elements
 * (16 bytes of f32, 8 of bf16); anything else takes the element-wise kernel. */
int vit_layer_norm_fwd(int dtype_x, int dtype_y, int rows, int D, const void* x, int64_t ldx, void* y,
                       int64_t ldy, const float* w, const float* b, float* mean, float* rstd, float eps,
                       void* stream);
/* xs = x + r (f32 residual stream + a Linear's output (dtype_r bf16 or f32), bias included; xs may alias
 * x) and, when y is non-null, y = LayerNorm(xs) (dtype_y) with mean/rstd: timm Block's `x = x + attn(norm1(x))` /
 * `x = x + mlp(norm2(x))` residual adds (VIT Block.forward via timm) fused into the LayerNorm that
 * follows them (norm2 of the same block, norm1 of the next); y == null: the add alone (last block).
 * D % 256 == 0, strides % 4 == 0, x / r / xs / y / w / b aligned to 4 elements (there is no element-wise
 * form: anything else is hipErrorInvalidValue). */
int vit_add_layer_norm_fwd(int dtype_r, int dtype_y, int rows, int D, const float* x, int64_t ldx, const void* r,
                           int64_t ldr, float* xs, int64_t ldxs, void* y, int64_t ldy, const float* w, const float* b,
                           float* mean, float* rstd, float eps, void* stream);
/* LayerNorm backward with fused residual-gradient add, optional GEMM-dtype copy
 * of dx (optionally dropping CLS rows), dgamma/dbeta, and dsum = column sums of dx
 * (bias gradient of the Linear whose output fed the residual: proj / fc2).
 * Vector kernels when D is 768 or 1024, every stride % 4 == 0 and x, dy, w, dres, dx, dx_copy are aligned to
 * 4 elements; the element-wise kernel otherwise. */
int vit_layer_norm_bwd(int dtype_x, int dtype_dy, int rows, int D, const void* x, int64_t ldx,
                       const void* dy, int64_t lddy, const float* w, const float* mean, const float* rstd,
                       const float* dres, int64_t ldres, float* dx, int64_t lddx, void* dx_copy, int64_t ld_copy,
                       int dtype_copy, int compact_np, float* dgamma, float* dbeta, float* dsum, float* partial,
                       int64_t partial_floats, int defer_reduce, void* stream);
/* defer_reduce = 1: dgamma / dbeta / dsum are not written; `partial` keeps their
 * [ceil(rows/64)][D] partials at float offsets 0, nblk*D, 2*nblk*D (followed by the
 * vit_colreduce scratch) for the caller to reduce with vit_colreduce. */
/* Additive to ABI 10: the same backward with a compact residual gradient.  dres holds one row (stride ldres)
 * per res_every rows of dx and is added to rows 0, res_every, 2 * res_every, ...; every other row adds zero
 * (bit for bit the dense form over a dres that is zero outside those rows, which is then neither allocated,
 * zero-filled nor read).  The class-token head (timm global_pool='token', VIT:139) sends a gradient into the
 * last block that is non-zero on each image's row 0 alone: res_every = tokens per image. */
int vit_layer_norm_bwd_cls(int dtype_x, int dtype_dy, int rows, int D, const void* x, int64_t ldx,
                           const void* dy, int64_t lddy, const float* w, const float* mean, const float* rstd,
                           const float* dres, int64_t ldres, int res_every, float* dx, int64_t lddx, void* dx_copy,
                           int64_t ld_copy, int dtype_copy, int compact_np, float* dgamma, float* dbeta, float* dsum,
                           float* partial, int64_t partial_floats, int defer_reduce, void* stream);
int vit_layer_norm_bwd_partial_floats(int rows, int D);
int vit_layer_norm_bwd_blocks(int rows); /* partial rows: the [nblk][D] partial blocks' nblk */

/* F.scaled_dot_product_attention(q,k,v) (timm Attention, head_dim 64, any N) reading q/k/v in
 * place from the qkv GEMM output; lse [B*H*N] f32.  causal = 1 masks key > query: the CLIP text
 * tower's nn.MultiheadAttention attn_mask (NEWP:298 through the CLIP-HBA fork, external).
 * N <= 288: the kernels that hold a head's K and V in LDS.  N > 288, non-causal: bf16 with
 * ld_qkv % 8 == 0 and ld_o % 4 == 0, and f32 with every row stride % 4 == 0, take the streamed MFMA
 * kernels of their dtype; causal or misaligned operands the generic scalar kernels (slow;
 * B*H <= 65535). */
int vit_sdpa_fwd(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, void* o,
                 int64_t ld_o, float* lse, float scale, int causal, void* stream);
/* Additive to ABI 10: the query-limited forward for a block whose output is read in row 0 of each image alone
 * (timm global_pool='token' after the last block, VIT:139).  bf16, N <= 288, ld_qkv % 8 == 0, ld_o % 4 == 0: the
 * resident MFMA kernel on query tile 0 -- rows 0..15 of every image keep vit_sdpa_fwd's bits in o and lse, every
 * other row gets o = 0 and lse = +inf (a backward over those rows then sees p = 0 and delta = 0 exactly).  Any
 * other dtype / N / alignment: vit_sdpa_fwd unmasked, all rows.  vit_sdpa_cls_count: host-side count of calls
 * that took the query-limited kernel (reset != 0 zeroes it after reading). */
int vit_sdpa_fwd_cls(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, void* o,
                     int64_t ld_o, float* lse, float scale, void* stream);
int vit_sdpa_cls_count(int reset);
/* One-query attention (additive to ABI 10): query row 0 of every image against all N keys and values, for the
 * class-token tail of the CLIP visual tower (ln_post reads x[:, 0] alone).  VIT_BF16 or VIT_F32, head_dim 64,
 * 1 <= N <= 2048; memory-bound K / V reads, f32 arithmetic, every reduction in a fixed order (two calls are
 * bitwise equal), no atomics, no workspace.  The sums are ordered differently from the MFMA kernels': the
 * results agree with vit_sdpa_fwd / vit_sdpa_bwd to rounding, not in bits.
 *   fwd: s_j = scale * (q0 . k_j), lse = logsumexp_j s_j (natural log), o0 = sum_j softmax(s)_j v_j; K and V are
 *        read once.  o_cls [B, D] in the qkv dtype, row b at b * ld_o (column h * 64) -- the dense o with
 *        ld_o = N * D is a valid argument; lse_cls [B * H] f32.
 *   bwd: p_j = exp(s_j - lse), delta = dO0 . o0 (computed in the kernel), ds_j = p_j (dO0 . v_j - delta).  Writes
 *        every element of dqkv [B*N, 3D] (qkv layout, qkv dtype): dq row 0 of each image = scale sum_j ds_j k_j,
 *        dq rows 1 .. N-1 exact zeros, dk_j = scale ds_j q0 and dv_j = p_j dO0 for every row.  do_cls [B, D], row
 *        b at b * ld_do.  K and V are read once.  No qkv bias partials are produced.  Consistency step: sum_j ds_j
 *        is zero in exact arithmetic; o0 arrives rounded to the dtype, which shifts delta and leaves a remainder
 *        r that a common offset of the keys multiplies into dq.  The kernel takes it back out with what it has
 *        summed by then: ds_j -= p_j r / sum_j p_j (dk_j is written from the corrected values, held in LDS: two
 *        floats a key, hence the bound on N).
 * head_dim != 64, N <= 0 or N > 2048, ld_qkv / ld_dqkv < 3D, a null operand, or a row stride or address that is
 * not a multiple of 16 bytes: hipErrorInvalidValue with nothing queued.
 * vit_sdpa_cls1_count: host-side count of launches of either kernel (reset != 0 zeroes it after reading). */
int vit_sdpa_cls1_fwd(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, void* o_cls,
                      int64_t ld_o, float* lse_cls, float scale, void* stream);
int vit_sdpa_cls1_bwd(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv,
                      const void* o_cls, int64_t ld_o, const void* do_cls, int64_t ld_do, const float* lse_cls,
                      void* dqkv, int64_t ld_dqkv, float scale, void* stream);
int vit_sdpa_cls1_count(int reset);
/* One-query attention at a row per sequence (additive to ABI 10), forward only: the query of (b, h) is row
 * qrow[b] of sequence b, the keys and values rows 0 .. nk - 1 with nk = qrow[b] + 1 if causal != 0, else N.  For
 * the last block of the CLIP text tower, of whose output ln_final reads the EOT row alone.  The
 * device code, decomposition and summation order are vit_sdpa_cls1_fwd's: qrow[b] = 0 for every b with causal = 0
 * gives that call's o and lse bit for bit, and a causal call equals the unmasked call on the first qrow[b] + 1
 * rows.  qrow: int64 [B] on the device; the host cannot see its values, so the kernel clamps each to [0, N - 1].
 * No K / V row >= nk is loaded; nothing but o_row [B, D] (qkv dtype, row b at b * ld_o, column h * 64) and
 * lse_row [B * H] (f32, natural log) is stored.  There is no backward: a caller takes this route only where no
 * attention backward follows.  head_dim != 64, N <= 0 or N > 2048, ld_qkv < 3D, a null operand (qrow included),
 * or a row stride or address that is not a multiple of 16 bytes: hipErrorInvalidValue with nothing queued.
 * vit_sdpa_row1_count: host-side count of its launches (reset != 0 zeroes it after reading). */
int vit_sdpa_row1_fwd(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv,
                      const int64_t* qrow, int causal, void* o_row, int64_t ld_o, float* lse_row, float scale,
                      void* stream);
int vit_sdpa_row1_count(int reset);
/* fp8 scaled-dot-product attention forward (BASELINE configs[4]: the sweep's frozen CLIP tower blocks
 * and the RSA evaluation forward; replaces the same F.scaled_dot_product_attention call as
 * vit_sdpa_fwd): q/k/v quantised in-kernel to block-scaled OCP e4m3 (E8M0 scale per 32 values),
 * S = QK^T and O = PV on v_mfma_scale_f32_32x32x64_f8f6f4, softmax in f32.  dtype = qkv/o dtype
 * (VIT_BF16 or VIT_F32); head_dim 64, N <= 320; lse may be null.  Forward only. */
int vit_sdpa_fwd_fp8(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, void* o,
                     int64_t ld_o, float* lse, float scale, int causal, void* stream);
/* The streamed form of vit_sdpa_fwd_fp8 (additive to ABI 10): the same quantisation, MFMAs and f32
 * online softmax, with K and V passing through a two-buffer LDS ring of 64-key chunks instead of
 * living there whole, so any N >= 1 runs; grid (B*H, ceil(N / 256)).  Up to 320 tokens o and lse are
 * bit for bit vit_sdpa_fwd_fp8's.  Same arguments and refusals otherwise (head_dim != 64,
 * ld_qkv % 8, ld_o % 4: hipErrorInvalidValue).  Forward only. */
int vit_sdpa_fwd_fp8_stream(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv,
                            void* o, int64_t ld_o, float* lse, float scale, int causal, void* stream);
/* Host-side count of vit_sdpa_fwd_fp8_stream calls that launched (reset != 0 zeroes it after reading). */
int vit_sdpa_fp8_stream_count(int reset);
/* The quantise-once form of vit_sdpa_fwd_fp8_stream (additive to ABI 10): K and V are quantised once per
 * head into a workspace and the forward streams the ready-made e4m3 images and E8M0 scale bytes through
 * the LDS ring, instead of quantising them again in every 256-query block.
 * vit_sdpa_fp8_kv_bytes: the workspace size in bytes for (B, H, N); its layout is private to the library
 * (hipErrorInvalidValue for B, H or N < 1 or a null `bytes`). */
int vit_sdpa_fp8_kv_bytes(int B, int H, int N, int64_t* bytes);
/* The pre-pass: quantises K and V of the fused qkv (dtype VIT_BF16 or VIT_F32) exactly as
 * vit_sdpa_fwd_fp8_stream does and writes every byte of the first vit_sdpa_fp8_kv_bytes bytes of ws, which
 * is then a pure function of K and V.  Refusals (hipErrorInvalidValue, nothing launched): head_dim != 64,
 * N < 1, ld_qkv % 8, a null ws, ws not 16-byte aligned, ws_bytes below vit_sdpa_fp8_kv_bytes. */
int vit_sdpa_fp8_quant_kv(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, void* ws,
                          int64_t ws_bytes, void* stream);
/* The consumer: o and lse bit for bit vit_sdpa_fwd_fp8_stream's at every N, with K and V read from ws (as
 * vit_sdpa_fp8_quant_kv left it for the same B, H, N) and nowhere else; qkv is read for Q alone, ws is not
 * written, lse may be null.  Refusals as the pre-pass, and ld_o % 4.  Forward only. */
int vit_sdpa_fwd_fp8_pre(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv,
                         const void* ws, int64_t ws_bytes, void* o, int64_t ld_o, float* lse, float scale,
                         int causal, void* stream);
/* Host-side count of vit_sdpa_fwd_fp8_pre calls that launched (reset != 0 zeroes it after reading). */
int vit_sdpa_fp8_pre_count(int reset);
/* SDPA backward into dqkv (qkv layout). delta_ws >= B*H*N floats.  dbias (optional, [3*H*64]) =
 * column sums of dqkv (the qkv Linear's bias gradient), fused into the kernels;
 * partial >= vit_sdpa_bwd_partial_floats(B, N, H*64).  dbias == NULL with partial != NULL (bf16
 * only): the kernels leave the per-image [B][3*H*64] partial sums in `partial` for the caller to
 * reduce (vit_colreduce_batch).  N > 288 (bf16): the partials come from a per-image column-sum pass
 * over dqkv after the two kernels; same layout, fixed summation order.  N > 288 (f32, non-causal,
 * every row stride % 4 == 0): the streamed f32 MFMA kernels, dbias by a column sum over dqkv. */
int vit_sdpa_bwd(int dtype, int B, int H, int N, int head_dim, const void* qkv, int64_t ld_qkv, const void* o,
                 int64_t ld_o, const void* dout, int64_t ld_do, const float* lse, void* dqkv, int64_t ld_dqkv,
                 float* delta_ws, float scale, int causal, float* dbias, float* partial, int64_t partial_floats,
                 void* stream);
int vit_sdpa_bwd_partial_floats(int B, int N, int D);
/* Kernel choice of vit_sdpa_fwd / vit_sdpa_bwd past 288 tokens where the streamed MFMA kernels apply:
 * -1 = from the environment (VIT_ATTN_LONG=0|1, default 1), 0 = the generic kernels, 1 = streamed
 * (bf16 and f32 alike; VIT_ATTN_F32_GENERIC=1 also keeps f32 on the generic kernels).
 * Returns the previous mode. */
int vit_sdpa_long_config(int mode);
/* Host-side count of vit_sdpa_fwd / vit_sdpa_bwd calls that took the streamed bf16 kernels, so a test
 * can see which kernel ran (reset != 0 zeroes it after reading). */
int vit_sdpa_long_count(int reset);
/* The same count for the streamed f32 kernels (additive to ABI 10). */
int vit_sdpa_long_f32_count(int reset);
/* fp32 arithmetic of the resident f32 attention kernels (f32 operands, N <= 288, head_dim 64, every row stride a
 * multiple of 4, causal or not): 0 = v_mfma_f32_16x16x4_f32, exact f32 products (default); 1 = every matrix
 * product of vit_sdpa_fwd (Q K^T, P V) and vit_sdpa_bwd (S, dP, dQ, dK, dV) as three bf16 MFMA products of hi + lo
 * operands (the rule of vit_gemm_f32_precision), f32 accumulate; the softmax, delta, lse, the scale factors and
 * the stores stay f32.  -1 keeps; any other value is ignored.  Returns the previous setting (initially
 * VIT_F32_ATTENTION = highest | high, else 0).  Independent of vit_gemm_f32_precision.  "At most bf16x3": the
 * streamed f32 kernels past 288 tokens (unless vit_sdpa_f32_long_precision(1) is set too), the generic kernels, vit_sdpa_cls1_* / vit_sdpa_row1_fwd and
 * vit_sdpa_fwd_cls are exact f32 in either mode.  +-inf in gives NaN out in mode 1 (the -inf of the masks is
 * applied after the products and is not affected).  Process-wide, read at launch time: a backward runs in the
 * mode current when it runs.  Additive to ABI 10.  Host-only, no GPU call. */
int vit_sdpa_f32_precision(int mode);
/* Host-side count of vit_sdpa_fwd / vit_sdpa_bwd calls that took the bf16x3 kernels (one per call; reset != 0
 * zeroes it after reading): a test's guard against a silent fallback. */
int vit_sdpa_f32_split_count(int reset);
/* fp32 arithmetic of the streamed f32 attention kernels (f32 operands, N > 288, head_dim 64, every row stride a
 * multiple of 4, not causal): 0 = v_mfma_f32_16x16x4_f32, exact f32 products (default); 1 = the three bf16 MFMA
 * products of vit_sdpa_f32_precision(1) on the streamed schedule, taken only while vit_sdpa_f32_precision is 1 as
 * well -- that switch alone leaves streamed attention exact.  -1 keeps; any other value is ignored.  Returns the
 * previous setting (initially 1 under VIT_F32_ATTENTION_LONG=1, else 0).  The generic kernels past 288 tokens
 * (causal, misaligned rows, vit_sdpa_long_config(0), VIT_ATTN_F32_GENERIC=1) stay exact f32.  Process-wide, read at
 * launch time.  Additive to ABI 10.  Host-only, no GPU call. */
int vit_sdpa_f32_long_precision(int mode);
/* Host-side count of vit_sdpa_fwd / vit_sdpa_bwd calls that took the streamed bf16x3 kernels (one per call; they
 * count in vit_sdpa_long_f32_count as well and never in vit_sdpa_f32_split_count; reset != 0 zeroes it). */
int vit_sdpa_long_f32_split_count(int reset);
/* Pre-split images through f32 "high" attention (additive to ABI 10), forward only.  qkv_img holds the
 * pre-split activation image (the rule of vit_gemm_f32_weight_image, row by row at the f32 row pitch ld_qkv: what
 * vit_linear_fwd_wimg writes with out_dtype VIT_DTYPE_F32_SPLIT) of the f32 qkv of vit_sdpa_fwd, and o_img receives the
 * image of the f32 o that vit_sdpa_fwd would write (row pitch ld_o; what vit_linear_fwd_wimg reads with dtype
 * VIT_DTYPE_F32_SPLIT); lse is vit_sdpa_fwd's.  The image forms of the bf16x3 kernels run: the same MFMAs on the same
 * bits, so o_img is the image of vit_sdpa_fwd's o and lse its lse, bit for bit.  Both ends are images or neither.
 * It launches only where vit_sdpa_fwd with f32 tensors would take the bf16x3 kernels: vit_sdpa_f32_precision is 1,
 * head_dim 64, ld_qkv and ld_o multiples of 4, qkv_img and o_img 16-byte aligned (checked here; vit_sdpa_fwd takes
 * that on trust), and either N <= 288 (causal or
 * not) or N > 288 with causal == 0, the streamed kernels on (vit_sdpa_long_config) and vit_sdpa_f32_long_precision 1.
 * Anything else returns hipErrorInvalidValue with nothing launched and nothing written: an image is never read as floats.
 * vit_sdpa_fwd_takes_image (host-only, no GPU call): 1 exactly when that entry would launch; strides_or = ld_qkv | ld_o,
 * ptrs_or = the OR of the addresses of qkv_img and o_img (lse is stored a float at a time: any address).  Ask before asking the qkv GEMM for an image.
 * vit_sdpa_f32_image_count: calls of vit_sdpa_fwd_image that launched since the last reset (reset != 0 zeroes it); they
 * count in vit_sdpa_f32_split_count (N <= 288) or vit_sdpa_long_f32_count and vit_sdpa_long_f32_split_count (past 288)
 * as the f32 forms do. */
int vit_sdpa_fwd_image(int B, int H, int N, int head_dim, const void* qkv_img, int64_t ld_qkv, void* o_img,
                       int64_t ld_o, float* lse, float scale, int causal, void* stream);
int vit_sdpa_fwd_takes_image(int B, int H, int N, int head_dim, int causal, int64_t strides_or, uint64_t ptrs_or);
int vit_sdpa_f32_image_count(int reset);
/* Tuning hook: the bf16 backward form for N <= 224 (-1 = from VIT_ATTN_BWD_SPLIT, 1 = whole-head fused
 * (the default), 2 = two kernels; 0, round 4's banded form, was removed in ABI 8: hipErrorInvalidValue).
 * The two forms agree to bf16 rounding (some f32 sums are ordered differently). */
int vit_sdpa_bwd_variant(int v);

/* torch.nn.functional.cross_entropy(outputs, targets) mean (VIT:140) and its gradient. */
int vit_cross_entropy_fwd(int B, int C, const float* logits, int64_t ld, const int64_t* target, float* row_lse,
                          float* row_loss, float* loss, void* stream);
int vit_cross_entropy_bwd(int dtype_out, int B, int C, const float* logits, int64_t ld, const int64_t* target,
                          const float* row_lse, const float* grad_loss, void* dlogits, int64_t ldd, void* stream);

/* Validation metrics of one batch (VIT:167-204's validate: F.cross_entropy(outputs, targets).item(),
 * outputs.max(1), predicted.eq(targets).sum().item() per batch) accumulated on the device: f32 logits
 * [B][C] (row stride ld), int64 targets in [0, C).  Adds into acc[6] (f64; the caller zeroes it with
 * vit_zero): [0] the batch's mean loss, [1] the sum of row losses, [2] rows whose target has rank 0
 * (first-maximum argmax == target), [3] rows with rank < topk, [4] B, [5] 1, where rank = classes with a
 * larger logit + classes with an equal logit and a smaller index.  A row whose log-sum-exp is not finite
 * adds its non-finite loss and counts as wrong.  row_ws >= 2*B floats.  Fixed-order sums, no atomics:
 * bitwise reproducible; successive calls on one stream accumulate. */
int vit_eval_metrics(int B, int C, const float* logits, int64_t ld, const int64_t* target, int topk, float* row_ws,
                     double* acc, void* stream);

/* torch.optim.SGD(lr, momentum, weight_decay).step() over all parameters in one
 * launch (VIT:143-144, VIT:294-299).  tensors: {float* p; const float* g; float* buf;
 * bf16* shadow; int64 n}[], chunks: {int tensor; int pad; int64 start}[] (4096 elems). */
int vit_sgd_step(const void* tensors, const void* chunks, int nchunks, const float* lr, float momentum,
                 float weight_decay, void* stream);
int vit_sgd_chunk_size(void);
int vit_sgd_tensor_bytes(void);
int vit_sgd_chunk_bytes(void);

/* DoRALayer.weight (NEWP:447-463): W[out,in] = (m * (D + (B@A)s) / (||.||_col + 1e-8))^T,
 * and its backward (dm, dA, dB) for AdamW (NEWP:1000-1001).  noise (nullable, [in,out] like D):
 * DoRALayer.forward's train-mode dropout of delta_D (NEWP:465-481), (B@A)s * noise with
 * noise = keep-mask / (1 - p); the backward masks the delta_D gradient the same way.
 * All three entry points return hipErrorInvalidValue, before anything is queued, for in <= 0,
 * out <= 0, r outside 1..64 (LoRA's range) or a null operand; only noise, the forward's nu and
 * slabs may be null. */
int vit_dora_weight_fwd(int in, int out, int r, const float* m, const float* A, const float* B, const float* D,
                        float scaling, const float* noise, float* W, float* nu, float* DnT_ws, float* colsq_ws,
                        void* stream);
int vit_dora_weight_bwd(int in, int out, int r, const float* m, const float* A, const float* B, const float* gW,
                        const float* DnT, float scaling, const float* nu, float* dm, float* dA, float* dB,
                        float* sdDnT_ws, const float* noise, void* stream);
/* ABI 7: the same with a split-K slab workspace (nullptr / 0 = unsplit), and the split-K GEMM it uses:
 * C [M][N] contiguous f32 = sum_r P(i,r) Q(j,r) in r-chunks of >= 128 summed in chunk order
 * (deterministic).  Slab contract (both functions): the split s is the largest with s <= 256 / tiles,
 * s <= R / 128 and s * M * N <= slab_floats, and the kernel writes at most s slabs of M * N floats
 * (chunks of ceil(R / s) rows); s < 2 runs unsplit.  DoRA's factor GEMMs are [in x r] and [r x out],
 * so 2 * max(in, out) * r floats allow a split of 2 and 2 * 256 * 1024 (the Python callers) their
 * full split at C3's in = out = 1024, r = 32. */
int vit_dora_weight_bwd_ws(int in, int out, int r, const float* m, const float* A, const float* B, const float* gW,
                           const float* DnT, float scaling, const float* nu, float* dm, float* dA, float* dB,
                           float* sdDnT_ws, float* slabs, int64_t slab_floats, const float* noise, void* stream);
int vit_gemm_splitk(int p_layout, int q_layout, int M, int N, int R, const float* P, int64_t ldp, const float* Q,
                    int64_t ldq, float* C, float* slabs, int64_t slab_floats, void* stream);
/* LoRALayer.weight (NEWP:330-332) and its backward (additive to ABI 10; csrc/lora.hip):
 *   W[i][j] = W0[i][j] + scaling * sum_k B[i][k] A[k][j]     W0, W [n, n], B [n, r], A [r, n], f32 row-major.
 * The reference adds B @ A ([in, out]) to W0 ([out, in]) without a transpose: the property exists only for
 * in == out = n and is not the weight LoRALayer.forward applies; nn.MultiheadAttention reads out_proj.weight
 * (quirk Q5), so on the CLIP-HBA path it is the weight that trains.  One launch; 1 <= r <= 64, any n >= 1
 * (16-byte loads / stores along j when n % 4 == 0 and W0, A, W are 16-byte aligned, scalar otherwise).
 * Backward, gW = dL/dW [n, n]:  dA [r, n] = scaling * B^T gW,  dB [n, r] = scaling * gW A^T, both overwritten
 * (dW0 = gW is the caller's).  gW is read once in 64 x 64 tiles; each tile's shares of dA and dB go to ws and
 * a second launch sums them in tile order: no atomics, the same bits on every run.  1 <= n <= 16384;
 * ws holds vit_lora_weight_bwd_ws_floats(n, r) = 2 * ceil(n / 64) * r * n floats (host-only query, 0 for
 * arguments the backward rejects) and is 16-byte aligned.  hipErrorInvalidValue for r or n out of range. */
int vit_lora_weight_fwd(int n, int r, const float* W0, const float* A, const float* B, float scaling, float* W,
                        void* stream);
int vit_lora_weight_bwd(int n, int r, const float* A, const float* B, const float* gW, float scaling, float* dA,
                        float* dB, float* ws, void* stream);
int vit_lora_weight_bwd_ws_floats(int n, int r);
/* torch.optim.AdamW step (NEWP:1181, NEWP:1001): tensors {float* p; const float* g; float* exp_avg;
 * float* exp_avg_sq; bf16* shadow (or null); int64 n; const float* coef}[] where coef points at
 * the tensor's {step_size, bc2_sqrt, decay, 0} in device memory: step_size = lr / (1 - beta1^step),
 * bc2_sqrt = sqrt(1 - beta2^step) for that tensor's own state['step'] (so a load_state_dict
 * resume, NEWP:1189-1195, continues the bias correction) and decay = 1 - lr * weight_decay of the
 * tensor's group.  The table is fixed across steps (only the coefficients change), so a captured
 * graph can replay it under a changing lr; chunks as vit_sgd_step.  (ABI 6: decay moved from a
 * scalar argument into coef.) */
int vit_adamw_step(const void* tensors, const void* chunks, int nchunks, float beta1, float beta2, float eps,
                   void* stream);
int vit_adamw_tensor_bytes(void);

/* CLIP-HBA forward/loss around the towers (NEWP:287-304 -> clip_model(image, prompts, pos_embedding),
 * the CLIP-HBA fork, external; OpenAI-CLIP semantics assumed):
 *   token_embed   x[s*L+t] = table[tokens[s*L+t]] + pos[t]         (token_embedding + positional_embedding)
 *   gather_rows   dst[i] = src[idx[i]]  (text EOT pooling x[arange, text.argmax(-1)], CLS rows)
 *   scatter_rows  dst[idx[i]] = src[i]  (their backward; dst zeroed by the caller)
 *   rownorm       y = exp(*log_scale) x / ||x|| (feature normalisation; log_scale null = 1), and backward
 *   mse           nn.MSELoss() mean (NEWP:994, CBASE criterion) and its gradient (grad_loss null = 1)
 * token_embed needs D % 4 == 0; ids outside [0, vocab) read the table's first / last row; 16-byte accesses when
 * table, pos and x are 16-byte aligned, one float per lane otherwise. */
int vit_token_embed(int rows, int L, int D, int vocab, const int64_t* tokens, const float* table, const float* pos,
                    float* x, void* stream);
int vit_gather_rows(int n, int D, const float* src, int64_t ld_src, const int64_t* idx, float* dst, int64_t ld_dst,
                    void* stream);
int vit_scatter_rows(int n, int D, const float* src, int64_t ld_src, const int64_t* idx, float* dst, int64_t ld_dst,
                     void* stream);
/* gather_blocks  dst[i] = src[idx[i]] for whole token blocks (the cached frozen-prefix rows of a batch,
 * VisualPrefixCache.take): rows of row_elems floats, contiguous in src and dst (row stride = row_elems),
 * row_elems % 4 == 0, src and dst 16-byte aligned; idx is int64 in device memory and must have been checked
 * against the rows of src by the caller (the kernel does not know their number).  Additive export, ABI 10. */
int vit_gather_blocks(int n, int64_t row_elems, const float* src, const int64_t* idx, float* dst, void* stream);
int vit_rownorm_fwd(int n, int D, const float* x, const float* log_scale, float* y, float* rnorm, void* stream);
int vit_rownorm_bwd(int n, int D, const float* x, const float* dy, const float* rnorm, const float* log_scale,
                    float* dx, void* stream);
int vit_mse_fwd(int n, const float* pred, const float* target, float* loss, void* stream);
int vit_mse_bwd(int n, const float* pred, const float* target, const float* grad_loss, float* dpred, void* stream);

/* ImageNet input transforms on the GPU (VIT:32-46, MEAS:152-158): RandomResizedCrop /
 * Resize+CenterCrop with Pillow's 8-bit bilinear resampling (bit-exact), horizontal flip, ToTensor and
 * Normalize, over a ragged batch of decoded RGB uint8 images in device memory.  params = device int64
 * [B][12] (see image.hip); coeff_ws >= vit_image_coeff_bytes(B, S, kmax) bytes; out f32 [B][3][S][S]. */
int vit_image_coeff_bytes(int B, int S, int kmax);
int vit_image_transform(int B, int S, const uint8_t* src, const int64_t* params, int kmax, int max_rows,
                        int* coeff_ws, uint8_t* tmp_ws, float* out, const float* norm6, void* stream);

/* helpers */
/* round-to-nearest-even cast; 4 elements per lane when x is 16-byte and y 8-byte aligned, else one */
int vit_cast_f32_bf16(const float* x, void* y, int64_t n, void* stream);
int vit_zero(void* p, int64_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_HIP_H */
