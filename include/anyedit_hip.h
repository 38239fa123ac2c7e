/* libanyedit_hip.so — C ABI of the MI355X (gfx950) AnyEdit denoising hot path.
 *
 * The reference (DCDmllm/AnyEdit) has NO C ABI on this path: its boundaries are Python callables that it already
 * swaps at exactly these points: the attention-class registry ldm/modules/attention.py:247-256,
 * the fused-op call xformers.ops.memory_efficient_attention at attention.py:222-233, the layer factories
 * conv_nd/linear/normalization at ldm/modules/diffusionmodules/util.py:202-238, and — the one real FFI in the tree —
 * pybind11 `_C.ms_deform_attn_forward` (GroundingDINO/.../csrc/vision.cpp:53-56).  Each entry point below names the
 * reference interface it replaces.  INTEGRATION.md shows the reference-side ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = error (AE_ERR_*); ae_last_error() returns the message (thread local);
 *   - never throws, never allocates caller-visible memory, never synchronises the device;
 *   - all data pointers are DEVICE pointers borrowed for the duration of the call; inputs are not mutated;
 *   - the last argument is the hipStream_t (as void*) the work is enqueued on (graph-capture safe);
 *   - "bf16" buffers are raw bfloat16 bits (uint16); activations are channels-last: [B, H*W, C] / [rows, C].
 */
#ifndef ANYEDIT_HIP_H
#define ANYEDIT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define AE_OK 0
#define AE_ERR_ARG (-1)
#define AE_ERR_LAUNCH (-2)
#define AE_ERR_UNSUPPORTED (-3)

/* epilogue selector of ae_gemm_bf16 */
#define AE_EPI_NONE 0  /* out = acc + bias + addvec (+ residual)                         */
#define AE_EPI_GELU 1  /* out = gelu_erf(acc + bias) (+ residual)   (SAM MLPBlock, common.py:13-27) */
#define AE_EPI_GEGLU 2 /* out[:, j] = a_j * gelu_erf(g_j), W rows interleaved 16 a / 16 g (attention.py:49-58) */
#define AE_EPI_SILU 3  /* out = silu(acc + bias)                    (time_embed, openaimodel.py:526-531) */
#define AE_EPI_RELU 4  /* out = max(acc + bias, 0) (+ residual)     (SAM decoder MLPs, mask_decoder.py:154-176, transformer.py:122) */

int ae_version(void);
const char* ae_last_error(void);
int ae_device_arch(char* buf, int n);                          /* e.g. "gfx950:sramecc+:xnack-" */
int ae_device_info(int* cus, long* hbm_bytes, int* clock_khz);

/* nn.Linear / 1x1 nn.Conv2d on channels-last rows (util.py:202-238 factories; attention.py:154-161 to_q/to_k/to_v/to_out,
 * :49-76 FeedForward/GEGLU, :296-318 proj_in/proj_out; openaimodel.py:233-240 skip 1x1, :526-531 time_embed, :214-219 emb_layers).
 *   C[M,N] = epi(A[M,K] @ W[N,K]^T); A2 != NULL: columns [Ksplit,K) of A come from A2 (skip-concat, openaimodel.py:780).
 *   K % 8 == 0, N % 4 == 0, rows 16-byte aligned.  addvec: fp32 [M/rows_per_batch, N] with row stride addvec_ld (0 = N).
 *   out_f32: C is fp32.
 *   colstats (optional, fp32 [ceil(M/32)][N][2]): per-channel (sum, sum of squares) of the stored bf16 output over each 32-row
 *   slab, produced by the GEMM's own epilogue where the tile plan allows (one extra pass over the L2-resident output otherwise):
 *   hand it to ae_groupnorm_nhwc_bf16 and the GroupNorm that consumes C (util.py:217-219) runs without its statistics pass.  */
int ae_gemm_bf16(const void* A, long lda, const void* A2, long lda2, int Ksplit, const void* W, long ldw, void* C, long ldc,
                 int M, int N, int K, const float* bias, const void* residual, long ldr, const float* addvec, long addvec_ld,
                 int rows_per_batch, int epilogue, int out_f32, float* colstats, void* stream);

/* Row-panel GEMM for the short-K (K = 320) Linear layers of the 64x64 UNet level, with the LayerNorm of BasicTransformerBlock
 * (attention.py:263-265, 271-275: norm1 -> to_q|k|v, norm2 -> to_q, norm3 -> GEGLU projection) optionally fused in front:
 *   C[M,N] = epi( LN(A)[M,K] @ W[N,K]^T + bias (+ residual) ),  ln_gamma == NULL: no LayerNorm.  epilogue: AE_EPI_NONE | AE_EPI_GEGLU.
 * A wave keeps 48 rows of A in registers for the whole launch (normalised there), W streams through an LDS ring by LDS-DMA.
 * ae_ln_gemm_supported() tells whether the kernel covers a shape (K == 320, N % 64 == 0, N <= 2560, M >= 192 * 192 rows: one 192-row block per CU); callers fall back to
 * ae_layernorm_bf16 + ae_gemm_bf16 otherwise.  A, W rows and C, residual rows 16-byte aligned.                                   */
int ae_ln_gemm_supported(int M, int N, int K, int epilogue);
int ae_ln_gemm_bf16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias,
                    const void* residual, long ldr, const float* ln_gamma, const float* ln_beta, float ln_eps, int epilogue,
                    float* colstats /* as for ae_gemm_bf16; NULL = none */, void* stream);

/* LayerNorm folded into the projection that consumes it (BasicTransformerBlock, attention.py:263-265, 271-275: norm1 -> to_q|k|v,
 * norm2 -> to_q, norm3 -> GEGLU projection) — at every channel width since round 5: 640 / 1280 on the tiled kernel's fold epilogues, 320 (the
 * shapes ae_ln_gemm_supported() covers) on the row-panel kernel's own fold forms, which replace its LayerNorm prologue (AE_RP_FOLD=0: off):
 *   LN(x) W^T + b = rstd_m (x W'^T - mu_m s) + c,   W' = W diag(gamma),  s[n] = sum_k W'[n][k] (over the bf16 values of W'),  c = W beta + b.
 * The GEMM that PRODUCES x (proj_in :296-318, attn1 / attn2 to_out :159-161) emits, next to its bf16 output, one (sum, sum of squares)
 * pair per row and 64-column slice (rowstats_out: fp32 [M][N / 64][2], statistics of the stored bf16 values); the GEMM that consumes
 * LN(x) multiplies the UN-normalised rows by W' and applies the two per-row scalars and the two per-column vectors in its epilogue
 * (ln_stats = the producer's rowstats_out with ln_parts = its N / 64 slices per row; ln_colsum = s; bias = c; the normalised width is K).
 * No LayerNorm launch, no read of x and write of LN(x) for it.  Exactly one of rowstats_out / ln_stats is non-NULL.  epilogue: AE_EPI_NONE
 * (+ residual) when emitting; AE_EPI_NONE or AE_EPI_GEGLU when consuming.  bf16 output, N % 64 == 0, 16-byte aligned rows.
 * ae_gemm_ln_plan(M, N, K, epilogue, mode) tells whether the kernel ae_gemm_ln_bf16 would run for this shape carries the epilogue
 * (mode 1 emit, 2 consume): 1 yes, 0 no — callers keep ae_layernorm_bf16 + ae_gemm_bf16 otherwise.                                    */
int ae_gemm_ln_plan(int M, int N, int K, int epilogue, int mode);
int ae_gemm_ln_bf16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias,
                    const void* residual, long ldr, int epilogue, float* rowstats_out, const float* ln_stats, int ln_parts,
                    const float* ln_colsum, float ln_eps, void* stream);

/* Fused feed-forward of a BasicTransformerBlock at the 64x64 UNet level (round 6; ldm/modules/attention.py:49-76 FeedForward / GEGLU behind norm3 of
 * BasicTransformerBlock._forward :271-275, `x = self.ff(self.norm3(x)) + x`, and — optionally — SpatialTransformer.proj_out + its residual behind the
 * block, :337-340) — ONE launch for LayerNorm -> GEGLU projection -> exact-erf gate -> ff2 (+ bias, + residual) [-> proj_out (+ bias, + residual3)];
 * the [M, H] gated hidden activation stays in registers (it was 126 MB written and re-read at UNet batch 12), and with W3 so does the block's output:
 *   F[M,C] = ( a .* gelu(g) ) W2^T + b2 (+ residual),   [a | g] = LayerNorm(X; gamma, beta, eps) W1^T + b1,   C = 320;
 *   Y = F (W3 == NULL)   or   Y[M,C] = bf16(F) W3^T + b3 (+ residual3).
 *   X, Y, residual, residual3 bf16 rows (16-byte aligned, strides % 8 == 0; Y aliases neither X nor residual3); W1 bf16 [2H, C] and b1 fp32 [2H] in the
 *   AE_EPI_GEGLU row order (16 'a' rows then their 16 gate rows); W2img bf16 [H / 32][C][32]: ff2's weight as the kernel's LDS images (row order, k
 *   permutation and 16-byte piece rotation as the header of csrc/ff_fused.hip states them; ops.pack_ff2_fused builds it once per weight version); b2 fp32
 *   [C] or NULL; W3 bf16 [C, C] row-major (ldw3) or NULL, b3 fp32 [C] or NULL; colstats: as for ae_gemm_bf16 (statistics of Y for the GroupNorm that
 *   consumes it; with W3 only), NULL = none.
 * ae_ff_fused_supported(M, C, H): 1 where the kernel covers the shape (C == 320, H % 64 == 0, H <= 1280, M >= 192 * 192 rows: one 192-row block per
 * CU), 0 otherwise — callers then run ae_gemm_ln_bf16 / ae_ln_gemm_bf16 (GEGLU) + ae_gemm_bf16 (+ ae_ln_gemm_bf16 for proj_out).  AE_FF_FUSED=0
 * answers 0 everywhere (A/B).                                                                                                                     */
int ae_ff_fused_supported(int M, int C, int H);
int ae_ff_fused_bf16(const void* X, long ldx, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* W1, long ldw1, const float* b1,
                     const void* W2img, const float* b2, const void* residual, long ldr, const void* W3, long ldw3, const float* b3,
                     const void* residual3, long ldr3, float* colstats, void* Y, long ldy, int M, int C, int H, void* stream);

/* 3x3 convolution, padding 1, as implicit GEMM (ResBlock in/out convs openaimodel.py:200-231, stem :536-542, head :726-730,
 * Downsample stride 2 :157-159, Upsample nearest-x2 + conv :108-118 via upsample2x=1).
 *   x [B,H,W,Cin] bf16 channels-last (Cin % 8 == 0), w [Cout, 9*CinPad] bf16 packed (ky,kx,cin) with CinPad = Cin
 *   rounded up to 64 (zero filled), y [B,Ho,Wo,Cout];
 *   addvec fp32 [B,Cout] (time-embedding add, openaimodel.py:262-272), residual bf16 [B,Ho,Wo,Cout] (skip, :274).
 *   workspace: NULL or ae_conv3x3_workspace_floats(...) fp32 elements (0 = not needed): enables split-K for the small-M,
 *   huge-K layers (8x8 / 16x16 latents) that cannot fill 256 CUs with output tiles alone.
 *   k_order: 0 = w packed (ky,kx,cin) as above; 1 = w packed (cin / 64, ky, kx, cin % 64) — the nine taps of a 64-channel chunk
 *   in consecutive K tiles, so a block re-reads its activation window from L2 (Cin % 64 == 0, no upsampling); same result.   */
long ae_conv3x3_workspace_floats(int B, int H, int W, int Cin, int Cout, int stride, int upsample2x);
int ae_conv3x3_bf16(const void* x, const void* w, const float* bias, const float* addvec, long addvec_ld, const void* residual,
                    void* y, int B, int H, int W, int Cin, int Cout, int stride, int upsample2x, int out_f32, float* workspace,
                    float* colstats /* as for ae_gemm_bf16 (M = B*Ho*Wo, N = Cout); NULL = none */, int k_order, void* stream);

/* Upsample (openaimodel.py:108-118: F.interpolate(scale_factor=2, mode="nearest") followed by the 3x3 conv) as FOUR 2x2 convolutions on the
 * low-resolution input: output pixel (2y+py, 2x+px) reads input rows {y-1, y} (py = 0) or {y, y+1} (py = 1), columns likewise, and the 3x3
 * taps that land on the same input pixel are summed at pack time — 4/9 of the multiply-adds of ae_conv3x3_bf16(..., upsample2x = 1), the same
 * function up to the rounding of the summed bf16 weights.
 *   x [B,H,W,Cin] bf16 channels-last (Cin % 64 == 0); y [B,2H,2W,Cout] bf16 (Cout % 8 == 0); bias fp32 [Cout] or NULL;
 *   w4 [4][Cout][4*Cin] bf16: set p = 2*py + px, K ordered (tap t = 2*i + j, cin) with
 *       w4[p][co][t*Cin + ci] = sum_{ky in S(py,i)} sum_{kx in S(px,j)} w[co][ci][ky][kx],   S(0,0)={0} S(0,1)={1,2} S(1,0)={0,1} S(1,1)={2}
 *   (summed in fp32 from the fp32 master weights, then rounded to bf16 once);
 *   colstats: as for ae_conv3x3_bf16, for the OUTPUT map ([B*4*H*W/32][Cout][2]; needs H*W % 32 == 0), or NULL.                       */
int ae_conv3x3_up2_bf16(const void* x, const void* w4, const float* bias, void* y, int B, int H, int W, int Cin, int Cout,
                        float* colstats, void* stream);

/* Launch plans: what the three entry points above would run for the given scalar arguments — the library's own selection code, run without
 * launching.  Host only: no GPU call, callable without a device.  0 and plan[0 .. AE_PLAN_INTS) filled, or the error the launch would return.
 *   plan[0..11]  the template arguments of the gemm_kernel instantiation: BM, BN, AMODE (0 dense, 1 conv), WAVES_M, WAVES_N, GLDS, WAVES_K, STAGES, CS,
 *                LAB, WA, XE (as the kernel's demangled name spells them);
 *   plan[12..15] grid, threads per block, dynamic LDS bytes, split-K factor;
 *   plan[16..17] 1 where the split-K reduce / the stand-alone column-statistics kernel follows;
 *   plan[18]     dense, ln_mode != 0 only: 1 = the row-panel kernel's fold forms take the launch instead (plan[0..17] are then zero).
 * Arguments that are pointers at the launch are flags here (workspace / colstats: given or not); every pointer counts as well aligned.
 *   ae_gemm_plan: Ksplit 0 = one source; ln_mode 0 = ae_gemm_bf16, 1 / 2 = ae_gemm_ln_bf16 emitting / consuming row statistics.                */
#define AE_PLAN_INTS 19
int ae_gemm_plan(int M, int N, int K, int epilogue, int Ksplit, int out_f32, int colstats, int ln_mode, int* plan);
int ae_conv3x3_plan(int B, int H, int W, int Cin, int Cout, int stride, int upsample2x, int out_f32, int workspace, int colstats, int k_order,
                    int* plan);
int ae_conv3x3_up2_plan(int B, int H, int W, int Cin, int Cout, int colstats, int* plan);

/* GroupNorm32 (+SiLU) (util.py:217-219 eps 1e-5; attention.py:88-89 eps 1e-6); input may be the channel-concat [x | x2].
 * workspace: fp32, ae_groupnorm_workspace_floats(B,HW,C,groups) elements.  act: 0 none, 1 SiLU.
 * counters: optional int32[B], ZERO on entry and zero again on exit, not shared with a launch running concurrently on another
 * stream: the last partial-sum block of each sample then runs the statistics fold itself (two launches instead of three, same
 * fixed summation order, bit-identical result).  NULL keeps the stand-alone finalize launch.  The tail is OFF unless AE_GN_TAIL=1:
 * measured 3 ms per UNet step slower on MI355X (every block's device-scope release is an L2 write-back).
 * stat_out: optional fp32 [B][groups][2] (mean, rstd) kept for ae_groupnorm_bwd_nhwc_bf16.
 * colstats / colstats2: optional per-channel slab statistics of x / x2 as written by the kernels that PRODUCED them (the `colstats`
 * output of ae_gemm_bf16 / ae_ln_gemm_bf16 / ae_conv3x3_bf16: [B*HW/32][C1][2] and [B*HW/32][C-C1][2]; HW % 32 == 0).  With them the
 * statistics pass over the activation is skipped: one block per (sample, group) folds the slab sums, then the apply launch runs.    */
int ae_groupnorm_rows_per_chunk(int HW, int C);
long ae_groupnorm_workspace_floats(int B, int HW, int C, int groups);
int ae_groupnorm_nhwc_bf16(const void* x, const void* x2, int C1, const float* gamma, const float* beta, void* y, int B, int HW,
                           int C, int groups, float eps, int act, float* workspace, int* counters, float* stat_out,
                           const float* colstats, const float* colstats2, void* stream);

/* nn.LayerNorm over the last dim (attention.py:263-265 eps 1e-5; SAM image_encoder.py:166-182 / common.py:30-43 eps 1e-6). */
int ae_layernorm_bf16(const void* x, const float* gamma, const float* beta, void* y, int M, int C, float eps, void* stream);

/* Fused attention forward = CrossAttention.forward core (attention.py:171-193) / xformers.ops.memory_efficient_attention
 * (attention.py:233) / SAM Attention.forward core (image_encoder.py:231-238).  q/k/v/out addressed by element strides
 * (batch, head, row); head_dim D in {8,16,32,40,48,64,80,96,128,160}.  rel_h/rel_w: optional fp32 [B*H,Nq,kH] / [B*H,Nq,kW]
 * decomposed relative-position bias (image_encoder.py:325-361), Nk == kH*kW.  key_mask: optional uint8 [B,Nk], 0 = masked
 * (attention.py:183-187).  out_scale: optional fp32 [B]; accumulate != 0: out += out_scale[b] * result (decoupled adapter
 * attention, ip_adapter/attention_processor.py:141-173 — the shape template of AnySD's expert K/V).
 * k2/v2 (optional, head_dim <= 96 or 160): a second key/value segment with its own softmax fused into the same launch:
 * out = Attn(q,k,v) + scale2[b] * Attn(q,k2,v2).                                                                           */
int ae_attn_fwd_bf16(const void* q, const void* k, const void* v, void* out, int B, int H, int Nq, int Nk, int D,
                     long q_sb, long q_sh, long q_sn, long k_sb, long k_sh, long k_sn, long v_sb, long v_sh, long v_sn,
                     long o_sb, long o_sh, long o_sn, float scale, const float* rel_h, const float* rel_w, int kH, int kW,
                     const unsigned char* key_mask, const float* out_scale, int accumulate, const void* k2, const void* v2,
                     int Nk2, long k2_sb, long k2_sh, long k2_sn, long v2_sb, long v2_sh, long v2_sn, const float* scale2,
                     float* lse, float* lse2, void* stream);
/* fp8 (OCP e4m3) attention forward (BASELINE.json configs[4], SAM image-encoder attention image_encoder.py:224-240, rel-pos bias
 * :325-361): Q, K, V and the probabilities are e4m3 operands of v_mfma_scale_f32_32x32x64_f8f6f4, logits / softmax / accumulation
 * fp32.  Scales: per (batch, head) amax of q, k, v measured on the fly (k: float scale folded into q; q and v: powers of two that
 * ride in the MFMA's E8M0 scale operand / the final normalisation).  head_dim % 8 == 0, <= 88.  rel_h / rel_w (optional): the
 * decomposed bias for key grids with kW == 64 (global attention on 64 x 64 tokens).  `workspace`: device scratch of at least
 * ae_attn_fp8_workspace_bytes(...) bytes, 256-byte aligned (quantised operands live there for the duration of the call).         */
long ae_attn_fp8_workspace_bytes(int B, int H, int Nq, int Nk, int D);
int ae_attn_fwd_fp8(const void* q, const void* k, const void* v, void* out, int B, int H, int Nq, int Nk, int D, long q_sb, long q_sh,
                    long q_sn, long k_sb, long k_sh, long k_sn, long v_sb, long v_sh, long v_sn, long o_sb, long o_sh, long o_sn,
                    float scale, const float* rel_h, const float* rel_w, int kH, int kW, void* workspace, long workspace_bytes,
                    void* stream);
/* lse / lse2 (optional, fp32 [B,H,Nq]): log2-domain log-sum-exp of the first / second segment's softmax, kept for
 * ae_attn_bwd_bf16.
 *
 * ---- training step (train.py:625-710; the in-tree restatement is LatentDiffusion.p_losses,
 * ddpm.py:889-932).  The UNet is frozen: layers are differentiated w.r.t. activations only; Linear / conv data-gradients reuse
 * ae_gemm_bf16 / ae_conv3x3_bf16 with transposed / rotated packed weights (upsample2x = 2: zero-insert gather = adjoint of the
 * stride-2 Downsample conv, openaimodel.py:157-159).
 *
 * Attention backward for one key/value segment (autograd of attention.py:171-193): delta [B,H,Nq] fp32 is an OUTPUT
 * (rowsum(P o dP) with the un-scaled dout; its sum over heads and rows is d/d out_scale[b]).  dk, dv may both be NULL.
 * out (optional, layout of dout): the forward output of THIS segment alone (no second segment, no out_scale folded in): delta is
 * then rowsum(dout o out), computed up front, and the dQ pass keeps one accumulator set instead of two.
 * workspace (optional): NULL or ae_attn_bwd_workspace_floats(...) fp32 elements, 16-byte aligned (0 = not needed): lets the dK / dV
 * pass of a FEW-key segment (cross-attention: 78 text or 16 adapter tokens against 4096 queries is only B H blocks) cut its query
 * tiles across blocks — fp32 partials, summed in split order by a second launch (deterministic).  Without it every shape runs
 * the one-block-per-128-keys pass.                                                                                             */
long ae_attn_bwd_workspace_floats(int B, int H, int Nq, int Nk, int D);
int ae_attn_bwd_bf16(const void* q, const void* k, const void* v, const void* dout, const void* out, const float* lse, float* delta, void* dq,
                     void* dk, void* dv, int B, int H, int Nq, int Nk, int D, long q_sb, long q_sh, long q_sn, long k_sb,
                     long k_sh, long k_sn, long v_sb, long v_sh, long v_sn, long o_sb, long o_sh, long o_sn, long dq_sb,
                     long dq_sh, long dq_sn, long dk_sb, long dk_sh, long dk_sn, long dv_sb, long dv_sh, long dv_sn,
                     float scale, const float* out_scale, int accumulate_dq, float* workspace, void* stream);
/* GroupNorm(+SiLU) backward w.r.t. the input(s) (autograd of util.py:217-219 + nn.SiLU); dx2 receives channels [C1, C).
 * counters: as for ae_groupnorm_nhwc_bf16.  stat_in: optional (mean, rstd) saved by the forward launch — the statistics pass over
 * x is skipped (three launches instead of five) and the gradient uses exactly the statistics the forward normalised with.      */
long ae_groupnorm_bwd_workspace_floats(int B, int HW, int C, int groups);
int ae_groupnorm_bwd_nhwc_bf16(const void* x, const void* x2, int C1, const float* gamma, const float* beta, const void* dy,
                               void* dx, void* dx2, int B, int HW, int C, int groups, float eps, int act, float* workspace,
                               int* counters, const float* stat_in, int accumulate, void* stream);
/* accumulate (GroupNorm: bit 0 -> dx, bit 1 -> dx2; LayerNorm: 0 / 1): the gradient is ADDED to what the output tensor already
 * holds (fp32 add, one rounding) — a tensor with several consumers collects its gradient without a separate ae_add_bf16 launch.
 * LayerNorm backward w.r.t. the input; row_stat (optional fp32 [M,2]) receives (mean, rstd) for the parameter gradients.    */
int ae_layernorm_bwd_bf16(const void* x, const float* gamma, const void* dy, void* dx, float* row_stat, int M, int C, float eps,
                          int accumulate, void* stream);
int ae_layernorm_param_grad_f32(const void* x, const void* dy, const float* row_stat, float* dgamma, float* dbeta, int M, int C,
                                void* stream);
/* y = a + b (gradient accumulation where a layer's input fans out).                                                          */
int ae_add_bf16(const void* a, const void* b, void* y, long n, void* stream);
/* y = a + alpha * b, bf16 (ControlNet residual injection: hs.pop() + scale * control.pop(), cldm.py:40-41, 336-338).          */
int ae_axpy_bf16(const void* a, const void* b, float alpha, void* y, long n, void* stream);
/* GEGLU un-fused for training (attention.py:49-57): h = [a | g] [M, 2F] -> y = a * gelu(g); backward -> dh.                   */
int ae_geglu_fwd_bf16(const void* h, void* y, long M, int F, void* stream);
int ae_geglu_bwd_bf16(const void* h, const void* dy, void* dh, long M, int F, void* stream);
/* adjoint of the nearest-x2 upsample (openaimodel.py:108-118): x [B,2H,2W,C] -> y [B,H,W,C] = 2x2 block sums.                  */
int ae_sumpool2x2_bf16(const void* x, void* y, int B, int H, int W, int C, void* stream);
/* out[n] = sum_m x[m, n] (bias gradient of the small trainable Linear layers).                                               */
int ae_colsum_bf16_f32(const void* x, float* out, int M, int N, long ld, void* stream);
/* d/dpred mean((pred - target)^2) * loss_scale (train.py:696).                                                               */
int ae_mse_grad_f32(const float* pred, const float* target, float* out, long n, float loss_scale, void* stream);
/* torch.optim.AdamW step on fp32 state (train.py:536-541); step counts from 1; grad is multiplied by grad_scale first.       */
int ae_adamw_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1, float beta2,
                 float eps, float weight_decay, int step, float grad_scale, void* stream);
/* out[r] = sum_j x[r, j] (fp32, fixed order): gate gradient = sum over heads and rows of the adapter segment's delta.     */
int ae_rowsum_f32(const float* x, float* out, int rows, long n, void* stream);
/* dst[code[b]] += src[b] in batch order (task-embedding gradient rows).                                                      */
int ae_scatter_add_rows_f32(const float* src, const int* code, float* dst, int B, int D, int n_rows, void* stream);
/* Backward of the task-router gate value w.r.t. the task embedding (ae_task_gate).                                           */
int ae_task_gate_bwd(const float* probs, const int* top1, const float* dgate, const float* Wg, int B, int Dt, int E, float* dte,
                     void* stream);
/* Gradient of the same gate value w.r.t. the router itself: dWg[e,:] = sum_b dlogit[b,e] task_embs[edit_code[b]],
 * dbg[e] = sum_b dlogit[b,e] (dbg may be NULL); samples summed in index order.  The router is a trainable of the adapter
 * group in our AnySD spec (train.py:483-485 optimises the adapter modules it lives in).                          */
int ae_task_gate_wgrad(const float* probs, const int* top1, const float* dgate, const float* task_emb, const long* edit_code, int B,
                       int n_tasks, int Dt, int E, float* dWg, float* dbg, void* stream);

/* AnySD per-expert adapter K/V projection of the training step, grouped over the samples of a batch (our spec; the
 * reference trains `adapter_modules` at train.py:410-424, 536-541).  x: [B*T, Dc] bf16 image-prompt rows (T <= 8 per sample),
 * W: [E, N, Dc] fp32 masters (rounded to bf16 in registers), experts: [B] int32 routed expert per sample.
 *   fwd    y[b*T+t, n]  = sum_k x[b*T+t, k] * W[experts[b], n, k]                              (bf16 out)
 *   dgrad  dx[b*T+t, k] = sum_n dy[b*T+t, n] * W[experts[b], n, k]                             (bf16 out, fixed summation order;
 *          partial: ae_expert_kv_dgrad_slices(N)*B*T*Dc floats of scratch)
 *   wgrad  dW[e, n, k]  = sum_{b: experts[b] == e} sum_t dy[b*T+t, n] * x[b*T+t, k]            (fp32, every expert written)      */
int ae_expert_kv_fwd(const void* x, const float* W, const int* experts, void* y, int B, int T, int N, int Dc, int E, void* stream);
int ae_expert_kv_dgrad_slices(int N);
int ae_expert_kv_dgrad(const void* dy, const float* W, const int* experts, void* dx, int B, int T, int N, int Dc, int E, float* partial,
                       void* stream);
int ae_expert_kv_wgrad(const void* dy, const void* x, const int* experts, float* dW, int B, int T, int N, int Dc, int E, void* stream);

/* out[b,y,x] = in[b,x,y], inner dim zero-padded to Xpad: NCHW <-> channels-last at the UNet boundary
 * ('b c h w -> b (h w) c', attention.py:329,337).                                                                           */
int ae_transpose_last2(const void* in, void* out, int B, int X, int Y, int Xpad, int in_bf16, int out_bf16, void* stream);
/* th.cat([h, hs.pop()], dim=1) (openaimodel.py:780) on channels-last rows.                                                   */
int ae_concat_channels_bf16(const void* a, int Ca, const void* b, int Cb, void* y, long rows, void* stream);
/* im2col of the UNet's stem conv (3x3, pad 1, stride 1 over the 8-channel input, openaimodel.py:536-542): x [B,H,W,8] bf16 -> y [B*H*W, 128] bf16,
 * column 8 tap + c (tap = 3 ky + kx), zeros outside the image and in columns 72..127; the conv is then ae_gemm_bf16 with the weight packed
 * [Cout, 128] in the same column order — K = 128 instead of nine K tiles that are 7/8 zero padding.                                            */
int ae_im2col3x3_c8_bf16(const void* x, void* y, int B, int H, int W, void* stream);
/* Adjoint of the channel concat: a (+)= y[:, :Ca], b (+)= y[:, Ca:] in one pass; a or b may be NULL (that half is skipped).       */
int ae_split_channels_bf16(const void* y, int Ca, int Cb, void* a, void* b, long rows, int accumulate_a, int accumulate_b, void* stream);
/* timestep_embedding (util.py:154-174): [cos | sin], t given as int64 or fp32.                                               */
int ae_timestep_embedding(const long* t_i64, const float* t_f32, void* out_bf16, float* out_f32, int B, int dim, float max_period,
                          void* stream);
/* CFG combine + DDIM update, fp32, unfused arithmetic (ddim.py:211-212, 228-250; 3-branch global_tool.py:172-177).
 * eps holds `branches` stacked copies of n elements: 2 -> [uncond, cond]; 3 -> [text, image, uncond].                        */
int ae_ddim_step_f32(const float* x, const float* eps, const float* noise, float* x_prev, float* pred_x0, float* e_out, long n,
                     int branches, float s0, float s1, float sqrt_one_minus_at, float sqrt_at, float sqrt_a_prev, float dir_coef,
                     float sigma_t, float temperature, void* stream);
/* PLMS multistep combination of eps predictions (PLMSSampler.p_sample_plms, plms.py:226-240); order 0 = (e + old1) / 2.           */
int ae_plms_combine_f32(const float* e_t, const float* old1, const float* old2, const float* old3, float* out, long n, int order,
                        void* stream);
/* DDIM inversion update (DDIMSampler.encode, ddim.py:253-298): x_next = cx*x + ce*e, e = CFG combination of `branches`
 * stacked predictions ([uncond, cond]); cx, ce from the host in float64 as the reference computes them.                       */
int ae_ddim_encode_step_f32(const float* x, const float* eps, float* x_next, long n, int branches, float scale, float cx, float ce,
                            void* stream);
/* q_sample (ddpm.py:356-359) fused with the mask blend (ddim.py:154-157; ip2p_order=1: global_tool.py:183-184).               */
int ae_mask_blend_f32(const float* img, const float* x0, const float* noise, const float* mask, float* out, int B, int C, int HW,
                      float sqrt_ac, float sqrt_one_minus_ac, int ip2p_order, void* stream);
int ae_q_sample_f32(const float* x0, const float* noise, const float* sqrt_ac, const float* sqrt_one_minus_ac, float* out, int B,
                    long per_sample, void* stream);
/* y = bf16(silu(x)): the nn.SiLU in front of ResBlock.emb_layers (openaimodel.py:212-219).                                    */
int ae_silu_to_bf16(const void* x, int in_bf16, void* y, long n, void* stream);
/* y = x + p broadcast with period (pos_embed add, image_encoder.py:108-109).                                                 */
int ae_add_bcast_bf16(const void* x, const void* p, void* y, long n, long period, void* stream);
/* Resampling without a convolution on channels-last rows: mode 0 = nearest x2 (Upsample(use_conv=False), openaimodel.py:108-118), mode 1 = 2x2 mean
 * (Downsample(use_conv=False) = avg_pool_nd, openaimodel.py:154-155; floor on odd sizes) — the h_upd / x_upd of ResBlock(up= / down=), :215-221, 254-260.
 * x [B, H, W, C] bf16 -> y [B, 2H, 2W, C] / [B, H/2, W/2, C]; C % 8 == 0.                                                                              */
int ae_resample2x_rows_bf16(const void* x, void* y, int B, int H, int W, int C, int mode, void* stream);
/* ResBlock(use_scale_shift_norm=True), openaimodel.py:264-268: y = act(x * (1 + scale[b]) + shift[b]) on the GroupNorm's output rows x [B * HW, C] bf16;
 * emb fp32 [B, >= 2C] with row stride ld_emb holds scale | shift (th.chunk(emb_out, 2, dim=1)); silu != 0 applies out_rest's SiLU.                     */
int ae_scale_shift_rows_bf16(const void* x, const float* emb, long ld_emb, void* y, int B, long HW, int C, int silu, void* stream);
/* window_partition / window_unpartition (image_encoder.py:243-289); arguments are always (image, windows).                    */
int ae_window_partition_bf16(const void* image, void* windows, int B, int H, int W, int C, int ws, int reverse, void* stream);
/* LayerNorm with the window partition of SAM's windowed blocks folded into its row addressing (image_encoder.py:166-182, 243-289).
 * mode 1: y[window rows] = window_partition(LayerNorm(x[image rows])), padding rows zero (norm1 + partition);
 * mode 2: xsum[image rows] = bf16(x[window rows] + shortcut[image rows]), y = LayerNorm(xsum) (un-partition + shortcut + norm2).
 * Same arithmetic as ae_layernorm_bf16 / ae_window_partition_bf16 / ae_add_bcast_bf16 in sequence (xsum bit for bit).             */
int ae_layernorm_window_supported(int C);
int ae_layernorm_window_bf16(const void* x, const void* shortcut, const float* gamma, const float* beta, void* y, void* xsum,
                             int B, int H, int W, int C, int ws, int mode, float eps, void* stream);
/* rel_h / rel_w einsums of add_decomposed_rel_pos (image_encoder.py:349-355); Rh [qH,kH,D], Rw [qW,kW,D] fp32.                */
int ae_sam_relpos_terms(const void* q, long q_sb, long q_sh, long q_sn, const float* Rh, const float* Rw, float* rel_h,
                        float* rel_w, int B, int heads, int qH, int qW, int kH, int kW, int D, void* stream);
/* PatchEmbed im2col (image_encoder.py:364-395): [B,Cin,H,W] fp32 -> [B*(H/P)*(W/P), Cin*P*P] bf16.                            */
int ae_patchify_f32_bf16(const float* x, void* y, int B, int Cin, int H, int W, int P, void* stream);
/* mean((a-b)^2) -> out[0] (train.py:696, ddpm.py:367-380).  partial: 1024 floats of scratch for the per-block sums, which a second
 * launch adds in block order (the same bits on every run).                                                                   */
int ae_mse_f32(const float* a, const float* b, float* out, float* partial, long n, void* stream);
/* AnySD task router (OUR spec, reference source absent — SURVEY.md §8a row A9): logits = task_emb[edit_code] @ Wg^T + bg,
 * softmax over E experts, top-1 index + probability per sample.                                                              */
int ae_task_gate(const float* task_emb, const long* edit_code, const float* Wg, const float* bg, int B, int n_tasks, int Dt,
                 int E, float* probs, int* top1, float* top1_prob, void* stream);

/* ---- first-stage autoencoder (the step on either side of the denoising loop) — reuses ae_conv3x3_bf16,
 * ae_gemm_bf16, ae_groupnorm_nhwc_bf16; two small kernels of its own:
 * P = softmax(scale * S) row-wise, fp32 logits -> bf16 (AttnBlock, diffusionmodules/model.py:188-192).                        */
int ae_softmax_rows_f32_bf16(const float* S, long lds, void* P, long ldp, int rows, int cols, float scale, void* stream);
/* DiagonalGaussianDistribution (distributions.py:25-37): moments [B, 2*per_half] -> z = mean + std * noise (noise NULL: mode),
 * optional mean / clamped logvar / std outputs.                                                                              */
int ae_gaussian_moments_f32(const float* moments, const float* noise, float* z, float* mean, float* logvar, float* std_out, int B,
                            long per_half, void* stream);

/* ---- GroundingDINO multi-scale deformable attention forward: replaces the reference's only native op,
 * `_C.ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step)`
 * (csrc/vision.cpp:53-56, csrc/MsDeformAttn/ms_deform_attn.h:22-41, ms_deform_im2col_cuda.cuh:237-299).
 * value [bs, S, heads, d] fp32 (S = sum_l H_l*W_l), spatial_shapes [L,2] / level_start_index [L] int64, sampling_loc
 * [bs, Q, heads, L, P, 2] in [0,1] (x, y), attn_weight [bs, Q, heads, L, P]; out [bs, Q, heads*d] fp32.                      */
int ae_ms_deform_attn_fwd_f32(const float* value, const long* spatial_shapes, const long* level_start_index, const float* sampling_loc,
                              const float* attn_weight, float* out, int bs, int S, int heads, int d, int Q, int L, int P, void* stream);
/* Backward of the same operator: `_C.ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
 * grad_output, im2col_step)` (csrc/vision.cpp:57, ms_deform_attn.h:43-64; called from MultiScaleDeformableAttnFunction.backward,
 * ms_deform_attn.py:68-90).  grad_out [bs, Q, heads*d] -> grad_value [bs, S, heads, d], grad_sampling_loc [bs, Q, heads, L, P, 2],
 * grad_attn_weight [bs, Q, heads, L, P]; all three fully overwritten.  grad_value accumulates with float atomics.              */
int ae_ms_deform_attn_bwd_f32(const float* value, const long* spatial_shapes, const long* level_start_index, const float* sampling_loc,
                              const float* attn_weight, const float* grad_out, float* grad_value, float* grad_sampling_loc,
                              float* grad_attn_weight, int bs, int S, int heads, int d, int Q, int L, int P, void* stream);
/* nn.Linear in EXACT fp32 (v_mfma_f32_16x16x4_f32: f32 in, f32 accumulate) for the four projections of GroundingDINO's
 * MultiScaleDeformableAttention (ms_deform_attn.py:281-288, 330-352: value_proj, sampling_offsets, attention_weights, output_proj),
 * which run in fp32 in the reference and feed bilinear sampling locations.  C[M,N] = A[M,K] W[N,K]^T + bias; K % 16 == 0.       */
int ae_linear_f32(const float* A, long lda, const float* W, long ldw, const float* bias, float* C, long ldc, int M, int N, int K,
                  void* stream);

/* DPM-Solver / DPM-Solver++ multistep step (ldm/models/diffusion/dpm_solver/dpm_solver.py:246-316 guidance, :352-365 data prediction,
 * :469-513 first-order and :723-777 second-order multistep updates): m = predict_x0 ? (x - sigma_s e)/alpha_s : e with e the guided
 * noise of model_out ([uncond, cond] when branches == 2; v_param: alpha_s*out + sigma_s*x); update != 0: x_next = a x - b m
 * - c inv_r0 (m - m_prev) (m_prev NULL: first order).  a, b, c, inv_r0: the reference's per-step scalars, computed by the caller. */
int ae_dpm_multistep_f32(const float* x, const float* model_out, const float* m_prev, float* m_cur, float* x_next, long n, int branches,
                         float scale, int v_param, int predict_x0, float sigma_s, float alpha_s, int update, float a, float b, float c,
                         float inv_r0, void* stream);

/* The DPM-Solver updates outside the multistep-2 fast path (dpm_solver.py:469-722 singlestep first / second / third update, :780-826
 * multistep third update): each is out = c0 x0 + c1 x1 + c2 x2 + c3 x3 with host-side fp32 scalars (x1..x3 may be NULL).              */
int ae_lincomb4_f32(float* out, const float* x0, float c0, const float* x1, float c1, const float* x2, float c2, const float* x3, float c3,
                    long n, void* stream);
/* Error estimate of the adaptive step-size solver (dpm_solver.py:925-927): out[b] = sqrt(mean(((x_higher - x_lower) / delta)^2)) over the
 * n_per_sample elements of sample b, delta = max(atol, rtol * max(|x_lower|, |x_prev|)).                                            */
int ae_dpm_adaptive_err_f32(const float* x_lower, const float* x_higher, const float* x_prev, float atol, float rtol, int B,
                            long n_per_sample, float* out, void* stream);

/* ---- SAM prompt encoder / mask decoder: the non-GEMM kernels behind SamPredictor.predict_torch
 * (segment_anything/predictor.py:168-245).
 * ae_layernorm_act_bf16: LayerNorm over a narrow last dim (C <= 512) with optional fused GELU (act 1) — the LayerNorm2d + GELU of
 *   MaskDecoder.output_upscaling (mask_decoder.py:53-60) on channels-last rows.
 * ae_sam_pe_encode_f32: PositionEmbeddingRandom (prompt_encoder.py:174-214) of N pixel coordinates (x, y): out [N, 2F] =
 *   cat(sin, cos)(2 pi ((2c-1) @ gauss[2,F])), c = (coords + offset) * (inv_w, inv_h).  labels (int32, optional): -1 -> encoding
 *   zeroed + table row 0 (not_a_point_embed); l >= 0 -> + table row 1+l (point_embeddings[l]) — PromptEncoder._embed_points /
 *   _embed_boxes (:73-102).  table [5, 2F].
 * ae_sam_mask_downscale_bf16: PromptEncoder.mask_downscaling[0:6] (:46-53) for mask_in_chans = 16: masks [B,1,4h,4w] fp32 ->
 *   channels-last rows [B*h*w, 16] bf16 (the closing 1x1 convolution is an ae_gemm_bf16).
 * ae_sam_mask_product_f32: masks = hyper_in @ upscaled_embedding (mask_decoder.py:141-149).  up: bf16 [B, h, w, 2,2, 2,2, C] = the
 *   two transposed convolutions' GEMM outputs left un-shuffled; hyper [B, M, C] fp32; out [B, M, 4h, 4w] fp32.
 * ae_sam_postprocess_masks: Sam.postprocess_masks (sam.py:133-162) fused: bilinear (Hl,Wl)->(S,S), crop [:ih,:iw], bilinear ->
 *   (oh,ow); writes fp32 logits and/or the (logit > threshold) uint8 mask.  merge != 0: out_u8 [oh,ow] = OR over the N masks
 *   (maskgeneration's mask_mode 'merge', tools/tool.py:239-241).
 * ae_nms_sorted_f32: greedy IoU suppression == torchvision.ops.nms (tools/tool.py:224) over XYXY boxes already sorted by
 *   descending score; keep[i] (uint8) = 1 for survivors.
 * ae_sam_preprocess_f32: Sam.preprocess (sam.py:164-174): (x - mean[c]) / std[c], zero-padded to [B, C, S, S]; x uint8 or fp32. */
int ae_layernorm_act_bf16(const void* x, const float* gamma, const float* beta, void* y, long M, int C, float eps, int act, void* stream);
int ae_sam_pe_encode_f32(const float* coords, const int* labels, const float* gauss, const float* table, float* out, int N, int F,
                         float offset, float inv_w, float inv_h, void* stream);
int ae_sam_mask_downscale_bf16(const float* masks, const float* w1, const float* b1, const float* g1, const float* e1, const float* w2,
                               const float* b2, const float* g2, const float* e2, void* out, int B, int h, int w, float eps, void* stream);
int ae_sam_mask_product_f32(const void* up, const float* hyper, float* out, int B, int h, int w, int M, int C, void* stream);
int ae_sam_postprocess_masks(const float* low, float* out_f32, void* out_u8, int N, int Hl, int Wl, int S, int ih, int iw, int oh, int ow,
                             float threshold, int merge, void* stream);
int ae_nms_sorted_f32(const float* boxes, void* keep, int N, float iou_threshold, void* stream);
int ae_sam_preprocess_f32(const void* x, int x_is_u8, float* y, int B, int C, int h, int w, int S, const float* mean, const float* stdv,
                          void* stream);

/* ---- CLIP text tower (ldm/modules/encoders/modules.py:107-150 FrozenCLIPEmbedder; ddpm.py:664-677 get_learned_conditioning;
 * tools/global_tool.py:360-396 _encode_prompt; train.py:644 text_encoder(input_ids)[0]; cldm/hack.py:23-68 chunked forward).  The
 * projections and LayerNorms of its 12 pre-LN layers are ae_gemm_bf16 / ae_layernorm_bf16 launches; these three are the rest.
 * ae_attn_causal_short_bf16: out = softmax(causal(q k^T * scale)) v for the tower's self-attention (the causal mask of
 *   transformers' CLIPTextTransformer).  q/k/v bf16 addressed through (batch, head, row) element strides as in ae_attn_fwd_bf16
 *   (so a packed [B*N, 3*H*D] projection is read in place), out bf16 through its own strides.  1 <= N <= 128, D in {32, 64};
 *   strides of q/k/v multiples of 8, of out multiples of 4; anything else is refused.  Row i attends keys [0, i]; row 0 returns v[0].
 * ae_clip_embed_bf16: CLIPTextEmbeddings: out[b*N + n] = token_table[ids[b*N + n]] + position_table[n], tables and out bf16 rows of
 *   C (C % 8 == 0).  ids int32 (ids_are_i64 = 0) or int64.  An id outside [0, vocab) is CLAMPED into the table by the kernel (the
 *   host cannot range-check device ids without a synchronisation; host-side ids are checked by the caller).
 * ae_bias_act_f32_bf16: the activation between CLIPMLP's fc1 and fc2: y = act(u + bias), u the fp32 product of
 *   ae_gemm_bf16(..., out_f32 = 1), y bf16 — the pre-activation is never rounded to bf16.  act 0: quick-GELU t * sigmoid(1.702 t)
 *   (OpenAI ViT-L/14), act 1: erf-GELU (SD-2's ViT-H text tower).  N % 4 == 0, row strides multiples of 4.                        */
int ae_attn_causal_short_bf16(const void* q, const void* k, const void* v, void* out, int B, int H, int N, int D,
                              long q_sb, long q_sh, long q_sn, long k_sb, long k_sh, long k_sn, long v_sb, long v_sh, long v_sn,
                              long o_sb, long o_sh, long o_sn, float scale, void* stream);
int ae_clip_embed_bf16(const void* ids, int ids_are_i64, const void* token_table, const void* position_table, void* out, int B, int N,
                       int C, int vocab, int positions, void* stream);
int ae_bias_act_f32_bf16(const float* u, long ldu, const float* bias, void* y, long ldy, long M, int N, int act, void* stream);
/* pooler_output (modules.py:141-142 layer == "pooled"): out[b] = z[b, first n with ids[b, n] == eos_token_id] (n = 0 when there is none), z the
 * final-normed bf16 [B, N, C], out bf16 [B, C]; the position is found on the device, so ids are not read back.                      */
int ae_clip_pool_eos_bf16(const void* ids, int ids_are_i64, const void* z, void* out, int B, int N, int C, long eos_token_id, void* stream);

/* ---- CLIP vision tower (train.py:404 CLIPVisionModelWithProjection.from_pretrained(image_encoder_path); train.py:689-691
 * image_encoder(reference_clip_images, output_hidden_states=True).hidden_states[-2]).  The projections, layer LayerNorms, fc1 activation and
 * the non-causal attention of its pre-LN layers are ae_gemm_bf16 / ae_layernorm_bf16 / ae_bias_act_f32_bf16 / ae_attn_fwd_bf16 launches;
 * these three are the rest.  All write bf16 with one rounding at the store, keep fp32 statistics, use no scratch and no atomics.
 * ae_clip_patch_rows_bf16: the im2col of CLIPVisionEmbeddings.patch_embedding (Conv2d(Cin, C, P, stride P, bias=False)) with the image
 *   processor's rescale + normalise fused in.  x: contiguous [B, Cin, H, W], x_dtype 0 fp32 / 1 bf16 / 2 uint8, H % P == 0, W % P == 0.
 *   rows: bf16 [B*(H/P)*(W/P), Kpad], Kpad = Cin*P*P rounded up to a multiple of 64; column c*P*P + ky*P + kx of row (b, gy, gx) holds
 *   (x[b, c, gy*P + ky, gx*P + kx] * rescale - mean[c]) / std[c]; mean = std = NULL: x * rescale (rescale = 1: plain conversion).  Columns
 *   [Cin*P*P, Kpad) are WRITTEN as zeros.  The matching weight image is the conv weight flattened to [C, Cin*P*P], zero-padded to Kpad.
 *   x needs only the alignment of its type (a P = 14 patch row of fp32 pixels is 8-byte aligned); wider loads are taken when P % 8 == 0.
 * ae_clip_vision_embed_ln_bf16: the token rows and pre_layrnorm in one launch: out[b*(1+G)] = LN(class_embedding + pos[0]),
 *   out[b*(1+G) + 1 + i] = LN(patch[(b*G + i) * ldp ...] + pos[1 + i]); patch is the fp32 product of ae_gemm_bf16(rows, Wpatch, out_f32 = 1),
 *   class_embedding [C] and pos [1+G, C] fp32, out bf16 [B*(1+G), C] (transformers' hidden_states[0]).  The un-normalised sum is never stored.
 *   C % 8 == 0, C <= 2048 (refused above), ldp % 4 == 0, pointers 16-byte aligned.
 * ae_clip_vision_pool_ln_bf16: post_layernorm of the class rows only: out[b] = LN(x[b * row_stride ...]), x bf16 (row_stride = N*C picks
 *   row b*N of a [B*N, C] buffer), out bf16 [B, C].  C % 8 == 0, C <= 2048, row_stride % 8 == 0.                                         */
int ae_clip_patch_rows_bf16(const void* x, int x_dtype, void* rows, int B, int Cin, int H, int W, int P, int Kpad, float rescale,
                            const float* mean, const float* stdv, void* stream);
int ae_clip_vision_embed_ln_bf16(const float* patch, long ldp, const float* class_embedding, const float* pos, const float* gamma,
                                 const float* beta, void* out, int B, int G, int C, float eps, void* stream);
int ae_clip_vision_pool_ln_bf16(const void* x, long row_stride, const float* gamma, const float* beta, void* out, int B, int C, float eps,
                                void* stream);

/* ---- DINOv2 image encoder (ldm/modules/encoders/modules.py:279-315 FrozenDinoV2Encoder: dinov2_vitg14 forward_features, class + patch tokens
 * after the final norm, projector = Linear(1536, 1024); the backbone is AnyEdit_Collection/other_modules/depth_anything_v2/dinov2.py:44-328
 * DinoVisionTransformer).  The patch im2col is ae_clip_patch_rows_bf16 (ImageNet mean / std), everything in the blocks is ae_gemm_bf16 /
 * ae_layernorm_bf16 / ae_attn_fwd_bf16 / ae_bias_act_f32_bf16, LayerScale (dinov2_layers/layer_scale.py) is folded into the weights at pack
 * time; these two are the rest.  Both write bf16 with one rounding at a 16-byte store, use no scratch and no atomics.
 * ae_dino_embed_bf16: the token rows (dinov2.py:212-219 prepare_tokens_with_masks, no masks, no register tokens):
 *   out[b*(1+G)] = cls_token + pos[0], out[b*(1+G) + 1 + i] = patch[(b*G + i) * ldp ...] + patch_bias + pos[1 + i]; patch is the fp32 product of
 *   ae_gemm_bf16(rows, Wpatch, out_f32 = 1), patch_bias / cls_token [C] and pos [1+G, C] fp32 (pos: dinov2.py:179-210 interpolate_pos_encoding
 *   for this grid, made on the host side once), out bf16 [B*(1+G), C].  No LayerNorm: DINOv2 has no pre-norm.  C % 8 == 0, ldp % 4 == 0,
 *   pointers 16-byte aligned.
 * ae_swiglu_f32_bf16: the gate of SwiGLUFFN (dinov2_layers/swiglu_ffn.py:29-33: x1, x2 = w12(x).chunk(2); silu(x1) * x2):
 *   y[m*ldy + j] = silu(u[m*ldu + j] + bias[j]) * (u[m*ldu + Hd + j] + bias[Hd + j]) for j < Hd, u the fp32 [M, 2*Hd] product of
 *   ae_gemm_bf16(..., out_f32 = 1) — the pre-activation is never rounded —, bias fp32 [2*Hd], y bf16.  Columns [Hd, ldy) of y are WRITTEN as
 *   zeros (a padded contraction width for w3 contracts against zeros).  Hd % 8 == 0, ldu % 4 == 0, ldu >= 2*Hd, ldy % 8 == 0, ldy >= Hd,
 *   pointers 16-byte aligned.                                                                                                              */
int ae_dino_embed_bf16(const float* patch, long ldp, const float* patch_bias, const float* cls_token, const float* pos, void* out, int B, int G,
                       int C, void* stream);
int ae_swiglu_f32_bf16(const float* u, long ldu, const float* bias, void* y, long ldy, long M, int Hd, void* stream);

/* ---- GroundingDINO's Swin backbone (GroundingDINO/groundingdino/models/GroundingDINO/backbone/swin_transformer.py:501-759 SwinTransformer,
 * built by build_swin_transformer :762-791; the detector of tools/tool.py runs it on every image).  Patch embedding is ae_clip_patch_rows_bf16 with
 * P = 4 + ae_gemm_bf16 + ae_layernorm_bf16, every norm ae_layernorm_bf16, qkv / proj / fc2 ae_gemm_bf16 (residual adds in the epilogue), fc1's GELU
 * ae_bias_act_f32_bf16, the NCHW outputs ae_transpose_last2; these two are the rest.  Both write bf16 with one rounding at the store, use no
 * scratch and no atomics.
 * ae_swin_window_attn_bf16: SwinTransformerBlock.forward from the pad after norm1 to the crop (:253-292) around the core of WindowAttention.forward
 *   (:140-171).  qkv: bf16 rows in IMAGE order [B*H*W, 3C] with row stride ldq, the packed output of one ae_gemm_bf16 (+bias) on norm1(x): column
 *   s*C + head*32 + j holds (q, k, v)[s] of that head (reshape(B_, N, 3, nH, D)).  out: bf16 rows in image order [B*H*W, C], row stride ldo.
 *   With Hp, Wp = H, W rounded up to multiples of ws, the token at in-window position (i, j) of window (wy, wx) has the shifted-frame coordinate
 *   (ys, xs) = (wy*ws + i, wx*ws + j) and the image coordinate ((ys + shift) mod Hp, (xs + shift) mod Wp); it is read from and written to that
 *   image row — no padded, rolled or partitioned copy exists.  A token with y >= H or x >= W is a pad token: its key and value are qkv_bias
 *   rounded to bf16 (the reference pads norm1's output with zeros, then applies qkv), it takes part in the softmax as a key, and its output row is
 *   never written.  Logits scale * q k^T + bias[head][query][key] are fp32 (bias: fp32 [nH, N, N], N = ws*ws, relative_position_bias_table
 *   gathered through relative_position_index); for shift > 0 exactly -100.0 is added where the regions 3 r(ys) + r(xs) of query and key differ,
 *   r(p) = 0 for p < L - ws, 1 for p < L - shift, 2 otherwise, L = Hp resp. Wp (BasicLayer.forward :417-443, computed in the kernel).  fp32
 *   softmax; probabilities are rounded to bf16 only as MFMA operands of P V.  head_dim C / nH must be 32, 1 <= ws <= 16, 0 <= shift < ws,
 *   ldq >= 3C, ldo >= C, both multiples of 8, pointers 16-byte aligned, B*H*W < 2^31; anything else is refused.  One launch covers all samples,
 *   windows and heads.
 * ae_swin_merge_ln_bf16: PatchMerging.forward up to the norm (:320-337): x bf16 [B, H, W, C] contiguous -> y bf16 [B*ceil(H/2)*ceil(W/2), 4C],
 *   row (b, i, j) = LayerNorm over 4C of cat(x(2i, 2j), x(2i+1, 2j), x(2i, 2j+1), x(2i+1, 2j+1)); a position outside the map is zeros and those
 *   zeros enter the statistics (the reference pads, then normalises).  gamma / beta fp32 [4C].  C % 8 == 0, 4C <= 4096, pointers 16-byte aligned.
 *   The `reduction` Linear behind it is an ae_gemm_bf16 without bias.                                                                          */
int ae_swin_window_attn_bf16(const void* qkv, long ldq, const float* qkv_bias, const float* bias, void* out, long ldo, int B, int H, int W, int C,
                             int nH, int ws, int shift, float scale, void* stream);
int ae_swin_merge_ln_bf16(const void* x, const float* gamma, const float* beta, void* y, int B, int H, int W, int C, float eps, void* stream);

/* ---- GroundingDINO's feature enhancer (GroundingDINO/groundingdino/models/GroundingDINO/transformer.py:406-595 TransformerEncoder: per layer a
 * BiAttentionBlock (fuse_modules.py:252-295), a text TransformerEncoderLayer (transformer_vanilla.py:72-123) and a
 * DeformableTransformerEncoderLayer (transformer.py:738-799)).  LayerNorms are ae_layernorm_bf16, projections and feed-forwards ae_gemm_bf16 /
 * ae_ln_gemm_bf16 (EPI_RELU), the deformable attention ae_linear_f32 + ae_ms_deform_attn_fwd_f32; these are the rest (csrc/gdino_encoder.hip).
 * No atomics, no scratch; every launch is deterministic.
 * ae_biattn_bf16: BiMultiHeadAttention.forward between the projections (fuse_modules.py:174-225), head_dim D = 256 only.  All rows bf16, row r of
 *   sample b at (b*N + r) * ld, head h in columns [h*D, (h+1)*D):  q [B, Nv] = v_proj output (the scale of :162 is passed as `scale` and applied to
 *   the fp32 logits), k [B, Nt] = l_proj output, val_v [B, Nv], val_l [B, Nt].  mask_v [B, Nv] / mask_l [B, Nt]: uint8, may be null; NON-ZERO = a
 *   PADDED token (the reference's sense, True = padding: :205-218 masked_fill(-inf)), removed as a KEY of the other stream's softmax.  Rows of
 *   padded QUERIES are computed like any others, as the reference does.
 *     out_v[b, i, h] = sum_j softmax_j(scale q_i . k_j over j with mask_l[b, j] == 0) val_l[j]        (:218-224)
 *     out_l[b, j, h] = sum_i softmax_i(scale q_i . k_j over i with mask_v[b, i] == 0) val_v[i]        (:193-211, :225)
 *   Both softmaxes are fp32 and subtract their own running maximum; probabilities are rounded to bf16 only as MFMA operands.  Left out: the
 *   subtraction of the global attn_weights.max() (:181-182) and the clamps to +-50000 (:184-202) — a softmax is invariant to a shift of its row, so
 *   they change a result only when the logits of one call span more than 50000.  Contract (not checked: it would be a host sync): every sample has
 *   at least one unmasked text token and one unmasked image token.  No buffer of size ~ Nv*Nt exists: the logits are recomputed per direction.  The
 *   text direction cuts the image tokens into partials of ae_biattn_split_rows(Nv) rows (at most 32 partials), each leaving (running maximum, sum,
 *   fp32 accumulator) in `workspace`; a combine kernel merges them in partial order, so two launches give bit-identical outputs.  workspace:
 *   ae_biattn_workspace_bytes(B, heads, Nv, Nt, D) bytes, 16-byte aligned, owned by the call until the next call on that stream (0 = unsupported
 *   sizes).  1 <= Nt <= 256, Nv >= 1, B*heads <= 65535, row strides >= heads*D and multiples of 8, pointers 16-byte aligned.  Three launches.
 * ae_attn_masked_short_bf16: the attention core of nn.MultiheadAttention as transformer_vanilla.py:115 calls it (attn_mask, no key_padding_mask):
 *   q/k/v bf16 addressed by (batch, head, row) element strides as ae_attn_causal_short_bf16; mask uint8 [B*H, N, N] contiguous, slice b*H + h, row =
 *   query, NON-ZERO = the key is ALLOWED (the reference passes ~text_self_attention_masks as a disallow mask, transformer.py:569; this takes the
 *   un-negated one); out bf16 through (batch, head, row) strides.  Contract: every row allows at least one key (the reference's masks contain the
 *   diagonal).  1 <= N <= 256, D in {32, 64}, B*H <= 65535; fp32 one-pass softmax.
 * ae_scale_residual_f32_bf16: out = res + gamma * (u + bias), rounded to bf16 once — BiAttentionBlock's layer-scaled residual (fuse_modules.py:293-294,
 *   u the fp32 product of out_v_proj / out_l_proj without bias) and the residual behind the fp32 deformable attention (transformer.py:793).  u fp32
 *   [M, N] row stride ldu, bias / gamma fp32 [N] or null (0 / 1), res and out bf16.  N % 4 == 0, strides multiples of 4.                           */
int ae_scale_residual_f32_bf16(const float* u, long ldu, const float* bias, const float* gamma, const void* res, long ldr, void* out, long ldo, long M,
                               int N, void* stream);
int ae_biattn_split_rows(int Nv);
long ae_biattn_workspace_bytes(int B, int heads, int Nv, int Nt, int D);
int ae_biattn_bf16(const void* q, long ldq, const void* k, long ldk, const void* val_v, long ldvv, const void* val_l, long ldvl, const void* mask_v,
                   const void* mask_l, void* out_v, long ldov, void* out_l, long ldol, int B, int heads, int Nv, int Nt, int D, float scale,
                   void* workspace, long workspace_bytes, void* stream);
int ae_attn_masked_short_bf16(const void* q, const void* k, const void* v, const void* mask, void* out, int B, int H, int N, int D, long q_sb, long q_sh,
                              long q_sn, long k_sb, long k_sh, long k_sn, long v_sb, long v_sh, long v_sn, long o_sb, long o_sh, long o_sn, float scale,
                              void* stream);

/* ---- GroundingDINO's query selection, decoder and heads (GroundingDINO/groundingdino/models/GroundingDINO/transformer.py:284-327 two-stage query
 * selection, :598-735 TransformerDecoder, :802-927 DeformableTransformerDecoderLayer; groundingdino.py:317-335 heads).  Self- and text
 * cross-attention are ae_attn_fwd_bf16 (head_dim 32, key mask), the deformable cross-attention ae_linear_f32 + ae_ms_deform_attn_fwd_f32 +
 * ae_scale_residual_f32_bf16, projections and feed-forwards ae_gemm_bf16, LayerNorms ae_layernorm_bf16; these are the rest
 * (csrc/gdino_decoder.hip).  No atomics, no scratch, no host synchronisation; every launch is deterministic.  Divisions are IEEE and logf / expf /
 * sinf / cosf the library's own, no fast-math variants: validity flags depend on fp32 values bit for bit.
 * ae_contrastive_bf16: ContrastiveEmbed.forward (utils.py:233-268) and / or its row maximum (transformer.py:291-295).  x bf16 rows, row n of sample b
 *   at (b*N + n) * ldx, C wide; y bf16 [B, T, C] contiguous; token_mask uint8 [B, T] or null, NON-ZERO = a USED token (the reference's
 *   text_token_mask).  logits (may be null) fp32, row (b*N + n) * ldl, max_text_len wide: x_n . y_t for used t < T, -inf for unused tokens and for
 *   columns T .. max_text_len-1 (:262-266).  rowmax (may be null) fp32 [B, N]: the maximum of that row, bit-equal to the maximum of the logits a call
 *   with both outputs stores; -inf when the sample has no used token.  With logits null nothing of size B*N*T is written or allocated.  MFMA on the
 *   bf16 operands, fp32 accumulation.  C % 32 == 0, C <= 256, 1 <= T <= max_text_len <= 256, N >= 1, B <= 65535, ldx % 8 == 0, x / y / logits
 *   16-byte aligned; the rest is refused.  The text rows are streamed through LDS in tiles of 64 tokens (33 856 bytes).
 * ae_topk_rows_f32: out int32 [B, k] = the first k indices of torch.sort(scores, dim=1, descending=True, stable=True) (transformer.py:301 with a
 *   defined order among ties): descending value, equal values by ascending index; -0.0 == +0.0; -inf entries are ordinary values; NaN of either
 *   sign orders above +inf and all NaNs are equal.  scores fp32, row b at b * ld.  1 <= k <= min(N, 1024), N <= ae_topk_rows_max_n() = 2^24.  One
 *   workgroup per row: radix select of the k-th key bit by bit, compaction in index order, rank sort in LDS.
 * ae_gdino_proposals_f32: gen_encoder_output_proposals (utils.py:56-116, learnedwh=None).  padding_mask uint8 [B, N], NON-ZERO = padding;
 *   shapes_hw / level_start: HOST arrays int [L, 2] / [L] (checked against each other and N, L <= 8).  proposals fp32 [B, N, 4]: log(p / (1 - p))
 *   of p = ((x + 0.5) / valid_W, (y + 0.5) / valid_H, 0.05 * 2^lvl, 0.05 * 2^lvl) (:86, :92, :105), valid_H / valid_W counted on the level's first
 *   column / first row (:74-75); padded rows and rows with a coordinate outside 0.01 < p < 0.99 hold +inf in all four (:102-107).  keep uint8
 *   [B, N]: 1 where the row is neither (the rows whose memory :110-111 keeps).  A valid extent of 0 gives +inf, not a fault.
 * ae_gdino_query_sine: ref fp32 [B, nq, 4] sigmoid boxes, valid_ratios fp32 [B, L, 2] -> ref_input fp32 [B, nq, L, 4] = ref[:, :, None] *
 *   cat([valid_ratios, valid_ratios], -1)[:, None] (transformer.py:667-671), and embed bf16 rows (b*nq + q) * lde, 512 wide =
 *   gen_sineembed_for_position(ref_input[:, :, 0, :]) (utils.py:204-230) in its (y, x, w, h) order.  lde >= 512, even.
 * ae_gdino_box_refine_f32: the last layer of a box MLP and the anchor update (transformer.py:721-724, groundingdino.py:322-324): h fp32 [M, 256]
 *   row stride ldh, w3 fp32 [4, 256], b3 fp32 [4], ref fp32 [M, 4]:  u = (h w3^T + b3) + inverse_sigmoid(ref) (util/misc.py:704, eps = 1e-3),
 *   boxes = sigmoid(u) fp32 [M, 4]; u_out (may be null) receives u.  ref_is_logit != 0 (transformer.py:296-306): ref is already un-sigmoided, may
 *   be +inf, and is added as it is (+inf gives a box of 1.0).                                                                                   */
int ae_contrastive_bf16(const void* x, long ldx, const void* y, const void* token_mask, float* logits, long ldl, float* rowmax, int B, int N, int T, int C,
                        int max_text_len, void* stream);
int ae_topk_rows_max_n(void);
int ae_topk_rows_f32(const float* scores, long ld, int* out, int B, int N, int k, void* stream);
int ae_gdino_proposals_f32(const void* padding_mask, const int* shapes_hw, const int* level_start, int L, float* proposals, void* keep, int B, int N,
                           void* stream);
int ae_gdino_query_sine(const float* ref, const float* valid_ratios, float* ref_input, void* embed, long lde, int B, int nq, int L, void* stream);
int ae_gdino_box_refine_f32(const float* h, long ldh, const float* w3, const float* b3, const float* ref, float* boxes, float* u_out, long M, int ref_is_logit,
                            void* stream);

/* ---- GroundingDINO's text side (GroundingDINO/groundingdino/models/GroundingDINO/groundingdino.py:233-283; bertwarper.py:180-273; the BertModel the
 * reference takes from transformers: BertEmbeddings, BertSelfAttention).  Projections are ae_gemm_bf16, the post-LayerNorms ae_layernorm_bf16, the
 * GELU ae_bias_act_f32_bf16; these are the rest (csrc/gdino_text.hip).  No atomics, no scratch, no host synchronisation; every launch is
 * deterministic; statistics in fp32, bf16 once at the store.
 * ae_gdino_text_spans: generate_masks_with_special_tokens / _and_transfer_map (bertwarper.py:180-273) without the host loop or torch.nonzero.  ids
 *   int32 / int64 [B, N] contiguous; n_special <= 8 special ids s0 .. s7 by value (groundingdino.py:119).  spans int32 [B, N, 2] = (lo, hi): query
 *   n may attend keys [lo, hi); position_ids int64 [B, N]; dense_mask (may be null) uint8 [B, N, N], 1 = allowed (bertwarper.py:199-215's
 *   attention_mask).  With e the first special position >= n and p the last special position before e: e exists, e != 0, e != N-1 -> [p+1, e+1),
 *   position n - (p+1); otherwise [n, n+1), position 0.  Contract (the reference's, which does not reset previous_col per row): column 0 of every
 *   row is a special token.  1 <= N <= 256, B <= 65535.  One launch.
 * ae_bert_embed_ln_bf16: BertEmbeddings.forward: out[b*N + n] = LayerNorm(word[ids] + position[position_ids] + token_type[type_ids]), the sum
 *   kept in fp32 registers and never stored.  ids / position_ids / type_ids int64 [B, N] (what a tokenizer and ae_gdino_text_spans give); position_ids null
 *   = n, type_ids null = row 0.  Tables bf16 [vocab | positions | types, C] contiguous, gamma / beta fp32 [C], out bf16 [B*N, C].  An index outside its table is
 *   clamped into it (device ids are not read back).  C % 8 == 0, C <= 2048 (a row lives in one wave's registers), everything 16-byte aligned.
 * ae_attn_span_short_bf16: BertSelfAttention's core under a block-diagonal mask: out = softmax(scale q k^T over keys [lo, hi)) v.  q/k/v/out bf16
 *   addressed by (batch, head, row) element strides exactly as ae_attn_masked_short_bf16 (a packed [B*N, 3*H*D] projection is read in place);
 *   spans int32 [B, N, 2] shared by all heads, contract 0 <= lo < hi <= N (a span outside it is forced inside: it can change a result, never an
 *   address).  A workgroup stages and multiplies only the 64-key tiles its 64 queries' spans touch; keys outside a query's span have probability
 *   exactly 0; k / v rows outside every span of a workgroup are never read.  1 <= N <= 256, D == 64, B*H <= 65535; fp32 one-pass softmax.      */
int ae_gdino_text_spans(const void* ids, int ids_are_i64, int B, int N, int n_special, long s0, long s1, long s2, long s3, long s4, long s5, long s6, long s7,
                        int* spans, long* position_ids, void* dense_mask, void* stream);
int ae_bert_embed_ln_bf16(const long* ids, const long* position_ids, const long* type_ids, const void* word_table, const void* position_table,
                          const void* type_table, const float* gamma, const float* beta, void* out, int B, int N, int C, int vocab, int positions, int types,
                          float eps, void* stream);
int ae_attn_span_short_bf16(const void* q, const void* k, const void* v, const int* spans, void* out, int B, int H, int N, int D, long q_sb, long q_sh,
                            long q_sn, long k_sb, long k_sh, long k_sn, long v_sb, long v_sh, long v_sn, long o_sb, long o_sh, long o_sn, float scale,
                            void* stream);

/* ---- GroundingDINO's neck and grounded-box filter (csrc/gdino_neck.hip): what joins the Swin stages, the transformer and the caller.  The input_proj
 * convolutions are ae_gemm_bf16 (1x1) and ae_conv3x3_bf16 (stride 2) with fp32 output.  No atomics, fixed reduction orders: every launch is
 * deterministic; current stream only, no host synchronisation, no allocation.
 * ae_gdino_level_geometry: for all L <= 8 levels of a batch in one launch: F.interpolate(m[None].float(), size=...).to(bool) (backbone.py:113,
 *   groundingdino.py:306), PositionEmbeddingSineHW.forward with normalize=True (position_encoding.py:98-131), the `+ level_embed[lvl]` and the
 *   flatten / cat of Transformer.forward (transformer.py:226-246) and Transformer.get_valid_ratio.  mask uint8 / bool [B, H, W], non-zero = padding, or
 *   null (nothing padded); shapes_hw [L][2] = (h, w) and level_start [L] on the host, sum h w == N; level_embed fp32 [L, 256] or null.
 *   mask_flatten uint8 [B, N]: mask_l[y][x] = mask[y H / h][x W / w] (integer division).  pos_flatten bf16 [B, N, 256]: channels 0..127 from
 *   y_embed = #{y' <= y : !mask_l[y'][x]}, 128..255 from x_embed = #{x' <= x : !mask_l[y][x']} (true prefix counts: the mask may have holes), each
 *   e / (e_last + 1e-6) * 2 pi in fp32, channel i of a half = sin (i even) / cos (i odd) of that / T ** (2 (i / 2) / 128), + level_embed in fp32, one
 *   bf16 rounding.  valid_ratios fp32 [B, L, 2] = (unpadded cells of row 0 / w, of column 0 / h).
 * ae_gdino_neck_groupnorm: the GroupNorm(32, 256) of input_proj (groundingdino.py:127-138) on the fp32 projection.  x fp32 [B * hw rows] of 256,
 *   row stride ldx; out bf16: row r of sample b goes to out + b * out_batch_stride + (out_row_offset + r) * 256 (elements) — a level's slice of
 *   src_flatten [B, N, 256].  Statistics: two-pass per 64-row chunk, chunks combined by mean = sum n_c mean_c / n, M2 = sum (M2_c + n_c (mean_c -
 *   mean)^2) in a fixed order.  workspace: ae_gdino_neck_groupnorm_workspace_floats(B, hw) floats, written and read inside the call.  Two launches.
 * ae_gdino_ground: get_grounding_output's filter (AnyEdit_Collection/adaptive_editing_pipelines/tools/tool.py:125-133) per image.  pred_logits fp32
 *   [B, nq, T] contiguous (-inf on unused columns), T % 32 == 0, T <= 256, nq <= 1024; pred_boxes fp32 [B, nq, 4].  score_q = max_t sigmoid(logit);
 *   query q is kept when score_q > box_threshold.  count int32 [B]; indices int32 [B, nq], scores fp32 [B, nq], boxes fp32 [B, nq, 4], token_bits
 *   uint32 [B, nq, T / 32] (bit t % 32 of word t / 32 = sigmoid(logit_t) > text_threshold): rows 0 .. count - 1 hold the kept queries in ascending
 *   query order, the rows behind them index -1 and zeros.  One launch.                                                                          */
int ae_gdino_level_geometry(const void* mask, int B, int H, int W, const int* shapes_hw, const int* level_start, int L, float temperatureH,
                            float temperatureW, const float* level_embed, void* mask_flatten, void* pos_flatten, float* valid_ratios, int N, void* stream);
long ae_gdino_neck_groupnorm_workspace_floats(int B, int hw);
int ae_gdino_neck_groupnorm(const float* x, long ldx, const float* gamma, const float* beta, float eps, void* out, long out_batch_stride,
                            long out_row_offset, int B, int hw, float* workspace, void* stream);
int ae_gdino_ground(const float* pred_logits, const float* pred_boxes, float box_threshold, float text_threshold, int* count, int* indices, float* scores,
                    float* boxes, void* token_bits, int B, int nq, int T, void* stream);

/* ---- HED edge detector (csrc/hed.hip; AnyEdit_Collection/other_modules/HED/__init__.py): what stands around the 3x3 convolutions, which are
 * ae_conv3x3_bf16.  Bandwidth-bound kernels, no atomics, fixed summation orders: every launch is deterministic; current stream only, no host
 * synchronisation, no allocation.
 * ae_hed_stem_bf16: `h = x - self.norm` (:45) and block1.convs[0] with its ReLU (:19, :29-30) in one launch.  x: uint8 (x_is_f32 = 0) or fp32 (1),
 *   element (b, c, y, x) at b sb + c sc + y sh + x sw (elements): a uint8 image [B, H, W, 3] and the fp32 [B, 3, H, W] of __call__ alike.  norm
 *   fp32 [3], w fp32 [C1, 3, 3, 3], bias fp32 [C1]; fp32 accumulation starting from the bias, taps in the order of w.  The zero padding applies
 *   to x - norm: a tap outside the image contributes 0.  out bf16 [B*H*W, C1], C1 % 8 == 0, C1 <= 512.
 * ae_relu_bf16: x = max(x, 0) in place on n bf16 values (:30 for the convolutions that are not last in their block); negative values, -0 and
 *   negative NaNs become +0.
 * ae_hed_tail_bf16: the end of DoubleConvBlock.__call__ (:30-31) and the next block's max_pool2d (:27) in one pass.  y bf16 [B, H, W, C], the
 *   last convolution's output BEFORE its ReLU, C % 8 == 0; wp fp32 [C], bp fp32 [1] (on the device).  proj fp32 [B, H, W] = sum_c relu(y)[c] wp[c]
 *   + bp, fp32 accumulation.  pooled bf16 [B, H/2, W/2, C] = max_pool2d(relu(y), 2, 2) (floor division: an odd last row or column is projected,
 *   not pooled), or NULL (block 5).  relu(y) itself is never written.
 * ae_hed_fuse: HEDdetector.__call__ :67-73.  p0 .. p4 fp32 [B, H >> k, W >> k], 16 <= H, W <= 16384.  Each is resized to H x W as
 *   cv2.resize(INTER_LINEAR) / F.interpolate(mode="bilinear", align_corners=False) define it (half-pixel centres, edge clamp, scale = src / dst per
 *   axis), the five are averaged in fp32, then sigmoid in fp64, * 255, clip, truncation.  out uint8 [B, H, W] (invert: 255 - v, cv2.bitwise_not);
 *   logits: optional fp32 [B, H, W], the mean before the sigmoid.                                                                             */
int ae_hed_stem_bf16(const void* x, int x_is_f32, long sb, long sc, long sh, long sw, const float* norm, const float* w, const float* bias, void* out,
                     int B, int H, int W, int C1, void* stream);
int ae_relu_bf16(void* x, long n, void* stream);
int ae_hed_tail_bf16(const void* y, const float* wp, const float* bp, float* proj, void* pooled, int B, int H, int W, int C, void* stream);
int ae_hed_fuse(const float* p0, const float* p1, const float* p2, const float* p3, const float* p4, void* out, float* logits, int B, int H, int W,
                int invert, void* stream);

/* ---- Depth Anything V2's DPT head (csrc/dpt.hip; AnyEdit_Collection/other_modules/depth_anything_v2/dpt.py, util/blocks.py) and img2depth's colour map
 * (visual_condition_tool.py:126-134): what stands around the head's convolutions (ae_conv3x3_bf16) and 1x1 products (ae_gemm_bf16).  Bandwidth-bound kernels,
 * 16 bytes per lane (C % 8 == 0), current stream only, no host synchronisation, no allocation, bit-identical from run to run.
 * ae_dpt_reassemble_bf16: projects[i] + resize_layers[i] (dpt.py:127-130) after their products.  prod fp32 [B (1 + gh gw), ldp], row = token (the class row of
 *   every image first), columns (ky k + kx) oc + c: the ConvTranspose2d(kernel = stride = k) product of that token, or with k = 1 the 1x1 product itself.
 *   out bf16 [B, gh k, gw k, oc] = bf16(prod + bias[c]) at pixel (gy k + ky, gx k + kx); the class rows are not read.  k in {1, 2, 4}; ldp % 4 == 0.
 * ae_dpt_resize_bf16: F.interpolate(mode="bilinear", align_corners=True) of x bf16 [B, h, w, C] to out bf16 [B, H, W, C], any two sizes with sides of
 *   1 .. 16384 (a destination side of 1 reads source index 0); source coordinate d (h - 1) / (H - 1) taken in integers.  addend (optional, bf16 [B, H, W, C]) is
 *   added in fp32 before the single rounding (blocks.py:133).  relu_out (optional, bf16 [B, H, W, C]) receives relu(out).
 * ae_dpt_relu_bf16: out = max(x, 0) on n bf16 values, out of place (n % 8 == 0); negative values, -0 and negative NaNs become +0.
 * ae_dpt_tail_bf16: dpt.py:111-114 and :182 on y bf16 [B, H, W, C], the output of output_conv2[0] BEFORE its ReLU: depth fp32 [B, H, W] =
 *   relu(sum_c relu(y)[c] wp[c] + bp), fp32 weights wp [C], bp [1] (on the device), fp32 accumulation.  The reference's third ReLU (:182) is a no-op on it.
 * ae_depth_resize_minmax_f32: dpt.py:192: x fp32 [B, h, w] -> out fp32 [B, H, W], bilinear, align_corners=True; minmax fp32 [B, 2] receives each image's
 *   (minimum, maximum) of the values written, equal to out.amin() / out.amax() bit for bit (integer atomics on the bit patterns; -0 is written as +0).  Two
 *   launches: the reset of minmax, then the resize.
 * ae_depth_colorize_u8: visual_condition_tool.py:131-133: out uint8 [B, H, W, 3] = table[uint8((d - min) / (max - min) * 255.0)] in fp32 with IEEE division
 *   and truncation; minmax fp32 [B, 2] on the device (the buffer ae_depth_resize_minmax_f32 wrote), table uint8 [256, 3].  max == min (0 / 0 in the reference,
 *   undefined there) gives index 0 at every pixel of that image.                                                                                 */
int ae_dpt_reassemble_bf16(const float* prod, long ldp, const float* bias, void* out, int B, int gh, int gw, int k, int oc, void* stream);
int ae_dpt_resize_bf16(const void* x, const void* addend, void* out, void* relu_out, int B, int h, int w, int H, int W, int C, void* stream);
int ae_dpt_relu_bf16(const void* x, void* out, long n, void* stream);
int ae_dpt_tail_bf16(const void* y, const float* wp, const float* bp, float* depth, int B, int H, int W, int C, void* stream);
int ae_depth_resize_minmax_f32(const float* x, float* out, float* minmax, int B, int h, int w, int H, int W, void* stream);
int ae_depth_colorize_u8(const float* depth, const float* minmax, const void* table, void* out, int B, int H, int W, void* stream);

/* ---- UniFormer backbone (csrc/uniformer.hip; AnyEdit_Collection/other_modules/uniformer/mmseg/models/backbones/uniformer.py): what stands around
 * the 1x1 convolutions and Linear layers (ae_gemm_bf16 / ae_ln_gemm_bf16), PatchEmbed's LayerNorm (ae_layernorm_bf16) and the global attention
 * (ae_attn_fwd_bf16).  Activations are channels-last bf16 rows [B, H, W, C], C % 8 == 0.  Bandwidth-bound kernels, 16 bytes per lane, no atomics,
 * fixed summation orders (bit-identical from run to run, an image's rows do not depend on its batch); current stream only, no host
 * synchronisation, no allocation.  Each returns AE_ERR_ARG with a message and launches nothing on a null pointer, a non-positive size,
 * C % 8 != 0, an unsupported k, or a map below the patch.
 * ae_dwconv_rows_bf16: the depthwise convolutions, nn.Conv2d(dim, dim, k, padding=k/2, groups=dim): CBlock.pos_embed (:66, k = 3), CBlock.attn
 *   (:70, k = 5), SABlock.pos_embed (:116, k = 3).  w fp32 [k k, C], tap-major (w[(ky k + kx) C + c] = weight[c, 0, ky, kx]); bias fp32 [C];
 *   residual: optional bf16 [B, H, W, C], may be x itself (`x = x + self.pos_embed(x)`, :78 / :129).  out = bf16(residual + bias + sum w x), fp32
 *   accumulation from the bias in (ky, kx) order, the residual last.  Zero padding by (y, x) within the image.  Out of place: out aliasing x is
 *   refused.  k in {3, 5}.
 * ae_patch2_rows_bf16: the gather of PatchEmbed.proj = nn.Conv2d(kernel_size = stride = 2) (:230, :234) for patch_embed2..4: x bf16 [B, H, W, C] ->
 *   out bf16 [B, H/2, W/2, 4 C], column (2 ky + kx) C + c = x[b, 2 oy + ky, 2 ox + kx, c]; floor division (an odd last row or column is dropped, as
 *   the strided convolution drops it).  A copy: exact.  H, W >= 2.
 * ae_layernorm_rows_nchw: the stage outputs, `norm_i(x.permute(0, 2, 3, 1))` then `.permute(0, 3, 1, 2).contiguous()` (:392-393, :400-401,
 *   :408-409, :416-417): LayerNorm over C (two-pass fp32 statistics) of x bf16 [B, H, W, C], written as out fp32 [B, C, H, W]; the transposition
 *   goes through LDS so that both sides are coalesced.  rows: optional bf16 [B, H, W, C] that receives the same values rounded once (x itself is
 *   allowed).  C <= 1024.                                                                                                                      */
int ae_dwconv_rows_bf16(const void* x, const float* w, const float* bias, const void* residual, void* out, int B, int H, int W, int C, int k, void* stream);
int ae_patch2_rows_bf16(const void* x, void* out, int B, int H, int W, int C, void* stream);
int ae_layernorm_rows_nchw(const void* x, const float* gamma, const float* beta, float eps, float* out, void* rows, int B, int H, int W, int C, void* stream);

/* ---- UPerNet head and the end of EncoderDecoder.simple_test (csrc/upernet.hip; AnyEdit_Collection/other_modules/uniformer/mmseg/models/decode_heads/
 * uper_head.py, psp_head.py, decode_head.py and segmentors/encoder_decoder.py): what stands around the head's ConvModules (ae_conv3x3_bf16, ae_gemm_bf16
 * with EPI_RELU).  Activations are channels-last bf16 rows, C % 8 == 0; every resize is F.interpolate(mode="bilinear", align_corners=False): source
 * coordinate (d + 0.5) n / N - 0.5 clamped at 0 (taken in integers: ((2 d + 1) n - N) / (2 N)), upper neighbour clamped at n - 1, value
 * hy (hx p00 + lx p01) + ly (hx p10 + lx p11) in fp32.  Bandwidth-bound kernels, 16 bytes per lane, no atomics, fixed summation orders (bit-identical
 * from run to run, an image's output does not depend on its batch); current stream only, no host synchronisation, no allocation.  Sides of 1 .. 16384.
 * Each returns AE_ERR_ARG with a message and launches nothing on a null pointer, a bad size, C % 8 != 0, a misaligned pointer or stride, or an aliasing
 * it does not cover.
 * ae_ppm_pool_rows_bf16: every nn.AdaptiveAvgPool2d(s) of PPM (psp_head.py) in one launch.  x bf16 [B, H, W, C]; scales: nscales (1 .. 4) host integers,
 *   each 1 .. 8; out bf16 [B, sum s s, C]: within an image scale k's s_k s_k bins follow scale k - 1's, row-major.  Bin i of an axis of length n covers
 *   floor(i n / s) .. ceil((i + 1) n / s) - 1 (bins overlap when s does not divide n and repeat pixels when n < s); the mean is an fp32 sum (pixels
 *   j, j + S, ... per split, row-major, the splits added in order; S depends on C only) divided by the area, rounded once.
 * ae_resize_concat_rows_bf16: nsrc (1 .. 5) sources, source i bf16 [B, src_h[i], src_w[i], src_c[i]] with row stride src_ld[i] and image stride src_img[i] (elements), resized to
 *   H x W and written to columns dst_col[i] .. dst_col[i] + src_c[i] of dst bf16 [B, H, W] rows of stride ld_dst; the other columns of dst are not
 *   touched.  relu[i] != 0: max(tap, 0) on every tap as it is read (a ConvModule's activation on an output only this kernel reads).  A source of the
 *   destination's size is copied bit for bit (with relu: negative values, -0 and negative NaNs become +0).  addend: optional bf16 rows of stride ld_add,
 *   with nsrc == 1 only, added in fp32 before the single rounding; it may be dst's own slice (`laterals[i - 1] += resize(laterals[i])`,
 *   uper_head.py).  No source may overlap dst.  Strides are multiples of 8 below 2^31 (src_img[i] is not read when B == 1).  The eight arrays are host arrays of nsrc entries.
 * ae_seg_argmax_u8: logits fp32 [B, h, w] rows of stride ld (ld % 4 == 0), classes in columns 0 .. ncls - 1 (ncls <= 256; columns from ncls on are never
 *   read).  Per output pixel of [B, Ho, Wo]: whole_inference's resize (Hm, Wm) -> (Ho, Wo) of encode_decode's resize (h, w) -> (Hm, Wm) (each of the outer
 *   four taps is a four-tap fp32 value; with (Hm, Wm) == (Ho, Wo) the outer stage is the identity and is skipped), then the argmax over the classes, the
 *   lowest index among equal values.  labels uint8 [B, Ho, Wo]; with palette uint8 [ncls, 3] (on the device) also colours uint8 [B, Ho, Wo, 3] =
 *   palette[label] (both or neither).  inference()'s softmax is left out: it is strictly increasing per pixel.                                  */
int ae_ppm_pool_rows_bf16(const void* x, void* out, int B, int H, int W, int C, const int* scales, int nscales, void* stream);
int ae_resize_concat_rows_bf16(const void* const* src, const int* src_h, const int* src_w, const int* src_c, const long* src_ld, const long* src_img,
                               const int* dst_col, const int* relu, int nsrc, const void* addend, long ld_add, void* dst, long ld_dst, int B, int H, int W, void* stream);
int ae_seg_argmax_u8(const float* logits, long ld, int ncls, const void* palette, void* labels, void* colours, int B, int h, int w, int Hm, int Wm, int Ho,
                     int Wo, void* stream);

/* ---- MasaCtrl, mutual self-attention control (csrc/masactrl.hip; AnyEdit_Collection/other_modules/masactrl/masactrl.py, registered on the UNet by
 * masactrl_utils.py::regiter_attention_editor_ldm).  The reference hook is handed sim and attn ([B h, N, N]) of every attention call; these entry points
 * never form them.  No atomics, fixed summation orders (a second call is bit-identical), current stream only, no host synchronisation, no allocation.
 * ae_attn_mutual_bf16: masactrl.py:41-72 (attn_batch / forward: the target's queries on the source's keys and values), :138-193 (mask-guided: sim_fg /
 *   sim_bg = sim + finfo.min on the other class, two softmaxes, the blend by the target mask) and :231-258, :285-334 (the same with generated masks).
 *   Self-attention in which sample b's queries read the keys and values of sample src[b]: out[b] = softmax_j(scale q_b . k_src[b],j) v_src[b],j.
 *   q / k / v bf16 addressed in place through (batch, head, row) element strides as ae_attn_fwd_bf16 takes them (rows 16-byte aligned), out bf16 through
 *   o-strides (multiples of 4); src: B host ints in [0, B), read during the call (B <= 64).  Classes (optional): qcls uint8 [B, N] or NULL, kcls uint8
 *   [B, N] and kcnt int32 [B, 2] (both indexed by src[b]; kcnt[s][c] = number of keys of sample s with class c, as ae_masactrl_classes writes it).  Key j
 *   is allowed for query (b, i) iff qcls is NULL, or qcls[b][i] == 255, or kcls[src[b]][j] == qcls[b][i]; classes are 0 / 1.  A query whose class has
 *   no key in its source (kcnt == 0; also a class byte other than 0, 1, 255) gets the plain mean of V over all keys: the reference adds finfo.min to every
 *   logit, which leaves them all equal in fp32.  One class-matched softmax per row replaces the reference's two softmaxes and its blend (the blend's mask
 *   is 0 / 1, so it selects).  fp32 logits and softmax statistics, bf16 probabilities into the PV product, fp32 accumulation; a key tile with no allowed
 *   key leaves a row's running maximum untouched (no NaN).  head_dim 40, 64, 80, 160 and any N >= 1; anything else: AE_ERR_UNSUPPORTED with a message.
 * ae_attn_token_map_bf16: masactrl.py:277-280 (`attn.reshape(-1, heads, N, Nk).mean(1)` of a 16x16 cross-attention, kept per layer) with the token
 *   selection of aggregate_cross_attn_map (:260-267: `attn_map[..., idx]`, summed over a list) taken at once:
 *     out[b][i] (+)= (1 / H) sum_h sum_{j in set_b} softmax_j(scale q_{b,h,i} . k_{b,h,j}),   out fp32 [B, N] contiguous, accumulate != 0: added to out.
 *   (The reference's mean over the collected layers is a positive factor that its min-max normalisation removes: summing the layers' maps is enough.)
 *   q / k bf16 read in place through (batch, head, row) strides; Nk <= 128, head_dim a multiple of 8 up to 160, B <= 64; token_sets: 2 B host uint64,
 *   bit j % 64 of word 2 b + j / 64 set iff token j belongs to sample b's set.  No PV product; the heads are added in order inside the launch.
 * ae_masactrl_classes: aggregate_cross_attn_map's min-max normalisation (:268-270), F.interpolate(mode="nearest") to the self-attention's resolution
 *   (:303, :315) and the in-place binarisation (:245-247, :321-323) of `npairs` (1 .. 8) maps in one launch, with no read-back.  Pair p reads the S x S
 *   map maps[sample[p] * map_ld ..] (fp32) and writes cls[out_row[p]][R R] (uint8, 1 where (x - min) / (max - min) >= thres at the nearest source pixel
 *   min(floor(dst * S / R), S - 1), fp32 as the reference) and counts[out_row[p]][2] (int32: zeros, ones).  sample / out_row: host arrays.  A constant
 *   map is 0 / 0 = NaN in the reference (its mask then stays NaN); here it gives all-zero classes, i.e. counts (R R, 0).                            */
int ae_attn_mutual_bf16(const void* q, const void* k, const void* v, void* out, int B, int H, int N, int D, long q_sb, long q_sh, long q_sn, long k_sb,
                        long k_sh, long k_sn, long v_sb, long v_sh, long v_sn, long o_sb, long o_sh, long o_sn, float scale, const int* src,
                        const unsigned char* qcls, const unsigned char* kcls, const int* kcnt, void* stream);
int ae_attn_token_map_bf16(const void* q, const void* k, float* out, int B, int H, int N, int Nk, int D, long q_sb, long q_sh, long q_sn, long k_sb,
                           long k_sh, long k_sn, float scale, const unsigned long long* token_sets, int accumulate, void* stream);
int ae_masactrl_classes(const float* maps, long map_ld, int S, int R, float thres, int npairs, const int* sample, const int* out_row, unsigned char* cls,
                        int* counts, void* stream);

/* ---- Prompt-to-Prompt attention control (csrc/prompt2prompt.hip; AnyEdit_Collection/other_modules/prompt2prompt/prompt_to_prompt_stable.py, registered on
 * the UNet by ptp_utils.py:175-273).  The reference hook materialises attention_probs ([B h, N, 77]) of every attention call and edits it in torch; these
 * entry points form no logit or probability buffer.  No atomics, fixed summation orders (a second call is bit-identical), current stream only, no host
 * synchronisation, no allocation.
 * ae_attn_p2p_bf16: prompt_to_prompt_stable.py:183-199 (AttentionControlEdit.forward: attn[1:] = replace_cross_attention(base, own) alpha + (1 - alpha)
 *   own), :216-217 (AttentionReplace: einsum with the mapper), :228-231 (AttentionRefine: gather and alphas), :243-248 (AttentionReweight: the equalizer,
 *   optionally over a previous controller), :132-136 and :138-146 (AttentionStore: the kept maps and their sums over the steps), followed by the
 *   hook's bmm with V (ptp_utils.py:226).  For a sample b with s = base[b] != b, per head:
 *     P_base = softmax_j(scale q_s k_s^T), P_own = softmax_j(scale q_b k_b^T), P' = (P_base M_b) * c_b + P_own * d_b, out_b = P' v_b;
 *   for base[b] == b, P' = P_own.  P' is not renormalised and may be negative.  store[store_row[b]][i][j] (+)= sum_h P'[b,h,i,j] (the head SUM, heads
 *   added in index order; accumulate != 0 adds to the store, 0 overwrites it).  (M, c, d) per controller, a = cross_replace_alpha[cur_step, e]:
 *   Replace (mapper_e, a, 1 - a); Refine (one-hot gather of mapper_e, alphas_e a, 1 - alphas_e a); Reweight (identity, eq_e a, 1 - a); Reweight over a
 *   previous (M0, c0, d0): (M0, c0 eq a, d0 eq a + 1 - a).
 *   q / k / v bf16 read in place through (batch, head, row) element strides as ae_attn_fwd_bf16 takes them (rows 16-byte aligned); out bf16 through
 *   o-strides (multiples of 4), or NULL: no PV product, only the store is written (v may then be NULL).  base, store_row: B host ints read during the
 *   call; base[b] in [0, B) and base[base[b]] == base[b] (a base that is itself edited is refused); store_row[b] in [-1, store_rows), -1 = not stored,
 *   no two samples share a row.  M fp32 [B, Nk, Nk] or NULL: NULL is the identity for every sample (no dense identity is read); c, d fp32 [B, Nk]
 *   (rows of unedited samples are not read); store fp32 [store_rows, N, Nk] or NULL.  fp32 logits, softmax, P_base M, blend and P' V on the VALU (no
 *   bf16 rounding between the operands and the one rounding of the output); a key past Nk has probability exactly 0; query rows past N are clamped for
 *   loads and never stored.  B <= 64, Nk <= 128, head_dim 40 / 64 / 80 / 160, any H, N >= 1; anything else: AE_ERR_UNSUPPORTED with a message.
 * ae_p2p_local_blend_f32: prompt_to_prompt_stable.py:61-73 (LocalBlend.__call__) in one launch with no read-back.  maps: host array of `nlayers`
 *   (1 .. 8) device pointers, each an fp32 [2, S S, Nk] store map (S <= 32); token_sets: 4 host uint64, bit j % 64 of word 2 b + j / 64 set iff token j
 *   is in sample b's set.  m_b[p] = sum_layers sum_{j in set_b} map_l[b][p][j] (the reference's mean over heads and layers is a positive factor its
 *   normalisation removes) -> 3x3 max-pool, stride 1, pad 1 -> nearest resize S -> (h, w), src = min(floor(dst S / out), S - 1) -> divided by the
 *   sample's maximum (fp32 IEEE) -> > threshold -> mask = mask_0 OR mask_1 -> out[1] = mask ? x[1] : x[0], out[0] = x[0].  x, out fp32 [2, C, h, w]
 *   contiguous, out == x allowed.  A map whose maximum is 0 is 0 / 0 = NaN in the reference, which compares false: its mask is 0 here.              */
int ae_attn_p2p_bf16(const void* q, const void* k, const void* v, void* out, int B, int H, int N, int Nk, int D, long q_sb, long q_sh, long q_sn, long k_sb,
                     long k_sh, long k_sn, long v_sb, long v_sh, long v_sn, long o_sb, long o_sh, long o_sn, float scale, const int* base, const float* M,
                     const float* c, const float* d, float* store, const int* store_row, int store_rows, int accumulate, void* stream);
int ae_p2p_local_blend_f32(const float* const* maps, int nlayers, int S, int Nk, const unsigned long long* token_sets, float threshold, const float* x,
                           float* out, int C, int h, int w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ANYEDIT_HIP_H */
