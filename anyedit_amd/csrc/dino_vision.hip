// DINOv2 image encoder (AnyEdit_Collection/other_modules/depth_anything_v2/dinov2.py:44-328 DinoVisionTransformer; ldm/modules/encoders/
// modules.py:279-315 FrozenDinoV2Encoder) for gfx950: the two pieces the library lacked.  The patch im2col (ae_clip_patch_rows_bf16 with the
// ImageNet mean / std), the projections, the LayerNorms, the GELU of the MLP towers and the non-causal attention run on existing entry points;
// LayerScale is folded into the weights at pack time and costs no launch.  This file adds
//
//   ae_dino_embed_bf16     the token rows (dinov2.py:212-219 prepare_tokens_with_masks): out[b, 0] = cls_token + pos[0],
//                          out[b, 1 + i] = patch[b G + i] + patch_bias + pos[1 + i]; patch the fp32 GEMM product, pos the fp32 table
//                          interpolated to this grid.  DINOv2 has no pre-norm: the sum is rounded to bf16 once and stored;
//   ae_swiglu_f32_bf16     the gate of SwiGLUFFN (dinov2_layers/swiglu_ffn.py:29-33): y[m, j] = silu(u[m, j] + b[j]) * (u[m, Hd + j] + b[Hd + j]),
//                          u the fp32 [M, 2 Hd] product of w12 (never rounded), y bf16 with its own leading dimension, columns [Hd, ldy)
//                          written as zeros.
//
// Both are bandwidth-bound elementwise kernels: one thread per 8 output columns, 16-byte loads and one 16-byte store, one rounding to bf16,
// no scratch, no atomics.  The gate is fp32 arithmetic (every step is relatively accurate); the three-term sum of the embedding can cancel, so
// it is taken in fp64 (53 bits hold the sum of three fp32 values of like magnitude exactly) and rounded to fp32 once: an fp32 sum would carry
// the error of its first addition, relative to |patch + bias|, into a result that may be orders of magnitude smaller.
#include "rowwave.hpp"

namespace {

// one thread per (token row, 8-channel chunk): row = b (G + 1) + n, n = 0 the class token, n = 1 + i patch i of sample b
__global__ __launch_bounds__(256) void dino_embed_kernel(const float* __restrict__ patch, long ldp, const float* __restrict__ patch_bias,
                                                        const float* __restrict__ cls, const float* __restrict__ pos, bf16_t* __restrict__ out,
                                                        int B, int G, int C) {
    const int ncc = C / 8, N = G + 1;
    const long total = (long)B * N * ncc;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
        const long row = id / ncc;
        const int c = (int)(id - row * ncc) * 8;
        const int b = (int)(row / N), n = (int)(row - (long)b * N);
        const f32x8 p = load8_f32(pos + (long)n * C + c);
        float r[8];
        if (n == 0) {
            const f32x8 a = load8_f32(cls + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = a.v[e] + p.v[e];
        } else {
            const f32x8 a = load8_f32(patch + ((long)b * G + (n - 1)) * ldp + c), pb = load8_f32(patch_bias + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = (float)(((double)a.v[e] + (double)pb.v[e]) + (double)p.v[e]);   // three terms may cancel: summed exactly, rounded once
        }
        store8_bf16(out + row * C + c, r);
    }
}

// one thread per (row, 8-column chunk) of the OUTPUT's leading dimension: chunks at or past Hd store zeros
__global__ __launch_bounds__(256) void swiglu_kernel(const float* __restrict__ u, long ldu, const float* __restrict__ bias, bf16_t* __restrict__ y, long ldy,
                                                    long M, int Hd) {
    const long nch = ldy / 8;
    const long total = M * nch;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
        const long m = id / nch;
        const int j = (int)(id - m * nch) * 8;
        float r[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (j < Hd) {
            const f32x8 x1 = load8_f32(u + m * ldu + j), x2 = load8_f32(u + m * ldu + Hd + j);
            const f32x8 b1 = load8_f32(bias + j), b2 = load8_f32(bias + Hd + j);
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = silu_f(x1.v[e] + b1.v[e]) * (x2.v[e] + b2.v[e]);
        }
        store8_bf16(y + m * ldy + j, r);
    }
}

unsigned grid_of(long total) {
    const long want = (total + 255) / 256;
    return (unsigned)(want < 4096 ? want : 4096);
}

}  // namespace

extern "C" int ae_dino_embed_bf16(const float* patch, long ldp, const float* patch_bias, const float* cls_token, const float* pos, void* out, int B, int G,
                                  int C, void* stream) {
    AE_REQUIRE(patch && patch_bias && cls_token && pos && out, "ae_dino_embed_bf16: null pointer");
    AE_REQUIRE(B > 0 && G > 0 && C > 0 && (long)B * (G + 1) < (1L << 31), "ae_dino_embed_bf16: bad sizes B=%d G=%d C=%d", B, G, C);
    AE_REQUIRE(C % 8 == 0, "ae_dino_embed_bf16: width %d must be a multiple of 8", C);
    AE_REQUIRE(ldp >= C && ldp % 4 == 0, "ae_dino_embed_bf16: patch row stride %ld must be >= C and a multiple of 4", ldp);
    AE_REQUIRE((((uintptr_t)patch | (uintptr_t)patch_bias | (uintptr_t)cls_token | (uintptr_t)pos | (uintptr_t)out) & 15) == 0,
               "ae_dino_embed_bf16: every pointer must be 16-byte aligned");
    const long total = (long)B * (G + 1) * (C / 8);
    hipLaunchKernelGGL(dino_embed_kernel, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, patch, ldp, patch_bias, cls_token, pos, (bf16_t*)out, B, G, C);
    return ae_check_launch("ae_dino_embed_bf16");
}

extern "C" int ae_swiglu_f32_bf16(const float* u, long ldu, const float* bias, void* y, long ldy, long M, int Hd, void* stream) {
    AE_REQUIRE(u && bias && y, "ae_swiglu_f32_bf16: null pointer");
    AE_REQUIRE(M > 0 && Hd > 0 && M < (1L << 31) && Hd < (1 << 28), "ae_swiglu_f32_bf16: bad sizes M=%ld Hd=%d", M, Hd);
    AE_REQUIRE(Hd % 8 == 0, "ae_swiglu_f32_bf16: hidden width %d must be a multiple of 8", Hd);
    AE_REQUIRE(ldu >= 2L * Hd && ldu % 4 == 0, "ae_swiglu_f32_bf16: u row stride %ld must be >= 2 Hd and a multiple of 4", ldu);
    AE_REQUIRE(ldy >= Hd && ldy % 8 == 0, "ae_swiglu_f32_bf16: y row stride %ld must be >= Hd and a multiple of 8 (columns Hd .. ldy are written as zeros)", ldy);
    AE_REQUIRE((((uintptr_t)u | (uintptr_t)bias | (uintptr_t)y) & 15) == 0, "ae_swiglu_f32_bf16: every pointer must be 16-byte aligned");
    hipLaunchKernelGGL(swiglu_kernel, dim3(grid_of(M * (ldy / 8))), dim3(256), 0, (hipStream_t)stream, u, ldu, bias, (bf16_t*)y, ldy, M, Hd);
    return ae_check_launch("ae_swiglu_f32_bf16");
}
