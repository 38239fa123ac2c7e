// CLIP vision tower (transformers' CLIPVisionModelWithProjection; train.py:404, 689-691 image_encoder(reference_clip_images,
// output_hidden_states=True).hidden_states[-2]) for gfx950: the three pieces the library lacked.  The projections, the LayerNorms of
// the layers, the fc1 activation and the non-causal attention run on ae_gemm_bf16 / ae_layernorm_bf16 / ae_bias_act_f32_bf16 /
// ae_attn_fwd_bf16; this file adds
//
//   ae_clip_patch_rows_bf16        im2col of CLIPVisionEmbeddings.patch_embedding (a stride-P convolution, no bias) with the image
//                                  processor's rescale + normalise fused in: [B, Cin, H, W] fp32 / bf16 / uint8 -> bf16 rows [B Gh Gw, Kpad],
//                                  pad columns written as zeros;
//   ae_clip_vision_embed_ln_bf16   token rows + pre_layrnorm in one launch: LN(class_embedding + pos[0]) and LN(patch + pos[1 + i]),
//                                  patch the fp32 GEMM product; the un-normalised sum lives in registers only;
//   ae_clip_vision_pool_ln_bf16    post_layernorm of the class rows alone (row b N of a [B N, C] buffer through a row stride).
//
// All three are bandwidth-bound row kernels: fp32 statistics (two passes over registers: mean, then centred variance), one rounding to
// bf16 at the 16-byte store, no scratch, no atomics.  The two LayerNorm kernels give one wave to a row and a lane up to LN_MAXCH chunks
// of 8 channels (wave_ln_store, rowwave.hpp): C <= LN_CMAX = 2048 (ViT-H 1280, ViT-bigG 1664), refused above.
#include "rowwave.hpp"

namespace {

// one wave per token row (b, n): n = 0 the class token, n = 1 + i patch i of sample b
__global__ __launch_bounds__(256) void vision_embed_ln_kernel(const float* __restrict__ patch, long ldp, const float* __restrict__ cls,
                                                             const float* __restrict__ pos, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, bf16_t* __restrict__ out, int B, int G, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int N = G + 1;
    if (row >= (long)B * N) return;
    const int b = (int)(row / N), n = (int)(row - (long)b * N);
    const float* src = n == 0 ? cls : patch + ((long)b * G + (n - 1)) * ldp;
    const float* pr = pos + (long)n * C;
    const int ncc = C / 8;
    f32x8 x[LN_MAXCH];
#pragma unroll
    for (int i = 0; i < LN_MAXCH; ++i) {
        const int cc = lane + i * 64;
        if (cc < ncc) {
            const f32x8 a = load8_f32(src + cc * 8), p = load8_f32(pr + cc * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[i].v[e] = a.v[e] + p.v[e];
        }
    }
    wave_ln_store(x, lane, ncc, C, gamma, beta, eps, out + row * C);
}

// one wave per sample: row b * ldx of the bf16 buffer
__global__ __launch_bounds__(256) void vision_pool_ln_kernel(const bf16_t* __restrict__ xin, long ldx, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, bf16_t* __restrict__ out, int B, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bf16_t* src = xin + b * ldx;
    const int ncc = C / 8;
    f32x8 x[LN_MAXCH];
#pragma unroll
    for (int i = 0; i < LN_MAXCH; ++i) {
        const int cc = lane + i * 64;
        if (cc < ncc) {
            const u32x4 t = *reinterpret_cast<const u32x4*>(src + cc * 8);
            x[i] = f32x8{{bf16lo(t.x), bf16hi(t.x), bf16lo(t.y), bf16hi(t.y), bf16lo(t.z), bf16hi(t.z), bf16lo(t.w), bf16hi(t.w)}};
        }
    }
    wave_ln_store(x, lane, ncc, C, gamma, beta, eps, out + b * C);
}

__device__ __forceinline__ float px_to_f32(float v) { return v; }
__device__ __forceinline__ float px_to_f32(bf16_t v) { return bf16_to_f32(v); }
__device__ __forceinline__ float px_to_f32(unsigned char v) { return (float)v; }

// 8 consecutive pixels of one image row.  VEC: the pointer is aligned to the whole 8-pixel run (32 / 16 / 8 bytes) and the run lies
// in one patch row (P % 8 == 0); otherwise element loads (P = 14: a patch row of fp32 pixels is only 8-byte aligned, and a chunk
// of 8 columns straddles patch rows).
__device__ __forceinline__ f32x8 load8_px(const float* p) { return load8_f32(p); }
__device__ __forceinline__ f32x8 load8_px(const bf16_t* p) {
    const u32x4 t = *reinterpret_cast<const u32x4*>(p);
    return f32x8{{bf16lo(t.x), bf16hi(t.x), bf16lo(t.y), bf16hi(t.y), bf16lo(t.z), bf16hi(t.z), bf16lo(t.w), bf16hi(t.w)}};
}
__device__ __forceinline__ f32x8 load8_px(const unsigned char* p) {
    const u32x2 t = *reinterpret_cast<const u32x2*>(p);
    return f32x8{{(float)(t.x & 255u), (float)((t.x >> 8) & 255u), (float)((t.x >> 16) & 255u), (float)(t.x >> 24),
                  (float)(t.y & 255u), (float)((t.y >> 8) & 255u), (float)((t.y >> 16) & 255u), (float)(t.y >> 24)}};
}

// one thread per (row, 8-column chunk) of the output: one 16-byte store each, pad columns as zeros
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void patch_rows_kernel(const T* __restrict__ x, bf16_t* __restrict__ rows, int B, int Cin, int H, int W, int P, int Kpad,
                                                        float rescale, const float* __restrict__ mean, const float* __restrict__ stdv) {
    const int Gh = H / P, Gw = W / P, PP = P * P, K = Cin * PP, nch = Kpad / 8;
    const long total = (long)B * Gh * Gw * nch;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
        const long row = id / nch;
        const int j0 = (int)(id - row * nch) * 8;
        const int gx = (int)(row % Gw), gy = (int)((row / Gw) % Gh), b = (int)(row / ((long)Gw * Gh));
        float r[8];
        if (VEC && j0 + 8 <= K) {
            const int c = j0 / PP, rem = j0 - c * PP, ky = rem / P, kx = rem - ky * P;
            const f32x8 v = load8_px(x + (((long)b * Cin + c) * H + (gy * P + ky)) * W + gx * P + kx);
            const float m = mean ? mean[c] : 0.f, s = mean ? stdv[c] : 1.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = mean ? __builtin_fmaf(v.v[e], rescale, -m) / s : v.v[e] * rescale;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int j = j0 + e;
                float o = 0.f;
                if (j < K) {
                    const int c = j / PP, rem = j - c * PP, ky = rem / P, kx = rem - ky * P;
                    const float v = px_to_f32(x[(((long)b * Cin + c) * H + (gy * P + ky)) * W + gx * P + kx]);
                    o = mean ? __builtin_fmaf(v, rescale, -mean[c]) / stdv[c] : v * rescale;
                }
                r[e] = o;
            }
        }
        *reinterpret_cast<u32x4*>(rows + row * Kpad + j0) =
            (u32x4){pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]), pack_bf16x2(r[4], r[5]), pack_bf16x2(r[6], r[7])};
    }
}

template <typename T>
void launch_patch_rows(const void* x, void* rows, int B, int Cin, int H, int W, int P, int Kpad, float rescale, const float* mean, const float* stdv,
                       hipStream_t s) {
    const long total = (long)B * (H / P) * (W / P) * (Kpad / 8);
    const long want = (total + 255) / 256;
    const dim3 grid((unsigned)(want < 4096 ? want : 4096)), block(256);
    // the vector path: whole 8-pixel runs inside a patch row (P % 8 == 0; P^2 % 8 == 0 follows, so a run never crosses a channel) that
    // start on their own alignment (W % 8 == 0 and the base pointer aligned to 8 pixels)
    const bool vec = P % 8 == 0 && W % 8 == 0 && ((uintptr_t)x % (8 * sizeof(T) < 16 ? 8 * sizeof(T) : 16)) == 0;
    if (vec) hipLaunchKernelGGL((patch_rows_kernel<T, true>), grid, block, 0, s, (const T*)x, (bf16_t*)rows, B, Cin, H, W, P, Kpad, rescale, mean, stdv);
    else hipLaunchKernelGGL((patch_rows_kernel<T, false>), grid, block, 0, s, (const T*)x, (bf16_t*)rows, B, Cin, H, W, P, Kpad, rescale, mean, stdv);
}

}  // namespace

extern "C" int ae_clip_patch_rows_bf16(const void* x, int x_dtype, void* rows, int B, int Cin, int H, int W, int P, int Kpad, float rescale,
                                       const float* mean, const float* stdv, void* stream) {
    AE_REQUIRE(x && rows, "ae_clip_patch_rows_bf16: null pointer");
    AE_REQUIRE(x_dtype >= 0 && x_dtype <= 2, "ae_clip_patch_rows_bf16: x_dtype must be 0 (fp32), 1 (bf16) or 2 (uint8), got %d", x_dtype);
    AE_REQUIRE(B > 0 && Cin > 0 && H > 0 && W > 0 && P > 0, "ae_clip_patch_rows_bf16: bad sizes B=%d Cin=%d H=%d W=%d P=%d", B, Cin, H, W, P);
    AE_REQUIRE(H % P == 0 && W % P == 0, "ae_clip_patch_rows_bf16: image %dx%d is not a whole number of %dx%d patches", H, W, P, P);
    AE_REQUIRE((long)Cin * P * P < (1L << 24), "ae_clip_patch_rows_bf16: patch of %d x %d x %d values is too large", Cin, P, P);
    AE_REQUIRE(Kpad == (Cin * P * P + 63) / 64 * 64, "ae_clip_patch_rows_bf16: Kpad=%d must be Cin*P*P=%d rounded up to a multiple of 64", Kpad, Cin * P * P);
    AE_REQUIRE((mean == nullptr) == (stdv == nullptr), "ae_clip_patch_rows_bf16: mean and std go together");
    AE_REQUIRE(((uintptr_t)rows & 15) == 0 && ((uintptr_t)x & (x_dtype == 0 ? 3 : x_dtype == 1 ? 1 : 0)) == 0,
               "ae_clip_patch_rows_bf16: rows must be 16-byte aligned, x aligned to its type");
    AE_REQUIRE((long)B * Cin * H * W < (1L << 40) && (long)B * (H / P) * (W / P) < (1L << 31), "ae_clip_patch_rows_bf16: batch too large");
    hipStream_t s = (hipStream_t)stream;
    if (x_dtype == 0) launch_patch_rows<float>(x, rows, B, Cin, H, W, P, Kpad, rescale, mean, stdv, s);
    else if (x_dtype == 1) launch_patch_rows<bf16_t>(x, rows, B, Cin, H, W, P, Kpad, rescale, mean, stdv, s);
    else launch_patch_rows<unsigned char>(x, rows, B, Cin, H, W, P, Kpad, rescale, mean, stdv, s);
    return ae_check_launch("ae_clip_patch_rows_bf16");
}

extern "C" int ae_clip_vision_embed_ln_bf16(const float* patch, long ldp, const float* class_embedding, const float* pos, const float* gamma,
                                            const float* beta, void* out, int B, int G, int C, float eps, void* stream) {
    AE_REQUIRE(patch && class_embedding && pos && gamma && beta && out, "ae_clip_vision_embed_ln_bf16: null pointer");
    AE_REQUIRE(B > 0 && G > 0 && C > 0 && (long)B * (G + 1) < (1L << 31), "ae_clip_vision_embed_ln_bf16: bad sizes B=%d G=%d C=%d", B, G, C);
    AE_REQUIRE(C % 8 == 0, "ae_clip_vision_embed_ln_bf16: width %d must be a multiple of 8", C);
    AE_REQUIRE(C <= LN_CMAX, "ae_clip_vision_embed_ln_bf16: width %d > %d unsupported (a row lives in one wave's registers)", C, LN_CMAX);
    AE_REQUIRE(ldp >= C && ldp % 4 == 0, "ae_clip_vision_embed_ln_bf16: patch row stride %ld must be >= C and a multiple of 4", ldp);
    AE_REQUIRE(eps >= 0.f, "ae_clip_vision_embed_ln_bf16: eps must not be negative");
    AE_REQUIRE((((uintptr_t)patch | (uintptr_t)class_embedding | (uintptr_t)pos | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15) == 0,
               "ae_clip_vision_embed_ln_bf16: every pointer must be 16-byte aligned");
    const long rows = (long)B * (G + 1);
    hipLaunchKernelGGL(vision_embed_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, patch, ldp, class_embedding, pos, gamma,
                       beta, (bf16_t*)out, B, G, C, eps);
    return ae_check_launch("ae_clip_vision_embed_ln_bf16");
}

extern "C" int ae_clip_vision_pool_ln_bf16(const void* x, long row_stride, const float* gamma, const float* beta, void* out, int B, int C, float eps,
                                           void* stream) {
    AE_REQUIRE(x && gamma && beta && out, "ae_clip_vision_pool_ln_bf16: null pointer");
    AE_REQUIRE(B > 0 && C > 0, "ae_clip_vision_pool_ln_bf16: bad sizes B=%d C=%d", B, C);
    AE_REQUIRE(C % 8 == 0, "ae_clip_vision_pool_ln_bf16: width %d must be a multiple of 8", C);
    AE_REQUIRE(C <= LN_CMAX, "ae_clip_vision_pool_ln_bf16: width %d > %d unsupported (a row lives in one wave's registers)", C, LN_CMAX);
    AE_REQUIRE(row_stride >= C && row_stride % 8 == 0, "ae_clip_vision_pool_ln_bf16: row stride %ld must be >= C and a multiple of 8", row_stride);
    AE_REQUIRE(eps >= 0.f, "ae_clip_vision_pool_ln_bf16: eps must not be negative");
    AE_REQUIRE((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15) == 0, "ae_clip_vision_pool_ln_bf16: every pointer must be 16-byte aligned");
    hipLaunchKernelGGL(vision_pool_ln_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, row_stride, gamma, beta,
                       (bf16_t*)out, B, C, eps);
    return ae_check_launch("ae_clip_vision_pool_ln_bf16");
}
