// UniFormer backbone (AnyEdit_Collection/other_modules/uniformer/mmseg/models/backbones/uniformer.py) for gfx950: what stands around the 1x1
// convolutions / Linear layers (ae_gemm_bf16, ae_ln_gemm_bf16), the LayerNorms of PatchEmbed (ae_layernorm_bf16) and the global attention
// (ae_attn_fwd_bf16).  Every kernel here is bandwidth-bound (no MFMA, no atomics, fixed summation orders: every launch is deterministic), moves
// 16 bytes per lane on its bf16 side, and uses no scratch.  Activations are channels-last bf16 rows [B*H*W, C], C % 8 == 0.
//
//   ae_dwconv_rows_bf16      the depthwise k x k convolutions (CBlock.pos_embed / .attn :66, :70; SABlock.pos_embed :116), k in {3, 5}, stride 1,
//                            zero padding k / 2, with the block's `x + pos_embed(x)` fused as an optional residual.  One thread owns 8 channels of
//                            DW_PX = 4 neighbouring pixels of one map row: per kernel row it loads the 4 + k - 1 chunks its pixels share once (16
//                            bytes each, plain global loads: the overlap between threads is served by the caches, no LDS tile) and the k weight
//                            chunks once (k = 5: from an LDS copy of the weights the block makes first).  The padding is decided by (y, x) inside the image, never by the row index: a thread reads neither the
//                            next map row nor the neighbouring image of the batch.
//   ae_patch2_rows_bf16      the im2col of PatchEmbed's Conv2d(kernel = stride = 2) (:230): [B, H, W, C] -> [B, H/2, W/2, 4C], column
//                            (2 ky + kx) C + c, floor on odd sizes (the last row / column is dropped, as the convolution drops it).  A copy.
//   ae_layernorm_rows_nchw   the stage outputs (:392-393 and its three siblings): LayerNorm over C, written as fp32 [B, C, H, W].  A block takes a
//                            tile of TP neighbouring pixels of one image: each wave normalises whole rows in its registers (16-byte loads, two-pass
//                            fp32 statistics) into an LDS tile, then the block writes the tile channel by channel, TP consecutive floats per
//                            channel, so both the bf16 reads and the fp32 writes are coalesced.  Optionally the bf16 rows are written too.
#include "rowwave.hpp"

namespace {

#ifndef AE_DW_LDSW
#define AE_DW_LDSW 1              // 0: every thread reads its weight chunks from global memory (A/B builds)
#endif
constexpr int DW_PX = 4;          // pixels of one map row per thread
constexpr size_t DW_LDS_MAX = 64 * 1024;
constexpr long DW_LDS_BLOCKS = 2048;   // 8 blocks of 256 threads per CU
constexpr int LNT_CMAX = 1024;    // widest row of ae_layernorm_rows_nchw (LN_MAXCH chunks per lane cover 2048; the LDS tile sets this)
constexpr int LNT_LDS = 64 * 1024;

__device__ __forceinline__ void fma8_bf16(float (&acc)[8], u32x4 t, const f32x8& w) {
    acc[0] = __builtin_fmaf(bf16lo(t.x), w.v[0], acc[0]); acc[1] = __builtin_fmaf(bf16hi(t.x), w.v[1], acc[1]);
    acc[2] = __builtin_fmaf(bf16lo(t.y), w.v[2], acc[2]); acc[3] = __builtin_fmaf(bf16hi(t.y), w.v[3], acc[3]);
    acc[4] = __builtin_fmaf(bf16lo(t.z), w.v[4], acc[4]); acc[5] = __builtin_fmaf(bf16hi(t.z), w.v[5], acc[5]);
    acc[6] = __builtin_fmaf(bf16lo(t.w), w.v[6], acc[6]); acc[7] = __builtin_fmaf(bf16hi(t.w), w.v[7], acc[7]);
}

// one thread per (8-channel chunk, group of DW_PX pixels of a map row); w = [K*K][C] tap-major.  acc = bias + taps in (ky, kx) order, + residual last
// LDSW: the block first copies the K*K*C weights and the C biases to LDS ([tap][C], then the bias) and every thread reads its chunks from there
template <int K, bool LDSW>
__global__ __launch_bounds__(256) void dwconv_rows_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         const bf16_t* res, bf16_t* __restrict__ out, int B, int H, int W, int C) {
    constexpr int R = K / 2, NW = DW_PX + K - 1;
    extern __shared__ __attribute__((aligned(16))) float wl[];
    if constexpr (LDSW) {
        for (int i = threadIdx.x * 4; i < K * K * C; i += blockDim.x * 4) *reinterpret_cast<f32x4*>(wl + i) = *reinterpret_cast<const f32x4*>(w + i);
        for (int i = threadIdx.x * 4; i < C; i += blockDim.x * 4) *reinterpret_cast<f32x4*>(wl + K * K * C + i) = *reinterpret_cast<const f32x4*>(bias + i);
        __syncthreads();
    }
    const int ncc = C / 8, nxg = (W + DW_PX - 1) / DW_PX;
    const long total = (long)B * H * nxg * ncc;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
        long t = id / ncc;
        const int c = (int)(id - t * ncc) * 8;
        const long t2 = t / nxg;
        const int x0 = (int)(t - t2 * nxg) * DW_PX;
        const int b = (int)(t2 / H), y = (int)(t2 - (long)b * H);
        const f32x8 bv = LDSW ? load8_f32(wl + K * K * C + c) : load8_f32(bias + c);
        float acc[DW_PX][8];
#pragma unroll
        for (int p = 0; p < DW_PX; ++p)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[p][e] = bv.v[e];
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int yy = y + ky - R;
            if (yy < 0 || yy >= H) continue;                           // zero padding above / below THIS image
            const bf16_t* rowp = x + ((long)b * H + yy) * W * C + c;
            u32x4 win[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const int xx = x0 + j - R;
                win[j] = (xx >= 0 && xx < W) ? *reinterpret_cast<const u32x4*>(rowp + (long)xx * C) : (u32x4){0u, 0u, 0u, 0u};   // left / right of THIS row
            }
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const f32x8 wv = LDSW ? load8_f32(wl + (ky * K + kx) * C + c) : load8_f32(w + (long)(ky * K + kx) * C + c);
#pragma unroll
                for (int p = 0; p < DW_PX; ++p) fma8_bf16(acc[p], win[p + kx], wv);
            }
        }
#pragma unroll
        for (int p = 0; p < DW_PX; ++p)
            if (x0 + p < W) {
                const long o = (((long)b * H + y) * W + x0 + p) * C + c;
                if (res) {
                    f32x8 r{{acc[p][0], acc[p][1], acc[p][2], acc[p][3], acc[p][4], acc[p][5], acc[p][6], acc[p][7]}};
                    add8_bf16(r, res + o);
                    store8_bf16(out + o, r.v);
                } else {
                    store8_bf16(out + o, acc[p]);
                }
            }
    }
}

// one thread per 16 bytes of the output
__global__ __launch_bounds__(256) void patch2_rows_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, int B, int H, int W, int C) {
    const int ncc = C / 8, Ho = H / 2, Wo = W / 2;
    const long total = (long)B * Ho * Wo * 4 * ncc;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
        long t = id / ncc;
        const int c = (int)(id - t * ncc) * 8;
        const int tap = (int)(t & 3);
        t >>= 2;                                      // output pixel
        const long t2 = t / Wo;
        const int ox = (int)(t - t2 * Wo);
        const int b = (int)(t2 / Ho), oy = (int)(t2 - (long)b * Ho);
        const long src = (((long)b * H + 2 * oy + (tap >> 1)) * W + 2 * ox + (tap & 1)) * C + c;     // 2 oy + 1 <= H - 1, 2 ox + 1 <= W - 1
        *reinterpret_cast<u32x4*>(out + id * 8) = *reinterpret_cast<const u32x4*>(x + src);
    }
}

// tile[cc][tp][e] at cc * (9 TP + 1) + 9 tp + e: the odd strides keep both the per-row writes (lanes differ in cc) and the per-channel reads
// (lanes differ in tp) off each other's banks
__global__ __launch_bounds__(256) void layernorm_rows_nchw_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 float eps, float* __restrict__ out, bf16_t* __restrict__ rows, int B, int HW, int C, int TP,
                                                                 int tp_shift) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int ncc = C / 8, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles = (HW + TP - 1) / TP, cstride = 9 * TP + 1;
    for (long t = blockIdx.x; t < (long)B * tiles; t += gridDim.x) {
        const int b = (int)(t / tiles);
        const int p0 = (int)(t - (long)b * tiles) * TP;
        const int np = HW - p0 < TP ? HW - p0 : TP;
        for (int tp = wave; tp < np; tp += 4) {
            const long row = (long)b * HW + p0 + tp;
            f32x8 xv[LN_MAXCH];
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < LN_MAXCH; ++i) {
                const int cc = lane + i * 64;
                xv[i] = f32x8{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
                if (cc < ncc) {
                    add8_bf16(xv[i], x + row * C + cc * 8);
#pragma unroll
                    for (int e = 0; e < 8; ++e) s += xv[i].v[e];
                }
            }
            const float mu = wave_reduce_sum(s) / (float)C;
            float q = 0.f;
#pragma unroll
            for (int i = 0; i < LN_MAXCH; ++i)
                if (lane + i * 64 < ncc) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float d = xv[i].v[e] - mu;
                        q += d * d;
                    }
                }
            const float rstd = rsqrtf(wave_reduce_sum(q) / (float)C + eps);
#pragma unroll
            for (int i = 0; i < LN_MAXCH; ++i) {
                const int cc = lane + i * 64;
                if (cc < ncc) {
                    const f32x8 g = load8_f32(gamma + cc * 8), bt = load8_f32(beta + cc * 8);
                    float r[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        r[e] = (xv[i].v[e] - mu) * rstd * g.v[e] + bt.v[e];
                        tile[cc * cstride + 9 * tp + e] = r[e];
                    }
                    if (rows) store8_bf16(rows + row * C + cc * 8, r);
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < C * TP; i += blockDim.x) {
            const int tp = i & (TP - 1), c = i >> tp_shift;
            if (tp < np) out[((long)b * C + c) * HW + p0 + tp] = tile[(c >> 3) * cstride + 9 * tp + (c & 7)];
        }
        __syncthreads();
    }
}

unsigned uf_grid(long total, int per_block, long cap = 8192) {
    const long want = (total + per_block - 1) / per_block;
    return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
}

bool uf_overlap(const void* a, long abytes, const void* b, long bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

}  // namespace

extern "C" int ae_dwconv_rows_bf16(const void* x, const float* w, const float* bias, const void* residual, void* out, int B, int H, int W, int C, int k,
                                   void* stream) {
    AE_REQUIRE(x && w && bias && out, "ae_dwconv_rows_bf16: null pointer");
    AE_REQUIRE(k == 3 || k == 5, "ae_dwconv_rows_bf16: k=%d is not built (depthwise 3x3 and 5x5 only)", k);
    AE_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 31), "ae_dwconv_rows_bf16: bad sizes B=%d H=%d W=%d", B, H, W);
    AE_REQUIRE(C > 0 && C % 8 == 0 && C <= 65536, "ae_dwconv_rows_bf16: C=%d must be a multiple of 8 (16 bytes per lane)", C);
    AE_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)residual | (uintptr_t)out) & 15) == 0,
               "ae_dwconv_rows_bf16: every pointer must be 16-byte aligned");
    const long bytes = (long)B * H * W * C * 2;
    AE_REQUIRE(!uf_overlap(x, bytes, out, bytes), "ae_dwconv_rows_bf16: out must not alias x (a pixel's neighbours are read after it is written)");
    const long total = (long)B * H * ((W + DW_PX - 1) / DW_PX) * (C / 8);
    const size_t lds = (size_t)(k * k + 1) * C * sizeof(float);
    // k = 5 with the weights in LDS: + 7 % on maps beyond the caches; k = 3 (9 taps) measured 0 .. - 5 % and keeps its global reads; rows
    // too wide for the LDS image read their weights from global memory too
    const bool ldsw = AE_DW_LDSW && k == 5 && lds <= DW_LDS_MAX;
    // with the weights in LDS a block copies them once and then walks the map: a few blocks per CU, not one per 256 threads
    const dim3 grid(uf_grid(total, 256, ldsw ? DW_LDS_BLOCKS : 1L << 20)), block(256);
    const bf16_t *xp = (const bf16_t*)x, *rp = (const bf16_t*)residual;
    bf16_t* op = (bf16_t*)out;
    hipStream_t st = (hipStream_t)stream;
    if (k == 3) hipLaunchKernelGGL((dwconv_rows_kernel<3, false>), grid, block, 0, st, xp, w, bias, rp, op, B, H, W, C);
    else if (ldsw) hipLaunchKernelGGL((dwconv_rows_kernel<5, true>), grid, block, lds, st, xp, w, bias, rp, op, B, H, W, C);
    else hipLaunchKernelGGL((dwconv_rows_kernel<5, false>), grid, block, 0, st, xp, w, bias, rp, op, B, H, W, C);
    return ae_check_launch("ae_dwconv_rows_bf16");
}

extern "C" int ae_patch2_rows_bf16(const void* x, void* out, int B, int H, int W, int C, void* stream) {
    AE_REQUIRE(x && out, "ae_patch2_rows_bf16: null pointer");
    AE_REQUIRE(B > 0 && (long)B * H * W < (1L << 31), "ae_patch2_rows_bf16: bad sizes B=%d H=%d W=%d", B, H, W);
    AE_REQUIRE(H >= 2 && W >= 2, "ae_patch2_rows_bf16: a %d x %d map is below the 2x2 patch", H, W);
    AE_REQUIRE(C > 0 && C % 8 == 0 && C <= 65536, "ae_patch2_rows_bf16: C=%d must be a multiple of 8 (16 bytes per lane)", C);
    AE_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "ae_patch2_rows_bf16: x and out must be 16-byte aligned");
    AE_REQUIRE(!uf_overlap(x, (long)B * H * W * C * 2, out, (long)B * (H / 2) * (W / 2) * 4 * C * 2), "ae_patch2_rows_bf16: out must not alias x");
    const long total = (long)B * (H / 2) * (W / 2) * 4 * (C / 8);
    hipLaunchKernelGGL(patch2_rows_kernel, dim3(uf_grid(total, 256, 1L << 20)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)out, B, H, W, C);
    return ae_check_launch("ae_patch2_rows_bf16");
}

extern "C" int ae_layernorm_rows_nchw(const void* x, const float* gamma, const float* beta, float eps, float* out, void* rows, int B, int H, int W, int C,
                                      void* stream) {
    AE_REQUIRE(x && gamma && beta && out, "ae_layernorm_rows_nchw: null pointer");
    AE_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 31), "ae_layernorm_rows_nchw: bad sizes B=%d H=%d W=%d", B, H, W);
    AE_REQUIRE(C > 0 && C % 8 == 0 && C <= LNT_CMAX, "ae_layernorm_rows_nchw: C=%d must be a multiple of 8, at most %d", C, LNT_CMAX);
    AE_REQUIRE(eps > 0.f, "ae_layernorm_rows_nchw: eps must be positive");
    AE_REQUIRE((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)rows) & 15) == 0 && ((uintptr_t)out & 3) == 0,
               "ae_layernorm_rows_nchw: x, gamma, beta and rows must be 16-byte aligned, out 4-byte aligned");
    const long HW = (long)H * W;
    AE_REQUIRE(!rows || !uf_overlap(x, (long)B * HW * C * 2, rows, (long)B * HW * C * 2) || rows == x,
               "ae_layernorm_rows_nchw: rows must be x itself or a buffer apart from it");
    int TP = 32, shift = 5;                                       // the widest pixel tile whose fp32 image fits the LDS budget
    while (TP > 8 && (long)(C / 8) * (9 * TP + 1) * 4 > LNT_LDS) TP >>= 1, --shift;
    const size_t lds = (size_t)(C / 8) * (9 * TP + 1) * sizeof(float);
    const long tiles = (long)B * ((HW + TP - 1) / TP);
    hipLaunchKernelGGL(layernorm_rows_nchw_kernel, dim3(uf_grid(tiles, 1, 1L << 20)), dim3(256), lds, (hipStream_t)stream, (const bf16_t*)x, gamma, beta, eps, out,
                       (bf16_t*)rows, B, (int)HW, C, TP, shift);
    return ae_check_launch("ae_layernorm_rows_nchw");
}
