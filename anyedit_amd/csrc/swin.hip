// GroundingDINO's Swin backbone (GroundingDINO/groundingdino/models/GroundingDINO/backbone/swin_transformer.py) for gfx950: the two pieces the
// library lacked.  Patch embedding, every LayerNorm, qkv / proj / fc1 / fc2, the GELU and the NHWC -> NCHW of the outputs run on existing
// entry points (ae_clip_patch_rows_bf16, ae_gemm_bf16, ae_layernorm_bf16, ae_bias_act_f32_bf16, ae_transpose_last2).  This file adds
//
//   ae_swin_window_attn_bf16   SwinTransformerBlock.forward from the pad after norm1 to the crop (swin_transformer.py:253-292) with the core of
//                              WindowAttention.forward inside it (:140-171): pad, cyclic shift, window partition, softmax(scale q k^T + relative
//                              position bias + shift mask) v, window reverse, shift back, crop — as the ROW ADDRESSING of one attention kernel.
//                              The shift mask of BasicLayer.forward (:417-443) is computed, not read.
//   ae_swin_merge_ln_bf16      PatchMerging.forward up to the norm (:320-337): the 2x2 gather with zero padding of odd maps and the LayerNorm
//                              over 4C in one pass; the `reduction` Linear behind it is an ae_gemm_bf16 without bias.
//
// Window attention: one 256-thread workgroup per (sample, window, head).  The token at in-window position (i, j) of window (wy, wx) has the
// shifted-frame coordinate (ys, xs) = (wy ws + i, wx ws + j) and the image coordinate ((ys + shift) mod Hp, (xs + shift) mod Wp), Hp / Wp the map
// rounded up to whole windows; it is read from that row of the packed qkv rows and its result is written to that row of out.  No partitioned,
// rolled or padded copy of the activation exists.  A token whose image coordinate lies outside the map is a PAD token: the reference pads norm1's
// output with zeros and qkv has a bias, so its key and value are qkv_bias rounded to bf16 (what the GEMM stores for a zero row) and it takes part in
// the softmax as a key; its output row does not exist and is never written.  K and V^T of the (window, head) are staged in LDS once (N = ws^2 <= 256
// keys of head_dim 32: at most 37 KB), each wave owns 16-row query fragments qf = wave, wave + 4, ...  Operand placement, staging, the one-pass
// softmax, PV and the store are the pieces of attn_short.hpp (head_dim 32 is one K step); particular to this kernel are the addressing table, the
// pad keys read from the bias, and the relative-position bias and shift penalty added to the logits.
#include "attn_short.hpp"

namespace {

constexpr int SWIN_D = 32;

struct SwinAttnArgs {
    const bf16_t* qkv; long ldq;
    const float* qkv_bias; const float* bias;
    bf16_t* out; long ldo;
    int H, W, C, nH, ws, shift, N, nWy, nWx, Hp, Wp;
    float scale;
};

// BasicLayer.forward's three slices along one axis of the shifted frame: [0, L - ws), [L - ws, L - shift), [L - shift, L)
__device__ __forceinline__ int shift_region(int p, int L, int ws, int shift) { return p < L - ws ? 0 : (p < L - shift ? 1 : 2); }

__device__ __forceinline__ u32x4 bias_chunk_bf16(const float* b) {  // 8 fp32 bias values -> the 8 bf16 the GEMM stores for an all-zero row
    const f32x4 a = *reinterpret_cast<const f32x4*>(b);
    const f32x4 c = *reinterpret_cast<const f32x4*>(b + 4);
    return (u32x4){pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]), pack_bf16x2(c[0], c[1]), pack_bf16x2(c[2], c[3])};
}

// loader of the window's staged keys: a real token from its image row, a pad token from the bias, no token as zeros
struct WindowRows {
    const bf16_t* base; long ld; const float* bias; const int* sRow;
    __device__ __forceinline__ u32x4 operator()(int key, int c) const {
        const int row = sRow[key];
        return row >= 0 ? *reinterpret_cast<const u32x4*>(base + (long)row * ld + c * 8) : (row == -1 ? bias_chunk_bf16(bias + c * 8) : (u32x4){0u, 0u, 0u, 0u});
    }
};

struct RealKey {  // the keys of the window among the nfrag fragments that were computed
    int nfrag, N, lg;
    __device__ __forceinline__ bool operator()(int kf, int r, float) const { return kf < nfrag && kf * 16 + lg * 4 + r < N; }
};

template <int NKF>  // 16-key fragments a row may span: N <= 16 NKF, NKF even (one PV MFMA contracts two)
__global__ __launch_bounds__(256) void swin_window_attn_kernel(const SwinAttnArgs p) {
    constexpr int NT = 256;
    constexpr int D = SWIN_D;
    constexpr int NS = NKF * 16;                       // staged keys (zeros past N)
    constexpr int KROW = D + 8;                        // LDS row strides (elements), +16 B pad
    constexpr int VROW = (NS + 63) / 64 * 64 + 8;      // V^T is permuted inside whole 64-key tiles
    static_assert(NKF % 2 == 0 && NKF <= 16, "even number of key fragments, at most 256 keys");

    __shared__ __attribute__((aligned(16))) bf16_t sK[NS * KROW];
    __shared__ __attribute__((aligned(16))) bf16_t sVt[D * VROW];
    __shared__ int sRow[NS];                                           // image row of token n; -1 pad token; -2 no such token
    __shared__ __attribute__((aligned(4))) uint8_t sReg[NS];           // shift-mask region 3 r(ys) + r(xs) of token n

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const int N = p.N, ws = p.ws;
    int w = blockIdx.x;
    const int h = w % p.nH; w /= p.nH;
    const int wx = w % p.nWx; w /= p.nWx;
    const int wy = w % p.nWy;
    const int b = w / p.nWy;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    // ---- the addressing: shifted-frame coordinate -> image row (or pad) and mask region, once per token
    for (int n = tid; n < NS; n += NT) {
        int row = -2, reg = 0;
        if (n < N) {
            const int i = n / ws, j = n - i * ws;
            const int ys = wy * ws + i, xs = wx * ws + j;
            int y = ys + p.shift, x = xs + p.shift;
            y = y >= p.Hp ? y - p.Hp : y;
            x = x >= p.Wp ? x - p.Wp : x;
            row = (y < p.H && x < p.W) ? (b * p.H + y) * p.W + x : -1;
            if (p.shift > 0) reg = 3 * shift_region(ys, p.Hp, ws, p.shift) + shift_region(xs, p.Wp, ws, p.shift);
        }
        sRow[n] = row;
        sReg[n] = (uint8_t)reg;
    }
    __syncthreads();

    // ---- stage K rows and V^T columns of all NS keys
    stage_k_rows<D, NT>(sK, NS, tid, WindowRows{p.qkv + p.C + h * D, p.ldq, p.qkv_bias + p.C + h * D, sRow});
    stage_vt<D, NT>(sVt, VROW, NS, tid, WindowRows{p.qkv + 2 * p.C + h * D, p.ldq, p.qkv_bias + 2 * p.C + h * D, sRow});
    __syncthreads();  // the last barrier: nothing below writes LDS

    const int nfrag = (N + 15) >> 4;  // key fragments that hold a real key
    const bool vec_bias = (N & 3) == 0;  // a lane's 4 keys are then all real or all past N, and their bias is one aligned 16-byte read
    const float* hbias = p.bias + (long)h * N * N;

    for (int qf = wave; qf < nfrag; qf += 4) {  // wave-uniform
        const int qrow = qf * 16 + l15;
        const int qc = min(qrow, N - 1);
        const int orow = qrow < N ? sRow[qrow] : -2;  // image row this lane's query reads and writes; < 0: nothing to store
        const int qreg = sReg[qc];

        // Q fragment: rows that are never stored read zeros
        const bf16x8_t qfr[1] = {as_bf16x8(orow >= 0 ? *reinterpret_cast<const u32x4*>(p.qkv + (long)orow * p.ldq + h * D + lg * 8) : zero4)};

        // ---- S^T = K Q^T: lane holds the logits of keys 16 kf + 4 g + r for query l15, fp32, in the exp2 domain
        f32x4 s[NKF];
        float mx = NEG_BIG;
#pragma unroll
        for (int kf = 0; kf < NKF; ++kf) {
            if (kf < nfrag) {
                const int key0 = kf * 16 + lg * 4;
                const f32x4 acc = logit_frag(sK, kf, qfr, l15, lg);
                const float* bp = hbias + (long)qc * N + key0;
                f32x4 bv = {0.f, 0.f, 0.f, 0.f};
                if (vec_bias) {
                    if (key0 < N) bv = *reinterpret_cast<const f32x4*>(bp);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (key0 + r < N) bv[r] = bp[r];
                }
                const uint32_t regs = *reinterpret_cast<const uint32_t*>(sReg + key0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float logit = __builtin_fmaf(acc[r], p.scale, bv[r]);
                    logit += (int)((regs >> (8 * r)) & 0xffu) != qreg ? -100.0f : 0.0f;   // :441 masked_fill(attn_mask != 0, -100.0): a finite penalty, not -inf
                    const float v = key0 + r < N ? logit * LOG2E : NEG_BIG;
                    s[kf][r] = v;
                    mx = fmaxf(mx, v);
                }
            } else {
                s[kf] = (f32x4){NEG_BIG, NEG_BIG, NEG_BIG, NEG_BIG};
            }
        }
        mx = query_max(mx);  // key 0 exists for every row: mx is a real logit
        float rs = 0.f;
#pragma unroll
        for (int kf = 0; kf < NKF; ++kf) s[kf] = exp_frag(s[kf], kf, mx, rs, RealKey{nfrag, N, lg});
        const float inv = 1.0f / query_sum(rs);

        f32x4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int j = 0; j < NKF / 2; ++j)
            if (2 * j < nfrag) pv_step(o, s[2 * j], s[2 * j + 1], sVt, VROW, pv_col(j, lg), l15);
        // store to the token's own image row; pad and padding rows are never stored
        if (orow >= 0) store_o_row(p.out + (long)orow * p.ldo + h * D, o, inv, lg);
    }
}

// One wave per output row: a lane holds chunks lane, lane + 64, ... of the 4C values (8 per chunk, at most 8 chunks: 4C <= 4096).  The statistics
// and the normalisation are fp64: x - mean cancels wherever a value sits next to the row mean, and an fp32 mean (relative error 2^-24 of |mean|)
// would leave such an element further from the exact result than one bf16 rounding allows.  The result is rounded to bf16 once, at the store.
constexpr int MERGE_MAXCH = 8;

__global__ __launch_bounds__(256) void swin_merge_ln_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           bf16_t* __restrict__ y, int H, int W, int C, long rows, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= rows) return;  // no barrier below
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
    const long per = (long)H2 * W2;
    const int b = (int)(row / per);
    const int rem = (int)(row - (long)b * per);
    const int i = rem / W2, j = rem - i * W2;
    const int cch = C / 8, nch = 4 * cch;

    // the 8 bf16 of a chunk stay packed (4 registers per chunk); they are widened where they are used
    u32x4 t[MERGE_MAXCH];
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < MERGE_MAXCH; ++k) {
        const int ch = lane + 64 * k;
        t[k] = (u32x4){0u, 0u, 0u, 0u};
        if (ch < nch) {
            const int q = ch / cch, c = (ch - q * cch) * 8;
            const int yy = 2 * i + (q & 1), xx = 2 * j + (q >> 1);   // :330-334 cat order: (2i, 2j), (2i+1, 2j), (2i, 2j+1), (2i+1, 2j+1)
            if (yy < H && xx < W) t[k] = *reinterpret_cast<const u32x4*>(x + (((long)b * H + yy) * W + xx) * C + c);   // outside the map: the zeros of F.pad, which enter the statistics
        }
        const float v[8] = {bf16lo(t[k].x), bf16hi(t[k].x), bf16lo(t[k].y), bf16hi(t[k].y), bf16lo(t[k].z), bf16hi(t[k].z), bf16lo(t[k].w), bf16hi(t[k].w)};
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += (double)v[e];   // chunks past nch hold zeros
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const double n = 4.0 * C;
    const double mean = sum / n;
    double sq = 0.0;
#pragma unroll
    for (int k = 0; k < MERGE_MAXCH; ++k)
        if (lane + 64 * k < nch) {
            const float v[8] = {bf16lo(t[k].x), bf16hi(t[k].x), bf16lo(t[k].y), bf16hi(t[k].y), bf16lo(t[k].z), bf16hi(t[k].z), bf16lo(t[k].w), bf16hi(t[k].w)};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double d = (double)v[e] - mean;
                sq += d * d;
            }
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    const double rstd = 1.0 / sqrt(sq / n + (double)eps);
#pragma unroll
    for (int k = 0; k < MERGE_MAXCH; ++k) {
        const int ch = lane + 64 * k;
        if (ch < nch) {
            const float v[8] = {bf16lo(t[k].x), bf16hi(t[k].x), bf16lo(t[k].y), bf16hi(t[k].y), bf16lo(t[k].z), bf16hi(t[k].z), bf16lo(t[k].w), bf16hi(t[k].w)};
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + ch * 8), g1 = *reinterpret_cast<const f32x4*>(gamma + ch * 8 + 4);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + ch * 8), b1 = *reinterpret_cast<const f32x4*>(beta + ch * 8 + 4);
            const float g[8] = {g0[0], g0[1], g0[2], g0[3], g1[0], g1[1], g1[2], g1[3]};
            const float be[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
            float r[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = (float)(((double)v[e] - mean) * rstd * (double)g[e] + (double)be[e]);
            *reinterpret_cast<u32x4*>(y + row * (4L * C) + ch * 8) =
                (u32x4){pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]), pack_bf16x2(r[4], r[5]), pack_bf16x2(r[6], r[7])};
        }
    }
}

}  // namespace

extern "C" int ae_swin_window_attn_bf16(const void* qkv, long ldq, const float* qkv_bias, const float* bias, void* out, long ldo, int B, int H, int W,
                                        int C, int nH, int ws, int shift, float scale, void* stream) {
    AE_REQUIRE(qkv && qkv_bias && bias && out, "ae_swin_window_attn_bf16: null pointer");
    AE_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && nH > 0, "ae_swin_window_attn_bf16: bad sizes B=%d H=%d W=%d C=%d heads=%d", B, H, W, C, nH);
    AE_REQUIRE(C % nH == 0 && C / nH == SWIN_D, "ae_swin_window_attn_bf16: head_dim %d/%d must be 32", C, nH);
    AE_REQUIRE(ws >= 1 && ws <= 16, "ae_swin_window_attn_bf16: window size %d must be in [1, 16]", ws);
    AE_REQUIRE(shift >= 0 && shift < ws, "ae_swin_window_attn_bf16: shift %d must be in [0, window size %d)", shift, ws);
    AE_REQUIRE(ldq >= 3L * C && ldq % 8 == 0, "ae_swin_window_attn_bf16: qkv row stride %ld must be >= 3C and a multiple of 8", ldq);
    AE_REQUIRE(ldo >= C && ldo % 8 == 0, "ae_swin_window_attn_bf16: out row stride %ld must be >= C and a multiple of 8", ldo);
    AE_REQUIRE((((uintptr_t)qkv | (uintptr_t)qkv_bias | (uintptr_t)bias | (uintptr_t)out) & 15) == 0,
               "ae_swin_window_attn_bf16: every pointer must be 16-byte aligned");
    AE_REQUIRE((long)B * H * W < (1L << 31), "ae_swin_window_attn_bf16: %ld token rows are past the 2^31 limit", (long)B * H * W);
    SwinAttnArgs a;
    a.qkv = (const bf16_t*)qkv; a.ldq = ldq; a.qkv_bias = qkv_bias; a.bias = bias; a.out = (bf16_t*)out; a.ldo = ldo;
    a.H = H; a.W = W; a.C = C; a.nH = nH; a.ws = ws; a.shift = shift; a.N = ws * ws;
    a.nWy = (H + ws - 1) / ws; a.nWx = (W + ws - 1) / ws; a.Hp = a.nWy * ws; a.Wp = a.nWx * ws; a.scale = scale;
    const long blocks = (long)B * a.nWy * a.nWx * nH;
    AE_REQUIRE(blocks < (1L << 31), "ae_swin_window_attn_bf16: %ld (window, head) blocks are past the grid limit", blocks);
    const dim3 grid((unsigned)blocks), block(256);
    if (a.N <= 64) hipLaunchKernelGGL(swin_window_attn_kernel<4>, grid, block, 0, (hipStream_t)stream, a);
    else if (a.N <= 160) hipLaunchKernelGGL(swin_window_attn_kernel<10>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(swin_window_attn_kernel<16>, grid, block, 0, (hipStream_t)stream, a);
    return ae_check_launch("ae_swin_window_attn_bf16");
}

extern "C" int ae_swin_merge_ln_bf16(const void* x, const float* gamma, const float* beta, void* y, int B, int H, int W, int C, float eps, void* stream) {
    AE_REQUIRE(x && gamma && beta && y, "ae_swin_merge_ln_bf16: null pointer");
    AE_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "ae_swin_merge_ln_bf16: bad sizes B=%d H=%d W=%d C=%d", B, H, W, C);
    AE_REQUIRE(C % 8 == 0, "ae_swin_merge_ln_bf16: width %d must be a multiple of 8", C);
    AE_REQUIRE(4 * C <= 64 * 8 * MERGE_MAXCH, "ae_swin_merge_ln_bf16: merged width 4*%d is past %d", C, 64 * 8 * MERGE_MAXCH);
    AE_REQUIRE((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) & 15) == 0, "ae_swin_merge_ln_bf16: every pointer must be 16-byte aligned");
    const long rows = (long)B * ((H + 1) / 2) * ((W + 1) / 2);
    AE_REQUIRE((long)B * H * W < (1L << 31), "ae_swin_merge_ln_bf16: %ld token rows are past the 2^31 limit", (long)B * H * W);
    hipLaunchKernelGGL(swin_merge_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, gamma, beta, (bf16_t*)y, H, W,
                       C, rows, eps);
    return ae_check_launch("ae_swin_merge_ln_bf16");
}
