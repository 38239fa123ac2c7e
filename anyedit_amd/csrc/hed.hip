// HED edge detector (AnyEdit_Collection/other_modules/HED/__init__.py: ControlNetHED_Apache2 :34-51, HEDdetector.__call__ :59-74) for gfx950: what
// stands around the twelve 3x3 convolutions that ae_conv3x3_bf16 already runs.  Every kernel here is bandwidth-bound (no MFMA, no atomics, fixed
// summation orders: every launch is deterministic), reads and writes 16 bytes per lane where the layout allows it, and uses no scratch.
//
//   ae_hed_stem_bf16   `x - norm`, the 3 -> C1 3x3 convolution, bias and ReLU (:45 and block1.convs[0]).  K is 27: a direct convolution in fp32
//                      on fp32 weights, one thread per (pixel, 8 output channels); the weights sit transposed in LDS ([tap][channel]) so a thread
//                      reads its 8 channels of a tap as two 16-byte LDS reads.  The zero padding applies to x - norm: a tap outside the image is
//                      0, not -norm * w.  Input by element strides: uint8 [B, H, W, 3] or fp32 [B, 3, H, W] alike.
//   ae_relu_bf16       ReLU in place on bf16 (the convolutions that are not last in their block), on the sign bits.
//   ae_hed_tail_bf16   the end of a block (:26-31) in one pass over its last pre-activation map y: proj = sum_c relu(y)[c] wp[c] + bp in fp32,
//                      and max_pool2d(relu(y), 2, 2) in bf16.  A group of G lanes (G the power of two that covers C / 8, at most 64) owns one
//                      2x2 quad of pixels: each lane holds 8-channel chunks of the four pixels, the pooled chunk is their maximum, the four dot
//                      products are reduced over the group by shuffles.  The full-resolution ReLU map is never written.
//   ae_hed_fuse        :66-73: the five side maps resized to H x W (bilinear, half-pixel centres, edge clamp, scale = src / dst per axis), their
//                      mean, sigmoid, * 255, clip, truncation to uint8, optionally 255 - v.  The source coordinate is taken in integers,
//                      (h (2 y + 1) - H) / (2 H), so the weights carry one fp32 rounding; the sigmoid is fp64 as in the reference (np.float64).
#include "rowwave.hpp"

namespace {

constexpr int HED_STEM_CMAX = 512;   // 28 * C1 floats of LDS (27 taps + bias) stay under 64 KB

template <bool U8>
__device__ __forceinline__ float hed_load(const void* x, long off) {
    if constexpr (U8) return (float)reinterpret_cast<const uint8_t*>(x)[off];
    else return reinterpret_cast<const float*>(x)[off];
}

// one thread per (pixel, 8-channel chunk); wl = [27][C1] weights (tap t = 9 ci + 3 ky + kx, the order of w[c][ci][ky][kx]) then [C1] bias
template <bool U8>
__global__ __launch_bounds__(256) void hed_stem_kernel(const void* __restrict__ x, long sb, long sc, long sh, long sw, const float* __restrict__ norm,
                                                      const float* __restrict__ w, const float* __restrict__ bias, bf16_t* __restrict__ out, int B, int H,
                                                      int W, int C1) {
    extern __shared__ __attribute__((aligned(16))) float wl[];
    for (int i = threadIdx.x; i < 27 * C1; i += blockDim.x) {
        const int c = i / 27, t = i - c * 27;
        wl[t * C1 + c] = w[i];
    }
    for (int i = threadIdx.x; i < C1; i += blockDim.x) wl[27 * C1 + i] = bias[i];
    __syncthreads();
    const float n0 = norm[0], n1 = norm[1], n2 = norm[2];
    const int ncc = C1 / 8;
    const long total = (long)B * H * W * ncc;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
        const long pix = id / ncc;
        const int c = (int)(id - pix * ncc) * 8;
        const long row = pix / W;
        const int px = (int)(pix - row * W);
        const int b = (int)(row / H), py = (int)(row - (long)b * H);
        float tap[27];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int yy = py + ky - 1, xx = px + kx - 1;
                const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
                const long off = (long)b * sb + (long)(in ? yy : 0) * sh + (long)(in ? xx : 0) * sw;
                tap[3 * ky + kx] = in ? hed_load<U8>(x, off) - n0 : 0.f;
                tap[9 + 3 * ky + kx] = in ? hed_load<U8>(x, off + sc) - n1 : 0.f;
                tap[18 + 3 * ky + kx] = in ? hed_load<U8>(x, off + 2 * sc) - n2 : 0.f;
            }
        f32x8 acc = load8_f32(wl + 27 * C1 + c);
#pragma unroll
        for (int t = 0; t < 27; ++t) {
            const f32x8 wt = load8_f32(wl + t * C1 + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc.v[e] = __builtin_fmaf(tap[t], wt.v[e], acc.v[e]);
        }
        float r[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = fmaxf(acc.v[e], 0.f);
        store8_bf16(out + pix * C1 + c, r);
    }
}

// a bf16 pair with the negative halves cleared to +0 (a negative NaN becomes 0 too)
__device__ __forceinline__ uint32_t relu_pair(uint32_t v) { return v & ~(((v >> 15) & 0x00010001u) * 0xffffu); }

__global__ __launch_bounds__(256) void relu_bf16_kernel(bf16_t* __restrict__ x, long n) {
    const long n8 = n / 8;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < n8; id += (long)gridDim.x * blockDim.x) {
        u32x4 v = *reinterpret_cast<const u32x4*>(x + id * 8);
        v = (u32x4){relu_pair(v.x), relu_pair(v.y), relu_pair(v.z), relu_pair(v.w)};
        *reinterpret_cast<u32x4*>(x + id * 8) = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - n8 * 8)) {   // at most 7 trailing elements
        bf16_t& t = x[n8 * 8 + threadIdx.x];
        t = (t & 0x8000u) ? (bf16_t)0 : t;
    }
}

struct bf16x8_f { float v[8]; };
__device__ __forceinline__ bf16x8_f relu8(u32x4 t) {
    t = (u32x4){relu_pair(t.x), relu_pair(t.y), relu_pair(t.z), relu_pair(t.w)};
    return bf16x8_f{{bf16lo(t.x), bf16hi(t.x), bf16lo(t.y), bf16hi(t.y), bf16lo(t.z), bf16hi(t.z), bf16lo(t.w), bf16hi(t.w)}};
}

// G lanes per 2x2 quad (G a power of two, 1 .. 64); the quads tile ceil(H / 2) x ceil(W / 2), so an odd last row or column is projected, not pooled
__global__ __launch_bounds__(256) void hed_tail_kernel(const bf16_t* __restrict__ y, const float* __restrict__ wp, const float* __restrict__ bp,
                                                      float* __restrict__ proj, bf16_t* __restrict__ pooled, int B, int H, int W, int C, int G) {
    const int ncc = C / 8, Hq = (H + 1) / 2, Wq = (W + 1) / 2, Hp = H / 2, Wp = W / 2;
    const long nquad = (long)B * Hq * Wq;
    const int l = threadIdx.x % G, qpb = blockDim.x / G;
    const float bias = bp[0];
    // every lane of a wave runs the same number of trips (the shuffles below need the whole group; a group past the end only skips its loads and stores)
    const long trips = (nquad + (long)gridDim.x * qpb - 1) / ((long)gridDim.x * qpb);
    for (long it = 0; it < trips; ++it) {
        const long q = (it * gridDim.x + blockIdx.x) * qpb + threadIdx.x / G;
        const bool live = q < nquad;
        const long qrow = live ? q / Wq : 0;
        const int qx = live ? (int)(q - qrow * Wq) : 0;
        const int b = (int)(qrow / Hq), qy = (int)(qrow - (long)b * Hq);
        const int y0 = 2 * qy, x0 = 2 * qx;
        const bool has_x = x0 + 1 < W, has_y = y0 + 1 < H;
        const bf16_t* base = y + (((long)b * H + y0) * W + x0) * C;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        if (live)
            for (int cc = l; cc < ncc; cc += G) {
                const int c = cc * 8;
                const f32x8 wv = load8_f32(wp + c);
                const u32x4 zero = (u32x4){0u, 0u, 0u, 0u};
                const bf16x8_f a00 = relu8(*reinterpret_cast<const u32x4*>(base + c));
                const bf16x8_f a01 = relu8(has_x ? *reinterpret_cast<const u32x4*>(base + C + c) : zero);
                const bf16x8_f a10 = relu8(has_y ? *reinterpret_cast<const u32x4*>(base + (long)W * C + c) : zero);
                const bf16x8_f a11 = relu8(has_x && has_y ? *reinterpret_cast<const u32x4*>(base + (long)W * C + C + c) : zero);
                float m[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    s[0] = __builtin_fmaf(a00.v[e], wv.v[e], s[0]);
                    s[1] = __builtin_fmaf(a01.v[e], wv.v[e], s[1]);
                    s[2] = __builtin_fmaf(a10.v[e], wv.v[e], s[2]);
                    s[3] = __builtin_fmaf(a11.v[e], wv.v[e], s[3]);
                    m[e] = fmaxf(fmaxf(a00.v[e], a01.v[e]), fmaxf(a10.v[e], a11.v[e]));
                }
                if (pooled && qy < Hp && qx < Wp) store8_bf16(pooled + (((long)b * Hp + qy) * Wp + qx) * C + c, m);   // bf16 values: the rounding is exact
            }
        for (int o = G >> 1; o > 0; o >>= 1) {
#pragma unroll
            for (int p = 0; p < 4; ++p) s[p] += __shfl_xor(s[p], o, 64);
        }
        if (live && l == 0) {
            float* pr = proj + ((long)b * H + y0) * W + x0;
            pr[0] = s[0] + bias;
            if (has_x) pr[1] = s[1] + bias;
            if (has_y) pr[W] = s[2] + bias;
            if (has_x && has_y) pr[W + 1] = s[3] + bias;
        }
    }
}

struct HedSides { const float* p[5]; };

// index and weight of the bilinear pair along one axis: source coordinate (n (2 d + 1) - N) / (2 N), clamped at 0; the upper neighbour clamped at n - 1
__device__ __forceinline__ void hed_axis(int d, int n, int N, int& i0, int& i1, float& l1) {
    int num = n * (2 * d + 1) - N;            // N <= 16384: below 2^29
    num = num < 0 ? 0 : num;
    const unsigned den = 2u * (unsigned)N;
    i0 = (int)((unsigned)num / den);
    l1 = (float)((unsigned)num - (unsigned)i0 * den) / (float)den;
    if (i0 >= n - 1) { i0 = n - 1; l1 = 0.f; }
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
}

__device__ __forceinline__ float hed_mean_logit(const HedSides& sd, int b, int py, int px, int H, int W) {
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int h = H >> k, w = W >> k;
        int y0, y1, x0, x1;
        float ly, lx;
        hed_axis(py, h, H, y0, y1, ly);
        hed_axis(px, w, W, x0, x1, lx);
        const float* m = sd.p[k] + (long)b * h * w;
        const float top = (1.f - lx) * m[(long)y0 * w + x0] + lx * m[(long)y0 * w + x1];
        const float bot = (1.f - lx) * m[(long)y1 * w + x0] + lx * m[(long)y1 * w + x1];
        sum += (1.f - ly) * top + ly * bot;
    }
    return sum / 5.0f;
}

__device__ __forceinline__ uint32_t hed_grey(float logit, int invert) {
    double v = 255.0 / (1.0 + exp(-(double)logit));
    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
    const uint32_t g = (uint32_t)v;   // truncation, as astype(np.uint8) of a value in [0, 255]
    return invert ? 255u - g : g;
}

// one thread per 4 consecutive output bytes of the flattened [B, H, W] map
__global__ __launch_bounds__(256) void hed_fuse_kernel(HedSides sd, uint8_t* __restrict__ out, float* __restrict__ logits, int B, int H, int W, int invert) {
    const long total = (long)B * H * W, n4 = (total + 3) / 4;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < n4; id += (long)gridDim.x * blockDim.x) {
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long i = id * 4 + j;
            if (i < total) {
                const unsigned row = (unsigned)i / (unsigned)W;   // B H W < 2^31
                const int px = (int)((unsigned)i - row * (unsigned)W);
                const int b = (int)(row / (unsigned)H), py = (int)(row - (unsigned)b * (unsigned)H);
                const float m = hed_mean_logit(sd, b, py, px, H, W);
                if (logits) logits[i] = m;
                word |= hed_grey(m, invert) << (8 * j);
            }
        }
        if (id * 4 + 3 < total) *reinterpret_cast<uint32_t*>(out + id * 4) = word;
        else
            for (long i = id * 4; i < total; ++i) out[i] = (uint8_t)(word >> (8 * (i - id * 4)));
    }
}

unsigned hed_grid(long total, int per_block, long cap = 8192) {
    const long want = (total + per_block - 1) / per_block;
    return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
}

}  // namespace

extern "C" int ae_hed_stem_bf16(const void* x, int x_is_f32, long sb, long sc, long sh, long sw, const float* norm, const float* w, const float* bias, void* out,
                                int B, int H, int W, int C1, void* stream) {
    AE_REQUIRE(x && norm && w && bias && out, "ae_hed_stem_bf16: null pointer");
    AE_REQUIRE(x_is_f32 == 0 || x_is_f32 == 1, "ae_hed_stem_bf16: x_is_f32 must be 0 (uint8) or 1 (fp32), got %d", x_is_f32);
    AE_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 31), "ae_hed_stem_bf16: bad sizes B=%d H=%d W=%d", B, H, W);
    AE_REQUIRE(C1 > 0 && C1 % 8 == 0 && C1 <= HED_STEM_CMAX, "ae_hed_stem_bf16: C1=%d must be a multiple of 8, at most %d", C1, HED_STEM_CMAX);
    AE_REQUIRE(sb >= 0 && sc >= 0 && sh >= 0 && sw >= 0, "ae_hed_stem_bf16: negative stride");
    AE_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)w & 3) == 0 && (!x_is_f32 || ((uintptr_t)x & 3) == 0),
               "ae_hed_stem_bf16: out must be 16-byte aligned, fp32 pointers 4-byte aligned");
    const long total = (long)B * H * W * (C1 / 8);
    const size_t lds = (size_t)28 * C1 * sizeof(float);
    const dim3 grid(hed_grid(total, 256, 2048)), block(256);   // every block stages the weights in LDS once: fewer, longer blocks
    if (x_is_f32)
        hipLaunchKernelGGL(hed_stem_kernel<false>, grid, block, lds, (hipStream_t)stream, x, sb, sc, sh, sw, norm, w, bias, (bf16_t*)out, B, H, W, C1);
    else
        hipLaunchKernelGGL(hed_stem_kernel<true>, grid, block, lds, (hipStream_t)stream, x, sb, sc, sh, sw, norm, w, bias, (bf16_t*)out, B, H, W, C1);
    return ae_check_launch("ae_hed_stem_bf16");
}

extern "C" int ae_relu_bf16(void* x, long n, void* stream) {
    AE_REQUIRE(x, "ae_relu_bf16: null pointer");
    AE_REQUIRE(n > 0, "ae_relu_bf16: bad size n=%ld", n);
    AE_REQUIRE(((uintptr_t)x & 15) == 0, "ae_relu_bf16: x must be 16-byte aligned");
    hipLaunchKernelGGL(relu_bf16_kernel, dim3(hed_grid(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x, n);
    return ae_check_launch("ae_relu_bf16");
}

extern "C" int ae_hed_tail_bf16(const void* y, const float* wp, const float* bp, float* proj, void* pooled, int B, int H, int W, int C, void* stream) {
    AE_REQUIRE(y && wp && bp && proj, "ae_hed_tail_bf16: null pointer");
    AE_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 31), "ae_hed_tail_bf16: bad sizes B=%d H=%d W=%d", B, H, W);
    AE_REQUIRE(C > 0 && C % 8 == 0 && C <= 65536, "ae_hed_tail_bf16: C=%d must be a multiple of 8", C);
    AE_REQUIRE(!pooled || (H >= 2 && W >= 2), "ae_hed_tail_bf16: a %d x %d map has no 2x2 window to pool (pass pooled = NULL)", H, W);
    AE_REQUIRE((((uintptr_t)y | (uintptr_t)wp | (uintptr_t)pooled) & 15) == 0 && (((uintptr_t)bp | (uintptr_t)proj) & 3) == 0,
               "ae_hed_tail_bf16: y, wp and pooled must be 16-byte aligned, bp and proj 4-byte aligned");
    int G = 1;
    while (G < 64 && G < C / 8) G *= 2;
    const long nquad = (long)B * ((H + 1) / 2) * ((W + 1) / 2);
    hipLaunchKernelGGL(hed_tail_kernel, dim3(hed_grid(nquad, 256 / G)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)y, wp, bp, proj, (bf16_t*)pooled, B, H,
                       W, C, G);
    return ae_check_launch("ae_hed_tail_bf16");
}

extern "C" int ae_hed_fuse(const float* p0, const float* p1, const float* p2, const float* p3, const float* p4, void* out, float* logits, int B, int H, int W,
                           int invert, void* stream) {
    AE_REQUIRE(p0 && p1 && p2 && p3 && p4 && out, "ae_hed_fuse: null pointer");
    AE_REQUIRE(B > 0 && H >= 16 && W >= 16 && H <= 16384 && W <= 16384 && (long)B * H * W < (1L << 31),
               "ae_hed_fuse: bad sizes B=%d H=%d W=%d (a side below 16 leaves the fifth map empty; at most 16384)", B, H, W);
    AE_REQUIRE(((uintptr_t)out & 3) == 0 && (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2 | (uintptr_t)p3 | (uintptr_t)p4 | (uintptr_t)logits) & 3) == 0,
               "ae_hed_fuse: every pointer must be 4-byte aligned");
    HedSides sd{{p0, p1, p2, p3, p4}};
    hipLaunchKernelGGL(hed_fuse_kernel, dim3(hed_grid(((long)B * H * W + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, sd, (uint8_t*)out, logits, B, H, W,
                       invert ? 1 : 0);
    return ae_check_launch("ae_hed_fuse");
}
