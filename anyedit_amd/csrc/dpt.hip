// Depth Anything V2's DPT head (AnyEdit_Collection/other_modules/depth_anything_v2/dpt.py: DPTHead :38-150, DepthAnythingV2.forward :176-184, infer_image
// :186-194; util/blocks.py: ResidualConvUnit :29-80, FeatureFusionBlock :83-148) and the colour map of img2depth (visual_condition_tool.py:126-134) for gfx950:
// what stands around the head's 3x3 convolutions (ae_conv3x3_bf16) and 1x1 products (ae_gemm_bf16).  Every kernel here is bandwidth-bound (no MFMA), reads and
// writes 16 bytes per lane where the layout allows it, uses no scratch and allocates nothing; every result is bit-identical from run to run (fixed summation
// orders; the only atomics are integer minima / maxima, which do not depend on their order).
//
//   ae_dpt_reassemble_bf16      the data movement of projects[i] + resize_layers[i] (:127-130).  A ConvTranspose2d with kernel = stride = k is one GEMM on the
//                               token rows, [M, oc] x [oc, k k oc], each token giving its own k x k block of output pixels; this kernel reads that fp32 product,
//                               skips the class row of every image, adds the fp32 bias, rounds once and scatters to the rows of the (gh k) x (gw k) map.  k = 1 is
//                               the plain "patch rows without the class row, + bias" of levels 3 and 4.
//   ae_dpt_resize_bf16          F.interpolate(mode="bilinear", align_corners=True) between any two sizes on channels-last rows (:147, blocks.py:144), optionally
//                               + a second row buffer in fp32 before the single rounding (blocks.py:133 skip_add) and optionally relu(result) as a second output
//                               (the next ResidualConvUnit reads both x and relu(x), blocks.py:67, :80).  The source coordinate dst (h - 1) / (H - 1) is taken in
//                               integers, so a weight carries one fp32 rounding (ae_hed_fuse does the same for its half-pixel grid).
//   ae_dpt_relu_bf16            out = relu(x), out of place (a convolution's output is kept as the skip while its rectified copy feeds the next convolution).
//   ae_dpt_tail_bf16            output_conv2[1 .. 4] and forward's F.relu (:111-114, :182) on the pre-activation rows of output_conv2[0]: ReLU, the C -> 1
//                               projection in fp32, bias, ReLU -> fp32 depth.  The reference applies a third ReLU (:182) to a value that is already >= 0: a no-op,
//                               not repeated here.
//   ae_depth_resize_minmax_f32  infer_image's resize of the depth to the image's size (:192, bilinear, align_corners=True) and, in the same pass, each image's
//                               minimum and maximum of the values written (visual_condition_tool.py:131 depth.min() / depth.max()).
//   ae_depth_colorize_u8        visual_condition_tool.py:131-133: idx = uint8((d - min) / (max - min) * 255.0) in fp32 (IEEE division, truncation), then a
//                               [256, 3] uint8 table.  min and max come from the device buffer of the previous kernel.  max == min (a constant map) is 0 / 0 in
//                               the reference and undefined there; here it gives index 0 everywhere.
#include "rowwave.hpp"

namespace {

constexpr int DPT_MAX_SIDE = 16384;   // d (h - 1) stays below 2^28

unsigned dpt_grid(long total, int per_block, long cap = 8192) {
    const long want = (total + per_block - 1) / per_block;
    return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
}

// a bf16 pair with the negative halves cleared to +0 (a negative NaN becomes 0 too)
__device__ __forceinline__ uint32_t dpt_relu_pair(uint32_t v) { return v & ~(((v >> 15) & 0x00010001u) * 0xffffu); }
__device__ __forceinline__ u32x4 dpt_relu8(u32x4 t) { return (u32x4){dpt_relu_pair(t.x), dpt_relu_pair(t.y), dpt_relu_pair(t.z), dpt_relu_pair(t.w)}; }

__device__ __forceinline__ f32x8 dpt_load8_bf16(const bf16_t* p) {  // 16-byte aligned
    const u32x4 t = *reinterpret_cast<const u32x4*>(p);
    return f32x8{{bf16lo(t.x), bf16hi(t.x), bf16lo(t.y), bf16hi(t.y), bf16lo(t.z), bf16hi(t.z), bf16lo(t.w), bf16hi(t.w)}};
}

// one thread per (output pixel, 8-channel chunk)
__global__ __launch_bounds__(256) void dpt_reassemble_kernel(const float* __restrict__ prod, long ldp, const float* __restrict__ bias, bf16_t* __restrict__ out, int B,
                                                            int gh, int gw, int k, int oc) {
    const int ncc = oc / 8, Ho = gh * k, Wo = gw * k;
    const long total = (long)B * Ho * Wo * ncc;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
        const long pix = id / ncc;
        const int c = (int)(id - pix * ncc) * 8;
        const long row = pix / Wo;
        const int X = (int)(pix - row * Wo);
        const int b = (int)(row / Ho), Y = (int)(row - (long)b * Ho);
        const int gy = Y / k, ky = Y - gy * k, gx = X / k, kx = X - gx * k;
        const long token = (long)b * (1 + gh * gw) + 1 + gy * gw + gx;            // + 1: the class row of image b
        const float* src = prod + token * ldp + (long)(ky * k + kx) * oc + c;
        const f32x8 v = load8_f32(src), bv = load8_f32(bias + c);
        float r[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = v.v[e] + bv.v[e];
        store8_bf16(out + pix * oc + c, r);
    }
}

// index pair and weight of the upper neighbour along one axis, align_corners=True: source coordinate d (n - 1) / (N - 1); N = 1 reads source 0
__device__ __forceinline__ void dpt_axis(int d, int n, int N, int& i0, int& i1, float& l1) {
    if (N <= 1 || n <= 1) { i0 = i1 = 0; l1 = 0.f; return; }
    const unsigned num = (unsigned)d * (unsigned)(n - 1), den = (unsigned)(N - 1);
    i0 = (int)(num / den);
    l1 = (float)(num - (unsigned)i0 * den) / (float)den;
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
}

// one thread per (output pixel, 8-channel chunk)
__global__ __launch_bounds__(256) void dpt_resize_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ addend, bf16_t* __restrict__ out,
                                                        bf16_t* __restrict__ relu_out, int B, int h, int w, int H, int W, int C) {
    const int ncc = C / 8;
    const long total = (long)B * H * W * ncc;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
        const long pix = id / ncc;
        const int c = (int)(id - pix * ncc) * 8;
        const long row = pix / W;
        const int X = (int)(pix - row * W);
        const int b = (int)(row / H), Y = (int)(row - (long)b * H);
        int y0, y1, x0, x1;
        float ly, lx;
        dpt_axis(Y, h, H, y0, y1, ly);
        dpt_axis(X, w, W, x0, x1, lx);
        const bf16_t* base = x + (long)b * h * w * C + c;
        const f32x8 a00 = dpt_load8_bf16(base + ((long)y0 * w + x0) * C), a01 = dpt_load8_bf16(base + ((long)y0 * w + x1) * C);
        const f32x8 a10 = dpt_load8_bf16(base + ((long)y1 * w + x0) * C), a11 = dpt_load8_bf16(base + ((long)y1 * w + x1) * C);
        const float my = 1.f - ly, mx = 1.f - lx;
        float r[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float top = mx * a00.v[e] + lx * a01.v[e];
            const float bot = mx * a10.v[e] + lx * a11.v[e];
            r[e] = my * top + ly * bot;
        }
        if (addend) {
            const f32x8 s = dpt_load8_bf16(addend + pix * C + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] += s.v[e];
        }
        const u32x4 packed = (u32x4){pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]), pack_bf16x2(r[4], r[5]), pack_bf16x2(r[6], r[7])};
        *reinterpret_cast<u32x4*>(out + pix * C + c) = packed;
        if (relu_out) *reinterpret_cast<u32x4*>(relu_out + pix * C + c) = dpt_relu8(packed);     // relu of the ROUNDED value: exactly relu(out)
    }
}

__global__ __launch_bounds__(256) void dpt_relu_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, long n8) {
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < n8; id += (long)gridDim.x * blockDim.x)
        *reinterpret_cast<u32x4*>(out + id * 8) = dpt_relu8(*reinterpret_cast<const u32x4*>(x + id * 8));
}

// G lanes per pixel (G a power of two, 1 .. 64, so a group never straddles a wave); every lane of a wave runs the same number of trips (the shuffles need the
// whole group; a group past the end only skips its loads and its store)
__global__ __launch_bounds__(256) void dpt_tail_kernel(const bf16_t* __restrict__ y, const float* __restrict__ wp, const float* __restrict__ bp,
                                                      float* __restrict__ depth, long npix, int C, int G) {
    const int ncc = C / 8;
    const int l = threadIdx.x % G, ppb = blockDim.x / G;
    const float bias = bp[0];
    const long trips = (npix + (long)gridDim.x * ppb - 1) / ((long)gridDim.x * ppb);
    for (long it = 0; it < trips; ++it) {
        const long p = (it * gridDim.x + blockIdx.x) * ppb + threadIdx.x / G;
        const bool live = p < npix;
        float s = 0.f;
        if (live)
            for (int cc = l; cc < ncc; cc += G) {
                const f32x8 wv = load8_f32(wp + cc * 8);
                const u32x4 t = dpt_relu8(*reinterpret_cast<const u32x4*>(y + p * C + cc * 8));                 // output_conv2[1]
                const float a[8] = {bf16lo(t.x), bf16hi(t.x), bf16lo(t.y), bf16hi(t.y), bf16lo(t.z), bf16hi(t.z), bf16lo(t.w), bf16hi(t.w)};
#pragma unroll
                for (int e = 0; e < 8; ++e) s = __builtin_fmaf(a[e], wv.v[e], s);                              // output_conv2[2]
            }
        for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (live && l == 0) {
            const float d = s + bias;
            depth[p] = d > 0.f ? d : 0.f;      // output_conv2[3]; NaN and -0 become +0.  forward's F.relu (:182) of this value changes nothing.
        }
    }
}

// minimum / maximum of floats as integer atomics on their bit patterns: non-negative floats order as signed integers, negative ones in reverse as unsigned
// integers.  The cell always holds a float; the result does not depend on the order of the updates.  v is never NaN or -0 here (the caller canonicalises).
__device__ __forceinline__ void dpt_atomic_min_f32(float* addr, float v) {
    if (v >= 0.f) atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMax(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void dpt_atomic_max_f32(float* addr, float v) {
    if (v >= 0.f) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}

__global__ __launch_bounds__(256) void depth_minmax_init_kernel(float* __restrict__ minmax, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        minmax[2 * b] = __uint_as_float(0x7f800000u);       // +inf
        minmax[2 * b + 1] = __uint_as_float(0xff800000u);   // -inf
    }
}

// blockIdx.y = image; the blocks of an image stride over its H W output pixels, reduce their minimum and maximum (wave shuffles, then 4 values in LDS) and send
// one pair of atomics each
__global__ __launch_bounds__(256) void depth_resize_minmax_kernel(const float* __restrict__ x, float* __restrict__ out, float* __restrict__ minmax, int h, int w, int H,
                                                                 int W) {
    __shared__ float red[2][4];
    const int b = blockIdx.y;
    const float* m = x + (long)b * h * w;
    float* o = out + (long)b * H * W;
    const int total = H * W;                                    // < 2^31 (checked by the caller)
    float lo = __uint_as_float(0x7f800000u), hi = __uint_as_float(0xff800000u);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int Y = (int)(i / W), X = (int)(i - (long)Y * W);
        int y0, y1, x0, x1;
        float ly, lx;
        dpt_axis(Y, h, H, y0, y1, ly);
        dpt_axis(X, w, W, x0, x1, lx);
        const float top = (1.f - lx) * m[(long)y0 * w + x0] + lx * m[(long)y0 * w + x1];
        const float bot = (1.f - lx) * m[(long)y1 * w + x0] + lx * m[(long)y1 * w + x1];
        float v = (1.f - ly) * top + ly * bot;
        v = v == 0.f ? 0.f : v;                                 // -0 -> +0: one bit pattern per value, as the integer order needs
        o[i] = v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, s, 64));
        hi = fmaxf(hi, __shfl_xor(hi, s, 64));
    }
    const int wave = threadIdx.x / 64;
    if (threadIdx.x % 64 == 0) { red[0][wave] = lo; red[1][wave] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        hi = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
        if (lo <= hi) {                                          // a block that saw no pixel (or only NaNs) sends nothing
            dpt_atomic_min_f32(minmax + 2 * b, lo);
            dpt_atomic_max_f32(minmax + 2 * b + 1, hi);
        }
    }
}

// one thread per 4 consecutive pixels of the flattened [B, H, W] map: 12 output bytes, three aligned words
__global__ __launch_bounds__(256) void depth_colorize_kernel(const float* __restrict__ depth, const float* __restrict__ minmax, const uint8_t* __restrict__ table,
                                                            uint8_t* __restrict__ out, long total, long HW) {
    __shared__ uint8_t lut[768];
    for (int i = threadIdx.x; i < 768; i += blockDim.x) lut[i] = table[i];
    __syncthreads();
    const long n4 = (total + 3) / 4;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < n4; id += (long)gridDim.x * blockDim.x) {
        uint8_t px[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long i = id * 4 + j;
            uint32_t idx = 0;
            if (i < total) {
                const long b = i / HW;
                const float mn = minmax[2 * b], mx = minmax[2 * b + 1];
                const float range = mx - mn;
                if (range > 0.f) {
                    const float t = __fmul_rn(__fdiv_rn(__fsub_rn(depth[i], mn), range), 255.0f);
                    idx = t >= 255.f ? 255u : (t > 0.f ? (uint32_t)t : 0u);     // astype(np.uint8): truncation; t is in [0, 255] for a depth inside [min, max]
                }
            }
            px[3 * j] = lut[3 * idx];
            px[3 * j + 1] = lut[3 * idx + 1];
            px[3 * j + 2] = lut[3 * idx + 2];
        }
        if (id * 4 + 3 < total) {
            uint32_t* o = reinterpret_cast<uint32_t*>(out + id * 12);
#pragma unroll
            for (int q = 0; q < 3; ++q)
                o[q] = (uint32_t)px[4 * q] | ((uint32_t)px[4 * q + 1] << 8) | ((uint32_t)px[4 * q + 2] << 16) | ((uint32_t)px[4 * q + 3] << 24);
        } else {
            const long left = (total - id * 4) * 3;
            for (long q = 0; q < left; ++q) out[id * 12 + q] = px[q];
        }
    }
}

}  // namespace

extern "C" int ae_dpt_reassemble_bf16(const float* prod, long ldp, const float* bias, void* out, int B, int gh, int gw, int k, int oc, void* stream) {
    AE_REQUIRE(prod && bias && out, "ae_dpt_reassemble_bf16: null pointer");
    AE_REQUIRE(k == 1 || k == 2 || k == 4, "ae_dpt_reassemble_bf16: k=%d is not covered (1, 2 or 4: the strides of the head's resize layers)", k);
    AE_REQUIRE(oc > 0 && oc % 8 == 0 && oc <= 65536, "ae_dpt_reassemble_bf16: oc=%d must be a multiple of 8", oc);
    AE_REQUIRE(B > 0 && gh > 0 && gw > 0 && gh * k <= DPT_MAX_SIDE && gw * k <= DPT_MAX_SIDE && (long)B * gh * k * gw * k < (1L << 31),
               "ae_dpt_reassemble_bf16: bad sizes B=%d grid %dx%d k=%d", B, gh, gw, k);
    AE_REQUIRE(ldp >= (long)k * k * oc && ldp % 4 == 0, "ae_dpt_reassemble_bf16: row stride %ld must be a multiple of 4 and at least k*k*oc = %ld", ldp, (long)k * k * oc);
    AE_REQUIRE((((uintptr_t)prod | (uintptr_t)bias | (uintptr_t)out) & 15) == 0, "ae_dpt_reassemble_bf16: every pointer must be 16-byte aligned");
    const long total = (long)B * gh * k * gw * k * (oc / 8);
    hipLaunchKernelGGL(dpt_reassemble_kernel, dim3(dpt_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, prod, ldp, bias, (bf16_t*)out, B, gh, gw, k, oc);
    return ae_check_launch("ae_dpt_reassemble_bf16");
}

extern "C" int ae_dpt_resize_bf16(const void* x, const void* addend, void* out, void* relu_out, int B, int h, int w, int H, int W, int C, void* stream) {
    AE_REQUIRE(x && out, "ae_dpt_resize_bf16: null pointer");
    AE_REQUIRE(C > 0 && C % 8 == 0 && C <= 65536, "ae_dpt_resize_bf16: C=%d must be a multiple of 8", C);
    AE_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && h <= DPT_MAX_SIDE && w <= DPT_MAX_SIDE && H <= DPT_MAX_SIDE && W <= DPT_MAX_SIDE &&
                   (long)B * H * W < (1L << 31) && (long)B * h * w < (1L << 31),
               "ae_dpt_resize_bf16: bad sizes B=%d %dx%d -> %dx%d (sides of 1 .. %d)", B, h, w, H, W, DPT_MAX_SIDE);
    AE_REQUIRE((((uintptr_t)x | (uintptr_t)addend | (uintptr_t)out | (uintptr_t)relu_out) & 15) == 0, "ae_dpt_resize_bf16: every pointer must be 16-byte aligned");
    AE_REQUIRE(out != x && out != addend && (!relu_out || (relu_out != x && relu_out != addend && relu_out != out)),
               "ae_dpt_resize_bf16: the outputs must not alias an input or each other");
    const long total = (long)B * H * W * (C / 8);
    hipLaunchKernelGGL(dpt_resize_kernel, dim3(dpt_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)addend, (bf16_t*)out,
                       (bf16_t*)relu_out, B, h, w, H, W, C);
    return ae_check_launch("ae_dpt_resize_bf16");
}

extern "C" int ae_dpt_relu_bf16(const void* x, void* out, long n, void* stream) {
    AE_REQUIRE(x && out, "ae_dpt_relu_bf16: null pointer");
    AE_REQUIRE(n > 0 && n % 8 == 0, "ae_dpt_relu_bf16: n=%ld must be a positive multiple of 8", n);
    AE_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "ae_dpt_relu_bf16: x and out must be 16-byte aligned");
    hipLaunchKernelGGL(dpt_relu_kernel, dim3(dpt_grid(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)out, n / 8);
    return ae_check_launch("ae_dpt_relu_bf16");
}

extern "C" int ae_dpt_tail_bf16(const void* y, const float* wp, const float* bp, float* depth, int B, int H, int W, int C, void* stream) {
    AE_REQUIRE(y && wp && bp && depth, "ae_dpt_tail_bf16: null pointer");
    AE_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 31), "ae_dpt_tail_bf16: bad sizes B=%d H=%d W=%d", B, H, W);
    AE_REQUIRE(C > 0 && C % 8 == 0 && C <= 65536, "ae_dpt_tail_bf16: C=%d must be a multiple of 8", C);
    AE_REQUIRE((((uintptr_t)y | (uintptr_t)wp) & 15) == 0 && (((uintptr_t)bp | (uintptr_t)depth) & 3) == 0,
               "ae_dpt_tail_bf16: y and wp must be 16-byte aligned, bp and depth 4-byte aligned");
    int G = 1;
    while (G < 64 && G < C / 8) G *= 2;
    const long npix = (long)B * H * W;
    hipLaunchKernelGGL(dpt_tail_kernel, dim3(dpt_grid(npix, 256 / G)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)y, wp, bp, depth, npix, C, G);
    return ae_check_launch("ae_dpt_tail_bf16");
}

extern "C" int ae_depth_resize_minmax_f32(const float* x, float* out, float* minmax, int B, int h, int w, int H, int W, void* stream) {
    AE_REQUIRE(x && out && minmax, "ae_depth_resize_minmax_f32: null pointer");
    AE_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0 && H > 0 && W > 0 && h <= DPT_MAX_SIDE && w <= DPT_MAX_SIDE && H <= DPT_MAX_SIDE && W <= DPT_MAX_SIDE &&
                   (long)B * H * W < (1L << 31) && (long)B * h * w < (1L << 31),
               "ae_depth_resize_minmax_f32: bad sizes B=%d %dx%d -> %dx%d (sides of 1 .. %d, B <= 65535)", B, h, w, H, W, DPT_MAX_SIDE);
    AE_REQUIRE((((uintptr_t)x | (uintptr_t)out | (uintptr_t)minmax) & 3) == 0, "ae_depth_resize_minmax_f32: every pointer must be 4-byte aligned");
    AE_REQUIRE(out != x, "ae_depth_resize_minmax_f32: out must not alias x");
    hipLaunchKernelGGL(depth_minmax_init_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, minmax, B);
    hipLaunchKernelGGL(depth_resize_minmax_kernel, dim3(dpt_grid((long)H * W, 256, 1024), B), dim3(256), 0, (hipStream_t)stream, x, out, minmax, h, w, H, W);
    return ae_check_launch("ae_depth_resize_minmax_f32");
}

extern "C" int ae_depth_colorize_u8(const float* depth, const float* minmax, const void* table, void* out, int B, int H, int W, void* stream) {
    AE_REQUIRE(depth && minmax && table && out, "ae_depth_colorize_u8: null pointer");
    AE_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 31), "ae_depth_colorize_u8: bad sizes B=%d H=%d W=%d", B, H, W);
    AE_REQUIRE((((uintptr_t)depth | (uintptr_t)minmax | (uintptr_t)out) & 3) == 0, "ae_depth_colorize_u8: depth, minmax and out must be 4-byte aligned");
    const long total = (long)B * H * W;
    hipLaunchKernelGGL(depth_colorize_kernel, dim3(dpt_grid((total + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, depth, minmax, (const uint8_t*)table,
                       (uint8_t*)out, total, (long)H * W);
    return ae_check_launch("ae_depth_colorize_u8");
}
