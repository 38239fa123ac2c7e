// UPerNet head and the end of EncoderDecoder.simple_test (AnyEdit_Collection/other_modules/uniformer/mmseg/models/decode_heads/uper_head.py,
// psp_head.py, decode_head.py; segmentors/encoder_decoder.py) for gfx950: what stands around the head's 3x3 convolutions (ae_conv3x3_bf16) and 1x1
// products (ae_gemm_bf16).  Every kernel here is bandwidth-bound (no MFMA, no atomics, fixed summation orders: every launch is deterministic and an
// image's output does not depend on its batch), moves 16 bytes per lane, and uses no scratch.  Activations are channels-last bf16 rows, C % 8 == 0.
//
//   ae_ppm_pool_rows_bf16       every AdaptiveAvgPool2d of the pooling pyramid (psp_head.py PPM) in one launch.  One block per output row (a bin of one
//                               scale of one image): its threads are 8-channel chunks x pixel splits; split j sums the bin's pixels j, j + S, ... in
//                               row-major order, the partial sums meet in LDS and are added in split order, then one division by the bin's area.
//   ae_resize_concat_rows_bf16  F.interpolate(mode="bilinear", align_corners=False) of up to five sources into column slices of one destination, with
//                               an optional ReLU on the taps as they are read and an optional addend; one thread per (destination pixel, 8-channel
//                               chunk of one slice).  The source coordinate (2 d + 1) n / (2 N) - 1/2 is taken in integers, so the weight carries a
//                               single rounding.  A source of the destination's size is copied bit for bit.
//   ae_seg_argmax_u8            encode_decode's and whole_inference's two resizes composed per output pixel, the argmax over classes, and the palette
//                               lookup.  A wave takes SEG_PX neighbouring pixels of one output row; a lane owns four classes (16 bytes of a logits
//                               row), so every tap is one coalesced read of the row; the taps stay in registers while the pixels share their source
//                               columns (a 4x upscale reloads them every fourth pixel).  The argmax is taken in the lane, then across the wave with
//                               (value, index) pairs: the larger value, and of equal values the lower index.
#include "rowwave.hpp"

namespace {

#ifndef AE_SEG_WIDE
#define AE_SEG_WIDE 1             // 0: the identity-size segment map runs the per-pixel wave reduction of the two-stage kernel (A/B builds)
#endif
constexpr int UP_MAX_SIDE = 16384;
constexpr int PPM_MAX_SCALES = 4, PPM_MAX_SCALE = 8;
constexpr int RC_MAX_SRC = 5;
constexpr int SEG_PX = 8;         // output pixels of one row per wave
constexpr int SEG_MAX_CLS = 256;  // 64 lanes x 4 classes

struct PpmScales { int s[PPM_MAX_SCALES]; };

struct RcSource {
    const bf16_t* p;
    int ld, img;      // row stride and image stride in elements (below 2^31: the entry point checks)
    int h, w, C, col, relu;
};
struct RcArgs { RcSource s[RC_MAX_SRC]; };

// align_corners=False along one axis: source coordinate ((2 d + 1) n - N) / (2 N) clamped at 0, upper neighbour clamped at n - 1
__device__ __forceinline__ void half_pixel_src(int d, int n, int N, int& i0, int& i1, float& l1) {
    int num = (2 * d + 1) * n - N;                 // below 2^29 for sides up to 16384
    num = num < 0 ? 0 : num;
    const int den = 2 * N;
    i0 = num / den;                                // at most n - 1: num < 2 N n - N
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l1 = (float)(num - i0 * den) / (float)den;
}

__device__ __forceinline__ f32x8 widen8(u32x4 t, bool relu) {
    f32x8 r{{bf16lo(t.x), bf16hi(t.x), bf16lo(t.y), bf16hi(t.y), bf16lo(t.z), bf16hi(t.z), bf16lo(t.w), bf16hi(t.w)}};
    if (relu) {
#pragma unroll
        for (int e = 0; e < 8; ++e) r.v[e] = fmaxf(r.v[e], 0.f);
    }
    return r;
}

// one block per output row; blockDim.x = 256
__global__ __launch_bounds__(256) void ppm_pool_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, int H, int W, int C, PpmScales sc, int nscales,
                                                      int bins_per_image) {
    __shared__ __attribute__((aligned(16))) float part[256 * 8];
    const int row = blockIdx.x, b = row / bins_per_image;
    int k = row - b * bins_per_image, s = sc.s[0];
#pragma unroll
    for (int i = 0; i < PPM_MAX_SCALES - 1; ++i)
        if (i < nscales - 1 && k >= s * s) {
            k -= s * s;
            s = sc.s[i + 1];
        }
    const int by = k / s, bx = k - by * s;
    const int y0 = by * H / s, y1 = ((by + 1) * H + s - 1) / s, x0 = bx * W / s, x1 = ((bx + 1) * W + s - 1) / s;
    const int bw = x1 - x0, np = (y1 - y0) * bw;
    const int ncc = C / 8, lanes_c = ncc < 256 ? ncc : 256, nsplit = 256 / lanes_c;
    const int cl = threadIdx.x % lanes_c, sp = threadIdx.x / lanes_c;
    const bf16_t* img = x + (long)b * H * W * C;
    for (int c0 = 0; c0 < ncc; c0 += lanes_c) {                    // the same trip count for every thread of the block
        const int cc = c0 + cl;
        const bool live = sp < nsplit && cc < ncc;
        f32x8 acc{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
        if (live)
            for (int p = sp; p < np; p += nsplit) {
                const int py = p / bw, px = p - py * bw;
                add8_bf16(acc, img + ((long)(y0 + py) * W + x0 + px) * C + cc * 8);
            }
        float* mine = part + threadIdx.x * 8;
        *reinterpret_cast<f32x4*>(mine) = (f32x4){acc.v[0], acc.v[1], acc.v[2], acc.v[3]};
        *reinterpret_cast<f32x4*>(mine + 4) = (f32x4){acc.v[4], acc.v[5], acc.v[6], acc.v[7]};
        __syncthreads();
        if (live && sp == 0) {
            for (int j = 1; j < nsplit; ++j) {
                const f32x8 o = load8_f32(part + (j * lanes_c + cl) * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc.v[e] += o.v[e];
            }
            const float area = (float)np;
            float r[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = acc.v[e] / area;
            store8_bf16(out + (long)row * C + cc * 8, r);
        }
        __syncthreads();
    }
}

// one thread per (destination pixel, 8-channel chunk of one slice); chunks = the slices' chunks summed
__global__ __launch_bounds__(256) void resize_concat_kernel(RcArgs a, int nsrc, const bf16_t* addend, long ld_add, bf16_t* dst, long ld_dst, int B, int H,
                                                           int W, int chunks) {
    const long total = (long)B * H * W * chunks;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
        const long pix = id / chunks;
        int cc = (int)(id - pix * chunks);
        RcSource s = a.s[0];
#pragma unroll
        for (int i = 1; i < RC_MAX_SRC; ++i)
            if (i < nsrc && cc >= s.C / 8) {
                cc -= s.C / 8;
                s = a.s[i];
            }
        const long t = pix / W;
        const int ox = (int)(pix - t * W);
        const int b = (int)(t / H), oy = (int)(t - (long)b * H);
        const int c = cc * 8;
        bf16_t* o = dst + pix * ld_dst + s.col + c;
        const bf16_t* src = s.p + (long)b * s.img + c;
        if (s.h == H && s.w == W && !addend) {                      // the same size: a copy, bit for bit (the ReLU on the bit patterns)
            u32x4 v = *reinterpret_cast<const u32x4*>(src + ((long)oy * W + ox) * (long)s.ld);
            if (s.relu) {
                uint32_t* q = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
                for (int e = 0; e < 4; ++e) q[e] &= ((q[e] & 0x8000u) ? 0xffff0000u : 0xffffffffu) & ((q[e] & 0x80000000u) ? 0x0000ffffu : 0xffffffffu);
            }
            *reinterpret_cast<u32x4*>(o) = v;
            continue;
        }
        int ya, yb, xa, xb;
        float ly, lx;
        half_pixel_src(oy, s.h, H, ya, yb, ly);
        half_pixel_src(ox, s.w, W, xa, xb, lx);
        const bool relu = s.relu != 0;
        const f32x8 p00 = widen8(*reinterpret_cast<const u32x4*>(src + ((long)ya * s.w + xa) * (long)s.ld), relu);
        const f32x8 p01 = widen8(*reinterpret_cast<const u32x4*>(src + ((long)ya * s.w + xb) * (long)s.ld), relu);
        const f32x8 p10 = widen8(*reinterpret_cast<const u32x4*>(src + ((long)yb * s.w + xa) * (long)s.ld), relu);
        const f32x8 p11 = widen8(*reinterpret_cast<const u32x4*>(src + ((long)yb * s.w + xb) * (long)s.ld), relu);
        const float hy = 1.f - ly, hx = 1.f - lx;
        f32x8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r.v[e] = hy * (hx * p00.v[e] + lx * p01.v[e]) + ly * (hx * p10.v[e] + lx * p11.v[e]);
        if (addend) add8_bf16(r, addend + pix * ld_add + c);
        store8_bf16(o, r.v);
    }
}

struct SegTaps { f32x4 p00, p01, p10, p11; };

// a lane's four classes [4 lane, 4 lane + 4) of one logits row; classes from ncls on are not read (zeros stand in; the argmax masks them)
__device__ __forceinline__ f32x4 seg_load(const float* __restrict__ row, int lane, int ncls) {
    const int c = 4 * lane;
    if (c + 4 <= ncls) return *reinterpret_cast<const f32x4*>(row + c);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (c < ncls) v[0] = row[c];
    if (c + 1 < ncls) v[1] = row[c + 1];
    if (c + 2 < ncls) v[2] = row[c + 2];
    return v;
}

__device__ __forceinline__ SegTaps seg_taps(const float* __restrict__ img, long ld, int w, int ya, int yb, int xa, int xb, int lane, int ncls) {
    SegTaps t;
    t.p00 = seg_load(img + ((long)ya * w + xa) * ld, lane, ncls);
    t.p01 = seg_load(img + ((long)ya * w + xb) * ld, lane, ncls);
    t.p10 = seg_load(img + ((long)yb * w + xa) * ld, lane, ncls);
    t.p11 = seg_load(img + ((long)yb * w + xb) * ld, lane, ncls);
    return t;
}

__device__ __forceinline__ f32x4 seg_blend(const SegTaps& t, float ly, float lx) {
    const float hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * t.p00 + lx * t.p01) + ly * (hx * t.p10 + lx * t.p11);
}

// the value of the (Hm, Wm) map at (Y, X): encode_decode's resize of the (h, w) logits
__device__ __forceinline__ f32x4 seg_mid(const float* __restrict__ img, long ld, int h, int w, int Hm, int Wm, int Y, int X, int lane, int ncls) {
    int ya, yb, xa, xb;
    float ly, lx;
    half_pixel_src(Y, h, Hm, ya, yb, ly);
    half_pixel_src(X, w, Wm, xa, xb, lx);
    return seg_blend(seg_taps(img, ld, w, ya, yb, xa, xb, lane, ncls), ly, lx);
}

// one wave per SEG_PX neighbouring pixels of an output row.  TWO: whole_inference's resize (Hm, Wm) -> (Ho, Wo) on top of encode_decode's
template <bool TWO>
__global__ __launch_bounds__(256) void seg_argmax_kernel(const float* __restrict__ logits, long ld, int ncls, const uint8_t* __restrict__ palette,
                                                        uint8_t* __restrict__ labels, uint8_t* __restrict__ colours, int B, int h, int w, int Hm, int Wm, int Ho,
                                                        int Wo) {
    const int lane = threadIdx.x & 63;
    const int segs = (Wo + SEG_PX - 1) / SEG_PX;
    const long total = (long)B * Ho * segs, nwaves = (long)gridDim.x * (blockDim.x >> 6);
    for (long id = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); id < total; id += nwaves) {
        const long t = id / segs;
        const int ox0 = (int)(id - t * segs) * SEG_PX;
        const int b = (int)(t / Ho), oy = (int)(t - (long)b * Ho);
        const float* img = logits + (long)b * h * w * ld;
        const int npx = Wo - ox0 < SEG_PX ? Wo - ox0 : SEG_PX;
        int ya, yb;
        float ly;
        half_pixel_src(oy, TWO ? Hm : h, Ho, ya, yb, ly);
        SegTaps taps{};
        int have_a = -1, have_b = -1;
        int mine = 0;                                   // the label of pixel lane (labels) / lane / 3 (colours): the two uses agree on lanes 0 .. 2 only,
        int mine_c = 0;                                 // so two registers
        for (int p = 0; p < npx; ++p) {
            int xa, xb;
            float lx;
            half_pixel_src(ox0 + p, TWO ? Wm : w, Wo, xa, xb, lx);
            f32x4 v;
            if constexpr (TWO) {
                SegTaps m;
                m.p00 = seg_mid(img, ld, h, w, Hm, Wm, ya, xa, lane, ncls);
                m.p01 = seg_mid(img, ld, h, w, Hm, Wm, ya, xb, lane, ncls);
                m.p10 = seg_mid(img, ld, h, w, Hm, Wm, yb, xa, lane, ncls);
                m.p11 = seg_mid(img, ld, h, w, Hm, Wm, yb, xb, lane, ncls);
                v = seg_blend(m, ly, lx);
            } else {
                if (xa != have_a || xb != have_b) {     // wave-uniform: the taps stay while the pixels share their source columns
                    taps = seg_taps(img, ld, w, ya, yb, xa, xb, lane, ncls);
                    have_a = xa, have_b = xb;
                }
                v = seg_blend(taps, ly, lx);
            }
            float best = 4 * lane < ncls ? v[0] : -__builtin_inff();      // a class the row does not have never wins
            int arg = 4 * lane;
#pragma unroll
            for (int e = 1; e < 4; ++e)
                if (4 * lane + e < ncls && v[e] > best) best = v[e], arg = 4 * lane + e;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(best, o, 64);
                const int oa = __shfl_xor(arg, o, 64);
                if (ov > best || (ov == best && oa < arg)) best = ov, arg = oa;
            }
            arg = arg < ncls ? arg : ncls - 1;          // only NaN logits can leave a lane with a class it never read: keep the palette read in bounds
            if (lane == p) mine = arg;
            if (lane / 3 == p) mine_c = arg;
        }
        const long o = ((long)b * Ho + oy) * Wo + ox0;
        if (lane < npx) labels[o + lane] = (uint8_t)mine;
        if (colours && lane < 3 * npx) colours[o * 3 + lane] = palette[mine_c * 3 + lane % 3];
    }
}

__device__ __forceinline__ void seg_better(float& bv, int& ba, float ov, int oa) {
    if (ov > bv || (ov == bv && oa < ba)) bv = ov, ba = oa;
}

// The identity-size form (whole_inference's resize skipped).  The wave's SEG_PX = 8 pixels are reduced together: lane l computes the x taps of pixel
// l & 7 once and the pixel loop reads them with v_readlane (wave-uniform, so the tap reload is a scalar branch); every lane ends the loop with a (value,
// index) pair per pixel, and the butterfly halves the pixels a lane still carries at each of its first three steps (4 + 2 + 1 exchanges), then
// finishes the one pixel left with three more: 10 exchanges of a pair instead of 8 x 6.  Lanes 8 q .. 8 q + 7 end with pixel q.
__global__ __launch_bounds__(256) void seg_argmax_wide_kernel(const float* __restrict__ logits, long ld, int ncls, const uint8_t* __restrict__ palette,
                                                             uint8_t* __restrict__ labels, uint8_t* __restrict__ colours, int B, int h, int w, int Ho, int Wo) {
    static_assert(SEG_PX == 8, "the butterfly below carries 8 pixels");
    const int lane = threadIdx.x & 63;
    const int segs = (Wo + SEG_PX - 1) / SEG_PX;
    const long total = (long)B * Ho * segs, nwaves = (long)gridDim.x * (blockDim.x >> 6);
    for (long id = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); id < total; id += nwaves) {
        const long t = id / segs;
        const int ox0 = (int)(id - t * segs) * SEG_PX;
        const int b = (int)(t / Ho), oy = (int)(t - (long)b * Ho);
        const float* img = logits + (long)b * h * w * ld;
        const int npx = Wo - ox0 < SEG_PX ? Wo - ox0 : SEG_PX;
        int ya, yb, mxa, mxb;
        float ly, mlx;
        half_pixel_src(oy, h, Ho, ya, yb, ly);
        const int mypx = ox0 + (lane & 7);
        half_pixel_src(mypx < Wo ? mypx : Wo - 1, w, Wo, mxa, mxb, mlx);       // past the row's end: the last pixel again, computed and not stored
        float bv[SEG_PX];
        int ba[SEG_PX];
        SegTaps taps{};
        int have_a = -1, have_b = -1;
#pragma unroll
        for (int p = 0; p < SEG_PX; ++p) {
            const int xa = __builtin_amdgcn_readlane(mxa, p), xb = __builtin_amdgcn_readlane(mxb, p);
            const float lx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mlx), p));
            if (xa != have_a || xb != have_b) {
                taps = seg_taps(img, ld, w, ya, yb, xa, xb, lane, ncls);
                have_a = xa, have_b = xb;
            }
            const f32x4 v = seg_blend(taps, ly, lx);
            float best = 4 * lane < ncls ? v[0] : -__builtin_inff();      // a class the row does not have never wins
            int arg = 4 * lane;
#pragma unroll
            for (int e = 1; e < 4; ++e)
                if (4 * lane + e < ncls && v[e] > best) best = v[e], arg = 4 * lane + e;
            bv[p] = best, ba[p] = arg;
        }
        const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
        float cv[4], dv[2];
        int ca[4], da[2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                   // lanes 32 .. 63 keep pixels 4 .. 7 and hand over 0 .. 3, the lower half the reverse
            cv[j] = h5 ? bv[4 + j] : bv[j], ca[j] = h5 ? ba[4 + j] : ba[j];
            seg_better(cv[j], ca[j], __shfl_xor(h5 ? bv[j] : bv[4 + j], 32, 64), __shfl_xor(h5 ? ba[j] : ba[4 + j], 32, 64));
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            dv[j] = h4 ? cv[2 + j] : cv[j], da[j] = h4 ? ca[2 + j] : ca[j];
            seg_better(dv[j], da[j], __shfl_xor(h4 ? cv[j] : cv[2 + j], 16, 64), __shfl_xor(h4 ? ca[j] : ca[2 + j], 16, 64));
        }
        float best = h3 ? dv[1] : dv[0];
        int arg = h3 ? da[1] : da[0];
        seg_better(best, arg, __shfl_xor(h3 ? dv[0] : dv[1], 8, 64), __shfl_xor(h3 ? da[0] : da[1], 8, 64));
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) seg_better(best, arg, __shfl_xor(best, o, 64), __shfl_xor(arg, o, 64));
        arg = arg < ncls ? arg : ncls - 1;              // only NaN logits can leave a lane with a class it never read: keep the palette read in bounds
        const int q = lane >> 3, r = lane & 7;          // this lane's pixel of the segment
        const long o = ((long)b * Ho + oy) * Wo + ox0 + q;
        if (q < npx && r == 0) labels[o] = (uint8_t)arg;
        if (colours && q < npx && r < 3) colours[o * 3 + r] = palette[arg * 3 + r];
    }
}

bool up_overlap(const void* a, long abytes, const void* b, long bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

unsigned up_grid(long want, long cap) { return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap)); }

bool up_side(int v) { return v >= 1 && v <= UP_MAX_SIDE; }

}  // namespace

extern "C" int ae_ppm_pool_rows_bf16(const void* x, void* out, int B, int H, int W, int C, const int* scales, int nscales, void* stream) {
    AE_REQUIRE(x && out && scales, "ae_ppm_pool_rows_bf16: null pointer");
    AE_REQUIRE(B > 0 && up_side(H) && up_side(W) && (long)B * H * W < (1L << 31), "ae_ppm_pool_rows_bf16: bad sizes B=%d H=%d W=%d", B, H, W);
    AE_REQUIRE(C > 0 && C % 8 == 0 && C <= 65536, "ae_ppm_pool_rows_bf16: C=%d must be a multiple of 8 (16 bytes per lane)", C);
    AE_REQUIRE(nscales >= 1 && nscales <= PPM_MAX_SCALES, "ae_ppm_pool_rows_bf16: %d scales: one launch takes 1 .. %d", nscales, PPM_MAX_SCALES);
    PpmScales sc{};
    int bins = 0;
    for (int i = 0; i < nscales; ++i) {
        AE_REQUIRE(scales[i] >= 1 && scales[i] <= PPM_MAX_SCALE, "ae_ppm_pool_rows_bf16: pool scale %d is outside 1 .. %d", scales[i], PPM_MAX_SCALE);
        sc.s[i] = scales[i];
        bins += scales[i] * scales[i];
    }
    AE_REQUIRE((long)B * bins < (1L << 31), "ae_ppm_pool_rows_bf16: bad sizes B=%d with %d bins per image", B, bins);
    AE_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "ae_ppm_pool_rows_bf16: x and out must be 16-byte aligned");
    AE_REQUIRE(!up_overlap(x, (long)B * H * W * C * 2, out, (long)B * bins * C * 2), "ae_ppm_pool_rows_bf16: out must not alias x");
    hipLaunchKernelGGL(ppm_pool_kernel, dim3((unsigned)(B * bins)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)out, H, W, C, sc, nscales, bins);
    return ae_check_launch("ae_ppm_pool_rows_bf16");
}

extern "C" int ae_resize_concat_rows_bf16(const void* const* src, const int* src_h, const int* src_w, const int* src_c, const long* src_ld, const long* src_img,
                                          const int* dst_col, const int* relu, int nsrc, const void* addend, long ld_add, void* dst, long ld_dst, int B, int H, int W,
                                          void* stream) {
    AE_REQUIRE(src && src_h && src_w && src_c && src_ld && src_img && dst_col && relu && dst, "ae_resize_concat_rows_bf16: null pointer");
    AE_REQUIRE(nsrc >= 1 && nsrc <= RC_MAX_SRC, "ae_resize_concat_rows_bf16: %d sources: one launch takes 1 .. %d", nsrc, RC_MAX_SRC);
    AE_REQUIRE(B > 0 && up_side(H) && up_side(W) && (long)B * H * W < (1L << 31), "ae_resize_concat_rows_bf16: bad sizes B=%d H=%d W=%d", B, H, W);
    AE_REQUIRE(ld_dst > 0 && ld_dst % 8 == 0 && ((uintptr_t)dst & 15) == 0, "ae_resize_concat_rows_bf16: dst must be 16-byte aligned with a row stride that is a multiple of 8");
    AE_REQUIRE(!addend || nsrc == 1, "ae_resize_concat_rows_bf16: the addend goes with a single source");
    const long dst_bytes = (long)B * H * W * ld_dst * 2;
    RcArgs a{};
    int chunks = 0;
    for (int i = 0; i < nsrc; ++i) {
        AE_REQUIRE(src[i], "ae_resize_concat_rows_bf16: null pointer (source %d)", i);
        AE_REQUIRE(up_side(src_h[i]) && up_side(src_w[i]), "ae_resize_concat_rows_bf16: bad sizes of source %d: %d x %d", i, src_h[i], src_w[i]);
        AE_REQUIRE(src_c[i] > 0 && src_c[i] % 8 == 0 && src_c[i] <= 65536, "ae_resize_concat_rows_bf16: source %d: C=%d must be a multiple of 8 (16 bytes per lane)", i,
                   src_c[i]);
        AE_REQUIRE(src_ld[i] >= src_c[i] && src_ld[i] % 8 == 0 && ((uintptr_t)src[i] & 15) == 0,
                   "ae_resize_concat_rows_bf16: source %d must be 16-byte aligned with a row stride that is a multiple of 8 and at least C", i);
        AE_REQUIRE(dst_col[i] >= 0 && dst_col[i] % 8 == 0 && (long)dst_col[i] + src_c[i] <= ld_dst,
                   "ae_resize_concat_rows_bf16: the slice of source %d, columns %d .. %d, does not fit the destination's %ld", i, dst_col[i], dst_col[i] + src_c[i], ld_dst);
        for (int j = 0; j < i; ++j)
            AE_REQUIRE(dst_col[i] >= dst_col[j] + src_c[j] || dst_col[j] >= dst_col[i] + src_c[i], "ae_resize_concat_rows_bf16: the slices of sources %d and %d overlap", j, i);
        const long span = ((long)src_h[i] * src_w[i] - 1) * src_ld[i] + src_c[i];          // elements one image reaches over
        AE_REQUIRE(src_img[i] % 8 == 0 && (B == 1 || src_img[i] >= span) && src_img[i] >= 0 && src_img[i] < (1L << 31) && src_ld[i] < (1L << 31),
                   "ae_resize_concat_rows_bf16: source %d: the image stride must be a multiple of 8 and at least one image", i);
        AE_REQUIRE(!up_overlap(src[i], ((long)(B - 1) * src_img[i] + span) * 2, dst, dst_bytes),
                   "ae_resize_concat_rows_bf16: dst must not alias source %d (only the addend may be the destination)", i);
        a.s[i] = RcSource{(const bf16_t*)src[i], (int)src_ld[i], (int)src_img[i], src_h[i], src_w[i], src_c[i], dst_col[i], relu[i] ? 1 : 0};
        chunks += src_c[i] / 8;
    }
    if (addend) {
        AE_REQUIRE(ld_add >= src_c[0] && ld_add % 8 == 0 && ((uintptr_t)addend & 15) == 0,
                   "ae_resize_concat_rows_bf16: the addend must be 16-byte aligned with a row stride that is a multiple of 8 and at least C");
        // the destination itself: every thread reads exactly the 16 bytes it then writes
        AE_REQUIRE(!up_overlap(addend, (long)B * H * W * ld_add * 2, dst, dst_bytes) || ((const char*)addend == (const char*)dst + (long)dst_col[0] * 2 && ld_add == ld_dst),
                   "ae_resize_concat_rows_bf16: the addend must be the destination's slice itself or a buffer apart from it");
    }
    const long total = (long)B * H * W * chunks;
    hipLaunchKernelGGL(resize_concat_kernel, dim3(up_grid((total + 255) / 256, 1L << 20)), dim3(256), 0, (hipStream_t)stream, a, nsrc, (const bf16_t*)addend, ld_add,
                       (bf16_t*)dst, ld_dst, B, H, W, chunks);
    return ae_check_launch("ae_resize_concat_rows_bf16");
}

extern "C" int ae_seg_argmax_u8(const float* logits, long ld, int ncls, const void* palette, void* labels, void* colours, int B, int h, int w, int Hm, int Wm,
                                int Ho, int Wo, void* stream) {
    AE_REQUIRE(logits && labels, "ae_seg_argmax_u8: null pointer");
    AE_REQUIRE((palette != nullptr) == (colours != nullptr), "ae_seg_argmax_u8: the palette and the colour image go together");
    AE_REQUIRE(ncls >= 1 && ncls <= SEG_MAX_CLS, "ae_seg_argmax_u8: %d classes: a uint8 label holds 1 .. %d", ncls, SEG_MAX_CLS);
    AE_REQUIRE(ld >= ncls && ld % 4 == 0 && ((uintptr_t)logits & 15) == 0, "ae_seg_argmax_u8: logits must be 16-byte aligned with a row stride that is a multiple of 4 and at least ncls");
    AE_REQUIRE(B > 0 && up_side(h) && up_side(w) && up_side(Hm) && up_side(Wm) && up_side(Ho) && up_side(Wo), "ae_seg_argmax_u8: bad sizes B=%d %dx%d -> %dx%d -> %dx%d", B, h,
               w, Hm, Wm, Ho, Wo);
    AE_REQUIRE((long)B * Ho * Wo < (1L << 31) && (long)B * h * w * ld < (1L << 40), "ae_seg_argmax_u8: bad sizes B=%d %dx%d -> %dx%d", B, h, w, Ho, Wo);
    const long waves = (long)B * Ho * ((Wo + SEG_PX - 1) / SEG_PX);
    const dim3 grid(up_grid((waves + 3) / 4, 1L << 20)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (Hm == Ho && Wm == Wo) {
#if AE_SEG_WIDE
        hipLaunchKernelGGL(seg_argmax_wide_kernel, grid, block, 0, st, logits, ld, ncls, (const uint8_t*)palette, (uint8_t*)labels, (uint8_t*)colours, B, h, w, Ho, Wo);
#else
        hipLaunchKernelGGL((seg_argmax_kernel<false>), grid, block, 0, st, logits, ld, ncls, (const uint8_t*)palette, (uint8_t*)labels, (uint8_t*)colours, B, h, w, Hm, Wm,
                           Ho, Wo);
#endif
    }
    else
        hipLaunchKernelGGL((seg_argmax_kernel<true>), grid, block, 0, st, logits, ld, ncls, (const uint8_t*)palette, (uint8_t*)labels, (uint8_t*)colours, B, h, w, Hm, Wm,
                           Ho, Wo);
    return ae_check_launch("ae_seg_argmax_u8");
}
