// Rows handled 8 channels (one 16-byte transaction) at a time, and the row-in-one-wave LayerNorm built on them (clip_vision.hip,
// dino_vision.hip, gdino_text.hip).
#pragma once
#include "common.hpp"

namespace {

constexpr int LN_MAXCH = 4;                    // 8-channel chunks per lane
constexpr int LN_CMAX = 64 * 8 * LN_MAXCH;     // 2048: the widest row that lives in one wave's registers

struct f32x8 { float v[8]; };

__device__ __forceinline__ f32x8 load8_f32(const float* p) {  // 16-byte aligned
    const f32x4 a = *reinterpret_cast<const f32x4*>(p);
    const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
    return f32x8{{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}};
}

__device__ __forceinline__ void add8_bf16(f32x8& x, const bf16_t* p) {  // 16-byte aligned
    const u32x4 t = *reinterpret_cast<const u32x4*>(p);
    x.v[0] += bf16lo(t.x); x.v[1] += bf16hi(t.x); x.v[2] += bf16lo(t.y); x.v[3] += bf16hi(t.y);
    x.v[4] += bf16lo(t.z); x.v[5] += bf16hi(t.z); x.v[6] += bf16lo(t.w); x.v[7] += bf16hi(t.w);
}

__device__ __forceinline__ void store8_bf16(bf16_t* p, const float (&r)[8]) {  // 16-byte aligned
    *reinterpret_cast<u32x4*>(p) = (u32x4){pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]), pack_bf16x2(r[4], r[5]), pack_bf16x2(r[6], r[7])};
}

// LayerNorm of one row held by a wave as x[i] = channels [8 (lane + 64 i), +8), and its bf16 store: fp32 statistics in two passes over the
// registers (sum in (i, e) order, mean, centred squares), one rounding at the store
__device__ __forceinline__ void wave_ln_store(const f32x8 (&x)[LN_MAXCH], int lane, int ncc, int C, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, float eps, bf16_t* __restrict__ y) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXCH; ++i)
        if (lane + i * 64 < ncc) {
#pragma unroll
            for (int e = 0; e < 8; ++e) s += x[i].v[e];
        }
    const float mu = wave_reduce_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXCH; ++i)
        if (lane + i * 64 < ncc) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = x[i].v[e] - mu;
                q += d * d;
            }
        }
    const float rstd = rsqrtf(wave_reduce_sum(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < LN_MAXCH; ++i) {
        const int cc = lane + i * 64;
        if (cc < ncc) {
            const f32x8 g = load8_f32(gamma + cc * 8), b = load8_f32(beta + cc * 8);
            float r[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = (x[i].v[e] - mu) * rstd * g.v[e] + b.v[e];
            store8_bf16(y + cc * 8, r);
        }
    }
}

}  // namespace
