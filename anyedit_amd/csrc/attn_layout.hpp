// What the two attention designs built on S^T = K Q^T / O^T = V^T P^T share (attn_short.hpp: a whole row in registers; attn_tile.hpp: streamed
// 64-key tiles): the exp2-domain constants and the placement of V^T in LDS.  Defined here once.
#pragma once
#include "common.hpp"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
// a removed (masked, padding, other-class) logit: finite, since attention.hip and clip_text.hip are built with -ffinite-math-only; behaves like
// masked_fill(-finfo.max) (ldm/modules/attention.py:186-187)
constexpr float NEG_BIG = -1.0e30f;

__device__ __forceinline__ int vt_pos(int key) {  // inside one 64-key tile: key = 16 f + 4 g + r  ->  16 g + 4 f + r
    return ((key >> 2) & 3) * 16 + (key >> 4) * 4 + (key & 3);
}

// two value rows (16 bytes each, d = 8c .. 8c+7 of keys `key`, `key + 1`, key even) -> V^T rows d, columns pos, pos + 1
__device__ __forceinline__ void store_vt_pair(bf16_t* sVt, int vrow, int c, int pos, u32x4 t0, u32x4 t1) {
    const uint32_t a0[4] = {t0.x, t0.y, t0.z, t0.w};
    const uint32_t a1[4] = {t1.x, t1.y, t1.z, t1.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t lo = __builtin_amdgcn_perm(a1[e], a0[e], 0x05040100u);  // {a0.lo16, a1.lo16}: d = 8c + 2e, one v_perm_b32
        const uint32_t hi = __builtin_amdgcn_perm(a1[e], a0[e], 0x07060302u);  // {a0.hi16, a1.hi16}: d = 8c + 2e + 1
        *reinterpret_cast<uint32_t*>(sVt + (c * 8 + 2 * e) * vrow + pos) = lo;
        *reinterpret_cast<uint32_t*>(sVt + (c * 8 + 2 * e + 1) * vrow + pos) = hi;
    }
}

}  // namespace
