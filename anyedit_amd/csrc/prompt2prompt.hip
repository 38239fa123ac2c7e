// Prompt-to-Prompt attention control kernels for gfx950 (MI355X).
//
// Replaces (AnyEdit_Collection/other_modules/prompt2prompt/prompt_to_prompt_stable.py, registered by ptp_utils.py:175-273):
//   :132-136  AttentionStore.forward            the per-head probabilities of every cross-attention call kept ([B h, N, 77]);
//   :183-199  AttentionControlEdit.forward      attn[1:] = replace_cross_attention(attn_base, attn_replace) * alpha + (1 - alpha) * attn_replace;
//   :216-217  AttentionReplace                  einsum('hpw,bwn->bhpn', attn_base, mapper);
//   :228-231  AttentionRefine                   attn_base[:, :, mapper] * alphas + att_replace * (1 - alphas);
//   :243-248  AttentionReweight                 attn_base * equalizer, optionally over a previous controller;
//   :61-73    LocalBlend.__call__               token-selected maps -> 3x3 max-pool -> nearest resize -> / max -> > threshold -> or -> blend.
// The reference hook materialises attention_probs for every call and edits it in torch; no logit or probability buffer is formed here.
//
// ae_attn_p2p_bf16: one wave per query row, lane l owns keys l and l + 64 (Nk <= 128), the whole row of probabilities lives in two registers per
// lane (the short-key design of token_map_kernel in masactrl.hip).  Per head a block stages, one after the other through ONE LDS buffer, the base
// sample's keys (edited samples only), the sample's own keys and the sample's own values.  Everything between the bf16 operands and the single bf16
// rounding of the output is fp32 on the VALU: logits by fmaf over the head dim, exp2-domain softmax, P_base M by fmaf over the base's tokens in index
// order (the row of P_base is broadcast through a per-wave LDS line, lane j reads column j of M), the (c, d) blend, and P' V by fmaf over the keys in
// index order.  The probability path therefore carries no bf16 rounding.  The head sum for the store is one register per (row, key) to which the
// heads are added in index order.  No atomics and no cross-wave reductions: a second call gives the same bits.
//
// ae_p2p_local_blend_f32: every block recomputes the two S x S maps (S <= 32: at most 2 x 1024 sums over the layers and the set's tokens, in layer
// then token order in one fp32 register), pools and normalises them in LDS, and blends a grid-strided slice of the pixels; nothing is read back.
#include "attn_tile.hpp"
#include <stdlib.h>

namespace {

constexpr int P2P_MAX_B = 64;
constexpr int P2P_MAXD = 160, P2P_MAXK = 128;
constexpr int P2P_RW = 4;           // query rows per wave
constexpr int P2P_QB = 4 * P2P_RW;  // per block
constexpr int P2P_ROW = P2P_MAXD + 8;

struct P2PArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o;
    const float* M; const float* c; const float* d; float* store;
    int B, H, N, Nk, D;
    long q_sb, q_sh, q_sn, k_sb, k_sh, k_sn, v_sb, v_sh, v_sn, o_sb, o_sh, o_sn;
    float c2;  // scale * log2(e)
    int accumulate;
    int base[P2P_MAX_B], srow[P2P_MAX_B];
};

__device__ __forceinline__ void p2p_stage(bf16_t* dst, const bf16_t* src, long sn, int rows, int dch, int tid) {
    for (int i = tid; i < rows * dch; i += 256) {
        const int row = i / dch, c = i - row * dch;
        *reinterpret_cast<u32x4*>(dst + row * P2P_ROW + c * 8) = *reinterpret_cast<const u32x4*>(src + (long)row * sn + c * 8);
    }
}

// softmax probabilities of one query row against the keys in LDS: p0 for key `lane`, p1 for key `lane + 64`; exactly 0 past Nk
__device__ __forceinline__ void p2p_probs(const bf16_t* sK, const bf16_t* qr, int dch, int lane, int Nk, float c2, float& p0, float& p1) {
    const bool in0 = lane < Nk, in1 = lane + 64 < Nk;
    const bf16_t* k0p = sK + min(lane, Nk - 1) * P2P_ROW;
    const bf16_t* k1p = sK + min(lane + 64, Nk - 1) * P2P_ROW;
    float s0 = 0.f, s1 = 0.f;
    for (int c = 0; c < dch; ++c) {
        const u32x4 qv = *reinterpret_cast<const u32x4*>(qr + c * 8);
        const u32x4 ka = *reinterpret_cast<const u32x4*>(k0p + c * 8);
        const u32x4 kb = *reinterpret_cast<const u32x4*>(k1p + c * 8);
        const uint32_t qw[4] = {qv.x, qv.y, qv.z, qv.w}, aw[4] = {ka.x, ka.y, ka.z, ka.w}, bw[4] = {kb.x, kb.y, kb.z, kb.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s0 = fmaf(bf16lo(qw[e]), bf16lo(aw[e]), s0);
            s0 = fmaf(bf16hi(qw[e]), bf16hi(aw[e]), s0);
            s1 = fmaf(bf16lo(qw[e]), bf16lo(bw[e]), s1);
            s1 = fmaf(bf16hi(qw[e]), bf16hi(bw[e]), s1);
        }
    }
    const float t0 = in0 ? s0 * c2 : NEG_BIG, t1 = in1 ? s1 * c2 : NEG_BIG;
    const float m = wave_reduce_max(fmaxf(t0, t1));  // lane 0 is always a real key
    const float e0 = in0 ? __builtin_amdgcn_exp2f(t0 - m) : 0.f, e1 = in1 ? __builtin_amdgcn_exp2f(t1 - m) : 0.f;
    const float den = wave_reduce_sum(e0 + e1);
    p0 = e0 / den;
    p1 = e1 / den;
}

__global__ __launch_bounds__(256) void attn_p2p_kernel(const P2PArgs p) {
    __shared__ __attribute__((aligned(16))) bf16_t sKV[P2P_MAXK * P2P_ROW];
    __shared__ float sP[4][P2P_RW][P2P_MAXK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int s = p.base[b];
    const bool edited = s != b;
    const int sr = p.store ? p.srow[b] : -1;
    if (!p.o && sr < 0) return;  // nothing to write for this sample (uniform over the block)
    const int q0 = blockIdx.x * P2P_QB + wave * P2P_RW;
    const int Nk = p.Nk, D = p.D, dch = D / 8;
    const bool in0 = lane < Nk, in1 = lane + 64 < Nk;
    const int j0 = min(lane, Nk - 1), j1 = min(lane + 64, Nk - 1);  // clamped: loads stay inside [0, Nk)
    float cc[2] = {0.f, 0.f}, dd[2] = {1.f, 1.f};
    if (edited) {
        cc[0] = p.c[(long)b * Nk + j0]; cc[1] = p.c[(long)b * Nk + j1];
        dd[0] = p.d[(long)b * Nk + j0]; dd[1] = p.d[(long)b * Nk + j1];
    }
    const float* Mb = p.M ? p.M + (long)b * Nk * Nk : nullptr;
    float (*wP)[P2P_MAXK] = sP[wave];

    float acc[P2P_RW][2];
#pragma unroll
    for (int qi = 0; qi < P2P_RW; ++qi) acc[qi][0] = acc[qi][1] = 0.f;

    for (int h = 0; h < p.H; ++h) {
        float mix[P2P_RW][2];
        if (edited) {
            __syncthreads();  // every wave is done with the previous contents of sKV
            p2p_stage(sKV, p.k + (long)s * p.k_sb + (long)h * p.k_sh, p.k_sn, Nk, dch, tid);
            __syncthreads();
            const bf16_t* qp = p.q + (long)s * p.q_sb + (long)h * p.q_sh;
#pragma unroll
            for (int qi = 0; qi < P2P_RW; ++qi) {
                const int row = min(q0 + qi, p.N - 1);  // clamped: rows past N are computed and not stored
                p2p_probs(sKV, qp + (long)row * p.q_sn, dch, lane, Nk, p.c2, mix[qi][0], mix[qi][1]);
                if (Mb) {
                    wP[qi][lane] = mix[qi][0];
                    wP[qi][lane + 64] = mix[qi][1];
                }
            }
            if (Mb) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int qi = 0; qi < P2P_RW; ++qi) mix[qi][0] = mix[qi][1] = 0.f;
                for (int i = 0; i < Nk; ++i) {  // (P_base M)[j] = sum_i P_base[i] M[i][j], i in index order
                    const float m0 = Mb[(long)i * Nk + j0], m1 = Mb[(long)i * Nk + j1];
#pragma unroll
                    for (int qi = 0; qi < P2P_RW; ++qi) {
                        const float pb = wP[qi][i];
                        mix[qi][0] = fmaf(pb, m0, mix[qi][0]);
                        mix[qi][1] = fmaf(pb, m1, mix[qi][1]);
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
        p2p_stage(sKV, p.k + (long)b * p.k_sb + (long)h * p.k_sh, p.k_sn, Nk, dch, tid);
        __syncthreads();
        {
            const bf16_t* qp = p.q + (long)b * p.q_sb + (long)h * p.q_sh;
#pragma unroll
            for (int qi = 0; qi < P2P_RW; ++qi) {
                const int row = min(q0 + qi, p.N - 1);
                float p0, p1;
                p2p_probs(sKV, qp + (long)row * p.q_sn, dch, lane, Nk, p.c2, p0, p1);
                if (edited) {  // P' = (P_base M) c + P_own d, not renormalised
                    p0 = fmaf(mix[qi][0], cc[0], p0 * dd[0]);
                    p1 = fmaf(mix[qi][1], cc[1], p1 * dd[1]);
                }
                p0 = in0 ? p0 : 0.f;
                p1 = in1 ? p1 : 0.f;
                acc[qi][0] += p0;
                acc[qi][1] += p1;
                wP[qi][lane] = p0;
                wP[qi][lane + 64] = p1;
            }
        }
        if (p.o) {
            __syncthreads();
            p2p_stage(sKV, p.v + (long)b * p.v_sb + (long)h * p.v_sh, p.v_sn, Nk, dch, tid);
            __syncthreads();  // (also orders this wave's wP writes before its reads)
            bf16_t* op = p.o + (long)b * p.o_sb + (long)h * p.o_sh;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int d0 = 128 * t + 2 * lane;  // this lane's two adjacent channels
                if (d0 >= D) continue;
                float o0[P2P_RW], o1[P2P_RW];
#pragma unroll
                for (int qi = 0; qi < P2P_RW; ++qi) o0[qi] = o1[qi] = 0.f;
                for (int j = 0; j < Nk; ++j) {  // keys in index order
                    const uint32_t vv = *reinterpret_cast<const uint32_t*>(sKV + j * P2P_ROW + d0);
                    const float v0 = bf16lo(vv), v1 = bf16hi(vv);
#pragma unroll
                    for (int qi = 0; qi < P2P_RW; ++qi) {
                        const float pj = wP[qi][j];
                        o0[qi] = fmaf(pj, v0, o0[qi]);
                        o1[qi] = fmaf(pj, v1, o1[qi]);
                    }
                }
#pragma unroll
                for (int qi = 0; qi < P2P_RW; ++qi) {
                    const int row = q0 + qi;
                    if (row < p.N) *reinterpret_cast<uint32_t*>(op + (long)row * p.o_sn + d0) = pack_bf16x2(o0[qi], o1[qi]);
                }
            }
        }
    }
    if (sr >= 0) {
#pragma unroll
        for (int qi = 0; qi < P2P_RW; ++qi) {
            const int row = q0 + qi;
            if (row >= p.N) continue;
            float* dst = p.store + ((long)sr * p.N + row) * Nk;
            if (in0) dst[lane] = p.accumulate ? dst[lane] + acc[qi][0] : acc[qi][0];
            if (in1) dst[lane + 64] = p.accumulate ? dst[lane + 64] + acc[qi][1] : acc[qi][1];
        }
    }
}

// ------------------------------------------------------------------------------------------------ local blend
constexpr int BLEND_MAX_LAYERS = 8, BLEND_MAX_S = 32, BLEND_MAX_BLOCKS = 16;
struct BlendArgs {
    const float* maps[BLEND_MAX_LAYERS];
    int L, S, Nk, C, h, w;
    float thr;
    unsigned long long set[4];  // sample b: words 2 b, 2 b + 1
    const float* x; float* out;
};

__global__ __launch_bounds__(256) void p2p_local_blend_kernel(const BlendArgs p) {
    __shared__ float sm[2][BLEND_MAX_S * BLEND_MAX_S], sp[2][BLEND_MAX_S * BLEND_MAX_S];
    __shared__ float s_mx[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = p.S, n = S * S, hw = p.h * p.w;
    // 1. m_b[pix] = sum over layers, then over the set's tokens in ascending order
    for (int idx = tid; idx < 2 * n; idx += 256) {
        const int b = idx / n, pix = idx - b * n;
        const unsigned long long w0 = p.set[2 * b], w1 = p.set[2 * b + 1];
        float a = 0.f;
        for (int l = 0; l < p.L; ++l) {
            const float* row = p.maps[l] + ((long)b * n + pix) * p.Nk;
            for (int j = 0; j < p.Nk; ++j) {
                const bool sel = j < 64 ? ((w0 >> j) & 1ull) : ((w1 >> (j - 64)) & 1ull);
                if (sel) a += row[j];
            }
        }
        sm[b][pix] = a;
    }
    __syncthreads();
    // 2. 3x3 max-pool, stride 1, pad 1 (the padding never wins: the window always holds its centre)
    for (int idx = tid; idx < 2 * n; idx += 256) {
        const int b = idx / n, pix = idx - b * n, y = pix / S, x = pix - y * S;
        float m = sm[b][pix];
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int yy = y + dy, xx = x + dx;
                if (yy >= 0 && yy < S && xx >= 0 && xx < S) m = fmaxf(m, sm[b][yy * S + xx]);
            }
        sp[b][pix] = m;
    }
    __syncthreads();
    // 3. nearest resize (F.interpolate without scale_factor: src = min(floor(dst * in / out), in - 1)) and the per-sample maximum of the resized map
    const float sy = (float)S / (float)p.h, sx = (float)S / (float)p.w;
    float mx[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        float m = sp[b][0];  // the resized map's pixel (0, 0)
        for (int i = tid; i < hw; i += 256) {
            const int oy = i / p.w, ox = i - oy * p.w;
            const int yy = min((int)floorf((float)oy * sy), S - 1), xx = min((int)floorf((float)ox * sx), S - 1);
            m = fmaxf(m, sp[b][yy * S + xx]);
        }
        m = wave_reduce_max(m);
        if (lane == 0) s_mx[b][wave] = m;
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 2; ++b) mx[b] = fmaxf(fmaxf(s_mx[b][0], s_mx[b][1]), fmaxf(s_mx[b][2], s_mx[b][3]));
    // 4.-7. normalise, threshold, or, blend
    const long plane = (long)hw, img = (long)p.C * hw;
    for (int i = blockIdx.x * 256 + tid; i < hw; i += gridDim.x * 256) {
        const int oy = i / p.w, ox = i - oy * p.w;
        const int yy = min((int)floorf((float)oy * sy), S - 1), xx = min((int)floorf((float)ox * sx), S - 1);
        bool mask = false;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            // an all-zero map is 0 / 0 = NaN in the reference, which compares false: 0 here
            if (mx[b] != 0.f) mask = mask || (sp[b][yy * S + xx] / mx[b] > p.thr);  // IEEE division, as the reference's fp32 tensor division
        }
        for (int ch = 0; ch < p.C; ++ch) {
            const float x0 = p.x[ch * plane + i], x1 = p.x[img + ch * plane + i];
            p.out[ch * plane + i] = x0;
            p.out[img + ch * plane + i] = mask ? x1 : x0;
        }
    }
}

}  // namespace

extern "C" int ae_attn_p2p_bf16(const void* q, const void* k, const void* v, void* out, int B, int H, int N, int Nk, int D, long q_sb, long q_sh,
                                long q_sn, long k_sb, long k_sh, long k_sn, long v_sb, long v_sh, long v_sn, long o_sb, long o_sh, long o_sn, float scale,
                                const int* base, const float* M, const float* c, const float* d, float* store, const int* store_row, int store_rows,
                                int accumulate, void* stream) {
    AE_REQUIRE(q && k && base, "ae_attn_p2p_bf16: null pointer");
    AE_REQUIRE(out || store, "ae_attn_p2p_bf16: neither an output nor a store to write");
    AE_REQUIRE(!out || v, "ae_attn_p2p_bf16: an output needs v");
    AE_REQUIRE(!store || store_row, "ae_attn_p2p_bf16: a store needs store_row");
    AE_REQUIRE(B > 0 && H > 0 && N > 0 && Nk > 0, "ae_attn_p2p_bf16: bad sizes B=%d H=%d N=%d Nk=%d", B, H, N, Nk);
    AE_REQUIRE(scale > 0.f, "ae_attn_p2p_bf16: scale must be positive");
    AE_REQUIRE((q_sb | q_sh | q_sn | k_sb | k_sh | k_sn) % 8 == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0,
               "ae_attn_p2p_bf16: q / k rows must be 16-byte aligned");
    AE_REQUIRE(!out || ((v_sb | v_sh | v_sn) % 8 == 0 && ((uintptr_t)v & 15) == 0 && (o_sb | o_sh | o_sn) % 4 == 0 && ((uintptr_t)out & 7) == 0),
               "ae_attn_p2p_bf16: v rows must be 16-byte aligned and out rows 8-byte aligned");
    if (B > P2P_MAX_B || Nk > P2P_MAXK || !(D == 40 || D == 64 || D == 80 || D == 160)) {
        ae_set_error("ae_attn_p2p_bf16: unsupported B=%d (<= %d), Nk=%d (<= %d) or head_dim %d (40, 64, 80, 160)", B, P2P_MAX_B, Nk, P2P_MAXK, D);
        return AE_ERR_UNSUPPORTED;
    }
    P2PArgs a{};
    bool any_edit = false;
    for (int b = 0; b < B; ++b) {
        AE_REQUIRE(base[b] >= 0 && base[b] < B, "ae_attn_p2p_bf16: base[%d]=%d outside [0, %d)", b, base[b], B);
        AE_REQUIRE(base[base[b]] == base[b], "ae_attn_p2p_bf16: base[%d]=%d is itself an edited sample (a base must be unedited)", b, base[b]);
        a.base[b] = base[b];
        any_edit = any_edit || base[b] != b;
        a.srow[b] = -1;
        if (store) {
            AE_REQUIRE(store_row[b] >= -1 && store_row[b] < store_rows, "ae_attn_p2p_bf16: store_row[%d]=%d outside [-1, %d)", b, store_row[b], store_rows);
            a.srow[b] = store_row[b];
        }
    }
    if (store) {
        for (int b = 0; b < B; ++b)
            for (int e = 0; e < b; ++e)
                AE_REQUIRE(a.srow[b] < 0 || a.srow[b] != a.srow[e], "ae_attn_p2p_bf16: samples %d and %d write the same store row %d", e, b, a.srow[b]);
    }
    AE_REQUIRE(!any_edit || (c && d), "ae_attn_p2p_bf16: an edited sample needs c and d");
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.o = (bf16_t*)out;
    a.M = M; a.c = c; a.d = d; a.store = store;
    a.B = B; a.H = H; a.N = N; a.Nk = Nk; a.D = D;
    a.q_sb = q_sb; a.q_sh = q_sh; a.q_sn = q_sn; a.k_sb = k_sb; a.k_sh = k_sh; a.k_sn = k_sn;
    a.v_sb = v_sb; a.v_sh = v_sh; a.v_sn = v_sn; a.o_sb = o_sb; a.o_sh = o_sh; a.o_sn = o_sn;
    a.c2 = scale * LOG2E; a.accumulate = accumulate;
    dim3 grid((unsigned)((N + P2P_QB - 1) / P2P_QB), (unsigned)B), block(256);
    hipLaunchKernelGGL(attn_p2p_kernel, grid, block, 0, (hipStream_t)stream, a);
    return ae_check_launch("ae_attn_p2p_bf16");
}

extern "C" int ae_p2p_local_blend_f32(const float* const* maps, int nlayers, int S, int Nk, const unsigned long long* token_sets, float threshold,
                                      const float* x, float* out, int C, int h, int w, void* stream) {
    AE_REQUIRE(maps && token_sets && x && out, "ae_p2p_local_blend_f32: null pointer");
    AE_REQUIRE(C > 0 && h > 0 && w > 0 && (long)C * h * w < (1L << 30), "ae_p2p_local_blend_f32: bad sizes C=%d h=%d w=%d", C, h, w);
    if (nlayers < 1 || nlayers > BLEND_MAX_LAYERS || S < 1 || S > BLEND_MAX_S || Nk < 1 || Nk > P2P_MAXK) {
        ae_set_error("ae_p2p_local_blend_f32: unsupported layers=%d (1 .. %d), S=%d (<= %d) or Nk=%d (<= %d)", nlayers, BLEND_MAX_LAYERS, S, BLEND_MAX_S, Nk,
                     P2P_MAXK);
        return AE_ERR_UNSUPPORTED;
    }
    BlendArgs a{};
    for (int l = 0; l < nlayers; ++l) {
        AE_REQUIRE(maps[l], "ae_p2p_local_blend_f32: map %d is null", l);
        a.maps[l] = maps[l];
    }
    a.L = nlayers; a.S = S; a.Nk = Nk; a.C = C; a.h = h; a.w = w; a.thr = threshold;
    for (int i = 0; i < 4; ++i) a.set[i] = token_sets[i];
    a.x = x; a.out = out;
    const int want = (h * w + 255) / 256;
    const int blocks = want < BLEND_MAX_BLOCKS ? want : BLEND_MAX_BLOCKS;
    hipLaunchKernelGGL(p2p_local_blend_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return ae_check_launch("ae_p2p_local_blend_f32");
}
