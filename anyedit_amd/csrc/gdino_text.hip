// GroundingDINO's text side (GroundingDINO/groundingdino/models/GroundingDINO/groundingdino.py:233-283, bertwarper.py:180-273, and the BertModel the
// reference takes from transformers) for gfx950: what the library could not run.  Projections, LayerNorms behind a residual, the GELU and feat_map
// run on existing entry points (ae_gemm_bf16, ae_layernorm_bf16, ae_bias_act_f32_bf16).  This file adds
//
//   ae_gdino_text_spans       generate_masks_with_special_tokens[_and_transfer_map] (bertwarper.py:180-273) in closed form: per token the key range
//                             [lo, hi) it may attend, its position id and, on request, the dense [B, N, N] mask — no host loop, no torch.nonzero.
//   ae_bert_embed_ln_bf16     BertEmbeddings: LayerNorm(word[ids] + position[position_ids] + token_type[type_ids]) in one launch; the sum is never stored.
//   ae_attn_span_short_bf16   BertSelfAttention's core under a block-diagonal mask: softmax(scale q k^T over keys [lo, hi)) v, head_dim 64.
//
// Span attention is attn_masked_short_kernel (gdino_encoder.hip) with two changes.  The mask is two integer compares against the lane's query's
// (lo, hi) instead of byte loads from a [B*H, N, N] array, which at BERT's 12 heads the caller would have to materialise per call.  And a workgroup
// (64 queries of one (sample, head), one 16-row MFMA fragment per wave) stages, multiplies and accumulates only over ITS key window: the union of
// its queries' spans widened to whole 64-key tiles (V^T is permuted inside whole tiles).  The window is block-uniform; a key outside a query's span
// has probability exactly 0 in that query's row, and a key outside the union is staged as zeros and never read from memory.  K rows and then V^T
// pass through one LDS buffer, S^T = K Q^T and O^T = V^T P^T with v_mfma_f32_16x16x32_bf16, one-pass fp32 softmax in the exp2 domain, bf16 once at
// the store.  No atomics, no scratch, no host synchronisation; two launches on the same inputs are bit-identical.
#include "common.hpp"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float NEG_BIG = -1.0e30f;
constexpr int TXT_NMAX = 256;

// ------------------------------------------------------------------------------------------------------------------ spans
struct SpecialIds { long v[8]; int n; };

// One workgroup per sample, one thread per token.  Closed form of the reference's loop under its own contract (column 0 is a special token): with
// e the first special position >= n and p the last special position before e, a token whose e exists and is neither 0 nor N-1 attends [p+1, e+1)
// at position n - (p+1); every other token (n = 0, a special at N-1, tokens whose next special is at N-1, padding after the last special) attends
// itself at position 0.
template <typename IdT>
__global__ __launch_bounds__(256) void text_spans_kernel(const IdT* __restrict__ ids, const SpecialIds sp, int* __restrict__ spans, long* __restrict__ pos,
                                                        uint8_t* __restrict__ dense, int N) {
    __shared__ uint8_t sSpec[TXT_NMAX];
    __shared__ int sLo[TXT_NMAX], sHi[TXT_NMAX];
    const int b = blockIdx.x, n = threadIdx.x;
    if (n < N) {
        const long id = (long)ids[(long)b * N + n];
        bool s = false;
#pragma unroll
        for (int i = 0; i < 8; ++i) s = s || (i < sp.n && id == sp.v[i]);
        sSpec[n] = s ? 1 : 0;
    }
    __syncthreads();
    if (n < N) {
        int e = n;
        while (e < N && !sSpec[e]) ++e;
        int lo = n, hi = n + 1;
        if (e < N && e != 0 && e != N - 1) {
            int p = e - 1;
            while (p >= 0 && !sSpec[p]) --p;
            lo = p + 1;
            hi = e + 1;
        }
        const long row = (long)b * N + n;
        *reinterpret_cast<int2*>(spans + 2 * row) = make_int2(lo, hi);
        pos[row] = (long)(n - lo);
        sLo[n] = lo;
        sHi[n] = hi;
    }
    if (dense == nullptr) return;   // uniform
    __syncthreads();
    uint8_t* d = dense + (long)b * N * N;
    for (int i = threadIdx.x; i < N * N; i += 256) {
        const int q = i / N, key = i - q * N;
        d[i] = (key >= sLo[q] && key < sHi[q]) ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------------------------ embeddings + LayerNorm
constexpr int LN_MAXCH = 4;                    // 8-channel chunks per lane
constexpr int LN_CMAX = 64 * 8 * LN_MAXCH;     // 2048: a row lives in one wave's registers (BERT-base 768, BERT-large 1024)

struct f32x8 { float v[8]; };

__device__ __forceinline__ f32x8 load8_f32(const float* p) {  // 16-byte aligned
    const f32x4 a = *reinterpret_cast<const f32x4*>(p);
    const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
    return f32x8{{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}};
}

__device__ __forceinline__ void add8_bf16(f32x8& x, const bf16_t* p) {
    const u32x4 t = *reinterpret_cast<const u32x4*>(p);
    x.v[0] += bf16lo(t.x); x.v[1] += bf16hi(t.x); x.v[2] += bf16lo(t.y); x.v[3] += bf16hi(t.y);
    x.v[4] += bf16lo(t.z); x.v[5] += bf16hi(t.z); x.v[6] += bf16lo(t.w); x.v[7] += bf16hi(t.w);
}

__device__ __forceinline__ long clamp_row(long i, int rows) { return i < 0 ? 0 : (i >= rows ? (long)rows - 1 : i); }

// one wave per token row: lane holds channels [8 (lane + 64 i), +8); two-pass statistics in fp32 on the un-rounded sum
__global__ __launch_bounds__(256) void bert_embed_ln_kernel(const long* __restrict__ ids, const long* __restrict__ pids, const long* __restrict__ tids,
                                                           const bf16_t* __restrict__ word, const bf16_t* __restrict__ ptab, const bf16_t* __restrict__ ttab,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, bf16_t* __restrict__ out, long rows,
                                                           int N, int C, int vocab, int positions, int types, float eps) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    // an index outside its table is clamped into it, never a wild read (ids on the GPU are not read back by the caller)
    const bf16_t* w = word + clamp_row(ids[row], vocab) * C;
    const bf16_t* pr = ptab + clamp_row(pids ? pids[row] : row % N, positions) * C;
    const bf16_t* tr = ttab + clamp_row(tids ? tids[row] : 0, types) * C;
    const int ncc = C / 8;
    f32x8 x[LN_MAXCH];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXCH; ++i) {
        const int cc = lane + i * 64;
        x[i] = f32x8{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
        if (cc < ncc) {
            add8_bf16(x[i], w + cc * 8);
            add8_bf16(x[i], pr + cc * 8);
            add8_bf16(x[i], tr + cc * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += x[i].v[e];
        }
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
    bf16_t* y = out + row * C;
#pragma unroll
    for (int i = 0; i < LN_MAXCH; ++i) {
        const int cc = lane + i * 64;
        if (cc < ncc) {
            const f32x8 g = load8_f32(gamma + cc * 8), bb = load8_f32(beta + cc * 8);
            float r[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = (x[i].v[e] - mu) * rstd * g.v[e] + bb.v[e];
            *reinterpret_cast<u32x4*>(y + cc * 8) = (u32x4){pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]), pack_bf16x2(r[4], r[5]), pack_bf16x2(r[6], r[7])};
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ span attention
__device__ __forceinline__ int vt_pos(int key) {  // inside one 64-key tile: key = 16 f + 4 g + r  ->  16 g + 4 f + r
    return ((key >> 2) & 3) * 16 + (key >> 4) * 4 + (key & 3);
}

// two value rows (16 bytes each, d = 8c .. 8c+7 of keys `key`, `key + 1`, key even) -> V^T rows d, columns pos, pos + 1
__device__ __forceinline__ void store_vt_pair(bf16_t* sVt, int vrow, int c, int pos, u32x4 t0, u32x4 t1) {
    const uint32_t a0[4] = {t0.x, t0.y, t0.z, t0.w};
    const uint32_t a1[4] = {t1.x, t1.y, t1.z, t1.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t lo = __builtin_amdgcn_perm(a1[e], a0[e], 0x05040100u);  // {a0.lo16, a1.lo16}: d = 8c + 2e
        const uint32_t hi = __builtin_amdgcn_perm(a1[e], a0[e], 0x07060302u);  // {a0.hi16, a1.hi16}: d = 8c + 2e + 1
        *reinterpret_cast<uint32_t*>(sVt + (c * 8 + 2 * e) * vrow + pos) = lo;
        *reinterpret_cast<uint32_t*>(sVt + (c * 8 + 2 * e + 1) * vrow + pos) = hi;
    }
}

struct SpanArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; const int* spans; bf16_t* o;
    int H, N;
    long q_sb, q_sh, q_sn, k_sb, k_sh, k_sn, v_sb, v_sh, v_sn, o_sb, o_sh, o_sn;
    float scale;
};

// (lo, hi) of query n of sample b, forced into 0 <= lo < hi <= N: a span that breaks the contract can change a result, never an address
__device__ __forceinline__ int2 load_span(const int* __restrict__ spans, int b, int n, int N) {
    const int2 s = *reinterpret_cast<const int2*>(spans + 2 * ((long)b * N + n));
    const int lo = min(max(s.x, 0), N - 1);
    return make_int2(lo, max(min(s.y, N), lo + 1));
}

// One workgroup per (batch, head, 64 query rows), one 16-row query fragment per wave.  The keys of the workgroup's window [w0, w1) pass through ONE
// LDS buffer: first the K rows (the window's logits, <= 16 key fragments, then live in registers and the softmax is one pass), then V^T.
__global__ __launch_bounds__(256) void attn_span_short_kernel(const SpanArgs p) {
    constexpr int D = 64, NKF = 16;
    constexpr int NT = 256;
    constexpr int NS = NKF * 16;    // the widest window
    constexpr int NC = D / 32;
    constexpr int NDF = D / 16;
    constexpr int DCH = D / 8;
    constexpr int KROW = D + 8;
    constexpr int VROW = NS + 8;
    constexpr int BUF = (NS * KROW > D * VROW) ? NS * KROW : D * VROW;
    static_assert(NS == TXT_NMAX && NKF % 4 == 0, "whole 64-key tiles, at most 256 keys");

    __shared__ __attribute__((aligned(16))) bf16_t sBuf[BUF];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
    const int N = p.N;
    const int qb = blockIdx.x * 64;

    // the workgroup's window: every wave reduces the same 64 spans, so the result is block-uniform without a barrier
    int ulo, uhi;
    {
        const int2 s = load_span(p.spans, b, min(qb + lane, N - 1), N);
        ulo = s.x;
        uhi = s.y;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            ulo = min(ulo, __shfl_xor(ulo, o, 64));
            uhi = max(uhi, __shfl_xor(uhi, o, 64));
        }
        ulo = __builtin_amdgcn_readfirstlane(ulo);
        uhi = __builtin_amdgcn_readfirstlane(uhi);
    }
    const int w0 = ulo & ~63;                        // 0 <= w0 <= ulo < uhi <= N <= 256
    const int nk = ((uhi + 63) & ~63) - w0;          // staged keys: whole tiles, 64 .. 256
    const int nfrag = (uhi - w0 + 15) >> 4;          // 16-key fragments that hold a key of the union

    const int q0 = qb + wave * 16;
    const bool active = q0 < N;   // wave-uniform
    const int qrow = q0 + l15, qc = min(qrow, N - 1);
    const bf16_t* kp = p.k + (long)b * p.k_sb + (long)h * p.k_sh;
    const bf16_t* vp = p.v + (long)b * p.v_sb + (long)h * p.v_sh;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    for (int id = tid; id < nk * DCH; id += NT) {
        const int rel = id / DCH, c = id - rel * DCH;
        const int key = w0 + rel;
        const u32x4 t = (key >= ulo && key < uhi) ? *reinterpret_cast<const u32x4*>(kp + (long)key * p.k_sn + c * 8) : zero4;
        *reinterpret_cast<u32x4*>(sBuf + rel * KROW + c * 8) = t;
    }
    __syncthreads();

    f32x4 s[NKF];
    float inv = 0.f;
    if (active) {
        bf16x8_t qf[NC];
        const bf16_t* qr = p.q + (long)b * p.q_sb + (long)h * p.q_sh + (long)qc * p.q_sn;
#pragma unroll
        for (int c = 0; c < NC; ++c) qf[c] = as_bf16x8(*reinterpret_cast<const u32x4*>(qr + c * 32 + lg * 8));
        const int2 own = load_span(p.spans, b, qc, N);   // allowed keys of this lane's query
        const float c2 = p.scale * LOG2E;
        float mx = NEG_BIG;
#pragma unroll
        for (int kf = 0; kf < NKF; ++kf) {
            if (kf < nfrag) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const bf16x8_t kfr = as_bf16x8(*reinterpret_cast<const u32x4*>(sBuf + (kf * 16 + l15) * KROW + c * 32 + lg * 8));
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr, qf[c], acc, 0, 0, 0);
                }
                const int key0 = w0 + kf * 16 + lg * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = key0 + r;
                    const float v = (key >= own.x && key < own.y) ? acc[r] * c2 : NEG_BIG;
                    s[kf][r] = v;
                    mx = fmaxf(mx, v);
                }
            } else {
                s[kf] = (f32x4){NEG_BIG, NEG_BIG, NEG_BIG, NEG_BIG};
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));   // a span holds a key, so mx is a real logit
        float rs = 0.f;
#pragma unroll
        for (int kf = 0; kf < NKF; ++kf)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = s[kf][r] > 0.5f * NEG_BIG ? __builtin_amdgcn_exp2f(s[kf][r] - mx) : 0.f;
                s[kf][r] = e;
                rs += e;
            }
        rs += __shfl_xor(rs, 16, 64);
        rs += __shfl_xor(rs, 32, 64);
        inv = 1.0f / rs;
    }
    __syncthreads();   // every wave has read the K rows

    for (int id = tid; id < (nk / 2) * DCH; id += NT) {
        const int pr = id / DCH, c = id - pr * DCH;
        const int rel = 2 * pr, key = w0 + rel;
        const u32x4 t0 = (key >= ulo && key < uhi) ? *reinterpret_cast<const u32x4*>(vp + (long)key * p.v_sn + c * 8) : zero4;
        const u32x4 t1 = (key + 1 >= ulo && key + 1 < uhi) ? *reinterpret_cast<const u32x4*>(vp + (long)(key + 1) * p.v_sn + c * 8) : zero4;
        store_vt_pair(sBuf, VROW, c, (rel & ~63) + vt_pos(rel & 63), t0, t1);
    }
    __syncthreads();   // the last barrier

    if (!active) return;
    f32x4 o[NDF];
#pragma unroll
    for (int df = 0; df < NDF; ++df) o[df] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NKF / 2; ++j) {
        if (2 * j < nfrag) {
            u32x4 pw;
            pw.x = pack_bf16x2(s[2 * j][0], s[2 * j][1]);
            pw.y = pack_bf16x2(s[2 * j][2], s[2 * j][3]);
            pw.z = pack_bf16x2(s[2 * j + 1][0], s[2 * j + 1][1]);
            pw.w = pack_bf16x2(s[2 * j + 1][2], s[2 * j + 1][3]);
            const bf16x8_t pb = as_bf16x8(pw);
#pragma unroll
            for (int df = 0; df < NDF; ++df) {
                const bf16x8_t vf = as_bf16x8(*reinterpret_cast<const u32x4*>(sBuf + (df * 16 + l15) * VROW + (j >> 1) * 64 + lg * 16 + (j & 1) * 8));
                o[df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pb, o[df], 0, 0, 0);
            }
        }
    }
    if (qrow < N) {
        bf16_t* op = p.o + (long)b * p.o_sb + (long)h * p.o_sh + (long)qrow * p.o_sn;
#pragma unroll
        for (int df = 0; df < NDF; ++df)
            *reinterpret_cast<u32x2*>(op + df * 16 + lg * 4) = (u32x2){pack_bf16x2(o[df][0] * inv, o[df][1] * inv), pack_bf16x2(o[df][2] * inv, o[df][3] * inv)};
    }
}

}  // namespace

extern "C" int ae_gdino_text_spans(const void* ids, int ids_are_i64, int B, int N, int n_special, long s0, long s1, long s2, long s3, long s4, long s5, long s6,
                                   long s7, int* spans, long* position_ids, void* dense_mask, void* stream) {
    AE_REQUIRE(ids && spans && position_ids, "ae_gdino_text_spans: null pointer");
    AE_REQUIRE(B > 0 && B <= 65535, "ae_gdino_text_spans: bad batch size %d (1 .. 65535)", B);
    AE_REQUIRE(N >= 1 && N <= TXT_NMAX, "ae_gdino_text_spans: %d tokens outside [1, %d] (one thread per token of a sample)", N, TXT_NMAX);
    AE_REQUIRE(n_special >= 0 && n_special <= 8, "ae_gdino_text_spans: %d special ids (at most 8 are passed by value)", n_special);
    AE_REQUIRE(((uintptr_t)ids & (ids_are_i64 ? 7 : 3)) == 0 && ((uintptr_t)spans & 7) == 0 && ((uintptr_t)position_ids & 7) == 0,
               "ae_gdino_text_spans: ids must be aligned to their type, spans and position_ids to 8 bytes");
    const SpecialIds sp{{s0, s1, s2, s3, s4, s5, s6, s7}, n_special};
    const hipStream_t st = (hipStream_t)stream;
    if (ids_are_i64)
        hipLaunchKernelGGL((text_spans_kernel<long>), dim3((unsigned)B), dim3(256), 0, st, (const long*)ids, sp, spans, position_ids, (uint8_t*)dense_mask, N);
    else
        hipLaunchKernelGGL((text_spans_kernel<int>), dim3((unsigned)B), dim3(256), 0, st, (const int*)ids, sp, spans, position_ids, (uint8_t*)dense_mask, N);
    return ae_check_launch("ae_gdino_text_spans");
}

extern "C" int ae_bert_embed_ln_bf16(const long* ids, const long* position_ids, const long* type_ids, const void* word_table,
                                     const void* position_table, const void* type_table, const float* gamma, const float* beta, void* out, int B, int N, int C,
                                     int vocab, int positions, int types, float eps, void* stream) {
    AE_REQUIRE(ids && word_table && position_table && type_table && gamma && beta && out, "ae_bert_embed_ln_bf16: null pointer");
    AE_REQUIRE(B > 0 && N > 0 && C > 0 && vocab > 0 && positions > 0 && types > 0 && (long)B * N < (1L << 31),
               "ae_bert_embed_ln_bf16: bad sizes B=%d N=%d C=%d vocab=%d positions=%d types=%d", B, N, C, vocab, positions, types);
    AE_REQUIRE(C % 8 == 0, "ae_bert_embed_ln_bf16: width %d must be a multiple of 8", C);
    AE_REQUIRE(C <= LN_CMAX, "ae_bert_embed_ln_bf16: width %d > %d unsupported (a row lives in one wave's registers)", C, LN_CMAX);
    AE_REQUIRE(position_ids || N <= positions, "ae_bert_embed_ln_bf16: %d tokens but the position table has %d rows", N, positions);
    AE_REQUIRE(eps >= 0.f, "ae_bert_embed_ln_bf16: eps must not be negative");
    AE_REQUIRE((((uintptr_t)word_table | (uintptr_t)position_table | (uintptr_t)type_table | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15) == 0 &&
                   (((uintptr_t)ids | (uintptr_t)position_ids | (uintptr_t)type_ids) & 7) == 0,
               "ae_bert_embed_ln_bf16: tables, gamma, beta and out must be 16-byte aligned, indices 8-byte aligned");
    const long rows = (long)B * N;
    hipLaunchKernelGGL(bert_embed_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ids, position_ids, type_ids, (const bf16_t*)word_table,
                       (const bf16_t*)position_table, (const bf16_t*)type_table, gamma, beta, (bf16_t*)out, rows, N, C, vocab, positions, types, eps);
    return ae_check_launch("ae_bert_embed_ln_bf16");
}

extern "C" int ae_attn_span_short_bf16(const void* q, const void* k, const void* v, const int* spans, void* out, int B, int H, int N, int D, long q_sb, long q_sh,
                                       long q_sn, long k_sb, long k_sh, long k_sn, long v_sb, long v_sh, long v_sn, long o_sb, long o_sh, long o_sn, float scale,
                                       void* stream) {
    AE_REQUIRE(q && k && v && spans && out, "ae_attn_span_short_bf16: null pointer");
    AE_REQUIRE(B > 0 && H > 0 && (long)B * H <= 65535, "ae_attn_span_short_bf16: bad sizes B=%d H=%d (B*H at most 65535)", B, H);
    AE_REQUIRE(N >= 1 && N <= TXT_NMAX, "ae_attn_span_short_bf16: sequence length %d outside [1, %d] (a window's logits live in registers)", N, TXT_NMAX);
    AE_REQUIRE(D == 64, "ae_attn_span_short_bf16: unsupported head_dim %d (64, BERT's, is the only one built)", D);
    AE_REQUIRE((q_sb | q_sh | q_sn | k_sb | k_sh | k_sn | v_sb | v_sh | v_sn) % 8 == 0 && (o_sb | o_sh | o_sn) % 4 == 0,
               "ae_attn_span_short_bf16: strides must keep q/k/v rows 16-byte aligned and out rows 8-byte aligned");
    AE_REQUIRE(q_sb >= 0 && q_sh >= 0 && q_sn >= 0 && k_sb >= 0 && k_sh >= 0 && k_sn >= 0 && v_sb >= 0 && v_sh >= 0 && v_sn >= 0 && o_sb >= 0 && o_sh >= 0 && o_sn >= D,
               "ae_attn_span_short_bf16: negative stride, or output rows that overlap");
    AE_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0 && ((uintptr_t)v & 15) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)spans & 7) == 0,
               "ae_attn_span_short_bf16: q/k/v must be 16-byte aligned, out and spans 8-byte aligned");
    AE_REQUIRE(scale > 0.f, "ae_attn_span_short_bf16: scale must be positive");
    SpanArgs a{};
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.spans = spans; a.o = (bf16_t*)out;
    a.H = H; a.N = N;
    a.q_sb = q_sb; a.q_sh = q_sh; a.q_sn = q_sn; a.k_sb = k_sb; a.k_sh = k_sh; a.k_sn = k_sn;
    a.v_sb = v_sb; a.v_sh = v_sh; a.v_sn = v_sn; a.o_sb = o_sb; a.o_sh = o_sh; a.o_sn = o_sn;
    a.scale = scale;
    hipLaunchKernelGGL(attn_span_short_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)(B * H)), dim3(256), 0, (hipStream_t)stream, a);
    return ae_check_launch("ae_attn_span_short_bf16");
}
