// GroundingDINO's text side (GroundingDINO/groundingdino/models/GroundingDINO/groundingdino.py:233-283, bertwarper.py:180-273, and the BertModel the
// reference takes from transformers) for gfx950: what the library could not run.  Projections, LayerNorms behind a residual, the GELU and feat_map
// run on existing entry points (ae_gemm_bf16, ae_layernorm_bf16, ae_bias_act_f32_bf16).  This file adds
//
//   ae_gdino_text_spans       generate_masks_with_special_tokens[_and_transfer_map] (bertwarper.py:180-273) in closed form: per token the key range
//                             [lo, hi) it may attend, its position id and, on request, the dense [B, N, N] mask — no host loop, no torch.nonzero.
//   ae_bert_embed_ln_bf16     BertEmbeddings: LayerNorm(word[ids] + position[position_ids] + token_type[type_ids]) in one launch; the sum is never stored.
//   ae_attn_span_short_bf16   BertSelfAttention's core under a block-diagonal mask: softmax(scale q k^T over keys [lo, hi)) v, head_dim 64.
//
// Span attention is attn_masked_short_kernel (attn_short.hpp, where the shared design is described) under the SpanMask policy of this file.  The
// mask is two integer compares against the lane's query's (lo, hi) instead of byte loads from a [B*H, N, N] array, which at BERT's 12 heads the
// caller would have to materialise per call.  And a workgroup stages, multiplies and accumulates only over ITS key window: the union of its 64
// queries' spans.  A key outside a query's span has probability exactly 0 in that query's row, and a key outside the union is staged as zeros
// and never read from memory.  No atomics, no scratch, no host synchronisation; two launches on the same inputs are bit-identical.  The
// embedding LayerNorm is built from the row-in-a-wave pieces of rowwave.hpp.
#include "attn_short.hpp"
#include "rowwave.hpp"

namespace {

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
#pragma unroll
    for (int i = 0; i < LN_MAXCH; ++i) {
        const int cc = lane + i * 64;
        x[i] = f32x8{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
        if (cc < ncc) {
            add8_bf16(x[i], w + cc * 8);
            add8_bf16(x[i], pr + cc * 8);
            add8_bf16(x[i], tr + cc * 8);
        }
    }
    wave_ln_store(x, lane, ncc, C, gamma, beta, eps, out + row * C);
}

// ------------------------------------------------------------------------------------------------------------------ span attention
// (lo, hi) of query n of sample b, forced into 0 <= lo < hi <= N: a span that breaks the contract can change a result, never an address
__device__ __forceinline__ int2 load_span(const int* __restrict__ spans, int b, int n, int N) {
    const int2 s = *reinterpret_cast<const int2*>(spans + 2 * ((long)b * N + n));
    const int lo = min(max(s.x, 0), N - 1);
    return make_int2(lo, max(min(s.y, N), lo + 1));
}

struct SpanMask {  // Mask policy of attn_masked_short_kernel: p.extra = spans [B, N, 2], shared by all heads
    int2 own;      // allowed keys of this lane's query
    // the union of the workgroup's 64 spans: every wave reduces the same 64, so the result is block-uniform without a barrier
    static __device__ __forceinline__ void window(const ShortAttnArgs& p, int b, int qb, int lane, int& ulo, int& uhi) {
        const int2 s = load_span((const int*)p.extra, b, min(qb + lane, p.N - 1), p.N);
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
    __device__ __forceinline__ SpanMask(const ShortAttnArgs& p, int b, int, int qc) : own(load_span((const int*)p.extra, b, qc, p.N)) {}
    __device__ __forceinline__ int frag(int key0) const { return key0; }
    __device__ __forceinline__ bool on(int key0, int r) const { return key0 + r >= own.x && key0 + r < own.y; }
};

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
    static const ShortAttnRules rules{"ae_attn_span_short_bf16", 65535, TXT_NMAX, "a window's logits live in registers", false, 8,
                                      "q/k/v must be 16-byte aligned, out and spans 8-byte aligned"};
    ShortAttnArgs a{};
    if (const int e = short_attn_args(a, rules, q, k, v, spans, out, B, H, N, D, q_sb, q_sh, q_sn, k_sb, k_sh, k_sn, v_sb, v_sh, v_sn, o_sb, o_sh, o_sn, scale)) return e;
    hipLaunchKernelGGL((attn_masked_short_kernel<64, 16, SpanMask>), dim3((unsigned)((N + 63) / 64), (unsigned)(B * H)), dim3(256), 0, (hipStream_t)stream, a);
    return ae_check_launch("ae_attn_span_short_bf16");
}
