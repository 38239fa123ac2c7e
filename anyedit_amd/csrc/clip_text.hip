// CLIP text tower (FrozenCLIPEmbedder) for gfx950: the three pieces the library lacked.  The projections, the residual adds and the
// LayerNorms of the tower run on ae_gemm_bf16 / ae_layernorm_bf16; this file adds
//
//   ae_attn_causal_short_bf16   causal self-attention for sequences of at most 128 tokens (CLIP: 77), head_dim 32 or 64
//                               (transformers CLIPAttention with the causal mask CLIPTextTransformer builds; reached through
//                               ldm/modules/encoders/modules.py:136-139 self.transformer(input_ids=tokens));
//   ae_clip_embed_bf16          CLIPTextEmbeddings: token_embedding[ids] + position_embedding[0:N];
//   ae_clip_pool_eos_bf16       pooler_output: the final-normed row at the first eos token of each prompt (modules.py:141-142 "pooled");
//   ae_bias_act_f32_bf16        the activation between fc1 and fc2 (CLIPMLP), applied to the fp32 fc1 product + bias and rounded to bf16
//                               ONCE, after the activation: quick-GELU u * sigmoid(1.702 u) (OpenAI ViT-L/14) or erf-GELU (SD-2's ViT-H).
//
// Attention kernel: one 256-thread workgroup per (batch, head), built from the pieces of attn_short.hpp (operand placement, staging, one-pass
// softmax, PV, store).  Particular to it: K and V^T of the head are staged once in two LDS buffers behind ONE barrier (a whole row is <= 128
// keys = 8 key fragments), each of the 4 waves owns 32 query rows as two 16-row MFMA fragments, and 16-key fragments wholly above the
// diagonal of a query fragment are skipped (wave-uniform), not computed and masked; inside the diagonal fragment masked logits take the
// file-wide finite -1e30 (-ffinite-math-only) and their probability is forced to 0.
#include "attn_short.hpp"

namespace {

constexpr int NMAX = 128;  // longest sequence: 8 key fragments of 16 in registers per query fragment

struct BelowDiagonal {  // the live keys of query row qrow among the nlive fragments that were computed
    int nlive, qrow, lg;
    __device__ __forceinline__ bool operator()(int kf, int r, float) const { return kf < nlive && kf * 16 + lg * 4 + r <= qrow; }
};

template <int D>
__global__ __launch_bounds__(256) void attn_causal_short_kernel(const ShortAttnArgs p) {
    constexpr int NT = 256;
    constexpr int NC = D / 32;      // K = 32 MFMAs per (key fragment, query fragment)
    constexpr int NDF = D / 16;     // 16-row fragments of O^T
    constexpr int KROW = D + 8;     // LDS row strides (elements), +16 B pad
    constexpr int VROW = NMAX + 8;
    static_assert(D == 32 || D == 64, "head_dim 32 or 64");

    __shared__ __attribute__((aligned(16))) bf16_t sK[NMAX * KROW];
    __shared__ __attribute__((aligned(16))) bf16_t sVt[D * VROW];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const int N = p.N;
    const bf16_t* qp = p.q + (long)b * p.q_sb + (long)h * p.q_sh;

    // ---- stage K rows and V^T columns [0, NS), NS = N rounded up to 32 (one PV MFMA contracts 32 keys): keys >= N are ZEROS, written,
    // not loaded — their probability is 0, and 0 * (whatever LDS held) must stay 0
    const int NS = (N + 31) & ~31;
    stage_k_rows<D, NT>(sK, NS, tid, RangeRows{p.k + (long)b * p.k_sb + (long)h * p.k_sh, p.k_sn, 0, 0, N});
    stage_vt<D, NT>(sVt, VROW, NS, tid, RangeRows{p.v + (long)b * p.v_sb + (long)h * p.v_sh, p.v_sn, 0, 0, N});
    __syncthreads();  // the only barrier: nothing below writes LDS

    const int q0 = wave * 32;
    if (q0 >= N) return;
    const float c2 = p.scale * LOG2E;
    const int nfrag = (N + 15) >> 4;  // key fragments that hold a real key
    bf16_t* op = p.o + (long)b * p.o_sb + (long)h * p.o_sh;

#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int qa0 = q0 + a * 16;
        if (qa0 >= N) break;  // wave-uniform: no real query in this fragment
        const int qrow = qa0 + l15;
        const int nlive = min(qa0 / 16 + 1, nfrag);  // key fragments at or below the diagonal of this query fragment

        bf16x8_t qf[NC];
        load_q_frag(qf, qp + (long)min(qrow, N - 1) * p.q_sn, lg);

        // ---- S^T = K Q^T in the exp2 domain, masked above the diagonal
        f32x4 s[8];
        float mx = NEG_BIG;
#pragma unroll
        for (int kf = 0; kf < 8; ++kf) {
            if (kf < nlive) {
                const f32x4 acc = logit_frag(sK, kf, qf, l15, lg);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kf * 16 + lg * 4 + r;
                    const float v = key <= qrow ? acc[r] * c2 : NEG_BIG;
                    s[kf][r] = v;
                    mx = fmaxf(mx, v);
                }
            } else {
                s[kf] = (f32x4){NEG_BIG, NEG_BIG, NEG_BIG, NEG_BIG};
            }
        }
        mx = query_max(mx);  // key 0 is live for every row: mx is a real logit
        float rs = 0.f;
#pragma unroll
        for (int kf = 0; kf < 8; ++kf) s[kf] = exp_frag(s[kf], kf, mx, rs, BelowDiagonal{nlive, qrow, lg});
        const float inv = 1.0f / query_sum(rs);

        f32x4 o[NDF];
#pragma unroll
        for (int df = 0; df < NDF; ++df) o[df] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (2 * j < nlive) pv_step(o, s[2 * j], s[2 * j + 1], sVt, VROW, pv_col(j, lg), l15);
        if (qrow < N) store_o_row(op + (long)qrow * p.o_sn, o, inv, lg);  // rows >= N are never stored
    }
}

// one block per output row: 8 channels (16 bytes) per thread
template <typename IdT>
__global__ __launch_bounds__(128) void clip_embed_kernel(const IdT* __restrict__ ids, const bf16_t* __restrict__ tok, const bf16_t* __restrict__ pos,
                                                        bf16_t* __restrict__ out, int N, int C, int vocab) {
    const long row = blockIdx.x;
    long id = (long)ids[row];
    id = id < 0 ? 0 : (id >= vocab ? (long)vocab - 1 : id);  // an id outside the table is clamped into it, never a wild read
    const bf16_t* t = tok + id * C;
    const bf16_t* q = pos + (row % N) * C;
    bf16_t* y = out + row * C;
    for (int c = threadIdx.x * 8; c < C; c += blockDim.x * 8) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(t + c);
        const u32x4 b = *reinterpret_cast<const u32x4*>(q + c);
        u32x4 r;
        r.x = pack_bf16x2(bf16lo(a.x) + bf16lo(b.x), bf16hi(a.x) + bf16hi(b.x));
        r.y = pack_bf16x2(bf16lo(a.y) + bf16lo(b.y), bf16hi(a.y) + bf16hi(b.y));
        r.z = pack_bf16x2(bf16lo(a.z) + bf16lo(b.z), bf16hi(a.z) + bf16hi(b.z));
        r.w = pack_bf16x2(bf16lo(a.w) + bf16lo(b.w), bf16hi(a.w) + bf16hi(b.w));
        *reinterpret_cast<u32x4*>(y + c) = r;
    }
}

// pooled output: the (final-normed) row at the FIRST eos token of each prompt (row 0 when there is none, as argmax of an all-false mask)
template <typename IdT>
__global__ __launch_bounds__(128) void clip_pool_kernel(const IdT* __restrict__ ids, const bf16_t* __restrict__ z, bf16_t* __restrict__ out, int N, int C, long eos) {
    __shared__ int spos;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        int pos = 0;
        for (int n = 0; n < N; ++n)
            if ((long)ids[(long)b * N + n] == eos) { pos = n; break; }
        spos = pos;
    }
    __syncthreads();
    const bf16_t* src = z + ((long)b * N + spos) * C;
    bf16_t* dst = out + (long)b * C;
    for (int c = threadIdx.x * 8; c < C; c += blockDim.x * 8) *reinterpret_cast<u32x4*>(dst + c) = *reinterpret_cast<const u32x4*>(src + c);
}

__device__ __forceinline__ float quick_gelu_f(float u) {  // u * sigmoid(1.702 u)
    return u * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((-1.702f * LOG2E) * u));
}

template <int ACT>
__global__ __launch_bounds__(256) void bias_act_kernel(const float* __restrict__ u, long ldu, const float* __restrict__ bias, bf16_t* __restrict__ y, long ldy,
                                                      long M, int N) {
    const int n4 = N / 4;
    const long total = M * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long m = i / n4;
        const int c = (int)(i - m * n4) * 4;
        const f32x4 x = *reinterpret_cast<const f32x4*>(u + m * ldu + c);
        const f32x4 bb = *reinterpret_cast<const f32x4*>(bias + c);
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = x[e] + bb[e];
            r[e] = ACT == 0 ? quick_gelu_f(t) : gelu_erf_f(t);
        }
        *reinterpret_cast<u32x2*>(y + m * ldy + c) = (u32x2){pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3])};
    }
}

}  // namespace

extern "C" int ae_attn_causal_short_bf16(const void* q, const void* k, const void* v, void* out, int B, int H, int N, int D,
                                         long q_sb, long q_sh, long q_sn, long k_sb, long k_sh, long k_sn,
                                         long v_sb, long v_sh, long v_sn, long o_sb, long o_sh, long o_sn, float scale, void* stream) {
    static const ShortAttnRules rules{"ae_attn_causal_short_bf16", (1L << 31) - 1, NMAX, "a whole row of keys lives in registers", true, 0,
                                      "q/k/v must be 16-byte aligned, out 8-byte aligned"};
    ShortAttnArgs a{};
    if (const int e = short_attn_args(a, rules, q, k, v, nullptr, out, B, H, N, D, q_sb, q_sh, q_sn, k_sb, k_sh, k_sn, v_sb, v_sh, v_sn, o_sb, o_sh, o_sn, scale)) return e;
    const dim3 grid((unsigned)(B * H)), block(256);
    if (D == 32) hipLaunchKernelGGL((attn_causal_short_kernel<32>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((attn_causal_short_kernel<64>), grid, block, 0, (hipStream_t)stream, a);
    return ae_check_launch("ae_attn_causal_short_bf16");
}

extern "C" int ae_clip_embed_bf16(const void* ids, int ids_are_i64, const void* token_table, const void* position_table, void* out, int B, int N, int C,
                                  int vocab, int positions, void* stream) {
    AE_REQUIRE(ids && token_table && position_table && out, "ae_clip_embed_bf16: null pointer");
    AE_REQUIRE(B > 0 && N > 0 && C > 0 && vocab > 0 && (long)B * N < (1L << 31), "ae_clip_embed_bf16: bad sizes B=%d N=%d C=%d vocab=%d", B, N, C, vocab);
    AE_REQUIRE(N <= positions, "ae_clip_embed_bf16: %d tokens but the position table has %d rows", N, positions);
    AE_REQUIRE(C % 8 == 0, "ae_clip_embed_bf16: width %d must be a multiple of 8", C);
    AE_REQUIRE(((uintptr_t)token_table & 15) == 0 && ((uintptr_t)position_table & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                   ((uintptr_t)ids & (ids_are_i64 ? 7 : 3)) == 0,
               "ae_clip_embed_bf16: tables and out must be 16-byte aligned, ids aligned to their type");
    const dim3 grid((unsigned)((long)B * N)), block(128);
    if (ids_are_i64)
        hipLaunchKernelGGL((clip_embed_kernel<long>), grid, block, 0, (hipStream_t)stream, (const long*)ids, (const bf16_t*)token_table, (const bf16_t*)position_table,
                           (bf16_t*)out, N, C, vocab);
    else
        hipLaunchKernelGGL((clip_embed_kernel<int>), grid, block, 0, (hipStream_t)stream, (const int*)ids, (const bf16_t*)token_table, (const bf16_t*)position_table,
                           (bf16_t*)out, N, C, vocab);
    return ae_check_launch("ae_clip_embed_bf16");
}

extern "C" int ae_bias_act_f32_bf16(const float* u, long ldu, const float* bias, void* y, long ldy, long M, int N, int act, void* stream) {
    AE_REQUIRE(u && bias && y, "ae_bias_act_f32_bf16: null pointer");
    AE_REQUIRE(M > 0 && N > 0 && N % 4 == 0, "ae_bias_act_f32_bf16: bad sizes M=%ld N=%d (N must be a multiple of 4)", M, N);
    AE_REQUIRE(ldu >= N && ldy >= N && ldu % 4 == 0 && ldy % 4 == 0, "ae_bias_act_f32_bf16: row strides must be >= N and multiples of 4");
    AE_REQUIRE(((uintptr_t)u & 15) == 0 && ((uintptr_t)bias & 15) == 0 && ((uintptr_t)y & 7) == 0, "ae_bias_act_f32_bf16: u and bias must be 16-byte aligned, y 8-byte aligned");
    AE_REQUIRE(act == 0 || act == 1, "ae_bias_act_f32_bf16: act must be 0 (quick-GELU) or 1 (erf-GELU), got %d", act);
    const long total = M * (N / 4);
    const long want = (total + 255) / 256;
    const dim3 grid((unsigned)(want < 2048 ? want : 2048)), block(256);
    if (act == 0) hipLaunchKernelGGL((bias_act_kernel<0>), grid, block, 0, (hipStream_t)stream, u, ldu, bias, (bf16_t*)y, ldy, M, N);
    else hipLaunchKernelGGL((bias_act_kernel<1>), grid, block, 0, (hipStream_t)stream, u, ldu, bias, (bf16_t*)y, ldy, M, N);
    return ae_check_launch("ae_bias_act_f32_bf16");
}

extern "C" int ae_clip_pool_eos_bf16(const void* ids, int ids_are_i64, const void* z, void* out, int B, int N, int C, long eos_token_id, void* stream) {
    AE_REQUIRE(ids && z && out, "ae_clip_pool_eos_bf16: null pointer");
    AE_REQUIRE(B > 0 && N > 0 && C > 0 && C % 8 == 0, "ae_clip_pool_eos_bf16: bad sizes B=%d N=%d C=%d (C must be a multiple of 8)", B, N, C);
    AE_REQUIRE(((uintptr_t)z & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)ids & (ids_are_i64 ? 7 : 3)) == 0,
               "ae_clip_pool_eos_bf16: z and out must be 16-byte aligned, ids aligned to their type");
    const dim3 grid((unsigned)B), block(128);
    if (ids_are_i64)
        hipLaunchKernelGGL((clip_pool_kernel<long>), grid, block, 0, (hipStream_t)stream, (const long*)ids, (const bf16_t*)z, (bf16_t*)out, N, C, eos_token_id);
    else
        hipLaunchKernelGGL((clip_pool_kernel<int>), grid, block, 0, (hipStream_t)stream, (const int*)ids, (const bf16_t*)z, (bf16_t*)out, N, C, eos_token_id);
    return ae_check_launch("ae_clip_pool_eos_bf16");
}
