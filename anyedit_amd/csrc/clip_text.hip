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
// Attention kernel: one 256-thread workgroup per (batch, head).  K and V^T of that head are staged in LDS once (rows >= N are written
// as zeros, never loaded), each of the 4 waves owns 32 query rows as two 16-row MFMA fragments.  The MFMA operand placement is the
// one of attention.hip: logits are computed transposed, S^T = K Q^T with v_mfma_f32_16x16x32_bf16, so a lane holds logits of ONE query
// row and the exponentiated P registers are already the B operand of O^T = V^T P^T (V is transposed while it is written to LDS, key
// index permuted per 64-key tile so a lane's 8 contraction slots are one 16-byte read).  A whole row (<= 128 keys = 8 key fragments)
// lives in registers, so the softmax is one pass: row maximum, exp2 with scale * log2(e) folded in, sum, normalise — no online rescale.
// 16-key fragments wholly above the diagonal of a query fragment are skipped (wave-uniform), not computed and masked; inside the
// diagonal fragment masked logits take the file-wide finite -1e30 (-ffinite-math-only) and their probability is forced to 0.
#include "common.hpp"

namespace {

constexpr int NMAX = 128;  // longest sequence: 8 key fragments of 16 in registers per query fragment
constexpr float LOG2E = 1.4426950408889634f;
constexpr float NEG_BIG = -1.0e30f;

struct CausalArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o;
    int B, H, N;
    long q_sb, q_sh, q_sn, k_sb, k_sh, k_sn, v_sb, v_sh, v_sn, o_sb, o_sh, o_sn;
    float scale;
};

__device__ __forceinline__ int vt_pos(int key) {  // inside one 64-key tile: key = 16 f + 4 g + r  ->  16 g + 4 f + r
    return ((key >> 2) & 3) * 16 + (key >> 4) * 4 + (key & 3);
}

template <int D>
__global__ __launch_bounds__(256) void attn_causal_short_kernel(const CausalArgs p) {
    constexpr int NT = 256;
    constexpr int NC = D / 32;      // K = 32 MFMAs per (key fragment, query fragment)
    constexpr int NDF = D / 16;     // 16-row fragments of O^T
    constexpr int DCH = D / 8;      // 16-byte chunks per row
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
    const bf16_t* kp = p.k + (long)b * p.k_sb + (long)h * p.k_sh;
    const bf16_t* vp = p.v + (long)b * p.v_sb + (long)h * p.v_sh;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    // ---- stage K rows and V^T columns [0, NS), NS = N rounded up to 32 (one PV MFMA contracts 32 keys): keys >= N are ZEROS, written,
    // not loaded — their probability is 0, and 0 * (whatever LDS held) must stay 0
    const int NS = (N + 31) & ~31;
    for (int id = tid; id < NS * DCH; id += NT) {
        const int key = id / DCH, c = id - key * DCH;
        const u32x4 t = key < N ? *reinterpret_cast<const u32x4*>(kp + (long)key * p.k_sn + c * 8) : zero4;
        *reinterpret_cast<u32x4*>(sK + key * KROW + c * 8) = t;
    }
    for (int id = tid; id < (NS / 2) * DCH; id += NT) {
        const int pr = id / DCH, c = id - pr * DCH;
        const int key = 2 * pr;
        const u32x4 t0 = key < N ? *reinterpret_cast<const u32x4*>(vp + (long)key * p.v_sn + c * 8) : zero4;
        const u32x4 t1 = key + 1 < N ? *reinterpret_cast<const u32x4*>(vp + (long)(key + 1) * p.v_sn + c * 8) : zero4;
        const int pos = (key & ~63) + vt_pos(key & 63);  // even; key + 1 lands at pos + 1
        const uint32_t a0[4] = {t0.x, t0.y, t0.z, t0.w};
        const uint32_t a1[4] = {t1.x, t1.y, t1.z, t1.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t lo = __builtin_amdgcn_perm(a1[e], a0[e], 0x05040100u);  // {a0.lo16, a1.lo16}: d = 8c + 2e
            const uint32_t hi = __builtin_amdgcn_perm(a1[e], a0[e], 0x07060302u);  // {a0.hi16, a1.hi16}: d = 8c + 2e + 1
            *reinterpret_cast<uint32_t*>(sVt + (c * 8 + 2 * e) * VROW + pos) = lo;
            *reinterpret_cast<uint32_t*>(sVt + (c * 8 + 2 * e + 1) * VROW + pos) = hi;
        }
    }
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

        // Q fragment (B operand of S^T = K Q^T): lane (q = l15, g) holds Q[q][32c + 8g .. +8]; rows >= N clamped into range (never stored)
        bf16x8_t qf[NC];
        {
            const bf16_t* qr = qp + (long)min(qrow, N - 1) * p.q_sn;
#pragma unroll
            for (int c = 0; c < NC; ++c) qf[c] = as_bf16x8(*reinterpret_cast<const u32x4*>(qr + c * 32 + lg * 8));
        }

        // ---- S^T = K Q^T: lane holds S^T[key = 16 kf + 4 g + r][q = l15], in the exp2 domain, masked above the diagonal
        f32x4 s[8];
        float mx = NEG_BIG;
#pragma unroll
        for (int kf = 0; kf < 8; ++kf) {
            if (kf < nlive) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const bf16x8_t kfr = as_bf16x8(*reinterpret_cast<const u32x4*>(sK + (kf * 16 + l15) * KROW + c * 32 + lg * 8));
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr, qf[c], acc, 0, 0, 0);
                }
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
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // key 0 is live for every row: mx is a real logit

        // ---- one-pass softmax: the whole row is in registers
        float rs = 0.f;
#pragma unroll
        for (int kf = 0; kf < 8; ++kf)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kf * 16 + lg * 4 + r;
                const float e = (kf < nlive && key <= qrow) ? __builtin_amdgcn_exp2f(s[kf][r] - mx) : 0.f;
                s[kf][r] = e;
                rs += e;
            }
        rs += __shfl_xor(rs, 16, 64);
        rs += __shfl_xor(rs, 32, 64);
        const float inv = 1.0f / rs;  // rs >= 1: the row maximum contributes exp2(0)

        // ---- O^T = V^T P^T: lane holds O^T[d = 16 df + 4 g + r][q = l15]; P as bf16, 32 keys (two fragments) per MFMA
        f32x4 o[NDF];
#pragma unroll
        for (int df = 0; df < NDF; ++df) o[df] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (2 * j < nlive) {
                u32x4 w;
                w.x = pack_bf16x2(s[2 * j][0], s[2 * j][1]);
                w.y = pack_bf16x2(s[2 * j][2], s[2 * j][3]);
                w.z = pack_bf16x2(s[2 * j + 1][0], s[2 * j + 1][1]);
                w.w = pack_bf16x2(s[2 * j + 1][2], s[2 * j + 1][3]);
                const bf16x8_t pb = as_bf16x8(w);
#pragma unroll
                for (int df = 0; df < NDF; ++df) {
                    const bf16x8_t vf = as_bf16x8(*reinterpret_cast<const u32x4*>(sVt + (df * 16 + l15) * VROW + (j >> 1) * 64 + lg * 16 + (j & 1) * 8));
                    o[df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pb, o[df], 0, 0, 0);
                }
            }
        }

        // ---- normalise and store: 4 consecutive d per lane -> 8-byte stores; rows >= N are never stored
        if (qrow < N) {
#pragma unroll
            for (int df = 0; df < NDF; ++df) {
                u32x2* dst = reinterpret_cast<u32x2*>(op + (long)qrow * p.o_sn + df * 16 + lg * 4);
                *dst = (u32x2){pack_bf16x2(o[df][0] * inv, o[df][1] * inv), pack_bf16x2(o[df][2] * inv, o[df][3] * inv)};
            }
        }
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
    AE_REQUIRE(q && k && v && out, "ae_attn_causal_short_bf16: null pointer");
    AE_REQUIRE(B > 0 && H > 0 && (long)B * H < (1L << 31), "ae_attn_causal_short_bf16: bad sizes B=%d H=%d", B, H);
    AE_REQUIRE(N >= 1 && N <= NMAX, "ae_attn_causal_short_bf16: sequence length %d outside [1, %d] (a whole row of keys lives in registers)", N, NMAX);
    AE_REQUIRE(D == 32 || D == 64, "ae_attn_causal_short_bf16: unsupported head_dim %d (supported: 32, 64)", D);
    AE_REQUIRE((q_sb | q_sh | q_sn | k_sb | k_sh | k_sn | v_sb | v_sh | v_sn) % 8 == 0 && (o_sb | o_sh | o_sn) % 4 == 0,
               "ae_attn_causal_short_bf16: strides must keep q/k/v rows 16-byte aligned and out rows 8-byte aligned");
    AE_REQUIRE(q_sb >= 0 && q_sh >= 0 && q_sn >= 0 && k_sb >= 0 && k_sh >= 0 && k_sn >= 0 && v_sb >= 0 && v_sh >= 0 && v_sn >= 0 && o_sb >= 0 && o_sh >= 0 && o_sn >= D,
               "ae_attn_causal_short_bf16: negative stride, or output rows that overlap");
    AE_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0 && ((uintptr_t)v & 15) == 0 && ((uintptr_t)out & 7) == 0,
               "ae_attn_causal_short_bf16: q/k/v must be 16-byte aligned, out 8-byte aligned");
    AE_REQUIRE(scale > 0.f, "ae_attn_causal_short_bf16: scale must be positive");
    CausalArgs a{};
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.o = (bf16_t*)out;
    a.B = B; a.H = H; a.N = N;
    a.q_sb = q_sb; a.q_sh = q_sh; a.q_sn = q_sn; a.k_sb = k_sb; a.k_sh = k_sh; a.k_sn = k_sn;
    a.v_sb = v_sb; a.v_sh = v_sh; a.v_sn = v_sn; a.o_sb = o_sb; a.o_sh = o_sh; a.o_sn = o_sn;
    a.scale = scale;
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
