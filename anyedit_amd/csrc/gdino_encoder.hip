// GroundingDINO's feature enhancer (GroundingDINO/groundingdino/models/GroundingDINO/transformer.py:406-595 TransformerEncoder) for gfx950: the
// two attentions the library could not run.  LayerNorms, every projection, the ReLU feed-forwards and the deformable sampling core run on existing
// entry points (ae_layernorm_bf16, ae_gemm_bf16, ae_ln_gemm_bf16, ae_linear_f32, ae_ms_deform_attn_fwd_f32).  This file adds
//
//   ae_biattn_bf16              BiMultiHeadAttention.forward from the first bmm to the two output bmms (fuse_modules.py:174-225): ONE logit
//                               matrix scale q k^T [Nv, Nt] per (sample, head) normalised along BOTH axes, head_dim 256.  No logit or
//                               probability matrix is ever stored: each direction is a streaming attention that recomputes the logits.
//   ae_attn_masked_short_bf16   the core of nn.MultiheadAttention as transformer_vanilla.py:115 calls it: self-attention over at most 256 text
//                               tokens with a full per-(batch, head, query) boolean mask, head_dim 32 or 64.
//   ae_scale_residual_f32_bf16  out = res + gamma (u + bias) with one rounding: BiAttentionBlock's layer-scaled residual (fuse_modules.py:293-294) on
//                               the fp32 out-projection product, and the residual behind the fp32 deformable attention (transformer.py:793).
//
// Bi-attention: both directions are the same kernel with the roles of the operands exchanged.
//   image direction  out_v = softmax over text keys (mask_l removed) (scale q k^T) val_l     queries q [Nv],  keys k [Nt],  values val_l
//   text direction   out_l = softmax over image keys (mask_v removed) (scale k q^T) val_v    queries k [Nt],  keys q [Nv],  values val_v
// One 256-thread workgroup owns 64 query rows (one 16-row MFMA fragment per wave) of one (sample, head) and walks a range of keys in chunks of
// BI_CHUNK = 64.  A chunk's key rows (64 x 256 bf16) and then its values, transposed (256 x 64), pass through ONE LDS buffer of 36 KB one after
// the other — K and V of a head at 256 x 256 are 128 KB each and do not fit beside each other, so they are streamed in key chunks and three
// workgroups (150 registers: three waves per SIMD) share a CU to cover each other's staging.  Operand placement, staging, the logit fragment
// and the PV step are those of attn_short.hpp (8 K steps for head_dim 256); a row does not fit in registers here, so the running maximum / sum
// live in the lane (online softmax in the exp2 domain, each softmax subtracts its own running maximum).  The image direction walks all
// (<= 256) text keys in one workgroup and stores bf16.  The text direction has few queries and very many keys: its key range
// is cut into at most BI_MAX_SPLIT partials of whole chunks (ae_biattn_split_rows); every partial writes its running maximum, its sum and its un-normalised fp32 accumulator to the workspace, and a combine kernel merges them IN PARTIAL ORDER — no
// floating-point atomics, so two launches on the same inputs are bit-identical.  The workspace is bounded by BI_MAX_SPLIT * Nt * 258 floats per
// (sample, head): nothing grows with Nv * Nt.
//
// Left out on purpose (fuse_modules.py:181-202): the subtraction of the global attn_weights.max() and both clamps to +-50000.  A softmax is
// invariant to a shift of its row, so the global maximum changes a result only through the clamps, and those act only when the logits of one
// call span more than 50000.
//
// Masked short attention is attn_masked_short_kernel (attn_short.hpp) under the ByteMask policy of this file: the window is all of [0, N).
#include "attn_short.hpp"

namespace {

// ------------------------------------------------------------------------------------------------------------------ bi-attention
constexpr int BI_D = 256;          // head_dim of the fusion attention (embed_dim 1024 / 4 heads)
constexpr int BI_NT_MAX = 256;     // text tokens
constexpr int BI_QTILE = 64;       // query rows per workgroup
constexpr int BI_CHUNK = 64;       // keys staged at a time
constexpr int BI_MAX_SPLIT = 32;   // partials of the text direction
constexpr int BI_MIN_SPLIT_CHUNKS = 2;   // a partial walks at least this many chunks
constexpr int BI_WS_ROW = BI_D + 2;      // floats per (partial, query) in the workspace: accumulator, running maximum, sum

struct BiArgs {
    const bf16_t* q; long ldq;       // queries [B * Nq rows]
    const bf16_t* k; long ldk;       // keys    [B * Nk rows]
    const bf16_t* v; long ldv;       // values  [B * Nk rows]
    const uint8_t* kmask;            // [B, Nk], non-zero = padded key, removed; may be null
    bf16_t* out; long ldo;           // !PARTIAL: [B * Nq rows]
    float* ws;                       // PARTIAL: [B * heads][nsplit][Nq][BI_WS_ROW]
    int heads, Nq, Nk, split_rows, nsplit;
    float c2;                        // scale * log2(e)
};

__host__ __device__ inline int bi_split_rows(int Nv) {
    const int nchunks = (Nv + BI_CHUNK - 1) / BI_CHUNK;
    int cps = (nchunks + BI_MAX_SPLIT - 1) / BI_MAX_SPLIT;
    cps = cps < BI_MIN_SPLIT_CHUNKS ? BI_MIN_SPLIT_CHUNKS : cps;
    return cps * BI_CHUNK;
}

template <bool PARTIAL>
__global__ __launch_bounds__(256, 2) void biattn_kernel(const BiArgs p) {
    constexpr int NT = 256;
    constexpr int D = BI_D;
    constexpr int NC = D / 32;               // K = 32 MFMA steps per logit fragment
    constexpr int NDF = D / 16;              // 16-row fragments of O^T
    constexpr int KROW = D + 8;              // LDS row strides (elements), +16 B pad
    constexpr int VROW = BI_CHUNK + 8;
    constexpr int BUF = (BI_CHUNK * KROW > D * VROW) ? BI_CHUNK * KROW : D * VROW;

    __shared__ __attribute__((aligned(16))) bf16_t sBuf[BUF];                 // the chunk's K rows, then its V^T
    __shared__ __attribute__((aligned(4))) uint8_t sLive[BI_CHUNK];           // 1: the key exists and is not masked

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const int bh = blockIdx.z, b = bh / p.heads, h = bh - b * p.heads;
    const int split = blockIdx.y;
    const int q0 = blockIdx.x * BI_QTILE + wave * 16;
    const bool active = q0 < p.Nq;           // wave-uniform; an idle wave still stages and meets every barrier
    const int qrow = q0 + l15;
    const int k_begin = split * p.split_rows;
    const int k_end = min(p.Nk, k_begin + p.split_rows);

    const bf16_t* kbase = p.k + (long)b * p.Nk * p.ldk + h * D;
    const bf16_t* vbase = p.v + (long)b * p.Nk * p.ldv + h * D;
    const uint8_t* mbase = p.kmask ? p.kmask + (long)b * p.Nk : nullptr;

    bf16x8_t qf[NC];   // rows >= Nq clamped into range (never stored)
    load_q_frag(qf, p.q + ((long)b * p.Nq + min(qrow, p.Nq - 1)) * p.ldq + h * D, lg);

    f32x4 o[NDF];
#pragma unroll
    for (int df = 0; df < NDF; ++df) o[df] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run = NEG_BIG, l_run = 0.f;

    for (int c0 = k_begin; c0 < k_end; c0 += BI_CHUNK) {   // block-uniform
        const int nkf = min(BI_CHUNK / 16, (k_end - c0 + 15) >> 4);   // key fragments of this chunk that hold a key
        __syncthreads();   // the previous chunk's V^T has been read
        // ---- stage K rows of keys [c0, c0 + 64): a key past k_end is zeros, written, never loaded
        stage_k_rows<D, NT>(sBuf, BI_CHUNK, tid, RangeRows{kbase, p.ldk, c0, 0, k_end});
        if (tid < BI_CHUNK) sLive[tid] = (c0 + tid < k_end && !(mbase && mbase[c0 + tid])) ? 1 : 0;
        __syncthreads();

        // ---- S^T = K Q^T: lane holds the logits of keys c0 + 16 kf + 4 g + r for query l15, exp2 domain; online softmax
        f32x4 s[BI_CHUNK / 16];
        if (active) {
            float mx = m_run;
#pragma unroll
            for (int kf = 0; kf < BI_CHUNK / 16; ++kf) {
                if (kf < nkf) {
                    const f32x4 acc = logit_frag(sBuf, kf, qf, l15, lg);
                    const uint32_t live = *reinterpret_cast<const uint32_t*>(sLive + kf * 16 + lg * 4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = ((live >> (8 * r)) & 0xffu) ? acc[r] * p.c2 : NEG_BIG;
                        s[kf][r] = v;
                        mx = fmaxf(mx, v);
                    }
                } else {
                    s[kf] = (f32x4){NEG_BIG, NEG_BIG, NEG_BIG, NEG_BIG};
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float alpha = __builtin_amdgcn_exp2f(m_run - mx);   // no live key so far: exp2(0) = 1 on an accumulator of zeros
            float rs = 0.f;
#pragma unroll
            for (int kf = 0; kf < BI_CHUNK / 16; ++kf)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = s[kf][r] > 0.5f * NEG_BIG ? __builtin_amdgcn_exp2f(s[kf][r] - mx) : 0.f;   // a removed key: exactly 0
                    s[kf][r] = e;
                    rs += e;
                }
            rs += __shfl_xor(rs, 16, 64);
            rs += __shfl_xor(rs, 32, 64);
            l_run = l_run * alpha + rs;
            m_run = mx;
#pragma unroll
            for (int df = 0; df < NDF; ++df) o[df] *= alpha;
        }
        __syncthreads();   // every wave has read the K rows

        // ---- stage V^T of the same keys into the same buffer (key index permuted inside the 64-key tile: a lane's 8 contraction slots are 16 bytes)
        stage_vt<D, NT>(sBuf, VROW, BI_CHUNK, tid, RangeRows{vbase, p.ldv, c0, 0, k_end});
        __syncthreads();

        // ---- O^T += V^T P^T: lane holds O^T[d = 16 df + 4 g + r][q = l15]; P as bf16, 32 keys (two fragments) per MFMA
        if (active) {
#pragma unroll
            for (int j = 0; j < BI_CHUNK / 32; ++j)
                if (2 * j < nkf) pv_step(o, s[2 * j], s[2 * j + 1], sBuf, VROW, pv_col(j, lg), l15);
        }
    }

    if (!active || qrow >= p.Nq) return;   // no barrier below
    if (PARTIAL) {
        float* w = p.ws + (((long)bh * p.nsplit + split) * p.Nq + qrow) * BI_WS_ROW;
#pragma unroll
        for (int df = 0; df < NDF; ++df) {
            float* dst = w + df * 16 + lg * 4;   // BI_WS_ROW is even: 8-byte aligned
            *reinterpret_cast<f32x2*>(dst) = (f32x2){o[df][0], o[df][1]};
            *reinterpret_cast<f32x2*>(dst + 2) = (f32x2){o[df][2], o[df][3]};
        }
        if (lg == 0) *reinterpret_cast<f32x2*>(w + BI_D) = (f32x2){m_run, l_run};
    } else {
        store_o_row(p.out + ((long)b * p.Nq + qrow) * p.ldo + h * D, o, 1.0f / l_run, lg);   // contract: at least one live key per sample
    }
}

// one workgroup per (sample, head, query), one thread per channel: the partials are merged in partial order 0, 1, ... — a fixed summation order
__global__ __launch_bounds__(BI_D) void biattn_combine_kernel(const float* __restrict__ ws, bf16_t* __restrict__ out, long ldo, int heads, int Nq, int nsplit) {
    const int j = blockIdx.x, bh = blockIdx.y, b = bh / heads, h = bh - b * heads;
    const int d = threadIdx.x;
    const float* w = ws + ((long)bh * nsplit * Nq + j) * BI_WS_ROW;
    const long step = (long)Nq * BI_WS_ROW;
    float M = NEG_BIG;
    for (int s = 0; s < nsplit; ++s) M = fmaxf(M, w[s * step + BI_D]);
    float acc = 0.f, den = 0.f;
    for (int s = 0; s < nsplit; ++s) {
        const float f = __builtin_amdgcn_exp2f(w[s * step + BI_D] - M);   // a partial without a live key: accumulator and sum are zeros
        acc = __builtin_fmaf(w[s * step + d], f, acc);
        den = __builtin_fmaf(w[s * step + BI_D + 1], f, den);
    }
    out[((long)b * Nq + j) * ldo + h * BI_D + d] = f32_to_bf16(acc / den);
}

// ------------------------------------------------------------------------------------------------------------------ masked short attention
constexpr int MS_NMAX = 256;

struct ByteMask {  // Mask policy of attn_masked_short_kernel: p.extra = uint8 [B*H, N, N], non-zero = the key is allowed
    const uint8_t* mrow;   // allowed keys of this lane's query
    int N;
    static __device__ __forceinline__ void window(const ShortAttnArgs& p, int, int, int, int& ulo, int& uhi) { ulo = 0; uhi = p.N; }
    __device__ __forceinline__ ByteMask(const ShortAttnArgs& p, int, int bh, int qc) : mrow((const uint8_t*)p.extra + ((long)bh * p.N + qc) * p.N), N(p.N) {}
    __device__ __forceinline__ uint32_t frag(int key0) const {  // byte r: key key0 + r
        uint32_t allow = 0u;
        if ((N & 3) == 0) {  // a lane's 4 keys are then one aligned 4-byte read, all inside the row
            if (key0 < N) allow = *reinterpret_cast<const uint32_t*>(mrow + key0);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (key0 + r < N) allow |= (mrow[key0 + r] ? 1u : 0u) << (8 * r);
        }
        return allow;
    }
    __device__ __forceinline__ bool on(uint32_t allow, int r) const { return (allow >> (8 * r)) & 0xffu; }
};

// out = res + gamma * (u + bias): the residual of a sub-block whose branch is an fp32 product, rounded to bf16 once
__global__ __launch_bounds__(256) void scale_residual_kernel(const float* __restrict__ u, long ldu, const float* __restrict__ bias, const float* __restrict__ gamma,
                                                            const bf16_t* __restrict__ res, long ldr, bf16_t* __restrict__ out, long ldo, long M, int N) {
    const int n4 = N / 4;
    const long total = M * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long m = i / n4;
        const int c = (int)(i - m * n4) * 4;
        const f32x4 x = *reinterpret_cast<const f32x4*>(u + m * ldu + c);
        const f32x4 bb = bias ? *reinterpret_cast<const f32x4*>(bias + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        const f32x4 g = gamma ? *reinterpret_cast<const f32x4*>(gamma + c) : (f32x4){1.f, 1.f, 1.f, 1.f};
        const u32x2 rr = *reinterpret_cast<const u32x2*>(res + m * ldr + c);
        const float r[4] = {bf16lo(rr.x), bf16hi(rr.x), bf16lo(rr.y), bf16hi(rr.y)};
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = __builtin_fmaf(g[e], x[e] + bb[e], r[e]);
        *reinterpret_cast<u32x2*>(out + m * ldo + c) = (u32x2){pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3])};
    }
}

}  // namespace

extern "C" int ae_scale_residual_f32_bf16(const float* u, long ldu, const float* bias, const float* gamma, const void* res, long ldr, void* out, long ldo, long M,
                                          int N, void* stream) {
    AE_REQUIRE(u && res && out, "ae_scale_residual_f32_bf16: null pointer");
    AE_REQUIRE(M > 0 && N > 0 && N % 4 == 0, "ae_scale_residual_f32_bf16: bad sizes M=%ld N=%d (N must be a multiple of 4)", M, N);
    AE_REQUIRE(ldu >= N && ldr >= N && ldo >= N && (ldu | ldr | ldo) % 4 == 0, "ae_scale_residual_f32_bf16: row strides must be >= N and multiples of 4");
    AE_REQUIRE((((uintptr_t)u | (uintptr_t)bias | (uintptr_t)gamma) & 15) == 0 && (((uintptr_t)res | (uintptr_t)out) & 7) == 0,
               "ae_scale_residual_f32_bf16: u, bias and gamma must be 16-byte aligned, res and out 8-byte aligned");
    const long total = M * (N / 4);
    const long want = (total + 255) / 256;
    hipLaunchKernelGGL(scale_residual_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, (hipStream_t)stream, u, ldu, bias, gamma, (const bf16_t*)res, ldr,
                       (bf16_t*)out, ldo, M, N);
    return ae_check_launch("ae_scale_residual_f32_bf16");
}

extern "C" int ae_biattn_split_rows(int Nv) { return Nv >= 1 ? bi_split_rows(Nv) : 0; }

extern "C" long ae_biattn_workspace_bytes(int B, int heads, int Nv, int Nt, int D) {
    if (B <= 0 || heads <= 0 || Nv <= 0 || Nt <= 0 || Nt > BI_NT_MAX || D != BI_D) return 0;
    const int rows = bi_split_rows(Nv);
    const long nsplit = (Nv + rows - 1) / rows;
    return (long)B * heads * nsplit * Nt * BI_WS_ROW * (long)sizeof(float);
}

extern "C" int ae_biattn_bf16(const void* q, long ldq, const void* k, long ldk, const void* val_v, long ldvv, const void* val_l, long ldvl, const void* mask_v,
                              const void* mask_l, void* out_v, long ldov, void* out_l, long ldol, int B, int heads, int Nv, int Nt, int D, float scale,
                              void* workspace, long workspace_bytes, void* stream) {
    AE_REQUIRE(q && k && val_v && val_l && out_v && out_l && workspace, "ae_biattn_bf16: null pointer");
    AE_REQUIRE(D == BI_D, "ae_biattn_bf16: head_dim %d must be %d (the only one the fusion attention is built for)", D, BI_D);
    AE_REQUIRE(Nt >= 1 && Nt <= BI_NT_MAX, "ae_biattn_bf16: %d text tokens outside [1, %d]", Nt, BI_NT_MAX);
    AE_REQUIRE(B > 0 && heads > 0 && Nv >= 1 && (long)B * heads <= 65535, "ae_biattn_bf16: bad sizes B=%d heads=%d Nv=%d (B*heads at most 65535)", B, heads, Nv);
    AE_REQUIRE((long)B * Nv < (1L << 31), "ae_biattn_bf16: %ld image token rows are past the 2^31 limit", (long)B * Nv);
    const long C = (long)heads * D;
    AE_REQUIRE(ldq >= C && ldk >= C && ldvv >= C && ldvl >= C && ldov >= C && ldol >= C && (ldq | ldk | ldvv | ldvl | ldov | ldol) % 8 == 0,
               "ae_biattn_bf16: every row stride must be >= heads*D = %ld and a multiple of 8", C);
    AE_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)val_v | (uintptr_t)val_l | (uintptr_t)out_v | (uintptr_t)out_l | (uintptr_t)workspace) & 15) == 0,
               "ae_biattn_bf16: every pointer must be 16-byte aligned");
    AE_REQUIRE(scale > 0.f, "ae_biattn_bf16: scale must be positive");
    const long need = ae_biattn_workspace_bytes(B, heads, Nv, Nt, D);
    AE_REQUIRE(workspace_bytes >= need, "ae_biattn_bf16: workspace of %ld bytes, %ld needed (ae_biattn_workspace_bytes)", workspace_bytes, need);
    const int rows = bi_split_rows(Nv), nsplit = (Nv + rows - 1) / rows;
    const hipStream_t st = (hipStream_t)stream;

    BiArgs a{};   // image direction: queries q, keys k, values val_l, every key in one workgroup
    a.q = (const bf16_t*)q; a.ldq = ldq; a.k = (const bf16_t*)k; a.ldk = ldk; a.v = (const bf16_t*)val_l; a.ldv = ldvl;
    a.kmask = (const uint8_t*)mask_l; a.out = (bf16_t*)out_v; a.ldo = ldov; a.ws = nullptr;
    a.heads = heads; a.Nq = Nv; a.Nk = Nt; a.split_rows = BI_NT_MAX; a.nsplit = 1; a.c2 = scale * LOG2E;
    const long qtiles_v = ((long)Nv + BI_QTILE - 1) / BI_QTILE;
    AE_REQUIRE(qtiles_v < (1L << 31), "ae_biattn_bf16: %ld query tiles are past the grid limit", qtiles_v);
    hipLaunchKernelGGL(biattn_kernel<false>, dim3((unsigned)qtiles_v, 1, (unsigned)(B * heads)), dim3(256), 0, st, a);

    BiArgs t{};   // text direction: queries k, keys q, values val_v, key range cut into nsplit partials
    t.q = (const bf16_t*)k; t.ldq = ldk; t.k = (const bf16_t*)q; t.ldk = ldq; t.v = (const bf16_t*)val_v; t.ldv = ldvv;
    t.kmask = (const uint8_t*)mask_v; t.out = nullptr; t.ldo = 0; t.ws = (float*)workspace;
    t.heads = heads; t.Nq = Nt; t.Nk = Nv; t.split_rows = rows; t.nsplit = nsplit; t.c2 = scale * LOG2E;
    hipLaunchKernelGGL(biattn_kernel<true>, dim3((unsigned)((Nt + BI_QTILE - 1) / BI_QTILE), (unsigned)nsplit, (unsigned)(B * heads)), dim3(256), 0, st, t);
    hipLaunchKernelGGL(biattn_combine_kernel, dim3((unsigned)Nt, (unsigned)(B * heads)), dim3(BI_D), 0, st, (const float*)workspace, (bf16_t*)out_l, ldol, heads, Nt,
                       nsplit);
    return ae_check_launch("ae_biattn_bf16");
}

extern "C" int ae_attn_masked_short_bf16(const void* q, const void* k, const void* v, const void* mask, void* out, int B, int H, int N, int D, long q_sb, long q_sh,
                                         long q_sn, long k_sb, long k_sh, long k_sn, long v_sb, long v_sh, long v_sn, long o_sb, long o_sh, long o_sn, float scale,
                                         void* stream) {
    static const ShortAttnRules rules{"ae_attn_masked_short_bf16", 65535, MS_NMAX, "a whole row of keys lives in registers", true, 4,
                                      "q/k/v must be 16-byte aligned, out 8-byte aligned, mask 4-byte aligned"};
    ShortAttnArgs a{};
    if (const int e = short_attn_args(a, rules, q, k, v, mask, out, B, H, N, D, q_sb, q_sh, q_sn, k_sb, k_sh, k_sn, v_sb, v_sh, v_sn, o_sb, o_sh, o_sn, scale)) return e;
    const dim3 grid((unsigned)((N + 63) / 64), (unsigned)(B * H)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (D == 32) {
        if (N <= 128) hipLaunchKernelGGL((attn_masked_short_kernel<32, 8, ByteMask>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((attn_masked_short_kernel<32, 16, ByteMask>), grid, block, 0, st, a);
    } else {
        if (N <= 128) hipLaunchKernelGGL((attn_masked_short_kernel<64, 8, ByteMask>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((attn_masked_short_kernel<64, 16, ByteMask>), grid, block, 0, st, a);
    }
    return ae_check_launch("ae_attn_masked_short_bf16");
}
