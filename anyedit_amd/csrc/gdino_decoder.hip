// GroundingDINO's language-guided query selection, decoder bookkeeping and heads (GroundingDINO/groundingdino/models/GroundingDINO/
// transformer.py:284-327 query selection, :598-735 TransformerDecoder, groundingdino.py:317-335 heads) for gfx950: the device code the library
// lacked.  Attention, the deformable sampling core, LayerNorms and every wide projection run on existing entry points.  This file adds
//
//   ae_contrastive_bf16       ContrastiveEmbed.forward (utils.py:233-268) x y^T with the token mask and the -inf padding to max_text_len, and / or
//                             its row maximum (transformer.py:295) without the logits ever being stored.
//   ae_topk_rows_f32          the first k entries of a stable descending sort of every row (transformer.py:301, with a defined order among ties).
//   ae_gdino_proposals_f32    gen_encoder_output_proposals (utils.py:56-116, learnedwh=None) in one launch.
//   ae_gdino_query_sine       reference_points_input (transformer.py:667-671) and gen_sineembed_for_position of its level-0 slice (utils.py:204-230).
//   ae_gdino_box_refine_f32   the last Linear of a box MLP plus the anchor update (transformer.py:721-724, groundingdino.py:322-324).
//
// No atomics, no scratch, no floating-point reduction whose order depends on timing: two launches on the same inputs are bit-identical.  Divisions
// are IEEE, logf / expf / sinf / cosf are the library's: the proposals' validity flags depend on fp32 values bit for bit.
//
// Contrastive: one 256-thread workgroup owns 64 rows of x of one sample (one 16-row MFMA fragment per wave; the rows live in registers as the B
// operand for the whole kernel) and STREAMS the sample's text rows through LDS in column tiles of 64 tokens (64 x (C + 8) bf16 <= 33 792 bytes,
// + 64 bytes of live flags).  Keeping all 256 x 256 text rows resident would take 132 KB and leave one workgroup per CU; the tile is read once
// per workgroup from L2 either way.  S^T = Y X^T with v_mfma_f32_16x16x32_bf16: a lane holds 4 consecutive tokens of ONE row of x, so the logits
// leave as 16-byte stores and the row maximum is two cross-lane steps.
//
// Top-k: one 1024-thread workgroup per row.  Scores become order-preserving 32-bit keys (NaN of either sign above +inf, -0.0 = +0.0).  The k-th
// largest key K is found bit by bit from the top (32 counting passes over the row, block-reduced through LDS without atomics).  Then every
// thread walks a CONTIGUOUS slice of the row, so a block-wide exclusive scan of (keys above K, keys equal to K) gives every selected entry its slot
// in index order: all keys above K, then the lowest-index k - G of the keys equal to K.  The k (key, index) pairs are ordered by a rank sort in
// LDS (k reads per thread, no barriers): pairs are distinct, so the ranks are a permutation.
#include "common.hpp"
#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------------------------ contrastive
constexpr int CE_CMAX = 256;
constexpr int CE_TMAX = 256;
constexpr int CE_TILE = 64;                 // tokens staged at a time
constexpr int CE_ROWS = 64;                 // rows of x per workgroup
constexpr int CE_NCMAX = CE_CMAX / 32;

struct ContrastiveArgs {
    const bf16_t* x; long ldx;              // [B * N rows]
    const bf16_t* y;                        // [B, T, C] contiguous
    const uint8_t* tmask;                   // [B, T], non-zero = used token; may be null
    float* logits; long ldl;                // [B * N rows][max_text_len]; may be null
    float* rowmax;                          // [B * N]; may be null
    int N, T, C, max_text_len;
};

__global__ __launch_bounds__(256) void contrastive_kernel(const ContrastiveArgs p) {
    __shared__ __attribute__((aligned(16))) bf16_t sY[CE_TILE * (CE_CMAX + 8)];
    __shared__ __attribute__((aligned(4))) uint8_t sLive[CE_TILE];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * CE_ROWS + wave * 16;
    const bool active = q0 < p.N;           // wave-uniform; an idle wave still stages and meets every barrier
    const int qrow = q0 + l15;
    const int nc = p.C >> 5, dch = p.C >> 3, krow = p.C + 8;
    const float NEG_INF = -__builtin_inff();
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    // rows of x (B operand): lane (row l15, g) holds x[row][32c + 8g .. +8]; rows >= N clamped into range (never stored)
    bf16x8_t xf[CE_NCMAX];
    {
        const bf16_t* xr = p.x + ((long)b * p.N + min(qrow, p.N - 1)) * p.ldx;
#pragma unroll
        for (int c = 0; c < CE_NCMAX; ++c) xf[c] = as_bf16x8(c < nc ? *reinterpret_cast<const u32x4*>(xr + c * 32 + lg * 8) : zero4);
    }
    const bf16_t* ybase = p.y + (long)b * p.T * p.C;
    const uint8_t* mbase = p.tmask ? p.tmask + (long)b * p.T : nullptr;
    float* lrow = p.logits ? p.logits + ((long)b * p.N + min(qrow, p.N - 1)) * p.ldl : nullptr;
    const bool vec_store = (p.ldl & 3) == 0;
    const int t_end = p.logits ? p.max_text_len : p.T;   // columns T .. max_text_len - 1 exist only in the stored logits

    float mx = NEG_INF;
    for (int t0 = 0; t0 < t_end; t0 += CE_TILE) {        // block-uniform
        const bool has_tokens = t0 < p.T;
        const int nkf = has_tokens ? min(CE_TILE / 16, (p.T - t0 + 15) >> 4) : 0;
        if (has_tokens) {
            __syncthreads();   // the previous tile has been read
            for (int id = tid; id < CE_TILE * dch; id += 256) {
                const int tok = id / dch, c = id - tok * dch;
                const u32x4 t = t0 + tok < p.T ? *reinterpret_cast<const u32x4*>(ybase + (long)(t0 + tok) * p.C + c * 8) : zero4;
                *reinterpret_cast<u32x4*>(sY + tok * krow + c * 8) = t;
            }
            if (tid < CE_TILE) sLive[tid] = (t0 + tid < p.T && (!mbase || mbase[t0 + tid])) ? 1 : 0;
            __syncthreads();
        }
        if (!active) continue;
#pragma unroll
        for (int kf = 0; kf < CE_TILE / 16; ++kf) {
            f32x4 s = {NEG_INF, NEG_INF, NEG_INF, NEG_INF};
            if (kf < nkf) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < CE_NCMAX; ++c)
                    if (c < nc) {
                        const bf16x8_t yf = as_bf16x8(*reinterpret_cast<const u32x4*>(sY + (kf * 16 + l15) * krow + c * 32 + lg * 8));
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf, xf[c], acc, 0, 0, 0);
                    }
                const uint32_t live = *reinterpret_cast<const uint32_t*>(sLive + kf * 16 + lg * 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[r] = ((live >> (8 * r)) & 0xffu) ? acc[r] : NEG_INF;
                    mx = fmaxf(mx, s[r]);
                }
            }
            const int tc = t0 + kf * 16 + lg * 4;        // this lane's 4 columns
            if (lrow && qrow < p.N && tc < p.max_text_len) {
                if (vec_store && tc + 3 < p.max_text_len) {
                    *reinterpret_cast<f32x4*>(lrow + tc) = s;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (tc + r < p.max_text_len) lrow[tc + r] = s[r];
                }
            }
        }
    }
    if (!active || !p.rowmax) return;       // no barrier below
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (lg == 0 && qrow < p.N) p.rowmax[(long)b * p.N + qrow] = mx;
}

// ------------------------------------------------------------------------------------------------------------------ top-k
constexpr int TK_THREADS = 1024;
constexpr int TK_WAVES = TK_THREADS / 64;
constexpr int TK_KMAX = 1024;
constexpr int TK_NMAX = 1 << 24;

// ascending order-preserving key of torch's descending sort order: NaN (either sign) > +inf > ... > +0.0 == -0.0 > ... > -inf; never 0
__device__ __forceinline__ uint32_t topk_key(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// inclusive scan inside a wave
__device__ __forceinline__ int wave_scan_i(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

__global__ __launch_bounds__(TK_THREADS) void topk_rows_kernel(const float* __restrict__ scores, long ld, int* __restrict__ out, int N, int k) {
    __shared__ int sCnt[2][TK_WAVES];       // double-buffered: one barrier per counting pass
    __shared__ int sScanG[TK_WAVES], sScanE[TK_WAVES];
    __shared__ uint32_t sKey[TK_KMAX];
    __shared__ int sIdx[TK_KMAX];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = scores + (long)blockIdx.x * ld;
    int* orow = out + (long)blockIdx.x * k;

    // ---- K = the k-th largest key: the largest K with count(key >= K) >= k, built from the top bit down
    uint32_t K = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = K | (1u << bit);
        int c = 0;
        for (int i = tid; i < N; i += TK_THREADS) c += topk_key(row[i]) >= cand ? 1 : 0;
        c = wave_sum_i(c);
        int* cnt = sCnt[bit & 1];
        if (lane == 0) cnt[wave] = c;
        __syncthreads();
        int total = 0;
#pragma unroll
        for (int w = 0; w < TK_WAVES; ++w) total += cnt[w];
        if (total >= k) K = cand;           // block-uniform
    }

    // ---- compaction in index order: thread t owns indices [t * chunk, (t + 1) * chunk)
    const int chunk = (N + TK_THREADS - 1) / TK_THREADS;
    const int i0 = min((long)tid * chunk, (long)N), i1 = min((long)i0 + chunk, (long)N);
    int g = 0, e = 0;
    for (int i = i0; i < i1; ++i) {
        const uint32_t key = topk_key(row[i]);
        g += key > K ? 1 : 0;
        e += key == K ? 1 : 0;
    }
    const int gs = wave_scan_i(g, lane), es = wave_scan_i(e, lane);
    if (lane == 63) { sScanG[wave] = gs; sScanE[wave] = es; }
    __syncthreads();
    int gbase = 0, ebase = 0, G = 0;
#pragma unroll
    for (int w = 0; w < TK_WAVES; ++w) {
        const int tg = sScanG[w], te = sScanE[w];
        if (w < wave) { gbase += tg; ebase += te; }
        G += tg;
    }
    int gpos = gbase + gs - g;              // slot of this thread's first key above K   (G < k by the choice of K)
    int epos = G + ebase + es - e;          // slot of this thread's first key equal to K (the first k - G of them are taken)
    for (int i = i0; i < i1; ++i) {
        const uint32_t key = topk_key(row[i]);
        if (key > K) {
            sKey[gpos] = key; sIdx[gpos] = i; ++gpos;
        } else if (key == K) {
            if (epos < k) { sKey[epos] = key; sIdx[epos] = i; }
            ++epos;
        }
    }
    __syncthreads();

    // ---- rank sort of the k pairs: descending key, ascending index
    if (tid < k) {
        const uint32_t mk = sKey[tid];
        const int mi = sIdx[tid];
        int rank = 0;
        for (int j = 0; j < k; ++j) {
            const uint32_t ok = sKey[j];
            const int oi = sIdx[j];
            rank += (ok > mk || (ok == mk && oi < mi)) ? 1 : 0;
        }
        orow[rank] = mi;
    }
}

// ------------------------------------------------------------------------------------------------------------------ proposals
constexpr int PR_LMAX = 8;

struct ProposalArgs {
    const uint8_t* mask;                    // [B, N], non-zero = padding
    float* prop;                            // [B, N, 4]
    uint8_t* keep;                          // [B, N]
    int N, L;
    int H[PR_LMAX], W[PR_LMAX], start[PR_LMAX];
};

__global__ __launch_bounds__(256) void proposals_kernel(const ProposalArgs p) {
    __shared__ int sPart[2][4];
    __shared__ int sValid[PR_LMAX][2];      // (valid_H, valid_W) of this sample per level
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const uint8_t* m = p.mask + (long)b * p.N;
    for (int l = 0; l < p.L; ++l) {         // block-uniform
        const int H = p.H[l], W = p.W[l];
        const uint8_t* ml = m + p.start[l];
        int ch = 0, cw = 0;
        for (int i = tid; i < H + W; i += 256) {
            if (i < H) ch += ml[(long)i * W] ? 0 : 1;     // first column (utils.py:74)
            else cw += ml[i - H] ? 0 : 1;                 // first row    (utils.py:75)
        }
        ch = wave_sum_i(ch);
        cw = wave_sum_i(cw);
        __syncthreads();                    // the previous level's partials have been read
        if (lane == 0) { sPart[0][wave] = ch; sPart[1][wave] = cw; }
        __syncthreads();
        if (tid == 0) {
            sValid[l][0] = sPart[0][0] + sPart[0][1] + sPart[0][2] + sPart[0][3];
            sValid[l][1] = sPart[1][0] + sPart[1][1] + sPart[1][2] + sPart[1][3];
        }
    }
    __syncthreads();
    const int n = blockIdx.x * 256 + tid;
    if (n >= p.N) return;
    int l = 0, W = p.W[0], st = 0;          // the level of this token: uniform reads of the arguments, selected per lane
    for (int j = 1; j < p.L; ++j) {
        const int sj = p.start[j], wj = p.W[j];
        if (n >= sj) { l = j; W = wj; st = sj; }
    }
    const int r = n - st;
    const int y = r / W, x = r - y * W;
    const float px = ((float)x + 0.5f) / (float)sValid[l][1];
    const float py = ((float)y + 0.5f) / (float)sValid[l][0];
    const float wh = 0.05f * (float)(1 << l);
    const float q[4] = {px, py, wh, wh};
    bool ok = m[n] == 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) ok = ok && (q[c] > 0.01f) && (q[c] < 0.99f);   // a NaN (0 / 0 never occurs: x + 0.5 > 0) or inf fails
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = ok ? logf(q[c] / (1.0f - q[c])) : __builtin_inff();
    *reinterpret_cast<f32x4*>(p.prop + ((long)b * p.N + n) * 4) = o;
    p.keep[(long)b * p.N + n] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------ query sine
// 10000 ** (2 * (j // 2) / 128) for j = 0, 2, .. 126 (utils.py:208-209), each the fp32 nearest to the exact value — the values torch's fp32 pow gives
__device__ const float SINE_DIM_T[64] = {
    1.0f, 1.1547819375991821f, 1.3335214853286743f, 1.539926528930664f, 1.778279423713684f, 2.053524971008301f, 2.3713736534118652f, 2.738419532775879f,
    3.1622776985168457f, 3.6517412662506104f, 4.216965198516846f, 4.869675159454346f, 5.6234130859375f, 6.493816375732422f, 7.498941898345947f, 8.659643173217773f,
    10.0f, 11.547820091247559f, 13.335214614868164f, 15.39926528930664f, 17.782794952392578f, 20.535249710083008f, 23.71373748779297f, 27.384197235107422f,
    31.62277603149414f, 36.51741409301758f, 42.16965103149414f, 48.69675064086914f, 56.234130859375f, 64.93816375732422f, 74.98941802978516f, 86.596435546875f,
    100.0f, 115.47819519042969f, 133.35214233398438f, 153.99264526367188f, 177.82794189453125f, 205.35250854492188f, 237.1373748779297f, 273.8419494628906f,
    316.2277526855469f, 365.17413330078125f, 421.6965026855469f, 486.967529296875f, 562.34130859375f, 649.3816528320312f, 749.8942260742188f, 865.9642944335938f,
    1000.0f, 1154.781982421875f, 1333.521484375f, 1539.926513671875f, 1778.2794189453125f, 2053.525146484375f, 2371.373779296875f, 2738.419677734375f,
    3162.277587890625f, 3651.7412109375f, 4216.96484375f, 4869.67529296875f, 5623.4130859375f, 6493.81640625f, 7498.94189453125f, 8659.6435546875f,
};

// one workgroup per (sample, query): thread t writes sin / cos of pair t % 64 of coordinate slot t / 64 (slots y, x, w, h: utils.py:227)
__global__ __launch_bounds__(256) void query_sine_kernel(const float* __restrict__ ref, const float* __restrict__ vr, float* __restrict__ rpi, bf16_t* __restrict__ emb,
                                                         long lde, int nq, int L) {
    const long row = blockIdx.x;            // b * nq + q
    const int b = (int)(row / nq);
    const int tid = threadIdx.x;
    const float* rr = ref + row * 4;
    const float* vb = vr + (long)b * L * 2;
    for (int i = tid; i < L * 4; i += 256) {               // reference_points[:, :, None] * cat([valid_ratios, valid_ratios], -1)
        const int l = i >> 2, c = i & 3;
        rpi[row * L * 4 + i] = rr[c] * vb[l * 2 + (c & 1)];
    }
    const int slot = tid >> 6, pair = tid & 63;
    const int c = slot == 0 ? 1 : (slot == 1 ? 0 : slot);
    const float v = rr[c] * vb[c & 1];                      // level 0
    const float arg = (v * 6.283185307179586f) / SINE_DIM_T[pair];
    *reinterpret_cast<uint32_t*>(emb + row * lde + slot * 128 + pair * 2) = pack_bf16x2(sinf(arg), cosf(arg));
}

// ------------------------------------------------------------------------------------------------------------------ box refinement
// one wave per row: u = h W3^T + b3 + (ref_is_logit ? ref : inverse_sigmoid(ref)), boxes = sigmoid(u)
__global__ __launch_bounds__(256) void box_refine_kernel(const float* __restrict__ h, long ldh, const float* __restrict__ w3, const float* __restrict__ b3,
                                                         const float* __restrict__ ref, float* __restrict__ boxes, float* __restrict__ u_out, long M, int ref_is_logit) {
    const int lane = threadIdx.x & 63;
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;                     // wave-uniform, no barrier in this kernel
    const f32x4 hv = *reinterpret_cast<const f32x4*>(h + m * ldh + lane * 4);
    float d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w3 + j * 256 + lane * 4);
        float s = hv[0] * wv[0];
        s = __builtin_fmaf(hv[1], wv[1], s);
        s = __builtin_fmaf(hv[2], wv[2], s);
        s = __builtin_fmaf(hv[3], wv[3], s);
        d[j] = wave_reduce_sum(s);          // xor butterfly: every lane holds the same sum
    }
    if (lane >= 4) return;
    const float dot = lane == 0 ? d[0] : (lane == 1 ? d[1] : (lane == 2 ? d[2] : d[3]));
    const float r = ref[m * 4 + lane];
    float base;
    if (ref_is_logit) {
        base = r;
    } else {                                // util/misc.py inverse_sigmoid, eps = 1e-3
        const float x = fminf(fmaxf(r, 0.f), 1.f);
        const float x1 = fmaxf(x, 1e-3f), x2 = fmaxf(1.0f - x, 1e-3f);
        base = logf(x1 / x2);
    }
    const float u = (dot + b3[lane]) + base;
    boxes[m * 4 + lane] = 1.0f / (1.0f + expf(-u));
    if (u_out) u_out[m * 4 + lane] = u;
}

}  // namespace

extern "C" int ae_contrastive_bf16(const void* x, long ldx, const void* y, const void* token_mask, float* logits, long ldl, float* rowmax, int B, int N, int T, int C,
                                   int max_text_len, void* stream) {
    AE_REQUIRE(x && y, "ae_contrastive_bf16: null pointer");
    AE_REQUIRE(logits || rowmax, "ae_contrastive_bf16: neither logits nor rowmax is asked for");
    AE_REQUIRE(C >= 32 && C % 32 == 0 && C <= CE_CMAX, "ae_contrastive_bf16: C=%d must be a multiple of 32, at most %d", C, CE_CMAX);
    AE_REQUIRE(T >= 1 && T <= max_text_len && max_text_len <= CE_TMAX, "ae_contrastive_bf16: need 1 <= T=%d <= max_text_len=%d <= %d", T, max_text_len, CE_TMAX);
    AE_REQUIRE(B >= 1 && B <= 65535 && N >= 1, "ae_contrastive_bf16: bad sizes B=%d N=%d (B at most 65535)", B, N);
    AE_REQUIRE((long)B * N < (1L << 31), "ae_contrastive_bf16: %ld rows are past the 2^31 limit", (long)B * N);
    AE_REQUIRE(ldx >= C && ldx % 8 == 0, "ae_contrastive_bf16: row stride of x %ld must be >= C and a multiple of 8", ldx);
    AE_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "ae_contrastive_bf16: x and y must be 16-byte aligned");
    if (logits) {
        AE_REQUIRE(ldl >= max_text_len, "ae_contrastive_bf16: row stride of logits %ld is below max_text_len %d", ldl, max_text_len);
        AE_REQUIRE(((uintptr_t)logits & 15) == 0, "ae_contrastive_bf16: logits must be 16-byte aligned");
    }
    ContrastiveArgs a{};
    a.x = (const bf16_t*)x; a.ldx = ldx; a.y = (const bf16_t*)y; a.tmask = (const uint8_t*)token_mask;
    a.logits = logits; a.ldl = logits ? ldl : 0; a.rowmax = rowmax;
    a.N = N; a.T = T; a.C = C; a.max_text_len = max_text_len;
    hipLaunchKernelGGL(contrastive_kernel, dim3((unsigned)((N + CE_ROWS - 1) / CE_ROWS), (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    return ae_check_launch("ae_contrastive_bf16");
}

extern "C" int ae_topk_rows_max_n(void) { return TK_NMAX; }

extern "C" int ae_topk_rows_f32(const float* scores, long ld, int* out, int B, int N, int k, void* stream) {
    AE_REQUIRE(scores && out, "ae_topk_rows_f32: null pointer");
    AE_REQUIRE(B >= 1 && N >= 1, "ae_topk_rows_f32: bad sizes B=%d N=%d", B, N);
    AE_REQUIRE(N <= TK_NMAX, "ae_topk_rows_f32: N=%d is above the largest supported row length %d", N, TK_NMAX);
    AE_REQUIRE(k >= 1 && k <= N && k <= TK_KMAX, "ae_topk_rows_f32: k=%d must be in [1, min(N=%d, %d)]", k, N, TK_KMAX);
    AE_REQUIRE(ld >= N, "ae_topk_rows_f32: row stride %ld is below N=%d", ld, N);
    hipLaunchKernelGGL(topk_rows_kernel, dim3((unsigned)B), dim3(TK_THREADS), 0, (hipStream_t)stream, scores, ld, out, N, k);
    return ae_check_launch("ae_topk_rows_f32");
}

extern "C" int ae_gdino_proposals_f32(const void* padding_mask, const int* shapes_hw, const int* level_start, int L, float* proposals, void* keep, int B, int N,
                                      void* stream) {
    AE_REQUIRE(padding_mask && shapes_hw && level_start && proposals && keep, "ae_gdino_proposals_f32: null pointer");
    AE_REQUIRE(L >= 1 && L <= PR_LMAX, "ae_gdino_proposals_f32: %d levels outside [1, %d]", L, PR_LMAX);
    AE_REQUIRE(B >= 1 && B <= 65535 && N >= 1, "ae_gdino_proposals_f32: bad sizes B=%d N=%d (B at most 65535)", B, N);
    AE_REQUIRE(((uintptr_t)proposals & 15) == 0, "ae_gdino_proposals_f32: proposals must be 16-byte aligned");
    ProposalArgs a{};
    long cur = 0;
    for (int l = 0; l < L; ++l) {
        const int H = shapes_hw[2 * l], W = shapes_hw[2 * l + 1];
        AE_REQUIRE(H >= 1 && W >= 1 && (long)H * W < (1L << 31), "ae_gdino_proposals_f32: level %d has shape (%d, %d)", l, H, W);
        AE_REQUIRE(level_start[l] == cur, "ae_gdino_proposals_f32: level %d starts at %d, the shapes before it say %ld", l, level_start[l], cur);
        a.H[l] = H; a.W[l] = W; a.start[l] = (int)cur;
        cur += (long)H * W;
        AE_REQUIRE(cur <= N, "ae_gdino_proposals_f32: the levels hold more than N=%d tokens", N);
    }
    AE_REQUIRE(cur == N, "ae_gdino_proposals_f32: the levels hold %ld tokens, N=%d", cur, N);
    a.mask = (const uint8_t*)padding_mask; a.prop = proposals; a.keep = (uint8_t*)keep; a.N = N; a.L = L;
    hipLaunchKernelGGL(proposals_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    return ae_check_launch("ae_gdino_proposals_f32");
}

extern "C" int ae_gdino_query_sine(const float* ref, const float* valid_ratios, float* ref_input, void* embed, long lde, int B, int nq, int L, void* stream) {
    AE_REQUIRE(ref && valid_ratios && ref_input && embed, "ae_gdino_query_sine: null pointer");
    AE_REQUIRE(B >= 1 && nq >= 1 && L >= 1 && L <= 64 && (long)B * nq < (1L << 31), "ae_gdino_query_sine: bad sizes B=%d nq=%d L=%d (L at most 64)", B, nq, L);
    AE_REQUIRE(lde >= 512 && lde % 2 == 0 && ((uintptr_t)embed & 3) == 0, "ae_gdino_query_sine: embedding rows are 512 wide; stride %ld must be >= 512 and even", lde);
    hipLaunchKernelGGL(query_sine_kernel, dim3((unsigned)((long)B * nq)), dim3(256), 0, (hipStream_t)stream, ref, valid_ratios, ref_input, (bf16_t*)embed, lde, nq, L);
    return ae_check_launch("ae_gdino_query_sine");
}

extern "C" int ae_gdino_box_refine_f32(const float* h, long ldh, const float* w3, const float* b3, const float* ref, float* boxes, float* u_out, long M, int ref_is_logit,
                                       void* stream) {
    AE_REQUIRE(h && w3 && b3 && ref && boxes, "ae_gdino_box_refine_f32: null pointer");
    AE_REQUIRE(M >= 1 && (M + 3) / 4 < (1L << 31), "ae_gdino_box_refine_f32: bad row count %ld", M);
    AE_REQUIRE(ldh >= 256 && ldh % 4 == 0, "ae_gdino_box_refine_f32: h rows are 256 wide; stride %ld must be >= 256 and a multiple of 4", ldh);
    AE_REQUIRE((((uintptr_t)h | (uintptr_t)w3) & 15) == 0, "ae_gdino_box_refine_f32: h and w3 must be 16-byte aligned");
    hipLaunchKernelGGL(box_refine_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, h, ldh, w3, b3, ref, boxes, u_out, M, ref_is_logit);
    return ae_check_launch("ae_gdino_box_refine_f32");
}
