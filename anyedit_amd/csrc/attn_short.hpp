// The row-in-registers attention design shared by the encoder towers, defined once: clip_text.hip (causal), gdino_encoder.hip (byte mask,
// streaming bi-attention), gdino_text.hip (spans) and swin.hip (windows) build their kernels from these pieces.
//
// Operand placement.  Logits are computed transposed, S^T = K Q^T with v_mfma_f32_16x16x32_bf16: K rows (stride D + 8 elements) are the A
// operand read from LDS, lane (q = lane & 15, g = lane >> 4) holds Q[q][32 c + 8 g .. +8] as the B operand, and the result fragment gives the
// lane the logits of keys 16 kf + 4 g + r (r = 0 .. 3) of ONE query row.  A whole row of at most 16 key fragments therefore lives in the lane's
// registers, the softmax is one fp32 pass in the exp2 domain (row maximum, exp2, sum; lanes g = 0 .. 3 of a query meet through two
// __shfl_xor), and the exponentiated registers of two neighbouring fragments, rounded to bf16, are already the B operand of O^T = V^T P^T.
// V is transposed while it is written to LDS, with the key index permuted inside each 64-key tile (vt_pos) so that the lane's 8 contraction
// slots — keys 16 (2 j) + 4 g + r and 16 (2 j + 1) + 4 g + r — are one 16-byte read.  O^T gives the lane 4 consecutive channels of its
// query: one 8-byte store per 16 channels.  Keys and query rows that exist only because a size is rounded up to whole fragments are excluded
// outright: the key is staged as zeros (written, never loaded) and its probability is exactly 0; the query row is clamped for its loads and
// never stored.
//
// Every helper is a forceinline template; loaders and predicates are small structs taken by value (a loader lambda kept in a variable once
// put its captures in scratch: DESIGN.md §7a).
#pragma once
#include "attn_layout.hpp"  // LOG2E, NEG_BIG, vt_pos, store_vt_pair: shared with the streaming 64-key-tile design (attn_tile.hpp)

namespace {

// ---------------------------------------------------------------------------------------------------------------- staging
// A loader returns the 16-byte chunk c (channels 8c .. 8c+7) of staged key `rel`.  RangeRows: staged key rel is row off + rel of a strided
// matrix when that row lies in [lo, hi), zeros otherwise (written, never loaded).
struct RangeRows {
    const bf16_t* base; long stride; int off, lo, hi;
    __device__ __forceinline__ u32x4 operator()(int rel, int c) const {
        const int key = off + rel;
        return (key >= lo && key < hi) ? *reinterpret_cast<const u32x4*>(base + (long)key * stride + c * 8) : (u32x4){0u, 0u, 0u, 0u};
    }
};

template <int D, int NT, class Load>  // K rows of staged keys [0, nk) -> sK, row stride D + 8
__device__ __forceinline__ void stage_k_rows(bf16_t* sK, int nk, int tid, Load load) {
    constexpr int DCH = D / 8;
    for (int id = tid; id < nk * DCH; id += NT) {
        const int key = id / DCH, c = id - key * DCH;
        *reinterpret_cast<u32x4*>(sK + key * (D + 8) + c * 8) = load(key, c);
    }
}

template <int D, int NT, class Load>  // V^T of staged keys [0, nk), nk even -> sVt, row stride vrow, keys permuted inside whole 64-key tiles
__device__ __forceinline__ void stage_vt(bf16_t* sVt, int vrow, int nk, int tid, Load load) {
    constexpr int DCH = D / 8;
    for (int id = tid; id < (nk / 2) * DCH; id += NT) {
        const int pr = id / DCH, c = id - pr * DCH;
        const int key = 2 * pr;  // its position is even; key + 1 lands beside it
        store_vt_pair(sVt, vrow, c, (key & ~63) + vt_pos(key & 63), load(key, c), load(key + 1, c));
    }
}

// ---------------------------------------------------------------------------------------------------------------- one query fragment
template <int NC>  // Q fragment of the lane's query row qr: NC = D / 32 K-steps
__device__ __forceinline__ void load_q_frag(bf16x8_t (&qf)[NC], const bf16_t* qr, int lg) {
#pragma unroll
    for (int c = 0; c < NC; ++c) qf[c] = as_bf16x8(*reinterpret_cast<const u32x4*>(qr + c * 32 + lg * 8));
}

template <int NC>  // raw logits of key fragment kf: the lane gets keys 16 kf + 4 g + r of query l15
__device__ __forceinline__ f32x4 logit_frag(const bf16_t* sK, int kf, const bf16x8_t (&qf)[NC], int l15, int lg) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const bf16x8_t kfr = as_bf16x8(*reinterpret_cast<const u32x4*>(sK + (kf * 16 + l15) * (NC * 32 + 8) + c * 32 + lg * 8));
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr, qf[c], acc, 0, 0, 0);
    }
    return acc;
}

// ---- the one-pass softmax of a row held as exp2-domain logits f32x4 s[NKF].  The loops over the row stay in the kernels, which hand single
// fragments to these helpers by value: a helper that took the row array by reference cost up to 16 registers per kernel.
//     mx = query_max(mx);  rs = 0;  for kf: s[kf] = exp_frag(s[kf], kf, mx, rs, live);  inv = 1 / query_sum(rs);
// Contract: the row has a live key, so the maximum is a real logit and the sum >= 1.
__device__ __forceinline__ float query_max(float mx) {  // over the four lanes g = 0 .. 3 of a query row
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    return fmaxf(mx, __shfl_xor(mx, 32, 64));
}
__device__ __forceinline__ float query_sum(float rs) {
    rs += __shfl_xor(rs, 16, 64);
    return rs + __shfl_xor(rs, 32, 64);
}

struct NotRemoved {  // live: every removed logit was set to NEG_BIG
    __device__ __forceinline__ bool operator()(int, int, float v) const { return v > 0.5f * NEG_BIG; }
};

template <class Live>  // un-normalised probabilities of fragment kf, exactly 0 where !live(kf, r, logit); adds them to the lane's sum rs
__device__ __forceinline__ f32x4 exp_frag(const f32x4 sk, int kf, float mx, float& rs, Live live) {
    f32x4 e;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        e[r] = live(kf, r, sk[r]) ? __builtin_amdgcn_exp2f(sk[r] - mx) : 0.f;
        rs += e[r];
    }
    return e;
}

// O^T += V^T P^T over the 32 keys of fragment pair j = (s0, s1) of the row, P rounded to bf16 here; the lane gets O^T[16 df + 4 g + r][q = l15].
// vcol: the lane's 16-byte column of sVt for the pair, pv_col(j, lg) when sVt holds whole 64-key tiles side by side.
__device__ __forceinline__ int pv_col(int j, int lg) { return (j >> 1) * 64 + lg * 16 + (j & 1) * 8; }

template <int NDF>
__device__ __forceinline__ void pv_step(f32x4 (&o)[NDF], const f32x4 s0, const f32x4 s1, const bf16_t* sVt, int vrow, int vcol, int l15) {
    const bf16x8_t pb = as_bf16x8((u32x4){pack_bf16x2(s0[0], s0[1]), pack_bf16x2(s0[2], s0[3]), pack_bf16x2(s1[0], s1[1]), pack_bf16x2(s1[2], s1[3])});
#pragma unroll
    for (int df = 0; df < NDF; ++df) {
        const bf16x8_t vf = as_bf16x8(*reinterpret_cast<const u32x4*>(sVt + (df * 16 + l15) * vrow + vcol));
        o[df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pb, o[df], 0, 0, 0);
    }
}

template <int NDF>  // normalise and store the lane's query row: 4 consecutive d per fragment -> 8-byte stores
__device__ __forceinline__ void store_o_row(bf16_t* orow, const f32x4 (&o)[NDF], float inv, int lg) {
#pragma unroll
    for (int df = 0; df < NDF; ++df)
        *reinterpret_cast<u32x2*>(orow + df * 16 + lg * 4) = (u32x2){pack_bf16x2(o[df][0] * inv, o[df][1] * inv), pack_bf16x2(o[df][2] * inv, o[df][3] * inv)};
}

// ---------------------------------------------------------------------------------------------------------------- strided q/k/v entry points
struct ShortAttnArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o;
    const void* extra;   // the byte mask or the spans; null for causal
    int H, N;
    long q_sb, q_sh, q_sn, k_sb, k_sh, k_sn, v_sb, v_sh, v_sn, o_sb, o_sh, o_sn;
    float scale;
};

// Masked attention over one key window, the kernel of ae_attn_masked_short_bf16 (Mask = the byte mask, gdino_encoder.hip) and of
// ae_attn_span_short_bf16 (Mask = the spans, gdino_text.hip).  One workgroup per (batch, head, 64 query rows), one 16-row query fragment per
// wave.  The keys of the workgroup's window pass through ONE LDS buffer: first the K rows (the window's logits, <= NKF key fragments, then live
// in registers), then V^T.  A Mask supplies
//   static window(p, b, qb, lane, ulo, uhi)   the block-uniform key range [ulo, uhi) that the workgroup's 64 queries (from row qb) may attend;
//                                             it is staged widened to whole 64-key tiles, keys outside it as zeros;
//   Mask(p, b, bh, qc)                        the lane's state for its query row qc;
//   frag(key0), on(frag, r)                   whether key key0 + r is allowed for that row.
// Contract: every row allows a key.
template <int D, int NKF, class Mask>  // NKF: 16-key fragments a window may span, a multiple of 4 (V^T is permuted inside whole 64-key tiles)
__global__ __launch_bounds__(256) void attn_masked_short_kernel(const ShortAttnArgs p) {
    constexpr int NT = 256;
    constexpr int NS = NKF * 16;    // the widest window
    constexpr int NC = D / 32;
    constexpr int NDF = D / 16;
    constexpr int KROW = D + 8;
    constexpr int VROW = NS + 8;
    constexpr int BUF = (NS * KROW > D * VROW) ? NS * KROW : D * VROW;
    static_assert((D == 32 || D == 64) && NKF % 4 == 0 && NKF <= 16, "head_dim 32 or 64, whole 64-key tiles, at most 256 keys");

    __shared__ __attribute__((aligned(16))) bf16_t sBuf[BUF];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
    const int N = p.N;
    const int qb = blockIdx.x * 64;

    int ulo, uhi;
    Mask::window(p, b, qb, lane, ulo, uhi);
    const int w0 = ulo & ~63;                        // 0 <= w0 <= ulo < uhi <= N <= 16 NKF
    const int nk = ((uhi + 63) & ~63) - w0;          // staged keys: whole tiles
    const int nfrag = (uhi - w0 + 15) >> 4;          // 16-key fragments that hold a key of the window

    const int q0 = qb + wave * 16;
    const bool active = q0 < N;   // wave-uniform; an idle wave still stages and meets every barrier
    const int qrow = q0 + l15, qc = min(qrow, N - 1);

    stage_k_rows<D, NT>(sBuf, nk, tid, RangeRows{p.k + (long)b * p.k_sb + (long)h * p.k_sh, p.k_sn, w0, ulo, uhi});
    __syncthreads();

    f32x4 s[NKF];
    float inv = 0.f;
    if (active) {
        bf16x8_t qf[NC];
        load_q_frag(qf, p.q + (long)b * p.q_sb + (long)h * p.q_sh + (long)qc * p.q_sn, lg);
        const Mask mask(p, b, bh, qc);
        const float c2 = p.scale * LOG2E;
        float mx = NEG_BIG;
#pragma unroll
        for (int kf = 0; kf < NKF; ++kf) {
            if (kf < nfrag) {
                const f32x4 acc = logit_frag(sBuf, kf, qf, l15, lg);
                const auto fr = mask.frag(w0 + kf * 16 + lg * 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = mask.on(fr, r) ? acc[r] * c2 : NEG_BIG;
                    s[kf][r] = v;
                    mx = fmaxf(mx, v);
                }
            } else {
                s[kf] = (f32x4){NEG_BIG, NEG_BIG, NEG_BIG, NEG_BIG};
            }
        }
        mx = query_max(mx);
        float rs = 0.f;
#pragma unroll
        for (int kf = 0; kf < NKF; ++kf) s[kf] = exp_frag(s[kf], kf, mx, rs, NotRemoved());
        inv = 1.0f / query_sum(rs);
    }
    __syncthreads();   // every wave has read the K rows

    stage_vt<D, NT>(sBuf, VROW, nk, tid, RangeRows{p.v + (long)b * p.v_sb + (long)h * p.v_sh, p.v_sn, w0, ulo, uhi});
    __syncthreads();   // the last barrier

    if (!active) return;
    f32x4 o[NDF];
#pragma unroll
    for (int df = 0; df < NDF; ++df) o[df] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NKF / 2; ++j)
        if (2 * j < nfrag) pv_step(o, s[2 * j], s[2 * j + 1], sBuf, VROW, pv_col(j, lg), l15);
    if (qrow < N) store_o_row(p.o + (long)b * p.o_sb + (long)h * p.o_sh + (long)qrow * p.o_sn, o, inv, lg);
}

// What differs between the three entry points in the shared requirements
struct ShortAttnRules {
    const char* fn;           // the entry point's name, for its messages
    long bh_max;              // B * H limit: the grid's y dimension (65535), or 2^31 - 1 on the x dimension
    int n_max;
    const char* n_why;
    bool d32;                 // head_dim 32 is built beside 64
    unsigned extra_align;     // byte alignment of `extra`; 0: there is none
    const char* align_text;
};

// the requirements the three entry points share, in the order and the words each of them had; fills `a`
inline int short_attn_args(ShortAttnArgs& a, const ShortAttnRules& r, const void* q, const void* k, const void* v, const void* extra, void* out, int B, int H, int N,
                           int D, long q_sb, long q_sh, long q_sn, long k_sb, long k_sh, long k_sn, long v_sb, long v_sh, long v_sn, long o_sb, long o_sh, long o_sn,
                           float scale) {
    AE_REQUIRE(q && k && v && out && (extra || !r.extra_align), "%s: null pointer", r.fn);
    AE_REQUIRE(B > 0 && H > 0 && (long)B * H <= r.bh_max, "%s: bad sizes B=%d H=%d%s", r.fn, B, H, r.bh_max == 65535 ? " (B*H at most 65535)" : "");
    AE_REQUIRE(N >= 1 && N <= r.n_max, "%s: sequence length %d outside [1, %d] (%s)", r.fn, N, r.n_max, r.n_why);
    if (r.d32) AE_REQUIRE(D == 32 || D == 64, "%s: unsupported head_dim %d (supported: 32, 64)", r.fn, D);
    else AE_REQUIRE(D == 64, "%s: unsupported head_dim %d (64, BERT's, is the only one built)", r.fn, D);
    AE_REQUIRE((q_sb | q_sh | q_sn | k_sb | k_sh | k_sn | v_sb | v_sh | v_sn) % 8 == 0 && (o_sb | o_sh | o_sn) % 4 == 0,
               "%s: strides must keep q/k/v rows 16-byte aligned and out rows 8-byte aligned", r.fn);
    AE_REQUIRE(q_sb >= 0 && q_sh >= 0 && q_sn >= 0 && k_sb >= 0 && k_sh >= 0 && k_sn >= 0 && v_sb >= 0 && v_sh >= 0 && v_sn >= 0 && o_sb >= 0 && o_sh >= 0 && o_sn >= D,
               "%s: negative stride, or output rows that overlap", r.fn);
    AE_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0 && ((uintptr_t)v & 15) == 0 && ((uintptr_t)out & 7) == 0 &&
                   (!r.extra_align || ((uintptr_t)extra & (r.extra_align - 1)) == 0),
               "%s: %s", r.fn, r.align_text);
    AE_REQUIRE(scale > 0.f, "%s: scale must be positive", r.fn);
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.o = (bf16_t*)out; a.extra = extra;
    a.H = H; a.N = N;
    a.q_sb = q_sb; a.q_sh = q_sh; a.q_sn = q_sn; a.k_sb = k_sb; a.k_sh = k_sh; a.k_sn = k_sn;
    a.v_sb = v_sb; a.v_sh = v_sh; a.v_sn = v_sn; a.o_sb = o_sb; a.o_sh = o_sh; a.o_sn = o_sn;
    a.scale = scale;
    return AE_OK;
}

}  // namespace
