// MasaCtrl (mutual self-attention control) kernels for gfx950 (MI355X).
//
// Replaces (AnyEdit_Collection/other_modules/masactrl/masactrl.py):
//   :41-72    MutualSelfAttentionControl.attn_batch / forward      sample b's queries read K / V of sample src[b];
//   :138-193  MutualSelfAttentionControlMask.attn_batch / forward  foreground / background logits (sim + finfo.min), two
//             softmaxes over the same source keys and the blend by the target mask: ONE class-matched softmax per row;
//   :231-334  MutualSelfAttentionControlMaskAuto                   the same with masks taken from cross-attention maps:
//             :277-280 the stored head-mean probabilities (ae_attn_token_map_bf16), :260-271 aggregate_cross_attn_map,
//             :300-303 / :312-323 resize and binarisation (ae_masactrl_classes).
// The reference hook receives sim and attn ([B h, N, N]) of every attention call; none of them is formed here.
//
// ae_attn_mutual_bf16: the streaming 64-key-tile design of attention.hip's general kernel with the same tile constants (AttnTile, attn_tile.hpp) and
// V^T placement (attn_layout.hpp); the kernel body is this file's own twin of attn_kernel's, kept equal to it bit for bit by tests/test_hip_masactrl.py: 4 waves x 2 query fragments, 64-key tiles through LDS, S^T = K Q^T with
// v_mfma_f32_16x16x32_bf16, fp32 online softmax in the exp2 domain, bf16 P as the B operand of O^T = V^T P^T.  The class
// bytes of a key tile ride through LDS beside K.  A disallowed logit is the finite -1e30; while a row has seen no allowed
// key its running maximum stays -1e30 and the exponent offset is taken as 0, so its probabilities are exactly 0 (no NaN, no
// exp2(0) = 1 for masked keys).  A row whose class has no key in its source (class count 0) has every logit replaced by 0:
// the plain mean of V over all keys, what sim + finfo.min gives in fp32.  No atomics: a second call is bit-identical.
#include "attn_tile.hpp"
#include <stdlib.h>
#include <type_traits>

namespace {

constexpr int MAX_B = 64;  // samples per launch (the remap / token sets travel by value)

struct MutualArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o;
    int B, H, N;
    long q_sb, q_sh, q_sn, k_sb, k_sh, k_sn, v_sb, v_sh, v_sn, o_sb, o_sh, o_sn;
    float scale;
    const uint8_t* qcls;  // [B, N] or null
    const uint8_t* kcls;  // [B, N], row src[b]
    const int* kcnt;      // [B, 2], row src[b]
    int src[MAX_B];
};

template <int D, int QF, bool DBUF, bool HAS_CLS>
__global__ __launch_bounds__(256, (D <= 96 ? 2 : 1)) void attn_mutual_kernel(const MutualArgs p) {
    using T = AttnTile<D, QF, 4, DBUF>;
    constexpr bool TAIL16 = T::TAIL16, ONES = T::ONES;
    constexpr int NW = 4, NT = T::NT, NC = T::NC, DQK = T::DQK, DV = T::DV, NDF = T::NDF, DCH = T::DCH, KROW = T::KROW, VROW = T::VROW, KCH = T::KCH, VCH = T::VCH,
                  NBUF = T::NBUF, KSZ = T::KSZ, VSZ = T::VSZ;

    __shared__ __attribute__((aligned(16))) bf16_t smem[NBUF * (KSZ + VSZ)];
    __shared__ __attribute__((aligned(16))) uint8_t sKc[NBUF * KT];
    bf16_t* const sK = smem;
    bf16_t* const sVt = smem + NBUF * KSZ;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    constexpr int QB = T::QB;
    const int N = p.N;
    const int nqb = (N + QB - 1) / QB;
    const int vb = xcd_remap(blockIdx.x, nqb * p.B * p.H);
    const int bh = vb / nqb, qb = vb % nqb;
    const int b = bh / p.H, h = bh % p.H;
    const int bs = p.src[b];
    const int q0 = qb * QB + wave * 16 * QF;

    const bf16_t* qp = p.q + (long)b * p.q_sb + (long)h * p.q_sh;
    const bf16_t* kp = p.k + (long)bs * p.k_sb + (long)h * p.k_sh;
    const bf16_t* vp = p.v + (long)bs * p.v_sb + (long)h * p.v_sh;
    const uint8_t* kc_row = HAS_CLS ? p.kcls + (long)bs * N : nullptr;

    if (DQK > D) {
        for (int i = tid; i < NBUF * KT * (DQK - D); i += NT) sK[(i / (DQK - D)) * KROW + D + i % (DQK - D)] = 0;
    }
    if (DV > D) {
        for (int i = tid; i < NBUF * (DV - D) * VROW; i += NT) {
            const int bufi = i / ((DV - D) * VROW), r = i % ((DV - D) * VROW);
            sVt[bufi * VSZ + D * VROW + r] = (ONES && r < VROW) ? (bf16_t)0x3F80 : (bf16_t)0;
        }
    }

    // ---- Q fragments: lane (q = l15, g) holds Q[q][32c + 8g .. +8]; rows clamped, pad zeroed
    bf16x8_t qf[QF][NC > 0 ? NC : 1];
    s16x4_t qt[QF];
    int qce[QF];     // class this row asks of its keys; 255 = any
    float c2a[QF];   // scale * log2(e), or 0 for a row whose class is empty in its source (all logits equal -> mean of V)
    const float c2 = p.scale * LOG2E;
#pragma unroll
    for (int a = 0; a < QF; ++a) {
        const int qrow = min(q0 + a * 16 + l15, N - 1);
#pragma unroll
        for (int c = 0; c < NC; ++c)
            qf[a][c] = as_bf16x8(*reinterpret_cast<const u32x4*>(qp + (long)qrow * p.q_sn + c * 32 + lg * 8));
        if (TAIL16) {
            const int d = NC * 32 + lg * 4;
            const u32x2 t = *reinterpret_cast<const u32x2*>(qp + (long)qrow * p.q_sn + (d < D ? d : 0));
            qt[a] = as_s16x4(d < D ? t : (u32x2){0u, 0u});
        }
        qce[a] = 255;
        c2a[a] = c2;
        if (HAS_CLS) {
            const int qc = p.qcls[(long)b * N + qrow];
            if (qc != 255) {
                const bool empty = qc > 1 || p.kcnt[bs * 2 + (qc & 1)] == 0;
                qce[a] = empty ? 255 : qc;
                c2a[a] = empty ? 0.f : c2;
            }
        }
    }

    f32x4 o[QF][NDF];
    float m_run[QF], l_run[QF];
#pragma unroll
    for (int a = 0; a < QF; ++a) {
        m_run[a] = NEG_BIG;
        l_run[a] = 0.f;
#pragma unroll
        for (int df = 0; df < NDF; ++df) o[a][df] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    auto row_sum = [&](int a) -> float {
        if (ONES) {
            const float v = o[a][D / 16][D % 4];
            return __shfl(v, l15 + 16 * ((D % 16) / 4), 64);
        }
        float l = l_run[a];
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        return l;
    };

    // ---- staging: per-thread (row, chunk) assignments are loop invariant
    int k_key[KCH], k_c[KCH], v_pr[VCH], v_c[VCH];
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
        const int id = min(tid + i * NT, KT * DCH - 1);
        k_key[i] = id / DCH;
        k_c[i] = id - k_key[i] * DCH;
    }
#pragma unroll
    for (int i = 0; i < VCH; ++i) {
        const int id = min(tid + i * NT, (KT / 2) * DCH - 1);
        v_pr[i] = id / DCH;
        v_c[i] = id - v_pr[i] * DCH;
    }
    u32x4 rk[KCH], rv[VCH][2];
    uint8_t rc = 0;
    const int last_key = N - 1;
    // bounds-checked buffer loads with 32-bit byte offsets: keys >= N fall past the extent and read as 0 (their P is forced to 0)
    const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(kp), 0, (int)(((long)last_key * p.k_sn + D) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(vp), 0, (int)(((long)last_key * p.v_sn + D) * 2), 0x00020000);
    int k_off[KCH], v_off[VCH];
#pragma unroll
    for (int i = 0; i < KCH; ++i) k_off[i] = (int)((long)k_key[i] * p.k_sn + k_c[i] * 8) * 2;
#pragma unroll
    for (int i = 0; i < VCH; ++i) v_off[i] = (int)((long)(2 * v_pr[i]) * p.v_sn + v_c[i] * 8) * 2;
    const int k_tile_bytes = (int)(KT * p.k_sn * 2), v_tile_bytes = (int)(KT * p.v_sn * 2), v_row_bytes = (int)(p.v_sn * 2);
    auto load_kv = [&](int k0) {
        const int tk = (k0 / KT) * k_tile_bytes, tv = (k0 / KT) * v_tile_bytes;
#pragma unroll
        for (int i = 0; i < KCH; ++i) rk[i] = __builtin_amdgcn_raw_buffer_load_b128(rsK, k_off[i] + tk, 0, 0);
#pragma unroll
        for (int i = 0; i < VCH; ++i) {
            rv[i][0] = __builtin_amdgcn_raw_buffer_load_b128(rsV, v_off[i] + tv, 0, 0);
            rv[i][1] = __builtin_amdgcn_raw_buffer_load_b128(rsV, v_off[i] + tv + v_row_bytes, 0, 0);
        }
        if (HAS_CLS) {
            if (tid < KT) rc = kc_row[min(k0 + tid, last_key)];
        }
    };
    auto store_kv = [&](int buf) {
        bf16_t* dK = sK + buf * KSZ;
        bf16_t* dV = sVt + buf * VSZ;
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            if (KT * DCH % NT == 0 || tid + i * NT < KT * DCH)
                *reinterpret_cast<u32x4*>(dK + k_key[i] * KROW + k_c[i] * 8) = rk[i];
        }
#pragma unroll
        for (int i = 0; i < VCH; ++i) {
            if ((KT / 2) * DCH % NT == 0 || tid + i * NT < (KT / 2) * DCH) {
                store_vt_pair(dV, VROW, v_c[i], vt_pos(2 * v_pr[i]), rv[i][0], rv[i][1]);
            }
        }
        if (HAS_CLS) {
            if (tid < KT) sKc[buf * KT + tid] = rc;
        }
    };

    const int ntiles = (N + KT - 1) / KT;
    load_kv(0);
    __syncthreads();
    store_kv(0);
    __syncthreads();

    auto tile_body = [&](int k0, int cur, auto tail_tag) {
        constexpr bool TAIL = decltype(tail_tag)::value;
        const bf16_t* cK = sK + cur * KSZ;
        const bf16_t* cV = sVt + cur * VSZ;
        uint32_t kw[4] = {0u, 0u, 0u, 0u};  // class bytes of this lane's keys 16 f + 4 lg + r
        if (HAS_CLS) {
#pragma unroll
            for (int f = 0; f < 4; ++f) kw[f] = *reinterpret_cast<const uint32_t*>(sKc + cur * KT + f * 16 + lg * 4);
        }

        f32x4 s[QF][4];
        // the K = 16 remainder first, for all key fragments, then the K = 32 chain (a 16x16x16 and a 16x16x32 MFMA close together
        // on one accumulator lose updates on gfx950: attention.hip keeps them apart the same way)
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            if (TAIL16) {
                const s16x4_t kt = as_s16x4(*reinterpret_cast<const u32x2*>(cK + (f * 16 + l15) * KROW + NC * 32 + lg * 4));
#pragma unroll
                for (int a = 0; a < QF; ++a)
                    s[a][f] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(kt, qt[a], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            } else {
#pragma unroll
                for (int a = 0; a < QF; ++a) s[a][f] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
        if (TAIL16) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const bf16x8_t kf = as_bf16x8(*reinterpret_cast<const u32x4*>(cK + (f * 16 + l15) * KROW + c * 32 + lg * 8));
#pragma unroll
                for (int a = 0; a < QF; ++a) s[a][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[a][c], s[a][f], 0, 0, 0);
            }
        }

        bf16x8_t pb[QF][2];
#pragma unroll
        for (int a = 0; a < QF; ++a) {
            constexpr bool PLAIN = !HAS_CLS && !TAIL;
            if (!PLAIN) {
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    const int kb = k0 + f * 16 + lg * 4;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = s[a][f][r] * c2a[a];
                        if (HAS_CLS) {
                            const int kc = (int)((kw[f] >> (8 * r)) & 0xffu);
                            if (qce[a] != 255 && kc != qce[a]) v = NEG_BIG;
                        }
                        if (TAIL) {
                            if (kb + r >= N) v = NEG_BIG;
                        }
                        s[a][f][r] = v;
                    }
                }
            }
            float mx = NEG_BIG;
#pragma unroll
            for (int f = 0; f < 4; ++f) mx = fmaxf(mx, fmaxf(fmaxf(s[a][f][0], s[a][f][1]), fmaxf(s[a][f][2], s[a][f][3])));
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            if (PLAIN) mx *= c2;  // scale > 0
            if (__any(mx > m_run[a])) {
                const float m_new = fmaxf(m_run[a], mx);
                const float alpha = __builtin_amdgcn_exp2f(m_run[a] - m_new);
                m_run[a] = m_new;
                l_run[a] *= alpha;
#pragma unroll
                for (int df = 0; df < NDF; ++df) {
                    o[a][df][0] *= alpha; o[a][df][1] *= alpha; o[a][df][2] *= alpha; o[a][df][3] *= alpha;
                }
            }
            // no allowed key so far: offset 0, so that every (disallowed, -1e30) logit of this tile exponentiates to exactly 0
            const float neg_m = (HAS_CLS && m_run[a] <= NEG_BIG) ? 0.f : -m_run[a];
#pragma unroll
            for (int f = 0; f < 4; ++f)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float e = PLAIN ? __builtin_amdgcn_exp2f(fmaf(s[a][f][r], c2, neg_m)) : __builtin_amdgcn_exp2f(s[a][f][r] + neg_m);
                    if (TAIL) {
                        if (k0 + f * 16 + lg * 4 + r >= N) e = 0.f;
                    }
                    s[a][f][r] = e;
                }
            if (!ONES) {
                float rs = 0.f;
#pragma unroll
                for (int f = 0; f < 4; ++f) rs += (s[a][f][0] + s[a][f][1]) + (s[a][f][2] + s[a][f][3]);
                l_run[a] += rs;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                u32x4 w;
                w.x = pack_bf16x2(s[a][2 * j][0], s[a][2 * j][1]);
                w.y = pack_bf16x2(s[a][2 * j][2], s[a][2 * j][3]);
                w.z = pack_bf16x2(s[a][2 * j + 1][0], s[a][2 * j + 1][1]);
                w.w = pack_bf16x2(s[a][2 * j + 1][2], s[a][2 * j + 1][3]);
                pb[a][j] = as_bf16x8(w);
            }
        }

#pragma unroll
        for (int df = 0; df < NDF; ++df) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const bf16x8_t vf = as_bf16x8(*reinterpret_cast<const u32x4*>(cV + (df * 16 + l15) * VROW + lg * 16 + j * 8));
#pragma unroll
                for (int a = 0; a < QF; ++a) o[a][df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pb[a][j], o[a][df], 0, 0, 0);
            }
        }
    };

    for (int t = 0; t < ntiles; ++t) {
        const int k0 = t * KT;
        const int cur = DBUF ? (t & 1) : 0;
        if (t + 1 < ntiles) load_kv(k0 + KT);
        if (k0 + KT > N) tile_body(k0, cur, std::true_type{});
        else tile_body(k0, cur, std::false_type{});
        if (DBUF) {
            if (t + 1 < ntiles) store_kv(cur ^ 1);
            __syncthreads();
        } else {
            __syncthreads();
            if (t + 1 < ntiles) {
                store_kv(0);
                __syncthreads();
            }
        }
    }

    bf16_t* op = p.o + (long)b * p.o_sb + (long)h * p.o_sh;
#pragma unroll
    for (int a = 0; a < QF; ++a) {
        const float rsum = row_sum(a);
        const float inv = rsum > 0.f ? 1.0f / rsum : 0.f;  // (class counts that contradict kcls: zeros, not NaN)
        const int qrow = q0 + a * 16 + l15;
        if (qrow >= N) continue;
#pragma unroll
        for (int df = 0; df < NDF; ++df) {
            const int d = df * 16 + lg * 4;
            if (d < D) {
                const float r0 = o[a][df][0] * inv, r1 = o[a][df][1] * inv, r2 = o[a][df][2] * inv, r3 = o[a][df][3] * inv;
                *reinterpret_cast<u32x2*>(op + (long)qrow * p.o_sn + d) = (u32x2){pack_bf16x2(r0, r1), pack_bf16x2(r2, r3)};
            }
        }
    }
}

template <int D, int QF, bool DBUF>
int launch_mutual(const MutualArgs& a, hipStream_t stream) {
    constexpr int QB = AttnTile<D, QF, 4, DBUF>::QB;
    const long blocks = (long)((a.N + QB - 1) / QB) * a.B * a.H;
    dim3 grid((unsigned)blocks), block(256);
    if (a.qcls) hipLaunchKernelGGL((attn_mutual_kernel<D, QF, DBUF, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((attn_mutual_kernel<D, QF, DBUF, false>), grid, block, 0, stream, a);
    return ae_check_launch("ae_attn_mutual_bf16");
}

// ------------------------------------------------------------------------------------------------ token map
struct TokArgs {
    const bf16_t* q; const bf16_t* k; float* out;
    int B, H, N, Nk, D;
    long q_sb, q_sh, q_sn, k_sb, k_sh, k_sn;
    float c2;      // scale * log2(e)
    float inv_h;
    int accumulate;
    unsigned long long set[2 * MAX_B];  // 128-bit token set of each sample: bit j of word j / 64
};

constexpr int TM_QW = 1;         // query rows per wave: the launch is a chain of dependent reductions, so it wants blocks, not reuse (8 rows per
                                 // wave: 32 blocks and 156 us at 256 queries x 77 keys x 8 heads of 160)
constexpr int TM_QB = 4 * TM_QW; // per block
constexpr int TM_MAXD = 160, TM_MAXK = 128;

// One wave per query row, lane l owns keys l and l + 64; the keys of one (sample, head) sit in LDS; heads are visited in order and
// their terms added in that order in one register: no atomics, the same bits on every call.
__global__ __launch_bounds__(256) void token_map_kernel(const TokArgs p) {
    constexpr int KROW = TM_MAXD + 8;
    __shared__ __attribute__((aligned(16))) bf16_t sK[TM_MAXK * KROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * TM_QB + wave * TM_QW;
    const int dch = p.D / 8;
    const unsigned long long w0 = p.set[2 * b], w1 = p.set[2 * b + 1];
    const bool in0 = lane < p.Nk, in1 = lane + 64 < p.Nk;
    const bool sel0 = in0 && ((w0 >> lane) & 1ull), sel1 = in1 && ((w1 >> lane) & 1ull);
    float acc[TM_QW];
#pragma unroll
    for (int i = 0; i < TM_QW; ++i) acc[i] = 0.f;

    for (int h = 0; h < p.H; ++h) {
        const bf16_t* kp = p.k + (long)b * p.k_sb + (long)h * p.k_sh;
        __syncthreads();  // every wave is done with the previous head's keys
        for (int i = tid; i < p.Nk * dch; i += 256) {
            const int row = i / dch, c = i - row * dch;
            *reinterpret_cast<u32x4*>(sK + row * KROW + c * 8) = *reinterpret_cast<const u32x4*>(kp + (long)row * p.k_sn + c * 8);
        }
        __syncthreads();
        const bf16_t* qp = p.q + (long)b * p.q_sb + (long)h * p.q_sh;
        const bf16_t* k0p = sK + min(lane, p.Nk - 1) * KROW;
        const bf16_t* k1p = sK + min(lane + 64, p.Nk - 1) * KROW;
#pragma unroll
        for (int qi = 0; qi < TM_QW; ++qi) {
            const int row = min(q0 + qi, p.N - 1);  // clamped: rows past N are computed and not stored
            const bf16_t* qr = qp + (long)row * p.q_sn;
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
            const float t0 = in0 ? s0 * p.c2 : NEG_BIG, t1 = in1 ? s1 * p.c2 : NEG_BIG;
            const float m = wave_reduce_max(fmaxf(t0, t1));   // lane 0 is always a real key
            const float e0 = in0 ? __builtin_amdgcn_exp2f(t0 - m) : 0.f, e1 = in1 ? __builtin_amdgcn_exp2f(t1 - m) : 0.f;
            const float den = wave_reduce_sum(e0 + e1);
            const float num = wave_reduce_sum((sel0 ? e0 : 0.f) + (sel1 ? e1 : 0.f));
            acc[qi] += num / den;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int qi = 0; qi < TM_QW; ++qi) {
            const int row = q0 + qi;
            if (row < p.N) {
                float* dst = p.out + (long)b * p.N + row;
                const float v = acc[qi] * p.inv_h;
                *dst = p.accumulate ? *dst + v : v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ classes
constexpr int MAX_PAIRS = 8;
struct ClsArgs {
    const float* maps; long map_ld;
    int S, R;
    float thres;
    uint8_t* cls; int* counts;
    int sample[MAX_PAIRS], orow[MAX_PAIRS];
};

__global__ __launch_bounds__(256) void masactrl_classes_kernel(const ClsArgs p) {
    __shared__ float s_mn[4], s_mx[4];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pr = blockIdx.x;
    const float* x = p.maps + (long)p.sample[pr] * p.map_ld;
    const int n = p.S * p.S;
    float mn = x[0], mx = x[0];
    for (int i = tid; i < n; i += 256) {
        const float v = x[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    mn = -wave_reduce_max(-mn);
    mx = wave_reduce_max(mx);
    if (lane == 0) { s_mn[wave] = mn; s_mx[wave] = mx; }
    __syncthreads();
    mn = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
    mx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    const float range = mx - mn;
    const float sc = (float)p.S / (float)p.R;   // F.interpolate(mode="nearest") without scale_factor: src = min(floor(dst * in / out), in - 1)
    const int rr = p.R * p.R;
    uint8_t* dst = p.cls + (long)p.orow[pr] * rr;
    int ones = 0;
    for (int i = tid; i < rr; i += 256) {
        const int oy = i / p.R, ox = i - oy * p.R;
        const int sy = min((int)floorf((float)oy * sc), p.S - 1), sx = min((int)floorf((float)ox * sc), p.S - 1);
        const float v = (x[sy * p.S + sx] - mn) / range;   // IEEE division, as the reference's fp32 tensor division
        const int c = (range > 0.f && v >= p.thres) ? 1 : 0;
        dst[i] = (uint8_t)c;
        ones += c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ones += __shfl_xor(ones, o, 64);
    if (lane == 0) s_cnt[wave] = ones;
    __syncthreads();
    if (tid == 0) {
        const int t = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        p.counts[p.orow[pr] * 2] = rr - t;
        p.counts[p.orow[pr] * 2 + 1] = t;
    }
}

}  // namespace

extern "C" int ae_attn_mutual_bf16(const void* q, const void* k, const void* v, void* out, int B, int H, int N, int D,
                                   long q_sb, long q_sh, long q_sn, long k_sb, long k_sh, long k_sn,
                                   long v_sb, long v_sh, long v_sn, long o_sb, long o_sh, long o_sn, float scale,
                                   const int* src, const unsigned char* qcls, const unsigned char* kcls, const int* kcnt, void* stream) {
    AE_REQUIRE(q && k && v && out && src, "ae_attn_mutual_bf16: null pointer");
    AE_REQUIRE(B > 0 && H > 0 && N > 0, "ae_attn_mutual_bf16: bad sizes B=%d H=%d N=%d", B, H, N);
    AE_REQUIRE(scale > 0.f, "ae_attn_mutual_bf16: scale must be positive");
    AE_REQUIRE((q_sb | q_sh | q_sn | k_sb | k_sh | k_sn | v_sb | v_sh | v_sn) % 8 == 0 && (o_sb | o_sh | o_sn) % 4 == 0,
               "ae_attn_mutual_bf16: strides must keep rows 16-byte aligned");
    AE_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0 && ((uintptr_t)v & 15) == 0 && ((uintptr_t)out & 7) == 0,
               "ae_attn_mutual_bf16: pointers must be 16-byte aligned");
    AE_REQUIRE(qcls == nullptr || (kcls && kcnt), "ae_attn_mutual_bf16: qcls needs kcls and the class counts");
    if (B > MAX_B) {
        ae_set_error("ae_attn_mutual_bf16: B=%d exceeds the %d samples one launch remaps", B, MAX_B);
        return AE_ERR_UNSUPPORTED;
    }
    MutualArgs a{};
    for (int b = 0; b < B; ++b) {
        AE_REQUIRE(src[b] >= 0 && src[b] < B, "ae_attn_mutual_bf16: src[%d]=%d outside [0, %d)", b, src[b], B);
        a.src[b] = src[b];
    }
    const long kv_lim = 1L << 31;
    if (((long)(N - 1) * k_sn + D) * 2 >= kv_lim || ((long)(N - 1) * v_sn + D) * 2 >= kv_lim) {
        ae_set_error("ae_attn_mutual_bf16: the K / V image of one (batch, head) spans 2^31 bytes or more (N=%d k_sn=%ld v_sn=%ld)", N, k_sn, v_sn);
        return AE_ERR_UNSUPPORTED;
    }
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.o = (bf16_t*)out;
    a.B = B; a.H = H; a.N = N;
    a.q_sb = q_sb; a.q_sh = q_sh; a.q_sn = q_sn; a.k_sb = k_sb; a.k_sh = k_sh; a.k_sn = k_sn;
    a.v_sb = v_sb; a.v_sh = v_sh; a.v_sn = v_sn; a.o_sb = o_sb; a.o_sh = o_sh; a.o_sn = o_sn;
    a.scale = scale; a.qcls = qcls; a.kcls = kcls; a.kcnt = kcnt;
    hipStream_t s = (hipStream_t)stream;
    switch (D) {
        case 40: return launch_mutual<40, 2, true>(a, s);
        case 64: return launch_mutual<64, 2, true>(a, s);
        case 80: return launch_mutual<80, 2, true>(a, s);
        case 160: return launch_mutual<160, 2, false>(a, s);
        default:
            ae_set_error("ae_attn_mutual_bf16: unsupported head_dim %d (supported: 40, 64, 80, 160)", D);
            return AE_ERR_UNSUPPORTED;
    }
}

extern "C" int ae_attn_token_map_bf16(const void* q, const void* k, float* out, int B, int H, int N, int Nk, int D,
                                      long q_sb, long q_sh, long q_sn, long k_sb, long k_sh, long k_sn, float scale,
                                      const unsigned long long* token_sets, int accumulate, void* stream) {
    AE_REQUIRE(q && k && out && token_sets, "ae_attn_token_map_bf16: null pointer");
    AE_REQUIRE(B > 0 && H > 0 && N > 0 && Nk > 0, "ae_attn_token_map_bf16: bad sizes B=%d H=%d N=%d Nk=%d", B, H, N, Nk);
    AE_REQUIRE((q_sb | q_sh | q_sn | k_sb | k_sh | k_sn) % 8 == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)k & 15) == 0,
               "ae_attn_token_map_bf16: q / k rows must be 16-byte aligned");
    if (Nk > TM_MAXK || D % 8 != 0 || D <= 0 || D > TM_MAXD || B > MAX_B) {
        ae_set_error("ae_attn_token_map_bf16: unsupported Nk=%d (<= %d), head_dim %d (multiple of 8, <= %d) or B=%d (<= %d)", Nk, TM_MAXK, D, TM_MAXD,
                     B, MAX_B);
        return AE_ERR_UNSUPPORTED;
    }
    TokArgs a{};
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.out = out;
    a.B = B; a.H = H; a.N = N; a.Nk = Nk; a.D = D;
    a.q_sb = q_sb; a.q_sh = q_sh; a.q_sn = q_sn; a.k_sb = k_sb; a.k_sh = k_sh; a.k_sn = k_sn;
    a.c2 = scale * LOG2E; a.inv_h = 1.0f / (float)H; a.accumulate = accumulate;
    for (int i = 0; i < 2 * B; ++i) a.set[i] = token_sets[i];
    dim3 grid((unsigned)((N + TM_QB - 1) / TM_QB), (unsigned)B), block(256);
    hipLaunchKernelGGL(token_map_kernel, grid, block, 0, (hipStream_t)stream, a);
    return ae_check_launch("ae_attn_token_map_bf16");
}

extern "C" int ae_masactrl_classes(const float* maps, long map_ld, int S, int R, float thres, int npairs, const int* sample, const int* out_row,
                                   unsigned char* cls, int* counts, void* stream) {
    AE_REQUIRE(maps && sample && out_row && cls && counts, "ae_masactrl_classes: null pointer");
    AE_REQUIRE(S > 0 && R > 0 && S <= 4096 && R <= 4096 && map_ld >= (long)S * S, "ae_masactrl_classes: bad sizes S=%d R=%d map_ld=%ld", S, R, map_ld);
    AE_REQUIRE(npairs > 0 && npairs <= MAX_PAIRS, "ae_masactrl_classes: 1 to %d (sample, output) pairs per launch, got %d", MAX_PAIRS, npairs);
    ClsArgs a{};
    a.maps = maps; a.map_ld = map_ld; a.S = S; a.R = R; a.thres = thres; a.cls = cls; a.counts = counts;
    for (int i = 0; i < npairs; ++i) {
        AE_REQUIRE(sample[i] >= 0 && out_row[i] >= 0, "ae_masactrl_classes: negative index in pair %d", i);
        a.sample[i] = sample[i];
        a.orow[i] = out_row[i];
    }
    hipLaunchKernelGGL(masactrl_classes_kernel, dim3((unsigned)npairs), dim3(256), 0, (hipStream_t)stream, a);
    return ae_check_launch("ae_masactrl_classes");
}
