// GroundingDINO's neck and its grounded-box filter for gfx950: what stands between the Swin stages and the transformer
// (GroundingDINO/groundingdino/models/GroundingDINO/groundingdino.py:287-316, backbone/backbone.py:108-114, backbone/position_encoding.py:98-131,
// transformer.py:226-246 + get_valid_ratio) and behind the heads (AnyEdit_Collection/adaptive_editing_pipelines/tools/tool.py:125-133).  The 1x1 and
// stride-2 projections of input_proj run on ae_gemm_bf16 / ae_conv3x3_bf16 as they are; this file adds
//
//   ae_gdino_level_geometry   every level's padding mask (nearest resize of the image mask), sine position embedding (+ level_embed) and valid
//                             ratios of a batch, written straight into the flattened [B, N, ...] layout the transformer reads.  One launch.
//   ae_gdino_neck_groupnorm   GroupNorm(32, 256) of one level's fp32 projection, stored as bf16 rows inside the concatenated src_flatten buffer.
//   ae_gdino_ground           per image: the queries whose best token probability exceeds box_threshold, compacted in query order, with score, box and
//                             the bit set of tokens above text_threshold.
//
// No atomics and no reduction whose order depends on timing: two launches on the same inputs are bit-identical.  Divisions are IEEE; powf / sinf /
// cosf / expf are the library's.
//
// Level geometry: one 256-thread workgroup per (sample, level row).  The level mask is mask_l[y][x] = mask[floor(y H / h)][floor(x W / w)] in
// integers (F.interpolate's "nearest" for every size a backbone makes).  The mask is arbitrary, so both embeddings are true prefix counts: thread x
// walks its column (h reads) for y_embed and its total, the row is scanned in 256-wide pieces with a carry for x_embed.  The two normalised values
// of a piece's tokens go through LDS; then 64 lanes share a token (4 channels = one 8-byte store each, 512 contiguous bytes per wave) and
// evaluate two sin / cos pairs.  At 800 x 800 a sample is 188 workgroups and 13 294 x 128 sin / cos pairs; the kernel is far from any roof and
// is written for launch count, not for bandwidth.
//
// GroupNorm: a 64-row chunk of a sample is one workgroup; a wave reads a row as 64 x 16 bytes, so a lane pair holds one group of 8 channels.  The
// first kernel keeps its chunk in registers and stores the chunk's (mean, sum of centred squares) per group: a two-pass statistic of the chunk.
// The second combines the chunks of its sample in a fixed order, mean = sum n_c mean_c / n and M2 = sum (M2_c + n_c (mean_c - mean)^2) — every
// term non-negative, no cancellation, the accuracy of a two-pass sum — and normalises its own chunk.  The partials are a caller-supplied workspace.
#include "common.hpp"
#include <math.h>

namespace {

__device__ __forceinline__ int wsum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// inclusive scan inside a wave
__device__ __forceinline__ int wscan_i(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// ------------------------------------------------------------------------------------------------------------------ level geometry
constexpr int LG_LMAX = 8;

struct GeometryArgs {
    const uint8_t* mask;                    // [B, H, W], non-zero = padding; may be null
    const float* level_embed;               // [L, 256]; may be null
    uint8_t* mask_out;                      // [B, N]
    bf16_t* pos;                            // [B, N, 256]
    float* valid_ratios;                    // [B, L, 2]
    int H, W, N, L;
    float tH, tW;
    int h[LG_LMAX], w[LG_LMAX], start[LG_LMAX], row0[LG_LMAX];
};

__global__ __launch_bounds__(256) void level_geometry_kernel(const GeometryArgs p) {
    __shared__ float sDim[128];             // [0, 64): temperatureH ** (2 k / 128), [64, 128): temperatureW ** ...   (position_encoding.py:113-118)
    __shared__ float sYe[256], sXe[256];
    __shared__ int sPart[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, row = blockIdx.x;
    int l = 0;                              // block-uniform
    for (int j = 1; j < p.L; ++j)
        if (row >= p.row0[j]) l = j;
    const int h = p.h[l], w = p.w[l], start = p.start[l], y = row - p.row0[l];
    const uint8_t* m = p.mask ? p.mask + (long)b * p.H * p.W : nullptr;
    const long sy = (long)y * p.H / h;

    if (tid < 128) sDim[tid] = powf(tid < 64 ? p.tH : p.tW, (float)(tid & 63) / 64.0f);

    int cnt = 0;
    for (int x = tid; x < w; x += 256) cnt += (m && m[sy * p.W + (long)x * p.W / w]) ? 0 : 1;
    cnt = wsum_i(cnt);
    if (lane == 0) sPart[0][wave] = cnt;
    __syncthreads();
    const int row_total = sPart[0][0] + sPart[0][1] + sPart[0][2] + sPart[0][3];

    const long tok0 = (long)b * p.N + start + (long)y * w;
    int carry = 0;
    for (int x0 = 0; x0 < w; x0 += 256) {   // block-uniform
        const int x = x0 + tid;
        const bool valid = x < w;
        const long sx = valid ? (long)x * p.W / w : 0;
        const int nm = (valid && !(m && m[sy * p.W + sx])) ? 1 : 0;
        int ycnt = 0, ytot = 0;
        if (valid) {
            for (int yy = 0; yy < h; ++yy) {
                const int v = (m && m[((long)yy * p.H / h) * p.W + sx]) ? 0 : 1;
                ytot += v;
                ycnt += yy <= y ? v : 0;
            }
        }
        const int incl = wscan_i(nm, lane);
        if (lane == 63) sPart[1][wave] = incl;
        __syncthreads();
        int before = carry, piece = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = sPart[1][k];
            before += k < wave ? t : 0;
            piece += t;
        }
        carry += piece;
        if (valid) {
            sYe[tid] = (float)ycnt / ((float)ytot + 1e-6f) * 6.283185307179586f;             // position_encoding.py:110
            sXe[tid] = (float)(before + incl) / ((float)row_total + 1e-6f) * 6.283185307179586f;
            p.mask_out[tok0 + x] = nm ? 0 : 1;
            if (y == 0 && x == 0) {                                                           // Transformer.get_valid_ratio
                float* vr = p.valid_ratios + ((long)b * p.L + l) * 2;
                vr[0] = (float)row_total / (float)w;
                vr[1] = (float)ytot / (float)h;
            }
        }
        __syncthreads();
        const int ntok = min(256, w - x0);
        const int part = lane >> 5, pr = (lane & 31) * 2;                                     // channels 4 lane .. 4 lane + 3 = pairs pr, pr + 1 of the y | x half
        const float d0 = sDim[part * 64 + pr], d1 = sDim[part * 64 + pr + 1];
        f32x4 le = {0.f, 0.f, 0.f, 0.f};
        if (p.level_embed) le = *reinterpret_cast<const f32x4*>(p.level_embed + l * 256 + lane * 4);
        for (int t = wave; t < ntok; t += 4) {
            const float e = part ? sXe[t] : sYe[t];
            const float a0 = e / d0, a1 = e / d1;
            u32x2 o;
            o[0] = pack_bf16x2(sinf(a0) + le[0], cosf(a0) + le[1]);
            o[1] = pack_bf16x2(sinf(a1) + le[2], cosf(a1) + le[3]);
            *reinterpret_cast<u32x2*>(p.pos + (tok0 + x0 + t) * 256 + lane * 4) = o;
        }
        __syncthreads();                    // sYe / sXe / sPart[1] are rewritten by the next piece
    }
}

// ------------------------------------------------------------------------------------------------------------------ neck GroupNorm
constexpr int GN_C = 256;
constexpr int GN_GROUPS = 32;
constexpr int GN_ROWS = 64;                 // rows of a chunk
constexpr int GN_RPW = GN_ROWS / 4;         // rows per wave

// sums the four waves' values of group g: the caller has written its lane-pair sum to s[wave][g]
__device__ __forceinline__ float gn_block_sum(const float (*s)[GN_GROUPS], int g) { return ((s[0][g] + s[1][g]) + s[2][g]) + s[3][g]; }

__global__ __launch_bounds__(256) void neck_gn_stats_kernel(const float* __restrict__ x, long ldx, float* __restrict__ part, int hw, int nchunk) {
    __shared__ float sS[4][GN_GROUPS], sQ[4][GN_GROUPS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 1;
    const int b = blockIdx.y, c = blockIdx.x;
    const int r0 = c * GN_ROWS, nrows = min(GN_ROWS, hw - r0);
    const float* xb = x + ((long)b * hw + r0) * ldx + lane * 4;
    f32x4 v[GN_RPW];
#pragma unroll
    for (int i = 0; i < GN_RPW; ++i) {
        const int r = wave + 4 * i;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        v[i] = r < nrows ? *reinterpret_cast<const f32x4*>(xb + (long)r * ldx) : z;
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < GN_RPW; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    s += __shfl_xor(s, 1, 64);
    if ((lane & 1) == 0) sS[wave][g] = s;
    __syncthreads();
    const float mean = gn_block_sum(sS, g) / (float)(nrows * 8);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < GN_RPW; ++i) {
        if (wave + 4 * i < nrows) {
            const float d0 = v[i][0] - mean, d1 = v[i][1] - mean, d2 = v[i][2] - mean, d3 = v[i][3] - mean;
            q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
    }
    q += __shfl_xor(q, 1, 64);
    if ((lane & 1) == 0) sQ[wave][g] = q;
    __syncthreads();
    if (tid < GN_GROUPS) {
        float* o = part + (((long)b * nchunk + c) * GN_GROUPS + tid) * 2;
        o[0] = gn_block_sum(sS, tid) / (float)(nrows * 8);
        o[1] = gn_block_sum(sQ, tid);
    }
}

__global__ __launch_bounds__(256) void neck_gn_apply_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ part, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, bf16_t* __restrict__ out, long out_bs, long row_off, int hw,
                                                            int nchunk) {
    __shared__ float sAcc[8][GN_GROUPS];
    __shared__ float sMean[GN_GROUPS], sRstd[GN_GROUPS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, c = blockIdx.x;
    const float* pb = part + (long)b * nchunk * GN_GROUPS * 2;
    const float n_all = (float)hw * 8.0f;
    {   // the sample's statistics from its chunks, in an order that no workgroup's timing changes: slice k takes chunks k, k + 8, ..; slices are added 0 .. 7
        const int g = tid & 31, k = tid >> 5;
        float a = 0.f;
        for (int j = k; j < nchunk; j += 8) a += (float)(min(GN_ROWS, hw - j * GN_ROWS) * 8) * pb[((long)j * GN_GROUPS + g) * 2];
        sAcc[k][g] = a;
        __syncthreads();
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) t += sAcc[i][g];
        const float mean = t / n_all;
        __syncthreads();                    // sAcc has been read
        a = 0.f;
        for (int j = k; j < nchunk; j += 8) {
            const float* pj = pb + ((long)j * GN_GROUPS + g) * 2;
            const float d = pj[0] - mean;
            a += pj[1] + (float)(min(GN_ROWS, hw - j * GN_ROWS) * 8) * (d * d);
        }
        sAcc[k][g] = a;
        __syncthreads();
        if (tid < GN_GROUPS) {
            t = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) t += sAcc[i][g];
            sMean[g] = mean;
            sRstd[g] = 1.0f / sqrtf(t / n_all + eps);
        }
        __syncthreads();
    }
    const int g = lane >> 1;
    const float mean = sMean[g], rstd = sRstd[g];
    const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + lane * 4), be = *reinterpret_cast<const f32x4*>(beta + lane * 4);
    const int r0 = c * GN_ROWS, nrows = min(GN_ROWS, hw - r0);
    const float* xb = x + ((long)b * hw + r0) * ldx + lane * 4;
    bf16_t* ob = out + (long)b * out_bs + (row_off + r0) * GN_C + lane * 4;
#pragma unroll 4
    for (int i = 0; i < GN_RPW; ++i) {
        const int r = wave + 4 * i;
        if (r >= nrows) break;
        const f32x4 v = *reinterpret_cast<const f32x4*>(xb + (long)r * ldx);
        u32x2 o;
        o[0] = pack_bf16x2(__builtin_fmaf((v[0] - mean) * rstd, ga[0], be[0]), __builtin_fmaf((v[1] - mean) * rstd, ga[1], be[1]));
        o[1] = pack_bf16x2(__builtin_fmaf((v[2] - mean) * rstd, ga[2], be[2]), __builtin_fmaf((v[3] - mean) * rstd, ga[3], be[3]));
        *reinterpret_cast<u32x2*>(ob + (long)r * GN_C) = o;
    }
}

// ------------------------------------------------------------------------------------------------------------------ grounding filter
constexpr int GR_THREADS = 1024;
constexpr int GR_WAVES = GR_THREADS / 64;
constexpr int GR_NQMAX = 1024;
constexpr int GR_TMAX = 256;
constexpr int GR_WMAX = GR_TMAX / 32;

// one workgroup per image.  A wave owns a query row at a time: 64 tokens per step, the text bits are the wave's ballot.  Then thread q holds query q:
// a block-wide exclusive scan of the keep flags is the row's slot, so the kept rows leave in query order (tool.py:131-133 keeps it).  Rows from
// `count` on are written too (index -1, zeros): the outputs are a function of the inputs alone.
__global__ __launch_bounds__(GR_THREADS) void ground_kernel(const float* __restrict__ logits, const float* __restrict__ boxes, float box_thr, float text_thr,
                                                            int* __restrict__ count, int* __restrict__ idx, float* __restrict__ scores, float* __restrict__ out_boxes,
                                                            uint32_t* __restrict__ bits, int nq, int T) {
    __shared__ float sScore[GR_NQMAX];
    __shared__ uint32_t sBits[GR_NQMAX * GR_WMAX];
    __shared__ int sTot[GR_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, words = T >> 5;
    const float* lg = logits + (long)b * nq * T;
    for (int q = wave; q < nq; q += GR_WAVES) {           // wave-uniform
        const float* row = lg + (long)q * T;
        float mx = 0.f;                                    // a sigmoid is never below 0
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int t = t0 + lane;
            const bool in = t < T;
            const float s = in ? 1.0f / (1.0f + expf(-row[t])) : 0.f;   // -inf -> 0
            mx = fmaxf(mx, s);
            const unsigned long long bal = __ballot(in && s > text_thr);
            if (lane == 0) {
                sBits[q * GR_WMAX + (t0 >> 5)] = (uint32_t)bal;
                if ((t0 >> 5) + 1 < words) sBits[q * GR_WMAX + (t0 >> 5) + 1] = (uint32_t)(bal >> 32);
            }
        }
        mx = wave_reduce_max(mx);
        if (lane == 0) sScore[q] = mx;
    }
    __syncthreads();
    const bool mine = tid < nq;
    const float sc = mine ? sScore[tid] : 0.f;
    const int keep = (mine && sc > box_thr) ? 1 : 0;
    const int incl = wscan_i(keep, lane);
    if (lane == 63) sTot[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < GR_WAVES; ++k) {
        const int t = sTot[k];
        before += k < wave ? t : 0;
        total += t;
    }
    if (tid == 0) count[b] = total;
    const long ob = (long)b * nq;
    if (keep) {
        const long o = ob + before + incl - 1;
        idx[o] = tid;
        scores[o] = sc;
        *reinterpret_cast<f32x4*>(out_boxes + o * 4) = *reinterpret_cast<const f32x4*>(boxes + (ob + tid) * 4);
        for (int k = 0; k < words; ++k) bits[o * words + k] = sBits[tid * GR_WMAX + k];
    }
    if (mine && tid >= total) {                            // the unused tail: rows total .. nq - 1, one per thread
        const long o = ob + tid;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        idx[o] = -1;
        scores[o] = 0.f;
        *reinterpret_cast<f32x4*>(out_boxes + o * 4) = z;
        for (int k = 0; k < words; ++k) bits[o * words + k] = 0u;
    }
}

}  // namespace

extern "C" int ae_gdino_level_geometry(const void* mask, int B, int H, int W, const int* shapes_hw, const int* level_start, int L, float temperatureH,
                                       float temperatureW, const float* level_embed, void* mask_flatten, void* pos_flatten, float* valid_ratios, int N,
                                       void* stream) {
    AE_REQUIRE(shapes_hw && level_start && mask_flatten && pos_flatten && valid_ratios, "ae_gdino_level_geometry: null pointer");
    AE_REQUIRE(L >= 1 && L <= LG_LMAX, "ae_gdino_level_geometry: %d levels outside [1, %d]", L, LG_LMAX);
    AE_REQUIRE(B >= 1 && B <= 65535 && N >= 1, "ae_gdino_level_geometry: bad sizes B=%d N=%d (B at most 65535)", B, N);
    AE_REQUIRE(H >= 1 && W >= 1 && (long)H * W < (1L << 31), "ae_gdino_level_geometry: image mask of (%d, %d)", H, W);
    AE_REQUIRE(temperatureH > 0.f && temperatureW > 0.f, "ae_gdino_level_geometry: temperatures must be positive");
    AE_REQUIRE(((uintptr_t)pos_flatten & 7) == 0 && ((uintptr_t)level_embed & 15) == 0, "ae_gdino_level_geometry: pos_flatten must be 8-byte, level_embed 16-byte aligned");
    GeometryArgs a{};
    long cur = 0, rows = 0;
    for (int l = 0; l < L; ++l) {
        const int h = shapes_hw[2 * l], w = shapes_hw[2 * l + 1];
        AE_REQUIRE(h >= 1 && w >= 1 && (long)h * w < (1L << 31), "ae_gdino_level_geometry: level %d has shape (%d, %d)", l, h, w);
        AE_REQUIRE(level_start[l] == cur, "ae_gdino_level_geometry: level %d starts at %d, the shapes before it say %ld", l, level_start[l], cur);
        a.h[l] = h; a.w[l] = w; a.start[l] = (int)cur; a.row0[l] = (int)rows;
        cur += (long)h * w;
        rows += h;
        AE_REQUIRE(cur <= N, "ae_gdino_level_geometry: the levels hold more than N=%d tokens", N);
    }
    AE_REQUIRE(cur == N, "ae_gdino_level_geometry: the levels hold %ld tokens, N=%d", cur, N);
    AE_REQUIRE(rows < (1L << 31), "ae_gdino_level_geometry: %ld level rows", rows);
    a.mask = (const uint8_t*)mask; a.level_embed = level_embed; a.mask_out = (uint8_t*)mask_flatten; a.pos = (bf16_t*)pos_flatten; a.valid_ratios = valid_ratios;
    a.H = H; a.W = W; a.N = N; a.L = L; a.tH = temperatureH; a.tW = temperatureW;
    hipLaunchKernelGGL(level_geometry_kernel, dim3((unsigned)rows, (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    return ae_check_launch("ae_gdino_level_geometry");
}

extern "C" long ae_gdino_neck_groupnorm_workspace_floats(int B, int hw) {
    if (B < 1 || hw < 1) return 0;
    return (long)B * ((hw + GN_ROWS - 1) / GN_ROWS) * GN_GROUPS * 2;
}

extern "C" int ae_gdino_neck_groupnorm(const float* x, long ldx, const float* gamma, const float* beta, float eps, void* out, long out_batch_stride,
                                       long out_row_offset, int B, int hw, float* workspace, void* stream) {
    AE_REQUIRE(x && gamma && beta && out && workspace, "ae_gdino_neck_groupnorm: null pointer");
    AE_REQUIRE(B >= 1 && B <= 65535 && hw >= 1 && (long)B * hw < (1L << 31), "ae_gdino_neck_groupnorm: bad sizes B=%d hw=%d (B at most 65535)", B, hw);
    AE_REQUIRE(ldx >= GN_C && ldx % 4 == 0, "ae_gdino_neck_groupnorm: rows are %d wide; stride %ld must be >= that and a multiple of 4", GN_C, ldx);
    AE_REQUIRE(out_row_offset >= 0 && out_batch_stride >= (out_row_offset + hw) * GN_C && out_batch_stride % 4 == 0,
               "ae_gdino_neck_groupnorm: a sample's %d rows at row %ld do not fit a batch stride of %ld elements", hw, out_row_offset, out_batch_stride);
    AE_REQUIRE((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0 && ((uintptr_t)out & 7) == 0,
               "ae_gdino_neck_groupnorm: x, gamma and beta must be 16-byte aligned, out 8-byte aligned");
    AE_REQUIRE(eps > 0.f, "ae_gdino_neck_groupnorm: eps must be positive");
    const int nchunk = (hw + GN_ROWS - 1) / GN_ROWS;
    const dim3 grid((unsigned)nchunk, (unsigned)B);
    hipLaunchKernelGGL(neck_gn_stats_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, workspace, hw, nchunk);
    hipLaunchKernelGGL(neck_gn_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, (const float*)workspace, gamma, beta, eps, (bf16_t*)out,
                       out_batch_stride, out_row_offset, hw, nchunk);
    return ae_check_launch("ae_gdino_neck_groupnorm");
}

extern "C" int ae_gdino_ground(const float* pred_logits, const float* pred_boxes, float box_threshold, float text_threshold, int* count, int* indices,
                               float* scores, float* boxes, void* token_bits, int B, int nq, int T, void* stream) {
    AE_REQUIRE(pred_logits && pred_boxes && count && indices && scores && boxes && token_bits, "ae_gdino_ground: null pointer");
    AE_REQUIRE(B >= 1 && nq >= 1 && nq <= GR_NQMAX, "ae_gdino_ground: bad sizes B=%d nq=%d (nq at most %d)", B, nq, GR_NQMAX);
    AE_REQUIRE(T >= 32 && T <= GR_TMAX && T % 32 == 0, "ae_gdino_ground: T=%d must be a multiple of 32 in [32, %d]", T, GR_TMAX);
    AE_REQUIRE((((uintptr_t)pred_boxes | (uintptr_t)boxes) & 15) == 0, "ae_gdino_ground: the box tensors must be 16-byte aligned");
    hipLaunchKernelGGL(ground_kernel, dim3((unsigned)B), dim3(GR_THREADS), 0, (hipStream_t)stream, pred_logits, pred_boxes, box_threshold, text_threshold, count,
                       indices, scores, boxes, (uint32_t*)token_bits, nq, T);
    return ae_check_launch("ae_gdino_ground");
}
