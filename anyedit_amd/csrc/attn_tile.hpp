// The constants of the streaming 64-key-tile attention design, derived once: attn_kernel (attention.hip) and attn_mutual_kernel (masactrl.hip) take every
// tile constant and LDS size from AttnTile<D, QF, NW, DBUF>; LOG2E, NEG_BIG, vt_pos and store_vt_pair come from attn_layout.hpp.
//
// The design: NW waves per block, each owns QF 16-row query fragments and keeps Q in registers as MFMA operands.  K / V are streamed in 64-key tiles
// through LDS (double-buffered when it fits), logits are computed TRANSPOSED, S^T = K Q^T, so a lane holds the 16 logits of keys 16 f + 4 g + r of ONE
// query row per tile, and the exponentiated registers, rounded to bf16, are the B operand of O^T = V^T P^T.  head_dim is padded inside the kernel
// (40 -> 48 for QK^T through one K = 16 MFMA, 48 for PV).
//
// The two kernel bodies are NOT shared.  Every body piece tried as a shared forceinline helper (pad fill, Q loads, K / V stager, QK^T tile, online-softmax
// step, PV tile, store, the tile loop's barrier protocol) kept the arithmetic but changed the generated code of some instantiation, and some of those
// measured slower than the separate kernels, one with other output bits (profiles/attn_tile_refactor_ab.txt).  What is here compiles
// to the same instructions as the separate definitions did.
#pragma once
#include "attn_layout.hpp"

namespace {

constexpr int KT = 64;  // keys per tile

template <int D_, int QF_, int NW_, bool DBUF_>
struct AttnTile {
    static_assert(D_ % 8 == 0, "head_dim must be a multiple of 8");
    static_assert(D_ % 32 == 0 || D_ % 32 == 8 || D_ % 32 == 16, "head_dim % 32 must be 0, 8 or 16");
    static constexpr int D = D_, QF = QF_, NW = NW_;
    static constexpr bool DBUF = DBUF_;
    static constexpr int NT = 64 * NW;              // threads per block
    static constexpr int QB = NW * 16 * QF;         // query rows per block
    static constexpr int NC = D / 32;               // full K=32 MFMAs per (key frag, q frag)
    static constexpr bool TAIL16 = (D % 32) != 0;   // head-dim remainder (8 or 16) goes through ONE K=16 MFMA instead of padding to 32
    static constexpr int DQK = NC * 32 + (TAIL16 ? 16 : 0);
    static constexpr int DV = (D + 15) / 16 * 16;
    static constexpr bool ONES = DV > D;  // a free padding row of V^T holds 1.0: the PV MFMA then also produces sum_k P[q][k] (the softmax
                                          // denominator, rescaled together with O) and the 32 VALU adds per tile disappear
    static constexpr int NDF = DV / 16;   // 16-row fragments of O^T
    static constexpr int DCH = D / 8;     // 16-byte chunks per K/V row
    static constexpr int KROW = DQK + 8;  // LDS row strides (elements), +16 B pad
    static constexpr int VROW = KT + 8;
    static constexpr int KCH = (KT * DCH + NT - 1) / NT;
    static constexpr int VCH = ((KT / 2) * DCH + NT - 1) / NT;
    static constexpr int NBUF = DBUF ? 2 : 1;
    static constexpr int KSZ = KT * KROW, VSZ = DV * VROW;
    static constexpr int SMEM = NBUF * (KSZ + VSZ);  // bf16 elements: sK = smem, sVt = smem + NBUF * KSZ
};

}  // namespace
