"""Route cases and the route ledger of gemm_conv.hip / attention_fast.hip (CASES, LEDGER: tools/route_check.py), of norm.hip (NORM_CASES,
NORM_LEDGER: tools/norm_route_check.py), of gemm_rowpanel.hip / ff_fused.hip (ROWPANEL_CASES, ROWPANEL_LEDGER:
tools/rowpanel_route_check.py) and of attention.hip (ATTN_GENERAL_CASES, ATTN_GENERAL_LEDGER: tools/attn_general_route_check.py; the
template-argument order and the case options stand above the cases), shared with tests/test_kernel_routes.py.

CASES: one dict per GPU case (op + shape + options); tools/route_check.py builds the seeded operands, runs the op through `ops`, records the
kernels it launched and checks the output element by element (see that script's docstring for the bound).

LEDGER / NORM_LEDGER: one row per kernel instantiation of the three files in the default build, keyed by the template-argument tuple as c++filt prints it
(`gemm_kernel<192, 320, 1, 2, 4, true, 1, 2, false, 0, 4, 0>`: BM, BN, AMODE (0 dense, 1 conv), WAVES_M, WAVES_N, GLDS, WAVES_K, STAGES,
CS, LAB, WA, XE; `attn_fast_kernel<D, OCC, SEG2, ABL, BIAS, QG, VSPLIT, SKV, NWV, SKT>`; `attn_pipe_kernel<D, KT, PV16>`).  Each row is
  ("default", [case ids])   reached with no AE_* variable set, by every case listed.
ATTN_GENERAL_LEDGER alone also has rows of the form
  ("env", {"AE_ATTN_FAST": "0", ...}, [case ids])   reached by every case listed in a process with every AE_* variable removed and exactly
                                                    those set: the variants that only a tuning knob of attention.hip selects.
The default build compiles nothing that no case reaches: every instantiation is a `default` row, or an `env` row whose environment the
test starts a child process for; what no environment reaches is not compiled.
"""

# --------------------------------------------------------------------------------------------------- cases
# conv: B, H, W, Cin, Cout; stride, ups (0 / 1 nearest / 2 zero-insert), cs (column statistics), k (k_order; None = ops.conv_k_order),
#       res / addvec / f32 epilogue options
# up2:  conv3x3_up2 (nearest x2 + conv as four 2x2 convs)
# gemm: M, N, K; epi ("none" / "geglu" / "gelu"), a2 (Ksplit of the two-source form), cpad (output columns past N: ldc > N), bias, res, f32,
#       cs (column statistics), rs (row statistics, gemm(rowstats=))
# ln:   gemm_ln (LayerNorm folded into the GEMM): M, N, K, epi
# attn: B, H, Nq, Nk, D; lay ("qkv": fused [B*N, 3*H*D] rows for self-attention, q rows + packed kv rows for cross-attention; "bhnd"),
#       nk2 (second segment), rel (kH, kW: SAM rel-pos bias)


def _conv(id, B, H, W, Cin, Cout, **kw):
    return dict(id=id, op="conv", B=B, H=H, W=W, Cin=Cin, Cout=Cout, **kw)


def _gemm(id, M, N, K, **kw):
    return dict(id=id, op="gemm", M=M, N=N, K=K, **kw)


def _attn(id, B, H, Nq, Nk, D, **kw):
    return dict(id=id, op="attn", B=B, H=H, Nq=Nq, Nk=Nk, D=D, **kw)


CASES = [
    # ---- conv, un-split 192x320 (fill >= 0.85 of whole CU rounds)
    _conv("c320_slab_b11", 11, 64, 64, 320, 320),                         # M % 192 = 128, slab form (chunk-major K)
    _conv("c320_slab_cs_b11", 11, 64, 64, 320, 320, cs=True, res=True),   # + column statistics epilogue + residual
    _conv("c320_slab_b10_w64", 10, 70, 64, 320, 320),                     # M % 192 = 64
    _conv("c320_slab_m32_w16", 17, 154, 16, 320, 320, cs=True),           # M % 192 = 32, width 16
    _conv("c320_slab_w48", 21, 48, 48, 320, 320),                         # width 48
    _conv("c320_slab_w96", 8, 64, 96, 320, 320),                          # width 96 (64x96 latent at batch 8)
    _conv("c320_slab_w192", 2, 128, 192, 320, 320, addvec=True),          # width 192 = the tile: one image row per tile
    _conv("c320_wrap_w64h2", 384, 2, 64, 320, 320),                       # short map: 192 / W == H + 1 (a tile runs into the next sample)
    _conv("c320_wrap_w16h11", 279, 11, 16, 320, 320, cs=True),
    _conv("c320_wrap_w96h1", 511, 1, 96, 320, 320),
    _conv("c320_tap_w40", 12, 96, 40, 320, 320),                          # width 40: tiles start mid-row (tap form)
    _conv("c320_tap_w56_cs", 10, 84, 56, 320, 320, cs=True),              # width 56, tap form + statistics
    _conv("c320_tap_k0", 11, 64, 64, 320, 320, k=0),                      # tap-major K order on the slab's shape
    _conv("c320_tap_k0_cs", 11, 64, 64, 320, 320, k=0, cs=True),
    _conv("c320_s2", 11, 128, 128, 320, 320, stride=2),                   # stride 2 (tap form; 64x64 output maps, M % 192 = 128)
    _conv("c320_ups", 11, 32, 32, 320, 320, ups=1),                       # nearest x2 gather: the plain loop
    _conv("c320_ups_cs", 11, 32, 32, 320, 320, ups=1, cs=True),
    _conv("c320_ups_zero", 11, 32, 32, 320, 320, ups=2),                  # zero-insert x2 (the adjoint of a stride-2 conv)
    _conv("c128_ups_zero", 3, 16, 24, 640, 1280, ups=2),                 # zero-insert x2 on the 128x128 tile
    _conv("c64_ups_zero", 2, 5, 7, 64, 128, ups=2),
    # ---- conv, split-K on the 192x320 tile (product geometries: UNet batch 3 / 6 per edited image)
    _conv("cs_64x96_b3_l2_640", 3, 32, 48, 640, 640),                     # 512x768: split 5, slab, width 48
    _conv("cs_64x96_b3_l2_320", 3, 32, 48, 320, 640),                     # split 2, tap form (ragged K range)
    _conv("cs_64x96_b3_l2_1280", 3, 32, 48, 1280, 640),                   # decoder skip concat
    _conv("cs_64x96_b3_l2_960", 3, 32, 48, 960, 640),
    _conv("cs_64x96_b6_l3_1280", 6, 16, 24, 1280, 1280),
    _conv("cs_64x96_b6_l3_2560", 6, 16, 24, 2560, 1280),
    _conv("cs_96x64_b3_l2_640", 3, 48, 32, 640, 640),                     # 768x512: width 32
    _conv("cs_96x64_b6_l3_1280", 6, 24, 16, 1280, 1280),
    _conv("cs_64x80_b3_l2_640", 3, 32, 40, 640, 640),                     # 512x640: width 40, tap form
    _conv("cs_64x80_b6_l3_1280", 6, 16, 20, 1280, 1280),                  # split 6: K ranges start mid-tap
    _conv("cs_64x80_b6_l3_1280_k0", 6, 16, 20, 1280, 1280, k=0),          # tap-major: a tap is 20 K tiles, a range 30
    _conv("cs_64x80_b6_l3_1920", 6, 16, 20, 1920, 1280),
    _conv("cs_64x80_b6_l3_640", 6, 16, 20, 640, 1280),
    _conv("cs_48x64_b3_l2_640", 3, 24, 32, 640, 640),
    _conv("cs_48x64_b6_l3_1280", 6, 12, 16, 1280, 1280),
    _conv("cs_48x64_b6_l3_2560", 6, 12, 16, 2560, 1280, cs=True),         # + stand-alone column statistics behind the reduce
    _conv("cs_f7", 3, 32, 34, 1280, 640),                                 # split 7, width 34, ragged last K range
    _conv("cs_f8", 6, 16, 16, 1280, 1280),                                # split 8, ragged last K range
    _conv("cs_f3", 5, 32, 48, 1280, 640),                                 # split 3
    _conv("cs_f5_ups", 6, 8, 12, 1280, 1280, ups=1),                      # split 5 under the nearest x2 gather: the plain loop
    _conv("cs_f4_slab", 5, 36, 32, 1280, 640),                            # split 4, slab form
    _conv("cs_f4_tap", 5, 32, 36, 640, 640),                              # split 4, tap form, width 36
    _conv("cs_s2_f2", 12, 64, 64, 320, 320, stride=2),                    # stride 2, split 2 (the 64x64 -> 32x32 downsampler at UNet batch 12)
    _conv("cs_s2_f5", 12, 32, 48, 640, 640, stride=2),                    # stride 2, split 5 (32x48 -> 16x24)
    # ---- conv, everything else
    _conv("c128_splitk", 2, 8, 8, 1280, 1280),                            # 128x128 split-K + splitk_reduce_kernel
    _conv("c128_splitk_cs", 3, 8, 12, 1280, 1280, cs=True),               # + colstats_kernel
    _conv("c128_splitk_rs", 2, 9, 9, 1224, 1280),                         # register-staged loader (Cin % 64 != 0), split-K
    _conv("c128_wa", 3, 32, 48, 640, 1280),                               # 128x128 weights-ahead
    _conv("c128_wa_cs", 3, 40, 41, 640, 1280, cs=True, res=True),         # + statistics epilogue, ragged M
    _conv("c128_rs", 5, 40, 40, 96, 640, addvec=True),                    # 128x128 register-staged (Cin 96)
    _conv("c160", 3, 64, 96, 320, 320),                                   # 128x160 (64x96 latent, batch 3)
    _conv("c160_rs", 3, 64, 95, 96, 320),                                 # 128x160 register-staged
    _conv("c64x128_tile", 3, 64, 80, 320, 320, f32=True),                 # 128x64 (64x80 latent, batch 3), fp32 output
    _conv("c64x128_rs", 3, 64, 79, 200, 320),
    _conv("c64", 2, 10, 13, 64, 100),                                     # 64x64 tile, ragged M and N
    _conv("c64_rs", 1, 9, 7, 40, 36),
    _conv("c64_s2", 2, 17, 15, 128, 256, stride=2),
    dict(id="up2_192", op="up2", B=20, H=24, W=24, Cin=320, Cout=320, cs=False),
    dict(id="up2_192_cs", op="up2", B=20, H=24, W=24, Cin=320, Cout=320, cs=True),
    dict(id="up2_128", op="up2", B=3, H=16, W=24, Cin=640, Cout=640, cs=False),
    dict(id="up2_128_cs", op="up2", B=3, H=16, W=24, Cin=640, Cout=640, cs=True),
    # ---- dense GEMM
    _gemm("g320_pp", 24500, 640, 640, bias=True, res=True, cpad=16),      # 192x320 2x4 ping-pong, ragged last tile, ldc > N
    _gemm("g320_pp_a2", 49000, 320, 1280, a2=640, cpad=8),                # + the two-source form
    _gemm("g320_geglu", 24500, 1280, 640, epi="geglu", bias=True, cpad=8),  # GEGLU 4x2
    dict(id="g320_ln_geglu", op="ln", M=24500, N=1280, K=640, epi="geglu"),   # LayerNorm fold XE = 2 on the GEGLU tile
    dict(id="g320_ln_xetail", op="ln", M=3060, N=3840, K=1280, epi="none"),   # the xe_tail rule (qkv of the 16x16 level)
    _gemm("g128_ring", 3000, 1280, 1280, bias=True, cpad=8),              # 128x128 three-stage ring (XE 0)
    _gemm("g128_ring_rs", 3000, 1280, 1280, rs=True),                     # ring, XE 1 (row statistics)
    dict(id="g128_ring_ln", op="ln", M=3000, N=1280, K=1280, epi="none"),     # ring, XE 2 (LayerNorm fold)
    _gemm("g192x128_ring", 4000, 1280, 2560, res=True, cpad=8),           # 192x128 three-stage ring
    _gemm("g64_ring", 700, 256, 1280, cpad=8),                            # 64x64 three-stage ring
    _gemm("g64_ring_a2", 700, 256, 1344, a2=640),
    _gemm("g128_wa", 4000, 1024, 640, bias=True, cpad=8),                 # 128x128 weights-ahead
    _gemm("g128_wa_a2", 4000, 1024, 640, a2=320, epi="gelu"),
    _gemm("g128_wa_rs", 4000, 1024, 640, rs=True),
    dict(id="g128_wa_ln", op="ln", M=4000, N=1024, K=640, epi="none"),
    _gemm("g128_wa_cs", 4000, 1024, 640, cs=True),
    _gemm("g128_wa_f32", 4000, 1024, 640, f32=True),
    _gemm("g128_short", 4000, 1024, 128),                                 # kt < 3: the two-stage kernel
    _gemm("g128_rs", 4000, 1024, 648, cpad=8),                            # K % 64 != 0: register-staged loader
    _gemm("g128x64", 3800, 576, 512, cpad=8),                             # 128x64 (4x2 waves)
    _gemm("g128x64_rs", 3800, 576, 520),
    _gemm("g64", 300, 260, 512, cpad=4),                                  # 64x64
    _gemm("g64_rs", 300, 260, 520),
    # ---- attention (fused-qkv rows / packed kv rows; every default row has a case whose last 128-query block is ragged, Nq % 128 != 0 —
    #      test_ledger_rows_are_well_formed checks it; product shapes with whole blocks are extra cases)
    _attn("a40_pipe64", 4, 8, 4032, 4032, 40, lay="qkv"),                 # 4032 = 63 x 64 keys: 64-key tiles
    _attn("a40_pipe128", 4, 8, 3968, 3968, 40, lay="qkv"),                # 3968 = 31 x 128 keys: 128-key tiles
    _attn("a40_pipe128_nq4000", 4, 8, 4000, 4096, 40, lay="qkv"),         # 128-key tiles, ragged last query block (q rows + kv rows)
    _attn("a40_pipe_6144", 3, 8, 6144, 6144, 40, lay="qkv"),              # 64x96 latent, B*heads = 24
    _attn("a40_pipe_5120", 6, 8, 5120, 5120, 40, lay="qkv"),              # 64x80 latent, B*heads = 48
    _attn("a40_pipe64_b6", 6, 8, 4032, 4032, 40, lay="qkv"),              # 4032 at B*heads = 48: 64-key tiles
    _attn("a40_4032_b3", 3, 8, 4032, 4032, 40, lay="qkv"),                # 4032 at B*heads = 24: too few 256-query blocks for the pipeline -> VSPLIT
    _attn("a40_qg2", 8, 8, 4000, 4000, 40, lay="qkv"),                    # Nk % 64 != 0: QG = 2
    _attn("a40_vsplit", 1, 8, 1000, 1000, 40, lay="qkv"),                 # small grid: VSPLIT
    _attn("a40_skv", 3, 8, 6144, 77, 40, lay="qkv"),                      # cross-attention, keys resident
    _attn("a40_skv_ng1", 1, 2, 300, 77, 40, lay="qkv"),                   # 1 / 4 / 8 query groups per block
    _attn("a40_skv_ng4", 24, 8, 1536, 77, 40, lay="qkv"),
    _attn("a40_skv_ng8", 18, 8, 4032, 77, 40, lay="qkv"),
    _attn("a40_skv_seg2", 3, 8, 5120, 77, 40, lay="qkv", nk2=1),          # + the second segment (1 key .. the short form's 64)
    _attn("a40_skv_seg2max", 6, 8, 4032, 77, 40, lay="qkv", nk2=64),
    _attn("a40_seg2_long", 1, 8, 1000, 300, 40, lay="qkv", nk2=77),       # second segment, long first segment
    _attn("a80_vsplit", 3, 8, 1536, 1536, 80, lay="qkv"),                 # 32x48 level self-attention
    _attn("a80_vsplit_1280", 6, 8, 1280, 1280, 80, lay="qkv"),
    _attn("a80_vsplit_1500", 3, 8, 1500, 1500, 80, lay="qkv"),            # ragged last query block
    _attn("a80_skv", 3, 8, 1536, 77, 80, lay="qkv"),
    _attn("a80_skv_ng8", 48, 8, 1000, 77, 80, lay="qkv"),
    _attn("a80_skv_seg2", 6, 8, 1280, 77, 80, lay="qkv", nk2=16),
    _attn("a80_skv_seg2_1000", 6, 8, 1000, 77, 80, lay="qkv", nk2=16),
    _attn("a80_seg2_long", 2, 8, 1000, 200, 80, lay="qkv", nk2=77),
    _attn("a80_relwin", 25, 16, 196, 196, 80, lay="bhnd", rel=(14, 14)),  # SAM windows: resident keys
    _attn("a80_relwin240", 4, 16, 240, 240, 80, lay="bhnd", rel=(15, 16)),  # window > 224 queries: tiled look-up bias
    _attn("a80_relglobal", 1, 16, 1024, 1024, 80, lay="bhnd", rel=(16, 64)),  # global attention rows of 64 keys
    _attn("a80_relglobal_1000", 1, 16, 1000, 1024, 80, lay="bhnd", rel=(16, 64)),  # + a ragged last query block
    _attn("a160", 3, 8, 96, 96, 160, lay="qkv"),                          # 8x12 level (64x96 latent): <= 128 keys, resident
    _attn("a160_320", 6, 8, 320, 320, 160, lay="qkv"),                    # 16x20 level
    _attn("a160_48", 3, 8, 48, 48, 160, lay="qkv"),
    _attn("a160_384", 3, 8, 384, 384, 160, lay="qkv"),                    # 16x24 level: > 128 keys, the tiled kernel
    _attn("a160_self80", 6, 8, 80, 80, 160, lay="qkv"),                   # 8x10 level self-attention (64x80 latent), B*heads = 48
    _attn("a160_skv", 6, 8, 80, 77, 160, lay="qkv"),
    _attn("a160_x96", 3, 8, 96, 77, 160, lay="qkv"),                      # 8x12 / 6x8 level cross-attention
    _attn("a160_x48", 6, 8, 48, 77, 160, lay="qkv"),
    _attn("a160_skv_seg2", 3, 8, 384, 77, 160, lay="qkv", nk2=8),
    _attn("a160_skv_seg2_300", 3, 8, 300, 77, 160, lay="qkv", nk2=8),
    _attn("a160_seg2_long", 3, 8, 384, 384, 160, lay="qkv", nk2=77),
    _attn("a160_seg2_long_300", 3, 8, 300, 384, 160, lay="qkv", nk2=77),
]

CASE_IDS = [c["id"] for c in CASES]


# --------------------------------------------------------------------------------------------------- ledger
def _g(*a):
    return "gemm_kernel<" + ", ".join(str(x).lower() for x in a) + ">"


def _af(*a):
    return "attn_fast_kernel<" + ", ".join(str(x).lower() for x in a) + ">"


LEDGER = {
    # dense
    _g(128, 128, 0, 4, 2, False, 1, 2, False, 0, 0, 0): ("default", ["g128_rs"]),
    _g(128, 128, 0, 4, 2, True, 1, 2, False, 0, 0, 0): ("default", ["g128_short"]),
    _g(128, 128, 0, 4, 2, True, 1, 2, False, 0, 1, 0): ("default", ["g128_wa", "g128_wa_a2", "g128_wa_f32"]),
    _g(128, 128, 0, 4, 2, True, 1, 2, False, 0, 1, 1): ("default", ["g128_wa_rs"]),
    _g(128, 128, 0, 4, 2, True, 1, 2, False, 0, 1, 2): ("default", ["g128_wa_ln"]),
    _g(128, 128, 0, 4, 2, True, 1, 2, True, 0, 1, 0): ("default", ["g128_wa_cs"]),
    _g(128, 128, 0, 4, 2, True, 1, 3, False, 0, 0, 0): ("default", ["g128_ring"]),
    _g(128, 128, 0, 4, 2, True, 1, 3, False, 0, 0, 1): ("default", ["g128_ring_rs"]),
    _g(128, 128, 0, 4, 2, True, 1, 3, False, 0, 0, 2): ("default", ["g128_ring_ln"]),
    _g(128, 64, 0, 4, 2, False, 1, 2, False, 0, 0, 0): ("default", ["g128x64_rs"]),
    _g(128, 64, 0, 4, 2, True, 1, 2, False, 0, 0, 0): ("default", ["g128x64"]),
    _g(192, 128, 0, 4, 2, True, 1, 3, False, 0, 0, 0): ("default", ["g192x128_ring"]),
    _g(192, 320, 0, 2, 4, True, 1, 2, False, 0, 3, 0): ("default", ["g320_pp", "g320_pp_a2"]),
    _g(192, 320, 0, 4, 2, True, 1, 2, False, 0, 3, 0): ("default", ["g320_geglu"]),
    _g(192, 320, 0, 4, 2, True, 1, 2, False, 0, 3, 2): ("default", ["g320_ln_geglu", "g320_ln_xetail"]),
    _g(64, 64, 0, 2, 2, False, 1, 2, False, 0, 0, 0): ("default", ["g64_rs"]),
    _g(64, 64, 0, 2, 2, True, 1, 2, False, 0, 0, 0): ("default", ["g64"]),
    _g(64, 64, 0, 2, 2, True, 1, 3, False, 0, 0, 0): ("default", ["g64_ring", "g64_ring_a2"]),
    # conv
    _g(128, 128, 1, 4, 2, False, 1, 2, False, 0, 0, 0): ("default", ["c128_rs", "c128_splitk_rs"]),
    _g(128, 128, 1, 4, 2, True, 1, 2, False, 0, 1, 0): ("default", ["c128_wa", "c128_splitk", "cs_48x64_b3_l2_640", "cs_48x64_b6_l3_1280", "c128_ups_zero", "up2_128"]),
    _g(128, 128, 1, 4, 2, True, 1, 2, True, 0, 1, 0): ("default", ["c128_wa_cs", "up2_128_cs"]),
    _g(128, 160, 1, 2, 2, False, 1, 2, False, 0, 0, 0): ("default", ["c160_rs"]),
    _g(128, 160, 1, 2, 2, True, 1, 2, False, 0, 0, 0): ("default", ["c160"]),
    _g(128, 64, 1, 2, 2, False, 1, 2, False, 0, 0, 0): ("default", ["c64x128_rs"]),
    _g(128, 64, 1, 2, 2, True, 1, 2, False, 0, 0, 0): ("default", ["c64x128_tile"]),
    _g(192, 320, 1, 2, 4, True, 1, 2, False, 0, 0, 0): ("default", ["c320_ups", "c320_ups_zero", "cs_f5_ups"]),
    _g(192, 320, 1, 2, 4, True, 1, 2, False, 0, 3, 0): ("default", ["c320_tap_w40", "c320_tap_k0", "c320_s2", "cs_64x96_b3_l2_320", "cs_64x80_b3_l2_640",
                                                                      "cs_64x80_b6_l3_1280", "cs_64x80_b6_l3_1280_k0", "cs_64x96_b6_l3_1280",
                                                                      "cs_64x96_b6_l3_2560", "cs_64x80_b6_l3_1920", "cs_64x80_b6_l3_640",
                                                                      "cs_f7", "cs_f8", "cs_f3", "cs_f4_tap", "cs_s2_f2", "cs_s2_f5", "up2_192"]),
    _g(192, 320, 1, 2, 4, True, 1, 2, False, 0, 4, 0): ("default", ["c320_slab_b11", "c320_slab_b10_w64", "c320_slab_w48", "c320_slab_w96", "c320_slab_w192",
                                                                      "c320_wrap_w64h2", "c320_wrap_w96h1", "cs_64x96_b3_l2_640", "cs_64x96_b3_l2_1280",
                                                                      "cs_64x96_b3_l2_960", "cs_96x64_b3_l2_640", "cs_96x64_b6_l3_1280", "cs_f4_slab"]),
    _g(192, 320, 1, 2, 4, True, 1, 2, True, 0, 0, 0): ("default", ["c320_ups_cs"]),
    _g(192, 320, 1, 2, 4, True, 1, 2, True, 0, 3, 0): ("default", ["c320_tap_w56_cs", "c320_tap_k0_cs", "up2_192_cs"]),
    _g(192, 320, 1, 2, 4, True, 1, 2, True, 0, 4, 0): ("default", ["c320_slab_cs_b11", "c320_slab_m32_w16", "c320_wrap_w16h11"]),
    _g(64, 64, 1, 2, 2, False, 1, 2, False, 0, 0, 0): ("default", ["c64_rs"]),
    _g(64, 64, 1, 2, 2, True, 1, 2, False, 0, 0, 0): ("default", ["c64", "c64_s2", "c64_ups_zero"]),
    "splitk_reduce_kernel": ("default", ["c128_splitk", "cs_64x96_b3_l2_640", "cs_64x80_b6_l3_1280", "cs_64x96_b6_l3_2560", "cs_64x80_b6_l3_1920",
                                         "cs_64x80_b6_l3_640", "cs_48x64_b6_l3_1280", "cs_f7", "cs_f8", "cs_f3", "cs_f4_slab", "cs_f4_tap",
                                         "cs_f5_ups", "cs_s2_f2", "cs_s2_f5"]),
    "colstats_kernel": ("default", ["c128_splitk_cs", "cs_48x64_b6_l3_2560"]),
    # attention
    _af(160, 1, False, 0, 0, 1, False, True, 4, 3): ("default", ["a160_skv", "a160", "a160_48", "a160_self80", "a160_x96", "a160_x48"]),
    _af(160, 1, True, 0, 0, 1, False, False, 4, 3): ("default", ["a160_seg2_long", "a160_seg2_long_300"]),
    _af(160, 1, True, 0, 0, 1, False, True, 4, 3): ("default", ["a160_skv_seg2", "a160_skv_seg2_300"]),
    _af(160, 2, False, 0, 0, 1, False, False, 4, 3): ("default", ["a160_320", "a160_384"]),
    _af(40, 3, False, 0, 0, 1, False, True, 4, 3): ("default", ["a40_skv", "a40_skv_ng1", "a40_skv_ng4", "a40_skv_ng8"]),
    _af(40, 3, False, 0, 0, 1, True, False, 4, 3): ("default", ["a40_vsplit", "a40_4032_b3"]),
    _af(40, 3, False, 0, 0, 2, True, False, 4, 3): ("default", ["a40_qg2"]),
    _af(40, 3, True, 0, 0, 1, False, False, 4, 3): ("default", ["a40_seg2_long"]),
    _af(40, 3, True, 0, 0, 1, False, True, 4, 3): ("default", ["a40_skv_seg2", "a40_skv_seg2max"]),
    _af(80, 2, False, 0, 0, 1, False, True, 4, 3): ("default", ["a80_skv", "a80_skv_ng8"]),
    _af(80, 2, False, 0, 1, 1, False, False, 4, 3): ("default", ["a80_relwin240"]),
    _af(80, 2, False, 0, 2, 1, False, False, 4, 3): ("default", ["a80_relglobal", "a80_relglobal_1000"]),
    _af(80, 2, False, 0, 3, 1, False, True, 7, 4): ("default", ["a80_relwin"]),
    _af(80, 2, True, 0, 0, 1, False, False, 4, 3): ("default", ["a80_seg2_long"]),
    _af(80, 2, True, 0, 0, 1, False, True, 4, 3): ("default", ["a80_skv_seg2", "a80_skv_seg2_1000"]),
    _af(80, 3, False, 0, 0, 1, True, False, 4, 3): ("default", ["a80_vsplit", "a80_vsplit_1280", "a80_vsplit_1500"]),
    "attn_pipe_kernel<40, 128, false>": ("default", ["a40_pipe128", "a40_pipe128_nq4000", "a40_pipe_6144", "a40_pipe_5120"]),
    "attn_pipe_kernel<40, 64, false>": ("default", ["a40_pipe64", "a40_pipe64_b6"]),
}


# --------------------------------------------------------------------------------------------------- norm.hip: cases
# (tools/norm_route_check.py runs them; tests/norm_ref.py holds the operands, the float64 reference and the bounds)
# gn:    ops.groupnorm: B, HW, C, groups; C1 (channels of the first source of a concat input, 0 = one source), silu, cs (statistics from
#        the producers' per-32-row column sums), stat (ask for (mean, rstd))
# gnb:   ops.groupnorm_bwd: the same, plus saved (the forward's (mean, rstd) are passed in) and acc (bit 0: dx +=, bit 1: dx2 +=)
# ln:    ops.layernorm: M, C; align=False offsets gamma / beta by 4 bytes (the rows kernel wants 16-byte aligned parameters)
# lnb:   ops.layernorm_bwd: M, C, param (parameter gradients), acc
# lnwin: ops.layernorm_window_partition (mode 1) / ops.window_merge_layernorm (mode 2): B, H, W, C, ws
# lnact: ops.layernorm_act: M, C, gelu
def _gn(id, B, HW, C, groups=32, C1=0, silu=False, cs=False, stat=True):
    return dict(id=id, op="gn", B=B, HW=HW, C=C, groups=groups, C1=C1, silu=silu, cs=cs, stat=stat)


def _gnb(id, B, HW, C, groups=32, C1=0, silu=False, saved=True, acc=0):
    return dict(id=id, op="gnb", B=B, HW=HW, C=C, groups=groups, C1=C1, silu=silu, saved=saved, acc=acc)


_LN_ROWS = {320: 8, 640: 16, 1280: 32, 2560: 64}      # C -> L of layernorm_rows_kernel<L, 5> / layernorm_window_kernel<L, 5, mode>
_NARROW = {8: 1, 16: 2, 24: 4, 64: 8, 104: 16, 256: 32, 512: 64}   # C -> L of layernorm_narrow_kernel<L, ACT>

NORM_CASES = [
    # ---- GroupNorm forward, one launch (HW <= 256): gn_slab_kernel<MAXCH, GP, 0>; GP groups per block so that a pack is whole 16-byte
    #      pieces (cpg = C / groups: GP 1 if cpg % 8 == 0, 2 if cpg % 4 == 0, 4 if cpg % 2 == 0); MAXCH from ceil(HW * GP * cpg / 8 / T)
    _gn("gn_s21_hw250", 3, 250, 256),                            # cpg 8: one piece per row, 250 of 256 threads
    _gn("gn_s21_hw1", 2, 1, 256, silu=True),                     # a single row: 8 elements per group
    _gn("gn_s41_hw200", 2, 200, 1280, silu=True),                # 1000 pieces = 3 * 256 + 232: ragged last piece
    _gn("gn_s81_hw256_cat", 2, 256, 1280, C1=648, silu=True),    # the 16x16 level; the concat split falls inside a group
    _gn("gn_s161_g8", 2, 256, 2560, groups=8),                   # cpg 320: 10 pieces per thread at 1024 threads
    _gn("gn_s22_hw64", 3, 64, 640),                              # cpg 20, packs of 2 groups
    _gn("gn_s22_hw9_cat", 3, 9, 640, C1=328, silu=True),         # 3x3 map; C1 = 8 * 40 + 8 inside a pack
    _gn("gn_s42_hw200_cat", 2, 200, 640, C1=328, silu=True),
    _gn("gn_s82_hw256_cat", 2, 256, 1920, C1=1288, silu=True),   # cpg 60; C1 = 10 * 120 + 88 inside a pack
    _gn("gn_s162_g2_cat", 2, 256, 264, groups=2, C1=136),        # cpg 132: one pack of 33 pieces per row
    _gn("gn_s24_hw255", 3, 255, 64),                             # cpg 2: a pack of 4 groups is one piece
    _gn("gn_s24_hw64_cat", 3, 64, 320, C1=168, silu=True),       # cpg 10; C1 = 4 * 40 + 8 inside a pack
    _gn("gn_s44_hw200_cat", 2, 200, 320, C1=168),
    _gn("gn_s84_hw256", 3, 256, 320, silu=True, stat=False),     # the product's 16x16 level at 320 channels, no statistics asked
    _gn("gn_s84_hw256_cat", 2, 256, 960, C1=328, silu=True),     # cpg 30; C1 % 120 != 0
    _gn("gn_s164_cat", 2, 256, 2112, C1=1064),                   # cpg 66: 33 pieces per row and pack
    # ---- GroupNorm forward, three launches (HW > 256, or the slab refused): gn_stats_kernel / gn_finalize_kernel / gn_apply_kernel<false>
    _gn("gn_t_hw257_c320", 3, 257, 320, silu=True),              # 32 rows per chunk: the last chunk has 1 row
    _gn("gn_t_hw1000_c320_cat8", 3, 1000, 320, C1=8),            # last chunk 8 rows; the first source is one piece wide
    _gn("gn_t_hw1000_c960_cat", 2, 1000, 960, C1=952, silu=True),  # 240 threads (not whole waves), 16 rows per chunk; the second source is one piece
    _gn("gn_t_hw257_c64", 3, 257, 64),                           # 8 pieces per row, 32 row slices, one row per thread
    _gn("gn_t_hw300_c64_g1", 3, 300, 64, groups=1),
    _gn("gn_t_hw300_c64_g8", 3, 300, 64, groups=8, silu=True),
    _gn("gn_t_hw260_c4096_g64", 2, 260, 4096, groups=64),        # 512 threads, one row slice, 8 rows per chunk (last: 4)
    _gn("gn_t_hw200_c8192_g8", 2, 200, 8192, groups=8),          # HW <= 256 but 25 pieces per thread: the slab refuses; 1024 threads
    # ---- GroupNorm forward from the producers' column statistics: gn_finalize_cs_kernel + apply
    _gn("gn_cs_hw32_c320", 3, 32, 320, cs=True, silu=True),      # one slab per sample
    _gn("gn_cs_hw288_c640", 3, 288, 640, cs=True),
    _gn("gn_cs_hw1024_c320", 3, 1024, 320, cs=True, silu=True),  # the 32x32 level
    _gn("gn_cs_hw32_c960_cat", 3, 32, 960, C1=640, cs=True),
    _gn("gn_cs_hw288_c640_cat", 3, 288, 640, C1=328, cs=True, silu=True),   # the split falls inside a group
    _gn("gn_cs_hw1024_c1920_cat", 3, 1024, 1920, C1=1288, cs=True, silu=True),
    # ---- GroupNorm backward, one launch (saved statistics, HW <= 256, at most 4 piece pairs per thread): gnb_slab_kernel<MAXCH, GP>
    _gnb("gnb_s21_hw250", 3, 250, 256, silu=True),
    _gnb("gnb_s41_hw200_cat", 2, 200, 1280, C1=648, silu=True, acc=3),
    _gnb("gnb_s41_hw256_c4096", 2, 256, 4096),                   # 4096 pieces = 4 * 1024: the last shape the slab takes
    _gnb("gnb_s22_hw64_cat", 3, 64, 640, C1=328, acc=1),
    _gnb("gnb_s42_hw200_cat", 2, 200, 640, C1=328, silu=True),
    _gnb("gnb_s24_hw64_cat", 3, 64, 320, C1=168, silu=True, acc=2),
    _gnb("gnb_s44_hw256_cat", 2, 256, 960, C1=328, silu=True, acc=3),
    # ---- GroupNorm backward, three launches: gnb_partial_kernel / gnb_finalize_kernel / gnb_apply_kernel
    _gnb("gnb_t_hw256_c4352", 2, 256, 4352),                     # 4352 pieces: 5 per thread, the slab refuses; saved statistics
    _gnb("gnb_t_saved_hw257_c320", 3, 257, 320, silu=True),
    _gnb("gnb_t_saved_hw1000_c960_cat", 2, 1000, 960, C1=8, acc=3),
    _gnb("gnb_t_own_hw257_c320", 3, 257, 320, saved=False, acc=1),             # its own statistics pass (gn_stats + gn_finalize)
    _gnb("gnb_t_own_hw200_c960_cat", 2, 200, 960, C1=952, silu=True, saved=False, acc=2),
    _gnb("gnb_t_own_hw1000_c64_g8", 3, 1000, 64, groups=8, saved=False),
]
# ---- LayerNorm, L lanes per row x 5 pieces (C = 40 L, parameters 16-byte aligned): M % rows-per-block in {1, rpb - 1}
for _C, _L in _LN_ROWS.items():
    _rpb = 4 * 64 // _L
    NORM_CASES += [dict(id=f"ln_r{_L}_m{2 * _rpb + 1}", op="ln", M=2 * _rpb + 1, C=_C, align=True),
                   dict(id=f"ln_r{_L}_m{3 * _rpb - 1}", op="ln", M=3 * _rpb - 1, C=_C, align=True)]
# ---- LayerNorm, one wave per row: layernorm_kernel<1 | 2 | 3 | 8> at both sides of each threshold, and the C = 40 L widths with misaligned parameters
NORM_CASES += [dict(id=f"ln_k_c{_C}_m{_M}", op="ln", M=_M, C=_C, align=True)
               for _C, _M in ((8, 5), (512, 1), (520, 5), (1024, 1), (1032, 5), (1536, 1), (1544, 5), (4096, 5))]
NORM_CASES += [dict(id=f"ln_mis_c{_C}_m{_M}", op="ln", M=_M, C=_C, align=False) for _C, _M in ((320, 5), (640, 5), (1280, 1), (2560, 5))]
# ---- LayerNorm backward: layernorm_bwd_kernel<1 | 2 | 4> (+ layernorm_param_grad_kernel, M <= 4096)
NORM_CASES += [dict(id=f"lnb_c{_C}_m{_M}" + ("_p" if _p else "") + ("_acc" if _a else ""), op="lnb", M=_M, C=_C, param=_p, acc=_a)
               for _C, _M, _p, _a in ((512, 7, True, 0), (512, 4096, True, 0), (520, 1, True, 1), (1024, 7, False, 1), (1032, 7, True, 0),
                                      (1032, 4096, True, 0), (2048, 1, False, 0), (2048, 4096, False, 1))]
# ---- LayerNorm with SAM's window partition: 14x14 windows on 20x27 (padding on both axes) and 28x28 (none)
NORM_CASES += [dict(id=f"lnwin_c{_C}_{_H}x{_W}_mode{_m}", op="lnwin", B=2, H=_H, W=_W, C=_C, ws=14, mode=_m)
               for _C in _LN_ROWS for (_H, _W) in ((20, 27), (28, 28)) for _m in (1, 2)]
# ---- narrow LayerNorm (+ GELU): one C per lane count, M = 301 is no multiple of any block's rows
NORM_CASES += [dict(id=f"lnact_c{_C}" + ("_gelu" if _g else ""), op="lnact", M=301, C=_C, gelu=_g) for _C in _NARROW for _g in (False, True)]

NORM_CASE_IDS = [c["id"] for c in NORM_CASES]


# --------------------------------------------------------------------------------------------------- norm.hip: ledger
def _ids(op, **kw):
    return [c["id"] for c in NORM_CASES if c["op"] == op and all(c[k] == v for k, v in kw.items())]


def _pref(*prefixes):
    return [i for i in NORM_CASE_IDS if i.startswith(prefixes)]


_GN3 = _pref("gn_t_")
_GNB3 = _pref("gnb_t_")
NORM_LEDGER = {
    "gn_slab_kernel<2, 1, 0>": ("default", _pref("gn_s21_")),
    "gn_slab_kernel<4, 1, 0>": ("default", _pref("gn_s41_")),
    "gn_slab_kernel<8, 1, 0>": ("default", _pref("gn_s81_")),
    "gn_slab_kernel<16, 1, 0>": ("default", _pref("gn_s161_")),
    "gn_slab_kernel<2, 2, 0>": ("default", _pref("gn_s22_")),
    "gn_slab_kernel<4, 2, 0>": ("default", _pref("gn_s42_")),
    "gn_slab_kernel<8, 2, 0>": ("default", _pref("gn_s82_")),
    "gn_slab_kernel<16, 2, 0>": ("default", _pref("gn_s162_")),
    "gn_slab_kernel<2, 4, 0>": ("default", _pref("gn_s24_")),
    "gn_slab_kernel<4, 4, 0>": ("default", _pref("gn_s44_")),
    "gn_slab_kernel<8, 4, 0>": ("default", _pref("gn_s84_")),
    "gn_slab_kernel<16, 4, 0>": ("default", _pref("gn_s164_")),
    "gn_stats_kernel": ("default", _GN3 + _pref("gnb_t_own_")),
    "gn_finalize_kernel": ("default", _GN3 + _pref("gnb_t_own_")),
    "gn_finalize_cs_kernel": ("default", _pref("gn_cs_")),
    "gn_apply_kernel<false>": ("default", _GN3 + _pref("gn_cs_")),
    "gnb_slab_kernel<2, 1>": ("default", _pref("gnb_s21_")),
    "gnb_slab_kernel<4, 1>": ("default", _pref("gnb_s41_")),
    "gnb_slab_kernel<2, 2>": ("default", _pref("gnb_s22_")),
    "gnb_slab_kernel<4, 2>": ("default", _pref("gnb_s42_")),
    "gnb_slab_kernel<2, 4>": ("default", _pref("gnb_s24_")),
    "gnb_slab_kernel<4, 4>": ("default", _pref("gnb_s44_")),
    "gnb_partial_kernel": ("default", _GNB3),
    "gnb_finalize_kernel": ("default", _GNB3),
    "gnb_apply_kernel": ("default", _GNB3),
    "layernorm_kernel<1>": ("default", ["ln_k_c8_m5", "ln_k_c512_m1", "ln_mis_c320_m5"]),
    "layernorm_kernel<2>": ("default", ["ln_k_c520_m5", "ln_k_c1024_m1", "ln_mis_c640_m5"]),
    "layernorm_kernel<3>": ("default", ["ln_k_c1032_m5", "ln_k_c1536_m1", "ln_mis_c1280_m1"]),
    "layernorm_kernel<8>": ("default", ["ln_k_c1544_m5", "ln_k_c4096_m5", "ln_mis_c2560_m5"]),
    "layernorm_bwd_kernel<1>": ("default", _ids("lnb", C=512)),
    "layernorm_bwd_kernel<2>": ("default", _ids("lnb", C=520) + _ids("lnb", C=1024)),
    "layernorm_bwd_kernel<4>": ("default", _ids("lnb", C=1032) + _ids("lnb", C=2048)),
    "layernorm_param_grad_kernel": ("default", _ids("lnb", param=True)),
}
for _C, _L in _LN_ROWS.items():
    NORM_LEDGER[f"layernorm_rows_kernel<{_L}, 5>"] = ("default", _pref(f"ln_r{_L}_"))
    for _m in (1, 2):
        NORM_LEDGER[f"layernorm_window_kernel<{_L}, 5, {_m}>"] = ("default", _ids("lnwin", C=_C, mode=_m))
for _C, _L in _NARROW.items():
    for _g in (False, True):
        NORM_LEDGER[f"layernorm_narrow_kernel<{_L}, {int(_g)}>"] = ("default", _ids("lnact", C=_C, gelu=_g))


# --------------------------------------------------------------------------------------------------- gemm_rowpanel.hip / ff_fused.hip: cases
# rp:    ops.gemm (lnm 0) / ops.ln_gemm (lnm 1: LayerNorm prologue), K = 320: M, N, epi ("none" / "geglu"); bias (default present), res, ldr (residual
#        row stride = N + ldr), aslice (A = columns 320..639 of a [M, 960] buffer), cpad (the output is a column slice of a buffer cpad + 8 wider),
#        cs (column statistics of the output)
# rs:    ops.gemm(rowstats=): the producer of a LayerNorm fold alone (bias + residual)
# chain: that producer at N = 320, then ops.gemm_ln (LayerNorm fold) on its stored rows and statistics: N, epi, res (the consumer's)
# ff:    ops.ff_fused: M, H, res, strided (x, w1, the output and the residual each with a row stride of its own), proj (None, or which of b3 / r3 /
#        cs the projection behind the block carries)
# env:   "hook" = the child runs with AE_ROWPANEL_ANY_M=1 (one block is enough), "default" = no AE_* variable (one 192-row block per CU from 192 blocks
#        on); tiled = the case sits below that threshold and must run gemm_kernel instead, within the same bound
# M: 192 one block, 193 a block with one live row, 207 / 208 / 209 a fragment's edge, 239 / 240 / 241 a wave's row-group edge, 383 two blocks less a row.
# N / 64 in {1, 2, 3, 4, 5, 15, 40}: 2 is the ring's lead, 3 the ring, 40 = RP_MAXN.
def _rp(id, M, N, epi="none", lnm=0, **kw):
    return dict(id=id, op="rp", M=M, N=N, epi=epi, lnm=lnm, env=kw.pop("env", "hook"), **kw)


def _ff(id, M, H, **kw):
    return dict(id=id, op="ff", M=M, H=H, env=kw.pop("env", "hook"), res=kw.pop("res", False), strided=kw.pop("strided", False), proj=kw.pop("proj", None), **kw)


RP_THRESHOLD_M = 191 * 192 + 1       # 192 blocks: the smallest M the default plan gives to the row-panel / fused feed-forward kernels
ROWPANEL_CASES = [
    # ---- plain, EPI none
    _rp("rp_n64_m192", 192, 64),
    _rp("rp_n128_m193", 193, 128, res=True),
    _rp("rp_n192_m207_nobias", 207, 192, bias=False, res=True, ldr=40),
    _rp("rp_n256_m208", 208, 256),
    _rp("rp_n320_m209_slices", 209, 320, aslice=True, cpad=24, res=True, ldr=8),
    _rp("rp_n960_m239", 239, 960, res=True),
    _rp("rp_n2560_m240", 240, 2560),
    _rp("rp_n320_m241_cs", 241, 320, cs=True),
    _rp("rp_n320_m383", 383, 320, res=True),
    _rp("rp_n320_threshold", RP_THRESHOLD_M, 320, res=True, env="default"),
    _rp("rp_n320_below_threshold", RP_THRESHOLD_M - 1, 320, res=True, env="default", tiled=True),
    # ---- plain, GEGLU
    _rp("rpg_n128_m193", 193, 128, "geglu"),
    _rp("rpg_n192_m383_nobias", 383, 192, "geglu", bias=False),
    _rp("rpg_n256_m241_slices", 241, 256, "geglu", aslice=True, cpad=16),
    _rp("rpg_n320_m208", 208, 320, "geglu"),
    _rp("rpg_n2560_m192", 192, 2560, "geglu"),
    # ---- LayerNorm prologue, EPI none
    _rp("rpl_n64_m192", 192, 64, lnm=1),
    _rp("rpl_n128_m208_cs", 208, 128, lnm=1, cs=True),
    _rp("rpl_n192_m239", 239, 192, lnm=1, res=True),
    _rp("rpl_n320_m193_slices", 193, 320, lnm=1, aslice=True, cpad=8, res=True, ldr=16),
    _rp("rpl_n960_m209", 209, 960, lnm=1),
    _rp("rpl_n2560_m383_nobias", 383, 2560, lnm=1, bias=False),
    # ---- LayerNorm prologue, GEGLU
    _rp("rplg_n128_m207_cs", 207, 128, "geglu", lnm=1, cs=True),
    _rp("rplg_n192_m384", 384, 192, "geglu", lnm=1),
    _rp("rplg_n320_m241", 241, 320, "geglu", lnm=1),
    _rp("rplg_n2560_m193", 193, 2560, "geglu", lnm=1),
    # ---- row statistics (the tail branch alone, an even and an odd number of pairs)
    dict(id="rs_n64_m193", op="rs", M=193, N=64, res=True, env="hook"),
    dict(id="rs_n128_m192", op="rs", M=192, N=128, res=False, env="hook"),
    dict(id="rs_n128_m209", op="rs", M=209, N=128, res=True, env="hook"),
    dict(id="rs_n320_m240", op="rs", M=240, N=320, res=True, env="hook"),
    # ---- producer (row statistics, N = 320) -> LayerNorm fold
    dict(id="chain_n64_m193", op="chain", M=193, N=64, epi="none", res=False, env="hook"),
    dict(id="chain_n128_m207", op="chain", M=207, N=128, epi="none", res=True, env="hook"),
    dict(id="chain_n192_m384", op="chain", M=384, N=192, epi="none", res=False, env="hook"),
    dict(id="chain_n960_m241", op="chain", M=241, N=960, epi="none", res=False, env="hook"),
    dict(id="chain_n960_m192", op="chain", M=192, N=960, epi="none", res=True, env="hook"),
    dict(id="chain_n128g_m209", op="chain", M=209, N=128, epi="geglu", res=False, env="hook"),
    dict(id="chain_n2560g_m192", op="chain", M=192, N=2560, epi="geglu", res=False, env="hook"),
    dict(id="chain_n2560g_m383", op="chain", M=383, N=2560, epi="geglu", res=False, env="hook"),
    # ---- fused feed-forward
    _ff("ff_h64_m192", 192, 64, res=True),
    _ff("ff_h128_m193", 193, 128),
    _ff("ff_h1280_m241_strided", 241, 1280, res=True, strided=True),
    _ff("ff_h64_m383_strided", 383, 64, strided=True),
    _ff("ff_h1280_m383", 383, 1280, res=True),
    _ff("ff_h64_threshold", RP_THRESHOLD_M, 64, res=True, env="default"),
    _ff("ff_h64_below_threshold", RP_THRESHOLD_M - 1, 64, res=True, env="default", tiled=True),
    _ff("ffp_h64_m193_all", 193, 64, res=True, proj=dict(b3=True, r3=True, cs=True)),
    _ff("ffp_h128_m241_bare", 241, 128, proj=dict(b3=False, r3=False, cs=False)),
    _ff("ffp_h1280_m192_b3_cs", 192, 1280, res=True, proj=dict(b3=True, r3=False, cs=True)),
    _ff("ffp_h64_m383_r3_strided", 383, 64, res=True, strided=True, proj=dict(b3=False, r3=True, cs=False)),
]
ROWPANEL_CASE_IDS = [c["id"] for c in ROWPANEL_CASES]


def _rk(epi, lnm, rs=False):
    return f"gemm_rowpanel_kernel<10, {epi}, {lnm}, {str(rs).lower()}>"


def _rpids(**kw):
    return [c["id"] for c in ROWPANEL_CASES if not c.get("tiled") and all(c.get(k) == v for k, v in kw.items())]


# gemm_rowpanel_kernel<KS, EPI (0 none, 2 GEGLU), LNM (0 plain, 1 LayerNorm prologue, 2 LayerNorm fold), RS (row statistics)>; ff_fused_kernel<PROJ>
ROWPANEL_LEDGER = {
    _rk(0, 0): ("default", _rpids(op="rp", epi="none", lnm=0)),
    _rk(2, 0): ("default", _rpids(op="rp", epi="geglu", lnm=0)),
    _rk(0, 1): ("default", _rpids(op="rp", epi="none", lnm=1)),
    _rk(2, 1): ("default", _rpids(op="rp", epi="geglu", lnm=1)),      # (every feed-forward case runs it too, for the stored hidden activation)
    _rk(0, 2): ("default", _rpids(op="chain", epi="none")),
    _rk(2, 2): ("default", _rpids(op="chain", epi="geglu")),
    _rk(0, 0, True): ("default", _rpids(op="rs") + _rpids(op="chain")),
    "ff_fused_kernel<false>": ("default", _rpids(op="ff")),
    "ff_fused_kernel<true>": ("default", [c["id"] for c in ROWPANEL_CASES if c["op"] == "ff" and c["proj"]]),
}


def expected_kernels(case_id):
    """ledger keys whose `default` row lists this case"""
    return sorted(k for led in (LEDGER, NORM_LEDGER, ROWPANEL_LEDGER) for k, (kind, v) in led.items() if kind == "default" and case_id in v)


# --------------------------------------------------------------------------------------------------- attention.hip: cases
# The general attn_kernel<D, QF, NW, DBUF, BIAS, HAS_MASK, SEG2, OCC4> (tools/attn_general_route_check.py):
#   D head dim; QF 16-row query fragments per wave; NW waves per block (a block owns QB = 16 QF NW query rows); DBUF double-buffered K/V tiles
#   (every head dim below 128); BIAS 0 none, 1 rel-pos bias by look-up (from LDS when kH, kW <= 32, else from global memory), 2 rel-pos bias with
#   one key-grid row per 64-key tile (kW == 64, Nk % 64 == 0); HAS_MASK key mask; SEG2 second key/value segment; OCC4 the 128-VGPR cap of the
#   rel-pos variants on eight waves.
# A case is an `attn` case with: env (a name of ATTN_GENERAL_ENVS: the AE_* variables of the child process that runs it), qf / nw / occ (the
# variant the library must pick for it there), and the options
#   mask  "rand" | "lead" (keys 0..63 removed) | "trail" (the last whole 64-key tile removed) | "tailkey" (a key inside the ragged last tile
#         removed) | "all" (sample 0 loses every key, sample 1 takes a random mask); the mask is [B, Nk], shared by a sample's heads, and sample 1
#         always differs from sample 0
#   gate  per-sample out_scale;  onto  accumulate=True onto a pre-filled output;  o_pad  output row stride = H D + o_pad
#   nk2   second segment of nk2 keys with a per-sample scale2;  rel  (kH, kW) rel-pos bias, Nk = kH kW
# Nq sits around QB (1, QB - 1, QB, QB + 1), Nk around the 64-key tile (1, 63, 64, 65, 128, 129, 193: no ragged tile, a ragged tile of one key,
# an odd and an even tile count for the double buffer).  B H = 6 (2 for the QF = 4 cases, which the dispatch takes from Nq > 1024, Nk >= 1024).
ATTN_GENERAL_ENVS = {
    "default": {},
    "nofast": {"AE_ATTN_FAST": "0"},                                                          # head dims 40 / 80 / 160 stay in attention.hip
    "w8": {"AE_ATTN_FAST": "0", "AE_ATTN_W8": "1"},                                           # eight waves of one fragment at d = 40 / 80
    "w8_occ4": {"AE_ATTN_FAST": "0", "AE_ATTN_W8": "1", "AE_ATTN_SAM_OCC": "4"},              # + the VGPR cap on the row-per-tile bias form
    "w8_occ0": {"AE_ATTN_FAST": "0", "AE_ATTN_W8": "1", "AE_ATTN_SAM_OCC": "0"},              # + no VGPR cap on the look-up bias form
    "shortk": {"AE_ATTN_FAST": "0", "AE_ATTN_SHORTK_QF1": "1"},                               # one fragment per wave under 256 keys
}
_AG_MASKS_ALL = ("rand", "lead", "trail", "tailkey", "all")
_AG_REL_LDS = ((14, 14), (3, 5), (5, 3), (1, 31), (32, 32))
_AG_REL_GLOBAL = ((2, 40), (40, 2), (33, 3))
_AG_REL_ROWS = ((1, 64), (3, 64))


def _ag(tag, env, D, Nq, Nk, qf, nw, i=0, **kw):
    kw.setdefault("B", 2)
    kw.setdefault("H", 3)
    kw.setdefault("lay", ("bhnd", "qkv")[i % 2])
    return dict(id=f"ag_{env}_d{D}q{qf}w{nw}_{tag}", op="attn", env=env, D=D, Nq=Nq, Nk=Nk, qf=qf, nw=nw, **kw)


def _ag_group(env, D, qf, nw, kinds, full=False, occ1=False, occ2=False, masks=None, rel1=None, rel2=None):
    """the cases of one (environment, D, QF, NW); kinds: which of plain / mask / rel1 / rel2 / seg2 / gate the library sends there in that
    environment; full: the whole edge set (else the reduced one: every row still gets a ragged last query block and every hazard of its kind)"""
    QB, out = 16 * qf * nw, []
    a = lambda tag, Nq, Nk, i=0, **kw: out.append(_ag(tag, env, D, Nq, Nk, qf, nw, i, **kw))
    if "plain" in kinds:
        edges = [(1, 1), (QB - 1, 63), (QB, 64), (QB + 1, 65), (QB // 2 + 1, 128), (QB + 1, 129), (QB + 2, 193)]
        for i, (Nq, Nk) in enumerate(edges if full else edges[:1] + edges[3:]):
            a(f"n{Nq}k{Nk}", Nq, Nk, i)
    if "mask" in kinds:
        for i, m in enumerate(masks or (_AG_MASKS_ALL if full else ("rand", "lead"))):
            Nq, Nk = {"rand": (QB - 1, 193), "lead": (QB + 1, 150), "trail": (QB + 1, 150), "tailkey": (QB, 150), "all": (QB + 1, 129)}[m]
            a(f"mask_{m}", Nq, Nk, i, mask=m)
        if full:
            a("mask_rand_k64", QB + 1, 64, 1, mask="rand")
            a("mask_lead_k65", 1, 65, 0, mask="lead")       # one live key behind a dead tile
    if "rel1" in kinds:
        grids = rel1 if rel1 is not None else (_AG_REL_LDS + _AG_REL_GLOBAL if full else ((5, 3), (3, 5), (33, 3)))
        for i, (kH, kW) in enumerate(grids):
            a(f"rel{kH}x{kW}", (QB + 3, QB - 1, 1, QB + 1)[i % 4], kH * kW, i, rel=(kH, kW), occ=occ1)
    if "rel2" in kinds:
        for i, (kH, kW) in enumerate(rel2 if rel2 is not None else _AG_REL_ROWS):
            a(f"rel{kH}x{kW}", (QB + 1, QB - 1)[i % 2], kH * kW, i, rel=(kH, kW), occ=occ2)
    if "seg2" in kinds:
        for i, nk2 in enumerate((1, 8, 64, 65) if full else (8, 65)):
            a(f"seg2_{nk2}", (QB + 1, QB - 1, QB, 1)[i % 4], (77, 129, 64, 193)[i % 4], i, nk2=nk2)
    if "gate" in kinds:
        for i, (g, o, pad) in enumerate(((True, False, 0), (False, True, 0), (True, True, 8), (False, False, 8))):
            for Nq in (QB, QB + 1):
                a(("gate" if g else "") + ("onto" if o else "") + (f"pad{pad}" if pad else "") + f"_n{Nq}", Nq, (129, 65)[i % 2], i, gate=g, onto=o, o_pad=pad)
    return out


def _ag_qf4(env, kinds):
    """d = 40 with four fragments per wave (QB = 256): the dispatch wants Nq > 1024 and Nk >= 1024"""
    out = []
    a = lambda tag, Nq, Nk, **kw: out.append(_ag(tag, env, 40, Nq, Nk, 4, 4, B=2, H=1, **kw))
    if "plain" in kinds:
        a("n1025k1024", 1025, 1024, lay="qkv")
        a("n1281k1087", 1281, 1087, lay="bhnd")
    if "mask" in kinds:
        a("mask_lead", 1281, 1087, mask="lead", lay="qkv")
        a("mask_tailkey", 1281, 1087, mask="tailkey", lay="bhnd")
        a("mask_rand", 1025, 1024, mask="rand", lay="bhnd")
        a("mask_trail", 1025, 1024, mask="trail", lay="qkv")
        a("mask_all", 1025, 1087, mask="all", lay="bhnd")
    if "rel1" in kinds:
        a("rel32x32", 1025, 1024, rel=(32, 32), lay="bhnd")
        a("rel33x32", 1281, 1056, rel=(33, 32), lay="qkv")
        a("rel4x257", 1027, 1028, rel=(4, 257), lay="bhnd")
    if "rel2" in kinds:
        a("rel16x64", 1025, 1024, rel=(16, 64), lay="qkv")
        a("rel17x64", 1281, 1088, rel=(17, 64), lay="bhnd")
    return out


ATTN_GENERAL_CASES = (
    # ---- no AE_* variable: every head dim attention_fast.hip does not own, and what it declines of 40 / 80 / 160 (a key mask; a rel-pos bias at
    #      d = 40 / 160, or at d = 80 on a grid that is neither kW == 64 nor within 16 x 16, or together with out_scale / accumulate)
    _ag_group("default", 8, 2, 4, ("plain", "mask", "rel1", "rel2", "seg2"), masks=("rand", "lead", "all"))
    + _ag_group("default", 16, 2, 4, ("plain", "mask", "rel1", "rel2", "seg2"))
    + _ag_group("default", 32, 2, 4, ("plain", "mask", "rel1", "rel2", "seg2", "gate"), full=True)
    + _ag_group("default", 48, 2, 4, ("plain", "mask", "rel1", "rel2", "seg2"), masks=("rand", "lead", "tailkey"), rel1=_AG_REL_LDS + _AG_REL_GLOBAL)
    + _ag_group("default", 64, 2, 4, ("plain", "mask", "rel1", "rel2", "seg2", "gate"), full=True)
    + _ag_group("default", 96, 2, 4, ("plain", "mask", "rel1", "rel2", "seg2"))
    + _ag_group("default", 128, 2, 4, ("plain", "mask", "rel1", "rel2"), masks=("rand", "lead", "trail"))
    + _ag_group("default", 128, 2, 4, ("plain",), full=True)[1:3]                                      # the single-buffer loop at 63 / 64 keys
    + _ag_group("default", 40, 2, 4, ("mask", "rel1", "rel2"), full=True)
    + _ag_qf4("default", ("mask", "rel1", "rel2"))
    + _ag_group("default", 80, 2, 4, ("mask",), full=True)
    + _ag_group("default", 80, 1, 8, ("rel1",), occ1=True, rel1=((1, 31), (32, 32), (17, 5)) + _AG_REL_GLOBAL)
    + [_ag("rel3x64_gate", "default", 80, 129, 192, 1, 8, rel=(3, 64), gate=True, occ=False),
       _ag("rel1x64_onto", "default", 80, 127, 64, 1, 8, rel=(1, 64), onto=True, occ=False)]
    + _ag_group("default", 160, 2, 4, ("mask", "rel1", "rel2"), full=True)
    # ---- AE_ATTN_FAST=0: the plain and two-segment forms of 40 / 80 / 160
    + _ag_group("nofast", 40, 2, 4, ("plain", "seg2"), full=True)
    + _ag_qf4("nofast", ("plain",))
    + _ag_group("nofast", 80, 2, 4, ("plain", "seg2"), full=True)
    + _ag_group("nofast", 160, 2, 4, ("plain",), full=True)
    + _ag_group("nofast", 160, 1, 4, ("seg2",), full=True)
    # ---- + AE_ATTN_W8=1: eight waves of one fragment
    + _ag_group("w8", 40, 1, 8, ("plain", "mask", "seg2", "rel1", "rel2"), occ1=True, masks=("rand", "lead", "tailkey", "all"))
    + _ag_group("w8", 80, 1, 8, ("plain", "mask", "seg2"), masks=("rand", "lead", "tailkey"))
    + _ag_group("w8_occ4", 40, 1, 8, ("rel2",), occ2=True)
    + _ag_group("w8_occ4", 80, 1, 8, ("rel2",), occ2=True)
    + _ag_group("w8_occ0", 40, 1, 8, ("rel1",), rel1=((14, 14), (3, 5), (1, 31), (40, 2)))
    + _ag_group("w8_occ0", 80, 1, 8, ("rel1",), rel1=((14, 14), (5, 3), (32, 32), (33, 3)))
    # ---- AE_ATTN_FAST=0 AE_ATTN_SHORTK_QF1=1: one fragment per wave on four waves (QB = 64) under 256 keys
    + _ag_group("shortk", 40, 1, 4, ("plain", "mask", "seg2"), full=True)
    + _ag_group("shortk", 80, 1, 4, ("plain", "mask", "seg2"), masks=("rand", "lead", "tailkey"))
    + _ag_group("shortk", 160, 1, 4, ("plain", "mask"), masks=("rand", "lead", "tailkey"))
)
ATTN_GENERAL_CASE_IDS = [c["id"] for c in ATTN_GENERAL_CASES]


def attn_general_key(c):
    """the instantiation a case of ATTN_GENERAL_CASES declares"""
    rel = c.get("rel")
    bias = 0 if not rel else 2 if rel[1] == 64 and c["Nk"] % 64 == 0 else 1
    args = (c["D"], c["qf"], c["nw"], c["D"] < 128, bias, bool(c.get("mask")), bool(c.get("nk2")), bool(c.get("occ")))
    return "attn_kernel<" + ", ".join(str(x).lower() for x in args) + ">"


# --------------------------------------------------------------------------------------------------- attention.hip: ledger
# One row per attn_kernel instantiation of the build.  A row is ("default", [case ids]) — reached with every AE_* variable removed — or
# ("env", {variables}, [case ids]) — reached in a child process with every AE_* variable removed and exactly those set, because only a tuning
# knob of attention.hip sends anything there.  All cases of a row run in one environment.
def _ag_row(key):
    cases = [c for c in ATTN_GENERAL_CASES if attn_general_key(c) == key]
    envs = sorted({c["env"] for c in cases})
    assert len(envs) <= 1, (key, envs)
    ids = [c["id"] for c in cases]
    return ("default", ids) if envs in ([], ["default"]) else ("env", dict(ATTN_GENERAL_ENVS[envs[0]]), ids)


def _agk(D, qf, nw, bias=0, mask=False, seg2=False, occ4=False):
    return attn_general_key(dict(D=D, qf=qf, nw=nw, Nk=64, rel=(None, (3, 5), (1, 64))[bias], mask=mask, nk2=seg2, occ=occ4))


_AG_FORMS = dict(plain=dict(), mask=dict(mask=True), rel1=dict(bias=1), rel2=dict(bias=2), seg2=dict(seg2=True))
_AG_ROWS = (
    [(D, 2, 4, f) for D in (8, 16, 32, 40, 48, 64, 96) for f in ("plain", "mask", "rel1", "rel2", "seg2")]
    + [(D, 2, 4, f) for D in (128, 160) for f in ("plain", "mask", "rel1", "rel2")]
    + [(40, 4, 4, f) for f in ("plain", "mask", "rel1", "rel2")]
    + [(80, 2, 4, f) for f in ("plain", "mask", "seg2")]
    + [(D, 1, 4, f) for D in (40, 80, 160) for f in ("plain", "mask", "seg2")]
    + [(D, 1, 8, f) for D in (40, 80) for f in ("plain", "mask", "rel1", "rel2", "seg2")]
)
ATTN_GENERAL_LEDGER = {_agk(D, qf, nw, **_AG_FORMS[f]): None for D, qf, nw, f in _AG_ROWS}
ATTN_GENERAL_LEDGER.update({_agk(D, 1, 8, bias=b, occ4=True): None for D in (40, 80) for b in (1, 2)})
ATTN_GENERAL_LEDGER = {k: _ag_row(k) for k in ATTN_GENERAL_LEDGER}


def attn_general_expected(case_id):
    """ATTN_GENERAL_LEDGER keys whose row lists this case"""
    return sorted(k for k, row in ATTN_GENERAL_LEDGER.items() if case_id in row[-1])
