"""Plain-torch fp32 restatement of GroundingDINO's Swin backbone (SwinTransformer: patch convolution with right / bottom zero padding, patch
norm, stages of pre-LN blocks with (shifted) window attention — pad, roll, partition, relative position bias, a -100 mask built from the
slices, reverse, roll back, crop, in the reference's order —, GELU MLP, PatchMerging, one norm per output) over a state dict — test
infrastructure: the CPU suite pins it to tests/golden/swin_tiny_*.npz (which the reference's own class produced), the GPU suite trusts it at
sizes the fixtures cannot hold.

`bf16_storage=True` gives the CONTROL of the project's standing tolerance rule (tests/dino_ref.py's convention): fp32 arithmetic, matrix
weights rounded to bf16 as the module packs them (patch embedding, qkv, proj, fc1, fc2, reduction) and every activation rounded to bf16 exactly
where the HIP path stores one in HBM.  Each `_st(...)` below is one `# bf16:` mark of anyedit_amd/groundingdino/swin_transformer.py; keep the
two lists in step.  NOT rounded: biases, LayerNorm vectors, the relative position bias, the fc1 product, logits and probabilities.

Also here, as separate functions the CPU suite compares: the kernel's closed forms (the mask regions 3 r(ys) + r(xs), the row addressing) next
to the reference-style constructions (slices; pad -> roll -> partition of an index image).
"""
import torch
import torch.nn.functional as F

GEOMETRIES = {  # build_swin_transformer's table
    "swin_T_224_1k": dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7),
    "swin_B_224_22k": dict(embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=7),
    "swin_B_384_22k": dict(embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=12),
    "swin_L_224_22k": dict(embed_dim=192, depths=[2, 2, 18, 2], num_heads=[6, 12, 24, 48], window_size=7),
    "swin_L_384_22k": dict(embed_dim=192, depths=[2, 2, 18, 2], num_heads=[6, 12, 24, 48], window_size=12),
}


def _round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def up(n, m):
    return (n + m - 1) // m * m


def relative_position_index(ws):
    """WindowAttention's buffer: [ws^2, ws^2], entry (a, b) = (ya - yb + ws - 1) (2 ws - 1) + (xa - xb + ws - 1)."""
    ys, xs = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    return (ys[:, None] - ys[None, :] + ws - 1) * (2 * ws - 1) + (xs[:, None] - xs[None, :] + ws - 1)


def gathered_bias(table, ws):
    """relative_position_bias_table [(2 ws - 1)^2, nH] -> [nH, N, N] as WindowAttention.forward gathers it."""
    N = ws * ws
    return table[relative_position_index(ws).reshape(-1)].view(N, N, -1).permute(2, 0, 1).contiguous()


def partition(x, ws):
    """[B, Hp, Wp, C] -> [B nW, ws ws, C], windows row-major."""
    B, Hp, Wp, C = x.shape
    return x.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def reverse(win, ws, Hp, Wp):
    B = win.shape[0] // ((Hp // ws) * (Wp // ws))
    return win.view(B, Hp // ws, Wp // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, -1)


def regions_by_slices(Hp, Wp, ws, shift):
    """BasicLayer.forward's img_mask: nine regions written through three slices per axis, in the shifted frame -> [Hp, Wp]."""
    img = torch.zeros(Hp, Wp)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[hs, wsl] = cnt
            cnt += 1
    return img


def regions_by_formula(Hp, Wp, ws, shift):
    """The kernel's closed form: 3 r(ys) + r(xs), r(p) = 0 for p < L - ws, 1 for p < L - shift, 2 otherwise."""
    r = lambda L: torch.tensor([0 if p < L - ws else (1 if p < L - shift else 2) for p in range(L)])
    return (3 * r(Hp)[:, None] + r(Wp)[None, :]).float()


def shift_mask(Hp, Wp, ws, shift):
    """[nW, N, N]: -100 where the regions of query and key differ, 0 elsewhere."""
    m = partition(regions_by_slices(Hp, Wp, ws, shift).view(1, Hp, Wp, 1), ws).squeeze(-1)
    d = m[:, None, :] - m[:, :, None]
    return torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))


def rows_by_partition(H, W, ws, shift):
    """Image row y W + x of every window token, -1 for pad tokens, by pad -> roll -> partition of an index image: [nW, N]."""
    Hp, Wp = up(H, ws), up(W, ws)
    idx = F.pad(torch.arange(H * W, dtype=torch.float32).view(1, H, W, 1), (0, 0, 0, Wp - W, 0, Hp - H), value=-1.0)
    if shift > 0:
        idx = torch.roll(idx, shifts=(-shift, -shift), dims=(1, 2))
    return partition(idx, ws).squeeze(-1).long()


def rows_by_formula(H, W, ws, shift):
    """The kernel's addressing: token (i, j) of window (wy, wx) sits at ((wy ws + i + shift) mod Hp, (wx ws + j + shift) mod Wp)."""
    Hp, Wp = up(H, ws), up(W, ws)
    out = []
    for wy in range(Hp // ws):
        for wx in range(Wp // ws):
            row = []
            for n in range(ws * ws):
                i, j = divmod(n, ws)
                y, x = (wy * ws + i + shift) % Hp, (wx * ws + j + shift) % Wp
                row.append(y * W + x if y < H and x < W else -1)
            out.append(row)
    return torch.tensor(out)


def window_attention(qkv, bias, H, W, heads, ws, shift, scale):
    """The reference's order on packed q | k | v rows that are ALREADY padded: qkv [B, Hp, Wp, 3C] (pad positions hold what the qkv Linear
    gives for a zero row) -> (softmax(...) v, softmax(...) |v|), both [B, H, W, C] (the second is the scale of the accumulated products, for
    an error bound).  Any float dtype; the GPU suite runs it in float64."""
    B, Hp, Wp, C3 = qkv.shape
    C, N = C3 // 3, ws * ws
    D = C // heads
    x = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2)) if shift > 0 else qkv
    win = partition(x, ws).view(-1, N, 3, heads, D).permute(2, 0, 3, 1, 4)
    q, k, v = win[0], win[1], win[2]
    attn = (q * scale) @ k.transpose(-2, -1) + bias.to(qkv.dtype)[None]
    if shift > 0:
        m = shift_mask(Hp, Wp, ws, shift).to(qkv.dtype)
        nW = m.shape[0]
        attn = (attn.view(-1, nW, heads, N, N) + m[None, :, None]).view(-1, heads, N, N)
    p = attn.softmax(-1)

    def back(t):
        o = reverse(t.transpose(1, 2).reshape(-1, N, C), ws, Hp, Wp)
        if shift > 0:
            o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
        return o[:, :H, :W].contiguous()

    return back(p @ v), back(p @ v.abs())


def merge_rows(x, H, W):
    """PatchMerging's gather: [B, H W, C] -> [B, ceil(H/2) ceil(W/2), 4C], odd maps zero-padded."""
    B, _, C = x.shape
    x = F.pad(x.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
    return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).flatten(1, 2)


def fixture_state_dict(arrs, prefix="w."):
    """State dict of a swin_tiny_*_w<i>.npz fixture: floats are stored as bf16 bit patterns (int16), the relative_position_index buffers as
    int16 integers."""
    import numpy as np
    out = {}
    for k, v in arrs.items():
        if k.startswith(prefix):
            t = torch.from_numpy(np.asarray(v))
            out[k[len(prefix):]] = t.long() if k.endswith("relative_position_index") else t.view(torch.bfloat16).float()
    return out


def swin_forward(sd, px, cfg, bf16_storage=False):
    """sd: state dict with the reference's keys; px [B, Cin, H, W]; cfg: embed_dim, depths, num_heads, window_size (+ patch_size 4, out_indices all
    stages, qk_scale None).  Which stages downsample is read from the state dict.  Returns dict(outs = the NCHW maps of out_indices,
    stage_in = the [B, H W, C] input of every stage, sizes = [(H, W)] of every stage)."""
    _st = _round if bf16_storage else (lambda t: t)
    f = lambda k: sd[k].float()
    w = (lambda k: _round(sd[k].float())) if bf16_storage else f
    ws, P = cfg["window_size"], cfg.get("patch_size", 4)
    depths, heads = cfg["depths"], cfg["num_heads"]
    out_indices = cfg.get("out_indices", tuple(range(len(depths))))
    x = _st(px.float())                                                                              # bf16: pixels as patch rows
    B, _, H, W = x.shape
    x = F.pad(x, (0, up(W, P) - W, 0, up(H, P) - H))
    x = F.conv2d(x, w("patch_embed.proj.weight"), f("patch_embed.proj.bias"), stride=P)
    H, W = x.shape[2:]
    x = _st(x.flatten(2).transpose(1, 2))                                                            # bf16: patch embedding
    if "patch_embed.norm.weight" in sd:
        x = _st(F.layer_norm(x, x.shape[-1:], f("patch_embed.norm.weight"), f("patch_embed.norm.bias"), 1e-5))   # bf16: patch norm output
    outs, stage_in, sizes = [], [], []
    for i, depth in enumerate(depths):
        C, nH = x.shape[-1], heads[i]
        scale = cfg.get("qk_scale") or (C // nH) ** -0.5
        Hp, Wp = up(H, ws), up(W, ws)
        stage_in.append(x)
        sizes.append((H, W))
        for j in range(depth):
            q = f"layers.{i}.blocks.{j}."
            shift = 0 if j % 2 == 0 else ws // 2
            h = _st(F.layer_norm(x, (C,), f(q + "norm1.weight"), f(q + "norm1.bias"), 1e-5))        # bf16: norm1 output
            h = F.pad(h.view(B, H, W, C), (0, 0, 0, Wp - W, 0, Hp - H))
            qkv = _st(F.linear(h, w(q + "attn.qkv.weight"), f(q + "attn.qkv.bias") if q + "attn.qkv.bias" in sd else None))   # bf16: packed q | k | v (a pad row: the bias)
            bias = gathered_bias(f(q + "attn.relative_position_bias_table"), ws)
            o = _st(window_attention(qkv, bias, H, W, nH, ws, shift, scale)[0].view(B, H * W, C))    # bf16: attention output
            x = _st(x + F.linear(o, w(q + "attn.proj.weight"), f(q + "attn.proj.bias")))             # bf16: residual stream after the attention add
            h = _st(F.layer_norm(x, (C,), f(q + "norm2.weight"), f(q + "norm2.bias"), 1e-5))        # bf16: norm2 output
            u = _st(F.gelu(F.linear(h, w(q + "mlp.fc1.weight"), f(q + "mlp.fc1.bias"))))             # bf16: activated hidden values (the fc1 product stays fp32)
            x = _st(x + F.linear(u, w(q + "mlp.fc2.weight"), f(q + "mlp.fc2.bias")))                 # bf16: residual stream after the MLP add
        if i in out_indices:
            z = _st(F.layer_norm(x, (C,), f(f"norm{i}.weight"), f(f"norm{i}.bias"), 1e-5))          # bf16: output norm
            outs.append(z.view(B, H, W, C).permute(0, 3, 1, 2).contiguous())
        d = f"layers.{i}.downsample."
        if d + "reduction.weight" in sd:
            m = _st(F.layer_norm(merge_rows(x, H, W), (4 * C,), f(d + "norm.weight"), f(d + "norm.bias"), 1e-5))   # bf16: merged and normed rows
            x = _st(F.linear(m, w(d + "reduction.weight")))                                          # bf16: reduced rows = the next stage's input
            H, W = (H + 1) // 2, (W + 1) // 2
    return dict(outs=tuple(outs), stage_in=stage_in, sizes=sizes)


def nested_masks(mask, shapes):
    """SwinTransformer.forward's masks: the input mask [B, H, W] bool nearest-interpolated to every output map."""
    return [F.interpolate(mask[None].float(), size=tuple(s)).to(torch.bool)[0] for s in shapes]


def seeded_state_dict(cfg, seed=0, dilation=False):
    """Seeded weights with the reference's keys for sizes no fixture can hold: Linear / conv weights at their fan-in scale, and the fixture
    generator's re-draws (relative position bias table N(0, 0.5^2), LayerNorm gamma U(0.25, 1.75), beta N(0, 0.1^2), every bias N(0, 0.3^2)),
    every tensor rounded to bf16; the index buffers as computed."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s, std: torch.randn(*s, generator=g) * std
    ws, P, Cin = cfg["window_size"], cfg.get("patch_size", 4), cfg.get("in_chans", 3)
    depths, heads = cfg["depths"], cfg["num_heads"]
    L = len(depths)
    dims = [cfg["embed_dim"] * 2 ** i for i in range(L)]
    down = [i < L - 1 for i in range(L)]
    if dilation:
        down[-2] = False
        dims[-1] = dims[-1] // 2
    sd = {}

    def norm(name, C):
        sd[name + ".weight"] = 0.25 + 1.5 * torch.rand(C, generator=g)
        sd[name + ".bias"] = n(C, std=0.1)

    def lin(name, o, i, bias=True):
        sd[name + ".weight"] = n(o, i, std=i ** -0.5)
        if bias:
            sd[name + ".bias"] = n(o, std=0.3)

    sd["patch_embed.proj.weight"] = n(dims[0], Cin, P, P, std=(Cin * P * P) ** -0.5)
    sd["patch_embed.proj.bias"] = n(dims[0], std=0.3)
    norm("patch_embed.norm", dims[0])
    for i in range(L):
        C = dims[i]
        for j in range(depths[i]):
            q = f"layers.{i}.blocks.{j}."
            norm(q + "norm1", C)
            lin(q + "attn.qkv", 3 * C, C)
            lin(q + "attn.proj", C, C)
            sd[q + "attn.relative_position_bias_table"] = n((2 * ws - 1) ** 2, heads[i], std=0.5)
            norm(q + "norm2", C)
            lin(q + "mlp.fc1", 4 * C, C)
            lin(q + "mlp.fc2", C, 4 * C)
        if down[i]:
            norm(f"layers.{i}.downsample.norm", 4 * C)
            lin(f"layers.{i}.downsample.reduction", 2 * C, 4 * C, bias=False)
        norm(f"norm{i}", C)
    sd = {k: _round(t) for k, t in sd.items()}
    for i in range(L):
        for j in range(depths[i]):
            sd[f"layers.{i}.blocks.{j}.attn.relative_position_index"] = relative_position_index(ws)
    return sd
