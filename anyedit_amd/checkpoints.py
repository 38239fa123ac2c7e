"""Key layouts of the weights AnyEdit loads, and the mapping between them — SURVEY.md §8(f) N4 "on-disk formats".

The reference reaches the same SD-1.5-shaped UNet through two libraries with two state-dict schemas:
  * the in-tree `ldm` UNet (`input_blocks.N.M...`, ldm/modules/diffusionmodules/openaimodel.py:413-786) — what this package mirrors and
    what `.ckpt` files of the CompVis lineage hold under `model.diffusion_model.`;
  * diffusers' UNet2DConditionModel / AutoencoderKL (`down_blocks.i.resnets.j...`), which is what `from_pretrained(..., subfolder="unet")`
    reads in train.py:405-412 and tools/global_tool.py:74-76 (InstructPix2Pix / AnySD weights ship in this layout).
The mapping is DERIVED by walking the constructed module (which block of which level is a ResBlock / SpatialTransformer / Down- or
Upsample), not from a table, so it holds for every geometry the UNet mirror builds (SD-1.5, SD-2.1 / AnyDoor, the tiny test nets).
diffusers is a third-party dependency absent from /root/reference and from this image: its side of the mapping is restated from its
published schema — PARITY UNPINNED (tests check bijectivity, shapes and a set of well-known key pairs).
"""
import re

from anyedit_amd.ldm.modules.attention import SpatialTransformer
from anyedit_amd.ldm.modules.diffusionmodules.openaimodel import Downsample, ResBlock, Upsample

_RES = (("in_layers.0", "norm1"), ("in_layers.2", "conv1"), ("emb_layers.1", "time_emb_proj"), ("out_layers.0", "norm2"),
        ("out_layers.3", "conv2"), ("skip_connection", "conv_shortcut"))


def unet_prefix_map(unet):
    """ldm module-path prefix -> diffusers prefix, for every leaf group of `unet` (a UNetModel mirror)."""
    pm = {"time_embed.0": "time_embedding.linear_1", "time_embed.2": "time_embedding.linear_2", "input_blocks.0.0": "conv_in",
          "out.0": "conv_norm_out", "out.2": "conv_out"}

    def add_res(ldm, dif):
        for a, b in _RES:
            pm[f"{ldm}.{a}"] = f"{dif}.{b}"

    level, n_res, n_att = 0, 0, 0
    for i, blk in enumerate(unet.input_blocks):
        if i == 0:
            continue
        for j, m in enumerate(blk):
            if isinstance(m, ResBlock):
                add_res(f"input_blocks.{i}.{j}", f"down_blocks.{level}.resnets.{n_res}")
                n_res += 1
            elif isinstance(m, SpatialTransformer):
                pm[f"input_blocks.{i}.{j}"] = f"down_blocks.{level}.attentions.{n_att}"
                n_att += 1
            elif isinstance(m, Downsample):
                pm[f"input_blocks.{i}.{j}.op"] = f"down_blocks.{level}.downsamplers.0.conv"
                level, n_res, n_att = level + 1, 0, 0
    n_res = n_att = 0
    for j, m in enumerate(unet.middle_block):
        if isinstance(m, ResBlock):
            add_res(f"middle_block.{j}", f"mid_block.resnets.{n_res}")
            n_res += 1
        elif isinstance(m, SpatialTransformer):
            pm[f"middle_block.{j}"] = f"mid_block.attentions.{n_att}"
            n_att += 1
    level, n_res, n_att = 0, 0, 0
    for i, blk in enumerate(unet.output_blocks):
        for j, m in enumerate(blk):
            if isinstance(m, ResBlock):
                add_res(f"output_blocks.{i}.{j}", f"up_blocks.{level}.resnets.{n_res}")
                n_res += 1
            elif isinstance(m, SpatialTransformer):
                pm[f"output_blocks.{i}.{j}"] = f"up_blocks.{level}.attentions.{n_att}"
                n_att += 1
            elif isinstance(m, Upsample):
                pm[f"output_blocks.{i}.{j}.conv"] = f"up_blocks.{level}.upsamplers.0.conv"
                level, n_res, n_att = level + 1, 0, 0
    return pm


def _key_map(keys, prefix_map):
    """Longest-prefix rewrite of every key; raises on a key no prefix covers."""
    order = sorted(prefix_map, key=len, reverse=True)
    out = {}
    for k in keys:
        for p in order:
            if k == p or k.startswith(p + "."):
                out[k] = prefix_map[p] + k[len(p):]
                break
        else:
            raise KeyError(f"no layout rule covers key '{k}'")
    return out


def unet_ldm_to_diffusers_keys(unet):
    """{ldm key: diffusers key} for every entry of unet.state_dict()."""
    return _key_map(unet.state_dict().keys(), unet_prefix_map(unet))


def _fit(t, like):
    """1x1-conv <-> linear weights differ only by trailing singleton dims between the two libraries' variants."""
    if t.shape != like.shape and t.numel() == like.numel() and t.squeeze().shape == like.squeeze().shape:
        return t.reshape(like.shape)
    return t


def convert_diffusers_unet(unet, diffusers_sd):
    """diffusers UNet2DConditionModel state dict -> state dict in `unet`'s (ldm) layout.  Every key must be consumed and every
    parameter of `unet` produced, with equal shapes (up to the 1x1-conv/linear reshape); anything else raises."""
    k2d = unet_ldm_to_diffusers_keys(unet)
    ref = unet.state_dict()
    missing = [d for d in k2d.values() if d not in diffusers_sd]
    extra = sorted(set(diffusers_sd) - set(k2d.values()))
    if missing or extra:
        raise KeyError(f"diffusers UNet layout mismatch: {len(missing)} missing (e.g. {missing[:3]}), {len(extra)} unexpected (e.g. {extra[:3]})")
    out = {}
    for k, d in k2d.items():
        t = _fit(diffusers_sd[d], ref[k])
        if t.shape != ref[k].shape:
            raise ValueError(f"{d} -> {k}: shape {tuple(t.shape)} != {tuple(ref[k].shape)}")
        out[k] = t
    return out


def convert_unet_to_diffusers(unet, ldm_sd=None):
    """The inverse direction (e.g. to hand trained weights back to a diffusers pipeline)."""
    sd = unet.state_dict() if ldm_sd is None else ldm_sd
    return {d: sd[k] for k, d in unet_ldm_to_diffusers_keys(unet).items()}


# ------------------------------------------------------------------------------------------------------------------ VAE
_VAE_RES = (("nin_shortcut", "conv_shortcut"),)
_VAE_ATTN = (("norm", "group_norm"), ("q", "to_q"), ("k", "to_k"), ("v", "to_v"), ("proj_out", "to_out.0"))


def vae_prefix_map(vae):
    """ldm AutoencoderKL (ldm/modules/diffusionmodules/model.py:452-653) prefix -> diffusers AutoencoderKL prefix."""
    pm = {"quant_conv": "quant_conv", "post_quant_conv": "post_quant_conv"}
    for side in ("encoder", "decoder"):
        net = getattr(vae, side)
        for name in ("conv_in", "conv_out"):
            pm[f"{side}.{name}"] = f"{side}.{name}"
        pm[f"{side}.norm_out"] = f"{side}.conv_norm_out"
        pm[f"{side}.mid.block_1"] = f"{side}.mid_block.resnets.0"
        pm[f"{side}.mid.block_2"] = f"{side}.mid_block.resnets.1"
        for a, b in _VAE_ATTN:
            pm[f"{side}.mid.attn_1.{a}"] = f"{side}.mid_block.attentions.0.{b}"
        levels = net.down if side == "encoder" else net.up
        n = len(levels)
        for i, lv in enumerate(levels):
            di = i if side == "encoder" else n - 1 - i                 # the ldm decoder indexes `up` from the lowest resolution's end
            grp = "down_blocks" if side == "encoder" else "up_blocks"
            for j in range(len(lv.block)):
                pm[f"{side}.{'down' if side == 'encoder' else 'up'}.{i}.block.{j}"] = f"{side}.{grp}.{di}.resnets.{j}"
            if hasattr(lv, "downsample"):
                pm[f"{side}.down.{i}.downsample.conv"] = f"{side}.down_blocks.{di}.downsamplers.0.conv"
            if hasattr(lv, "upsample"):
                pm[f"{side}.up.{i}.upsample.conv"] = f"{side}.up_blocks.{di}.upsamplers.0.conv"
    return pm


def vae_ldm_to_diffusers_keys(vae):
    km = _key_map([k for k in vae.state_dict().keys() if not k.startswith("loss.")], vae_prefix_map(vae))
    return {k: re.sub(r"\.nin_shortcut\.", ".conv_shortcut.", d) for k, d in km.items()}


def convert_diffusers_vae(vae, diffusers_sd):
    """diffusers AutoencoderKL state dict -> `vae`'s (ldm) layout; the mid-block attention projections are Linear there and 1x1 convs
    here (reshape only).  Older diffusers files name them query/key/value/proj_attn: accepted as aliases."""
    alias = {"to_q": "query", "to_k": "key", "to_v": "value", "to_out.0": "proj_attn"}
    ref = vae.state_dict()
    out = {}
    for k, d in vae_ldm_to_diffusers_keys(vae).items():
        if d not in diffusers_sd:
            for new, old in alias.items():
                if f".attentions.0.{new}." in d and d.replace(f".{new}.", f".{old}.") in diffusers_sd:
                    d = d.replace(f".{new}.", f".{old}.")
                    break
            else:
                raise KeyError(f"diffusers VAE layout mismatch: '{d}' (for '{k}') not found")
        t = _fit(diffusers_sd[d], ref[k])
        if t.shape != ref[k].shape:
            raise ValueError(f"{d} -> {k}: shape {tuple(t.shape)} != {tuple(ref[k].shape)}")
        out[k] = t
    return out


def load_unet_weights(unet, path, location="cpu"):
    """Load a UNet from any of the on-disk forms: an ldm state dict (bare, or under `model.diffusion_model.` in a full SD checkpoint)
    or a diffusers `diffusion_pytorch_model.{safetensors,bin}`.  Returns the layout that was recognised."""
    from anyedit_amd.cldm.model import load_state_dict
    sd = load_state_dict(path, location)
    own = set(unet.state_dict().keys())
    if own <= set(sd.keys()):
        unet.load_state_dict({k: sd[k] for k in own})
        return "ldm"
    pref = "model.diffusion_model."
    if all(pref + k in sd for k in own):
        unet.load_state_dict({k: sd[pref + k] for k in own})
        return "ldm-checkpoint"
    unet.load_state_dict(convert_diffusers_unet(unet, sd))
    return "diffusers"


def text_encoder_state_dict(embedder, sd):
    """The CLIP text tower's entries of a state dict, in `embedder`'s (FrozenCLIPEmbedder) key layout.  Recognised forms: a full SD-1.5
    checkpoint (`cond_stage_model.transformer.text_model.*`), the tower alone (`transformer.text_model.*`), a transformers CLIPTextModel
    (`text_model.*`) and newer transformers that dropped that level (`embeddings.*`, `encoder.*`, `final_layer_norm.*`).  The
    `position_ids` buffer of old checkpoints is dropped.  Every parameter of the tower must be found with its shape; anything else raises."""
    own = embedder.state_dict()
    hit = None
    for pref in ("cond_stage_model.", "", "text_encoder."):
        for strip in ("", "transformer.", "transformer.text_model."):     # the file's keys lack this leading part of ours
            if all(pref + k[len(strip):] in sd for k in own):
                hit = {k: sd[pref + k[len(strip):]] for k in own}
                break
        if hit is not None:
            break
    if hit is None:
        raise KeyError(f"no CLIP text tower found: none of the known layouts holds all {len(own)} tensors (e.g. '{next(iter(own))}')")
    for k, v in hit.items():
        if tuple(v.shape) != tuple(own[k].shape):
            raise ValueError(f"{k}: shape {tuple(v.shape)} in the file, {tuple(own[k].shape)} in the tower")
    return hit


def load_clip_vision(tower, path_or_state_dict, location="cpu"):
    """Fills a `CLIPVisionModelWithProjection` (train.py:404 `from_pretrained(args.image_encoder_path)`) from a file or a state dict.
    Recognised forms: the Hugging Face layout (`vision_model.*`, `visual_projection.weight`), the same under an `image_encoder.` prefix (keys
    outside that prefix are ignored then), and the form without the `vision_model.` level (`embeddings.*`, `pre_layrnorm.*`, `encoder.*`,
    `post_layernorm.*`).  Missing or unexpected keys are reported as `load_state_dict(strict=True)` reports them.  Returns the form found."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        from anyedit_amd.cldm.model import load_state_dict
        sd = load_state_dict(sd, location)
    layout = "huggingface"
    if any(k.startswith("image_encoder.") for k in sd):
        sd = {k[len("image_encoder."):]: v for k, v in sd.items() if k.startswith("image_encoder.")}
        layout = "image_encoder"
    if not any(k.startswith("vision_model.") for k in sd):
        sd = {(k if k.startswith("visual_projection.") else "vision_model." + k): v for k, v in sd.items()}
        layout += "-flat"
    tower.load_state_dict(sd, strict=True)
    return layout


def load_dinov2(module, path_or_state_dict, location="cpu"):
    """Fills a `DinoVisionTransformer` or a `FrozenDinoV2Encoder` (modules.py:285-287 `dinov2.load_state_dict(torch.load(DINOv2_weight_path))`)
    from a file or a state dict.  Recognised forms: a bare DINOv2 file (`cls_token`, `pos_embed`, `blocks.N.*` ...: `dinov2_vit*14_pretrain.pth`)
    into the tower or into the encoder's `.model` (its projector is left as it is); an AnyDoor checkpoint's `cond_stage_model.`-prefixed entries
    (keys outside that prefix are ignored then) and the flat `model.*` / `projector.*` dict, both into the encoder.  Missing or unexpected
    keys are reported as `load_state_dict(strict=True)` reports them.  Returns the form found."""
    from anyedit_amd.ldm.modules.encoders.dino_vision import FrozenDinoV2Encoder
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        from anyedit_amd.cldm.model import load_state_dict
        sd = load_state_dict(sd, location)
    encoder = isinstance(module, FrozenDinoV2Encoder)
    layout = "encoder"
    if any(k.startswith("cond_stage_model.") for k in sd):
        sd = {k[len("cond_stage_model."):]: v for k, v in sd.items() if k.startswith("cond_stage_model.")}
        layout = "cond_stage_model"
    if any(k.startswith(("model.", "projector.")) for k in sd):
        if not encoder:
            raise ValueError(f"load_dinov2: the state dict holds an encoder ({layout}: model.* / projector.*); pass a FrozenDinoV2Encoder, or its .model with a bare DINOv2 file")
        module.load_state_dict(sd, strict=True)
        return layout
    (module.model if encoder else module).load_state_dict(sd, strict=True)
    return "dinov2"


def load_groundingdino_backbone(model, path_or_state_dict, location="cpu"):
    """Fills a `groundingdino.swin_transformer.SwinTransformer` from a file or a state dict.  Recognised forms: a bare Swin state dict
    (`patch_embed.*`, `layers.I.*`, `normI.*`); a GroundingDINO checkpoint (groundingdino/util/inference.py:35-36 `torch.load(path)["model"]`)
    whose backbone sits under `backbone.0.` (`Joiner[0]`; every other entry is ignored); the same with a `module.` prefix in front.  The
    persistent `relative_position_index` buffers are checked against the computed ones.  Missing or unexpected keys are reported as
    `load_state_dict(strict=True)` reports them.  Returns the form found."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        from anyedit_amd.cldm.model import load_state_dict
        sd = load_state_dict(sd, location)
    layout = "swin"
    if isinstance(sd.get("model"), dict):
        sd = sd["model"]
        layout = "groundingdino"
    for prefix, name in (("module.backbone.0.", "groundingdino-module"), ("backbone.0.", "groundingdino")):
        if any(k.startswith(prefix) for k in sd):
            sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
            layout = name
            break
    model.load_state_dict(sd, strict=True)
    return layout


def load_groundingdino_encoder(module, path_or_state_dict, location="cpu"):
    """Fills a `groundingdino.transformer.TransformerEncoder` (the feature enhancer) from a file or a state dict.  Recognised forms: a bare
    encoder state dict (`layers.I.*`, `text_layers.I.*`, `fusion_layers.I.*`); a GroundingDINO checkpoint (`torch.load(path)["model"]` or the
    dict itself) whose enhancer sits under `transformer.encoder.` (every other entry is ignored); the same with a `module.` prefix in front.
    Strict: a key the module has and the checkpoint lacks, or the reverse, raises a KeyError that names it.  Returns the form found."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        from anyedit_amd.cldm.model import load_state_dict
        sd = load_state_dict(sd, location)
    layout = "encoder"
    if isinstance(sd.get("model"), dict):
        sd = sd["model"]
    for prefix, name in (("module.transformer.encoder.", "groundingdino-module"), ("transformer.encoder.", "groundingdino")):
        if any(k.startswith(prefix) for k in sd):
            sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
            layout = name
            break
    own = module.state_dict()
    missing = sorted(k for k in own if k not in sd)
    if missing:
        raise KeyError(f"load_groundingdino_encoder: {len(missing)} tensor(s) of the module are not in the checkpoint ({layout} form), first: '{missing[0]}'")
    unexpected = sorted(k for k in sd if k not in own)
    if unexpected:
        raise KeyError(f"load_groundingdino_encoder: {len(unexpected)} checkpoint tensor(s) have no place in the module ({layout} form), first: '{unexpected[0]}'")
    module.load_state_dict(sd, strict=True)
    return layout


def load_groundingdino_transformer(module, path_or_state_dict, location="cpu"):
    """Fills a `groundingdino.transformer.Transformer` (with its heads attached: enc_out_bbox_embed, decoder.bbox_embed, ...) from a file or a
    state dict.  Recognised forms: a bare Transformer state dict; a GroundingDINO checkpoint (`torch.load(path)["model"]` or the dict itself) whose
    `transformer.*` entries are read — such a checkpoint lists the shared box head under `bbox_embed.*` too; only the `transformer.` copies are
    read; the same with a `module.` prefix in front.  Strict, as `load_groundingdino_encoder`.  Returns the form found."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        from anyedit_amd.cldm.model import load_state_dict
        sd = load_state_dict(sd, location)
    layout = "transformer"
    if isinstance(sd.get("model"), dict):
        sd = sd["model"]
    for prefix, name in (("module.transformer.", "groundingdino-module"), ("transformer.", "groundingdino")):
        if any(k.startswith(prefix) for k in sd):
            sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
            layout = name
            break
    own = module.state_dict()
    missing = sorted(k for k in own if k not in sd)
    if missing:
        raise KeyError(f"load_groundingdino_transformer: {len(missing)} tensor(s) of the module are not in the checkpoint ({layout} form), first: '{missing[0]}'")
    unexpected = sorted(k for k in sd if k not in own)
    if unexpected:
        raise KeyError(f"load_groundingdino_transformer: {len(unexpected)} checkpoint tensor(s) have no place in the module ({layout} form), first: '{unexpected[0]}'")
    module.load_state_dict(sd, strict=True)
    return layout


def load_groundingdino_text(module, path_or_state_dict, location="cpu"):
    """Fills a `groundingdino.groundingdino.GroundingDINOText` (`bert.*` + `feat_map.*`) from a file or a state dict.  Recognised forms: a
    GroundingDINO checkpoint (`torch.load(path)["model"]` or the dict itself) whose `bert.*` and `feat_map.*` entries are read and every other
    entry ignored; the same with a `module.` prefix in front; a bare BertModel state dict (`embeddings.*`, `encoder.layer.N.*`, `pooler.dense.*`)
    with `feat_map.*` beside it.  The `embeddings.position_ids` / `embeddings.token_type_ids` buffers of older checkpoints are tolerated.
    Strict, as `load_groundingdino_encoder`.  Returns the form found."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        from anyedit_amd.cldm.model import load_state_dict
        sd = load_state_dict(sd, location)
    if isinstance(sd.get("model"), dict):
        sd = sd["model"]
    if any(k.startswith("module.bert.") for k in sd):
        layout = "groundingdino-module"
        sd = {k[len("module."):]: v for k, v in sd.items() if k.startswith(("module.bert.", "module.feat_map."))}
    elif any(k.startswith("bert.") for k in sd):
        layout = "groundingdino"
        sd = {k: v for k, v in sd.items() if k.startswith(("bert.", "feat_map."))}
    else:
        layout = "bert"
        sd = {(k if k.startswith("feat_map.") else "bert." + k): v for k, v in sd.items()}
    sd = {k: v for k, v in sd.items() if k not in ("bert.embeddings.position_ids", "bert.embeddings.token_type_ids")}
    own = module.state_dict()
    missing = sorted(k for k in own if k not in sd)
    if missing:
        raise KeyError(f"load_groundingdino_text: {len(missing)} tensor(s) of the module are not in the checkpoint ({layout} form), first: '{missing[0]}'")
    unexpected = sorted(k for k in sd if k not in own)
    if unexpected:
        raise KeyError(f"load_groundingdino_text: {len(unexpected)} checkpoint tensor(s) have no place in the module ({layout} form), first: '{unexpected[0]}'")
    module.load_state_dict(sd, strict=True)
    return layout


GROUNDINGDINO_TOLERATED = ("bert.embeddings.position_ids", "bert.embeddings.token_type_ids")
GROUNDINGDINO_TOLERATED_PREFIXES = ("label_enc.",)


def load_groundingdino(model, path_or_state_dict, location="cpu"):
    """Fills a `groundingdino.groundingdino.GroundingDINO` from a file or a state dict: a checkpoint's `{"model": ...}` (groundingdino/util/
    inference.py:35-36) or the bare state dict, with or without a `module.` prefix on every key.  Strict: every tensor of the model must be in
    the checkpoint (a shared head under every alias, as PyTorch saves it) and every checkpoint tensor must have a place, except the entries
    public checkpoints carry and the model does not hold: the buffers `bert.embeddings.position_ids` (and `bert.embeddings.token_type_ids` of
    newer transformers versions) and the denoising label table `label_enc.*` (a training device; inference never reads it).  The Swin tower's
    persistent `relative_position_index` buffers are checked against the computed ones by its own load hook.  Returns the form found."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        from anyedit_amd.cldm.model import load_state_dict
        sd = load_state_dict(sd, location)
    layout = "state_dict"
    if isinstance(sd.get("model"), dict):
        sd, layout = sd["model"], "checkpoint"
    if sd and all(k.startswith("module.") for k in sd):
        sd, layout = {k[len("module."):]: v for k, v in sd.items()}, layout + "-module"
    sd = {k: v for k, v in sd.items() if k not in GROUNDINGDINO_TOLERATED and not k.startswith(GROUNDINGDINO_TOLERATED_PREFIXES)}
    own = model.state_dict()
    missing = sorted(k for k in own if k not in sd)
    if missing:
        raise KeyError(f"load_groundingdino: {len(missing)} tensor(s) of the model are not in the checkpoint ({layout} form), first: '{missing[0]}'")
    unexpected = sorted(k for k in sd if k not in own)
    if unexpected:
        raise KeyError(f"load_groundingdino: {len(unexpected)} checkpoint tensor(s) have no place in the model ({layout} form), first: '{unexpected[0]}'")
    model.load_state_dict(sd, strict=True)
    return layout


HED_PREFIXES = ("module.", "netNetwork.")


def load_hed(model, path_or_state_dict, location="cpu"):
    """Fills a `hed.ControlNetHED_Apache2` (HED/__init__.py:57 `load_state_dict(torch.load(path))`) from a `ControlNetHED.pth` file or a state
    dict: `norm`, `blockN.convs.M.{weight,bias}`, `blockN.projection.{weight,bias}`, bare or with a `module.` or `netNetwork.` prefix on every
    key.  Strict: missing or unexpected keys are reported as `load_state_dict(strict=True)` reports them.  Returns the form found."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        from anyedit_amd.cldm.model import load_state_dict
        sd = load_state_dict(sd, location)
    layout = "state_dict"
    for pref in HED_PREFIXES:
        if sd and all(k.startswith(pref) for k in sd):
            sd, layout = {k[len(pref):]: v for k, v in sd.items()}, pref.rstrip(".")
            break
    model.load_state_dict(sd, strict=True)
    return layout


def load_depth_anything(model, path_or_state_dict, location="cpu"):
    """Fills a `depth_anything_v2.DepthAnythingV2` from a `depth_anything_v2_vit{s,b,l}.pth` file or a state dict: `pretrained.*` (the DINOv2 tower)
    and `depth_head.*`, bare or with a `module.` prefix on every key.  Strict: missing or unexpected keys are reported as
    `load_state_dict(strict=True)` reports them.  Returns the form found."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        from anyedit_amd.cldm.model import load_state_dict
        sd = load_state_dict(sd, location)
    layout = "state_dict"
    if sd and all(k.startswith("module.") for k in sd):
        sd, layout = {k[len("module."):]: v for k, v in sd.items()}, "module"
    model.load_state_dict(sd, strict=True)
    return layout


def load_uniformer(model, path_or_state_dict, location="cpu"):
    """Fills a `uniformer.UniFormer` from a file or a state dict in one of these forms: the bare backbone (`patch_embed1.proj.weight`, ...), or an
    mmseg segmentor checkpoint (`{"state_dict": ...}` or flat) whose `backbone.*` entries are taken and whose `decode_head.*` / `auxiliary_head.*`
    entries are skipped; a `module.` prefix on every key is accepted in either form.  Strict over the backbone's own keys: missing or unexpected
    ones are reported as `load_state_dict(strict=True)` reports them (`num_batches_tracked` is an ordinary BatchNorm buffer).  Returns the form
    found."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        from anyedit_amd.cldm.model import load_state_dict
        sd = load_state_dict(sd, location)
    if "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    layout = "state_dict"
    if sd and all(k.startswith("module.") for k in sd):
        sd, layout = {k[len("module."):]: v for k, v in sd.items()}, "module"
    if any(k.startswith("backbone.") for k in sd):
        other = [k for k in sd if not k.startswith(("backbone.", "decode_head.", "auxiliary_head."))]
        if other:
            raise KeyError(f"load_uniformer: a segmentor checkpoint with entries outside backbone / decode_head / auxiliary_head: {other[:4]}")
        sd, layout = {k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, layout + "+backbone"
    model.load_state_dict(sd, strict=True)
    return layout


def load_segmentor(model, path_or_state_dict, location="cpu"):
    """Fills a `uniformer.upernet.EncoderDecoder` from an mmseg segmentor checkpoint (`{"state_dict": ..., "meta": ...}` from a file or a dict, or a
    flat state dict), as `init_segmentor` does: strict over `backbone.*` and `decode_head.*` (missing or unexpected keys are reported as
    `load_state_dict(strict=True)` reports them); `auxiliary_head.*` entries, the FCN head that never runs at inference, are accepted and skipped; a
    `module.` prefix on every key is accepted.  `meta['CLASSES']` / `meta['PALETTE']` become `model.CLASSES` / `model.PALETTE` unless the model was
    built with `classes=` / `palette=`.  Returns the form found."""
    ck = path_or_state_dict
    if not isinstance(ck, dict):
        import torch
        ck = torch.load(ck, map_location=location, weights_only=False)      # `meta` is read too: load_state_dict would unwrap it away
    meta = ck.get("meta") if isinstance(ck.get("meta"), dict) else {}
    sd = ck["state_dict"] if "state_dict" in ck and isinstance(ck["state_dict"], dict) else {k: v for k, v in ck.items() if k != "meta"}
    layout = "state_dict"
    if sd and all(k.startswith("module.") for k in sd):
        sd, layout = {k[len("module."):]: v for k, v in sd.items()}, "module"
    other = [k for k in sd if not k.startswith(("backbone.", "decode_head.", "auxiliary_head."))]
    if other:
        raise KeyError(f"load_segmentor: entries outside backbone / decode_head / auxiliary_head: {other[:4]}")
    if any(k.startswith("auxiliary_head.") for k in sd):
        sd, layout = {k: v for k, v in sd.items() if not k.startswith("auxiliary_head.")}, layout + "-auxiliary_head"
    model.load_state_dict(sd, strict=True)
    if meta.get("CLASSES") is not None and not model._classes_override:
        model.CLASSES = list(meta["CLASSES"])
    if meta.get("PALETTE") is not None and not model._palette_override:
        model.set_palette(meta["PALETTE"])
    return layout


def load_sd_checkpoint(path, unet=None, vae=None, text_encoder=None, location="cpu"):
    """`load_unet_weights`' sibling for a FULL SD-1.5 state dict (CompVis lineage): routes `model.diffusion_model.*` to `unet`,
    `first_stage_model.*` to `vae` and `cond_stage_model.*` to `text_encoder` (a FrozenCLIPEmbedder); a part given as None is skipped.
    Returns the names of the parts that were filled."""
    from anyedit_amd.cldm.model import load_state_dict
    sd = load_state_dict(path, location)
    done = []
    for name, mod, pref in (("unet", unet, "model.diffusion_model."), ("vae", vae, "first_stage_model.")):
        if mod is None:
            continue
        own = [k for k in mod.state_dict().keys() if not k.startswith("loss.")]
        missing = [k for k in own if pref + k not in sd]
        if missing:
            raise KeyError(f"{name}: {len(missing)} tensors are not in the checkpoint under '{pref}' (e.g. '{missing[0]}')")
        mod.load_state_dict({k: sd[pref + k] for k in own}, strict=False)
        done.append(name)
    if text_encoder is not None:
        text_encoder.load_state_dict(text_encoder_state_dict(text_encoder, sd))
        done.append("text_encoder")
    return done
