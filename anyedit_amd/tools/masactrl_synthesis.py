"""Action-change image pairs: mirror of `consistent_synthesis` (AnyEdit_Collection/adaptive_editing_pipelines/action_change_tool.py:15-45) on the
latent-diffusion model and DDIM sampler of this package.

The reference draws one start code, expands it over the (source, target) prompts, registers a MutualSelfAttentionControl(step, layer) on the
pipeline's UNet and samples with classifier-free guidance.  Here the editor is registered on `model.model.diffusion_model`
(anyedit_amd.masactrl.register_attention_editor_ldm) and `DDIMSampler.sample` runs with `unconditional_conditioning`: its `[uncond, cond]` batch
(ddim.py:156-171) is the `[u_s, u_t, c_s, c_t]` order the editors assume.  Eager only: an editor counts attention calls on the host, so the
sampling loop must not be captured into a graph across the start step."""
import torch

from anyedit_amd.masactrl import MutualSelfAttentionControl, register_attention_editor_ldm, unregister_attention_editor_ldm


@torch.no_grad()
def consistent_synthesis(model, sampler, prompts, start_code=None, step=4, layer=10, guidance_scale=7.5, steps=50, editor=None):
    """model: a LatentDiffusion (get_learned_conditioning, decode_first_stage, model.diffusion_model); sampler: a DDIMSampler on it; prompts:
    [source prompt, target prompt].  start_code: [1, C, h, w] latent noise (default: a fresh 1 x 4 x 64 x 64 draw), expanded over the prompts.
    editor: an AttentionBase of anyedit_amd.masactrl (default MutualSelfAttentionControl(step, layer, total_steps=steps)); it is reset, registered
    for the run and unregistered afterwards.  Returns the decoded images, [len(prompts), 3, H, W]."""
    prompts = list(prompts)
    n = len(prompts)
    if n < 2:
        raise ValueError("consistent_synthesis: needs the source prompt and at least one target prompt")
    device = next(model.parameters()).device
    if start_code is None:
        start_code = torch.randn(1, 4, 64, 64, device=device)
    if start_code.dim() != 4 or start_code.shape[0] != 1:
        raise ValueError(f"consistent_synthesis: start_code must be [1, C, h, w], got {tuple(start_code.shape)}")
    start_code = start_code.to(device).expand(n, -1, -1, -1).contiguous()
    if editor is None:
        editor = MutualSelfAttentionControl(step, layer, total_steps=steps)
    editor.reset()
    register_attention_editor_ldm(model, editor)
    try:
        cond = model.get_learned_conditioning(prompts)
        uncond = model.get_learned_conditioning([""] * n)
        samples, _ = sampler.sample(steps, n, tuple(start_code.shape[1:]), cond, eta=0.0, x_T=start_code, verbose=False,
                                    unconditional_guidance_scale=guidance_scale, unconditional_conditioning=uncond)
        return model.decode_first_stage(samples)
    finally:
        unregister_attention_editor_ldm(model)
