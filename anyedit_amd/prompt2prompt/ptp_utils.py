"""Mirror of AnyEdit_Collection/other_modules/prompt2prompt/ptp_utils.py on the latent-diffusion model and the HIP attention operators.

The reference swaps every attention module's `forward` for a closure that materialises attention_probs ([B h, N, 77]) and hands it to the
controller (ptp_utils.py:175-273).  Here `CrossAttention.rows` consults the same `editor` attribute that MasaCtrl uses: registration stores a
small per-module adapter there that binds the module's place name ("down" / "mid" / "up" for input_blocks / middle_block / output_blocks) and
calls `controller(attn_module, is_cross, place, B, N, core, **operands)` with the projected operands in place and `core`, the launches of the
uncontrolled attention.  `text2image_ldm_stable` runs its own loop over `DDIMSampler.p_sample_ddim` and applies `controller.step_callback` after
every step (ptp_utils.py:65-78); the sampler itself is unchanged.  Eager only: a controller counts attention calls and steps on the host and its
gates open and close between steps, so the loop must not be captured into a graph.

The tokenizer is passed in wherever the reference reads its module-level global.  Not built: LOW_RESOURCE, the diffusers registration,
text2image_ldm (the BERT-conditioned variant), text_under_image / view_images and the other image helpers, graph capture across steps."""
import numpy as np
import torch

from .seq_aligner import get_word_inds  # noqa: F401  (ptp_utils.py:276-294 is the same function)

_PLACES = (("input_blocks", "down"), ("middle_block", "mid"), ("output_blocks", "up"))


def update_alpha_time_word(alpha, bounds, prompt_ind, word_inds=None):
    """ptp_utils.py:297-309: alpha[start:end, prompt_ind, word_inds] = 1 and 0 outside, with (start, end) = int(bounds * steps)"""
    if type(bounds) is float:
        bounds = 0, bounds
    start, end = int(bounds[0] * alpha.shape[0]), int(bounds[1] * alpha.shape[0])
    if word_inds is None:
        word_inds = torch.arange(alpha.shape[2])
    alpha[:start, prompt_ind, word_inds] = 0
    alpha[start:end, prompt_ind, word_inds] = 1
    alpha[end:, prompt_ind, word_inds] = 0
    return alpha


def get_time_words_attention_alpha(prompts, num_steps, cross_replace_steps, tokenizer, max_num_words=77):
    """ptp_utils.py:312-330: fp32 [num_steps + 1, len(prompts) - 1, 1, 1, max_num_words]"""
    if type(cross_replace_steps) is not dict:
        cross_replace_steps = {"default_": cross_replace_steps}
    if "default_" not in cross_replace_steps:
        cross_replace_steps["default_"] = (0., 1.)
    alpha = torch.zeros(num_steps + 1, len(prompts) - 1, max_num_words)
    for i in range(len(prompts) - 1):
        alpha = update_alpha_time_word(alpha, cross_replace_steps["default_"], i)
    for key, item in cross_replace_steps.items():
        if key == "default_":
            continue
        inds = [get_word_inds(prompts[i], key, tokenizer) for i in range(1, len(prompts))]
        for i, ind in enumerate(inds):
            if len(ind) > 0:
                alpha = update_alpha_time_word(alpha, item, i, ind)
    return alpha.reshape(num_steps + 1, len(prompts) - 1, 1, 1, max_num_words)


class _PlacedEditor:
    """What `CrossAttention.rows` finds as `editor`: the controller with the module's place name bound at registration"""

    def __init__(self, controller, place):
        self.controller, self.place = controller, place

    def __call__(self, attn, is_cross, B, N, core, **operands):
        return self.controller(attn, is_cross, self.place, B, N, core, **operands)


class _DummyController:
    """ptp_utils.py:243-249: registration with controller=None"""
    num_att_layers = 0

    def __call__(self, attn, is_cross, place, B, N, core, **operands):
        return core()


def _placed_modules(model):
    from anyedit_amd.ldm.modules.attention import CrossAttention
    unet = model.model.diffusion_model
    out = []
    for name, net in unet.named_children():
        for key, place in _PLACES:
            if key in name:
                out += [(m, place) for m in net.modules() if isinstance(m, CrossAttention)]
    return out


def register_attention_control(model, controller):
    """ptp_utils.py:175-273 on model.model.diffusion_model: every CrossAttention module consults the controller; controller.num_att_layers = their
    number.  Returns the controller."""
    if controller is None:
        controller = _DummyController()
    mods = _placed_modules(model)
    for m, place in mods:
        m.editor = _PlacedEditor(controller, place)
    controller.num_att_layers = len(mods)
    return controller


def unregister(model):
    """Removes the attribute: the modules issue exactly the launches of a model that never had a controller.  Returns how many had one."""
    n = 0
    for m, _ in _placed_modules(model):
        if "editor" in m.__dict__:
            del m.__dict__["editor"]
            n += 1
    return n


@torch.no_grad()
def text2image_ldm_stable(model, sampler, prompts, controller, num_inference_steps=50, guidance_scale=7.5, latent=None, decode=True):
    """ptp_utils.py:131-172 on a LatentDiffusion `model` (get_learned_conditioning, decode_first_stage) and a DDIMSampler on it: the controller is
    registered for the run, one latent ([1, C, h, w]; default a fresh 1 x 4 x 64 x 64 draw) is expanded over the prompts, every step is one
    `p_sample_ddim` with classifier-free guidance on the [uncond, cond] batch followed by `controller.step_callback(latents)`.  Returns
    (images as uint8 [n, H, W, 3] numpy, or the final latents with decode=False; the start latent)."""
    prompts = list(prompts)
    n = len(prompts)
    device = next(model.parameters()).device
    if latent is None:
        latent = torch.randn(1, 4, 64, 64, device=device)
    if latent.dim() != 4 or latent.shape[0] != 1:
        raise ValueError(f"text2image_ldm_stable: latent must be [1, C, h, w], got {tuple(latent.shape)}")
    latents = latent.to(device).float().expand(n, -1, -1, -1).contiguous()
    if controller is not None and hasattr(controller, "reset"):
        controller.reset()
    register_attention_control(model, controller)
    try:
        cond = model.get_learned_conditioning(prompts)
        uncond = model.get_learned_conditioning([""] * n)
        sampler.make_schedule(ddim_num_steps=num_inference_steps, ddim_eta=0.0, verbose=False)
        steps = np.flip(sampler.ddim_timesteps)
        for i, step in enumerate(steps):
            index = len(steps) - i - 1
            ts = torch.full((n,), int(step), device=device, dtype=torch.long)
            latents, _ = sampler.p_sample_ddim(latents, cond, ts, index=index, unconditional_guidance_scale=guidance_scale,
                                               unconditional_conditioning=uncond)
            if controller is not None:
                latents = controller.step_callback(latents)
    finally:
        unregister(model)
    if not decode:
        return latents, latent
    image = model.decode_first_stage(latents)
    image = (image / 2 + 0.5).clamp(0, 1)
    image = (image.float().cpu().permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8)
    return image, latent
