"""Mirror of AnyEdit_Collection/other_modules/masactrl/masactrl_utils.py on the HIP attention operators.

The reference swaps `CrossAttention.forward` for a closure that materialises sim and attn ([B h, N, N]) and hands them to the editor
(masactrl_utils.py:151-193).  Here `CrossAttention.rows` consults an `editor` attribute instead and hands it the projected operands in place
(the packed [B N, 3 inner] projection of a self-attention, the q rows and the cached K|V rows of a cross-attention) together with `core`, the
launches it would issue without an editor; an editor replaces only the attention core, so the LayerNorm folds, row statistics and `kv_cache`
around it run as they do without one.  Not built: AttentionStore and the diffusers registration (masactrl_utils.py:43-144)."""


class AttentionBase:
    """masactrl_utils.py:14-40.  Every CrossAttention call counts, self and cross; `cur_att_layer // 2` is the transformer block's index."""

    def __init__(self):
        self.cur_step = 0
        self.num_att_layers = -1
        self.cur_att_layer = 0

    def after_step(self):
        pass

    def __call__(self, attn, is_cross, B, N, core, **operands):
        out = self.forward(attn, is_cross, B, N, core, **operands)
        self.cur_att_layer += 1
        if self.cur_att_layer == self.num_att_layers:
            self.cur_att_layer = 0
            self.cur_step += 1
            self.after_step()
        return out

    def forward(self, attn, is_cross, B, N, core, **operands):
        """attn: the CrossAttention module; core(): the uncontrolled attention, [B, N, inner] bf16.  Self-attention: operands = {qkv}; cross:
        {q, kv, Nk}."""
        return core()

    def reset(self):
        self.cur_step = 0
        self.cur_att_layer = 0


def _attention_modules(model):
    from anyedit_amd.ldm.modules.attention import CrossAttention
    unet = model.model.diffusion_model
    mods = []
    for name, net in unet.named_children():          # masactrl_utils.py:205-211: the input, middle and output blocks
        if "input" in name or "middle" in name or "output" in name:
            mods += [m for m in net.modules() if isinstance(m, CrossAttention)]
    return mods


def register_attention_editor_ldm(model, editor):
    """masactrl_utils.py:147-212: every CrossAttention under model.model.diffusion_model consults `editor`; editor.num_att_layers = their number."""
    mods = _attention_modules(model)
    for m in mods:
        m.editor = editor
    editor.num_att_layers = len(mods)
    return editor


regiter_attention_editor_ldm = register_attention_editor_ldm   # the reference's spelling


def unregister_attention_editor_ldm(model):
    """Removes the attribute: the modules issue exactly the launches of a model that never had an editor.  Returns how many had one."""
    n = 0
    for m in _attention_modules(model):
        if "editor" in m.__dict__:
            del m.__dict__["editor"]
            n += 1
    return n


unregister = unregister_attention_editor_ldm
