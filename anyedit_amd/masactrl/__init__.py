"""MasaCtrl (mutual self-attention control) for the action-change edit pairs: the reference's `other_modules/masactrl` package on HIP."""
from .masactrl_utils import (AttentionBase, register_attention_editor_ldm, regiter_attention_editor_ldm, unregister_attention_editor_ldm,  # noqa: F401
                             unregister)
from .masactrl import MutualSelfAttentionControl, MutualSelfAttentionControlMask, MutualSelfAttentionControlMaskAuto  # noqa: F401
