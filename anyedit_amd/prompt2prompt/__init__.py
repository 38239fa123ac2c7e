from . import ptp_utils, seq_aligner  # noqa: F401
from .ptp_utils import register_attention_control, unregister, text2image_ldm_stable  # noqa: F401
from .prompt_to_prompt_stable import (LocalBlend, AttentionControl, EmptyControl, AttentionStore, AttentionControlEdit, AttentionReplace,  # noqa: F401
                                      AttentionRefine, AttentionReweight, get_equalizer, aggregate_attention, mask_from_CA)
