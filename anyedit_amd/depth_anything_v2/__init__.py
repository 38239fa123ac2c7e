"""Depth Anything V2 (AnyEdit_Collection/other_modules/depth_anything_v2) on HIP: the DINOv2 tower of ldm/modules/encoders/dino_vision.py under the DPT
head of dpt.py.  The annotator of the `visual_depth` condition (tools.tool.img2depth)."""
from anyedit_amd.depth_anything_v2.dpt import (DepthAnythingV2, DPTHead, FeatureFusionBlock, ResidualConvUnit, ENCODERS, get_size,  # noqa: F401
                                               spectral_r_table)
