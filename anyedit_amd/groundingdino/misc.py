"""GroundingDINO/groundingdino/util/misc.py:151-190 NestedTensor, as far as the backbone needs it: a batch of images with its padding mask
(True where a pixel is padding)."""


class NestedTensor:
    def __init__(self, tensors, mask):
        self.tensors = tensors
        self.mask = mask

    def to(self, device):
        mask = self.mask.to(device) if self.mask is not None else None
        return NestedTensor(self.tensors.to(device), mask)

    def decompose(self):
        return self.tensors, self.mask

    def __repr__(self):
        return str(self.tensors)
