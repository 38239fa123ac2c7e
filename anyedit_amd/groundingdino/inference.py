"""Grounded boxes from the detector: GroundingDINO/groundingdino/util/inference.py:21-25 (`preprocess_caption`), util/utils.py:599-608
(`get_phrases_from_posmap`) and AnyEdit_Collection/adaptive_editing_pipelines/tools/tool.py:104-147 (`load_sam_image_from_Image`,
`get_grounding_output`).

tool.py:125-133 copies the [nq, 256] logits to the host, takes the sigmoid and filters there.  Here the filter is `ops.gdino_ground`: the GPU
compacts the kept queries in query order with their score, box and token bit set, and the host reads `count` and those rows in one
synchronisation; the logits are never copied.  `GroundingDetector(model)` is the `det_model(image_pil, det_prompt, box_threshold, text_threshold)`
callable that `anyedit_amd.tools.tool.maskgeneration` takes.
"""
import numpy as np
import torch

from anyedit_amd import ops

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def preprocess_caption(caption):
    """inference.py:21-25 / tool.py:117-120."""
    result = caption.lower().strip()
    return result if result.endswith(".") else result + "."


def resized_size(w, h, size=800, max_size=1333):
    """datasets/transforms.py:89-107 (`get_size_with_aspect_ratio`): the (height, width) `RandomResize([800], max_size=1333)` gives a w x h image."""
    if max_size is not None:
        mn, mx = float(min(w, h)), float(max(w, h))
        if mx / mn * size > max_size:
            size = int(round(max_size * mn / mx))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def load_image_tensor(image_pil):
    """tool.py:104-114: shorter side to 800 (longer at most 1333, PIL bilinear), ToTensor, Normalize with the ImageNet constants -> fp32 [3, h, w]."""
    from PIL import Image
    image_pil = image_pil.convert("RGB")
    oh, ow = resized_size(*image_pil.size)
    if (ow, oh) != image_pil.size:
        image_pil = image_pil.resize((ow, oh), Image.BILINEAR)
    x = torch.from_numpy(np.asarray(image_pil, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255.0)
    mean, std = torch.tensor(IMAGENET_MEAN).view(3, 1, 1), torch.tensor(IMAGENET_STD).view(3, 1, 1)
    return (x - mean) / std


def get_phrases_from_posmap(posmap, tokenized, tokenizer):
    """utils.py:599-608: the decoded tokens a 1-d bool posmap selects."""
    assert isinstance(posmap, torch.Tensor), "posmap must be torch.Tensor"
    if posmap.dim() != 1:
        raise NotImplementedError("posmap must be 1-dim")
    non_zero_idx = posmap.nonzero(as_tuple=True)[0].tolist()
    token_ids = [tokenized["input_ids"][i] for i in non_zero_idx]
    return tokenizer.decode(token_ids)


def format_phrase(phrase, score, with_logits=True):
    """tool.py:142-145: the phrase with the first four characters of the score."""
    return phrase + f"({str(score)[:4]})" if with_logits else phrase


def posmaps_from_bits(bits, T):
    """int32 [n, T // 32] token bit sets (`ops.gdino_ground`) -> bool [n, T]"""
    b = bits.to(torch.int64) & 0xFFFFFFFF
    return ((b[:, :, None] >> torch.arange(32, device=bits.device)) & 1).bool().reshape(bits.shape[0], -1)[:, :T]


def ground_outputs(pred_logits, pred_boxes, box_threshold, text_threshold):
    """`ops.gdino_ground` on a batch and its read-back: per image (kept query indices long [n], scores fp32 [n], boxes fp32 [n, 4], posmaps bool
    [n, T]) on the CPU.  One host synchronisation; [B, nq, 14] words cross, not the logits."""
    count, idx, scores, boxes, bits = ops.gdino_ground(pred_logits.contiguous(), pred_boxes.contiguous(), box_threshold, text_threshold)
    host = [t.to("cpu", non_blocking=True) for t in (count, idx, scores, boxes, bits)]
    torch.cuda.current_stream().synchronize()
    count, idx, scores, boxes, bits = host
    T = pred_logits.shape[-1]
    out = []
    for b in range(pred_logits.shape[0]):
        n = int(count[b])
        out.append((idx[b, :n].long(), scores[b, :n].clone(), boxes[b, :n].clone(), posmaps_from_bits(bits[b, :n], T)))
    return out


def get_grounding_output(model, image, caption, box_threshold, text_threshold, with_logits=True, device="cuda"):
    """tool.py:116-147.  image: fp32 [3, h, w] (`load_image_tensor`).  Returns (boxes_filt fp32 [n, 4] on the CPU as (cx, cy, w, h) in [0, 1],
    pred_phrases)."""
    caption = preprocess_caption(caption)
    model = model.to(device)
    image = image.to(device)
    with torch.no_grad():
        outputs = model(image[None], captions=[caption])
    _, scores, boxes_filt, posmaps = ground_outputs(outputs["pred_logits"], outputs["pred_boxes"], box_threshold, text_threshold)[0]
    tokenizer = model.tokenizer
    tokenized = tokenizer(caption)
    pred_phrases = [format_phrase(get_phrases_from_posmap(pm, tokenized, tokenizer), s.item(), with_logits) for pm, s in zip(posmaps, scores)]
    return boxes_filt, pred_phrases


class GroundingDetector:
    """`det_model(image_pil, det_prompt, box_threshold, text_threshold) -> (boxes_filt, pred_phrases)` for `tools.tool.maskgeneration`
    (tool.py:166-269 makes it from `load_sam_image_from_Image` and `get_grounding_output`)."""

    def __init__(self, model, device="cuda"):
        self.model, self.device = model.to(device).eval(), device

    def __call__(self, image_pil, det_prompt, box_threshold=0.25, text_threshold=0.25, with_logits=True):
        return get_grounding_output(self.model, load_image_tensor(image_pil), det_prompt, box_threshold, text_threshold, with_logits, self.device)
