"""Keypoint post-processing — host-side mirror of torchvision/models/detection/roi_heads.py
(`heatmaps_to_keypoints`, `keypointrcnn_inference`).

Both keep the reference's names, arguments and results, but decode every detection of the batch with
`tvmi::heatmaps_to_keypoints` (csrc/keypoints.hip: three launches, no host sync) instead of the reference's
per-detection loop of `.item()` + bicubic `F.interpolate` + `argmax` + indexing.
"""
from typing import List, Tuple

import torch
from torch import Tensor

from ._loader import load as _load


def heatmaps_to_keypoints(maps: Tensor, rois: Tensor) -> Tuple[Tensor, Tensor]:
    """maps [R,K,H,W] (float32 / float16 / bfloat16), rois [R,4] xyxy -> keypoints [R,K,3] (x, y, 1), scores [R,K].

    Device tensors only: the product path is the HIP kernel and there is no CPU fallback."""
    _load()
    if not (maps.is_cuda and rois.is_cuda):
        raise RuntimeError("vision_amd.heatmaps_to_keypoints needs device tensors (no CPU fallback in the product path)")
    return torch.ops.tvmi.heatmaps_to_keypoints(maps, rois)


def keypointrcnn_inference(x: Tensor, boxes: List[Tensor]) -> Tuple[List[Tensor], List[Tensor]]:
    """roi_heads.py keypointrcnn_inference: x [sum(n_i),K,H,W] keypoint logits, boxes[i] [n_i,4] -> per-image
    keypoints [n_i,K,3] and scores [n_i,K].  One launch sequence for the whole batch; the split sizes are host-known."""
    boxes_per_image = [b.size(0) for b in boxes]
    rois = torch.cat(list(boxes), 0) if len(boxes) != 1 else boxes[0]
    kp, scores = heatmaps_to_keypoints(x, rois)
    return list(kp.split(boxes_per_image, 0)), list(scores.split(boxes_per_image, 0))
