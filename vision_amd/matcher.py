"""Ground-truth matching for detector training — host-side mirror of torchvision/models/detection/_utils.py `Matcher` on
`box_iou(gt, boxes)` as called per image by `RegionProposalNetwork.assign_targets_to_anchors` (rpn.py),
`RoIHeads.assign_targets_to_proposals` (roi_heads.py) and `RetinaNet.compute_loss` (retinanet.py).

The reference loops over the images in Python: per image a [G, A] IoU matrix, ~15-20 small launches and one host sync (the
`torch.where` of `set_low_quality_matches_`).  Here every image of the batch is matched by `tvmi::match_boxes`
(csrc/matcher.hip: a workspace clear and at most two launches, no host sync); the offsets come from host-known shapes.
"""
from typing import Dict, List, Sequence, Tuple

import torch
from torch import Tensor

from ._loader import load as _load
from .detection_post import _host_to_device


def _offsets(sizes: Sequence[int], device) -> Tensor:
    off = [0]
    for n in sizes:
        off.append(off[-1] + int(n))
    return _host_to_device(off, torch.int64, device)


def _cat(ts: Sequence[Tensor]) -> Tensor:
    return ts[0] if len(ts) == 1 else torch.cat(list(ts), 0)


def _match(gt_boxes: Sequence[Tensor], boxes: Sequence[Tensor], high: float, low: float, allow_low_quality: bool,
           gt_labels=None):
    """(matches, matched_gt, labels) over the concatenated batch, and the per-image box counts."""
    _load()
    if len(gt_boxes) != len(boxes):
        raise ValueError(f"match_boxes: {len(gt_boxes)} gt lists for {len(boxes)} box lists")
    if not len(boxes):
        raise ValueError("match_boxes: empty batch")
    gt2 = [g.reshape(-1, 4) for g in gt_boxes]
    n_box = [b.shape[0] for b in boxes]
    n_gt = [g.shape[0] for g in gt2]
    for nb, ng in zip(n_box, n_gt):
        if ng and not nb:  # Matcher.__call__ on a [G, 0] matrix
            raise ValueError("No proposal boxes available for one of the images during training")
    for t in list(gt_boxes) + list(boxes) + list(gt_labels or []):
        if not t.is_cuda:
            raise RuntimeError("vision_amd.match_boxes needs device tensors (no CPU fallback in the product path)")
    dev = boxes[0].device
    labels = None if gt_labels is None else _cat([lb.reshape(-1).to(torch.int64) for lb in gt_labels])
    matches, matched_gt, lab = torch.ops.tvmi.match_boxes(
        _cat(list(boxes)), _offsets(n_box, dev), _cat(gt2), _offsets(n_gt, dev), labels, float(high), float(low),
        bool(allow_low_quality))
    return matches, matched_gt, lab, n_box


def match_boxes(gt_boxes: List[Tensor], boxes: List[Tensor], high: float, low: float,
                allow_low_quality: bool = False) -> List[Tensor]:
    """Per image i: `Matcher(high, low, allow_low_quality)(box_iou(gt_boxes[i], boxes[i]))`, int64 [n_i] (a gt index,
    -1 below `low`, -2 in [low, high)), and -1 everywhere for an image without gt (RetinaNet's convention).  float32 device
    tensors; one launch sequence for the batch, no host sync."""
    matches, _, _, n_box = _match(gt_boxes, boxes, high, low, allow_low_quality)
    return list(matches.split(n_box, 0))


def rpn_assign_targets(anchors: List[Tensor], targets: List[Dict[str, Tensor]], high: float = 0.7, low: float = 0.3,
                       allow_low_quality_matches: bool = True) -> Tuple[List[Tensor], List[Tensor]]:
    """rpn.py RegionProposalNetwork.assign_targets_to_anchors: per image, float32 labels (1 matched, 0 background, -1
    between the thresholds) and the matched gt boxes (zeros for an image without gt)."""
    matches, matched_gt, _, n_box = _match([t["boxes"] for t in targets], anchors, high, low, allow_low_quality_matches)
    labels = (matches >= 0).to(torch.float32) - (matches == -2).to(torch.float32)
    return list(labels.split(n_box, 0)), list(matched_gt.split(n_box, 0))


def roi_heads_assign_targets(proposals: List[Tensor], gt_boxes: List[Tensor], gt_labels: List[Tensor], high: float = 0.5,
                             low: float = 0.5, allow_low_quality_matches: bool = False) -> Tuple[List[Tensor], List[Tensor]]:
    """roi_heads.py RoIHeads.assign_targets_to_proposals: per image, the clamped matched gt indices and the int64 labels
    (the gt's label, 0 background, -1 between the thresholds; index 0 and label 0 for an image without gt)."""
    matches, _, labels, n_box = _match(gt_boxes, proposals, high, low, allow_low_quality_matches, gt_labels=gt_labels)
    return list(matches.clamp(min=0).split(n_box, 0)), list(labels.split(n_box, 0))
