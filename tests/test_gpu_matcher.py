"""Batched ground-truth matching (`vision_amd.match_boxes` / `rpn_assign_targets` / `roi_heads_assign_targets`,
csrc/matcher.hip) against the reference's per-image loop (torchvision 0.30), restated here as torch ops on the device:

  ops/boxes.py box_iou(gt, boxes) -> [G, N]; models/detection/_utils.py Matcher(high, low, allow_low_quality)
  rpn.py RegionProposalNetwork.assign_targets_to_anchors, roi_heads.py RoIHeads.assign_targets_to_proposals,
  retinanet.py RetinaNet.compute_loss (the matched_idxs it hands to head.compute_loss)

Every comparison is exact: matches, labels and matched gt boxes.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ---- the reference, restated
def box_iou(boxes1, boxes2):
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    lt = torch.max(boxes1[:, None, :2], boxes2[:, :2])
    rb = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    union = area1[:, None] + area2 - inter
    return inter / union


box_iou.__module__ = "torchvision.ops.boxes"  # what the integration wrappers recognise as the reference's similarity


class Matcher:
    BELOW_LOW_THRESHOLD = -1
    BETWEEN_THRESHOLDS = -2

    def __init__(self, high_threshold, low_threshold, allow_low_quality_matches=False):
        assert low_threshold <= high_threshold
        self.high_threshold = high_threshold
        self.low_threshold = low_threshold
        self.allow_low_quality_matches = allow_low_quality_matches

    def __call__(self, match_quality_matrix):
        if match_quality_matrix.numel() == 0:
            if match_quality_matrix.shape[0] == 0:
                raise ValueError("No ground-truth boxes available for one of the images during training")
            raise ValueError("No proposal boxes available for one of the images during training")
        matched_vals, matches = match_quality_matrix.max(dim=0)
        all_matches = matches.clone() if self.allow_low_quality_matches else None
        below_low_threshold = matched_vals < self.low_threshold
        between_thresholds = (matched_vals >= self.low_threshold) & (matched_vals < self.high_threshold)
        matches[below_low_threshold] = self.BELOW_LOW_THRESHOLD
        matches[between_thresholds] = self.BETWEEN_THRESHOLDS
        if self.allow_low_quality_matches:
            highest_quality_foreach_gt, _ = match_quality_matrix.max(dim=1)
            pairs = torch.where(match_quality_matrix == highest_quality_foreach_gt[:, None])
            matches[pairs[1]] = all_matches[pairs[1]]
        return matches


class RegionProposalNetwork(torch.nn.Module):
    def __init__(self, high=0.7, low=0.3):
        super().__init__()
        self.proposal_matcher = Matcher(high, low, allow_low_quality_matches=True)
        self.box_similarity = box_iou

    def assign_targets_to_anchors(self, anchors, targets):
        labels, matched_gt_boxes = [], []
        for anchors_per_image, targets_per_image in zip(anchors, targets):
            gt_boxes = targets_per_image["boxes"]
            if gt_boxes.numel() == 0:
                device = anchors_per_image.device
                matched_gt_boxes_per_image = torch.zeros(anchors_per_image.shape, dtype=torch.float32, device=device)
                labels_per_image = torch.zeros((anchors_per_image.shape[0],), dtype=torch.float32, device=device)
            else:
                match_quality_matrix = self.box_similarity(gt_boxes, anchors_per_image)
                matched_idxs = self.proposal_matcher(match_quality_matrix)
                matched_gt_boxes_per_image = gt_boxes[matched_idxs.clamp(min=0)]
                labels_per_image = (matched_idxs >= 0).to(dtype=torch.float32)
                labels_per_image[matched_idxs == self.proposal_matcher.BELOW_LOW_THRESHOLD] = 0.0
                labels_per_image[matched_idxs == self.proposal_matcher.BETWEEN_THRESHOLDS] = -1.0
            labels.append(labels_per_image)
            matched_gt_boxes.append(matched_gt_boxes_per_image)
        return labels, matched_gt_boxes


class RoIHeads(torch.nn.Module):
    def __init__(self, high=0.5, low=0.5):
        super().__init__()
        self.proposal_matcher = Matcher(high, low, allow_low_quality_matches=False)
        self.box_similarity = box_iou

    def assign_targets_to_proposals(self, proposals, gt_boxes, gt_labels):
        matched_idxs, labels = [], []
        for proposals_in_image, gt_boxes_in_image, gt_labels_in_image in zip(proposals, gt_boxes, gt_labels):
            if gt_boxes_in_image.numel() == 0:
                device = proposals_in_image.device
                clamped = torch.zeros((proposals_in_image.shape[0],), dtype=torch.int64, device=device)
                labels_in_image = torch.zeros((proposals_in_image.shape[0],), dtype=torch.int64, device=device)
            else:
                match_quality_matrix = box_iou(gt_boxes_in_image, proposals_in_image)
                matched_idxs_in_image = self.proposal_matcher(match_quality_matrix)
                clamped = matched_idxs_in_image.clamp(min=0)
                labels_in_image = gt_labels_in_image[clamped].to(dtype=torch.int64)
                labels_in_image[matched_idxs_in_image == self.proposal_matcher.BELOW_LOW_THRESHOLD] = 0
                labels_in_image[matched_idxs_in_image == self.proposal_matcher.BETWEEN_THRESHOLDS] = -1
            matched_idxs.append(clamped)
            labels.append(labels_in_image)
        return matched_idxs, labels


class _Head:
    def compute_loss(self, targets, head_outputs, anchors, matched_idxs):
        return matched_idxs


class RetinaNet(torch.nn.Module):
    def __init__(self, high=0.5, low=0.4):
        super().__init__()
        self.proposal_matcher = Matcher(high, low, allow_low_quality_matches=True)
        self.head = _Head()

    def compute_loss(self, targets, head_outputs, anchors):
        matched_idxs = []
        for anchors_per_image, targets_per_image in zip(anchors, targets):
            if targets_per_image["boxes"].numel() == 0:
                matched_idxs.append(torch.full((anchors_per_image.size(0),), -1, dtype=torch.int64,
                                               device=anchors_per_image.device))
                continue
            match_quality_matrix = box_iou(targets_per_image["boxes"], anchors_per_image)
            matched_idxs.append(self.proposal_matcher(match_quality_matrix))
        return self.head.compute_loss(targets, head_outputs, anchors, matched_idxs)


def reference_matches(gt, boxes, high, low, allow):
    return [torch.full((b.shape[0],), -1, dtype=torch.int64, device=b.device) if g.numel() == 0
            else Matcher(high, low, allow)(box_iou(g, b)) for g, b in zip(gt, boxes)]


# ---- inputs
def _boxes(n, g, W=1344.0, H=800.0, smin=8.0, smax=512.0):
    c = torch.rand(n, 2, generator=g) * torch.tensor([W, H])
    s = smin * (smax / smin) ** torch.rand(n, 1, generator=g)
    ar = 2.0 ** (2 * torch.rand(n, 1, generator=g) - 1)
    wh = torch.cat([s * ar.sqrt(), s / ar.sqrt()], 1)
    return torch.cat([c - wh / 2, c + wh / 2], 1)


def _anchors(A, g):
    """An FPN-like anchor set: a regular grid of centres with three sizes and three aspect ratios per level, cut to A."""
    out = []
    for stride, size in ((4, 32), (8, 64), (16, 128), (32, 256), (64, 512)):
        ys, xs = torch.meshgrid(torch.arange(0, 800, stride, dtype=torch.float32),
                                torch.arange(0, 1344, stride, dtype=torch.float32), indexing="ij")
        ctr = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)
        for ar in (0.5, 1.0, 2.0):
            w, h = size / ar ** 0.5, size * ar ** 0.5
            out.append(torch.cat([ctr - torch.tensor([w / 2, h / 2]), ctr + torch.tensor([w / 2, h / 2])], 1))
    a = torch.cat(out)
    a = a[torch.randperm(a.shape[0], generator=g)[:A]] if A <= a.shape[0] else torch.cat([a, _boxes(A - a.shape[0], g)])
    return a.round()  # anchors in the reference are rounded to integers


def _check_all(gt, boxes, labels_list, rpn=(0.7, 0.3), roi=(0.5, 0.5), retina=(0.5, 0.4)):
    import vision_amd

    targets = [{"boxes": g, "labels": lb} for g, lb in zip(gt, labels_list)]
    rl, rg = RegionProposalNetwork(*rpn).assign_targets_to_anchors(boxes, targets)
    fl, fg = vision_amd.rpn_assign_targets(boxes, targets, *rpn)
    assert len(fl) == len(rl) == len(fg) == len(rg)
    for a, b in zip(fl, rl):
        assert a.dtype == b.dtype and torch.equal(a, b)
    for a, b in zip(fg, rg):
        assert a.dtype == b.dtype and torch.equal(a, b)
    ri, rlb = RoIHeads(*roi).assign_targets_to_proposals(boxes, gt, labels_list)
    fi, flb = vision_amd.roi_heads_assign_targets(boxes, gt, labels_list, *roi)
    for a, b in zip(fi + flb, ri + rlb):
        assert a.dtype == b.dtype and torch.equal(a, b)
    for allow in (True, False):
        ref = reference_matches(gt, boxes, *retina, allow)
        got = vision_amd.match_boxes(gt, boxes, *retina, allow)
        for a, b in zip(got, ref):
            assert a.dtype == b.dtype and torch.equal(a, b)


def _labels(gt, g):
    return [torch.randint(1, 91, (t.shape[0],), generator=g).to(DEV) for t in gt]


@pytest.mark.parametrize("B", [1, 2, 8])
def test_rpn_sized_batches(B):
    g = torch.Generator().manual_seed(100 + B)
    A = 268_569
    anchors = _anchors(A, g).to(DEV)
    counts = [int(torch.randint(0, 61, (1,), generator=g)) for _ in range(B)]
    counts[0] = max(counts[0], 1)
    if B > 1:
        counts[1] = 0  # an image without gt
        counts[-1] = 60
    gt = [_boxes(n, g).to(DEV) for n in counts]
    boxes = [anchors] * B
    _check_all(gt, boxes, _labels(gt, g))


@pytest.mark.parametrize("B", [1, 3, 8])
def test_roi_heads_sized_batches_with_ragged_proposals(B):
    g = torch.Generator().manual_seed(200 + B)
    gt = [_boxes(int(torch.randint(0, 40, (1,), generator=g)), g).to(DEV) for _ in range(B)]
    # RoIHeads appends the gt to the proposals (add_gt_proposals): 2000 + G per image, then ragged counts
    boxes = [torch.cat([_boxes(2000 - 37 * i, g).to(DEV), t]) for i, t in enumerate(gt)]
    _check_all(gt, boxes, _labels(gt, g))


def test_sizes_not_a_multiple_of_the_block():
    g = torch.Generator().manual_seed(3)
    for ns in ((1,), (255, 257), (1023, 1, 1025, 3), (4097,)):
        gt = [_boxes(5, g).to(DEV) for _ in ns]
        boxes = [torch.cat([_boxes(n - min(n, 3), g), gt[i][: min(n, 3)].cpu()]).to(DEV) for i, n in enumerate(ns)]
        _check_all(gt, boxes, _labels(gt, g))


def test_many_gt_boxes_take_the_chunk_loop():
    g = torch.Generator().manual_seed(4)
    gt = [_boxes(3000, g, smin=16, smax=256).to(DEV), _boxes(1500, g).to(DEV)]
    boxes = [_boxes(700, g, smin=16, smax=256).to(DEV), _boxes(300, g).to(DEV)]
    _check_all(gt, boxes, _labels(gt, g))


def test_duplicate_gt_boxes_tie_to_the_lowest_index():
    import vision_amd

    g = torch.Generator().manual_seed(5)
    base = _boxes(6, g)
    gt = torch.cat([base[3:4], base[:3], base[3:4], base[1:2]]).to(DEV)  # 0 == 4, 2 == 5
    boxes = torch.cat([base, _boxes(500, g)]).to(DEV)
    _check_all([gt], [boxes], _labels([gt], g))
    m = vision_amd.match_boxes([gt], [boxes], 0.7, 0.3, True)[0]
    assert m[3] == 0 and m[1] == 2  # the first of the duplicates


def test_iou_exactly_at_the_thresholds():
    import vision_amd

    gt = torch.tensor([[0.0, 0.0, 10.0, 10.0]], device=DEV)
    boxes = torch.tensor([[0.0, 0.0, 10.0, 5.0],     # IoU 0.5 exactly
                          [0.0, 0.0, 10.0, 7.0],     # IoU 0.7f, which is below the double 0.7
                          [0.0, 0.0, 10.0, 3.0],     # IoU 0.3f
                          [0.0, 0.0, 10.0, 2.0]], device=DEV)
    iou = box_iou(gt, boxes)[0]
    assert iou[0].item() == 0.5 and iou[1].item() == torch.tensor(0.7).item() and iou[1].item() < 0.7
    m = vision_amd.match_boxes([gt], [boxes], 0.7, 0.3, False)[0]
    assert m.tolist() == [-2, 0, -2, -1]  # float32 comparisons: 0.7f >= 0.7f, 0.3f >= 0.3f
    m = vision_amd.match_boxes([gt], [boxes], 0.5, 0.5, False)[0]
    assert m.tolist() == [0, 0, -1, -1]
    for allow in (False, True):
        for th in ((0.7, 0.3), (0.5, 0.5), (0.7, 0.7)):
            assert torch.equal(vision_amd.match_boxes([gt], [boxes], *th, allow)[0],
                               reference_matches([gt], [boxes], *th, allow)[0])
    _check_all([gt], [boxes], [torch.tensor([7], device=DEV)])


def test_low_quality_restore_gives_the_boxes_own_argmax():
    import vision_amd

    gt = torch.tensor([[0.0, 0.0, 10.0, 10.0], [5.0, 0.0, 25.0, 10.0]], device=DEV)
    boxes = torch.tensor([[0.0, 0.0, 12.0, 10.0],      # IoU 0.833 with g0, 0.28 with g1: g1's best, argmax g0
                          [100.0, 100.0, 110.0, 110.0],
                          [0.0, 0.0, 10.0, 20.0]], device=DEV)  # IoU 0.5 with g0
    iou = box_iou(gt, boxes)
    assert iou[1].argmax() == 0 and iou[:, 0].argmax() == 0
    m = vision_amd.match_boxes([gt], [boxes], 0.9, 0.3, True)[0]
    assert m.tolist() == [0, -1, -2]  # restored to its own argmax g0, not to g1
    assert torch.equal(m, reference_matches([gt], [boxes], 0.9, 0.3, True)[0])
    _check_all([gt], [boxes], [torch.tensor([3, 4], device=DEV)], rpn=(0.9, 0.3))


def test_zero_area_and_inverted_boxes():
    import vision_amd

    gt = torch.tensor([[0.0, 0.0, 10.0, 10.0], [5.0, 5.0, 5.0, 5.0]], device=DEV)  # g1 has zero area
    boxes = torch.tensor([[0.0, 0.0, 10.0, 20.0],       # IoU 0.5 with g0: g0's best
                          [50.0, 50.0, 40.0, 70.0],     # x inverted: area -200, IoU -0.0 with g0
                          [200.0, 200.0, 210.0, 210.0],  # IoU +0.0
                          [5.0, 5.0, 5.0, 5.0],          # zero area: NaN with g1
                          [7.0, 7.0, 7.0, 7.0]], device=DEV)
    iou = box_iou(gt, boxes)
    assert str(iou[0, 1].item()) == "-0.0" and iou[1, 3].isnan()
    for allow in (True, False):
        for th in ((0.7, 0.3), (0.5, 0.4), (0.3, 0.1)):
            assert torch.equal(vision_amd.match_boxes([gt], [boxes], *th, allow)[0],
                               reference_matches([gt], [boxes], *th, allow)[0])
    # g0's best is 0.5: only box 0 is restored (a raw-bit key would make -0.0 the best and restore boxes 1 and 2)
    g0 = gt[:1]
    assert vision_amd.match_boxes([g0], [boxes[:3]], 0.7, 0.3, True)[0].tolist() == [0, -1, -1]
    _check_all([gt, g0], [boxes, boxes[:3]], [torch.tensor([1, 2], device=DEV), torch.tensor([1], device=DEV)])


def test_results_are_reproducible():
    import vision_amd

    g = torch.Generator().manual_seed(8)
    gt = [_boxes(50, g).to(DEV) for _ in range(4)]
    boxes = [_anchors(100_000, g).to(DEV) for _ in range(4)]
    a = vision_amd.match_boxes(gt, boxes, 0.7, 0.3, True)
    b = vision_amd.match_boxes(gt, boxes, 0.7, 0.3, True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_matching_is_sync_free():
    import vision_amd

    g = torch.Generator().manual_seed(9)
    gt = [_boxes(n, g).to(DEV) for n in (7, 0, 30)]
    labels = _labels(gt, g)
    boxes = [_boxes(n, g).to(DEV) for n in (5000, 3000, 4000)]
    targets = [{"boxes": t} for t in gt]
    vision_amd.match_boxes(gt, boxes, 0.7, 0.3, True)  # first call: loads the library
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        vision_amd.match_boxes(gt, boxes, 0.5, 0.4, True)
        vision_amd.rpn_assign_targets(boxes, targets)
        vision_amd.roi_heads_assign_targets(boxes, gt, labels)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()


def test_fuse_detection_model_swaps_the_assign_methods():
    import vision_amd

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.rpn, self.roi_heads = RegionProposalNetwork(), RoIHeads()

    g = torch.Generator().manual_seed(10)
    gt = [_boxes(n, g).to(DEV) for n in (12, 0, 3)]
    labels = _labels(gt, g)
    targets = [{"boxes": t, "labels": lb} for t, lb in zip(gt, labels)]
    anchors = [_anchors(20_000, g).to(DEV)] * 3
    proposals = [torch.cat([_boxes(2000, g).to(DEV), t]) for t in gt]

    ref = Model()
    model = vision_amd.fuse_detection_model(Model(), training_targets=False)
    assert "assign_targets_to_anchors" not in vars(model.rpn)
    assert "assign_targets_to_proposals" not in vars(model.roi_heads)
    vision_amd.fuse_detection_model(model, training_targets=True)
    assert "assign_targets_to_anchors" in vars(model.rpn)
    assert "assign_targets_to_proposals" in vars(model.roi_heads)

    for a, b in zip(sum(model.rpn.assign_targets_to_anchors(anchors, targets), []),
                    sum(ref.rpn.assign_targets_to_anchors(anchors, targets), [])):
        assert torch.equal(a, b)
    for a, b in zip(sum(model.roi_heads.assign_targets_to_proposals(proposals, gt, labels), []),
                    sum(ref.roi_heads.assign_targets_to_proposals(proposals, gt, labels), [])):
        assert torch.equal(a, b)

    retina = vision_amd.fuse_detection_model(RetinaNet(), training_targets=False)
    assert "compute_loss" not in vars(retina)
    vision_amd.fuse_detection_model(retina, training_targets=True)
    assert "compute_loss" in vars(retina)
    for a, b in zip(retina.compute_loss(targets, {}, anchors), RetinaNet().compute_loss(targets, {}, anchors)):
        assert torch.equal(a, b)

    # the fused path really ran: under sync-error mode the restated reference (torch.where) would raise
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        model.rpn.assign_targets_to_anchors(anchors, targets)
        model.roi_heads.assign_targets_to_proposals(proposals, gt, labels)
        retina.compute_loss(targets, {}, anchors)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
