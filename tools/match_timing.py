"""Ground-truth matching of a detector training step: the fused `vision_amd` calls (csrc/matcher.hip) against the reference's
per-image loop restated on the device (torchvision 0.30: ops/boxes.py box_iou + models/detection/_utils.py Matcher, as
called by rpn.py assign_targets_to_anchors, roi_heads.py assign_targets_to_proposals and retinanet.py compute_loss).

Workloads (seeded), each at --batches images:
  rpn        268,569 FPN anchors per image (800 x 1344), Matcher(0.7, 0.3, True), G ~ 7 on average, at most 50;
  roi_heads  2000 proposals + the G gt per image (add_gt_proposals), Matcher(0.5, 0.5, False), with gt labels;
  retinanet  120,087 anchors per image (P3-P7 of 800 x 800), Matcher(0.5, 0.4, True).
Device-event timing after warm-up; prints ONE JSON line.

    python tools/match_timing.py                                  # every workload, batches 2, 4, 8
    python tools/match_timing.py --fused-only --reps 20           # for a kernel trace of the fused calls:
    rocprofv3 --kernel-trace --stats -d <dir> -o match -- python tools/match_timing.py --fused-only ...
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def box_iou(boxes1, boxes2):
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    lt = torch.max(boxes1[:, None, :2], boxes2[:, :2])
    rb = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


def matcher(iou, high, low, allow):
    vals, matches = iou.max(dim=0)
    all_matches = matches.clone() if allow else None
    below = vals < low
    between = (vals >= low) & (vals < high)
    matches[below] = -1
    matches[between] = -2
    if allow:
        best, _ = iou.max(dim=1)
        pairs = torch.where(iou == best[:, None])
        matches[pairs[1]] = all_matches[pairs[1]]
    return matches


def rpn_loop(anchors, targets, high=0.7, low=0.3):
    labels, matched = [], []
    for a, t in zip(anchors, targets):
        gt = t["boxes"]
        if gt.numel() == 0:
            matched.append(torch.zeros(a.shape, dtype=torch.float32, device=a.device))
            labels.append(torch.zeros((a.shape[0],), dtype=torch.float32, device=a.device))
            continue
        idx = matcher(box_iou(gt, a), high, low, True)
        matched.append(gt[idx.clamp(min=0)])
        lb = (idx >= 0).to(torch.float32)
        lb[idx == -1] = 0.0
        lb[idx == -2] = -1.0
        labels.append(lb)
    return labels, matched


def roi_heads_loop(proposals, gt_boxes, gt_labels, high=0.5, low=0.5):
    idxs, labels = [], []
    for p, gt, gl in zip(proposals, gt_boxes, gt_labels):
        if gt.numel() == 0:
            idxs.append(torch.zeros((p.shape[0],), dtype=torch.int64, device=p.device))
            labels.append(torch.zeros((p.shape[0],), dtype=torch.int64, device=p.device))
            continue
        m = matcher(box_iou(gt, p), high, low, False)
        c = m.clamp(min=0)
        lb = gl[c].to(torch.int64)
        lb[m == -1] = 0
        lb[m == -2] = -1
        idxs.append(c)
        labels.append(lb)
    return idxs, labels


def retinanet_loop(anchors, targets, high=0.5, low=0.4):
    return [torch.full((a.size(0),), -1, dtype=torch.int64, device=a.device) if t["boxes"].numel() == 0
            else matcher(box_iou(t["boxes"], a), high, low, True) for a, t in zip(anchors, targets)]


def _boxes(n, g, smin=16.0, smax=600.0):
    c = torch.rand(n, 2, generator=g) * torch.tensor([1344.0, 800.0])
    s = smin * (smax / smin) ** torch.rand(n, 1, generator=g)
    ar = 2.0 ** (2 * torch.rand(n, 1, generator=g) - 1)
    wh = torch.cat([s * ar.sqrt(), s / ar.sqrt()], 1)
    return torch.cat([c - wh / 2, c + wh / 2], 1)


def _anchors(levels, sizes, ratios, W=1344):
    out = []
    for stride, size in zip(levels, sizes):
        ys, xs = torch.meshgrid(torch.arange(0, 800, stride, dtype=torch.float32),
                                torch.arange(0, W, stride, dtype=torch.float32), indexing="ij")
        ctr = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)
        for s in size:
            for r in ratios:
                half = torch.tensor([s / r ** 0.5, s * r ** 0.5]) / 2
                out.append(torch.cat([ctr - half, ctr + half], 1))
    return torch.cat(out).round()


def workload(kind, B, seed=0, device="cuda"):
    g = torch.Generator().manual_seed(seed + B)
    counts = (-7.0 * torch.log1p(-torch.rand(B, generator=g))).round().clamp(1, 50).long().tolist()  # exponential, mean ~7
    counts[0] = 50  # the largest image of COCO-like batches
    gt = [_boxes(n, g).to(device) for n in counts]
    labels = [torch.randint(1, 91, (n,), generator=g).to(device) for n in counts]
    if kind == "rpn":    # rpn.py AnchorGenerator((32,), (64,), (128,), (256,), (512,)) x 3 ratios on strides 4..64
        a = _anchors((4, 8, 16, 32, 64), ((32,), (64,), (128,), (256,), (512,)), (0.5, 1.0, 2.0)).to(device)
        boxes = [a] * B
    elif kind == "retinanet":  # 3 scales x 3 ratios on strides 8..128 (P3-P7) of an 800 x 800 image: 120,087
        a = _anchors((8, 16, 32, 64, 128), tuple(tuple(x * 2 ** (k / 3) for k in range(3)) for x in (32, 64, 128, 256, 512)),
                     (0.5, 1.0, 2.0), W=800).to(device)
        boxes = [a] * B
    else:
        boxes = [torch.cat([_boxes(2000, g).to(device), t]) for t in gt]
    return gt, labels, boxes


def time_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--kinds", nargs="+", default=["rpn", "roi_heads", "retinanet"])
    ap.add_argument("--reps", type=int, default=100, help="timed calls of the fused path")
    ap.add_argument("--loop-reps", type=int, default=10, help="timed calls of the loop")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true", help="run the fused path only (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("match_timing.py needs a GPU")
    import vision_amd

    rows = []
    for kind in args.kinds:
        for B in args.batches:
            gt, labels, boxes = workload(kind, B)
            targets = [{"boxes": t, "labels": lb} for t, lb in zip(gt, labels)]
            if kind == "rpn":
                fused = lambda: vision_amd.rpn_assign_targets(boxes, targets)  # noqa: E731
                loop = lambda: rpn_loop(boxes, targets)  # noqa: E731
            elif kind == "roi_heads":
                fused = lambda: vision_amd.roi_heads_assign_targets(boxes, gt, labels)  # noqa: E731
                loop = lambda: roi_heads_loop(boxes, gt, labels)  # noqa: E731
            else:
                fused = lambda: vision_amd.match_boxes(gt, boxes, 0.5, 0.4, True)  # noqa: E731
                loop = lambda: retinanet_loop(boxes, targets)  # noqa: E731
            row = {"kind": kind, "B": B, "boxes_per_image": boxes[0].shape[0], "gt": [t.shape[0] for t in gt]}
            row["fused_ms"] = round(time_ms(fused, args.reps, args.warmup), 4)
            if not args.fused_only:
                row["loop_ms"] = round(time_ms(loop, args.loop_reps, 2), 4)
                row["speedup"] = round(row["loop_ms"] / row["fused_ms"], 1)
                f, r = fused(), loop()
                f = list(f) if isinstance(f, tuple) else [f]
                r = list(r) if isinstance(r, tuple) else [r]
                row["outputs_equal"] = all(torch.equal(torch.cat(x), torch.cat(y)) for x, y in zip(f, r))
            rows.append(row)
    print(json.dumps({"workloads": rows}))


if __name__ == "__main__":
    main()
