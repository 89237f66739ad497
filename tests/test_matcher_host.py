"""Host side of the batched ground-truth matching (no GPU): the C-ABI entry, the dispatcher schema and fake kernel, the
public functions' refusals and the integration wrappers' fall-back to the reference's methods (the compute is in
test_gpu_matcher.py)."""
import ctypes
import types

import pytest
import torch

from helpers import ROOT  # noqa: F401


def _lib():
    import vision_amd

    lib = vision_amd._loader.kernels()
    lib.tvmi_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_entry():
    import os
    import re

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tvmi.h")).read(), flags=re.S)
    lib = _lib()
    for sym in ("tvmi_match_boxes", "tvmi_match_boxes_workspace_bytes"):
        assert re.search(r"\b" + sym + r"\s*\(", text), sym
        assert hasattr(lib, sym), sym


def test_entry_refuses_bad_arguments_before_any_launch():
    lib = _lib()
    ws = lib.tvmi_match_boxes_workspace_bytes
    ws.restype = ctypes.c_size_t
    ws.argtypes = [ctypes.c_int64]
    assert ws(0) == 0 and ws(3000) >= 3000 * 4 and ws(3000) % 256 == 0
    f = lib.tvmi_match_boxes
    f.restype = ctypes.c_int
    f.argtypes = ([ctypes.c_void_p] * 5 + [ctypes.c_int] + [ctypes.c_int64] * 3 + [ctypes.c_double] * 2 + [ctypes.c_int]
                  + [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p])
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below returns before a launch
    big = 1 << 20

    def call(boxes=p, bo=p, gt=p, go=p, gl=None, dt=0, N=10, M=3, B=2, high=0.7, low=0.3, allow=1, matches=p, matched=p,
             labels=None, wsp=p, wsb=big):
        return f(boxes, bo, gt, go, gl, dt, N, M, B, high, low, allow, matches, matched, labels, wsp, wsb, None)

    assert call(N=0, M=0, B=0, boxes=None, bo=None, gt=None, go=None, matches=None, matched=None, wsp=None, wsb=0) == 0
    assert call(N=-1) != 0
    assert b"match_boxes" in lib.tvmi_last_error()
    assert call(M=-1) != 0
    assert call(B=-1) != 0
    assert call(high=0.3, low=0.7) != 0  # low > high
    assert b"low threshold" in lib.tvmi_last_error()
    assert call(dt=5) != 0  # float64 boxes are not served
    assert call(boxes=None) != 0
    assert call(gt=None) != 0
    assert call(matched=None) != 0
    assert call(gl=p) != 0  # gt_labels without labels
    assert call(wsp=None) != 0  # allow_low_quality needs the workspace
    assert call(wsb=64) != 0
    assert call(boxes=ctypes.c_void_p(4100)) != 0  # not 16-byte aligned


def test_schema_is_registered():
    import vision_amd  # noqa: F401

    op = torch.ops.tvmi.match_boxes.default
    assert str(op._schema) == ("tvmi::match_boxes(Tensor boxes, Tensor box_offsets, Tensor gt, Tensor gt_offsets, "
                               "Tensor? gt_labels, float high, float low, bool allow_low_quality) -> (Tensor, Tensor, Tensor)")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("tvmi::match_boxes", "CUDA")


def test_fake_kernel_gives_shapes_and_dtypes():
    import vision_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        bo, go = torch.empty(3, dtype=torch.int64), torch.empty(3, dtype=torch.int64)
        m, g, lb = torch.ops.tvmi.match_boxes(torch.empty(50, 4), bo, torch.empty(7, 4), go, None, 0.7, 0.3, True)
        assert m.shape == (50,) and m.dtype == torch.int64
        assert g.shape == (50, 4) and g.dtype == torch.float32
        assert lb.shape == (0,) and lb.dtype == torch.int64
        _, _, lb = torch.ops.tvmi.match_boxes(torch.empty(50, 4), bo, torch.empty(7, 4), go,
                                              torch.empty(7, dtype=torch.int64), 0.5, 0.5, False)
        assert lb.shape == (50,) and lb.dtype == torch.int64


def test_public_functions_refuse_cpu_tensors():
    import vision_amd

    gt, boxes = [torch.tensor([[0.0, 0.0, 10.0, 10.0]])], [torch.rand(5, 4)]
    with pytest.raises(RuntimeError):
        vision_amd.match_boxes(gt, boxes, 0.7, 0.3, True)
    with pytest.raises(RuntimeError):
        vision_amd.rpn_assign_targets(boxes, [{"boxes": gt[0]}])
    with pytest.raises(RuntimeError):
        vision_amd.roi_heads_assign_targets(boxes, gt, [torch.ones(1, dtype=torch.int64)])


def test_image_with_gt_but_no_boxes_raises_the_reference_error():
    import vision_amd

    # raised from the shapes alone, before anything touches a device
    with pytest.raises(ValueError, match="^No proposal boxes available for one of the images during training$"):
        vision_amd.match_boxes([torch.zeros(2, 4)], [torch.zeros(0, 4)], 0.7, 0.3, True)


class Matcher:
    BELOW_LOW_THRESHOLD = -1
    BETWEEN_THRESHOLDS = -2

    def __init__(self, high, low, allow):
        self.high_threshold, self.low_threshold, self.allow_low_quality_matches = high, low, allow


class SSDMatcher(Matcher):
    pass


def box_iou(a, b):
    return None


box_iou.__module__ = "torchvision.ops.boxes"


def other_iou(a, b):
    return None


class RegionProposalNetwork(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.proposal_matcher = Matcher(0.7, 0.3, True)
        self.box_similarity = box_iou

    def assign_targets_to_anchors(self, anchors, targets):
        return "reference"


class RoIHeads(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.proposal_matcher = Matcher(0.5, 0.5, False)

    def assign_targets_to_proposals(self, proposals, gt_boxes, gt_labels):
        return "reference"


class RetinaNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.proposal_matcher = Matcher(0.5, 0.4, True)

    def compute_loss(self, targets, head_outputs, anchors):
        return "reference"


def test_wrappers_fall_back_to_the_reference():
    from vision_amd import integration

    cpu = [torch.rand(4, 4)]
    tgt = [{"boxes": torch.rand(2, 4), "labels": torch.ones(2, dtype=torch.int64)}]
    rpn, rh, rn = RegionProposalNetwork(), RoIHeads(), RetinaNet()
    a = integration.make_assign_targets_to_anchors(RegionProposalNetwork.assign_targets_to_anchors)
    p = integration.make_assign_targets_to_proposals(RoIHeads.assign_targets_to_proposals)
    c = integration.make_retinanet_compute_loss(RetinaNet.compute_loss)
    # CPU tensors
    assert a(rpn, cpu, tgt) == "reference"
    assert p(rh, cpu, [tgt[0]["boxes"]], [tgt[0]["labels"]]) == "reference"
    assert c(rn, tgt, {}, cpu) == "reference"
    # a foreign matcher class (a subclass too) and a foreign similarity: the reference, whatever the tensors
    if torch.cuda.is_available():
        cpu = [t.cuda() for t in cpu]
        tgt = [{k: v.cuda() for k, v in tgt[0].items()}]
    for m in (SSDMatcher(0.7, 0.3, True), types.SimpleNamespace(high_threshold=0.7, low_threshold=0.3,
                                                                allow_low_quality_matches=True)):
        rpn.proposal_matcher = rh.proposal_matcher = rn.proposal_matcher = m
        assert a(rpn, cpu, tgt) == "reference"
        assert p(rh, cpu, [tgt[0]["boxes"]], [tgt[0]["labels"]]) == "reference"
        assert c(rn, tgt, {}, cpu) == "reference"
    rpn.proposal_matcher = Matcher(0.7, 0.3, True)
    rpn.box_similarity = other_iou
    assert a(rpn, cpu, tgt) == "reference"


def test_fuse_binds_training_targets_only_when_asked():
    import vision_amd

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.rpn, self.roi_heads = RegionProposalNetwork(), RoIHeads()

    model = vision_amd.fuse_detection_model(Model())
    assert "assign_targets_to_anchors" not in vars(model.rpn)
    assert "assign_targets_to_proposals" not in vars(model.roi_heads)
    vision_amd.fuse_detection_model(model, training_targets=True)
    assert "assign_targets_to_anchors" in vars(model.rpn)
    assert "assign_targets_to_proposals" in vars(model.roi_heads)
    assert model.rpn.assign_targets_to_anchors([torch.rand(3, 4)], [{"boxes": torch.rand(1, 4)}]) == "reference"  # CPU

    rn = vision_amd.fuse_detection_model(RetinaNet(), training_targets=True)
    assert "compute_loss" in vars(rn)

    class MyRetinaNet(RetinaNet):  # a subclass with a loss of its own keeps it
        def compute_loss(self, targets, head_outputs, anchors):
            return "own"

    assert "compute_loss" not in vars(vision_amd.fuse_detection_model(MyRetinaNet(), training_targets=True))
