"""Host side of the keypoint decoding (no GPU): the C-ABI entry, the dispatcher schema and fake kernel, the autofuse
target and the integration wrapper's fall-back to the reference's function (the compute is in test_gpu_keypoints.py)."""
import ctypes
import sys
import types

import pytest
import torch

from helpers import ROOT  # noqa: F401

K = 17


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
    for sym in ("tvmi_heatmaps_to_keypoints", "tvmi_heatmaps_to_keypoints_workspace_bytes"):
        assert re.search(r"\b" + sym + r"\s*\(", text), sym
        assert hasattr(lib, sym), sym


def test_entry_refuses_bad_arguments_before_any_launch():
    lib = _lib()
    ws = lib.tvmi_heatmaps_to_keypoints_workspace_bytes
    ws.restype = ctypes.c_size_t
    ws.argtypes = [ctypes.c_int64, ctypes.c_int64]
    assert ws(0, K) == 0 and ws(400, K) >= 400 * K * 8
    f = lib.tvmi_heatmaps_to_keypoints
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_int64] * 4 + [ctypes.c_void_p, ctypes.c_size_t,
                                                                                 ctypes.c_void_p]
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below returns before a launch
    assert f(fake, fake, fake, fake, 0, 0, K, 56, 56, None, 0, None) == 0  # R == 0: nothing to do
    assert f(fake, fake, fake, fake, 0, 3, 0, 56, 56, fake, 1 << 20, None) != 0  # K == 0
    assert f(fake, fake, fake, fake, 0, 3, K, 56, 56, None, 1 << 20, None) != 0  # no workspace
    assert f(fake, fake, fake, fake, 0, 3, K, 56, 56, fake, 64, None) != 0  # workspace too small
    assert b"heatmaps_to_keypoints" in lib.tvmi_last_error()
    assert f(fake, fake, fake, fake, 4, 3, K, 56, 56, fake, 1 << 20, None) != 0  # float64 maps are not served


def test_schema_is_registered():
    import vision_amd  # noqa: F401

    op = torch.ops.tvmi.heatmaps_to_keypoints.default
    assert str(op._schema) == "tvmi::heatmaps_to_keypoints(Tensor maps, Tensor rois) -> (Tensor, Tensor)"
    assert torch._C._dispatch_has_kernel_for_dispatch_key("tvmi::heatmaps_to_keypoints", "CUDA")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_fake_kernel_gives_reference_shapes_dtypes_and_strides(dtype):
    import vision_amd  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        xy, sc = torch.ops.tvmi.heatmaps_to_keypoints(torch.empty(5, K, 56, 56, dtype=dtype), torch.empty(5, 4))
        # the reference: xy_preds [R, 3, K] returned as xy_preds.permute(0, 2, 1), end_scores [R, K] float32
        assert xy.shape == (5, K, 3) and xy.stride() == (3 * K, 1, K) and xy.dtype == torch.float32
        assert sc.shape == (5, K) and sc.stride() == (K, 1) and sc.dtype == torch.float32
        xy0, sc0 = torch.ops.tvmi.heatmaps_to_keypoints(torch.empty(0, K, 56, 56, dtype=dtype), torch.empty(0, 4))
        assert xy0.shape == (0, K, 3) and sc0.shape == (0, K)


def test_public_functions_refuse_cpu_tensors():
    import vision_amd

    x, b = torch.randn(2, K, 56, 56), torch.tensor([[0.0, 0.0, 10.0, 10.0], [1.0, 2.0, 30.0, 40.0]])
    with pytest.raises(RuntimeError):
        vision_amd.heatmaps_to_keypoints(x, b)
    with pytest.raises(RuntimeError):
        vision_amd.keypointrcnn_inference(x, [b])


def test_autofuse_lists_and_swaps_the_module_global(monkeypatch):
    from vision_amd import autofuse

    assert (None, "keypointrcnn_inference", "make_keypointrcnn_inference") in \
        autofuse._TARGETS["torchvision.models.detection.roi_heads"]
    monkeypatch.delenv("TVMI_NO_PY_REGISTRATIONS", raising=False)  # the lazy wrapper sets it; restored afterwards
    mod = types.ModuleType("torchvision.models.detection.roi_heads")  # never inserted into sys.modules
    calls = []

    def keypointrcnn_inference(x, boxes):
        calls.append(len(boxes))
        return "reference"

    mod.keypointrcnn_inference = keypointrcnn_inference
    n_before = len(autofuse._patched)
    autofuse._patch_module(mod)
    try:
        swapped = mod.keypointrcnn_inference
        assert swapped is not keypointrcnn_inference and swapped._tvmi_autofused
        autofuse._patch_module(mod)  # idempotent
        assert mod.keypointrcnn_inference is swapped and len(autofuse._patched) == n_before + 1
        assert swapped(torch.randn(1, K, 56, 56), [torch.zeros(1, 4)]) == "reference" and calls == [1]  # CPU: the original
    finally:
        autofuse.uninstall()
    assert mod.keypointrcnn_inference is keypointrcnn_inference
    assert "torchvision.models.detection.roi_heads" not in sys.modules or \
        sys.modules["torchvision.models.detection.roi_heads"] is not mod


def test_integration_wrapper_and_fuse_fall_back_on_cpu():
    import vision_amd
    from vision_amd import autofuse, integration

    calls = []

    def keypointrcnn_inference(x, boxes):
        calls.append(x.device.type)
        return "reference"

    fn = integration.make_keypointrcnn_inference(keypointrcnn_inference)
    assert fn(torch.randn(1, K, 56, 56), [torch.zeros(1, 4)]) == "reference" and calls == ["cpu"]

    name = "tvmi_test_kp_host_roi_heads"
    mod = types.ModuleType(name)
    mod.keypointrcnn_inference = keypointrcnn_inference

    class RoIHeads(torch.nn.Module):
        def __init__(self, predictor):
            super().__init__()
            self.keypoint_predictor = predictor

        def forward(self, x, boxes):
            return getattr(sys.modules[type(self).__module__], "keypointrcnn_inference")(x, boxes)

    RoIHeads.__module__ = name
    model = types.SimpleNamespace(roi_heads=RoIHeads(None))
    sys.modules[name] = mod
    try:
        vision_amd.fuse_detection_model(model)  # no keypoint predictor: nothing to route
        assert mod.keypointrcnn_inference is keypointrcnn_inference
        model.roi_heads.keypoint_predictor = torch.nn.Identity()
        vision_amd.fuse_detection_model(model, keypoints=False)
        assert mod.keypointrcnn_inference is keypointrcnn_inference
        vision_amd.fuse_detection_model(model)
        assert mod.keypointrcnn_inference._tvmi_autofused
        calls.clear()
        assert model.roi_heads(torch.randn(2, K, 56, 56), [torch.zeros(2, 4)]) == "reference" and calls == ["cpu"]
    finally:
        sys.modules.pop(name, None)
        autofuse._patched[:] = [p for p in autofuse._patched if p[0] is not mod]
