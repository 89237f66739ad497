"""Keypoint R-CNN inference decoding (`vision_amd.heatmaps_to_keypoints` / `keypointrcnn_inference`, csrc/keypoints.hip)
against the reference's per-detection loop (torchvision 0.30 roi_heads.py heatmaps_to_keypoints), restated here:

  w = clamp(x2 - x1, min=1); h = clamp(y2 - y1, min=1); OW = ceil(w); OH = ceil(h); wc = w / OW; hc = h / OH
  roi_map = bicubic resize (align_corners=False) of maps[i] to [OH, OW]; pos = argmax (first max, NaN first)
  xy = ((pos % OW + 0.5) * wc + x1, (pos // OW + 0.5) * hc + y1, 1); score = roi_map[k, pos]
"""
import sys
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
K = 17


def _geometry(rois):
    """The reference's per-ROI sizes and corrections, in float32 on the host (true divisions)."""
    r = rois.detach().float().cpu()
    w = (r[:, 2] - r[:, 0]).clamp(min=1)
    h = (r[:, 3] - r[:, 1]).clamp(min=1)
    return r, w, h, w.ceil(), h.ceil()


def _xy_at(pos_x, pos_y, i, r, w, h, wce, hce):
    wc, hc = w[i] / wce[i], h[i] / hce[i]
    return (pos_x.float() + 0.5) * wc + r[i, 0], (pos_y.float() + 0.5) * hc + r[i, 1]


def _device_loop(maps, rois):
    """The reference loop on the device with vision_amd.interpolate (bicubic2d_kernel for K = 17 and sides <= 600)."""
    import vision_amd

    r, w, h, wce, hce = _geometry(rois)
    R = maps.shape[0]
    xy = torch.ones(R, 3, K)
    sc = torch.empty(R, K)
    for i in range(R):
        OW, OH = int(wce[i]), int(hce[i])
        roi_map = vision_amd.interpolate(maps[i][:, None], size=(OH, OW), mode="bicubic", align_corners=False)[:, 0]
        flat = roi_map.reshape(K, -1)
        pos = flat.argmax(1)
        sc[i] = flat.gather(1, pos[:, None])[:, 0].float().cpu()
        pos = pos.cpu()
        xy[i, 0], xy[i, 1] = _xy_at(pos % OW, pos // OW, i, r, w, h, wce, hce)
    return xy.permute(0, 2, 1), sc


def _cpu_map(maps, i, wce, hce):
    """The reference's roi_map on the CPU in float32 (torch's own bicubic).  At the maps' own size it is the maps: ATen's
    CUDA kernel copies then (the contract), where the CPU kernel multiplies the zero-weight taps (a NaN would spread)."""
    m = maps[i].float().cpu()[:, None]
    if (int(hce[i]), int(wce[i])) == tuple(m.shape[-2:]):
        return m[:, 0].clone()
    return F.interpolate(m, size=(int(hce[i]), int(wce[i])), mode="bicubic", align_corners=False)[:, 0]


def _blobs(R, H, W, g):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    c = torch.rand(R, K, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])
    s = 1.0 + 4.0 * torch.rand(R, K, 1, 1, generator=g)
    d2 = (xx - c[..., 0, None, None]) ** 2 + (yy - c[..., 1, None, None]) ** 2
    return 8.0 * torch.exp(-d2 / (2 * s * s)) - 1.0


def _rois_small(g):
    """64 boxes with fractional coordinates and sides 1..600 px, plus the special cases."""
    n = 64
    xy = torch.rand(n, 2, generator=g) * 700
    wh = 1.0 + torch.rand(n, 2, generator=g) * 599.0
    rois = torch.cat([xy, xy + wh], 1)
    rois[0] = torch.tensor([10.25, 20.5, 10.25 + 55.5, 20.5 + 55.75])  # ceil size exactly 56 x 56: the copy path
    rois[1] = torch.tensor([300.5, 40.0, 290.25, 180.5])  # x2 < x1: width clamps to 1
    rois[2] = torch.tensor([5.5, 6.5, 5.75, 6.6])  # 1 x 1
    rois[3] = torch.tensor([0.0, 0.0, 600.0, 599.5])
    return rois


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("kind", ["randn", "blobs"])
def test_bit_exact_against_device_loop(dtype, kind):
    import vision_amd

    g = torch.Generator().manual_seed(11)
    rois = _rois_small(g)
    R = rois.shape[0]
    maps = torch.randn(R, K, 56, 56, generator=g) * 3 if kind == "randn" else _blobs(R, 56, 56, g)
    maps, rois_d = maps.to(DEV, dtype), rois.to(DEV)
    xy, sc = vision_amd.heatmaps_to_keypoints(maps, rois_d)
    rxy, rsc = _device_loop(maps, rois_d)
    assert xy.shape == (R, K, 3) and sc.shape == (R, K) and xy.dtype == sc.dtype == torch.float32
    assert torch.equal(xy.cpu(), rxy), (xy.cpu() != rxy).nonzero()[:5]
    assert torch.equal(sc.cpu(), rsc)


def _check_one(v, OW, i, k, geo, xy, sc, exact=False):
    """One (ROI, k) against the CPU oracle's flat map v: the kernel's xy is the reference formula at a position p whose
    oracle value is within 1e-5 * max(1, |max|) of the oracle's max, and its score within that tolerance of v[p].
    exact: where the oracle's margin between its top two values is far above the tolerance, p IS the oracle's argmax.
    Returns True when the exact rule applied."""
    r, w, h, wce, hce = geo
    m = v.max()
    tol = 1e-5 * max(1.0, abs(float(m)))
    cand = (v >= m - tol).nonzero()[:, 0]
    cx, cy = _xy_at(cand % OW, cand // OW, i, r, w, h, wce, hce)
    hit = (cx == xy[i, k, 0]) & (cy == xy[i, k, 1])
    assert hit.any(), (i, k, xy[i, k], float(m))
    p = cand[hit][0]
    assert abs(float(v[p]) - float(sc[i, k])) <= tol, (i, k)
    assert xy[i, k, 2] == 1
    if exact and v.numel() > 1:
        top2 = v.topk(2).values
        if float(top2[0] - top2[1]) > 10 * tol:
            assert int(p) == int(v.argmax()), (i, k)
            return True
    return False


def _check_near_tie(maps, rois, xy, sc, exact=False):
    """_check_one for every (ROI, k); returns the number checked with the exact rule."""
    geo = _geometry(rois)
    xy, sc = xy.cpu(), sc.cpu()
    n_exact = 0
    for i in range(rois.shape[0]):
        V = _cpu_map(maps, i, geo[3], geo[4])
        for k in range(K):
            n_exact += _check_one(V[k].reshape(-1), V.shape[2], i, k, geo, xy, sc, exact)
    return n_exact


def test_against_cpu_reference_with_near_tie_rule():
    import vision_amd

    g = torch.Generator().manual_seed(5)
    rois = torch.tensor([[0.0, 0.0, 1333.0, 800.0],  # full image: hundreds of chunks
                         [100.25, 50.5, 1000.25, 750.75],  # 900 x 700
                         [12.5, 7.25, 140.0, 99.0],
                         [600.0, 300.0, 633.3, 305.1],
                         [40.0, 500.0, 41.0, 720.0]])
    maps = (torch.randn(5, K, 56, 56, generator=g) * 3).to(DEV)
    xy, sc = vision_amd.heatmaps_to_keypoints(maps, rois.to(DEV))
    _check_near_tie(maps, rois, xy, sc)


def test_unique_peak_gives_the_oracle_position():
    import vision_amd

    g = torch.Generator().manual_seed(6)
    rois = torch.tensor([[0.0, 0.0, 1333.0, 800.0], [100.25, 50.5, 1000.25, 750.75], [12.5, 7.25, 140.0, 99.0],
                         [20.0, 30.0, 45.5, 41.25]])
    R = rois.shape[0]
    maps = torch.randn(R, K, 56, 56, generator=g) * 0.01
    idx = torch.randint(0, 56 * 56, (R, K), generator=g)
    maps.view(R, K, -1).scatter_(2, idx[..., None], 10.0)  # one spike per map
    maps_d = maps.to(DEV)
    xy, sc = vision_amd.heatmaps_to_keypoints(maps_d, rois.to(DEV))
    n_exact = _check_near_tie(maps_d, rois, xy, sc, exact=True)
    assert n_exact >= R * K // 2, n_exact


def test_ties_zero_and_negative_zero_give_flat_index_zero():
    import vision_amd

    rois = torch.tensor([[3.5, 4.25, 90.0, 70.5], [0.0, 0.0, 56.0, 56.0], [10.0, 10.0, 700.0, 500.0]])
    r, w, h, wce, hce = _geometry(rois)
    for fill in (0.0, -0.0):
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            maps = torch.full((3, K, 56, 56), fill, device=DEV, dtype=dtype)
            xy, sc = vision_amd.heatmaps_to_keypoints(maps, rois.to(DEV))
            for i in range(3):
                ex, ey = _xy_at(torch.tensor(0), torch.tensor(0), i, r, w, h, wce, hce)
                assert torch.equal(xy[i, :, 0].cpu(), ex.expand(K)) and torch.equal(xy[i, :, 1].cpu(), ey.expand(K))
            assert torch.equal(sc.cpu(), torch.zeros(3, K))


def test_nan_pixel_gives_first_nan_position():
    import vision_amd

    g = torch.Generator().manual_seed(8)
    # scales 0.5 / 0.25 / 1 (copy): the source indices are exact, so the CPU oracle's NaN region is unambiguous
    rois = torch.tensor([[10.0, 20.0, 234.0, 132.0], [0.5, 0.5, 56.5, 56.5], [5.0, 5.0, 117.0, 229.0]])
    maps = torch.randn(3, K, 56, 56, generator=g)
    maps[0, 3, 30, 17] = float("nan")
    maps[1, 0, 0, 40] = float("nan")
    maps[1, 0, 50, 2] = float("nan")
    maps[2, 16, 55, 55] = float("nan")
    maps_d = maps.to(DEV)
    xy, sc = vision_amd.heatmaps_to_keypoints(maps_d, rois.to(DEV))
    xy, sc = xy.cpu(), sc.cpu()
    geo = _geometry(rois)
    nan_at = {(0, 3), (1, 0), (2, 16)}
    for i in range(3):
        V = _cpu_map(maps_d, i, geo[3], geo[4])
        OW = V.shape[2]
        for k in range(K):
            v = V[k].reshape(-1)
            if (i, k) not in nan_at:
                assert not torch.isnan(v).any()
                _check_one(v, OW, i, k, geo, xy, sc)
                continue
            p = torch.isnan(v).nonzero()[0, 0]
            assert torch.isnan(sc[i, k])
            ex, ey = _xy_at(p % OW, p // OW, i, *geo)
            assert xy[i, k, 0] == ex and xy[i, k, 1] == ey, (i, k)


def test_non_finite_roi_gives_nan_for_that_roi_only():
    import vision_amd

    g = torch.Generator().manual_seed(9)
    rois = _rois_small(g)[:8].clone()
    rois[2, 0] = float("nan")
    rois[5, 3] = float("inf")
    rois[6] = torch.tensor([0.0, 0.0, 3e38, 3e38])  # finite, but a map far above 2^31 pixels
    maps = (torch.randn(8, K, 56, 56, generator=g) * 3).to(DEV)
    xy, sc = vision_amd.heatmaps_to_keypoints(maps, rois.to(DEV))
    bad = [2, 5, 6]
    good = [i for i in range(8) if i not in bad]
    assert torch.isnan(xy[bad, :, :2]).all() and torch.isnan(sc[bad]).all()
    assert (xy[:, :, 2] == 1).all()
    gxy, gsc = vision_amd.heatmaps_to_keypoints(maps[good], rois[good].to(DEV))
    assert torch.equal(xy[good], gxy) and torch.equal(sc[good], gsc)


def test_batched_inference_matches_per_image_calls():
    import vision_amd

    g = torch.Generator().manual_seed(10)
    counts = [100, 0, 37, 1]
    boxes = []
    for n in counts:
        xy = torch.rand(n, 2, generator=g) * 600
        boxes.append(torch.cat([xy, xy + 1 + torch.rand(n, 2, generator=g) * 400], 1).to(DEV))
    x = (torch.randn(sum(counts), K, 56, 56, generator=g) * 3).to(DEV)
    kps, scores = vision_amd.keypointrcnn_inference(x, boxes)
    assert len(kps) == len(scores) == 4
    off = 0
    for n, b, kp, s in zip(counts, boxes, kps, scores):
        assert kp.shape == (n, K, 3) and s.shape == (n, K)
        if n:
            assert kp.stride() == (3 * K, 1, K)  # the reference's permuted view of [n, 3, K]
            ekp, es = vision_amd.heatmaps_to_keypoints(x[off:off + n], b)
            assert torch.equal(kp, ekp) and torch.equal(s, es)
            assert (kp[:, :, 2] == 1).all()
        off += n
    kp0, s0 = vision_amd.keypointrcnn_inference(x[:0], [boxes[1]])
    assert kp0[0].shape == (0, K, 3) and s0[0].shape == (0, K)
    e_kp, e_s = vision_amd.heatmaps_to_keypoints(x[:0], boxes[1])
    assert e_kp.shape == (0, K, 3) and e_s.shape == (0, K)


def test_inference_is_sync_free():
    import vision_amd

    g = torch.Generator().manual_seed(12)
    boxes = [torch.tensor([[1.5, 2.5, 300.0, 200.0], [50.0, 60.0, 70.0, 90.0]], device=DEV),
             torch.tensor([[0.0, 0.0, 1333.0, 800.0]], device=DEV)]
    x = torch.randn(3, K, 56, 56, generator=g).to(DEV)
    vision_amd.keypointrcnn_inference(x, boxes)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        kps, scores = vision_amd.keypointrcnn_inference(x, boxes)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert kps[1].shape == (1, K, 3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_results_are_reproducible_under_racing_chunks(dtype):
    import vision_amd

    g = torch.Generator().manual_seed(13)
    R = 24
    rois = torch.tensor([[0.25, 0.5, 1333.0, 800.0]]).repeat(R, 1).to(DEV)
    maps = _blobs(R, 56, 56, g).to(DEV, dtype)  # broad flat tops: many equal 16-bit values racing for one key
    a = vision_amd.heatmaps_to_keypoints(maps, rois)
    b = vision_amd.heatmaps_to_keypoints(maps, rois)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_fuse_detection_model_routes_keypoint_inference():
    import vision_amd
    from vision_amd import autofuse

    name = "tvmi_test_kp_roi_heads"
    mod = types.ModuleType(name)
    calls = []

    def keypointrcnn_inference(x, boxes):  # the reference's function, restated: one loop call per image
        calls.append(x.device.type)
        if not x.is_cuda:
            return [], []
        kp, sc = _device_loop(x, torch.cat(boxes, 0))
        n = [b.shape[0] for b in boxes]
        return list(kp.split(n)), list(sc.split(n))

    class RoIHeads(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.keypoint_predictor = torch.nn.Identity()

        def forward(self, x, boxes):
            return getattr(sys.modules[type(self).__module__], "keypointrcnn_inference")(x, boxes)

    RoIHeads.__module__ = name
    mod.keypointrcnn_inference = keypointrcnn_inference
    mod.RoIHeads = RoIHeads

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.roi_heads = RoIHeads()

    sys.modules[name] = mod
    try:
        model = vision_amd.fuse_detection_model(Model())
        vision_amd.fuse_detection_model(model)  # idempotent: never wraps twice
        fused = mod.keypointrcnn_inference
        assert getattr(fused, "_tvmi_autofused", False) and fused.__wrapped__ is keypointrcnn_inference
        g = torch.Generator().manual_seed(14)
        boxes = [torch.tensor([[1.5, 2.5, 300.0, 200.0], [50.0, 60.0, 70.0, 90.0]], device=DEV),
                 torch.tensor([[10.0, 5.0, 120.0, 330.0]], device=DEV)]
        x = (torch.randn(3, K, 56, 56, generator=g) * 3).to(DEV)
        kps, scores = model.roi_heads(x, boxes)
        assert calls == []
        ekp, es = vision_amd.keypointrcnn_inference(x, boxes)
        for a, b in zip(kps + scores, ekp + es):
            assert torch.equal(a, b)
        rkp, rs = keypointrcnn_inference(x, boxes)  # and the reference restated on the device agrees
        for a, b in zip(kps + scores, rkp + rs):
            assert torch.equal(a.cpu(), b)
        calls.clear()
        model.roi_heads(x.cpu(), [b.cpu() for b in boxes])
        assert calls == ["cpu"]
    finally:
        sys.modules.pop(name, None)
        autofuse._patched[:] = [p for p in autofuse._patched if p[0] is not mod]
