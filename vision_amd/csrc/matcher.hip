// matcher.hip — ground-truth matching of anchors / proposals for detector training, every image of the batch at once, for gfx950.
//
// Reference: torchvision 0.30 models/detection/_utils.py Matcher (+ set_low_quality_matches_), called per image by
// RegionProposalNetwork.assign_targets_to_anchors (rpn.py), RoIHeads.assign_targets_to_proposals (roi_heads.py) and
// RetinaNet.compute_loss (retinanet.py) on box_iou(gt, boxes) (ops/boxes.py), a [G, A] matrix:
//   vals, matches = iou.max(dim=0)                       (first max over gt; NaN counts as the max)
//   matches[vals < low] = -1; matches[(vals >= low) & (vals < high)] = -2
//   allow_low_quality: best_g = iou.max(dim=1); for every (g, i) with iou[g, i] == best_g[g]: matches[i] = all_matches[i]
// The reference loops over images in Python with ~15-20 launches and one host sync (the torch.where of the restore) each.
// Here the whole batch is at most three operations on the caller's stream whatever B, N and G are, and nothing is read back:
//   0. hipMemsetAsync of the per-gt key workspace (allow_low_quality only);
//   1. match_gt_best_kernel (allow_low_quality only): per gt, the order-preserving key of its best IoU.  A block stages its
//      image's gt in LDS (in chunks of kGtChunk), computes the IoU of its kBoxesPerThread * 256 boxes, reduces per gt over the
//      wave, then through an LDS atomicMax, and issues ONE device-scope atomicMax per gt per block.  Max is order-independent,
//      so the result is reproducible; no block ever waits for another.
//   2. match_assign_kernel: per box, the IoU against every gt of its image again, the first argmax, the thresholds, the
//      restore, and the outputs.
// A block's box range may straddle images; it walks the images that overlap it (found by binary search in box_offsets).
// Arithmetic: iou() is the operation sequence of box_iou_pairwise_kernel (postprocess.hip) for float32 boxes, so every value
// is bit-identical to the reference's box_iou; the Makefile's -ffp-contract=off keeps each operation a separate rounding.
// Keys: -0.0 is folded onto +0.0 (they compare equal) and every NaN onto one key above +inf (torch's max propagates NaN), so
// the unsigned order of the keys is the float order; the raw bits would rank -0.0 above every positive IoU.
#include <climits>

#include "tvmi_common.h"

namespace tvmi {
namespace {

constexpr int kMatchThreads = 256;
constexpr int kBoxesPerThread = 4;  // pass 1: boxes per thread (one wave reduction per gt serves four boxes)
constexpr int kGtChunk = 1024;      // gt boxes staged in LDS at a time (16 KB of boxes + 4 KB of keys / best values)

__device__ __forceinline__ float iou(float ax1, float ay1, float ax2, float ay2, float area1, float bx1, float by1, float bx2,
                                     float by2, float area2) {
  auto tmax = [](float a, float b) { return (a != a || a > b) ? a : b; };  // torch.max / torch.min propagate NaN
  auto tmin = [](float a, float b) { return (a != a || a < b) ? a : b; };
  auto clamp0 = [](float v) { return v < 0.f ? 0.f : v; };                 // clamp(min=0) keeps NaN and -0.0
  const float w = clamp0(tmin(ax2, bx2) - tmax(ax1, bx1)), h = clamp0(tmin(ay2, by2) - tmax(ay1, by1));
  const float inter = w * h;
  const float uni = area1 + area2 - inter;
  return inter / uni;
}

__device__ __forceinline__ unsigned int order_key(float v) {
  if (v != v) return 0xFFFFFFFFu;
  unsigned int u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key_value(unsigned int k) {
  if (k == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// last image whose first box is <= i (offsets[0] = 0 <= i < offsets[B] = N)
__device__ __forceinline__ int image_of(const int64_t* __restrict__ offsets, int B, int64_t i) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int64_t clamp_off(int64_t v, int64_t n) { return v < 0 ? 0 : (v > n ? n : v); }

__global__ __launch_bounds__(kMatchThreads) void match_gt_best_kernel(const float4* __restrict__ boxes,
                                                                      const int64_t* __restrict__ box_off,
                                                                      const float4* __restrict__ gt,
                                                                      const int64_t* __restrict__ gt_off, int64_t N,
                                                                      int64_t M, int B, unsigned int* __restrict__ keys) {
  __shared__ float4 sg[kGtChunk];
  __shared__ unsigned int skey[kGtChunk];
  const int t = threadIdx.x, lane = t & (kWave - 1);
  const int64_t lo = (int64_t)blockIdx.x * (kMatchThreads * kBoxesPerThread);
  const int64_t hi = lo + kMatchThreads * kBoxesPerThread < N ? lo + kMatchThreads * kBoxesPerThread : N;
  for (int img = image_of(box_off, B, lo); img < B && clamp_off(box_off[img], N) < hi; ++img) {
    const int64_t b0 = clamp_off(box_off[img], N), b1 = clamp_off(box_off[img + 1], N);
    const int64_t g0 = clamp_off(gt_off[img], M), g1 = clamp_off(gt_off[img + 1], M);
    if (b1 <= b0 || g1 <= g0) continue;  // uniform over the block
    float4 bx[kBoxesPerThread];
    float area2[kBoxesPerThread];
    bool live[kBoxesPerThread];
    for (int j = 0; j < kBoxesPerThread; ++j) {
      const int64_t i = lo + j * kMatchThreads + t;
      live[j] = i >= b0 && i < b1;
      bx[j] = live[j] ? boxes[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      area2[j] = (bx[j].z - bx[j].x) * (bx[j].w - bx[j].y);
    }
    for (int64_t c0 = g0; c0 < g1; c0 += kGtChunk) {
      const int n = (int)(g1 - c0 < kGtChunk ? g1 - c0 : kGtChunk);
      __syncthreads();  // the previous chunk's keys have been flushed
      for (int k = t; k < n; k += kMatchThreads) {
        sg[k] = gt[c0 + k];
        skey[k] = 0u;
      }
      __syncthreads();
      for (int k = 0; k < n; ++k) {
        const float4 a = sg[k];
        const float area1 = (a.z - a.x) * (a.w - a.y);
        unsigned int best = 0u;  // below every real key
        for (int j = 0; j < kBoxesPerThread; ++j) {
          if (!live[j]) continue;
          const unsigned int key = order_key(iou(a.x, a.y, a.z, a.w, area1, bx[j].x, bx[j].y, bx[j].z, bx[j].w, area2[j]));
          best = key > best ? key : best;
        }
        for (int off = kWave / 2; off > 0; off >>= 1) {
          const unsigned int o = (unsigned int)__shfl_xor((int)best, off);
          best = o > best ? o : best;
        }
        if (lane == 0 && best != 0u) atomicMax(&skey[k], best);
      }
      __syncthreads();
      for (int k = t; k < n; k += kMatchThreads)
        if (skey[k] != 0u) atomicMax(&keys[c0 + k], skey[k]);
    }
  }
}

__global__ __launch_bounds__(kMatchThreads) void match_assign_kernel(
    const float4* __restrict__ boxes, const int64_t* __restrict__ box_off, const float4* __restrict__ gt,
    const int64_t* __restrict__ gt_off, const int64_t* __restrict__ gt_labels, int64_t N, int64_t M, int B, float high,
    float low, int allow_low, const unsigned int* __restrict__ keys, int64_t* __restrict__ matches,
    float4* __restrict__ matched_gt, int64_t* __restrict__ labels) {
  __shared__ float4 sg[kGtChunk];
  __shared__ float sbest[kGtChunk];
  const int t = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * kMatchThreads;
  const int64_t hi = lo + kMatchThreads < N ? lo + kMatchThreads : N;
  const int64_t i = lo + t;
  for (int img = image_of(box_off, B, lo); img < B && clamp_off(box_off[img], N) < hi; ++img) {
    const int64_t b0 = clamp_off(box_off[img], N), b1 = clamp_off(box_off[img + 1], N);
    if (b1 <= b0) continue;
    const int64_t g0 = clamp_off(gt_off[img], M), g1 = clamp_off(gt_off[img + 1], M);
    const bool mine = i >= b0 && i < b1;
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mine) b = boxes[i];
    const float area2 = (b.z - b.x) * (b.w - b.y);
    float val = 0.f;
    int arg = -1;          // first argmax, the reference's all_matches[i]
    bool restore = false;  // iou == the best of some gt
    for (int64_t c0 = g0; c0 < g1; c0 += kGtChunk) {
      const int n = (int)(g1 - c0 < kGtChunk ? g1 - c0 : kGtChunk);
      __syncthreads();
      for (int k = t; k < n; k += kMatchThreads) {
        sg[k] = gt[c0 + k];
        if (allow_low) sbest[k] = key_value(keys[c0 + k]);
      }
      __syncthreads();
      if (!mine) continue;
      for (int k = 0; k < n; ++k) {
        const float4 a = sg[k];
        const float area1 = (a.z - a.x) * (a.w - a.y);
        const float v = iou(a.x, a.y, a.z, a.w, area1, b.x, b.y, b.z, b.w, area2);
        // torch max(dim=0): NaN wins (the first one), otherwise strictly greater; ties (-0.0 == +0.0 included) keep the first
        if (arg < 0 || (v != v && val == val) || v > val) {
          val = v;
          arg = (int)(c0 - g0) + k;
        }
        if (allow_low && v == sbest[k]) restore = true;
      }
    }
    if (!mine) continue;
    int64_t m = -1;  // an image without gt: -1 everywhere
    if (arg >= 0) {
      m = arg;
      if (val < low) m = -1;
      else if (val < high) m = -2;  // val >= low here; NaN falls through both and keeps its index
      if (restore) m = arg;
    }
    matches[i] = m;
    const int64_t src = g0 + (m < 0 ? 0 : m);
    matched_gt[i] = arg >= 0 ? gt[src] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (labels) labels[i] = m >= 0 ? gt_labels[src] : (m == -1 ? 0 : -1);
  }
}

}  // namespace
}  // namespace tvmi

using namespace tvmi;

extern "C" size_t tvmi_match_boxes_workspace_bytes(int64_t M) {
  if (M <= 0) return 0;
  return ((size_t)M * sizeof(unsigned int) + 255) & ~size_t(255);
}

extern "C" int tvmi_match_boxes(const float* boxes, const int64_t* box_offsets, const float* gt, const int64_t* gt_offsets,
                                const int64_t* gt_labels, tvmi_dtype dt, int64_t N, int64_t M, int64_t B, double high,
                                double low, int allow_low_quality, int64_t* matches, float* matched_gt, int64_t* labels,
                                void* workspace, size_t workspace_bytes, void* stream) {
  TVMI_CHECK_ARG(N >= 0 && M >= 0 && B >= 0, "match_boxes: negative size");
  TVMI_CHECK_ARG(low <= high, "match_boxes: low threshold above high threshold");
  TVMI_CHECK_ARG(dt == TVMI_F32, "match_boxes: float32 boxes expected");
  TVMI_CHECK_ARG(N < INT_MAX && M < INT_MAX && B < INT_MAX, "match_boxes: size too large");
  TVMI_CHECK_ARG((gt_labels == nullptr) == (labels == nullptr), "match_boxes: gt_labels and labels go together");
  if (N == 0) return 0;
  TVMI_CHECK_ARG(B >= 1, "match_boxes: boxes without images");
  TVMI_CHECK_ARG(boxes && box_offsets && gt_offsets && matches && matched_gt && (M == 0 || gt), "match_boxes: null pointer");
  TVMI_CHECK_ARG(!allow_low_quality || M == 0 ||
                     (workspace && workspace_bytes >= tvmi_match_boxes_workspace_bytes(M) && ((uintptr_t)workspace & 255) == 0),
                 "match_boxes: workspace too small or not 256-byte aligned");
  TVMI_CHECK_ARG(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)gt & 15) == 0 && ((uintptr_t)matched_gt & 15) == 0,
                 "match_boxes: boxes, gt and matched_gt must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  unsigned int* keys = (unsigned int*)workspace;
  const bool low_quality = allow_low_quality && M > 0;
  if (low_quality) {
    const hipError_t e = hipMemsetAsync(keys, 0, (size_t)M * sizeof(unsigned int), s);
    if (e != hipSuccess) return set_error((int)e, "tvmi_match_boxes: workspace clear");
    const int64_t per = kMatchThreads * kBoxesPerThread;
    match_gt_best_kernel<<<(unsigned)((N + per - 1) / per), kMatchThreads, 0, s>>>(
        (const float4*)boxes, box_offsets, (const float4*)gt, gt_offsets, N, M, (int)B, keys);
  }
  match_assign_kernel<<<(unsigned)((N + kMatchThreads - 1) / kMatchThreads), kMatchThreads, 0, s>>>(
      (const float4*)boxes, box_offsets, (const float4*)gt, gt_offsets, gt_labels, N, M, (int)B, (float)high, (float)low,
      low_quality ? 1 : 0, keys, matches, (float4*)matched_gt, labels);
  TVMI_RETURN_LAUNCH_STATUS("tvmi_match_boxes");
}
