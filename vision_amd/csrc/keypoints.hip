// keypoints.hip — Keypoint R-CNN inference decoding for every detection at once, for gfx950.
//
// Reference: torchvision 0.30 models/detection/roi_heads.py, keypointrcnn_inference -> heatmaps_to_keypoints.  For each
// detection i the reference runs, in a Python loop with two blocking .item() reads and about a dozen launches:
//   w = clamp(x2 - x1, min=1), h = clamp(y2 - y1, min=1); OW = int(ceil(w)), OH = int(ceil(h)); wc = w / OW, hc = h / OH
//   roi_map = F.interpolate(maps[i][:, None], size=(OH, OW), mode="bicubic", align_corners=False)   (maps' dtype)
//   pos = roi_map.reshape(K, -1).argmax(1)            (first index of the max; NaN counts as the max)
//   xy[i] = ((pos % OW + 0.5) * wc + x1, (pos // OW + 0.5) * hc + y1, 1), score[i] = roi_map[k, pos]
// Here the whole batch is three launches whatever R and the box sizes are, and the host reads nothing back:
//   1. kp_plan_kernel (one workgroup): each ROI's OW, OH, wc, hc from the device rois (the reference's float32 operations
//      in its order), its chunk count, the exclusive scan of the counts, and the zeroed [R, K] key buffer.
//   2. kp_search_kernel (a persistent grid sized from the CU count, not from R): grid-strides over the chunk ids and finds
//      a chunk's ROI by binary search in the scan.  A chunk is CW output columns x G*RB output rows of one ROI, for all K
//      keypoints (CW = the power of two >= OW, at most 256; G = 256 / CW row groups; RB <= 8 rows per thread), so one
//      full-image box is spread over hundreds of workgroups.  Thread t owns column t % CW and RB consecutive rows.
//   3. kp_decode_kernel: keys -> xy [R, 3, K] and scores [R, K].
// Arithmetic: every upsampled value is bit-identical to bicubic2d_kernel (resize.hip), the per-output form of
// tvmi_upsample_bicubic2d: the same source_index / floor / clamp / cubic1 / cubic2, each input row's horizontal sum
// ld(x0)*cx0 + ld(x1)*cx1 + ld(x2)*cx2 + ld(x3)*cx3 left to right, rows combined as acc = +0.0f; acc += r_k * cy_k, and the
// same-size copy when (OH, OW) == (H, W).  The evaluation is separable: a thread keeps the horizontal sums of the four
// input rows its current output row needs in registers and slides that window down its rows, so each input row's sum is
// computed once per column and the vertical combine costs 8 flops per output.  The chunk's input patch (the taps of its
// first and last rows and columns) is staged in LDS for a batch of keypoints when one keypoint's patch fits in 32 KB; a
// larger patch (huge maps, strong downsampling) is read from global memory / L2, so any H, W >= 1 works.
// Argmax: each value is rounded to the map dtype (the reference's fp16 / bf16 roi_map) and widened back; a thread keeps
// its first maximum (NaN beats everything, the first NaN wins), the wave and the workgroup reduce 64-bit keys
//   ord(value) << 32 | (0xFFFFFFFF - flat index)     (ord: order-preserving bits, -0.0 == +0.0, every NaN the largest)
// and ONE device-scope atomicMax per chunk and keypoint merges them.  The maximum key does not depend on arrival order,
// so results are bitwise reproducible.
// Limits: any K >= 1, H, W >= 1 with H * W < 2^31; a per-ROI map of up to 2^31 - 1 pixels.  An ROI with a non-finite
// coordinate, or a larger map, gets NaN x, y and score (column 2 stays 1); the launch does not fail (the reference raises
// inside int(nan)).  The -ffp-contract=off of the Makefile keeps every operation above a separate rounding.
#include <algorithm>
#include <climits>
#include <cmath>
#include <mutex>

#include "resample_common.h"
#include "tvmi_common.h"

namespace tvmi {
namespace {

constexpr int kKpThreads = 256;     // one chunk per workgroup
constexpr int kKpLog2Threads = 8;
constexpr int kKpRows = 8;          // RB: output rows per thread at most
constexpr int kPlanThreads = 1024;
constexpr int kPatchFloats = 8192;  // 32 KB of LDS: the input patch of a chunk for a batch of keypoints

struct KpPlan {
  float x1, y1, wc, hc, sw, sh;
  int OW, OH;
  int cw_log2;  // chunk columns CW = 1 << cw_log2
  int ncx;      // column strips of the ROI
  int rb;       // rows per thread
  int flags;    // kValid | kCopy
};
constexpr int kValid = 1, kCopy = 2;

inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }
inline size_t keys_bytes(int64_t R, int64_t K) { return align256((size_t)R * (size_t)K * sizeof(unsigned long long)); }
inline size_t start_bytes(int64_t R) { return align256((size_t)(R + 1) * sizeof(long long)); }

__global__ __launch_bounds__(kPlanThreads) void kp_plan_kernel(const float* __restrict__ rois, int R, int K, int H, int W,
                                                               KpPlan* __restrict__ plan, long long* __restrict__ start,
                                                               unsigned long long* __restrict__ keys) {
  __shared__ long long wave_sum[kPlanThreads / kWave];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  for (int64_t i = t; i < (int64_t)R * K; i += kPlanThreads) keys[i] = 0ull;
  long long carry = 0;
  for (int base = 0; base < R; base += kPlanThreads) {
    const int r = base + t;
    long long n = 0;
    if (r < R) {
      const float x1 = rois[4 * (int64_t)r], y1 = rois[4 * (int64_t)r + 1];
      const float x2 = rois[4 * (int64_t)r + 2], y2 = rois[4 * (int64_t)r + 3];
      float w = x2 - x1, h = y2 - y1;
      w = w < 1.f ? 1.f : w;  // torch.clamp(min=1): NaN stays NaN
      h = h < 1.f ? 1.f : h;
      const float wceil = ceilf(w), hceil = ceilf(h);
      KpPlan p;
      p.x1 = x1;
      p.y1 = y1;
      p.flags = 0;
      p.OW = p.OH = 1;
      p.wc = p.hc = p.sw = p.sh = 0.f;
      p.cw_log2 = 0;
      p.ncx = p.rb = 1;
      const bool finite = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && isfinite(w) && isfinite(h);
      if (finite && (double)wceil * (double)hceil <= 2147483647.0) {
        p.OW = (int)wceil;
        p.OH = (int)hceil;
        p.wc = w / (float)p.OW;
        p.hc = h / (float)p.OH;
        p.sw = compute_scale(W, p.OW, false, -1.0);
        p.sh = compute_scale(H, p.OH, false, -1.0);
        int cl = 0;
        while (cl < kKpLog2Threads && (1 << cl) < p.OW) ++cl;
        const int groups = kKpThreads >> cl;
        p.cw_log2 = cl;
        p.ncx = (p.OW - 1) / (1 << cl) + 1;
        p.rb = std::min(kKpRows, (p.OH - 1) / groups + 1);
        p.flags = kValid | ((p.OH == H && p.OW == W) ? kCopy : 0);
        n = (long long)p.ncx * (((long long)p.OH - 1) / ((long long)groups * p.rb) + 1);
      }
      plan[r] = p;
    }
    long long v = n;  // inclusive scan of the chunk counts: wave, then across the waves of the workgroup
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const long long u = __shfl_up(v, d);
      if (lane >= d) v += u;
    }
    if (lane == kWave - 1) wave_sum[wv] = v;
    __syncthreads();
    long long before = carry, tile = 0;
    for (int j = 0; j < kPlanThreads / kWave; ++j) {
      before += j < wv ? wave_sum[j] : 0;
      tile += wave_sum[j];
    }
    if (r < R) start[r] = before + v - n;
    carry += tile;
    __syncthreads();
  }
  if (t == 0) start[R] = carry;
}

// order-preserving bits: -0.0 == +0.0, every NaN above +inf
__device__ __forceinline__ unsigned ord_bits(float v) {
  if (v != v) return 0xFFFFFFFFu;
  const unsigned u = __float_as_uint(v + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float from_ord_bits(unsigned o) {
  if (o == 0xFFFFFFFFu) return __builtin_nanf("");
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// the value the reference's roi_map holds: rounded to the map dtype, widened back
template <typename T>
__device__ __forceinline__ float in_map_dtype(float v) {
  T s;
  st(&s, v);
  return ld(&s);
}

// horizontal sum of one input row: bicubic2d_kernel's `r`, from the map or from its copy in LDS (same values, same operations)
template <typename T>
__device__ __forceinline__ float row_sum(const T* __restrict__ row, const int (&xx)[4], const float (&cx)[4]) {
  return ld(row + xx[0]) * cx[0] + ld(row + xx[1]) * cx[1] + ld(row + xx[2]) * cx[2] + ld(row + xx[3]) * cx[3];
}

// first input tap of output index o along an axis (bicubic2d_kernel: source_index, floor, min)
__device__ __forceinline__ int first_tap(float scale, int o, int in) {
  return min((int)floorf(source_index(scale, o, false, true)), in - 1);
}

template <typename T>
__global__ __launch_bounds__(kKpThreads) void kp_search_kernel(const T* __restrict__ maps, const KpPlan* __restrict__ plan,
                                                               const long long* __restrict__ start,
                                                               unsigned long long* __restrict__ keys, int R, int K, int H,
                                                               int W) {
  __shared__ unsigned long long red[2][kKpThreads / kWave];
  __shared__ float patch[kPatchFloats];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const float A = -0.75f;
  const long long total = start[R];
  int phase = 0;  // parity of the workgroup's reductions: the red[] slot written after a barrier is never the one read before it
  for (long long c = blockIdx.x; c < total; c += gridDim.x) {
    int lo = 0, hi = R - 1;  // the last ROI with start[r] <= c (an empty ROI has start[r] == start[r + 1])
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (start[mid] <= c) lo = mid;
      else hi = mid - 1;
    }
    const KpPlan p = plan[lo];
    const long long local = c - start[lo];
    const int sx = (int)(local % p.ncx);
    const long long sy = local / p.ncx;
    const int cw = 1 << p.cw_log2;
    const int ox = sx * cw + (t & (cw - 1));
    const long long oy0 = (sy * (kKpThreads >> p.cw_log2) + (t >> p.cw_log2)) * p.rb;
    const int nrows = ox < p.OW ? (int)std::max<long long>(0, std::min<long long>(p.rb, p.OH - oy0)) : 0;
    // horizontal taps of the thread's column, vertical taps of its rows: bicubic2d_kernel's index arithmetic
    float cx[4];
    int xx[4];
    {
      const float rx = source_index(p.sw, min(ox, p.OW - 1), false, true);
      const int ix = min((int)floorf(rx), W - 1);
      const float tx = fminf(fmaxf(rx - (float)ix, 0.f), 1.f);
      cx[0] = cubic2(tx + 1.f, A);
      cx[1] = cubic1(tx, A);
      cx[2] = cubic1(1.f - tx, A);
      cx[3] = cubic2(1.f - tx + 1.f, A);
#pragma unroll
      for (int k = 0; k < 4; ++k) xx[k] = max(min(ix - 1 + k, W - 1), 0);
    }
    float cy[kKpRows][4];
    int y_first[kKpRows];  // unclamped index of the row's first input tap
#pragma unroll
    for (int j = 0; j < kKpRows; ++j) {
      const int oy = (int)std::min<long long>(oy0 + j, p.OH - 1);
      const float ry = source_index(p.sh, oy, false, true);
      const int iy = min((int)floorf(ry), H - 1);
      const float ty = fminf(fmaxf(ry - (float)iy, 0.f), 1.f);
      cy[j][0] = cubic2(ty + 1.f, A);
      cy[j][1] = cubic1(ty, A);
      cy[j][2] = cubic1(1.f - ty, A);
      cy[j][3] = cubic2(1.f - ty + 1.f, A);
      y_first[j] = iy - 1;
    }
    const bool copy = (p.flags & kCopy) != 0;
    // The chunk's input patch: the taps of its first and last rows / columns bound every tap of the chunk (the tap index
    // is monotone in the output index).  Batches of kb keypoints' patches are staged in LDS with all their loads in flight,
    // so a (chunk, keypoint) pays no dependent global-load latency; kb == 0 (patch above 32 KB, or the copy path): the
    // taps are read from global memory directly.
    const int groups = kKpThreads >> p.cw_log2;
    const int oy_a = (int)(sy * groups * p.rb), oy_b = (int)std::min<long long>(sy * groups * p.rb + groups * p.rb, p.OH) - 1;
    const int ox_a = sx * cw, ox_b = min(ox_a + cw, p.OW) - 1;
    const int ylo = max(first_tap(p.sh, oy_a, H) - 1, 0), yhi = min(first_tap(p.sh, oy_b, H) + 2, H - 1);
    const int xlo = max(first_tap(p.sw, ox_a, W) - 1, 0), xhi = min(first_tap(p.sw, ox_b, W) + 2, W - 1);
    const int nc = xhi - xlo + 1, P = (yhi - ylo + 1) * nc;
    const int kb = copy ? 0 : min(K, kPatchFloats / P);
    int xs[4];  // the thread's tap columns inside the patch
#pragma unroll
    for (int q = 0; q < 4; ++q) xs[q] = xx[q] - xlo;
    const int64_t HW = (int64_t)H * W;
    for (int k0 = 0, k1 = 0; k0 < K; k0 = k1) {
      k1 = kb > 0 ? min(K, k0 + kb) : K;
      if (kb > 0) {  // every thread is past the last barrier of the previous batch: no read of the old patch is pending
        const T* __restrict__ src = maps + ((int64_t)lo * K + k0) * HW + (int64_t)ylo * W + xlo;
        const int n = (k1 - k0) * P;
#pragma unroll 4
        for (int i = t; i < n; i += kKpThreads) {
          const int kk = i / P, rem = i - kk * P, r = rem / nc;
          patch[i] = ld(src + kk * HW + (int64_t)r * W + (rem - r * nc));
        }
        __syncthreads();
      }
    for (int k = k0; k < k1; ++k) {
      const T* __restrict__ m = maps + ((int64_t)lo * K + k) * HW;
      const float* __restrict__ pk = patch + (k - k0) * P;
      float best = 0.f;
      int best_j = -1;
      if (copy) {
        for (int j = 0; j < nrows; ++j) {
          const float v = ld(m + (oy0 + j) * W + ox);
          if (best_j < 0 || v > best || (v != v && best == best)) {
            best = v;
            best_j = j;
          }
        }
      } else {
        float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;  // horizontal sums of input rows wb .. wb + 3 (clamped into the map)
        int wb = INT_MIN / 2;
#pragma unroll
        for (int j = 0; j < kKpRows; ++j) {
          if (j < nrows) {
            const int need = y_first[j];  // non-decreasing in j
            if (need - wb >= 4) wb = need - 4;
            while (wb < need) {
              w0 = w1;
              w1 = w2;
              w2 = w3;
              const int row = max(min(wb + 4, H - 1), 0);
              w3 = kb > 0 ? row_sum(pk + (row - ylo) * nc, xs, cx) : row_sum(m + (int64_t)row * W, xx, cx);
              ++wb;
            }
            float acc = 0.f;
            acc += w0 * cy[j][0];
            acc += w1 * cy[j][1];
            acc += w2 * cy[j][2];
            acc += w3 * cy[j][3];
            const float v = in_map_dtype<T>(acc);
            if (best_j < 0 || v > best || (v != v && best == best)) {
              best = v;
              best_j = j;
            }
          }
        }
      }
      unsigned long long key = 0ull;
      if (best_j >= 0) {
        const unsigned idx = (unsigned)((oy0 + best_j) * p.OW + ox);
        key = ((unsigned long long)ord_bits(best) << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
      }
#pragma unroll
      for (int d = kWave / 2; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d);
        key = o > key ? o : key;
      }
      if (lane == 0) red[phase][wv] = key;
      __syncthreads();
      if (t == 0) {
#pragma unroll
        for (int j = 1; j < kKpThreads / kWave; ++j) key = red[phase][j] > key ? red[phase][j] : key;
        if (key != 0ull) atomicMax(keys + (int64_t)lo * K + k, key);
      }
      phase ^= 1;
    }
    }
  }
}

__global__ __launch_bounds__(256) void kp_decode_kernel(const KpPlan* __restrict__ plan,
                                                        const unsigned long long* __restrict__ keys, float* __restrict__ xy,
                                                        float* __restrict__ scores, int64_t R, int64_t K) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= R * K) return;
  const int64_t r = i / K, k = i - r * K;
  const KpPlan p = plan[r];
  const unsigned long long key = keys[i];
  float x = __builtin_nanf(""), y = x, s = x;
  if ((p.flags & kValid) && key != 0ull) {
    const unsigned idx = 0xFFFFFFFFu - (unsigned)key;
    const int x_int = (int)(idx % (unsigned)p.OW), y_int = (int)(idx / (unsigned)p.OW);
    x = ((float)x_int + 0.5f) * p.wc + p.x1;
    y = ((float)y_int + 0.5f) * p.hc + p.y1;
    s = from_ord_bits((unsigned)(key >> 32));
  }
  xy[(r * 3 + 0) * K + k] = x;
  xy[(r * 3 + 1) * K + k] = y;
  xy[(r * 3 + 2) * K + k] = 1.f;
  scores[i] = s;
}

// workgroups of the persistent search grid: 4 per CU of the current device (queried once per device)
int search_groups() {
  static std::mutex mu;
  static int groups[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    (void)hipGetLastError();
    return 4 * 256;
  }
  std::lock_guard<std::mutex> lock(mu);
  if (groups[dev] == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    groups[dev] = 4 * cus;
  }
  return groups[dev];
}

}  // namespace
}  // namespace tvmi

using namespace tvmi;

extern "C" size_t tvmi_heatmaps_to_keypoints_workspace_bytes(int64_t R, int64_t K) {
  if (R <= 0 || K <= 0) return 0;
  return keys_bytes(R, K) + start_bytes(R) + align256((size_t)R * sizeof(KpPlan));
}

extern "C" int tvmi_heatmaps_to_keypoints(const void* maps, const float* rois, float* xy, float* scores, tvmi_dtype dt,
                                          int64_t R, int64_t K, int64_t H, int64_t W, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  TVMI_CHECK_ARG(R >= 0 && K >= 1 && H >= 1 && W >= 1, "heatmaps_to_keypoints: R >= 0, K >= 1, H >= 1, W >= 1 expected");
  if (R == 0) return 0;
  TVMI_CHECK_ARG(maps && rois && xy && scores && workspace, "heatmaps_to_keypoints: null pointer");
  TVMI_CHECK_ARG(R < INT_MAX && K < INT_MAX && R * K <= INT_MAX && H * W < (1ll << 31),
                 "heatmaps_to_keypoints: size too large");
  TVMI_CHECK_ARG(workspace_bytes >= tvmi_heatmaps_to_keypoints_workspace_bytes(R, K) &&
                     ((uintptr_t)workspace & 255) == 0,
                 "heatmaps_to_keypoints: workspace too small or not 256-byte aligned");
  TVMI_CHECK_ARG(dt == TVMI_F32 || dt == TVMI_F16 || dt == TVMI_BF16, "heatmaps_to_keypoints: unsupported dtype");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned long long* keys = (unsigned long long*)ws;
  long long* start = (long long*)(ws + keys_bytes(R, K));
  KpPlan* plan = (KpPlan*)(ws + keys_bytes(R, K) + start_bytes(R));
  kp_plan_kernel<<<1, kPlanThreads, 0, s>>>(rois, (int)R, (int)K, (int)H, (int)W, plan, start, keys);
  const dim3 grid((unsigned)search_groups());
  if (dt == TVMI_F32)
    kp_search_kernel<float><<<grid, kKpThreads, 0, s>>>((const float*)maps, plan, start, keys, (int)R, (int)K, (int)H, (int)W);
  else if (dt == TVMI_F16)
    kp_search_kernel<__half><<<grid, kKpThreads, 0, s>>>((const __half*)maps, plan, start, keys, (int)R, (int)K, (int)H, (int)W);
  else
    kp_search_kernel<__hip_bfloat16><<<grid, kKpThreads, 0, s>>>((const __hip_bfloat16*)maps, plan, start, keys, (int)R,
                                                                 (int)K, (int)H, (int)W);
  kp_decode_kernel<<<(unsigned)ceil_div(R * K, 256), 256, 0, s>>>(plan, keys, xy, scores, R, K);
  TVMI_RETURN_LAUNCH_STATUS("tvmi_heatmaps_to_keypoints");
}
