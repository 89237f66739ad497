// resample_common.h — the scale / source-index rules and cubic convolution coefficients of PyTorch core's
// interpolation (torch 2.10.0), shared by resize.hip and keypoints.hip so that both round the same way.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tvmi {

// UpSample.h:259-287
__device__ __host__ inline float compute_scale(int64_t in, int64_t out, bool align, double scale_arg) {
  if (align) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  return scale_arg > 0. ? (float)(1.0 / scale_arg) : (float)in / (float)out;
}

// UpSample.h:289-318
__device__ __forceinline__ float source_index(float scale, int dst, bool align, bool cubic) {
  if (align) return scale * (float)dst;
  const float s = scale * ((float)dst + 0.5f) - 0.5f;
  return (!cubic && s < 0.f) ? 0.f : s;
}

// UpSample.h:400-435 (A = -0.75 for bicubic)
__device__ __forceinline__ float cubic1(float x, float A) { return ((A + 2) * x - (A + 3)) * x * x + 1; }
__device__ __forceinline__ float cubic2(float x, float A) { return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A; }

}  // namespace tvmi
