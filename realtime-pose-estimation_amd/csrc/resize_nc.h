// F.interpolate(mode="bilinear", align_corners=False) with PyTorch-CPU's arithmetic, shared by the aggregation
// kernel (aggregate.hip) and the flip-test decode samplers (decode.hip), so that both produce the same bits:
//   * source index  real = fma(scale, o + 0.5, -0.5) (ATen's CPU build contracts the expression), clamped at 0,
//     scale = float(in) / float(out);  i0 = floor(real), i1 = i0 + (i0 < in - 1), l1 = real - i0, l0 = 1 - l1;
//   * value  T = fma(v0, lx0, v1 * lx1) per row, out = fma(T0, ly0, T1 * ly1);
//   * the identity (a plain copy) when both sizes agree.
#pragma once
#include <hip/hip_runtime.h>

namespace rtpe {

__device__ __forceinline__ void axis_nc(float scale, int n_in, int n_out, int o, int* i0, int* i1, float* l0, float* l1) {
  if (n_in == n_out) { *i0 = *i1 = o; *l0 = 1.f; *l1 = 0.f; return; }
  float real = __builtin_fmaf(scale, (float)o + 0.5f, -0.5f);   // ATen's build contracts scale * (o + 0.5) - 0.5
  real = real < 0.f ? 0.f : real;
  int a = (int)real;
  a = a < n_in - 1 ? a : n_in - 1;
  *i0 = a;
  *i1 = a + (a < n_in - 1 ? 1 : 0);
  float l = real - (float)a;
  l = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);             // guard_index_and_lambda
  *l1 = l;
  *l0 = 1.f - l;
}

// one output value from a plane `b` of row length w: the copy when `ident` (both sizes agree), else the four taps
__device__ __forceinline__ float taps_nc(const float* b, int w, bool ident, int y0, int y1, int x0, int x1, float ly0,
                                         float ly1, float lx0, float lx1) {
  if (ident) return b[(size_t)y0 * w + x0];
  const float v00 = b[(size_t)y0 * w + x0], v01 = b[(size_t)y0 * w + x1];
  const float v10 = b[(size_t)y1 * w + x0], v11 = b[(size_t)y1 * w + x1];
  const float t0 = __builtin_fmaf(v00, lx0, v01 * lx1);
  const float t1 = __builtin_fmaf(v10, lx0, v11 * lx1);
  return __builtin_fmaf(t0, ly0, t1 * ly1);
}

}  // namespace rtpe
