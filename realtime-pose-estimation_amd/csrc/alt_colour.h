// The alternative colour spaces of one pixel: skimage.color.rgb2lab / rgb2hsv on fp32 RGB in [0, 1]
// (rtpe/dataloaders.py:352-356 of the reference; constants of skimage.color.colorconv).  Written once: rgb_to_alt_kernel
// (student_ops.hip) and frames_kernel (frames.hip) both call rgb_to_alt_pixel, so the frames front end gives the bits of
// rtpe_rgb_to_alt by construction.  The build has -ffp-contract=off: every product and sum below is rounded on its own.
#pragma once
#include <hip/hip_runtime.h>

namespace rtpe {

// sRGB -> linear, one channel.  Its argument has 256 possible values for a uint8 frame (u / 255.f): frames_kernel may
// read it from a table that this same function filled.
__device__ __forceinline__ float srgb_to_linear(float v) {
  return v > 0.04045f ? powf((v + 0.055f) / 1.055f, 2.4f) : v / 12.92f;
}

// linear RGB -> XYZ (D65) -> Lab
__device__ __forceinline__ void linear_to_lab(float R, float G, float B, float& o0, float& o1, float& o2) {
  float X = 0.412453f * R + 0.357580f * G + 0.180423f * B;
  float Y = 0.212671f * R + 0.715160f * G + 0.072169f * B;
  float Z = 0.019334f * R + 0.119193f * G + 0.950227f * B;
  X /= 0.95047f; Z /= 1.08883f;
  auto f = [](float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + 16.f / 116.f; };
  const float fx = f(X), fy = f(Y), fz = f(Z);
  o0 = 116.f * fy - 16.f;
  o1 = 500.f * (fx - fy);
  o2 = 200.f * (fy - fz);
}

__device__ __forceinline__ void rgb_to_hsv(float r, float g, float bl, float& o0, float& o1, float& o2) {
  const float mx = fmaxf(r, fmaxf(g, bl)), mn = fminf(r, fminf(g, bl));
  const float d = mx - mn;
  float h = 0.f;
  if (d != 0.f) {
    if (mx == r) h = (g - bl) / d;
    else if (mx == g) h = 2.f + (bl - r) / d;
    else h = 4.f + (r - g) / d;
    h = h / 6.f;
    h = h - floorf(h);                                   // (h / 6) % 1
  }
  o0 = h;
  o1 = d == 0.f ? 0.f : d / mx;
  o2 = mx;
}

// mode 0: LAB, 1: HSV (rtpe_rgb_to_alt's `mode`)
__device__ __forceinline__ void rgb_to_alt_pixel(float r, float g, float bl, int mode, float& o0, float& o1, float& o2) {
  if (mode == 0)
    linear_to_lab(srgb_to_linear(r), srgb_to_linear(g), srgb_to_linear(bl), o0, o1, o2);
  else
    rgb_to_hsv(r, g, bl, o0, o1, o2);
}

}  // namespace rtpe
