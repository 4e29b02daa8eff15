// Averaged-tag decode (legacy/valid_ae_avg.py:189-195): the pinned float order of the channel mean, and the launch of
// the batched mean plane that decode.hip's rtpe_ms_mean_prep puts behind the prep of the smallest scale.
#pragma once
#include <hip/hip_runtime.h>

namespace rtpe {

// PyTorch-CPU's mean(dim=1) of a (N,C,h,w) float32 tensor for one pixel, `at(c)` its value in channel c: the channels
// in blocks of 16, every block summed one channel after the other from +0.0f, the block sums added in order; the
// C % 16 channels behind the last full block summed from +0.0f on their own and added last; then ONE true division by
// float(C) (x / 17.0f is not x * (1 / 17.0f)).  This is the order of ATen's vectorised outer reduction (found by
// experiment, tests/test_tag_mean_host.py redoes the fit); the H*W % 32 pixels at the end of a plane that ATen sends
// through a scalar path with another order get THIS order here.  The order is ATen's up to C = kMeanMaxChannels = 272
// (17 blocks of 16); from C = 273 on ATen groups the blocks at one more level, which is not restated: callers refuse.
constexpr int kMeanMaxChannels = 272;

template <class F>
__device__ __forceinline__ float mean_ordered(int C, F at) {
  const int full = C & ~15;
  float blocks = 0.f;
  for (int b = 0; b < full; b += 16) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) s = s + at(b + c);
    blocks = b == 0 ? s : blocks + s;
  }
  float rest = 0.f;
  for (int c = full; c < C; ++c) rest = rest + at(c);
  const float sum = full ? rest + blocks : rest;
  return sum / (float)C;
}

// M[n0 + i] (oh, ow) for i = 0..n-1: the mean over j of rs_(oh,ow)(T[(n0 + i) * J + j]), T (planes, sh, sw) dense,
// M (images, oh, ow) dense; arguments are the caller's check (tag_mean.hip)
int launch_mean_plane(const float* T, int J, int sh, int sw, float* M, int n0, int n, int oh, int ow,
                      hipStream_t stream);

}  // namespace rtpe
