// Averaged-tag decode (the reference's legacy/valid_ae_avg.py:189-195): every joint of an image is grouped by ONE tag
// map, the mean of the J un-mirrored tag maps, `tags[0].mean(dim=1)` on the CPU.  Two kernels, both bit-equal to that
// op (compiled with -ffp-contract=off; the order is mean_ordered of tag_mean.h):
//   * channel_mean_kernel: (N,C,h,w) -> (N,h,w), the public op (rtpe_channel_mean).  Memory-bound: one coalesced read
//     of every plane, one write;
//   * mean_plane_kernel: the batched decode's plane M = mean_j rs_(oh,ow)(T_j) from the tag maps T at the refined size
//     of the smallest scale, which the prep kernel of that scale wrote (decode.hip): per pixel the two axis entries
//     once, J samples with resize_nc.h's arithmetic, reduced in registers, one write.  The (N,J,oh,ow) tensor that the
//     per-image chain builds is never written.
// No atomics: one thread owns one output pixel.
#include "rtpe_common.h"
#include "resize_nc.h"
#include "tag_mean.h"
#include "rtpe_hip.h"

namespace rtpe {

__global__ void __launch_bounds__(256) channel_mean_kernel(const float* __restrict__ x, long long img_st,
                                                           long long ch_st, int C, int npix,
                                                           float* __restrict__ out) {
  const float* b = x + (size_t)blockIdx.y * img_st;
  float* o = out + (size_t)blockIdx.y * npix;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256)
    o[i] = mean_ordered(C, [&](int c) { return b[(size_t)c * ch_st + i]; });
}

struct MeanPlaneArgs {
  const float* T;     // (planes, sh, sw): plane (n0 + blockIdx.y) * J + j
  float* M;           // (images, oh, ow)
  int J, sh, sw, oh, ow, n0;
  float sy, sx;       // float(in) / float(out)
};

__global__ void __launch_bounds__(256) mean_plane_kernel(const MeanPlaneArgs a) {
  const int n = a.n0 + blockIdx.y, npix = a.oh * a.ow;
  const size_t src_plane = (size_t)a.sh * a.sw;
  const float* T = a.T + (size_t)n * a.J * src_plane;
  float* M = a.M + (size_t)n * npix;
  const bool ident = a.sh == a.oh && a.sw == a.ow;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
    const int y = i / a.ow, x = i - y * a.ow;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    axis_nc(a.sy, a.sh, a.oh, y, &y0, &y1, &ly0, &ly1);
    axis_nc(a.sx, a.sw, a.ow, x, &x0, &x1, &lx0, &lx1);
    M[i] = mean_ordered(a.J, [&](int j) {
      return taps_nc(T + (size_t)j * src_plane, a.sw, ident, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
    });
  }
}

static dim3 pixel_grid(int npix, int images) {
  return dim3((npix + 255) / 256 < 1024 ? (npix + 255) / 256 : 1024, images);
}

int launch_mean_plane(const float* T, int J, int sh, int sw, float* M, int n0, int n, int oh, int ow,
                      hipStream_t stream) {
  MeanPlaneArgs a;
  a.T = T; a.M = M; a.J = J; a.sh = sh; a.sw = sw; a.oh = oh; a.ow = ow; a.n0 = n0;
  a.sy = (float)sh / (float)oh;
  a.sx = (float)sw / (float)ow;
  hipLaunchKernelGGL(mean_plane_kernel, pixel_grid(oh * ow, n), dim3(256), 0, stream, a);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

}  // namespace rtpe

using namespace rtpe;

extern "C" int rtpe_channel_mean(const float* x, int32_t N, int32_t C, int32_t h, int32_t w, int64_t img_stride,
                                 int64_t ch_stride, float* out, void* stream) {
  RTPE_REQUIRE(x && out, "channel_mean: null argument");
  RTPE_REQUIRE(N > 0 && N <= 65535 && C > 0 && C <= kMeanMaxChannels && h > 0 && w > 0 &&
                   (int64_t)h * w < 0x7fffffff,
               "channel_mean: bad shape (%d, %d, %d, %d): 1 <= N <= 65535, 1 <= C <= %d (beyond that PyTorch-CPU's "
               "mean takes an order that is not pinned here)", N, C, h, w, kMeanMaxChannels);
  RTPE_REQUIRE(ch_stride >= (int64_t)h * w && img_stride >= (int64_t)(C - 1) * ch_stride + (int64_t)h * w,
               "channel_mean: a stride is shorter than what it steps over (planes are dense, channels and images "
               "must not overlap)");
  hipLaunchKernelGGL(channel_mean_kernel, pixel_grid(h * w, N), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     x, (long long)img_stride, (long long)ch_stride, C, h * w, out);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}
