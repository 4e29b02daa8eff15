// The students' front end (include/rtpe_hip_frames.h): N uint8 HWC frames of different sizes -> the normalised fp32
// NCHW image canvas and, optionally, the LAB / HSV canvas of AttentionStudentSteps' second input, in one launch.
// Replaces, per image, torchvision ToTensor + Normalize (rtpe/dataloaders.py:346-358 of the reference), one
// rtpe_rgb_to_alt launch and the two slice copies into zeroed canvases of students.pack_mixed.  The kernel writes
// EVERY element of both canvases (0.0 outside an image), so they need no memset.  Store-bound: 3 B in, 12 or 24 B out
// per pixel.
//
// The arithmetic is that of the kernels it stands in for: (g / 255.f - mean) / stdev as warp_pixel (preprocess.hip),
// and rgb_to_alt_pixel (alt_colour.h), which rgb_to_alt_kernel calls too.
#include "rtpe_common.h"
#include "alt_colour.h"

namespace rtpe {

// One entry of the job table (device memory, 32 bytes, layout in include/rtpe_hip_frames.h)
struct FrameJob {
  unsigned long long src;     // (h, w, 3) uint8, row stride `stride` bytes
  int h, w, stride, reserved0;
  unsigned long long reserved1;
};
static_assert(sizeof(FrameJob) == 32, "FrameJob: 32-byte table entries");

struct FramesArgs {
  const FrameJob* jobs;
  float* canvas;              // (N, 3, Hc, Wc) fp32
  float* alt;                 // the same shape, or null (ALT < 0)
  int Hc, Wc;
  float mean[3], stdev[3];
};

// 16 bytes where all four floats are inside the canvas row and the address is 16-byte aligned (a plane row starts at a
// multiple of Wc floats, so for Wc % 4 != 0 the alignment changes from row to row), one float at a time elsewhere
__device__ __forceinline__ void store_row4(float* p, int x, int Wc, float v0, float v1, float v2, float v3) {
  if (x + 3 < Wc && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    *reinterpret_cast<float4*>(p) = make_float4(v0, v1, v2, v3);
    return;
  }
  const float v[4] = {v0, v1, v2, v3};
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (x + i < Wc) p[i] = v[i];
}

// Grid over the canvas, blockIdx.z = image n, whose job entry is uniform over the workgroup (scalar loads).  A workgroup
// covers 256 x 4 canvas pixels; a thread owns 4 consecutive x of one row.  ALT: -1 no second canvas, 0 LAB, 1 HSV.
// LUT (LAB only): the sRGB linearisation is read from a 256-entry LDS table that the workgroup fills with
// srgb_to_linear((float)u / 255.f), the very call the direct form makes per channel - the same bits by construction,
// 256 powf per workgroup instead of up to 3072.
template <int ALT, bool LUT>
__global__ void __launch_bounds__(256) frames_kernel(const FramesArgs a) {
  static_assert(!LUT || ALT == 0, "the table holds the sRGB linearisation of the LAB form");
  const FrameJob& j = a.jobs[blockIdx.z];
  const int h = j.h, w = j.w;
  const int x = ((int)blockIdx.x * 64 + (int)(threadIdx.x & 63)) * 4;
  const int y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
  // (uniform: a workgroup wholly outside its image reads nothing and fills no table)
  const bool wg_inside = (int)blockIdx.x * 256 < w && (int)blockIdx.y * 4 < h;
  __shared__ float lin[LUT ? 256 : 1];
  if constexpr (LUT) {
    if (wg_inside) {
      lin[threadIdx.x] = srgb_to_linear((float)threadIdx.x / 255.f);
      __syncthreads();
    }
  }
  if (x >= a.Wc || y >= a.Hc) return;
  float o[3][4], q[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) o[c][i] = q[c][i] = 0.f;
  if (wg_inside && y < h && x < w) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(j.src) + (size_t)y * (size_t)j.stride + (size_t)x * 3;
    unsigned char u[4][3];
    if (x + 3 < w && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {     // the 12 bytes of four pixels as three dwords
      const unsigned int* d = reinterpret_cast<const unsigned int*>(p);
      const unsigned int d0 = d[0], d1 = d[1], d2 = d[2];
      u[0][0] = d0 & 255; u[0][1] = (d0 >> 8) & 255; u[0][2] = (d0 >> 16) & 255;
      u[1][0] = d0 >> 24; u[1][1] = d1 & 255; u[1][2] = (d1 >> 8) & 255;
      u[2][0] = (d1 >> 16) & 255; u[2][1] = d1 >> 24; u[2][2] = d2 & 255;
      u[3][0] = (d2 >> 8) & 255; u[3][1] = (d2 >> 16) & 255; u[3][2] = d2 >> 24;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) u[i][c] = x + i < w ? p[(size_t)i * 3 + c] : (unsigned char)0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (x + i >= w) continue;
      float t[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {   // ToTensor (/255) -> Normalize ((t - mean) / std)
        t[c] = (float)u[i][c] / 255.f;
        o[c][i] = (t[c] - a.mean[c]) / a.stdev[c];
      }
      if constexpr (LUT)
        linear_to_lab(lin[u[i][0]], lin[u[i][1]], lin[u[i][2]], q[0][i], q[1][i], q[2][i]);
      else if constexpr (ALT >= 0)
        rgb_to_alt_pixel(t[0], t[1], t[2], ALT, q[0][i], q[1][i], q[2][i]);
    }
  }
  const size_t plane = (size_t)a.Hc * (size_t)a.Wc;
  const size_t at = (size_t)blockIdx.z * 3 * plane + (size_t)y * (size_t)a.Wc + (size_t)x;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    store_row4(a.canvas + at + (size_t)c * plane, x, a.Wc, o[c][0], o[c][1], o[c][2], o[c][3]);
    if constexpr (ALT >= 0) store_row4(a.alt + at + (size_t)c * plane, x, a.Wc, q[c][0], q[c][1], q[c][2], q[c][3]);
  }
}

// LAB through the LDS table or direct: the same bits; which is faster is in profiles/frames_kernel_ab.txt
// (RTPE_FRAMES_LAB_LUT=0 / 1 in the environment picks the other form, read at every call: the A/B runs in one process)
#ifndef RTPE_FRAMES_LAB_LUT
#define RTPE_FRAMES_LAB_LUT 1
#endif

}  // namespace rtpe

extern "C" int rtpe_frames_table_bytes(int32_t n_images, size_t* bytes) {
  using namespace rtpe;
  RTPE_REQUIRE(bytes, "frames_table_bytes: null argument");
  RTPE_REQUIRE(n_images > 0 && n_images <= 65535, "frames_table_bytes: n_images=%d (1..65535)", n_images);
  *bytes = sizeof(FrameJob) * (size_t)n_images;
  return RTPE_OK;
}

extern "C" int rtpe_frames_table_fill(const uint64_t* src_addr, const int32_t* src_hws, int32_t n_images, int32_t Hc,
                                      int32_t Wc, void* table, size_t table_bytes) {
  using namespace rtpe;
  RTPE_REQUIRE(src_addr && src_hws && table, "frames_table_fill: null argument");
  size_t need = 0;
  if (int rc = rtpe_frames_table_bytes(n_images, &need)) return rc;
  RTPE_REQUIRE(table_bytes >= need, "frames_table_fill: table of %zu bytes, %zu needed", table_bytes, need);
  for (int n = 0; n < n_images; ++n) {
    const int32_t h = src_hws[3 * n], w = src_hws[3 * n + 1], stride = src_hws[3 * n + 2];
    RTPE_REQUIRE(src_addr[n] && h >= 32 && w >= 32 && h <= Hc && w <= Wc && w <= INT32_MAX / 3 && stride >= 3 * w,
                 "frames_table_fill: image %d: address %#llx h=%d w=%d stride=%d in a %d x %d canvas (sides of 32 up to the "
                 "canvas's, stride >= 3 * w)", n, (unsigned long long)src_addr[n], h, w, stride, Hc, Wc);
  }
  unsigned char* jobs = reinterpret_cast<unsigned char*>(table);      // (the caller's buffer may be unaligned)
  for (int n = 0; n < n_images; ++n) {
    FrameJob j;
    memset(&j, 0, sizeof(j));
    j.src = src_addr[n];
    j.h = src_hws[3 * n];
    j.w = src_hws[3 * n + 1];
    j.stride = src_hws[3 * n + 2];
    memcpy(jobs + (size_t)n * sizeof(j), &j, sizeof(j));
  }
  return RTPE_OK;
}

extern "C" int rtpe_frames_to_canvases(const void* table_dev, int32_t n_images, int32_t Hc, int32_t Wc, const float* mean,
                                       const float* stdev, int32_t alt_mode, void* canvas, void* alt_canvas, void* stream) {
  using namespace rtpe;
  RTPE_REQUIRE(table_dev && mean && stdev && canvas, "frames_to_canvases: null argument");
  RTPE_REQUIRE(alt_mode >= -1 && alt_mode <= 1, "frames_to_canvases: alt_mode=%d (-1 none, 0 LAB, 1 HSV)", alt_mode);
  RTPE_REQUIRE((alt_canvas != nullptr) == (alt_mode >= 0), "frames_to_canvases: alt_mode=%d %s a second canvas", alt_mode,
               alt_mode >= 0 ? "needs" : "takes no");
  RTPE_REQUIRE(reinterpret_cast<uintptr_t>(table_dev) % 8 == 0, "frames_to_canvases: the table must be 8-byte aligned");
  RTPE_REQUIRE(reinterpret_cast<uintptr_t>(canvas) % 4 == 0 && reinterpret_cast<uintptr_t>(alt_canvas) % 4 == 0,
               "frames_to_canvases: the canvases must be 4-byte aligned");
  size_t need = 0;
  if (int rc = rtpe_frames_table_bytes(n_images, &need)) return rc;
  RTPE_REQUIRE(Hc >= 32 && Wc >= 32 && (Hc + 3) / 4 <= 65535, "frames_to_canvases: canvas %d x %d", Hc, Wc);
  FramesArgs a;
  a.jobs = reinterpret_cast<const FrameJob*>(table_dev);
  a.canvas = reinterpret_cast<float*>(canvas);
  a.alt = reinterpret_cast<float*>(alt_canvas);
  a.Hc = Hc;
  a.Wc = Wc;
  for (int c = 0; c < 3; ++c) {
    RTPE_REQUIRE(stdev[c] > 0.f, "frames_to_canvases: std must be positive");
    a.mean[c] = mean[c];
    a.stdev[c] = stdev[c];
  }
  const dim3 grid((Wc + 255) / 256, (Hc + 3) / 4, n_images), block(256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (alt_mode < 0)
    hipLaunchKernelGGL((frames_kernel<-1, false>), grid, block, 0, s, a);
  else if (alt_mode == 1)
    hipLaunchKernelGGL((frames_kernel<1, false>), grid, block, 0, s, a);
  else if (env_int("RTPE_FRAMES_LAB_LUT", RTPE_FRAMES_LAB_LUT))
    hipLaunchKernelGGL((frames_kernel<0, true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((frames_kernel<0, false>), grid, block, 0, s, a);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}
