// Pre-processing on the GPU: the step in front of the hot path.
// Replaces, for one uint8 HWC image, transforms.py:181-192 `resize_align_multi_scale`
// (cv2.warpAffine with the 2x3 matrix of get_affine_transform :59-93, rot = 0) followed by
// torchvision ToTensor + Normalize (validate_hhrnet.py:63-67, teacher_inference.py:70-73):
// uint8 HWC in, normalised NCHW fp32 out, one pass, no intermediate image.
//
// Sampling convention (cv2 is not available to pin its INTER_LINEAR fixed-point scheme, so this
// is the documented convention of THIS implementation): destination pixel (x, y) samples the
// source at  M_inv * (x, y, 1)  (pixel centres at integer coordinates, as warpAffine),
// bilinear weights in fp32 (cv2 quantises them to 1/32), out-of-image taps contribute 0
// (BORDER_CONSTANT).  With round_u8 the interpolated value is rounded to a grey level
// (floor(v + 0.5), clamped to [0, 255]) before ToTensor, because the reference's warp returns a
// uint8 image (transforms.py:185-190); ToTensor and Normalize are the true divisions torchvision
// performs (x / 255, then (x - mean) / std).  HBM-bound: 3 B in, 12 B out per pixel.
//
// Two kernels around one per-pixel function (warp_pixel): warp_normalize_kernel for one image, its arguments in the
// kernel-argument segment (rtpe_warp_normalize), and warp_normalize_batch_kernel for every image of a chunk at one scale,
// its per-image arguments in a job table in device memory (rtpe_warp_normalize_batch, include/rtpe_hip_warp.h).
#include "rtpe_common.h"

namespace rtpe {

struct WarpArgs {
  const unsigned char* src;   // (h, w, 3) uint8, row stride `stride` bytes
  float* dst;                 // (3, oh, ow) fp32
  int h, w, stride, oh, ow;
  float m[6];                 // dst -> src:  sx = m0*x + m1*y + m2,  sy = m3*x + m4*y + m5
  float mean[3], stdev[3];
  int round_u8;
};

// One entry of the batched warp's job table (device memory, 64 bytes, layout in include/rtpe_hip_warp.h): job
// (scale s, image n) is entry s * n_images + n.
struct WarpJob {
  unsigned long long src;     // (h, w, 3) uint8, row stride `stride` bytes
  int h, w, stride, reserved0;
  float m[6];                 // dst -> src, as WarpArgs::m
  unsigned long long dst;     // this job's (3, H_s, W_s) fp32 planes
  unsigned long long reserved1;
};
static_assert(sizeof(WarpJob) == 64, "WarpJob: 64-byte table entries");

struct WarpBatchArgs {
  const WarpJob* jobs;        // the n_images entries of ONE scale
  int oh, ow;
  float mean[3], stdev[3];
  int round_u8;
};

// The arithmetic of one destination pixel, written once: both kernels call it, so the batched warp gives the bits of
// the one-image warp by construction.  out[c] = normalised channel c of destination pixel (x, y).
__device__ __forceinline__ void warp_pixel(const unsigned char* src, int h, int w, int stride, const float* m,
                                           const float* mean, const float* stdev, int round_u8, int x, int y,
                                           float* out) {
  const float sx = __builtin_fmaf(m[0], (float)x, __builtin_fmaf(m[1], (float)y, m[2]));
  const float sy = __builtin_fmaf(m[3], (float)x, __builtin_fmaf(m[4], (float)y, m[5]));
  const float fx = floorf(sx), fy = floorf(sy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float lx = sx - fx, ly = sy - fy;
  float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int xx = x0 + dx, yy = y0 + dy;
      const float wgt = (dx ? lx : 1.f - lx) * (dy ? ly : 1.f - ly);
      if ((unsigned)xx < (unsigned)w && (unsigned)yy < (unsigned)h) {
        const unsigned char* p = src + (size_t)yy * stride + xx * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = __builtin_fmaf(wgt, (float)p[c], v[c]);
      }
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) {   // [uint8 image] -> ToTensor (/255) -> Normalize ((t - mean) / std)
    float g = v[c];
    if (round_u8) g = fminf(fmaxf(floorf(g + 0.5f), 0.f), 255.f);
    out[c] = (g / 255.f - mean[c]) / stdev[c];
  }
}

__global__ void __launch_bounds__(256) warp_normalize_kernel(const WarpArgs a) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.ow || y >= a.oh) return;
  float o[3];
  warp_pixel(a.src, a.h, a.w, a.stride, a.m, a.mean, a.stdev, a.round_u8, x, y, o);
#pragma unroll
  for (int c = 0; c < 3; ++c) a.dst[((size_t)c * a.oh + y) * a.ow + x] = o[c];
}

// Every image of a chunk at one scale in one launch: blockIdx.z = image n, whose job entry (uniform over the
// workgroup: scalar loads) names its source and its destination planes.  A thread computes XPT consecutive x of one
// row; with XPT == 4 it stores them as one 16-byte store per channel where all four are inside the row and the
// address is 16-byte aligned (a plane row starts at a multiple of ow floats, so for ow % 4 != 0 the alignment changes
// from row to row), and one float at a time elsewhere.
#ifndef RTPE_WARP_XPT
#define RTPE_WARP_XPT 1
#endif
template <int XPT>
__global__ void __launch_bounds__(256) warp_normalize_batch_kernel(const WarpBatchArgs a) {
  const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * XPT;
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.ow || y >= a.oh) return;
  const WarpJob& j = a.jobs[blockIdx.z];
  const unsigned char* src = reinterpret_cast<const unsigned char*>(j.src);
  float* dst = reinterpret_cast<float*>(j.dst);
  const int h = j.h, w = j.w, stride = j.stride;
  const float m[6] = {j.m[0], j.m[1], j.m[2], j.m[3], j.m[4], j.m[5]};
  float o[XPT][3];
#pragma unroll
  for (int i = 0; i < XPT; ++i)
    if (i == 0 || x + i < a.ow) warp_pixel(src, h, w, stride, m, a.mean, a.stdev, a.round_u8, x + i, y, o[i]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float* p = dst + ((size_t)c * a.oh + y) * a.ow + x;
    if constexpr (XPT == 4) {
      if (x + 3 < a.ow && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        *reinterpret_cast<float4*>(p) = make_float4(o[0][c], o[1][c], o[2][c], o[3][c]);
        continue;
      }
    }
#pragma unroll
    for (int i = 0; i < XPT; ++i)
      if (x + i < a.ow) p[i] = o[i][c];
  }
}

}  // namespace rtpe

extern "C" int rtpe_warp_normalize(const void* src_hwc_u8, int32_t h, int32_t w, int32_t stride_bytes,
                                   const float* m_dst_to_src, const float* mean, const float* stdev, void* dst_chw_f32,
                                   int32_t oh, int32_t ow, int32_t round_u8, void* stream) {
  using namespace rtpe;
  RTPE_REQUIRE(src_hwc_u8 && dst_chw_f32 && m_dst_to_src && mean && stdev, "warp_normalize: null argument");
  RTPE_REQUIRE(h > 0 && w > 0 && oh > 0 && ow > 0 && stride_bytes >= 3 * w, "warp_normalize: h=%d w=%d stride=%d oh=%d ow=%d",
               h, w, stride_bytes, oh, ow);
  WarpArgs a;
  a.src = reinterpret_cast<const unsigned char*>(src_hwc_u8);
  a.dst = reinterpret_cast<float*>(dst_chw_f32);
  a.h = h; a.w = w; a.stride = stride_bytes; a.oh = oh; a.ow = ow;
  a.round_u8 = round_u8 != 0;
  for (int i = 0; i < 6; ++i) a.m[i] = m_dst_to_src[i];
  for (int c = 0; c < 3; ++c) {
    RTPE_REQUIRE(stdev[c] > 0.f, "warp_normalize: std must be positive");
    a.mean[c] = mean[c];
    a.stdev[c] = stdev[c];
  }
  hipLaunchKernelGGL(warp_normalize_kernel, dim3((ow + 63) / 64, (oh + 3) / 4), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

// ---- the batched warp: job table (host) + one launch per scale ---------------------------------------------------------
extern "C" int rtpe_warp_batch_table_bytes(int32_t n_images, int32_t n_scales, size_t* bytes) {
  using namespace rtpe;
  RTPE_REQUIRE(bytes, "warp_batch_table_bytes: null argument");
  RTPE_REQUIRE(n_images > 0 && n_images <= 65535 && n_scales > 0 && n_scales <= 16,
               "warp_batch_table_bytes: n_images=%d (1..65535) n_scales=%d (1..16)", n_images, n_scales);
  *bytes = sizeof(WarpJob) * (size_t)n_images * (size_t)n_scales;
  return RTPE_OK;
}

extern "C" int rtpe_warp_batch_table_fill(const uint64_t* src_addr, const int32_t* src_hws, const float* matrices,
                                          const uint64_t* dst_base, const int32_t* sizes, int32_t n_images,
                                          int32_t n_scales, void* table, size_t table_bytes) {
  using namespace rtpe;
  RTPE_REQUIRE(src_addr && src_hws && matrices && dst_base && sizes && table, "warp_batch_table_fill: null argument");
  size_t need = 0;
  if (int rc = rtpe_warp_batch_table_bytes(n_images, n_scales, &need)) return rc;
  RTPE_REQUIRE(table_bytes >= need, "warp_batch_table_fill: table of %zu bytes, %zu needed", table_bytes, need);
  for (int n = 0; n < n_images; ++n) {
    const int32_t h = src_hws[3 * n], w = src_hws[3 * n + 1], stride = src_hws[3 * n + 2];
    RTPE_REQUIRE(src_addr[n] && h > 0 && w > 0 && w <= INT32_MAX / 3 && stride >= 3 * w,
                 "warp_batch_table_fill: image %d: address %#llx h=%d w=%d stride=%d", n, (unsigned long long)src_addr[n], h,
                 w, stride);
  }
  for (int s = 0; s < n_scales; ++s)
    RTPE_REQUIRE(dst_base[s] && dst_base[s] % sizeof(float) == 0 && sizes[2 * s] > 0 && sizes[2 * s + 1] > 0,
                 "warp_batch_table_fill: scale %d: address %#llx H=%d W=%d", s, (unsigned long long)dst_base[s],
                 sizes[2 * s], sizes[2 * s + 1]);
  unsigned char* jobs = reinterpret_cast<unsigned char*>(table);      // (the caller's buffer may be unaligned)
  for (int s = 0; s < n_scales; ++s) {
    const uint64_t image_bytes = 3ull * (uint64_t)sizes[2 * s] * (uint64_t)sizes[2 * s + 1] * sizeof(float);
    for (int n = 0; n < n_images; ++n) {
      WarpJob j;
      memset(&j, 0, sizeof(j));
      j.src = src_addr[n];
      j.h = src_hws[3 * n];
      j.w = src_hws[3 * n + 1];
      j.stride = src_hws[3 * n + 2];
      for (int i = 0; i < 6; ++i) j.m[i] = matrices[((size_t)s * n_images + n) * 6 + i];
      j.dst = dst_base[s] + (uint64_t)n * image_bytes;
      memcpy(jobs + ((size_t)s * n_images + n) * sizeof(j), &j, sizeof(j));
    }
  }
  return RTPE_OK;
}

extern "C" int rtpe_warp_normalize_batch(const void* table_dev, int32_t n_images, int32_t n_scales, const int32_t* sizes,
                                         const float* mean, const float* stdev, int32_t round_u8, void* stream) {
  using namespace rtpe;
  RTPE_REQUIRE(table_dev && sizes && mean && stdev, "warp_normalize_batch: null argument");
  RTPE_REQUIRE(reinterpret_cast<uintptr_t>(table_dev) % 8 == 0, "warp_normalize_batch: the table must be 8-byte aligned");
  size_t need = 0;
  if (int rc = rtpe_warp_batch_table_bytes(n_images, n_scales, &need)) return rc;
  WarpBatchArgs a;
  a.round_u8 = round_u8 != 0;
  for (int c = 0; c < 3; ++c) {
    RTPE_REQUIRE(stdev[c] > 0.f, "warp_normalize_batch: std must be positive");
    a.mean[c] = mean[c];
    a.stdev[c] = stdev[c];
  }
  for (int s = 0; s < n_scales; ++s)
    RTPE_REQUIRE(sizes[2 * s] > 0 && sizes[2 * s + 1] > 0 && (sizes[2 * s] + 3) / 4 <= 65535,
                 "warp_normalize_batch: scale %d: H=%d W=%d", s, sizes[2 * s], sizes[2 * s + 1]);
  constexpr int XPT = RTPE_WARP_XPT;
  for (int s = 0; s < n_scales; ++s) {
    a.jobs = reinterpret_cast<const WarpJob*>(table_dev) + (size_t)s * n_images;
    a.oh = sizes[2 * s];
    a.ow = sizes[2 * s + 1];
    hipLaunchKernelGGL(warp_normalize_batch_kernel<XPT>, dim3((a.ow + 64 * XPT - 1) / (64 * XPT), (a.oh + 3) / 4, n_images),
                       dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    RTPE_HIP_CHECK(hipGetLastError());
  }
  return RTPE_OK;
}
