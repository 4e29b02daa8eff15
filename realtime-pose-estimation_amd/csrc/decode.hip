// Heatmap -> keypoint decode on gfx950: bilinear upsample, 5x5 max-pool NMS,
// top-K per (image, joint), tag gather, quarter-pixel adjust, tag-penalised
// arg-max refine.  Replaces validate_hhrnet.py:94-98 and the device side of
// rtpe/third_party/group.py:125-287 of the reference.
//
// Everything here is HBM/latency-bound integer + fp32 compare work, so the
// design goal is to touch the low-resolution network outputs once and never
// materialise the upsampled (h, w) maps (fused path): a sampler evaluates
// PyTorch-CPU's exact bilinear formula on the fly.  Bit-exactness rules:
//   * compiled with -ffp-contract=off; the fused multiply-adds that PyTorch's
//     CPU kernel performs are written explicitly (T = fma(v0,l0,v1*l1)),
//   * ties in top-K and arg-max go to the lowest flat index (np.argmax /
//     first-occurrence semantics); keys are (order-preserving value bits << 32
//     | ~index) so one unsigned 64-bit max does both.
#include "rtpe_common.h"
#include "resize_nc.h"          // align_corners=False bilinear of the flip-test chain (aggregate.hip's arithmetic)
#include "tag_mean.h"           // launch_mean_plane (tag_mean.hip): the averaged-tag test's shared planes

namespace rtpe {

typedef unsigned long long u64;

// ---------------------------------------------------------------------------
// samplers
// ---------------------------------------------------------------------------
struct DirectMap {          // dense (planes, h, w)
  const float* p;
  int h, w;
  __device__ __forceinline__ float at(int plane, int y, int x) const {
    return p[((size_t)plane * h + y) * w + x];
  }
};

struct Axis {               // one axis of F.interpolate(bilinear, align_corners=True)
  float scale;              // float(in-1)/float(out-1)
  int n_in, same;
  __device__ __forceinline__ void at(int o, int* i0, int* i1, float* l0, float* l1) const {
    if (same) { *i0 = *i1 = o; *l0 = 1.f; *l1 = 0.f; return; }
    const float real = scale * (float)o;
    int a = (int)real;
    a = a < n_in - 1 ? a : n_in - 1;
    *i0 = a;
    *i1 = a + (a < n_in - 1 ? 1 : 0);
    float l = real - (float)a;
    l = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
    *l1 = l;
    *l0 = 1.f - l;
  }
};

// PyTorch's CPU op has a second kernel for small outputs: with out_h + out_w <= 128 (whatever the input size)
// upsample_bilinear2d resizes through its channels-last kernel (aten/src/ATen/native/cpu/UpSampleKernel.cpp,
// _use_vectorized_kernel_cond_2d), which takes the same taps and axis weights but multiplies the weights first,
// w_ab = ly_a * lx_b, and sums four products - the channels in vectors of 16 as
//     fma(w00, v00, fma(w01, v01, fma(w11, v11, w10 * v10)))
// and the channels left over (C % 16: of the 17 heat or tag maps of one F.interpolate call, the last) as
//     fma(w11, v11, fma(w10, v10, fma(w00, v00, w01 * v01)))
// (the contractions of an AVX-512 build, pinned on PyTorch itself by tests/test_sizes_decode_gpu.py through the oracle).
constexpr int kSmallOutput = 128;
__device__ __forceinline__ float bilinear_small(float v00, float v01, float v10, float v11, float ly0, float ly1,
                                                float lx0, float lx1, bool tail) {
  const float w00 = ly0 * lx0, w01 = ly0 * lx1, w10 = ly1 * lx0, w11 = ly1 * lx1;
  if (tail) return __builtin_fmaf(w11, v11, __builtin_fmaf(w10, v10, __builtin_fmaf(w00, v00, w01 * v01)));
  return __builtin_fmaf(w00, v00, __builtin_fmaf(w01, v01, __builtin_fmaf(w11, v11, w10 * v10)));
}

struct BilinearMap {        // low-res planes sampled at (oh, ow) resolution
  const float* p;
  int sh, sw, J;
  int small;                // oh + ow <= kSmallOutput: the sample arithmetic of PyTorch's small-output kernel
  long long img_stride;     // elements between images; plane j of image n at n*img_stride + j*sh*sw
  Axis ay, ax;
  // plane j of an image is channel j of the J that one F.interpolate call resizes: beyond the last full vector of 16?
  __device__ __forceinline__ bool tail(int plane) const { return plane % J >= J - (J & 15); }
  __device__ __forceinline__ float at(int plane, int y, int x) const {
    const int n = plane / J, j = plane - n * J;
    return sample(p + (size_t)n * img_stride + (size_t)j * sh * sw, y, x, j >= J - (J & 15));
  }
  // the sample of the source plane at b; in_tail: the plane's channel lies in the tail of the 16-wide vector
  __device__ __forceinline__ float sample(const float* b, int y, int x, bool in_tail) const {
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    ay.at(y, &y0, &y1, &ly0, &ly1);
    ax.at(x, &x0, &x1, &lx0, &lx1);
    const float v00 = b[y0 * sw + x0], v01 = b[y0 * sw + x1];
    const float v10 = b[y1 * sw + x0], v11 = b[y1 * sw + x1];
    if (small) return bilinear_small(v00, v01, v10, v11, ly0, ly1, lx0, lx1, in_tail);
    const float t0 = __builtin_fmaf(v00, lx0, v01 * lx1);
    const float t1 = __builtin_fmaf(v10, lx0, v11 * lx1);
    return __builtin_fmaf(t0, ly0, t1 * ly1);
  }
};

static int small_output(int oh, int ow) { return oh + ow <= kSmallOutput; }

static Axis make_axis(int n_in, int n_out) {
  Axis a;
  a.n_in = n_in;
  a.same = n_in == n_out;
  a.scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
  return a;
}

struct BilinearTag {        // D == 1
  BilinearMap m;
  __device__ __forceinline__ float at(int plane, int y, int x, int) const { return m.at(plane, y, x); }
};

// One tag plane per image, shared by all its joints (the dual-head students' det[:, J:J+1]): D == 1, (N, 1, th, tw) at
// an image stride.  The (image * J + joint) plane index that the top-k merge (tag_shared_joints = 0) and the adjust /
// refine kernels pass selects the image's plane here, and only here.  The sample is BilinearMap::at's on channel
// `joint` of the plane expanded to (N, J, th, tw): the same taps and weights, and for a small output the tap order of
// that channel (the tail of the 16-wide vector or not) - the joint decides no address, only that order.
struct SharedBilinearTag {
  BilinearMap m;            // p, img_stride: the shared planes; J: the joints that share one
  __device__ __forceinline__ float at(int plane, int y, int x, int) const {
    const int n = plane / m.J, j = plane - n * m.J;
    return m.sample(m.p + (size_t)n * m.img_stride, y, x, j >= m.J - (m.J & 15));
  }
};

// ---------------------------------------------------------------------------
// per-image decode sizes: every image n of a batch is sampled at its own (oh_n, ow_n).  The sizes and the four
// axes that go with them come from a device-visible table of one SizeEntry per image, written on the host by
// rtpe_decode_sizes_fill with make_axis (layout: include/rtpe_hip.h).  A kernel resolves its plane's entry once, at its
// start (plane_view / plane_tag: the index plane / J is uniform wherever the plane comes from the grid), and runs
// the bodies of the one-size decode on the BilinearMap it gets: per sample the arithmetic is BilinearMap::at's.
// Flat pixel indices (the top-k table's `ind`, the arg-max keys) are y * w_enc + x with ONE width w_enc >= every
// ow_n for the whole batch: for x < ow_n the order of the indices of an image is that of its own row-major order.
// For every other map the three helpers are the identity: (h, w) stay the launch-wide scalars and w_enc == w.
// ---------------------------------------------------------------------------
struct SizeEntry {
  int32_t oh, ow;
  Axis hy, hx, ty, tx;      // heat map rows / columns, tag map rows / columns
  int32_t small;            // oh + ow <= kSmallOutput (BilinearMap::small)
  int32_t reserved;
};
static_assert(sizeof(SizeEntry) == 64, "SizeEntry is 64 bytes in the ABI");

struct NetSizesMap {        // the refined heat maps, image n at tab[n]'s size
  BilinearMap m;            // source planes; its two axes are not read
  const SizeEntry* tab;
  int w_enc;
};

struct NetSizesTag {        // the per-joint tag maps of the same images, D == 1
  BilinearMap m;
  const SizeEntry* tab;
};

// NetSizesTag with ONE tag plane per image, shared by its J joints (a mixed-size batch of the dual-head students decoded
// from its canvas, include/rtpe_hip_mixdec.h): plane_tag gives a SharedBilinearTag with the axes of the image's entry,
// so the (image * J + joint) plane index selects the image's plane and the joint's tap order there, and only there.
// m.sh / m.sw are the canvas extents (the pitch); the image's own extents are the n_in of its entry's axes.
struct NetMixedTag {
  BilinearMap m;            // p, img_stride: the shared planes; J: the joints that share one
  const SizeEntry* tab;
};

template <class Map> struct PerImageSize { static constexpr bool value = false; };
template <> struct PerImageSize<NetSizesMap> { static constexpr bool value = true; };

// the map of `plane`'s image and, for per-image sizes, that image's (h, w)
template <class Map>
__device__ __forceinline__ const Map& plane_view(const Map& m, int, int*, int*) { return m; }
__device__ __forceinline__ BilinearMap plane_view(const NetSizesMap& s, int plane, int* h, int* w) {
  const SizeEntry* e = s.tab + plane / s.m.J;
  BilinearMap v = s.m;
  v.ay = e->hy;
  v.ax = e->hx;
  v.small = e->small;
  *h = e->oh;
  *w = e->ow;
  return v;
}
template <class TagMap>
__device__ __forceinline__ const TagMap& plane_tag(const TagMap& t, int) { return t; }
__device__ __forceinline__ BilinearTag plane_tag(const NetSizesTag& s, int plane) {
  const SizeEntry* e = s.tab + plane / s.m.J;
  BilinearTag v{s.m};
  v.m.ay = e->ty;
  v.m.ax = e->tx;
  v.m.small = e->small;
  return v;
}
__device__ __forceinline__ SharedBilinearTag plane_tag(const NetMixedTag& s, int plane) {
  const SizeEntry* e = s.tab + plane / s.m.J;
  SharedBilinearTag v{s.m};
  v.m.ay = e->ty;
  v.m.ax = e->tx;
  v.m.small = e->small;
  return v;
}
// the width that flat indices are formed and split with
template <class Map>
__host__ __device__ __forceinline__ int enc_width(const Map&, int w) { return w; }
__host__ __device__ __forceinline__ int enc_width(const NetSizesMap& s, int) { return s.w_enc; }
// idx = y * w + x of the image's own width -> the batch's encoding
template <class Map>
__device__ __forceinline__ unsigned enc_index(const Map&, unsigned idx, int) { return idx; }
__device__ __forceinline__ unsigned enc_index(const NetSizesMap& s, unsigned idx, int w) {
  const unsigned y = idx / (unsigned)w;
  return y * (unsigned)s.w_enc + (idx - y * (unsigned)w);
}

__device__ __forceinline__ unsigned order_bits(float v) {   // monotone float -> uint
  if (v == 0.f) v = 0.f;                                     // -0 == +0
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unorder_bits(unsigned k) {
  const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(u);
}
__device__ __forceinline__ u64 make_key(float v, unsigned idx) {
  return ((u64)order_bits(v) << 32) | (u64)(0xffffffffu - idx);
}

__device__ __forceinline__ u64 wave_max(u64 k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)k, o), hi = __shfl_xor((unsigned)(k >> 32), o);
    const u64 other = ((u64)hi << 32) | lo;
    k = other > k ? other : k;
  }
  return k;
}

// block-wide max of a key; red must hold blockDim/64 entries; all threads get the result
__device__ __forceinline__ u64 block_max(u64 k, u64* red) {
  k = wave_max(k);
  const int wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wv] = k;
  __syncthreads();
  u64 r = red[0];
  for (int i = 1; i < nw; ++i) r = red[i] > r ? red[i] : r;
  return r;
}

// ---------------------------------------------------------------------------
// plain bilinear upsample and NMS (API parity with F.interpolate / parser.nms)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bilinear_kernel(BilinearMap m, int planes, int oh, int ow, float* dst) {
  const size_t total = (size_t)planes * oh * ow;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int x = (int)(i % ow);
    const size_t r = i / ow;
    const int y = (int)(r % oh), pl = (int)(r / oh);
    dst[i] = m.at(pl, y, x);
  }
}

constexpr int kTH = 32, kTW = 64;   // NMS / top-k tile (2048 px, 8 per thread)
constexpr int kMaxPad = 4;          // supports nms kernels up to 9x9
constexpr int kMaxCand = 512;       // local maxima of a tile handled by the one-pass rank sort

// per-tile samples of the (virtual) full-resolution map.  For the bilinear sampler the two
// axis computations are done once per tile row / column (tables in LDS) instead of once per
// sample; the per-sample arithmetic is exactly BilinearMap::at's.
struct AxisTab {
  int i0[kTW + 2 * kMaxPad], i1[kTW + 2 * kMaxPad];
  float l0[kTW + 2 * kMaxPad], l1[kTW + 2 * kMaxPad];
};

// returns false (and leaves `raw` unfilled) only when the caller passed `pos_flag` and no source value under
// the tile is positive
constexpr int kTRows = 24;          // source rows of a tile kept as horizontally interpolated rows (separable sampling)

template <class Map>
__device__ __forceinline__ bool fill_raw(const Map& m, int plane, int h, int w, int y0, int x0, int pad, float* raw,
                                         AxisTab*, AxisTab*, float*, int, int* = nullptr, float* = nullptr) {
  const int PW = kTW + 2 * pad, PH = kTH + 2 * pad;
  for (int i = threadIdx.x; i < PH * PW; i += 256) {
    const int py = i / PW, px = i - py * PW;
    const int y = y0 - pad + py, x = x0 - pad + px;
    raw[i] = ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w) ? m.at(plane, y, x) : -INFINITY;
  }
  return true;
}

template <>
__device__ __forceinline__ bool fill_raw<BilinearMap>(const BilinearMap& m, int plane, int h, int w, int y0, int x0,
                                                      int pad, float* raw, AxisTab* ty, AxisTab* tx, float* stage,
                                                      int stage_floats, int* pos_flag, float* tbuf) {
  const int PW = kTW + 2 * pad, PH = kTH + 2 * pad;
  for (int i = threadIdx.x; i < PH + PW; i += 256) {
    const bool isy = i < PH;
    const int k = isy ? i : i - PH;
    const int o = (isy ? y0 : x0) - pad + k;
    AxisTab* t = isy ? ty : tx;
    const int lim = isy ? h : w;
    int a0 = -1, a1 = -1;
    float f0 = 0.f, f1 = 0.f;
    if ((unsigned)o < (unsigned)lim) (isy ? m.ay : m.ax).at(o, &a0, &a1, &f0, &f1);
    t->i0[k] = a0; t->i1[k] = a1; t->l0[k] = f0; t->l1[k] = f1;
  }
  __syncthreads();
  const int n = plane / m.J, j = plane - n * m.J;
  const float* b = m.p + (size_t)n * m.img_stride + (size_t)j * m.sh * m.sw;
  // The source pixels a tile needs form a small rectangle (about half the tile per axis when the map
  // is upsampled 2x): stage it in LDS once (in `stage`, the row-max buffer, free at this point) and take
  // the four taps of every sample from there instead of from L1; same arithmetic, same result.
  const int ky0 = max(0, pad - y0), ky1 = min(PH - 1, h - 1 - (y0 - pad));
  const int kx0 = max(0, pad - x0), kx1 = min(PW - 1, w - 1 - (x0 - pad));
  const int sr0 = ty->i0[ky0], sr1 = ty->i1[ky1], sc0 = tx->i0[kx0], sc1 = tx->i1[kx1];
  const int er = sr1 - sr0 + 1, ec = sc1 - sc0 + 1;
  const bool staged = stage != nullptr && ky0 <= ky1 && kx0 <= kx1 && er > 0 && ec > 0 && er * ec <= stage_floats;
  if (staged) {
    bool pos = false;
    // four loads in flight per thread before the first LDS write (the plain loop compiled to one load + vmcnt(0) per
    // element: one memory round trip per 256 source values; a tile has ~700)
    for (int i0 = threadIdx.x; i0 < er * ec; i0 += 4 * 256) {
      float v4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + k * 256;
        const int ii = i < er * ec ? i : 0;               // (no branch around the load)
        const int r = ii / ec, c = ii - r * ec;
        v4[k] = b[(sr0 + r) * m.sw + sc0 + c];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + k * 256;
        if (i < er * ec) {
          stage[i] = v4[k];
          pos |= v4[k] > 0.f;
        }
      }
    }
    if (pos_flag != nullptr && pos) *pos_flag = 1;         // (the caller zeroed it before the axis-table barrier)
    __syncthreads();
    // every sample is a combination of these values with weights >= 0: none positive here means no positive
    // sample, i.e. no candidate in the tile (the top-k only takes positive local maxima)
    if (pos_flag != nullptr && *pos_flag == 0) return false;
  }
  // sample (py, px): the four taps and three multiply-adds of F.interpolate(align_corners=True), in its order
  const bool small_tail = m.tail(plane);
  auto sample = [&](int r0, int r1, float ly0, float ly1, int c0, int c1, float lx0, float lx1) -> float {
    if (r0 < 0 || c0 < 0) return -INFINITY;               // outside the image
    float v00, v01, v10, v11;
    if (staged) {
      const float* s0 = stage + (r0 - sr0) * ec - sc0;
      const float* s1 = stage + (r1 - sr0) * ec - sc0;
      v00 = s0[c0]; v01 = s0[c1]; v10 = s1[c0]; v11 = s1[c1];
    } else {
      v00 = b[r0 * m.sw + c0]; v01 = b[r0 * m.sw + c1];
      v10 = b[r1 * m.sw + c0]; v11 = b[r1 * m.sw + c1];
    }
    if (m.small) return bilinear_small(v00, v01, v10, v11, ly0, ly1, lx0, lx1, small_tail);
    const float t0 = __builtin_fmaf(v00, lx0, v01 * lx1);
    const float t1 = __builtin_fmaf(v10, lx0, v11 * lx1);
    return __builtin_fmaf(t0, ly0, t1 * ly1);
  };
  if (tbuf != nullptr && staged && er <= kTRows && (PW & 3) == 0 && !m.small) {   // (small outputs are not separable)
    // Separable form (5x5 window path): T(r, px) = fma(v(r, c0), lx0, v(r, c1) * lx1) depends on the SOURCE row r and
    // the output column only, and every source row serves ~4 output rows (as their upper or lower row): the
    // horizontal step is done once per (source row, column), the vertical step fma(T(r0), ly0, T(r1) * ly1) takes
    // 4 columns per thread with 16-byte LDS accesses.  The same operations on the same operands as
    // BilinearMap::at: bit-equal.
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    {
      const int c0 = tx->i0[lane], c1 = tx->i1[lane];
      const float lx0 = tx->l0[lane], lx1 = tx->l1[lane];
      for (int r = wv; r < er; r += 4) {
        const float* srow = stage + r * ec - sc0;
        tbuf[r * PW + lane] = c0 < 0 ? 0.f : __builtin_fmaf(srow[c0], lx0, srow[c1] * lx1);
      }
      const int extra = PW - 64;                           // 2 * pad columns
      for (int i = threadIdx.x; i < er * extra; i += 256) {
        const int r = i / extra, px = 64 + i - r * extra;
        const int e0 = tx->i0[px], e1 = tx->i1[px];
        const float* srow = stage + r * ec - sc0;
        tbuf[r * PW + px] = e0 < 0 ? 0.f : __builtin_fmaf(srow[e0], tx->l0[px], srow[e1] * tx->l1[px]);
      }
    }
    __syncthreads();
    const int groups = PW >> 2;                            // 4 columns per thread and row
    for (int i = threadIdx.x; i < PH * groups; i += 256) {
      const int py = i / groups, cg = i - py * groups;
      const int r0 = ty->i0[py];
      float4 o = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      if (r0 >= 0) {
        const int r1 = ty->i1[py];
        const float ly0 = ty->l0[py], ly1 = ty->l1[py];
        const float4 a = *reinterpret_cast<const float4*>(tbuf + (r0 - sr0) * PW + 4 * cg);
        const float4 bq = *reinterpret_cast<const float4*>(tbuf + (r1 - sr0) * PW + 4 * cg);
        const int x = x0 - pad + 4 * cg;                   // columns outside the image stay -inf
        if ((unsigned)(x + 0) < (unsigned)w) o.x = __builtin_fmaf(a.x, ly0, bq.x * ly1);
        if ((unsigned)(x + 1) < (unsigned)w) o.y = __builtin_fmaf(a.y, ly0, bq.y * ly1);
        if ((unsigned)(x + 2) < (unsigned)w) o.z = __builtin_fmaf(a.z, ly0, bq.z * ly1);
        if ((unsigned)(x + 3) < (unsigned)w) o.w = __builtin_fmaf(a.w, ly0, bq.w * ly1);
      }
      *reinterpret_cast<float4*>(raw + py * PW + 4 * cg) = o;
    }
    __syncthreads();                                       // `stage` becomes the row-max buffer again
    return true;
  }
  // lane = column (its axis entry stays in registers), wave = every 4th row (its axis entry is wave-uniform):
  // per sample only the four taps and the result touch LDS - with one table look-up per sample and axis the
  // kernel was bound by the LDS instruction rate.  Columns 64.. of the padded tile go in one extra pass.
  {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c0 = tx->i0[lane], c1 = tx->i1[lane];
    const float lx0 = tx->l0[lane], lx1 = tx->l1[lane];
    for (int py = wv; py < PH; py += 4) {
      const int r0 = __builtin_amdgcn_readfirstlane(ty->i0[py]), r1 = __builtin_amdgcn_readfirstlane(ty->i1[py]);
      const float ly0 = ty->l0[py], ly1 = ty->l1[py];
      raw[py * PW + lane] = sample(r0, r1, ly0, ly1, c0, c1, lx0, lx1);
    }
    const int extra = PW - 64;                             // 2 * pad columns
    for (int i = threadIdx.x; i < PH * extra; i += 256) {
      const int py = i / extra, px = 64 + i - py * extra;
      raw[py * PW + px] = sample(ty->i0[py], ty->i1[py], ty->l0[py], ty->l1[py], tx->i0[px], tx->i1[px], tx->l0[px],
                                 tx->l1[px]);
    }
  }
  if (staged) __syncthreads();                          // `stage` becomes the row-max buffer again
  return true;
}

// ---------------------------------------------------------------------------
// flip test (upstream single-scale + flip protocol, rtpe/inference.py): the heat map at the projection size (oh, ow)
//     heat(y, x) = (rs(A_o)(y, x) + rs(A_f)(y, x)) / 2
// with rs = F.interpolate(bilinear, align_corners=False) from the refined resolution (sh, sw), evaluated with
// aggregate.hip's arithmetic (resize_nc.h): the two rs values are exactly what aggregate_results' copy and its
// accumulate-and-divide call read, and (a + b) / 2 is the kernel's dst + v, then / div.  A_o / A_f are the
// stage-averaged maps of the image and of its mirror image (flip_prep_kernel below) as dense (planes, sh, sw).
// ---------------------------------------------------------------------------
struct NcAxes {             // (sh, sw) -> (oh, ow) planes, align_corners=False
  int sh, sw, oh, ow;
  float sy, sx;             // float(in) / float(out)
  bool ident;               // both sizes agree: the kernel copies
  __device__ __forceinline__ float at(const float* plane, int y, int x) const {
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    axis_nc(sy, sh, oh, y, &y0, &y1, &ly0, &ly1);
    axis_nc(sx, sw, ow, x, &x0, &x1, &lx0, &lx1);
    return taps_nc(plane, sw, ident, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
  }
};

struct FlipHeatMap {
  const float* ao;          // (planes, sh, sw) stage average of the image
  const float* af;          // (planes, sh, sw) the same of the mirror image, mirrored back, joints swapped
  NcAxes a;
  __device__ __forceinline__ float at(int plane, int y, int x) const {
    const size_t off = (size_t)plane * a.sh * a.sw;
    const float o = a.at(ao + off, y, x), f = a.at(af + off, y, x);
    return (o + f) / 2.f;
  }
};

struct FlipTag {            // D == 2: [rs(T_o), rs(T_f)], the image's tag first (torch.cat order of aggregate_results)
  const float* to;
  const float* tf;
  NcAxes a;
  __device__ __forceinline__ float at(int plane, int y, int x, int d) const {
    return a.at((d == 0 ? to : tf) + (size_t)plane * a.sh * a.sw, y, x);
  }
};

// AGS (one tag map shared by all joints of an image, valid_ae1dim.py's AGS branch): D == 1, ONE plane per image,
// (N, sh, sw).  The (image * J + joint) plane index that the top-k merge (tag_shared_joints = 0) and the adjust /
// refine kernels pass is mapped to the image here, and only here.
struct AgsTag {
  const float* p;
  int J;
  NcAxes a;
  __device__ __forceinline__ float at(int plane, int y, int x, int) const {
    return a.at(p + (size_t)(plane / J) * a.sh * a.sw, y, x);
  }
};

// The tile of the flip heat map: axis tables once per tile row / column, the source rectangles of BOTH planes staged
// in LDS (in `stage`, the row-max buffer, free at this point), then per sample the eight taps from there and the
// arithmetic of FlipHeatMap::at (same operations, same operands: bit-equal).  The separable form of the
// align_corners=True sampler does not apply: the identity branch and the two planes per sample would need two
// row buffers; the register-blocked max passes of the 5x5 path (nms_tile / topk_tile_kernel) run on its output.
template <>
__device__ __forceinline__ bool fill_raw<FlipHeatMap>(const FlipHeatMap& m, int plane, int h, int w, int y0, int x0,
                                                      int pad, float* raw, AxisTab* ty, AxisTab* tx, float* stage,
                                                      int stage_floats, int* pos_flag, float*) {
  const int PW = kTW + 2 * pad, PH = kTH + 2 * pad;
  const NcAxes& A = m.a;
  for (int i = threadIdx.x; i < PH + PW; i += 256) {
    const bool isy = i < PH;
    const int k = isy ? i : i - PH;
    const int o = (isy ? y0 : x0) - pad + k;
    AxisTab* t = isy ? ty : tx;
    int a0 = -1, a1 = -1;
    float f0 = 0.f, f1 = 0.f;
    if ((unsigned)o < (unsigned)(isy ? h : w)) {
      if (isy) axis_nc(A.sy, A.sh, A.oh, o, &a0, &a1, &f0, &f1);
      else axis_nc(A.sx, A.sw, A.ow, o, &a0, &a1, &f0, &f1);
    }
    t->i0[k] = a0; t->i1[k] = a1; t->l0[k] = f0; t->l1[k] = f1;
  }
  __syncthreads();
  const size_t off = (size_t)plane * A.sh * A.sw;
  const float* bo = m.ao + off;
  const float* bf = m.af + off;
  const int ky0 = max(0, pad - y0), ky1 = min(PH - 1, h - 1 - (y0 - pad));
  const int kx0 = max(0, pad - x0), kx1 = min(PW - 1, w - 1 - (x0 - pad));
  const int sr0 = ty->i0[ky0], sr1 = ty->i1[ky1], sc0 = tx->i0[kx0], sc1 = tx->i1[kx1];   // i0, i1 grow with o
  const int er = sr1 - sr0 + 1, ec = sc1 - sc0 + 1;
  const bool staged = stage != nullptr && ky0 <= ky1 && kx0 <= kx1 && er > 0 && ec > 0 && 2 * er * ec <= stage_floats;
  const int ne = er * ec;
  if (staged) {
    bool pos = false;
    for (int i0 = threadIdx.x; i0 < 2 * ne; i0 += 4 * 256) {
      float v4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + k * 256;
        const int ii = i < 2 * ne ? i : 0;                // (no branch around the load)
        const int q = ii < ne ? ii : ii - ne;
        const int r = q / ec, c = q - r * ec;
        v4[k] = (ii < ne ? bo : bf)[(size_t)(sr0 + r) * A.sw + sc0 + c];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + k * 256;
        if (i < 2 * ne) {
          stage[i] = v4[k];
          pos |= v4[k] > 0.f;
        }
      }
    }
    if (pos_flag != nullptr && pos) *pos_flag = 1;         // (the caller zeroed it before the axis-table barrier)
    __syncthreads();
    // every sample is (a + b) / 2 of combinations of these values with weights >= 0: none positive, no candidate
    if (pos_flag != nullptr && *pos_flag == 0) return false;
  }
  auto sample = [&](int r0, int r1, float ly0, float ly1, int c0, int c1, float lx0, float lx1) -> float {
    if (r0 < 0 || c0 < 0) return -INFINITY;               // outside the image
    float o, f;
    if (staged) {
      const float* so = stage - sc0;
      const float* sf = stage + ne - sc0;
      o = taps_nc(so + (r0 - sr0) * ec, ec, A.ident, 0, r1 - r0, c0, c1, ly0, ly1, lx0, lx1);
      f = taps_nc(sf + (r0 - sr0) * ec, ec, A.ident, 0, r1 - r0, c0, c1, ly0, ly1, lx0, lx1);
    } else {
      o = taps_nc(bo, A.sw, A.ident, r0, r1, c0, c1, ly0, ly1, lx0, lx1);
      f = taps_nc(bf, A.sw, A.ident, r0, r1, c0, c1, ly0, ly1, lx0, lx1);
    }
    return (o + f) / 2.f;
  };
  {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c0 = tx->i0[lane], c1 = tx->i1[lane];
    const float lx0 = tx->l0[lane], lx1 = tx->l1[lane];
    for (int py = wv; py < PH; py += 4) {
      const int r0 = __builtin_amdgcn_readfirstlane(ty->i0[py]), r1 = __builtin_amdgcn_readfirstlane(ty->i1[py]);
      const float ly0 = ty->l0[py], ly1 = ty->l1[py];
      raw[py * PW + lane] = sample(r0, r1, ly0, ly1, c0, c1, lx0, lx1);
    }
    const int extra = PW - 64;                             // 2 * pad columns
    for (int i = threadIdx.x; i < PH * extra; i += 256) {
      const int py = i / extra, px = 64 + i - py * extra;
      raw[py * PW + px] = sample(ty->i0[py], ty->i1[py], ty->l0[py], ty->l1[py], tx->i0[px], tx->i1[px], tx->l0[px],
                                 tx->l1[px]);
    }
  }
  if (staged) __syncthreads();                          // `stage` becomes the row-max buffer again
  return true;
}


// ---------------------------------------------------------------------------
// multi-scale test (upstream protocol with scale_factors s_0 > s_1 > ..., rtpe/inference.py multi_scale_inference
// with project2image=True): the heat map at the projection size (oh, ow) of the scale-1 input
//     H_i = flip ? (rs_i(A_o^i) + rs_i(A_f^i)) / 2 : rs_i(A_o^i)
//     F = H_0, then F = F + H_i for i = 1, 2, ... in this order, then F = F / S (a true division) when S > 1
// rs_i = align_corners=False from the refined resolution of scale i (a copy when the sizes agree, as for s = 2).
// These are the values of aggregate_results' copy / accumulate calls and of the final resize_combine(div=S): the
// sum order is part of the result.  A_o^i / A_f^i as written by ms_prep_kernel (below), dense (planes, sh_i, sw_i).
// ---------------------------------------------------------------------------
constexpr int kMaxScales = 4;

struct MultiScaleHeatMap {
  const float* ao[kMaxScales];
  const float* af[kMaxScales];  // flip only
  NcAxes a[kMaxScales];
  int S;
  bool flip;
  __device__ __forceinline__ float entry(int i, int plane, int y, int x) const {
    const size_t off = (size_t)plane * a[i].sh * a[i].sw;
    const float o = a[i].at(ao[i] + off, y, x);
    if (!flip) return o;
    const float f = a[i].at(af[i] + off, y, x);
    return (o + f) / 2.f;
  }
  __device__ __forceinline__ float at(int plane, int y, int x) const {
    float F = entry(0, plane, y, x);
#pragma unroll
    for (int i = 1; i < kMaxScales; ++i)
      if (i < S) F = F + entry(i, plane, y, x);
    return S > 1 ? F / (float)S : F;
  }
};

// The tile of the multi-scale heat map.  Per scale, the source rectangle of its plane(s) is staged in LDS (`stage`,
// the row-max buffer, free at this point) while it fits, in scale order; an identity entry (a copy: every source value
// read once per tile) and an entry that no longer fits are read from global memory.  The axes are evaluated in
// registers (lane = column, row axes per wave-uniform row) - S AxisTab pairs would not fit beside the tile.  Per sample
// the operations of MultiScaleHeatMap::at on the same operands: bit-equal.  The early-out (no positive source value:
// no candidate) needs every entry staged.
template <>
__device__ __forceinline__ bool fill_raw<MultiScaleHeatMap>(const MultiScaleHeatMap& m, int plane, int h, int w, int y0,
                                                            int x0, int pad, float* raw, AxisTab*, AxisTab*, float* stage,
                                                            int stage_floats, int* pos_flag, float*) {
  const int PW = kTW + 2 * pad, PH = kTH + 2 * pad;
  const int np = m.flip ? 2 : 1;
  const int ky0 = max(0, pad - y0), ky1 = min(PH - 1, h - 1 - (y0 - pad));
  const int kx0 = max(0, pad - x0), kx1 = min(PW - 1, w - 1 - (x0 - pad));
  const bool can = stage != nullptr && ky0 <= ky1 && kx0 <= kx1;
  int sr0[kMaxScales], sc0[kMaxScales], ec[kMaxScales], ne[kMaxScales], at0[kMaxScales];   // at0 < 0: not staged
  int used = 0;
  bool all = can;
#pragma unroll
  for (int i = 0; i < kMaxScales; ++i) {
    sr0[i] = sc0[i] = 0;
    ec[i] = ne[i] = 0;
    at0[i] = -1;
    if (i >= m.S || !can) continue;
    const NcAxes& A = m.a[i];
    int r0, r1, c0, c1, d;
    float f0, f1;
    axis_nc(A.sy, A.sh, A.oh, y0 - pad + ky0, &r0, &d, &f0, &f1);    // i0, i1 grow with o
    axis_nc(A.sy, A.sh, A.oh, y0 - pad + ky1, &d, &r1, &f0, &f1);
    axis_nc(A.sx, A.sw, A.ow, x0 - pad + kx0, &c0, &d, &f0, &f1);
    axis_nc(A.sx, A.sw, A.ow, x0 - pad + kx1, &d, &c1, &f0, &f1);
    sr0[i] = r0;
    sc0[i] = c0;
    ec[i] = c1 - c0 + 1;
    ne[i] = (r1 - r0 + 1) * ec[i];
    if (!A.ident && used + np * ne[i] <= stage_floats) {
      at0[i] = used;
      used += np * ne[i];
    } else {
      all = false;
    }
  }
  __syncthreads();                                         // the caller zeroed pos_flag
  if (used > 0) {
    bool pos = false;
    for (int i0 = threadIdx.x; i0 < used; i0 += 4 * 256) {
      float v4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int ii = i0 + k * 256 < used ? i0 + k * 256 : 0;    // (no branch around the load)
        const float* src = m.ao[0];
        int q = 0, e = 1, sw = 0;
#pragma unroll
        for (int s = 0; s < kMaxScales; ++s) {             // the staged entry ii falls in (offsets grow with s)
          if (at0[s] >= 0 && ii >= at0[s]) {
            const bool second = ii >= at0[s] + ne[s];
            q = ii - at0[s] - (second ? ne[s] : 0);
            src = (second ? m.af[s] : m.ao[s]) + (size_t)plane * m.a[s].sh * m.a[s].sw +
                  (size_t)sr0[s] * m.a[s].sw + sc0[s];
            e = ec[s];
            sw = m.a[s].sw;
          }
        }
        const int r = q / e, c = q - r * e;
        v4[k] = src[(size_t)r * sw + c];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + k * 256;
        if (i < used) {
          stage[i] = v4[k];
          pos |= v4[k] > 0.f;
        }
      }
    }
    if (pos_flag != nullptr && pos) *pos_flag = 1;
    __syncthreads();
    // every sample combines these values with weights >= 0 (and divides by S > 0): none positive, no candidate
    if (all && pos_flag != nullptr && *pos_flag == 0) return false;
  }
  auto value = [&](int s, int r0, int r1, float ly0, float ly1, int c0, int c1, float lx0, float lx1) -> float {
    const NcAxes& A = m.a[s];
    float o, f = 0.f;
    if (at0[s] >= 0) {
      const float* so = stage + at0[s] + (r0 - sr0[s]) * ec[s] - sc0[s];
      o = taps_nc(so, ec[s], A.ident, 0, r1 - r0, c0, c1, ly0, ly1, lx0, lx1);
      if (m.flip) f = taps_nc(so + ne[s], ec[s], A.ident, 0, r1 - r0, c0, c1, ly0, ly1, lx0, lx1);
    } else {
      const size_t off = (size_t)plane * A.sh * A.sw;
      o = taps_nc(m.ao[s] + off, A.sw, A.ident, r0, r1, c0, c1, ly0, ly1, lx0, lx1);
      if (m.flip) f = taps_nc(m.af[s] + off, A.sw, A.ident, r0, r1, c0, c1, ly0, ly1, lx0, lx1);
    }
    return m.flip ? (o + f) / 2.f : o;
  };
  auto combine = [&](int y, const int (&c0)[kMaxScales], const int (&c1)[kMaxScales], const float (&l0)[kMaxScales],
                     const float (&l1)[kMaxScales]) -> float {
    float F = 0.f;
#pragma unroll
    for (int s = 0; s < kMaxScales; ++s) {
      if (s >= m.S) continue;
      int r0, r1;
      float ly0, ly1;
      axis_nc(m.a[s].sy, m.a[s].sh, m.a[s].oh, y, &r0, &r1, &ly0, &ly1);
      const float hv = value(s, r0, r1, ly0, ly1, c0[s], c1[s], l0[s], l1[s]);
      F = s == 0 ? hv : F + hv;
    }
    return m.S > 1 ? F / (float)m.S : F;
  };
  auto x_axes = [&](int x, int (&c0)[kMaxScales], int (&c1)[kMaxScales], float (&l0)[kMaxScales],
                    float (&l1)[kMaxScales]) {
#pragma unroll
    for (int s = 0; s < kMaxScales; ++s) {
      c0[s] = c1[s] = 0;
      l0[s] = 1.f;
      l1[s] = 0.f;
      if (s < m.S) axis_nc(m.a[s].sx, m.a[s].sw, m.a[s].ow, x, &c0[s], &c1[s], &l0[s], &l1[s]);
    }
  };
  {
    // lane = column (its x axes stay in registers), wave = every 4th row; columns 64.. in one extra pass
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = x0 - pad + lane;
    const bool xin = (unsigned)x < (unsigned)w;
    int c0[kMaxScales], c1[kMaxScales];
    float l0[kMaxScales], l1[kMaxScales];
    x_axes(xin ? x : 0, c0, c1, l0, l1);
    for (int py = wv; py < PH; py += 4) {
      const int y = y0 - pad + py;
      raw[py * PW + lane] = xin && (unsigned)y < (unsigned)h ? combine(y, c0, c1, l0, l1) : -INFINITY;
    }
    const int extra = PW - 64;                             // 2 * pad columns
    for (int i = threadIdx.x; i < PH * extra; i += 256) {
      const int py = i / extra, px = 64 + i - py * extra;
      const int y = y0 - pad + py, xe = x0 - pad + px;
      float v = -INFINITY;
      if ((unsigned)y < (unsigned)h && (unsigned)xe < (unsigned)w) {
        int e0[kMaxScales], e1[kMaxScales];
        float m0[kMaxScales], m1[kMaxScales];
        x_axes(xe, e0, e1, m0, m1);
        v = combine(y, e0, e1, m0, m1);
      }
      raw[py * PW + px] = v;
    }
  }
  if (used > 0) __syncthreads();                        // `stage` becomes the row-max buffer again
  return true;
}

template <class Map>
__device__ __forceinline__ bool nms_tile(const Map& m, int plane, int h, int w, int y0, int x0, int pad,
                                         float* raw, float* rowmax, AxisTab* ty, AxisTab* tx, int* pos_flag = nullptr,
                                         int rowmax_floats = (kTH + 2 * kMaxPad) * kTW, float* tbuf = nullptr) {
  // raw: (kTH+2p) x (kTW+2p) samples (-inf outside the image); rowmax: horizontal window max
  const int PW = kTW + 2 * pad, PH = kTH + 2 * pad;
  if (!fill_raw(m, plane, h, w, y0, x0, pad, raw, ty, tx, rowmax, rowmax_floats, pos_flag, tbuf)) return false;
  __syncthreads();
  if (pad == 2 && tbuf != nullptr) {
    // 5-wide window, 8 outputs per thread from 12 inputs (three 16-byte reads, two 16-byte writes) instead of
    // five 4-byte reads per output; max is exact, so any grouping gives the same bits
    for (int i = threadIdx.x; i < PH * (kTW / 8); i += 256) {
      const int py = i / (kTW / 8), g8 = i - py * (kTW / 8);
      const float4* src = reinterpret_cast<const float4*>(raw + py * PW + 8 * g8);
      const float4 q0 = src[0], q1 = src[1], q2 = src[2];
      const float x[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
      float pr[11], o[8];
#pragma unroll
      for (int j = 0; j < 11; ++j) pr[j] = fmaxf(x[j], x[j + 1]);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = fmaxf(fmaxf(pr[j], pr[j + 2]), x[j + 4]);
      float4* dst = reinterpret_cast<float4*>(rowmax + py * kTW + 8 * g8);
      dst[0] = make_float4(o[0], o[1], o[2], o[3]);
      dst[1] = make_float4(o[4], o[5], o[6], o[7]);
    }
    __syncthreads();
    return true;
  }
  for (int i = threadIdx.x; i < PH * kTW; i += 256) {
    const int py = i / kTW, px = i - py * kTW;
    float v = raw[py * PW + px];
    for (int d = 1; d <= 2 * pad; ++d) v = fmaxf(v, raw[py * PW + px + d]);
    rowmax[i] = v;
  }
  __syncthreads();
  return true;
}

template <class Map>
__global__ void __launch_bounds__(256) nms_kernel(Map m, int h, int w, int pad, float* out) {
  __shared__ float raw[(kTH + 2 * kMaxPad) * (kTW + 2 * kMaxPad)];
  __shared__ float rowmax[(kTH + 2 * kMaxPad) * kTW];
  const int tiles_x = (w + kTW - 1) / kTW;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, plane = blockIdx.y;
  const int y0 = ty * kTH, x0 = tx * kTW;
  __shared__ AxisTab taby, tabx;
  nms_tile(m, plane, h, w, y0, x0, pad, raw, rowmax, &taby, &tabx);
  const int PW = kTW + 2 * pad;
  for (int i = threadIdx.x; i < kTH * kTW; i += 256) {
    const int ly = i / kTW, lx = i - ly * kTW;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= h || x >= w) continue;
    float mx = rowmax[ly * kTW + lx];
    for (int d = 1; d <= 2 * pad; ++d) mx = fmaxf(mx, rowmax[(ly + d) * kTW + lx]);
    const float v = raw[(ly + pad) * PW + lx + pad];
    out[((size_t)plane * h + y) * w + x] = v * (mx == v ? 1.f : 0.f);   // det * (maxm == det).float()
  }
}

// ---------------------------------------------------------------------------
// top-K, phase 1: per tile, the K best positive local maxima as sorted keys
// ---------------------------------------------------------------------------
template <class Map, int PAD>     // PAD >= 0: the NMS padding as a compile-time constant (divisions by PW become shifts/muls)
__global__ void __launch_bounds__(256) topk_tile_kernel(Map m, int h, int w, int pad_rt, int K, u64* cand, int fast,
                                                        int planes, int tiles) {
  const int pad = PAD >= 0 ? PAD : pad_rt;
  // Workgroups are dealt to the 8 XCDs round robin (blockIdx.x % 8).  An XCD takes whole planes and walks their
  // tiles in row-major order: horizontally and vertically adjacent tiles share the 128-byte lines at the edges of
  // their source rectangles (36 floats per row of a 2x upsampled map: 2-3 lines for 1.1 lines of payload), and with
  // (tile, plane) as the grid they were fetched once per XCD's L2 - 758 MB per batch for 279 MB of maps (PMC, round 2).
  const int xcd = (int)(blockIdx.x & 7u), slot = (int)(blockIdx.x >> 3);
  const int plane_l = slot / tiles;
  const int tile = slot - plane_l * tiles;
  const int plane = plane_l * 8 + xcd;
  if (plane >= planes) return;                             // grid padding (whole workgroup)
  const auto& pm = plane_view(m, plane, &h, &w);           // per-image sizes: this image's (h, w), its own tiling
  const int we = enc_width(m, w);
  constexpr int kP = PAD >= 0 ? PAD : kMaxPad;           // the common 5x5 window needs 19 KiB of tiles, not 21.8: one more block per CU
  __shared__ __attribute__((aligned(16))) float raw[(kTH + 2 * kP) * (kTW + 2 * kP)];
  __shared__ __attribute__((aligned(16))) float rowmax[(kTH + 2 * kP) * kTW];
  constexpr bool kFast = PAD == 2;                       // 5x5 window: separable sampling, register-blocked max passes
  __shared__ __attribute__((aligned(16))) float tbuf_s[kFast ? kTRows * (kTW + 4) : 4];
  float* const tbuf = kFast && fast ? tbuf_s : nullptr;
  __shared__ u64 red[4];
  const int tiles_x = (w + kTW - 1) / kTW;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y0 = ty * kTH, x0 = tx * kTW;
  __shared__ AxisTab taby, tabx;
  __shared__ u64 clist[kMaxCand];
  __shared__ int ccount, any_positive;
  if (threadIdx.x == 0) { ccount = 0; any_positive = 0; }
  // the grid is sized for the largest image of the batch: a tile beyond this image's own leaves an empty list
  if ((PerImageSize<Map>::value && y0 >= h) ||
      !nms_tile(pm, plane, h, w, y0, x0, pad, raw, rowmax, &taby, &tabx, &any_positive, (kTH + 2 * kP) * kTW, tbuf)) {
    u64* outp0 = cand + ((size_t)plane * tiles + tile) * K;                 // nothing positive under this tile
    for (int r = threadIdx.x; r < K; r += 256) outp0[r] = 0;
    return;
  }
  const int PW = kTW + 2 * pad;
  u64 mine[8];   // this thread's 8 pixels as keys (0 = not a positive local maximum)
  if (tbuf != nullptr) {
    // thread = 2 rows x 4 columns: six 16-byte reads of the row maxima give both vertical windows
    const int ry = threadIdx.x >> 4, cg = threadIdx.x & 15;
    const int ly = 2 * ry, lx = 4 * cg;
    float4 rm[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) rm[d] = *reinterpret_cast<const float4*>(rowmax + (ly + d) * kTW + lx);
    const float mid[4] = {fmaxf(fmaxf(rm[1].x, rm[2].x), fmaxf(rm[3].x, rm[4].x)), fmaxf(fmaxf(rm[1].y, rm[2].y), fmaxf(rm[3].y, rm[4].y)),
                          fmaxf(fmaxf(rm[1].z, rm[2].z), fmaxf(rm[3].z, rm[4].z)), fmaxf(fmaxf(rm[1].w, rm[2].w), fmaxf(rm[3].w, rm[4].w))};
    const float top[4] = {rm[0].x, rm[0].y, rm[0].z, rm[0].w}, bot[4] = {rm[5].x, rm[5].y, rm[5].z, rm[5].w};
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const float2* c2 = reinterpret_cast<const float2*>(raw + (ly + rr + 2) * PW + lx + 2);   // 8-byte aligned
      const float2 va = c2[0], vb = c2[1];
      const float v4[4] = {va.x, va.y, vb.x, vb.y};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float mx = fmaxf(mid[j], rr == 0 ? top[j] : bot[j]);
        const int y = y0 + ly + rr, x = x0 + lx + j;
        u64 key = 0;
        if (y < h && x < w && mx == v4[j] && v4[j] > 0.f) key = make_key(v4[j], (unsigned)(y * we + x));
        mine[rr * 4 + j] = key;
        if (key != 0) {
          const int pos = atomicAdd(&ccount, 1);
          if (pos < kMaxCand) clist[pos] = key;
        }
      }
    }
  } else {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int i = threadIdx.x + q * 256;
    const int ly = i / kTW, lx = i - ly * kTW;
    const int y = y0 + ly, x = x0 + lx;
    u64 key = 0;
    if (y < h && x < w) {
      float mx = rowmax[ly * kTW + lx];
      for (int d = 1; d <= 2 * pad; ++d) mx = fmaxf(mx, rowmax[(ly + d) * kTW + lx]);
      const float v = raw[(ly + pad) * PW + lx + pad];
      if (mx == v && v > 0.f) key = make_key(v, (unsigned)(y * we + x));
    }
    mine[q] = key;
    if (key != 0) {                 // compact the (few) local maxima of the tile
      const int pos = atomicAdd(&ccount, 1);
      if (pos < kMaxCand) clist[pos] = key;
    }
  }
  }
  __syncthreads();
  u64* outp = cand + ((size_t)plane * tiles + tile) * K;
  const int nc = ccount;
  if (nc <= kMaxCand) {
    // rank sort: keys are unique (the pixel index is part of the key), so the rank of a key is
    // the number of larger ones; one pass, no further barriers
    for (int t = threadIdx.x; t < nc; t += 256) {
      const u64 key = clist[t];
      int rank = 0;
      for (int j = 0; j < nc; ++j) rank += clist[j] > key ? 1 : 0;
      if (rank < K) outp[rank] = key;
    }
    for (int r = nc + threadIdx.x; r < K; r += 256) outp[r] = 0;
    return;
  }
  // plateau-heavy tile (more local maxima than the list holds): K rounds of a block-wide max
  for (int k = 0; k < K; ++k) {
    u64 best = mine[0];
#pragma unroll
    for (int q = 1; q < 8; ++q) best = mine[q] > best ? mine[q] : best;
    best = block_max(best, red);
    if (threadIdx.x == 0) outp[k] = best;
    if (best == 0) {              // exhausted: the rest of the list is empty
      for (int r = k + 1 + threadIdx.x; r < K; r += 256) outp[r] = 0;
      break;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (mine[q] == best) mine[q] = 0;
  }
}

// ---------------------------------------------------------------------------
// top-K, phase 2: merge the per-tile lists of one plane, gather tags, pad with
// zero-valued pixels in index order (what a stable top-k of the NMS map gives)
// ---------------------------------------------------------------------------
template <class Map>
__device__ float nms_value_at(const Map& m, int plane, int h, int w, int pad, int y, int x) {
  const float v = m.at(plane, y, x);
  float mx = v;
  for (int dy = -pad; dy <= pad; ++dy)
    for (int dx = -pad; dx <= pad; ++dx) {
      const int yy = y + dy, xx = x + dx;
      if ((unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w) mx = fmaxf(mx, m.at(plane, yy, xx));
    }
  return v * (mx == v ? 1.f : 0.f);
}

template <class Map, class TagMap>
__global__ void __launch_bounds__(256) topk_merge_kernel(Map m, TagMap tm, int tag_shared_joints, int D,
                                                         int h, int w, int pad, int K, int tiles,
                                                         u64* cand, float* val_k, int* ind_k, float* tag_k) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  u64* red = reinterpret_cast<u64*>(smem_raw);          // 4 entries
  u64* lkeys = red + 4;
  const int plane = blockIdx.x;
  const auto& pm = plane_view(m, plane, &h, &w);
  const int we = enc_width(m, w);
  const int n = tiles * K;
  u64* gk = cand + (size_t)plane * n;
  constexpr int kOwn = 8;
  const bool merge_heads = tiles <= kOwn * 256;
  const bool use_lds = !merge_heads && (size_t)n * 8 + 32 <= 150 * 1024;
  u64* keys = gk;                                         // flat pointer: LDS copy when it fits
  if (use_lds) {
    for (int i = threadIdx.x; i < n; i += 256) lkeys[i] = gk[i];
    __syncthreads();
    keys = lkeys;
  }
  const int tag_plane = tag_shared_joints > 0 ? plane / tag_shared_joints : plane;
  const auto& pt = plane_tag(tm, tag_plane);
  int found = 0;
  if (merge_heads) {
    // every tile list is sorted (largest first, zeros behind): only the heads compete.  A thread keeps the
    // head of each of its (<= kOwn) tiles in registers and re-reads one key after it won a round
    u64 head[kOwn];
    int pos[kOwn];
#pragma unroll
    for (int o = 0; o < kOwn; ++o) {
      const int t = threadIdx.x + o * 256;
      pos[o] = 0;
      head[o] = t < tiles ? gk[(size_t)t * K] : 0;
    }
    for (int k = 0; k < K; ++k) {
      u64 mine = head[0];
#pragma unroll
      for (int o = 1; o < kOwn; ++o) mine = head[o] > mine ? head[o] : mine;
      const u64 best = block_max(mine, red);
      if (best == 0) break;
#pragma unroll
      for (int o = 0; o < kOwn; ++o)
        if (head[o] == best) {                               // keys are unique: exactly one owner
          ++pos[o];
          head[o] = pos[o] < K ? gk[(size_t)(threadIdx.x + o * 256) * K + pos[o]] : 0;
        }
      if (threadIdx.x == 0) {
        const unsigned idx = 0xffffffffu - (unsigned)(best & 0xffffffffu);
        val_k[(size_t)plane * K + k] = unorder_bits((unsigned)(best >> 32));
        ind_k[(size_t)plane * K + k] = (int)idx;
      }
      ++found;
      __syncthreads();
    }
  } else
  for (int k = 0; k < K; ++k) {
    u64 best = 0;
    for (int i = threadIdx.x; i < n; i += 256) best = keys[i] > best ? keys[i] : best;
    best = block_max(best, red);
    if (best == 0) break;
    for (int i = threadIdx.x; i < n; i += 256)
      if (keys[i] == best) keys[i] = 0;
    if (threadIdx.x == 0) {
      const unsigned idx = 0xffffffffu - (unsigned)(best & 0xffffffffu);
      val_k[(size_t)plane * K + k] = unorder_bits((unsigned)(best >> 32));
      ind_k[(size_t)plane * K + k] = (int)idx;
    }
    ++found;
    __syncthreads();
  }
  // zero padding: the first K - found pixels, in index order, whose NMS value is zero.  256 pixels per round,
  // one per thread (a round almost always suffices); each thread's rank among the zero-valued ones comes from
  // a ballot + the wave totals.  (One thread walking the pixels cost 200 us per batch: 25 bilinear samples per
  // pixel, one after the other, in every plane with fewer than K positive maxima - most planes.)
  {
    int* wtot = reinterpret_cast<int*>(red);               // 4 wave totals (red is free here)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int total_px = h * w;
    __syncthreads();
    for (int base = 0; found < K && base < total_px; base += 256) {
      const int idx = base + threadIdx.x;
      bool z = false;
      if (idx < total_px) z = nms_value_at(pm, plane, h, w, pad, idx / w, idx - (idx / w) * w) == 0.f;
      const unsigned long long mask = __ballot(z);
      if (lane == 0) wtot[wv] = __popcll(mask);
      __syncthreads();
      int before = __popcll(mask & ((1ull << lane) - 1ull));
      int total = 0;
      for (int i = 0; i < 4; ++i) { before += i < wv ? wtot[i] : 0; total += wtot[i]; }
      const int k = found + before;
      if (z && k < K) {
        val_k[(size_t)plane * K + k] = 0.f;
        ind_k[(size_t)plane * K + k] = (int)enc_index(m, (unsigned)idx, w);
      }
      found = found + total < K ? found + total : K;
      __syncthreads();
    }
    for (int k = found + threadIdx.x; k < K; k += 256) { val_k[(size_t)plane * K + k] = 0.f; ind_k[(size_t)plane * K + k] = 0; }
  }
  __syncthreads();
  __threadfence_block();
  for (int i = threadIdx.x; i < K * D; i += 256) {
    const int k = i / D, d = i - k * D;
    const int idx = ind_k[(size_t)plane * K + k];
    tag_k[((size_t)plane * K + k) * D + d] = pt.at(tag_plane, idx / we, idx - (idx / we) * we, d);
  }
}

struct DirectTag {          // (planes, h, w, D)
  const float* p;
  int h, w, D;
  __device__ __forceinline__ float at(int plane, int y, int x, int d) const {
    return p[(((size_t)plane * h + y) * w + x) * D + d];
  }
};

// ---------------------------------------------------------------------------
// adjust + refine: one workgroup per (person, joint)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float pairwise8_sum(const float* a, int n) {   // numpy contiguous f32 add.reduce
  if (n < 8) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s = s + a[i];
    return s;
  }
  float r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i + 8 <= n; i += 8)
    for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
  float s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) s = s + a[i];
  return s;
}

constexpr int kMaxJ = 32, kMaxD = 32;
constexpr int kRefineGroup = 16;     // people handled per pass over the pixels
constexpr int kRefineStripes = 10;   // row stripes per (image, joint) map (refine scan)
constexpr int kArgmaxStripes = 20;   // plane-maximum pass: half the rows per block = half the staged source rows (24 KiB:
                                     // six blocks per CU instead of three)

// (1) one block per person: copy rows, adjust detected joints (group.py:181-200),
//     mean tag of the detected joints (group.py:214-222), score (group.py:272)
template <class Map>
__global__ void __launch_bounds__(64) adjust_prepare_kernel(Map m, int J, int h, int w, int D,
                                                            const float* ans_in, float* ans_out,
                                                            const int* person_img, int do_adjust,
                                                            float* scores, float* mean_tag, const int* P_dev) {
  const int p = blockIdx.x, j = threadIdx.x;
  if (P_dev != nullptr && p >= *P_dev) return;               // P_dev: the grid covers the capacity, the people end here
  const int row_len = 3 + D;
  const float* kp = ans_in + (size_t)p * J * row_len;
  const int img = person_img ? person_img[p] : 0;
  const auto& pm = plane_view(m, img * J, &h, &w);
  if (j < J) {
    float* out = ans_out + ((size_t)p * J + j) * row_len;
    for (int c = 0; c < row_len; ++c) out[c] = kp[j * row_len + c];
    if (do_adjust && kp[j * row_len + 2] > 0.f) {
      const int plane = img * J + j;
      float cx = kp[j * row_len + 0], cy = kp[j * row_len + 1];
      const int col = (int)cx, row = (int)cy;
      const int cr = col + 1 < w - 1 ? col + 1 : w - 1, cl = col - 1 > 0 ? col - 1 : 0;
      const int rd = row + 1 < h - 1 ? row + 1 : h - 1, ru = row - 1 > 0 ? row - 1 : 0;
      cx += pm.at(plane, row, cr) > pm.at(plane, row, cl) ? 0.25f : -0.25f;
      cy += pm.at(plane, rd, col) > pm.at(plane, ru, col) ? 0.25f : -0.25f;
      out[0] = cx + 0.5f;
      out[1] = cy + 0.5f;
    }
  }
  if (j == 0) {
    float v[kMaxJ];
    if (scores) {
      for (int q = 0; q < J; ++q) v[q] = kp[q * row_len + 2];
      scores[p] = pairwise8_sum(v, J) / (float)J;
    }
    for (int d = 0; d < D; ++d) {
      int n = 0;
      for (int q = 0; q < J; ++q)
        if (kp[q * row_len + 2] > 0.f) v[n++] = kp[q * row_len + 3 + d];
      float s;
      if (D == 1) {
        s = pairwise8_sum(v, n);
      } else {
        s = 0.f;
        for (int i = 0; i < n; ++i) s = s + v[i];
      }
      mean_tag[(size_t)p * D + d] = s / (float)n;
    }
  }
}

// (1b) shortcut for the arg-max of refine (group.py:229-233).  The score of person p at pixel x is
//      det(x) - round(|tag(x) - mean_p|) <= det(x).  Let q* be the FIRST pixel attaining max det of the
//      plane: if the penalty of p at q* is 0, then q* is exactly np.argmax of p's score map (no pixel
//      can score higher than max det, and one that ties it is a later det maximum).  Only the
//      (person, joint) pairs whose penalty at q* is not 0 need the full scan below.
template <class Map>
__device__ __forceinline__ void argmax_rows(const Map& m, int plane, int w, int y_begin, int y_end, float* bv,
                                            unsigned* bi, float*, int) {
  const int npix = (y_end - y_begin) * w;
  int y = y_begin + (int)(threadIdx.x / (unsigned)w), x = (int)(threadIdx.x % (unsigned)w);
  const int dy = 256 / w, dx = 256 - dy * w;
  for (int i = threadIdx.x; i < npix; i += 256) {
    const float dv = m.at(plane, y, x);
    const bool up = dv > *bv || *bi == 0xffffffffu;          // increasing index order: '>' keeps the first maximum
    *bv = up ? dv : *bv;
    *bi = up ? (unsigned)(y * w + x) : *bi;
    x += dx; y += dy;
    if (x >= w) { x -= w; y += 1; }
  }
}

// bilinear maps: a thread owns up to 8 fixed columns (their x-axis taps and weights stay in registers),
// the y-axis taps of a row are the same for the whole block; per pixel 4 loads + 5 flops remain
template <>
__device__ __forceinline__ void argmax_rows<BilinearMap>(const BilinearMap& m, int plane, int w, int y_begin,
                                                         int y_end, float* bv, unsigned* bi, float* lds,
                                                         int lds_floats) {
  constexpr int kCols = 8;
  if (w > 256 * kCols) {                                      // very wide maps: the generic walk
    const int npix = (y_end - y_begin) * w;
    int y = y_begin + (int)(threadIdx.x / (unsigned)w), x = (int)(threadIdx.x % (unsigned)w);
    const int dy = 256 / w, dx = 256 - dy * w;
    for (int i = threadIdx.x; i < npix; i += 256) {
      const float dv = m.at(plane, y, x);
      const bool up = dv > *bv || *bi == 0xffffffffu;
      *bv = up ? dv : *bv;
      *bi = up ? (unsigned)(y * w + x) : *bi;
      x += dx; y += dy;
      if (x >= w) { x -= w; y += 1; }
    }
    return;
  }
  const int n = plane / m.J, j = plane - n * m.J;
  const bool small_tail = m.tail(plane);
  const float* b = m.p + (size_t)n * m.img_stride + (size_t)j * m.sh * m.sw;
  // the source rows of the stripe are contiguous in memory: one coalesced copy into LDS, then the four
  // taps of every pixel come from there (the gather of 4-byte taps through L1 was the whole cost)
  int sr0, sr1, t0i, t1i;
  float tf0, tf1;
  m.ay.at(y_begin, &sr0, &t0i, &tf0, &tf1);
  m.ay.at(y_end - 1, &t1i, &sr1, &tf0, &tf1);
  const int nsrc = (sr1 - sr0 + 1) * m.sw;
  const bool staged = lds != nullptr && nsrc > 0 && nsrc <= lds_floats;
  if (staged) {
    const float* g = b + sr0 * m.sw;
    for (int i = threadIdx.x; i < nsrc; i += 256) lds[i] = g[i];
    __syncthreads();
  }
  int c0[kCols], c1[kCols];
  float lx0[kCols], lx1[kCols];
#pragma unroll
  for (int k = 0; k < kCols; ++k) {
    const int x = threadIdx.x + k * 256;
    c0[k] = c1[k] = 0; lx0[k] = lx1[k] = 0.f;
    if (x < w) m.ax.at(x, &c0[k], &c1[k], &lx0[k], &lx1[k]);
  }
  for (int y = y_begin; y < y_end; ++y) {
    int r0, r1;
    float ly0, ly1;
    m.ay.at(y, &r0, &r1, &ly0, &ly1);
    const int o0 = (staged ? r0 - sr0 : r0) * m.sw, o1 = (staged ? r1 - sr0 : r1) * m.sw;
#pragma unroll
    for (int k = 0; k < kCols; ++k) {
      const int x = threadIdx.x + k * 256;
      if (x < w) {
        float v00, v01, v10, v11;
        if (staged) {                                         // uniform branch: LDS taps
          v00 = lds[o0 + c0[k]]; v01 = lds[o0 + c1[k]]; v10 = lds[o1 + c0[k]]; v11 = lds[o1 + c1[k]];
        } else {
          v00 = b[o0 + c0[k]]; v01 = b[o0 + c1[k]]; v10 = b[o1 + c0[k]]; v11 = b[o1 + c1[k]];
        }
        float dv;
        if (m.small) {                                        // uniform branch
          dv = bilinear_small(v00, v01, v10, v11, ly0, ly1, lx0[k], lx1[k], small_tail);
        } else {
          const float t0 = __builtin_fmaf(v00, lx0[k], v01 * lx1[k]);
          const float t1 = __builtin_fmaf(v10, lx0[k], v11 * lx1[k]);
          dv = __builtin_fmaf(t0, ly0, t1 * ly1);
        }
        const bool up = dv > *bv || *bi == 0xffffffffu;      // a thread's pixels come in increasing index order
        *bv = up ? dv : *bv;
        *bi = up ? (unsigned)(y * w + x) : *bi;
      }
    }
  }
}

template <class Map>
__global__ void __launch_bounds__(256) plane_argmax_kernel(Map m, int h, int w, u64* plane_key, int lds_floats,
                                                           const unsigned char* known) {
  extern __shared__ __attribute__((aligned(16))) float argmax_src[];
  __shared__ u64 red[4];
  const int plane = blockIdx.y;
  if (known != nullptr && known[plane]) return;            // its maximum came with the top-k table
  const auto& pm = plane_view(m, plane, &h, &w);
  const int rows = (h + gridDim.x - 1) / gridDim.x;
  const int y_begin = blockIdx.x * rows, y_end = min(h, y_begin + rows);
  if (y_begin >= y_end) return;
  float bv = -INFINITY;
  unsigned bi = 0xffffffffu;
  argmax_rows(pm, plane, w, y_begin, y_end, &bv, &bi, lds_floats > 0 ? argmax_src : nullptr, lds_floats);
  const u64 k = block_max(bi == 0xffffffffu ? 0 : make_key(bv, enc_index(m, bi, w)), red);
  if (threadIdx.x == 0 && k != 0) atomicMax(&plane_key[plane], k);
}

// the first pixel that attains a plane's maximum, taken from the top-k table of the same map (possibly in pinned
// host memory: one read per plane here, not one per missing joint): its first entry - the best positive 5x5
// local maximum, ties by lowest index - IS that pixel whenever the maximum is positive; otherwise 0 = full scan
__global__ void __launch_bounds__(256) plane_key_from_topk_kernel(const float* topk_val, const int* topk_ind, int K,
                                                                  int n_planes, u64* plane_key, unsigned char* known) {
  const int plane = blockIdx.x * 256 + threadIdx.x;
  if (plane >= n_planes) return;
  const float v = topk_val[(size_t)plane * K];
  plane_key[plane] = v > 0.f ? make_key(v, (unsigned)topk_ind[(size_t)plane * K]) : 0;
  known[plane] = v > 0.f;                                  // the others (nowhere positive) still need the pass
}

template <class TagMap>
__global__ void __launch_bounds__(256) refine_shortcut_kernel(TagMap tm, int J, int w, int D, const float* ans_in,
                                                              const int* person_img, int P, const float* mean_tag,
                                                              const u64* plane_key, u64* best_key,
                                                              unsigned char* need_scan, const int* P_dev) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P * J) return;
  const int p = i / J, j = i - p * J;
  if (P_dev != nullptr && p >= *P_dev) return;
  const int row_len = 3 + D;
  need_scan[i] = 0;
  if (ans_in[(size_t)i * row_len + 2] != 0.f) return;       // only missing joints are refined
  const int plane = (person_img ? person_img[p] : 0) * J + j;
  const u64 key = plane_key[plane];
  if (key == 0) { need_scan[i] = 1; return; }
  const int idx = (int)(0xffffffffu - (unsigned)(key & 0xffffffffu));
  const int y = idx / w, x = idx - y * w;                    // w: the width the indices are encoded with
  const auto& pt = plane_tag(tm, plane);
  float ss;                                                  // the exact expressions of refine_scan_kernel
  if (D == 1) {
    const float d0 = pt.at(plane, y, x, 0) - mean_tag[p];
    ss = d0 * d0;
  } else if (D < 8) {
    const float d0 = pt.at(plane, y, x, 0) - mean_tag[(size_t)p * D];
    ss = d0 * d0;
    for (int d = 1; d < D; ++d) { const float dd = pt.at(plane, y, x, d) - mean_tag[(size_t)p * D + d]; ss = ss + dd * dd; }
  } else {
    float sq[kMaxD];
    for (int d = 0; d < D; ++d) { const float dd = pt.at(plane, y, x, d) - mean_tag[(size_t)p * D + d]; sq[d] = dd * dd; }
    ss = pairwise8_sum(sq, D);
  }
  if (rintf(sqrtf(ss)) == 0.f) best_key[i] = key;            // score = det - 0: the key of the plane maximum
  else need_scan[i] = 1;
}

// (2) one block per (image, joint, row stripe): every person of the image that
//     misses this joint is scored against every pixel of the stripe; the map is
//     sampled once per pixel for all of them.  arg-max keys are merged with
//     atomicMax (value bits << 32 | ~index: the first maximum wins, as np.argmax)
template <class Map, class TagMap, bool kD1>
__global__ void __launch_bounds__(256) refine_scan_kernel(Map m, TagMap tm, int J, int h, int w, int D,
                                                          const float* ans_in, const int* person_img, int P,
                                                          const float* mean_tag, u64* best_key,
                                                          const unsigned char* need_scan, const int* P_dev) {
  __shared__ int lo_hi[2];
  __shared__ int n_need;
  __shared__ int need[512];
  __shared__ u64 red[kRefineGroup];
  __shared__ float gmean[kRefineGroup * kMaxD];
  const int plane = blockIdx.y, img = plane / J, j = plane - img * J;
  const auto& pm = plane_view(m, plane, &h, &w);
  const auto& pt = plane_tag(tm, plane);
  const int we = enc_width(m, w);
  const int row_len = 3 + D;
  if (threadIdx.x == 0) {
    if (P_dev != nullptr) P = *P_dev;        // P was the capacity: the rows beyond the people were never written
    int lo = 0, hi = P;                      // persons are sorted by image: [lo, hi) = this image
    if (person_img) {
      int a = 0, b = P;
      while (a < b) { const int c = (a + b) >> 1; if (person_img[c] < img) a = c + 1; else b = c; }
      lo = a; b = P;
      while (a < b) { const int c = (a + b) >> 1; if (person_img[c] <= img) a = c + 1; else b = c; }
      hi = a;
    } else if (img != 0) {
      hi = 0;
    }
    lo_hi[0] = lo; lo_hi[1] = hi;
    n_need = 0;
  }
  __syncthreads();
  const int lo = lo_hi[0], hi = lo_hi[1];
  const int rows = (h + gridDim.x - 1) / gridDim.x;
  const int y_begin = blockIdx.x * rows, y_end = min(h, y_begin + rows);
  if (y_begin >= y_end) return;
  const int npix = (y_end - y_begin) * w;
  for (int base = lo; base < hi; base += 512) {          // people needing joint j, 512 at a time
    __syncthreads();
    if (threadIdx.x == 0) n_need = 0;
    __syncthreads();
    for (int p = base + threadIdx.x; p < min(hi, base + 512); p += 256)
      if (ans_in[((size_t)p * J + j) * row_len + 2] == 0.f && (need_scan == nullptr || need_scan[(size_t)p * J + j]))
        need[atomicAdd(&n_need, 1)] = p;
    __syncthreads();
    const int nn = n_need;
    for (int g0 = 0; g0 < nn; g0 += kRefineGroup) {
      const int gn = min(kRefineGroup, nn - g0);
      __syncthreads();
      if (threadIdx.x < kRefineGroup) red[threadIdx.x] = 0;
      for (int i = threadIdx.x; i < gn * D; i += 256)
        gmean[(i / D) * kMaxD + i % D] = mean_tag[(size_t)need[g0 + i / D] * D + i % D];
      __syncthreads();
      // per-thread running arg-max: pixels are visited in increasing index order, so a
      // strict '>' keeps the first maximum (np.argmax, group.py:233)
      float bscore[kRefineGroup];
      unsigned bidx[kRefineGroup];
#pragma unroll
      for (int q = 0; q < kRefineGroup; ++q) { bscore[q] = -INFINITY; bidx[q] = 0xffffffffu; }
      if (kD1) {
        // D == 1 (what validate_hhrnet.py passes): branch-free over the 16 slots of the
        // group; unused slots (>= gn) carry mean 0 and are dropped afterwards
        float gm[kRefineGroup];
#pragma unroll
        for (int q = 0; q < kRefineGroup; ++q) gm[q] = q < gn ? gmean[q * kMaxD] : 0.f;
        int y = y_begin + (int)(threadIdx.x / (unsigned)w), x = (int)(threadIdx.x % (unsigned)w);
        const int dy = 256 / w, dx = 256 - dy * w;          // advance of 256 pixels in (y, x)
        for (int i = threadIdx.x; i < npix; i += 256) {
          const float dv = pm.at(plane, y, x);
          const float tv = pt.at(plane, y, x, 0);
          const unsigned idx = (unsigned)(y * we + x);
          bool slow = false;
          float kk[kRefineGroup];
#pragma unroll
          for (int q = 0; q < kRefineGroup; ++q) {
            const float a = fabsf(tv - gm[q]);
            kk[q] = rintf(a);
            // round(sqrt(fl(d*d))) == round(|d|) unless |d| sits within a few ulp of a
            // half-integer (sqrt(fl(a*a)) is within 1.5*2^-24 relative of a)
            slow |= fabsf(fabsf(a - kk[q]) - 0.5f) <= a * 4e-7f;
          }
          if (slow) {                                         // rare: the exact expression
#pragma unroll
            for (int q = 0; q < kRefineGroup; ++q) {
              const float d0 = tv - gm[q];
              kk[q] = rintf(sqrtf(d0 * d0));
            }
          }
#pragma unroll
          for (int q = 0; q < kRefineGroup; ++q) {
            const float score = dv - kk[q];
            const bool up = score > bscore[q] || bidx[q] == 0xffffffffu;
            bscore[q] = up ? score : bscore[q];
            bidx[q] = up ? idx : bidx[q];
          }
          x += dx; y += dy;
          if (x >= w) { x -= w; y += 1; }
        }
      } else {
        for (int i = threadIdx.x; i < npix; i += 256) {
          const int yy = i / w, x = i - yy * w, y = y_begin + yy;
          const float dv = pm.at(plane, y, x);
          const unsigned idx = (unsigned)(y * we + x);
          float tv[kMaxD];
          for (int d = 0; d < D; ++d) tv[d] = pt.at(plane, y, x, d);
          for (int q = 0; q < gn; ++q) {
            float ss;
            if (D < 8) {
              const float d0 = tv[0] - gmean[q * kMaxD];
              ss = d0 * d0;
              for (int d = 1; d < D; ++d) { const float dd = tv[d] - gmean[q * kMaxD + d]; ss = ss + dd * dd; }
            } else {
              float sq[kMaxD];
              for (int d = 0; d < D; ++d) { const float dd = tv[d] - gmean[q * kMaxD + d]; sq[d] = dd * dd; }
              ss = pairwise8_sum(sq, D);
            }
            const float score = dv - rintf(sqrtf(ss));
#pragma unroll
            for (int u = 0; u < kRefineGroup; ++u)            // static register indexing
              if (u == q && (score > bscore[u] || bidx[u] == 0xffffffffu)) { bscore[u] = score; bidx[u] = idx; }
          }
        }
      }
#pragma unroll
      for (int q = 0; q < kRefineGroup; ++q) {
        if (q < gn) {
          const u64 mine = bidx[q] == 0xffffffffu ? 0 : make_key(bscore[q], bidx[q]);
          const u64 k = wave_max(mine);
          if ((threadIdx.x & 63) == 0) atomicMax(&red[q], k);
        }
      }
      __syncthreads();
      if (threadIdx.x < gn)
        atomicMax(&best_key[(size_t)need[g0 + threadIdx.x] * J + j], red[threadIdx.x]);
    }
  }
}

// (3) fill the joints that were missing and whose arg-max has a positive value (group.py:233-262)
template <class Map>
__global__ void __launch_bounds__(256) refine_finalize_kernel(Map m, int J, int h, int w, int D,
                                                              const float* ans_in, float* ans_out,
                                                              const int* person_img, int P, const u64* best_key,
                                                              const int* P_dev) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P * J) return;
  const int p = i / J, j = i - p * J;
  if (P_dev != nullptr && p >= *P_dev) return;
  const int row_len = 3 + D;
  if (ans_in[(size_t)i * row_len + 2] != 0.f) return;
  const u64 key = best_key[i];
  if (key == 0) return;
  const int plane = (person_img ? person_img[p] : 0) * J + j;
  const auto& pm = plane_view(m, plane, &h, &w);
  const int we = enc_width(m, w);
  const int idx = (int)(0xffffffffu - (unsigned)(key & 0xffffffffu));
  const int y = idx / we, x = idx - y * we;
  const float v = pm.at(plane, y, x);
  if (v > 0.f) {
    const int xr = x + 1 < w - 1 ? x + 1 : w - 1, xl = x - 1 > 0 ? x - 1 : 0;
    const int yd = y + 1 < h - 1 ? y + 1 : h - 1, yu = y - 1 > 0 ? y - 1 : 0;
    float* out = ans_out + (size_t)i * row_len;
    out[0] = (float)x + 0.5f + (pm.at(plane, y, xr) > pm.at(plane, y, xl) ? 0.25f : -0.25f);
    out[1] = (float)y + 0.5f + (pm.at(plane, yd, x) > pm.at(plane, yu, x) ? 0.25f : -0.25f);
    out[2] = v;
  }
}

constexpr int kShortcutPlanes = 1 << 16;   // plane maxima kept for the arg-max shortcut (more planes: full scans only)
static size_t refine_scratch(int P, int J, int D) {
  return (size_t)P * J * sizeof(u64) + (size_t)P * D * sizeof(float) + 256 + (size_t)kShortcutPlanes * sizeof(u64) +
         (size_t)P * J + kShortcutPlanes;                  // + need_scan flags + per-plane "maximum known" flags
}

template <class Map, class TagMap>
static int adjust_refine_run(const Map& m, const TagMap& tm, int n_img, int J, int h, int w, int D,
                             const float* ans_in, float* ans_out, const int* person_img, int P, int do_adjust,
                             int do_refine, float* scores, void* scratch, size_t scratch_bytes, hipStream_t s,
                             const float* topk_val = nullptr, const int* topk_ind = nullptr, int topk_k = 0,
                             const int32_t* P_dev = nullptr) {
  // P_dev (device-visible): the number of people is read on the device and P is the capacity of the buffers - the
  // grids, the best_key memset and the offsets inside the scratch buffer are sized by P as ever, the kernels that
  // index people return at once for p >= *P_dev.  Null: P people, the launches as they always were.
  RTPE_REQUIRE(scratch && scratch_bytes >= refine_scratch(P, J, D), "adjust_refine: scratch too small");
  u64* best_key = reinterpret_cast<u64*>(scratch);
  float* mean_tag = reinterpret_cast<float*>(best_key + (size_t)P * J);
  hipLaunchKernelGGL((adjust_prepare_kernel<Map>), dim3(P), dim3(64), 0, s, m, J, h, w, D, ans_in, ans_out,
                     person_img, do_adjust, scores, mean_tag, P_dev);
  RTPE_HIP_CHECK(hipGetLastError());
  if (!do_refine) return RTPE_OK;
  RTPE_HIP_CHECK(hipMemsetAsync(best_key, 0, (size_t)P * J * sizeof(u64), s));
  unsigned char* need_scan = nullptr;
  if (n_img * J <= kShortcutPlanes) {
    char* tail = reinterpret_cast<char*>(mean_tag + (size_t)P * D);
    u64* plane_key = reinterpret_cast<u64*>(tail + ((256 - ((uintptr_t)tail & 255)) & 255));
    need_scan = reinterpret_cast<unsigned char*>(plane_key + kShortcutPlanes);
    unsigned char* known = nullptr;
    if (topk_val != nullptr) {
      known = need_scan + (size_t)P * J;
      hipLaunchKernelGGL(plane_key_from_topk_kernel, dim3((n_img * J + 255) / 256), dim3(256), 0, s, topk_val, topk_ind,
                         topk_k, n_img * J, plane_key, known);
    } else {
      RTPE_HIP_CHECK(hipMemsetAsync(plane_key, 0, (size_t)n_img * J * sizeof(u64), s));
    }
    hipLaunchKernelGGL((plane_argmax_kernel<Map>), dim3(kArgmaxStripes, n_img * J), dim3(256), 24 * 1024, s, m, h, w,
                       plane_key, 24 * 1024 / 4, known);
    RTPE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((refine_shortcut_kernel<TagMap>), dim3((P * J + 255) / 256), dim3(256), 0, s, tm, J,
                       enc_width(m, w), D, ans_in, person_img, P, mean_tag, plane_key, best_key, need_scan, P_dev);
    RTPE_HIP_CHECK(hipGetLastError());
  }
  if (D == 1)
    hipLaunchKernelGGL((refine_scan_kernel<Map, TagMap, true>), dim3(kRefineStripes, n_img * J), dim3(256), 0, s,
                       m, tm, J, h, w, D, ans_in, person_img, P, mean_tag, best_key, need_scan, P_dev);
  else
    hipLaunchKernelGGL((refine_scan_kernel<Map, TagMap, false>), dim3(kRefineStripes, n_img * J), dim3(256), 0, s,
                       m, tm, J, h, w, D, ans_in, person_img, P, mean_tag, best_key, need_scan, P_dev);
  RTPE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((refine_finalize_kernel<Map>), dim3((P * J + 255) / 256), dim3(256), 0, s, m, J, h, w, D,
                     ans_in, ans_out, person_img, P, best_key, P_dev);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------
static BilinearMap make_bilinear(const float* p, int sh, int sw, long long img_stride, int J, int oh, int ow) {
  BilinearMap m;
  m.p = p; m.sh = sh; m.sw = sw; m.J = J; m.img_stride = img_stride;
  m.small = small_output(oh, ow);
  m.ay = make_axis(sh, oh);
  m.ax = make_axis(sw, ow);
  return m;
}

static size_t topk_scratch(int planes, int h, int w, int K) {
  const size_t tiles = (size_t)((h + kTH - 1) / kTH) * ((w + kTW - 1) / kTW);
  return (size_t)planes * tiles * K * sizeof(u64);
}

template <class Map, class TagMap>
static int topk_run(const Map& m, const TagMap& tm, int planes, int tag_shared_joints, int D, int h, int w,
                    int K, int ksize, int pad, float* val_k, int* ind_k, float* tag_k, void* scratch,
                    size_t scratch_bytes, hipStream_t s) {
  RTPE_REQUIRE(ksize == 2 * pad + 1 && pad >= 0 && pad <= kMaxPad, "nms: ksize=%d pad=%d unsupported", ksize, pad);
  RTPE_REQUIRE(planes > 0 && h > 0 && w > 0 && K > 0 && (size_t)h * w < 0x7fffffffu, "topk: bad shape");
  RTPE_REQUIRE(scratch_bytes >= topk_scratch(planes, h, w, K), "topk: scratch too small");
  const int tiles = ((h + kTH - 1) / kTH) * ((w + kTW - 1) / kTW);
  u64* cand = reinterpret_cast<u64*>(scratch);
  // RTPE_TOPK_FAST=0: the 5x5 path without the separable sampling / register-blocked max passes (same bits)
  static const int fast = getenv("RTPE_TOPK_FAST") ? atoi(getenv("RTPE_TOPK_FAST")) : 1;
  const size_t grid = (size_t)((planes + 7) / 8) * 8 * tiles;                     // whole planes per XCD
  RTPE_REQUIRE(grid < 0x7fffffffu, "topk: %d planes x %d tiles do not fit one grid", planes, tiles);
  if (pad == 2)
    hipLaunchKernelGGL((topk_tile_kernel<Map, 2>), dim3((unsigned)grid), dim3(256), 0, s, m, h, w, pad, K, cand, fast, planes, tiles);
  else
    hipLaunchKernelGGL((topk_tile_kernel<Map, -1>), dim3((unsigned)grid), dim3(256), 0, s, m, h, w, pad, K, cand, 0, planes, tiles);
  RTPE_HIP_CHECK(hipGetLastError());
  size_t lds = 32 + (size_t)tiles * K * 8;
  if (lds > 150 * 1024 || tiles <= 8 * 256) lds = 32;     // the head merge (tiles <= kOwn * 256) needs no copy of the lists
  auto kern = topk_merge_kernel<Map, TagMap>;
  static unsigned long long attr_mask = 0;
  if (first_use_on_device(&attr_mask)) {
    RTPE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  }
  hipLaunchKernelGGL(kern, dim3(planes), dim3(256), lds, s, m, tm, tag_shared_joints, D, h, w, pad, K, tiles,
                     cand, val_k, ind_k, tag_k);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

// ---------------------------------------------------------------------------
// flip test, step 1: the four maps at the refined resolution (h2, w2) the projection samples, from the network
// outputs of the image (P (N,2J,h4,w4), R (N,J,h2,w2)) and of its mirror image (Pf, Rf), in ONE pass over them:
//     A_o = (rs(P[:, j]) + R[:, j]) / 2                        T_o = rs(P[:, J + j])
//     A_f = (flip(rs(Pf[:, q])) + flip(Rf[:, q])) / 2          T_f = flip(rs(Pf[:, J + q]))      q = perm[j]
// rs = align_corners=False to (h2, w2), flip = mirror of the RESIZED map (x -> w2 - 1 - x): the values the
// get_multi_stage_outputs calls of rtpe/inference.py write (rs, then dst + v and / 2 as separate operations).
// ---------------------------------------------------------------------------
struct FlipPrepArgs {
  const float *p, *r, *pf, *rf;
  long long p_st, r_st, pf_st, rf_st;   // elements between images
  int J, h4, w4, h2, w2;
  float sy, sx;                         // float(h4) / float(h2), float(w4) / float(w2)
  int perm[kMaxJ];
  int plane0;                           // first output plane: image offset * J (a sub-batch lands in a larger buffer)
  float *ao, *af, *to, *tf;             // (planes, h2, w2) each; those an instance does not write may be null
};

// FLIP: also the mirror image's maps (A_f, T_f); TAGS: also the tag maps (T_o, T_f); AGS: the j == 0 planes also write
// the image's shared tag plane rs(P[:, J]) to `to` at plane plane0 / J + n (the expression of T_o[:, 0]); TF = false:
// TAGS without T_f (the averaged-tag test reads the un-mirrored tag maps only); AVG (with FLIP): neither A_o nor A_f is
// written but their average H = (A_o + A_f) / 2, to `ao` (the decode without projection averages at this resolution)
template <bool FLIP, bool TAGS, bool AGS = false, bool TF = TAGS, bool AVG = false>
__device__ __forceinline__ void prep_planes(const FlipPrepArgs& a) {
  const int plane = blockIdx.y, n = plane / a.J, j = plane - n * a.J, q = a.perm[j];
  const int npix = a.h2 * a.w2;
  const size_t src_plane = (size_t)a.h4 * a.w4;
  const bool ident = a.h4 == a.h2 && a.w4 == a.w2;
  const float* P = a.p + (size_t)n * a.p_st;
  const float* R = a.r + (size_t)n * a.r_st + (size_t)j * npix;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
    const int y = i / a.w2, x = i - y * a.w2;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    axis_nc(a.sy, a.h4, a.h2, y, &y0, &y1, &ly0, &ly1);
    axis_nc(a.sx, a.w4, a.w2, x, &x0, &x1, &lx0, &lx1);
    const size_t o = (size_t)(a.plane0 + plane) * npix + i;
    const float ph = taps_nc(P + (size_t)j * src_plane, a.w4, ident, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
    const float ho = (ph + R[i]) / 2.f;
    if (!AVG) a.ao[o] = ho;
    if (TAGS) a.to[o] = taps_nc(P + (size_t)(a.J + j) * src_plane, a.w4, ident, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
    if (AGS && j == 0)
      a.to[(size_t)(a.plane0 / a.J + n) * npix + i] =
          taps_nc(P + (size_t)a.J * src_plane, a.w4, ident, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
    if (FLIP) {
      const float* Pf = a.pf + (size_t)n * a.pf_st;
      const float* Rf = a.rf + (size_t)n * a.rf_st + (size_t)q * npix;
      const int xs = a.w2 - 1 - x;
      int f0, f1;
      float lf0, lf1;
      axis_nc(a.sx, a.w4, a.w2, xs, &f0, &f1, &lf0, &lf1);
      const float fh = taps_nc(Pf + (size_t)q * src_plane, a.w4, ident, y0, y1, f0, f1, ly0, ly1, lf0, lf1);
      const float hf = (fh + Rf[(size_t)y * a.w2 + xs]) / 2.f;
      if (AVG) a.ao[o] = (ho + hf) / 2.f;
      else a.af[o] = hf;
      if (TF)
        a.tf[o] = taps_nc(Pf + (size_t)(a.J + q) * src_plane, a.w4, ident, y0, y1, f0, f1, ly0, ly1, lf0, lf1);
    }
  }
}

__global__ void __launch_bounds__(256) flip_prep_kernel(const FlipPrepArgs a) { prep_planes<true, true>(a); }

// multi-scale test, step 1 for one scale (and one sub-batch of its images): A_o [, A_f] [, T_o [, T_f]] of the scale
template <bool FLIP, bool TAGS>
__global__ void __launch_bounds__(256) ms_prep_kernel(const FlipPrepArgs a) { prep_planes<FLIP, TAGS>(a); }

// AGS multi-scale test, step 1 for the smallest scale: A_o [, A_f] of the scale and the images' shared tag planes
template <bool FLIP>
__global__ void __launch_bounds__(256) ags_prep_kernel(const FlipPrepArgs a) { prep_planes<FLIP, false, true>(a); }

// averaged-tag multi-scale test, step 1 for the smallest scale: A_o [, A_f] and the J un-mirrored tag maps T_o of the
// scale (tag_mean.hip's mean_plane_kernel reduces them behind this kernel)
template <bool FLIP>
__global__ void __launch_bounds__(256) mean_prep_kernel(const FlipPrepArgs a) { prep_planes<FLIP, true, false, false>(a); }

// decode without projection (include/rtpe_hip_noproj.h), step 1 for one scale with flip: H = (A_o + A_f) / 2 of the
// scale at its refined size [, T_o and T_f].  Without flip H = A_o: ms_prep_kernel<false, TAGS> writes it
template <bool TAGS>
__global__ void __launch_bounds__(256) np_prep_kernel(const FlipPrepArgs a) { prep_planes<true, TAGS, false, TAGS, true>(a); }

// step 2 for every scale but the first: F = F + rs(H) in place at the decode grid, then F = F / div on the last scale
// (div = 1: no division) - aggregate.hip's `dst + v`, then `/ div`, as separate operations.  One grid row per plane;
// a thread handles V consecutive pixels of a row (V = 4: 16-byte loads and stores of F; needs ow % 4 == 0)
struct NpAccumArgs {
  const float* h;           // (N*J, sh, sw): H of the scale
  float* f;                 // (N*J, oh, ow): F
  NcAxes a;                 // (sh, sw) -> (oh, ow)
  int plane0;               // first plane: image offset * J
  float div;
};

template <int V>
__global__ void __launch_bounds__(256) np_accum_kernel(const NpAccumArgs a) {
  const int plane = a.plane0 + blockIdx.y;
  const NcAxes& A = a.a;
  const long long npix = (long long)A.oh * A.ow;
  const float* src = a.h + (size_t)plane * A.sh * A.sw;
  float* dst = a.f + (size_t)plane * npix;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V; i < npix; i += (long long)gridDim.x * 256 * V) {
    const int y = (int)(i / A.ow), x = (int)(i - (long long)y * A.ow);
    int y0, y1;
    float ly0, ly1;
    axis_nc(A.sy, A.sh, A.oh, y, &y0, &y1, &ly0, &ly1);
    float v[V];
    if constexpr (V == 4) {
      const float4 d = *reinterpret_cast<const float4*>(dst + i);
      v[0] = d.x; v[1] = d.y; v[2] = d.z; v[3] = d.w;
    } else {
      v[0] = dst[i];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      int x0, x1;
      float lx0, lx1;
      axis_nc(A.sx, A.sw, A.ow, x + k, &x0, &x1, &lx0, &lx1);
      v[k] = v[k] + taps_nc(src, A.sw, A.ident, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
      if (a.div != 1.f) v[k] = v[k] / a.div;
    }
    if constexpr (V == 4) *reinterpret_cast<float4*>(dst + i) = make_float4(v[0], v[1], v[2], v[3]);
    else dst[i] = v[0];
  }
}

}  // namespace rtpe

using namespace rtpe;

extern "C" int rtpe_bilinear_upsample(const float* src, int32_t planes, int32_t h, int32_t w, float* dst,
                                      int32_t oh, int32_t ow, void* stream) {
  RTPE_REQUIRE(src && dst && planes > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "bilinear: bad argument");
  BilinearMap m = make_bilinear(src, h, w, 0, planes, oh, ow);   // one "image" of `planes` planes
  m.small = 0;    // (the channel of a plane within its F.interpolate call is not known here: the separable formula)
  const size_t total = (size_t)planes * oh * ow;
  size_t blocks = (total + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(bilinear_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     m, planes, oh, ow, dst);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

extern "C" int rtpe_nms(const float* det, int32_t planes, int32_t h, int32_t w, int32_t ksize, int32_t pad,
                        float* out, void* stream) {
  RTPE_REQUIRE(det && out && planes > 0 && h > 0 && w > 0, "nms: bad argument");
  RTPE_REQUIRE(ksize == 2 * pad + 1 && pad >= 0 && pad <= kMaxPad, "nms: ksize=%d pad=%d unsupported", ksize, pad);
  DirectMap m{det, h, w};
  const int tiles = ((h + kTH - 1) / kTH) * ((w + kTW - 1) / kTW);
  hipLaunchKernelGGL((nms_kernel<DirectMap>), dim3(tiles, planes), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), m, h, w, pad, out);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

extern "C" int rtpe_topk_scratch_bytes(int32_t planes, int32_t h, int32_t w, int32_t K, size_t* bytes) {
  RTPE_REQUIRE(bytes && planes > 0 && h > 0 && w > 0 && K > 0, "topk_scratch_bytes: bad argument");
  *bytes = topk_scratch(planes, h, w, K);
  return RTPE_OK;
}

extern "C" int rtpe_topk(const float* det, const float* tag, int32_t planes, int32_t joints,
                         int32_t tag_per_joint, int32_t h, int32_t w, int32_t D, int32_t K, int32_t nms_ksize,
                         int32_t nms_pad, float* val_k, int32_t* ind_k, float* tag_k, void* scratch,
                         size_t scratch_bytes, void* stream) {
  RTPE_REQUIRE(det && tag && val_k && ind_k && tag_k && scratch && D > 0 && joints > 0, "topk: bad argument");
  DirectMap m{det, h, w};
  DirectTag tm{tag, h, w, D};
  return topk_run(m, tm, planes, tag_per_joint ? 0 : joints, D, h, w, K, nms_ksize, nms_pad, val_k, ind_k, tag_k,
                  scratch, scratch_bytes, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int rtpe_adjust_refine_scratch_bytes(int32_t P, int32_t J, int32_t D, size_t* bytes) {
  RTPE_REQUIRE(bytes && P >= 0 && J > 0 && D > 0, "adjust_refine_scratch_bytes: bad argument");
  *bytes = refine_scratch(P, J, D);
  return RTPE_OK;
}

extern "C" int rtpe_adjust_refine(const float* det, const float* tag, int32_t N, int32_t J, int32_t h, int32_t w,
                                  int32_t D, const float* ans_in, float* ans_out, const int32_t* person_img,
                                  int32_t P, int32_t do_adjust, int32_t do_refine, float* scores, void* scratch,
                                  size_t scratch_bytes, void* stream) {
  RTPE_REQUIRE(det && tag && ((ans_in && ans_out && ans_in != ans_out) || P == 0) && N > 0 && J > 0 &&
                   J <= kMaxJ && D > 0 && D <= kMaxD,
               "adjust_refine: bad argument (J<=%d, D<=%d)", kMaxJ, kMaxD);
  if (P <= 0) return RTPE_OK;
  DirectMap m{det, h, w};
  DirectTag tm{tag, h, w, D};
  return adjust_refine_run(m, tm, N, J, h, w, D, ans_in, ans_out, person_img, P, do_adjust, do_refine, scores,
                           scratch, scratch_bytes, reinterpret_cast<hipStream_t>(stream));
}

// ---------------------------------------------------------------------------
// The batch decodes.  Every kind runs the same device stages over its own samplers: [prepare the maps,] fused NMS +
// top-k + tag gather (decode_topk), then - after the grouping - adjust + refine (decode_adjust_refine).  A kind is a
// host struct that holds the leading arguments of its entries, "where the maps of the batch are" (N, J, oh, ow among
// them), and knows two things: check(who) - RTPE_OK or the refusal, the entry's name `who` first in the message - and
// with_maps(f) - build the samplers and return f(Map, TagMap, D).  The entries build a kind and call a stage.
// ---------------------------------------------------------------------------
struct TopkTables {         // the candidate tables a top-k writes: (N,J,K), (N,J,K), (N,J,K,D)
  float* val_k;
  int32_t* ind_k;
  float* tag_k;
};

struct RefineTail {         // the ending every adjust + refine entry of the batch decodes shares
  const float* ans_in;
  float* ans_out;
  const int32_t* person_img;
  int32_t P, do_adjust, do_refine;
  float* scores;
  const float* topk_val;    // the top-k table of the same maps (the arg-max shortcut's plane maxima) or null, null, 0
  const int32_t* topk_ind;
  int32_t K;
  void* scratch;
  size_t scratch_bytes;
  void* stream;
};

// The two endings, as the entries declare them (the prototypes in include/ spell them out) and as they pass them on.
// (TOPK_PARAMS: where nothing stands between the top-k arguments; the multi-scale entries have maps_bytes there.)
#define TOPK_PARAMS                                                                                          \
  int32_t K, int32_t nms_ksize, int32_t nms_pad, float *val_k, int32_t *ind_k, float *tag_k, void *scratch,  \
      size_t scratch_bytes, void *stream
#define TOPK_ARGS K, nms_ksize, nms_pad, {val_k, ind_k, tag_k}, scratch, scratch_bytes, stream
#define REFINE_PARAMS                                                                                        \
  const float *ans_in, float *ans_out, const int32_t *person_img, int32_t P, int32_t do_adjust,              \
      int32_t do_refine, float *scores, const float *topk_val, const int32_t *topk_ind, int32_t K,           \
      void *scratch, size_t scratch_bytes, void *stream
#define REFINE_TAIL                                                                                          \
  RefineTail{ans_in, ans_out, person_img, P, do_adjust, do_refine, scores, topk_val, topk_ind, K, scratch,   \
             scratch_bytes, stream}

// what decode_topk refuses before it launches (rtpe_topk_flip asks first: its prepare kernel goes before the top-k)
template <class Src>
static int topk_check(const char* who, Src& src, int K, const TopkTables& t, const void* scratch) {
  const int rc = src.check(who);
  if (rc != RTPE_OK) return rc;
  RTPE_REQUIRE(t.val_k && t.ind_k && t.tag_k && scratch, "%s: null argument", who);
  RTPE_REQUIRE(src.oh > 0 && src.ow > 0 && K > 0, "%s: bad shape", who);
  return RTPE_OK;
}

template <class Src>
static int decode_topk(const char* who, Src src, int K, int ksize, int pad, const TopkTables& t, void* scratch,
                       size_t scratch_bytes, void* stream) {
  const int rc = topk_check(who, src, K, t, scratch);
  if (rc != RTPE_OK) return rc;
  // tag_shared_joints = 0: every kind's tag sampler takes the (image * J + joint) plane index
  return src.with_maps([&](const auto& m, const auto& tm, int D) {
    return topk_run(m, tm, src.N * src.J, 0, D, src.oh, src.ow, K, ksize, pad, t.val_k, t.ind_k, t.tag_k, scratch,
                    scratch_bytes, reinterpret_cast<hipStream_t>(stream));
  });
}

// The forms of an adjust + refine entry.  kNeedTopk: the entry has no form without the top-k table.  kCountOnDevice
// (the _n entries): the number of people is read on the device, from P_dev, and t.P is the capacity of ans_in /
// ans_out / person_img / scores and of the scratch buffer (adjust_refine_run); without it P_dev stays null: t.P people.
enum { kAnyForm = 0, kNeedTopk = 1, kCountOnDevice = 2 };
template <class Src>
static int decode_adjust_refine(const char* who, Src src, const RefineTail& t, int form,
                                const int32_t* P_dev = nullptr) {
  const bool need_topk = form & kNeedTopk;
  RTPE_REQUIRE(P_dev != nullptr || !(form & kCountOnDevice), "%s: P_dev is null", who);
  const int rc = src.check(who);
  if (rc != RTPE_OK) return rc;
  RTPE_REQUIRE(((t.ans_in && t.ans_out && t.ans_in != t.ans_out) || t.P == 0) && src.J <= kMaxJ,
               "%s: bad argument (ans_in and ans_out: two buffers; J <= %d)", who, kMaxJ);
  RTPE_REQUIRE((t.topk_val == nullptr) == (t.topk_ind == nullptr) && (t.topk_val == nullptr || t.K > 0) &&
                   (t.topk_val != nullptr || !need_topk),
               "%s: topk_val and topk_ind go together (K > 0)%s", who, need_topk ? " and are required" : "");
  if (t.P <= 0) return RTPE_OK;
  return src.with_maps([&](const auto& m, const auto& tm, int D) {
    return adjust_refine_run(m, tm, src.N, src.J, src.oh, src.ow, D, t.ans_in, t.ans_out, t.person_img, t.P,
                             t.do_adjust, t.do_refine, t.scores, t.scratch, t.scratch_bytes,
                             reinterpret_cast<hipStream_t>(t.stream), t.topk_val, t.topk_ind, t.K, P_dev);
  });
}

// ---------------------------------------------------------------------------
// The network outputs as they are: J refined heat maps per image and their tag maps, sampled align_corners=True, D = 1.
// ONE kind with two independent switches (include/rtpe_hip.h and rtpe_hip_shared.h / _sizes.h / _mixdec.h hold the
// prototypes of the four combinations):
//   shared  the tag is ONE plane per image, (N, 1, th, tw) at tg_img_stride, shared by the J joints (the dual-head
//           students; SharedBilinearTag / NetMixedTag) - else one tag map per joint.  Both maps may be channel slices
//           of one (N, J + 1, h, w) tensor: the strides say where an image's planes start.  Bit for bit the per-joint
//           decode of the tag plane expanded to J channels.
//   sized   every image is decoded at its own size, read from a table (SizeEntry, fill_size_table) - else at (oh, ow).
//           Then (oh, ow) are the largest height and the largest width of the batch - the tile grid, the scratch
//           buffer and the stripes are sized by them - and w_enc is the width of the flat indices.
// With both (a mixed-size batch decoded from its canvas) (hh, hw) / (th, tw) are the PITCH of the planes - the canvas
// extents, which only address.  Image n's own extents, which only clamp, are the n_in of its entry's axes
// (rtpe_decode_mixed_fill); the axes that make_bilinear derives from the pitch are never read (NetSizesMap,
// NetMixedTag).  Every heat-map kernel of a sized decode is the NetSizesMap instantiation, shared tag or not.
// ---------------------------------------------------------------------------
struct NetSrc {
  const float* hm;
  int32_t hh, hw;
  int64_t hm_img_stride;
  const float* tg;
  int32_t th, tw;
  int64_t tg_img_stride;
  int32_t N, J, oh, ow;
  bool shared, sized;
  const void* table;        // sized only
  size_t table_bytes;
  int32_t w_enc;
  // Each switch brings the checks its entries came with, no more: the shared kinds look at J <= kMaxJ (the top-k
  // too) and at the image strides, the kinds without the switches at neither, nor at the sizes of the maps.
  int check(const char* who) const {
    if (shared) {
      RTPE_REQUIRE(hm && tg && (table || !sized), "%s: null argument", who);
      RTPE_REQUIRE(N > 0 && J > 0 && J <= kMaxJ, "%s: bad argument (N=%d, J=%d; J <= %d)", who, N, J, kMaxJ);
    } else {
      RTPE_REQUIRE(hm && tg && (table || !sized) && N > 0 && J > 0, "%s: bad argument", who);
    }
    if (shared || sized)
      RTPE_REQUIRE(hh > 0 && hw > 0 && th > 0 && tw > 0 && oh > 0 && ow > 0, "%s: bad shape", who);
    if (shared)
      RTPE_REQUIRE(hm_img_stride >= (int64_t)J * hh * hw && tg_img_stride >= (int64_t)th * tw,
                   "%s: an image stride is below the size of an image's planes", who);
    if (!sized) return RTPE_OK;
    RTPE_REQUIRE(table_bytes >= (size_t)N * sizeof(SizeEntry), "%s: sizes table too small (%zu < %zu bytes)", who,
                 table_bytes, (size_t)N * sizeof(SizeEntry));
    RTPE_REQUIRE(w_enc >= ow, "%s: w_enc=%d is below the largest width %d", who, w_enc, ow);
    RTPE_REQUIRE((int64_t)oh * w_enc <= 0x7fffffff, "%s: y * w_enc + x exceeds 32 bits (max_oh=%d, w_enc=%d)", who, oh,
                 w_enc);
    return RTPE_OK;
  }
  template <class F>
  int with_maps(F f) const {
    const BilinearMap heat = make_bilinear(hm, hh, hw, hm_img_stride, J, oh, ow);
    const BilinearMap tag = make_bilinear(tg, th, tw, tg_img_stride, J, oh, ow);
    if (!sized) return shared ? f(heat, SharedBilinearTag{tag}, 1) : f(heat, BilinearTag{tag}, 1);
    const SizeEntry* tab = reinterpret_cast<const SizeEntry*>(table);
    const NetSizesMap m{heat, tab, w_enc};
    return shared ? f(m, NetMixedTag{tag, tab}, 1) : f(m, NetSizesTag{tag, tab}, 1);
  }
};

// The leading arguments of the thirteen entries - the maps, then one decode size or the table - and the NetSrc they
// make.  (The prototypes in the headers spell every list out; these follow them name for name.)
#define NET_MAPS_PARAMS                                                                                        \
  const float *hm, int32_t hh, int32_t hw, int64_t hm_img_stride, const float *tg, int32_t th, int32_t tw,     \
      int64_t tg_img_stride, int32_t N, int32_t J
#define NET_TABLE_PARAMS \
  const void *sizes_table, size_t table_bytes, int32_t max_oh, int32_t max_ow, int32_t w_enc
#define NET_ONE_SIZE(shared) \
  NetSrc{hm, hh, hw, hm_img_stride, tg, th, tw, tg_img_stride, N, J, oh, ow, shared, false, nullptr, 0, ow}
#define NET_SIZED(shared)                                                                                    \
  NetSrc{hm, hh, hw, hm_img_stride, tg, th, tw, tg_img_stride, N, J, max_oh, max_ow, shared, true, sizes_table, \
         table_bytes, w_enc}

extern "C" int rtpe_topk_fused(NET_MAPS_PARAMS, int32_t oh, int32_t ow, TOPK_PARAMS) {
  return decode_topk("topk_fused", NET_ONE_SIZE(false), TOPK_ARGS);
}

extern "C" int rtpe_adjust_refine_fused(NET_MAPS_PARAMS, int32_t oh, int32_t ow, const float* ans_in, float* ans_out,
                                        const int32_t* person_img, int32_t P, int32_t do_adjust,
                                        int32_t do_refine, float* scores, void* scratch, size_t scratch_bytes,
                                        void* stream) {
  // the one entry without the top-k table: null, null, 0 in its place
  return decode_adjust_refine("adjust_refine_fused", NET_ONE_SIZE(false),
                              {ans_in, ans_out, person_img, P, do_adjust, do_refine, scores, nullptr, nullptr, 0,
                               scratch, scratch_bytes, stream}, kAnyForm);
}

extern "C" int rtpe_adjust_refine_fused_topk(NET_MAPS_PARAMS, int32_t oh, int32_t ow, REFINE_PARAMS) {
  return decode_adjust_refine("adjust_refine_fused_topk", NET_ONE_SIZE(false), REFINE_TAIL, kNeedTopk);
}

// rtpe_adjust_refine_fused_topk with the number of people read on the device: P is the capacity of ans_in /
// ans_out / person_img / scores and of the scratch buffer, *P_dev (device-visible, written by an earlier
// command of the stream) the number of people.  The same for every `_n` entry below.
extern "C" int rtpe_adjust_refine_fused_topk_n(NET_MAPS_PARAMS, int32_t oh, int32_t ow, REFINE_PARAMS,
                                               const int32_t* P_dev) {
  return decode_adjust_refine("adjust_refine_fused_topk_n", NET_ONE_SIZE(false), REFINE_TAIL,
                              kNeedTopk | kCountOnDevice, P_dev);
}

// shared: the outputs of a dual-head student as they are (include/rtpe_hip_shared.h)
extern "C" int rtpe_topk_fused_shared(NET_MAPS_PARAMS, int32_t oh, int32_t ow, TOPK_PARAMS) {
  return decode_topk("topk_fused_shared", NET_ONE_SIZE(true), TOPK_ARGS);
}

extern "C" int rtpe_adjust_refine_fused_shared_topk(NET_MAPS_PARAMS, int32_t oh, int32_t ow, REFINE_PARAMS) {
  return decode_adjust_refine("adjust_refine_fused_shared_topk", NET_ONE_SIZE(true), REFINE_TAIL, kNeedTopk);
}

extern "C" int rtpe_adjust_refine_fused_shared_topk_n(NET_MAPS_PARAMS, int32_t oh, int32_t ow, REFINE_PARAMS,
                                                      const int32_t* P_dev) {
  return decode_adjust_refine("adjust_refine_fused_shared_topk_n", NET_ONE_SIZE(true), REFINE_TAIL,
                              kNeedTopk | kCountOnDevice, P_dev);
}

// sized: the size tables (HOST functions) and the entries that read them (include/rtpe_hip_sizes.h, rtpe_hip_mixdec.h)
extern "C" int rtpe_decode_sizes_bytes(int32_t N, size_t* bytes) {
  RTPE_REQUIRE(bytes && N > 0, "decode_sizes_bytes: bad argument");
  *bytes = (size_t)N * sizeof(SizeEntry);
  return RTPE_OK;
}

// Entry n: the axes of an image decoded at out_hw[n] whose maps span heat_hw[step * n] / tag_hw[step * n] of planes of
// pitch (hh, hw) / (th, tw); step = 0: the same extents for every image.  Everything is checked before the first entry
// is written: a wrong entry would make the device read outside the planes.
static int fill_size_table(const char* who, const int32_t* out_hw, const int32_t* heat_hw, const int32_t* tag_hw,
                           int step, int N, int hh, int hw, int th, int tw, void* table, int32_t* max_oh,
                           int32_t* max_ow) {
  int mh = 0, mw = 0;
  for (int n = 0; n < N; ++n) {
    const int32_t *o = out_hw + 2 * n, *he = heat_hw + step * n, *te = tag_hw + step * n;
    RTPE_REQUIRE(o[0] > 0 && o[1] > 0, "%s: image %d has size %d x %d", who, n, o[0], o[1]);
    RTPE_REQUIRE(he[0] > 0 && he[1] > 0 && te[0] > 0 && te[1] > 0,
                 "%s: image %d has map extents %d x %d (heat), %d x %d (tag)", who, n, he[0], he[1], te[0], te[1]);
    RTPE_REQUIRE(he[0] <= hh && he[1] <= hw, "%s: image %d: heat extent %d x %d is above the pitch %d x %d", who, n,
                 he[0], he[1], hh, hw);
    RTPE_REQUIRE(te[0] <= th && te[1] <= tw, "%s: image %d: tag extent %d x %d is above the pitch %d x %d", who, n,
                 te[0], te[1], th, tw);
    mh = o[0] > mh ? o[0] : mh;
    mw = o[1] > mw ? o[1] : mw;
  }
  SizeEntry* tab = reinterpret_cast<SizeEntry*>(table);
  for (int n = 0; n < N; ++n) {
    const int32_t *he = heat_hw + step * n, *te = tag_hw + step * n;
    SizeEntry e;
    memset(&e, 0, sizeof(e));
    e.oh = out_hw[2 * n];
    e.ow = out_hw[2 * n + 1];
    e.hy = make_axis(he[0], e.oh);
    e.hx = make_axis(he[1], e.ow);
    e.ty = make_axis(te[0], e.oh);
    e.tx = make_axis(te[1], e.ow);
    e.small = small_output(e.oh, e.ow);
    tab[n] = e;
  }
  if (max_oh) *max_oh = mh;
  if (max_ow) *max_ow = mw;
  return RTPE_OK;
}

// every image's maps span the whole planes: extent = pitch
extern "C" int rtpe_decode_sizes_fill(const int32_t* sizes_hw, int32_t N, int32_t hh, int32_t hw, int32_t th,
                                      int32_t tw, void* table, size_t table_bytes, int32_t* max_oh,
                                      int32_t* max_ow) {
  RTPE_REQUIRE(sizes_hw && table && N > 0, "decode_sizes_fill: bad argument");
  RTPE_REQUIRE(hh > 0 && hw > 0 && th > 0 && tw > 0, "decode_sizes_fill: bad shape");
  RTPE_REQUIRE(table_bytes >= (size_t)N * sizeof(SizeEntry), "decode_sizes_fill: sizes table too small (%zu < %zu bytes)",
               table_bytes, (size_t)N * sizeof(SizeEntry));
  // step = 0: these two pairs serve as every image's extents (their per-image checks in fill_size_table then repeat
  // the shape check above and cannot fail)
  const int32_t heat[2] = {hh, hw}, tag[2] = {th, tw};
  return fill_size_table("decode_sizes_fill", sizes_hw, heat, tag, 0, N, hh, hw, th, tw, table, max_oh, max_ow);
}

extern "C" int rtpe_decode_mixed_fill(const int32_t* out_hw, const int32_t* heat_hw, const int32_t* tag_hw, int32_t N,
                                      int32_t hh, int32_t hw, int32_t th, int32_t tw, void* table, size_t table_bytes,
                                      int32_t* max_oh, int32_t* max_ow) {
  RTPE_REQUIRE(out_hw && heat_hw && table && N > 0, "decode_mixed_fill: bad argument");
  RTPE_REQUIRE(hh > 0 && hw > 0 && th > 0 && tw > 0, "decode_mixed_fill: bad shape");
  RTPE_REQUIRE(table_bytes >= (size_t)N * sizeof(SizeEntry), "decode_mixed_fill: sizes table too small (%zu < %zu bytes)",
               table_bytes, (size_t)N * sizeof(SizeEntry));
  // (tag_hw null: the tag extents are the heat extents)
  return fill_size_table("decode_mixed_fill", out_hw, heat_hw, tag_hw ? tag_hw : heat_hw, 2, N, hh, hw, th, tw, table,
                         max_oh, max_ow);
}

extern "C" int rtpe_topk_fused_sizes(NET_MAPS_PARAMS, NET_TABLE_PARAMS, TOPK_PARAMS) {
  return decode_topk("topk_fused_sizes", NET_SIZED(false), TOPK_ARGS);
}

extern "C" int rtpe_adjust_refine_fused_topk_sizes(NET_MAPS_PARAMS, NET_TABLE_PARAMS, REFINE_PARAMS) {
  return decode_adjust_refine("adjust_refine_fused_topk_sizes", NET_SIZED(false), REFINE_TAIL, kNeedTopk);
}

extern "C" int rtpe_adjust_refine_fused_topk_sizes_n(NET_MAPS_PARAMS, NET_TABLE_PARAMS, REFINE_PARAMS,
                                                     const int32_t* P_dev) {
  return decode_adjust_refine("adjust_refine_fused_topk_sizes_n", NET_SIZED(false), REFINE_TAIL,
                              kNeedTopk | kCountOnDevice, P_dev);
}

// shared and sized: a mixed-size batch of a dual-head student decoded from its canvas (include/rtpe_hip_mixdec.h)
extern "C" int rtpe_topk_fused_mixed(NET_MAPS_PARAMS, NET_TABLE_PARAMS, TOPK_PARAMS) {
  return decode_topk("topk_fused_mixed", NET_SIZED(true), TOPK_ARGS);
}

extern "C" int rtpe_adjust_refine_fused_mixed_topk(NET_MAPS_PARAMS, NET_TABLE_PARAMS, REFINE_PARAMS) {
  return decode_adjust_refine("adjust_refine_fused_mixed_topk", NET_SIZED(true), REFINE_TAIL, kNeedTopk);
}

extern "C" int rtpe_adjust_refine_fused_mixed_topk_n(NET_MAPS_PARAMS, NET_TABLE_PARAMS, REFINE_PARAMS,
                                                     const int32_t* P_dev) {
  return decode_adjust_refine("adjust_refine_fused_mixed_topk_n", NET_SIZED(true), REFINE_TAIL,
                              kNeedTopk | kCountOnDevice, P_dev);
}

// ---------------------------------------------------------------------------
// The prepare kernels' arguments (flip test and multi-scale test): the checks of the network outputs of the images
// and, with `flip`, of their mirror images, and the FlipPrepArgs they make - all but plane0 and the output maps.
// (h2, w2): the refined size of the scale.  J <= kMaxJ is the caller's check.
// ---------------------------------------------------------------------------
static int fill_prep(const char* who, const float* preds, int h4, int w4, int64_t preds_st, const float* refined,
                     int h2, int w2, int64_t refined_st, const float* preds_f, int64_t preds_f_st,
                     const float* refined_f, int64_t refined_f_st, int J, const int32_t* flip_index, bool flip,
                     FlipPrepArgs* a) {
  RTPE_REQUIRE(preds && refined && (!flip || (preds_f && refined_f && flip_index)), "%s: null argument", who);
  RTPE_REQUIRE(h4 > 0 && w4 > 0, "%s: bad shape", who);
  RTPE_REQUIRE(preds_st >= (int64_t)2 * J * h4 * w4 && refined_st >= (int64_t)J * h2 * w2 &&
                   (!flip || (preds_f_st >= (int64_t)2 * J * h4 * w4 && refined_f_st >= (int64_t)J * h2 * w2)),
               "%s: an image stride is shorter than the image", who);
  memset(a, 0, sizeof(*a));
  unsigned seen = 0;
  for (int j = 0; flip && j < J; ++j) {
    const int q = flip_index[j];
    RTPE_REQUIRE(q >= 0 && q < J && !(seen & (1u << q)), "%s: flip_index is not a permutation of 0..%d", who, J - 1);
    seen |= 1u << q;
    a->perm[j] = q;
  }
  a->p = preds; a->r = refined; a->pf = preds_f; a->rf = refined_f;
  a->p_st = preds_st; a->r_st = refined_st; a->pf_st = preds_f_st; a->rf_st = refined_f_st;
  a->J = J; a->h4 = h4; a->w4 = w4; a->h2 = h2; a->w2 = w2;
  a->sy = (float)h4 / (float)h2;
  a->sx = (float)w4 / (float)w2;
  return RTPE_OK;
}

static dim3 prep_grid(int npix, int planes) {
  return dim3((npix + 255) / 256 < 1024 ? (npix + 255) / 256 : 1024, planes);
}

static NcAxes nc_axes(int sh, int sw, int oh, int ow) {
  NcAxes a;
  a.sh = sh; a.sw = sw; a.oh = oh; a.ow = ow;
  a.sy = (float)sh / (float)oh;
  a.sx = (float)sw / (float)ow;
  a.ident = sh == oh && sw == ow;
  return a;
}

// ---------------------------------------------------------------------------
// flip test (single scale): rtpe/inference.py multi_scale_inference(scale_factors=(1,), flip_test=True,
// project2image=True) for a whole batch, the projected maps never built.  The maps buffer: A_o, A_f, T_o, T_f of
// flip_prep_kernel, (N*J, h2, w2) each; D = 2
// ---------------------------------------------------------------------------
struct FlipSrc {
  const float* maps;
  int32_t h2, w2, N, J, oh, ow;
  size_t plane_floats() const { return (size_t)N * J * h2 * w2; }
  int check(const char* who) const {
    RTPE_REQUIRE(maps && N > 0 && J > 0 && J <= kMaxJ && h2 > 0 && w2 > 0 && oh > 0 && ow > 0 && N * J <= 65535,
                 "%s: bad argument (1 <= J <= %d, at most 65535 planes per call)", who, kMaxJ);
    return RTPE_OK;
  }
  template <class F>
  int with_maps(F f) const {
    const size_t n = plane_floats();
    const NcAxes a = nc_axes(h2, w2, oh, ow);
    return f(FlipHeatMap{maps, maps + n, a}, FlipTag{maps + 2 * n, maps + 3 * n, a}, 2);
  }
};
#define FLIP_SRC FlipSrc{maps, h2, w2, N, J, oh, ow}

extern "C" int rtpe_flip_maps_bytes(int32_t N, int32_t J, int32_t h2, int32_t w2, size_t* bytes) {
  RTPE_REQUIRE(bytes && N > 0 && J > 0 && h2 > 0 && w2 > 0, "flip_maps_bytes: bad argument");
  *bytes = (size_t)4 * N * J * h2 * w2 * sizeof(float);
  return RTPE_OK;
}

extern "C" int rtpe_topk_flip(const float* preds, int32_t h4, int32_t w4, int64_t preds_img_stride,
                              const float* refined, int32_t h2, int32_t w2, int64_t refined_img_stride,
                              const float* preds_f, int64_t preds_f_img_stride, const float* refined_f,
                              int64_t refined_f_img_stride, int32_t N, int32_t J, const int32_t* flip_index,
                              int32_t oh, int32_t ow, int32_t K, int32_t nms_ksize, int32_t nms_pad, float* val_k,
                              int32_t* ind_k, float* tag_k, float* maps, size_t maps_bytes, void* scratch,
                              size_t scratch_bytes, void* stream) {
  FlipSrc src = FLIP_SRC;
  const TopkTables tables{val_k, ind_k, tag_k};
  int rc = topk_check("topk_flip", src, K, tables, scratch);
  if (rc != RTPE_OK) return rc;
  RTPE_REQUIRE((int64_t)h2 * w2 < 0x7fffffff, "topk_flip: bad shape");
  const size_t n = src.plane_floats();
  RTPE_REQUIRE(maps_bytes >= 4 * n * sizeof(float), "topk_flip: maps buffer too small (%zu < %zu bytes)", maps_bytes,
               4 * n * sizeof(float));
  FlipPrepArgs a;
  rc = fill_prep("topk_flip", preds, h4, w4, preds_img_stride, refined, h2, w2, refined_img_stride, preds_f,
                 preds_f_img_stride, refined_f, refined_f_img_stride, J, flip_index, true, &a);
  if (rc != RTPE_OK) return rc;
  a.ao = maps; a.af = maps + n; a.to = maps + 2 * n; a.tf = maps + 3 * n;
  hipLaunchKernelGGL(flip_prep_kernel, prep_grid(h2 * w2, N * J), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     a);
  RTPE_HIP_CHECK(hipGetLastError());
  // (repeats topk_check, which passed above: nothing is refused here that was not refused before the launch)
  return decode_topk("topk_flip", src, K, nms_ksize, nms_pad, tables, scratch, scratch_bytes, stream);
}

extern "C" int rtpe_adjust_refine_flip(const float* maps, int32_t h2, int32_t w2, int32_t N, int32_t J, int32_t oh,
                                       int32_t ow, REFINE_PARAMS) {
  return decode_adjust_refine("adjust_refine_flip", FLIP_SRC, REFINE_TAIL, kAnyForm);
}

extern "C" int rtpe_adjust_refine_flip_n(const float* maps, int32_t h2, int32_t w2, int32_t N, int32_t J, int32_t oh,
                                         int32_t ow, REFINE_PARAMS, const int32_t* P_dev) {
  return decode_adjust_refine("adjust_refine_flip_n", FLIP_SRC, REFINE_TAIL, kCountOnDevice, P_dev);
}

// ---------------------------------------------------------------------------
// multi-scale test: rtpe/inference.py multi_scale_inference(scale_factors, flip_test, project2image=True) for a whole
// batch, the maps at the projection size never built.  The maps buffer, in floats: per scale i (the loop order,
// descending) A_o^i then, with flip, A_f^i, each (N*J, h2_i, w2_i); then T_o and, with flip, T_f of the scale-1 entry
// `base`, (N*J, h2_base, w2_base) each (D = 1 + flip).
// AGS (multi_scale_inference(..., ags=True)): the heat maps as above, no T_o / T_f; the tag of every joint of image n
// is ONE plane, rs_(oh,ow)(rs_(h2,w2)(P_L[n, J])) of the smallest scale L = S-1 (D = 1), stored at the refined size of
// that scale, (N, h2[S-1], w2[S-1]), at offset `to` (`tf` unused) and projected on the fly.
// Averaged tag (multi_scale_inference(..., ags="mean"), include/rtpe_hip_tagmean.h): the heat maps as above; at `to`
// the J un-mirrored tag maps of the smallest scale, (N*J, h2[S-1], w2[S-1]); at `mean` the shared tag planes M at the
// decode size, (N, oh, ow), which mean_plane_kernel writes and the decode reads through AgsTag as an identity copy.
// ---------------------------------------------------------------------------
enum { kTagPerJoint = 0, kTagFirst = 1, kTagMean = 2 };     // the `ags` of the functions below
struct MsLayout {
  size_t ao[kMaxScales], af[kMaxScales], to, tf, total;   // float offsets into the maps buffer; total floats
  size_t mean;                                            // kTagMean only: the shared tag planes M
};

static int ms_layout(int N, int J, int S, const int32_t* h2, const int32_t* w2, int base, int flip, int ags,
                     MsLayout* L, int oh = 0, int ow = 0) {
  RTPE_REQUIRE(h2 && w2, "ms: null size array");
  RTPE_REQUIRE(N > 0 && J > 0 && J <= kMaxJ, "ms: N=%d J=%d (1 <= J <= %d)", N, J, kMaxJ);
  RTPE_REQUIRE((int64_t)N * J <= 65535, "ms: at most 65535 planes per call");
  RTPE_REQUIRE(S >= 1 && S <= kMaxScales, "ms: %d scales (1 <= S <= %d)", S, kMaxScales);
  RTPE_REQUIRE(base >= 0 && base < S, "ms: the scale-1 entry %d is not one of the %d scales", base, S);
  RTPE_REQUIRE(flip == 0 || flip == 1, "ms: flip must be 0 or 1");
  size_t o = 0;
  for (int i = 0; i < S; ++i) {
    RTPE_REQUIRE(h2[i] > 0 && w2[i] > 0 && (int64_t)h2[i] * w2[i] < 0x7fffffff, "ms: bad size %d x %d of scale %d",
                 h2[i], w2[i], i);
    const size_t n = (size_t)N * J * h2[i] * w2[i];
    L->ao[i] = o;
    o += n;
    L->af[i] = o;
    if (flip) o += n;
  }
  if (ags == kTagMean) {
    RTPE_REQUIRE(oh > 0 && ow > 0 && (int64_t)oh * ow < 0x7fffffff, "ms: bad decode size %d x %d", oh, ow);
    L->to = L->tf = o;                                    // (no T_f: `tf` is never used)
    o += (size_t)N * J * h2[S - 1] * w2[S - 1];
    L->mean = o;
    L->total = o + (size_t)N * oh * ow;
    return RTPE_OK;
  }
  const size_t nb = ags ? (size_t)N * h2[S - 1] * w2[S - 1] : (size_t)N * J * h2[base] * w2[base];
  L->to = o;
  o += nb;
  L->tf = ags ? L->to : o;
  if (flip && !ags) o += nb;
  L->total = o;
  return RTPE_OK;
}

struct MsSrc {
  const float* maps;
  int32_t N, J, S;
  const int32_t *h2, *w2;
  int32_t base, flip, oh, ow;
  size_t maps_bytes;
  int ags;                  // kTagPerJoint / kTagFirst / kTagMean
  MsLayout L;               // filled by check()
  int check(const char* who) {
    const int rc = ms_layout(N, J, S, h2, w2, base, flip, ags, &L, oh, ow);
    if (rc != RTPE_OK) return rc;
    RTPE_REQUIRE(maps && oh > 0 && ow > 0, "%s: bad argument", who);
    RTPE_REQUIRE(maps_bytes >= L.total * sizeof(float), "%s: maps buffer too small (%zu < %zu bytes)", who, maps_bytes,
                 L.total * sizeof(float));
    return RTPE_OK;
  }
  template <class F>
  int with_maps(F f) const {
    MultiScaleHeatMap m;
    memset(&m, 0, sizeof(m));
    m.S = S;
    m.flip = flip != 0;
    for (int i = 0; i < S; ++i) {
      m.ao[i] = maps + L.ao[i];
      m.af[i] = flip ? maps + L.af[i] : nullptr;
      m.a[i] = nc_axes(h2[i], w2[i], oh, ow);
    }
    if (ags == kTagMean) return f(m, AgsTag{maps + L.mean, J, nc_axes(oh, ow, oh, ow)}, 1);     // (an identity copy)
    if (ags) return f(m, AgsTag{maps + L.to, J, nc_axes(h2[S - 1], w2[S - 1], oh, ow)}, 1);
    // D = 1 + flip: FlipTag's second map is never read with D = 1
    return f(m, FlipTag{maps + L.to, flip ? maps + L.tf : nullptr, nc_axes(h2[base], w2[base], oh, ow)}, 1 + flip);
  }
};
#define MS_SRC(ags) MsSrc{maps, N, J, S, h2, w2, base, flip, oh, ow, maps_bytes, ags}

static int ms_maps_bytes(const char* who, int N, int J, int S, const int32_t* h2, const int32_t* w2, int base,
                         int flip, int ags, size_t* bytes, int oh = 0, int ow = 0) {
  RTPE_REQUIRE(bytes, "%s: null argument", who);
  MsLayout L;
  const int rc = ms_layout(N, J, S, h2, w2, base, flip, ags, &L, oh, ow);
  if (rc != RTPE_OK) return rc;
  *bytes = L.total * sizeof(float);
  return RTPE_OK;
}

extern "C" int rtpe_ms_maps_bytes(int32_t N, int32_t J, int32_t S, const int32_t* h2, const int32_t* w2, int32_t base,
                                  int32_t flip, size_t* bytes) {
  return ms_maps_bytes("ms_maps_bytes", N, J, S, h2, w2, base, flip, false, bytes);
}

extern "C" int rtpe_ms_ags_maps_bytes(int32_t N, int32_t J, int32_t S, const int32_t* h2, const int32_t* w2,
                                      int32_t base, int32_t flip, size_t* bytes) {
  return ms_maps_bytes("ms_ags_maps_bytes", N, J, S, h2, w2, base, flip, true, bytes);
}

extern "C" int rtpe_ms_mean_maps_bytes(int32_t N, int32_t J, int32_t S, const int32_t* h2, const int32_t* w2,
                                       int32_t base, int32_t flip, int32_t oh, int32_t ow, size_t* bytes) {
  return ms_maps_bytes("ms_mean_maps_bytes", N, J, S, h2, w2, base, flip, kTagMean, bytes, oh, ow);
}

// rtpe_ms_prep / rtpe_ms_ags_prep / rtpe_ms_mean_prep: the same checks and arguments; `ags` picks the layout and the
// kernels ((oh, ow): the averaged-tag layout only)
static int ms_prep_impl(const float* preds, int32_t h4, int32_t w4, int64_t preds_img_stride, const float* refined,
                        int64_t refined_img_stride, const float* preds_f, int64_t preds_f_img_stride,
                        const float* refined_f, int64_t refined_f_img_stride, int32_t n0, int32_t n, int32_t N,
                        int32_t J, const int32_t* flip_index, int32_t S, const int32_t* h2, const int32_t* w2,
                        int32_t base, int32_t flip, int32_t scale, float* maps, size_t maps_bytes, void* stream,
                        int ags, int oh = 0, int ow = 0) {
  MsLayout L;
  int rc = ms_layout(N, J, S, h2, w2, base, flip, ags, &L, oh, ow);
  if (rc != RTPE_OK) return rc;
  RTPE_REQUIRE(maps, "ms_prep: null argument");
  RTPE_REQUIRE(scale >= 0 && scale < S, "ms_prep: scale %d of %d", scale, S);
  RTPE_REQUIRE(n > 0 && n0 >= 0 && (int64_t)n0 + n <= N, "ms_prep: images %d..%d of %d", n0, n0 + n - 1, N);
  RTPE_REQUIRE(maps_bytes >= L.total * sizeof(float), "ms_prep: maps buffer too small (%zu < %zu bytes)", maps_bytes,
               L.total * sizeof(float));
  FlipPrepArgs a;
  rc = fill_prep("ms_prep", preds, h4, w4, preds_img_stride, refined, h2[scale], w2[scale], refined_img_stride,
                 preds_f, preds_f_img_stride, refined_f, refined_f_img_stride, J, flip_index, flip != 0, &a);
  if (rc != RTPE_OK) return rc;
  a.plane0 = n0 * J;
  a.ao = maps + L.ao[scale];
  a.af = flip ? maps + L.af[scale] : nullptr;
  // AGS: no per-joint tag maps; the smallest scale (the last of the loop) also writes the shared tag planes
  // averaged tag: the smallest scale writes its un-mirrored per-joint tag maps, and M goes behind it
  const bool tags = !ags && scale == base, ags_tag = ags == kTagFirst && scale == S - 1;
  const bool mean_tag = ags == kTagMean && scale == S - 1;
  a.to = tags || ags_tag || mean_tag ? maps + L.to : nullptr;
  a.tf = tags && flip ? maps + L.tf : nullptr;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid = prep_grid(h2[scale] * w2[scale], n * J);
  if (mean_tag && flip) hipLaunchKernelGGL((mean_prep_kernel<true>), grid, dim3(256), 0, s, a);
  else if (mean_tag) hipLaunchKernelGGL((mean_prep_kernel<false>), grid, dim3(256), 0, s, a);
  else if (ags_tag && flip) hipLaunchKernelGGL((ags_prep_kernel<true>), grid, dim3(256), 0, s, a);
  else if (ags_tag) hipLaunchKernelGGL((ags_prep_kernel<false>), grid, dim3(256), 0, s, a);
  else if (flip && tags) hipLaunchKernelGGL((ms_prep_kernel<true, true>), grid, dim3(256), 0, s, a);
  else if (flip) hipLaunchKernelGGL((ms_prep_kernel<true, false>), grid, dim3(256), 0, s, a);
  else if (tags) hipLaunchKernelGGL((ms_prep_kernel<false, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((ms_prep_kernel<false, false>), grid, dim3(256), 0, s, a);
  RTPE_HIP_CHECK(hipGetLastError());
  if (mean_tag) return launch_mean_plane(maps + L.to, J, h2[scale], w2[scale], maps + L.mean, n0, n, oh, ow, s);
  return RTPE_OK;
}

extern "C" int rtpe_ms_prep(const float* preds, int32_t h4, int32_t w4, int64_t preds_img_stride, const float* refined,
                            int64_t refined_img_stride, const float* preds_f, int64_t preds_f_img_stride,
                            const float* refined_f, int64_t refined_f_img_stride, int32_t n0, int32_t n, int32_t N,
                            int32_t J, const int32_t* flip_index, int32_t S, const int32_t* h2, const int32_t* w2,
                            int32_t base, int32_t flip, int32_t scale, float* maps, size_t maps_bytes, void* stream) {
  return ms_prep_impl(preds, h4, w4, preds_img_stride, refined, refined_img_stride, preds_f, preds_f_img_stride,
                      refined_f, refined_f_img_stride, n0, n, N, J, flip_index, S, h2, w2, base, flip, scale, maps,
                      maps_bytes, stream, false);
}

extern "C" int rtpe_ms_ags_prep(const float* preds, int32_t h4, int32_t w4, int64_t preds_img_stride,
                                const float* refined, int64_t refined_img_stride, const float* preds_f,
                                int64_t preds_f_img_stride, const float* refined_f, int64_t refined_f_img_stride,
                                int32_t n0, int32_t n, int32_t N, int32_t J, const int32_t* flip_index, int32_t S,
                                const int32_t* h2, const int32_t* w2, int32_t base, int32_t flip, int32_t scale,
                                float* maps, size_t maps_bytes, void* stream) {
  return ms_prep_impl(preds, h4, w4, preds_img_stride, refined, refined_img_stride, preds_f, preds_f_img_stride,
                      refined_f, refined_f_img_stride, n0, n, N, J, flip_index, S, h2, w2, base, flip, scale, maps,
                      maps_bytes, stream, true);
}

extern "C" int rtpe_topk_ms(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2, const int32_t* w2,
                            int32_t base, int32_t flip, int32_t oh, int32_t ow, int32_t K, int32_t nms_ksize,
                            int32_t nms_pad, float* val_k, int32_t* ind_k, float* tag_k, size_t maps_bytes,
                            void* scratch, size_t scratch_bytes, void* stream) {
  return decode_topk("topk_ms", MS_SRC(kTagPerJoint), TOPK_ARGS);
}

extern "C" int rtpe_topk_ms_ags(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                                const int32_t* w2, int32_t base, int32_t flip, int32_t oh, int32_t ow, int32_t K,
                                int32_t nms_ksize, int32_t nms_pad, float* val_k, int32_t* ind_k, float* tag_k,
                                size_t maps_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  return decode_topk("topk_ms_ags", MS_SRC(kTagFirst), TOPK_ARGS);
}

extern "C" int rtpe_adjust_refine_ms(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                                     const int32_t* w2, int32_t base, int32_t flip, int32_t oh, int32_t ow,
                                     size_t maps_bytes, REFINE_PARAMS) {
  return decode_adjust_refine("adjust_refine_ms", MS_SRC(kTagPerJoint), REFINE_TAIL, kAnyForm);
}

extern "C" int rtpe_adjust_refine_ms_n(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                                       const int32_t* w2, int32_t base, int32_t flip, int32_t oh, int32_t ow,
                                       size_t maps_bytes, REFINE_PARAMS, const int32_t* P_dev) {
  return decode_adjust_refine("adjust_refine_ms_n", MS_SRC(kTagPerJoint), REFINE_TAIL, kCountOnDevice, P_dev);
}

extern "C" int rtpe_adjust_refine_ms_ags(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                                         const int32_t* w2, int32_t base, int32_t flip, int32_t oh, int32_t ow,
                                         size_t maps_bytes, REFINE_PARAMS) {
  return decode_adjust_refine("adjust_refine_ms_ags", MS_SRC(kTagFirst), REFINE_TAIL, kAnyForm);
}

extern "C" int rtpe_adjust_refine_ms_ags_n(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                                           const int32_t* w2, int32_t base, int32_t flip, int32_t oh, int32_t ow,
                                           size_t maps_bytes, REFINE_PARAMS, const int32_t* P_dev) {
  return decode_adjust_refine("adjust_refine_ms_ags_n", MS_SRC(kTagFirst), REFINE_TAIL, kCountOnDevice, P_dev);
}

// averaged tag (include/rtpe_hip_tagmean.h): the `_ags` entries with the layout that holds T and M
extern "C" int rtpe_ms_mean_prep(const float* preds, int32_t h4, int32_t w4, int64_t preds_img_stride,
                                 const float* refined, int64_t refined_img_stride, const float* preds_f,
                                 int64_t preds_f_img_stride, const float* refined_f, int64_t refined_f_img_stride,
                                 int32_t n0, int32_t n, int32_t N, int32_t J, const int32_t* flip_index, int32_t S,
                                 const int32_t* h2, const int32_t* w2, int32_t base, int32_t flip, int32_t scale,
                                 int32_t oh, int32_t ow, float* maps, size_t maps_bytes, void* stream) {
  return ms_prep_impl(preds, h4, w4, preds_img_stride, refined, refined_img_stride, preds_f, preds_f_img_stride,
                      refined_f, refined_f_img_stride, n0, n, N, J, flip_index, S, h2, w2, base, flip, scale, maps,
                      maps_bytes, stream, kTagMean, oh, ow);
}

extern "C" int rtpe_topk_ms_mean(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                                 const int32_t* w2, int32_t base, int32_t flip, int32_t oh, int32_t ow, int32_t K,
                                 int32_t nms_ksize, int32_t nms_pad, float* val_k, int32_t* ind_k, float* tag_k,
                                 size_t maps_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  return decode_topk("topk_ms_mean", MS_SRC(kTagMean), TOPK_ARGS);
}

extern "C" int rtpe_adjust_refine_ms_mean(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                                          const int32_t* w2, int32_t base, int32_t flip, int32_t oh, int32_t ow,
                                          size_t maps_bytes, REFINE_PARAMS) {
  return decode_adjust_refine("adjust_refine_ms_mean", MS_SRC(kTagMean), REFINE_TAIL, kAnyForm);
}

extern "C" int rtpe_adjust_refine_ms_mean_n(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                                            const int32_t* w2, int32_t base, int32_t flip, int32_t oh, int32_t ow,
                                            size_t maps_bytes, REFINE_PARAMS, const int32_t* P_dev) {
  return decode_adjust_refine("adjust_refine_ms_mean_n", MS_SRC(kTagMean), REFINE_TAIL, kCountOnDevice, P_dev);
}

// ---------------------------------------------------------------------------
// multi-scale (and flip) test WITHOUT projection to the image (include/rtpe_hip_noproj.h): rtpe/inference.py
// multi_scale_inference(scale_factors, flip_test, project2image=False) for a whole batch.  The decode grid is r_0 =
// (h2[0], w2[0]), the refined size of the largest scale.  The maps buffer, in floats:
//     F                  (N*J, h2_0, w2_0)        the heat map, summed in place while the scales arrive
//     T_o [, T_f]        (N*J, h2_b, w2_b) each   the tag maps of the scale-1 entry b = base at ITS refined size
//     H_i, i = 1..S-1    (N*J, h2_i, w2_i)        the flip-averaged heat map of a later scale, read by its accumulate
// rtpe_ms_np_prep of scale 0 writes H_0 straight into F; of a later scale, H_i and behind it F += rs(H_i) [/ S on the
// last].  The decode reads F at integer pixels (DirectMap); the tags through FlipTag: a copy when scale 1 is first,
// else the four taps of rs_(r_b -> r_0) on the fly (the arithmetic of aggregate_results' resize; the top-k gathers K
// tags per plane and refine reads tags for missing joints only, so a resized copy would move more bytes).
// ---------------------------------------------------------------------------
struct NpLayout {
  size_t f, to, tf, h[kMaxScales], total;     // float offsets; h[0] = f
};

static int np_layout(int N, int J, int S, const int32_t* h2, const int32_t* w2, int base, int flip, NpLayout* L) {
  MsLayout M;                                 // (its checks: sizes, S <= kMaxScales, base one of the scales, J, planes)
  const int rc = ms_layout(N, J, S, h2, w2, base, flip, kTagPerJoint, &M);
  if (rc != RTPE_OK) return rc;
  const size_t P = (size_t)N * J;
  size_t o = P * h2[0] * w2[0];
  L->f = L->h[0] = 0;
  L->to = o;
  o += P * h2[base] * w2[base];
  L->tf = o;
  if (flip) o += P * h2[base] * w2[base];
  for (int i = 1; i < S; ++i) {
    L->h[i] = o;
    o += P * h2[i] * w2[i];
  }
  L->total = o;
  return RTPE_OK;
}

struct NpSrc {
  const float* maps;
  int32_t N, J, S;
  const int32_t *h2, *w2;
  int32_t base, flip;
  size_t maps_bytes;
  int32_t oh, ow;           // filled by check(): the decode grid r_0
  NpLayout L;               // likewise
  int check(const char* who) {
    const int rc = np_layout(N, J, S, h2, w2, base, flip, &L);
    if (rc != RTPE_OK) return rc;
    oh = h2[0];
    ow = w2[0];
    RTPE_REQUIRE(maps, "%s: bad argument", who);
    RTPE_REQUIRE(maps_bytes >= L.total * sizeof(float), "%s: maps buffer too small (%zu < %zu bytes)", who, maps_bytes,
                 L.total * sizeof(float));
    return RTPE_OK;
  }
  template <class F>
  int with_maps(F f) const {
    return f(DirectMap{maps + L.f, oh, ow},
             FlipTag{maps + L.to, flip ? maps + L.tf : nullptr, nc_axes(h2[base], w2[base], oh, ow)}, 1 + flip);
  }
};
#define NP_SRC NpSrc{maps, N, J, S, h2, w2, base, flip, maps_bytes}

extern "C" int rtpe_ms_np_maps_bytes(int32_t N, int32_t J, int32_t S, const int32_t* h2, const int32_t* w2,
                                     int32_t base, int32_t flip, size_t* bytes) {
  RTPE_REQUIRE(bytes, "ms_np_maps_bytes: null argument");
  NpLayout L;
  const int rc = np_layout(N, J, S, h2, w2, base, flip, &L);
  if (rc != RTPE_OK) return rc;
  *bytes = L.total * sizeof(float);
  return RTPE_OK;
}

extern "C" int rtpe_ms_np_prep(const float* preds, int32_t h4, int32_t w4, int64_t preds_img_stride,
                               const float* refined, int64_t refined_img_stride, const float* preds_f,
                               int64_t preds_f_img_stride, const float* refined_f, int64_t refined_f_img_stride,
                               int32_t n0, int32_t n, int32_t N, int32_t J, const int32_t* flip_index, int32_t S,
                               const int32_t* h2, const int32_t* w2, int32_t base, int32_t flip, int32_t scale,
                               float* maps, size_t maps_bytes, void* stream) {
  NpLayout L;
  int rc = np_layout(N, J, S, h2, w2, base, flip, &L);
  if (rc != RTPE_OK) return rc;
  RTPE_REQUIRE(maps, "ms_np_prep: null argument");
  RTPE_REQUIRE(scale >= 0 && scale < S, "ms_np_prep: scale %d of %d", scale, S);
  RTPE_REQUIRE(n > 0 && n0 >= 0 && (int64_t)n0 + n <= N, "ms_np_prep: images %d..%d of %d", n0, n0 + n - 1, N);
  RTPE_REQUIRE(maps_bytes >= L.total * sizeof(float), "ms_np_prep: maps buffer too small (%zu < %zu bytes)",
               maps_bytes, L.total * sizeof(float));
  FlipPrepArgs a;
  rc = fill_prep("ms_np_prep", preds, h4, w4, preds_img_stride, refined, h2[scale], w2[scale], refined_img_stride,
                 preds_f, preds_f_img_stride, refined_f, refined_f_img_stride, J, flip_index, flip != 0, &a);
  if (rc != RTPE_OK) return rc;
  a.plane0 = n0 * J;
  a.ao = maps + L.h[scale];                   // scale 0: F itself
  const bool tags = scale == base;
  a.to = tags ? maps + L.to : nullptr;
  a.tf = tags && flip ? maps + L.tf : nullptr;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid = prep_grid(h2[scale] * w2[scale], n * J);
  if (flip && tags) hipLaunchKernelGGL((np_prep_kernel<true>), grid, dim3(256), 0, s, a);
  else if (flip) hipLaunchKernelGGL((np_prep_kernel<false>), grid, dim3(256), 0, s, a);
  else if (tags) hipLaunchKernelGGL((ms_prep_kernel<false, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((ms_prep_kernel<false, false>), grid, dim3(256), 0, s, a);
  RTPE_HIP_CHECK(hipGetLastError());
  if (scale == 0) return RTPE_OK;
  NpAccumArgs b;
  b.h = maps + L.h[scale];
  b.f = maps + L.f;
  b.a = nc_axes(h2[scale], w2[scale], h2[0], w2[0]);
  b.plane0 = n0 * J;
  b.div = scale == S - 1 ? (float)S : 1.f;
  const long long npix = (long long)h2[0] * w2[0];
  if (w2[0] % 4 == 0 && (reinterpret_cast<uintptr_t>(maps) & 15) == 0) {
    const long long blocks = (npix / 4 + 255) / 256;
    hipLaunchKernelGGL((np_accum_kernel<4>), dim3((unsigned)(blocks < 1024 ? blocks : 1024), n * J), dim3(256), 0, s, b);
  } else {
    const long long blocks = (npix + 255) / 256;
    hipLaunchKernelGGL((np_accum_kernel<1>), dim3((unsigned)(blocks < 1024 ? blocks : 1024), n * J), dim3(256), 0, s, b);
  }
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

extern "C" int rtpe_topk_ms_np(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                               const int32_t* w2, int32_t base, int32_t flip, int32_t K, int32_t nms_ksize,
                               int32_t nms_pad, float* val_k, int32_t* ind_k, float* tag_k, size_t maps_bytes,
                               void* scratch, size_t scratch_bytes, void* stream) {
  return decode_topk("topk_ms_np", NP_SRC, TOPK_ARGS);
}

extern "C" int rtpe_adjust_refine_ms_np(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                                        const int32_t* w2, int32_t base, int32_t flip,
                                        size_t maps_bytes, REFINE_PARAMS) {
  return decode_adjust_refine("adjust_refine_ms_np", NP_SRC, REFINE_TAIL, kAnyForm);
}

extern "C" int rtpe_adjust_refine_ms_np_n(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                                          const int32_t* w2, int32_t base, int32_t flip,
                                          size_t maps_bytes, REFINE_PARAMS, const int32_t* P_dev) {
  return decode_adjust_refine("adjust_refine_ms_np_n", NP_SRC, REFINE_TAIL, kCountOnDevice, P_dev);
}
