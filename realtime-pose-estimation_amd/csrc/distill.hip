// Distillation targets and the forward values of the distillation losses (include/rtpe_hip_distill.h; the rules:
// DESIGN.md section 4, "Distillation targets and losses").  Four families of kernels:
//   * gt_heatmaps_kernel: one output pixel per thread, the windows of the image's people for the workgroup's joint staged
//     in LDS in chunks of RTPE_DISTILL_CHUNK, the pixel's value the maximum over the windows that cover it;
//   * targets_kernel: the same stamp maximum evaluated at the (up to) four align_corners=False taps of an output pixel,
//     and the teacher's align_corners=True sample evaluated at those taps, so neither map exists at image resolution;
//   * elem_kernel: normalisation, background weighting, masking (float32) and the loss elements (float64), one partial
//     sum per workgroup; loss_final_kernel adds the partials in index order;
//   * minmax kernels: per-workgroup partials and a last pass (min and max are exact, so order does not matter).
// The file is compiled without contraction: every fused multiply-add below is explicit.
#include "rtpe_common.h"
#include "rtpe_hip_distill.h"
#include "resize_nc.h"          // axis_nc: the align_corners=False axis of PyTorch-CPU

#include <math.h>

namespace rtpe {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSmallOut = 128;          // out_h + out_w up to which PyTorch-CPU resizes with its small-output kernel

struct Win { int ulx, uly, brx, bry; };         // window [ulx, brx) x [uly, bry) with br clipped to the image; empty: brx == ulx

// the window of one joint (x, y, v): int() truncation, skipped outside the image, corners rounded half to even in float64
__device__ __forceinline__ Win joint_window(const double* jt, int H, int W, double s3) {
  Win q = {0, 0, 0, 0};
  const double px = jt[0], py = jt[1], v = jt[2];
  if (!(v > 0.0)) return q;
  if (!(px > -1.0 && px < (double)W && py > -1.0 && py < (double)H)) return q;     // trunc(p) in [0, n)
  const double x = (double)(int)px, y = (double)(int)py;
  q.ulx = (int)rint(x - s3 - 1.0);
  q.uly = (int)rint(y - s3 - 1.0);
  const int bx = (int)rint(x + s3 + 2.0), by = (int)rint(y + s3 + 2.0);
  q.brx = bx < W ? bx : W;
  q.bry = by < H ? by : H;
  if (q.brx <= q.ulx || q.bry <= q.uly) q.brx = q.ulx;
  return q;
}

// stage the windows of people [p0, p0 + cnt) of joint j; all threads of the workgroup call it
__device__ __forceinline__ void stage_windows(Win* s, const double* joints, int p0, int cnt, int J, int j, int H, int W,
                                              double s3) {
  __syncthreads();                        // the previous chunk has been read by everyone
  if ((int)threadIdx.x < cnt) s[threadIdx.x] = joint_window(joints + ((size_t)(p0 + threadIdx.x) * J + j) * 3, H, W, s3);
  __syncthreads();
}

__device__ __forceinline__ float stamp_max(const Win* s, int cnt, const float* patch, int S, int Y, int X, float v) {
  for (int k = 0; k < cnt; ++k) {
    const Win q = s[k];
    if (X >= q.ulx && X < q.brx && Y >= q.uly && Y < q.bry) {
      const int cx = X - q.ulx, cy = Y - q.uly;
      if (cx < S && cy < S) v = fmaxf(v, patch[(size_t)cy * S + cx]);       // (rint(a + k) - rint(a) <= ceil(k): always)
    }
  }
  return v;
}

// the people rows of image n, clipped to the table
__device__ __forceinline__ void people_range(const int32_t* offsets, int n, int P_total, int* o0, int* o1) {
  int a = offsets[n], b = offsets[n + 1];
  a = a < 0 ? 0 : a;
  b = b > P_total ? P_total : b;
  *o0 = a;
  *o1 = b > a ? b : a;
}

struct GtArgs {
  const int32_t* offsets;
  const double* joints;
  const float* patch;
  float* out;
  double s3;
  int P_total, J, H, W, S, bpp;
};

__global__ __launch_bounds__(kThreads) void gt_heatmaps_kernel(GtArgs a) {
  __shared__ Win s_win[RTPE_DISTILL_CHUNK];
  const int plane = blockIdx.x / a.bpp, tile = blockIdx.x - plane * a.bpp;
  const int n = plane / a.J, j = plane - n * a.J;
  const int pix = tile * kThreads + threadIdx.x, hw = a.H * a.W;
  const int Y = pix / a.W, X = pix - Y * a.W;
  int o0, o1;
  people_range(a.offsets, n, a.P_total, &o0, &o1);
  float v = 0.f;
  for (int p0 = o0; p0 < o1; p0 += RTPE_DISTILL_CHUNK) {
    const int cnt = o1 - p0 < RTPE_DISTILL_CHUNK ? o1 - p0 : RTPE_DISTILL_CHUNK;
    stage_windows(s_win, a.joints, p0, cnt, a.J, j, a.H, a.W, a.s3);
    if (pix < hw) v = stamp_max(s_win, cnt, a.patch, a.S, Y, X, v);
  }
  if (pix < hw) a.out[(size_t)plane * hw + pix] = v;
}

// ---- resizes -------------------------------------------------------------------------------------------------------
// one axis of F.interpolate(bilinear, align_corners=True): the arithmetic of decode.hip's Axis
__device__ __forceinline__ void axis_ac(float scale, int n_in, int n_out, int o, int* i0, int* i1, float* l0, float* l1) {
  if (n_in == n_out) { *i0 = *i1 = o; *l0 = 1.f; *l1 = 0.f; return; }
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

// four taps to one value: PyTorch-CPU's generic kernel, or its small-output kernel (decode.hip, bilinear_small), whose
// order differs for the channels behind the last full vector of 16
__device__ __forceinline__ float combine(float v00, float v01, float v10, float v11, float ly0, float ly1, float lx0,
                                         float lx1, bool small, bool tail) {
  if (small) {
    const float w00 = ly0 * lx0, w01 = ly0 * lx1, w10 = ly1 * lx0, w11 = ly1 * lx1;
    if (tail) return __builtin_fmaf(w11, v11, __builtin_fmaf(w10, v10, __builtin_fmaf(w00, v00, w01 * v01)));
    return __builtin_fmaf(w00, v00, __builtin_fmaf(w01, v01, __builtin_fmaf(w11, v11, w10 * v10)));
  }
  const float t0 = __builtin_fmaf(v00, lx0, v01 * lx1);
  const float t1 = __builtin_fmaf(v10, lx0, v11 * lx1);
  return __builtin_fmaf(t0, ly0, t1 * ly1);
}

struct Resize {             // (n_in_y, n_in_x) -> (n_out_y, n_out_x)
  float sy, sx;
  int ih, iw, oh, ow, ident, small;
};

static Resize make_resize(int ih, int iw, int oh, int ow, bool align_corners) {
  Resize r;
  r.ih = ih; r.iw = iw; r.oh = oh; r.ow = ow;
  r.ident = ih == oh && iw == ow;
  r.small = oh + ow <= kSmallOut;
  if (align_corners) {
    r.sy = oh > 1 ? (float)(ih - 1) / (float)(oh - 1) : 0.f;
    r.sx = ow > 1 ? (float)(iw - 1) / (float)(ow - 1) : 0.f;
  } else {
    r.sy = (float)ih / (float)oh;
    r.sx = (float)iw / (float)ow;
  }
  return r;
}

// the align_corners=True sample at (Y, X) of the output grid of `r` from a source plane
__device__ __forceinline__ float sample_ac(const float* b, const Resize& r, int Y, int X, bool tail) {
  if (r.ident) return b[(size_t)Y * r.iw + X];
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  axis_ac(r.sy, r.ih, r.oh, Y, &y0, &y1, &ly0, &ly1);
  axis_ac(r.sx, r.iw, r.ow, X, &x0, &x1, &lx0, &lx1);
  return combine(b[(size_t)y0 * r.iw + x0], b[(size_t)y0 * r.iw + x1], b[(size_t)y1 * r.iw + x0],
                 b[(size_t)y1 * r.iw + x1], ly0, ly1, lx0, lx1, r.small, tail);
}

// ---- reductions ----------------------------------------------------------------------------------------------------
struct MinMax { float gmin, gmax, tmin, tmax; };

__device__ __forceinline__ MinMax minmax_neutral() { return {INFINITY, -INFINITY, INFINITY, -INFINITY}; }

__device__ __forceinline__ MinMax minmax_join(MinMax a, MinMax b) {
  return {fminf(a.gmin, b.gmin), fmaxf(a.gmax, b.gmax), fminf(a.tmin, b.tmin), fmaxf(a.tmax, b.tmax)};
}

// all threads call it; thread 0 holds the workgroup's result
__device__ __forceinline__ MinMax minmax_block(MinMax v, MinMax* s) {
  for (int d = 32; d > 0; d >>= 1) {
    MinMax o;
    o.gmin = __shfl_down(v.gmin, d, 64); o.gmax = __shfl_down(v.gmax, d, 64);
    o.tmin = __shfl_down(v.tmin, d, 64); o.tmax = __shfl_down(v.tmax, d, 64);
    v = minmax_join(v, o);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) s[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < kWaves; ++k) v = minmax_join(v, s[k]);
  return v;
}

// one workgroup: the partial records -> the four values; an absent tensor reads (0, 0)
__global__ __launch_bounds__(kThreads) void minmax_final_kernel(const MinMax* part, int n_part, int has_gt,
                                                                int has_teacher, float* out) {
  __shared__ MinMax s[kWaves];
  MinMax v = minmax_neutral();
  for (int i = threadIdx.x; i < n_part; i += kThreads) v = minmax_join(v, part[i]);
  v = minmax_block(v, s);
  if (threadIdx.x == 0) {
    out[0] = has_gt ? v.gmin : 0.f; out[1] = has_gt ? v.gmax : 0.f;
    out[2] = has_teacher ? v.tmin : 0.f; out[3] = has_teacher ? v.tmax : 0.f;
  }
}

// ---- targets -------------------------------------------------------------------------------------------------------
struct TargetArgs {
  const int32_t* offsets;
  const double* joints;
  const float* patch;
  const float* teacher;
  float* gt_out;
  float* teacher_out;
  MinMax* part;
  double s3;
  Resize r1, r2;            // teacher source -> image (align_corners=True), image -> output (align_corners=False)
  int P_total, J, H, W, S, bpp;
};

__global__ __launch_bounds__(kThreads) void targets_kernel(TargetArgs a) {
  __shared__ Win s_win[RTPE_DISTILL_CHUNK];
  __shared__ MinMax s_mm[kWaves];
  const int plane = blockIdx.x / a.bpp, tile = blockIdx.x - plane * a.bpp;
  const int n = plane / a.J, j = plane - n * a.J;
  const int hw = a.r2.oh * a.r2.ow;
  const int pix = tile * kThreads + threadIdx.x;
  const bool live = pix < hw;
  const int oy = live ? pix / a.r2.ow : 0, ox = live ? pix - oy * a.r2.ow : 0;
  const bool tail = j >= a.J - (a.J & 15);
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  axis_nc(a.r2.sy, a.H, a.r2.oh, oy, &y0, &y1, &ly0, &ly1);
  axis_nc(a.r2.sx, a.W, a.r2.ow, ox, &x0, &x1, &lx0, &lx1);
  MinMax mm = minmax_neutral();
  if (a.gt_out) {
    int o0, o1;
    people_range(a.offsets, n, a.P_total, &o0, &o1);
    float v00 = 0.f, v01 = 0.f, v10 = 0.f, v11 = 0.f;
    for (int p0 = o0; p0 < o1; p0 += RTPE_DISTILL_CHUNK) {
      const int cnt = o1 - p0 < RTPE_DISTILL_CHUNK ? o1 - p0 : RTPE_DISTILL_CHUNK;
      stage_windows(s_win, a.joints, p0, cnt, a.J, j, a.H, a.W, a.s3);
      if (live) {
        v00 = stamp_max(s_win, cnt, a.patch, a.S, y0, x0, v00);
        if (!a.r2.ident) {
          v01 = stamp_max(s_win, cnt, a.patch, a.S, y0, x1, v01);
          v10 = stamp_max(s_win, cnt, a.patch, a.S, y1, x0, v10);
          v11 = stamp_max(s_win, cnt, a.patch, a.S, y1, x1, v11);
        }
      }
    }
    if (live) {
      const float g = a.r2.ident ? v00 : combine(v00, v01, v10, v11, ly0, ly1, lx0, lx1, a.r2.small, tail);
      a.gt_out[(size_t)plane * hw + pix] = g;
      mm.gmin = mm.gmax = g;
    }
  }
  if (a.teacher_out && live) {
    const float* b = a.teacher + (size_t)plane * a.r1.ih * a.r1.iw;
    float t;
    if (a.r2.ident) {
      t = sample_ac(b, a.r1, y0, x0, tail);
    } else {
      t = combine(sample_ac(b, a.r1, y0, x0, tail), sample_ac(b, a.r1, y0, x1, tail), sample_ac(b, a.r1, y1, x0, tail),
                  sample_ac(b, a.r1, y1, x1, tail), ly0, ly1, lx0, lx1, a.r2.small, tail);
    }
    a.teacher_out[(size_t)plane * hw + pix] = t;
    mm.tmin = mm.tmax = t;
  }
  mm = minmax_block(mm, s_mm);
  if (threadIdx.x == 0) a.part[blockIdx.x] = mm;
}

// (N, H, W) planes -> (N, 1, oh, ow), align_corners=False; one channel per resize call: the tail order when small
__global__ __launch_bounds__(kThreads) void plane_resize_kernel(const float* src, float* dst, Resize r, int bpp) {
  const int n = blockIdx.x / bpp, tile = blockIdx.x - n * bpp;
  const int hw = r.oh * r.ow, pix = tile * kThreads + threadIdx.x;
  if (pix >= hw) return;
  const int oy = pix / r.ow, ox = pix - oy * r.ow;
  const float* b = src + (size_t)n * r.ih * r.iw;
  float v;
  if (r.ident) {
    v = b[pix];
  } else {
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    axis_nc(r.sy, r.ih, r.oh, oy, &y0, &y1, &ly0, &ly1);
    axis_nc(r.sx, r.iw, r.ow, ox, &x0, &x1, &lx0, &lx1);
    v = combine(b[(size_t)y0 * r.iw + x0], b[(size_t)y0 * r.iw + x1], b[(size_t)y1 * r.iw + x0],
                b[(size_t)y1 * r.iw + x1], ly0, ly1, lx0, lx1, r.small, true);
  }
  dst[(size_t)n * hw + pix] = v;
}

// ---- normalise and loss --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void minmax_partial_kernel(const float* gt, const float* teacher, size_t n,
                                                                  MinMax* part) {
  __shared__ MinMax s[kWaves];
  MinMax v = minmax_neutral();
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
    const float g = gt[i];
    v.gmin = fminf(v.gmin, g); v.gmax = fmaxf(v.gmax, g);
    if (teacher) {
      const float t = teacher[i];
      v.tmin = fminf(v.tmin, t); v.tmax = fmaxf(v.tmax, t);
    }
  }
  v = minmax_block(v, s);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

struct ElemArgs {
  const float* pred;
  const float* teacher;
  const float* gt;
  const float* mask;
  const float* minmax;      // null: no normalisation
  float* gt_out;
  float* teacher_out;
  float* mask_out;
  double* part;             // (gridDim.x, 2): teacher and gt sums of the workgroup
  size_t n;
  long long chw, hw;        // J * h * w, h * w
  int J, pred_channels, mask_channels, kind;
  float bf, pw_t, pw_g;
};

// softplus(x) = log(1 + exp(x)) without cancellation for x << 0
__device__ __forceinline__ double softplus(double x) { return (x > 0.0 ? x : 0.0) + log1p(exp(-fabs(x))); }

// BCE-with-logits with pos_weight: (1 - y) softplus(x) + pw y softplus(-x); every term >= 0 for y in [0, 1]
__device__ __forceinline__ double bce(double x, double y, double pw) {
  return (1.0 - y) * softplus(x) + pw * y * softplus(-x);
}

__global__ __launch_bounds__(kThreads) void elem_kernel(ElemArgs a) {
  __shared__ double s_sum[kWaves][2];
  float gmin = 0.f, gdiv = 1.f, tmin = 0.f, tdiv = 1.f;
  if (a.minmax) {           // x - min if min < 0, then / max if max > 1: the maximum after the shift is max - min
    const float g0 = a.minmax[0], g1 = a.minmax[1], t0 = a.minmax[2], t1 = a.minmax[3];
    gmin = g0 < 0.f ? g0 : 0.f;
    gdiv = g0 < 0.f ? g1 - g0 : g1;
    tmin = t0 < 0.f ? t0 : 0.f;
    tdiv = t0 < 0.f ? t1 - t0 : t1;
  }
  double st = 0.0, sg = 0.0;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (size_t)gridDim.x * kThreads) {
    const long long img = (long long)(i / (size_t)a.chw), rem = (long long)(i - (size_t)img * a.chw);
    const long long j = rem / a.hw, pix = rem - j * a.hw;
    float g = a.gt[i], t = a.teacher ? a.teacher[i] : 0.f;
    if (a.minmax) {
      if (gmin < 0.f) g = g - gmin;
      if (gdiv > 1.f) g = g / gdiv;
      if (tmin < 0.f) t = t - tmin;
      if (tdiv > 1.f) t = t / tdiv;
    }
    float m = 1.f;
    if (a.mask) {
      m = a.mask[a.mask_channels == 1 ? (size_t)(img * a.hw + pix) : i];
      if (g == 0.f) m = m * a.bf;
    }
    if (a.gt_out) a.gt_out[i] = g;
    if (a.teacher_out) a.teacher_out[i] = t;
    if (a.mask_out) a.mask_out[i] = m;
    if (a.pred) {
      float p = a.pred[(size_t)((img * a.pred_channels + j) * a.hw + pix)];
      if (a.mask) { p = p * m; g = g * m; t = t * m; }
      const double x = (double)p;
      if (a.kind == RTPE_DISTILL_BCE) {
        sg += bce(x, (double)g, (double)a.pw_g);
        if (a.teacher) st += bce(x, (double)t, (double)a.pw_t);
      } else {
        const double dg = x - (double)g;
        sg += dg * dg;
        if (a.teacher) { const double dt = x - (double)t; st += dt * dt; }
      }
    }
  }
  if (!a.pred) return;
  for (int d = 32; d > 0; d >>= 1) {
    st += __shfl_down(st, d, 64);
    sg += __shfl_down(sg, d, 64);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { s_sum[wave][0] = st; s_sum[wave][1] = sg; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kWaves; ++k) { st += s_sum[k][0]; sg += s_sum[k][1]; }
    a.part[2 * blockIdx.x] = st;
    a.part[2 * blockIdx.x + 1] = sg;
  }
}

// one workgroup: the partials into LDS, added in index order; means, the mix, both precisions
__global__ __launch_bounds__(kThreads) void loss_final_kernel(const double* part, int n_part, double n_elems, double alpha,
                                                              unsigned char* out) {
  __shared__ double s[2 * RTPE_DISTILL_MAX_BLOCKS];
  for (int i = threadIdx.x; i < 2 * n_part; i += kThreads) s[i] = part[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double st = 0.0, sg = 0.0;
  for (int k = 0; k < n_part; ++k) { st += s[2 * k]; sg += s[2 * k + 1]; }
  const double lt = st / n_elems, lg = sg / n_elems;
  const double mixed = alpha * lt + (1.0 - alpha) * lg;
  double* o64 = reinterpret_cast<double*>(out);
  float* o32 = reinterpret_cast<float*>(out + 24);
  o64[0] = lt; o64[1] = lg; o64[2] = mixed;
  o32[0] = (float)lt; o32[1] = (float)lg; o32[2] = (float)mixed; o32[3] = 0.f;
}

constexpr size_t kScratchMinMax = 0;            // 4 floats
constexpr size_t kScratchMmPart = 64;           // RTPE_DISTILL_MAX_BLOCKS records of 16 bytes
constexpr size_t kScratchSums = kScratchMmPart + 16 * RTPE_DISTILL_MAX_BLOCKS;     // ... pairs of doubles
static_assert(kScratchSums + 16 * RTPE_DISTILL_MAX_BLOCKS <= RTPE_DISTILL_SCRATCH_BYTES, "scratch layout");
static_assert(sizeof(MinMax) == 16 && sizeof(Win) == 16, "record sizes");

int blocks_per_plane(int h, int w) { return (int)(((long long)h * w + kThreads - 1) / kThreads); }

int reduction_blocks(size_t n) {
  const size_t b = (n + kThreads - 1) / kThreads;
  return (int)(b < RTPE_DISTILL_MAX_BLOCKS ? b : RTPE_DISTILL_MAX_BLOCKS);
}

int check_patch(const char* who, int S, double sigma) {
  RTPE_REQUIRE(sigma > 0.0 && sigma <= 1e6, "%s: sigma = %g must be positive", who, sigma);
  RTPE_REQUIRE(S > 0 && S <= RTPE_DISTILL_MAX_PATCH && S == (int)ceil(6.0 * sigma + 3.0),
               "%s: a patch table of S = %d for sigma = %g; S = ceil(6 sigma + 3) = %d and at most %d is needed", who, S,
               sigma, (int)ceil(6.0 * sigma + 3.0), RTPE_DISTILL_MAX_PATCH);
  return RTPE_OK;
}

// normalise (pred null) and loss share their checks and launches
int run_elem(const char* who, int kind, int normalise, const float* pred, int pred_channels, const float* teacher,
             const float* gt, const float* mask, int mask_channels, int N, int J, int h, int w, double alpha, float bf,
             float pw_t, float pw_g, const float* minmax, float* gt_out, float* teacher_out, float* mask_out,
             void* loss_out, void* scratch, size_t scratch_bytes, void* stream) {
  RTPE_REQUIRE(gt && scratch, "%s: null gt or scratch", who);
  RTPE_REQUIRE(N > 0 && J > 0 && h > 0 && w > 0, "%s: N = %d, J = %d, h = %d, w = %d must be positive", who, N, J, h, w);
  RTPE_REQUIRE(!mask || mask_channels == 1 || mask_channels == J, "%s: mask_channels = %d is neither 1 nor J = %d", who,
               mask_channels, J);
  RTPE_REQUIRE(!(teacher_out && !teacher) && !(mask_out && !mask), "%s: an output without its input", who);
  RTPE_REQUIRE(bf >= 0.f && bf <= 1.f, "%s: background_factor = %g outside [0, 1]", who, (double)bf);
  RTPE_REQUIRE(scratch_bytes >= RTPE_DISTILL_SCRATCH_BYTES && reinterpret_cast<uintptr_t>(scratch) % 8 == 0,
               "%s: scratch of %zu bytes; %d bytes, 8-byte aligned, are needed", who, scratch_bytes,
               RTPE_DISTILL_SCRATCH_BYTES);
  if (pred) {
    RTPE_REQUIRE(kind == RTPE_DISTILL_BCE || kind == RTPE_DISTILL_MSE, "%s: kind = %d is neither 0 (bce) nor 1 (mse)",
                 who, kind);
    RTPE_REQUIRE(pred_channels >= J, "%s: pred_channels = %d is below J = %d", who, pred_channels, J);
    RTPE_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "%s: alpha = %g outside [0, 1]", who, alpha);
    RTPE_REQUIRE(loss_out && reinterpret_cast<uintptr_t>(loss_out) % 8 == 0, "%s: loss_out is null or not 8-byte aligned",
                 who);
    RTPE_REQUIRE((long long)N * pred_channels <= 0x7fffffffLL, "%s: N * pred_channels = %lld is too large", who,
                 (long long)N * pred_channels);
  }
  RTPE_REQUIRE((long long)h * w <= 0x7fffffffLL && (long long)N * J <= 0x7fffffffLL, "%s: h * w or N * J exceeds 2^31 - 1",
               who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned char* sc = static_cast<unsigned char*>(scratch);
  ElemArgs a;
  a.n = (size_t)N * J * h * w;
  a.hw = (long long)h * w;
  a.chw = a.hw * J;
  const int blocks = reduction_blocks(a.n);
  a.minmax = nullptr;
  if (normalise) {
    a.minmax = minmax;
    if (!minmax) {
      MinMax* part = reinterpret_cast<MinMax*>(sc + kScratchMmPart);
      float* mm = reinterpret_cast<float*>(sc + kScratchMinMax);
      hipLaunchKernelGGL(minmax_partial_kernel, dim3(blocks), dim3(kThreads), 0, st, gt, teacher, a.n, part);
      hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(kThreads), 0, st, (const MinMax*)part, blocks, 1,
                         teacher ? 1 : 0, mm);
      a.minmax = mm;
    }
  }
  a.pred = pred; a.teacher = teacher; a.gt = gt; a.mask = mask;
  a.gt_out = gt_out; a.teacher_out = teacher_out; a.mask_out = mask_out;
  a.part = reinterpret_cast<double*>(sc + kScratchSums);
  a.J = J; a.pred_channels = pred_channels; a.mask_channels = mask_channels; a.kind = kind;
  a.bf = bf; a.pw_t = pw_t; a.pw_g = pw_g;
  hipLaunchKernelGGL(elem_kernel, dim3(blocks), dim3(kThreads), 0, st, a);
  if (pred)
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(kThreads), 0, st, (const double*)a.part, blocks, (double)a.n,
                       alpha, static_cast<unsigned char*>(loss_out));
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

}  // namespace
}  // namespace rtpe

using namespace rtpe;

extern "C" int rtpe_gt_heatmaps(const int32_t* offsets, const double* joints, int32_t P_total, int32_t N, int32_t J,
                                int32_t H, int32_t W, const float* patch, int32_t S, double sigma, float* out,
                                void* stream) {
  RTPE_REQUIRE(offsets && joints && patch && out, "gt_heatmaps: null offsets, joints, patch or out");
  RTPE_REQUIRE(N > 0 && J > 0 && H > 0 && W > 0 && P_total >= 0,
               "gt_heatmaps: N = %d, J = %d, H = %d, W = %d must be positive, P_total = %d not negative", N, J, H, W,
               P_total);
  if (int rc = check_patch("gt_heatmaps", S, sigma)) return rc;
  RTPE_REQUIRE(reinterpret_cast<uintptr_t>(joints) % 8 == 0, "gt_heatmaps: joints must be 8-byte aligned");
  RTPE_REQUIRE((long long)H * W <= 0x7fffffffLL - kThreads && (long long)P_total * J <= 0x7fffffffLL / 3,
               "gt_heatmaps: H * W or P_total * J is too large");
  GtArgs a;
  a.bpp = blocks_per_plane(H, W);
  const long long blocks = (long long)N * J * a.bpp;
  RTPE_REQUIRE(blocks <= 0x7fffffffLL, "gt_heatmaps: %lld workgroups, at most 2^31 - 1 fit one launch", blocks);
  a.offsets = offsets; a.joints = joints; a.patch = patch; a.out = out;
  a.s3 = 3 * sigma;
  a.P_total = P_total; a.J = J; a.H = H; a.W = W; a.S = S;
  hipLaunchKernelGGL(gt_heatmaps_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     a);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

extern "C" int rtpe_distill_targets_scratch_bytes(int32_t N, int32_t J, int32_t h, int32_t w, size_t* bytes) {
  RTPE_REQUIRE(bytes, "distill_targets_scratch_bytes: null bytes");
  RTPE_REQUIRE(N > 0 && J > 0 && h > 0 && w > 0,
               "distill_targets_scratch_bytes: N = %d, J = %d, h = %d, w = %d must be positive", N, J, h, w);
  RTPE_REQUIRE((long long)h * w <= 0x7fffffffLL - kThreads, "distill_targets_scratch_bytes: h * w is too large");
  const long long blocks = (long long)N * J * blocks_per_plane(h, w);
  RTPE_REQUIRE(blocks <= 0x7fffffffLL, "distill_targets_scratch_bytes: %lld workgroups, at most 2^31 - 1 fit one launch",
               blocks);
  *bytes = (size_t)blocks * sizeof(MinMax);
  return RTPE_OK;
}

extern "C" int rtpe_distill_targets(const int32_t* offsets, const double* joints, int32_t P_total, const float* patch,
                                    int32_t S, double sigma, const float* teacher, int32_t ht, int32_t wt,
                                    const float* mask, const float* segm, int32_t N, int32_t J, int32_t H, int32_t W,
                                    int32_t h, int32_t w, int32_t ha, int32_t wa, float* gt_out, float* teacher_out,
                                    float* mask_out, float* segm_out, float* minmax, void* scratch,
                                    size_t scratch_bytes, void* stream) {
  RTPE_REQUIRE(minmax && scratch, "distill_targets: null minmax or scratch");
  RTPE_REQUIRE(N > 0 && J > 0 && H > 0 && W > 0 && h > 0 && w > 0,
               "distill_targets: N = %d, J = %d, H = %d, W = %d, h = %d, w = %d must be positive", N, J, H, W, h, w);
  const bool has_gt = offsets || joints || patch || gt_out;
  RTPE_REQUIRE(!has_gt || (offsets && joints && patch && gt_out),
               "distill_targets: offsets, joints, patch and gt_out go together: all or none");
  RTPE_REQUIRE(!teacher == !teacher_out && !mask == !mask_out && !segm == !segm_out,
               "distill_targets: teacher, mask and segm each go with their output: both or neither");
  if (has_gt) {
    if (int rc = check_patch("distill_targets", S, sigma)) return rc;
    RTPE_REQUIRE(P_total >= 0 && (long long)P_total * J <= 0x7fffffffLL / 3,
                 "distill_targets: P_total = %d is negative or P_total * J too large", P_total);
    RTPE_REQUIRE(reinterpret_cast<uintptr_t>(joints) % 8 == 0, "distill_targets: joints must be 8-byte aligned");
  }
  RTPE_REQUIRE(!teacher || (ht > 0 && wt > 0), "distill_targets: teacher source of (%d, %d)", ht, wt);
  RTPE_REQUIRE(!segm || (ha > 0 && wa > 0), "distill_targets: attention grid of (%d, %d)", ha, wa);
  RTPE_REQUIRE((long long)H * W <= 0x7fffffffLL && (long long)h * w <= 0x7fffffffLL - kThreads &&
               (!teacher || (long long)ht * wt <= 0x7fffffffLL) && (!segm || (long long)ha * wa <= 0x7fffffffLL - kThreads),
               "distill_targets: a plane of more than 2^31 - 1 pixels");
  TargetArgs a;
  a.bpp = blocks_per_plane(h, w);
  const long long blocks = (long long)N * J * a.bpp;
  const long long blocks_seg = segm ? (long long)N * blocks_per_plane(ha, wa) : 0;
  RTPE_REQUIRE(blocks <= 0x7fffffffLL && blocks_seg <= 0x7fffffffLL,
               "distill_targets: %lld workgroups, at most 2^31 - 1 fit one launch", blocks > blocks_seg ? blocks : blocks_seg);
  RTPE_REQUIRE(scratch_bytes / sizeof(MinMax) >= (size_t)blocks && reinterpret_cast<uintptr_t>(scratch) % 8 == 0,
               "distill_targets: scratch of %zu bytes; %zu bytes, 8-byte aligned, are needed", scratch_bytes,
               (size_t)blocks * sizeof(MinMax));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  a.offsets = offsets; a.joints = joints; a.patch = patch; a.teacher = teacher;
  a.gt_out = gt_out; a.teacher_out = teacher_out;
  a.part = static_cast<MinMax*>(scratch);
  a.s3 = 3 * sigma;
  a.r1 = make_resize(teacher ? ht : H, teacher ? wt : W, H, W, true);
  a.r2 = make_resize(H, W, h, w, false);
  a.P_total = P_total; a.J = J; a.H = H; a.W = W; a.S = S;
  const bool main_launch = has_gt || teacher;
  if (main_launch) hipLaunchKernelGGL(targets_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(kThreads), 0, st, (const MinMax*)a.part,
                     main_launch ? (int)blocks : 0, has_gt ? 1 : 0, teacher ? 1 : 0, minmax);
  if (mask)
    hipLaunchKernelGGL(plane_resize_kernel, dim3((unsigned)((long long)N * a.bpp)), dim3(kThreads), 0, st, mask, mask_out,
                       a.r2, a.bpp);
  if (segm)
    hipLaunchKernelGGL(plane_resize_kernel, dim3((unsigned)blocks_seg), dim3(kThreads), 0, st, segm, segm_out,
                       make_resize(H, W, ha, wa, false), blocks_per_plane(ha, wa));
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

extern "C" int rtpe_distill_normalise(const float* gt, const float* teacher, const float* mask, int32_t mask_channels,
                                      int32_t N, int32_t J, int32_t h, int32_t w, float background_factor,
                                      const float* minmax, float* gt_out, float* teacher_out, float* mask_out,
                                      void* scratch, size_t scratch_bytes, void* stream) {
  RTPE_REQUIRE(gt_out, "distill_normalise: null gt_out");
  return run_elem("distill_normalise", 0, 1, nullptr, 0, teacher, gt, mask, mask_channels, N, J, h, w, 0.0,
                  background_factor, 1.f, 1.f, minmax, gt_out, teacher_out, mask_out, nullptr, scratch, scratch_bytes,
                  stream);
}

extern "C" int rtpe_distill_loss(int32_t kind, int32_t normalise, const float* pred, int32_t pred_channels,
                                 const float* teacher, const float* gt, const float* mask, int32_t mask_channels,
                                 int32_t N, int32_t J, int32_t h, int32_t w, double alpha, float background_factor,
                                 float teacher_pos_weight, float gt_pos_weight, const float* minmax, float* gt_out,
                                 float* teacher_out, float* mask_out, void* loss_out, void* scratch,
                                 size_t scratch_bytes, void* stream) {
  RTPE_REQUIRE(pred, "distill_loss: null pred");
  return run_elem("distill_loss", kind, normalise, pred, pred_channels, teacher, gt, mask, mask_channels, N, J, h, w,
                  alpha, background_factor, teacher_pos_weight, gt_pos_weight, minmax, gt_out, teacher_out, mask_out,
                  loss_out, scratch, scratch_bytes, stream);
}
