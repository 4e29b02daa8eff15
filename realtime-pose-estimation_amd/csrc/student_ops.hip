// The small NHWC ops of the dual-head student (config 5: AttentionStudent,
// rtpe/students.py:595-771 of the reference, built from ContextAwareModule
// :145-201 and SELayer :118-142).  All are single-pass, HBM/latency-bound;
// channel counts are multiples of 4 (16-byte rows pieces).  avgpool, se, cam_combine, sigmoid_add, gate_mul, aux_pack and
// resize also have an fp16 form (the half bodies: 16-byte pieces of 8 channels).
#include "rtpe_common.h"
#include "alt_colour.h"

namespace rtpe {

typedef _Float16 half4v __attribute__((ext_vector_type(4)));

// fp16 NHWC -> fp32 NHWC (the tofp32 at the end of the half-wrapped stem, fp16util.py:64-68)
__global__ void __launch_bounds__(256) cast_kernel(const _Float16* x, int in_ld, float* y, int out_ld, int C,
                                                   size_t pixels) {
  const int c4 = C >> 2;
  const size_t total = pixels * c4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t p = i / c4;
    const int c = (int)(i - p * c4) * 4;
    const half4v v = *reinterpret_cast<const half4v*>(x + p * in_ld + c);
    *reinterpret_cast<float4*>(y + p * out_ld + c) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  }
}

// The seven templates below exist in two storage precisions, like the convs (conv_mfma.hip, Prec<T>): fp32 (float, 4 channels
// per 16-byte access) and fp16 (_Float16, 8 channels per 16-byte access: the half bodies of AttentionStudent(body_half=True)
// and AttentionStudentStepsHalf).  The arithmetic is fp32 in both; Elem<T>::rnd marks the points at which PyTorch-CPU's half
// ops round to fp16 (pinned by tests/test_student_half_host.py and tests/test_steps_half_host.py) and is the identity for
// fp32, whose instantiations compute what they always did.
template <typename T> struct Elem;
template <> struct Elem<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ float rnd(float v) { return v; }
};
template <> struct Elem<_Float16> {
  static constexpr int N = 8;
  // (the fp32 value is kept opaque, as in conv_mfma.hip's epilogue: the compiler would fuse the operation before it with the
  // conversion into one v_fma_mix*_f16, which rounds the exact result once where PyTorch rounds to fp32 and then to fp16)
  static __device__ __forceinline__ float rnd(float v) {
    asm volatile("" : "+v"(v));
    return (float)(_Float16)v;
  }
};

template <typename T> struct Row {           // 16 bytes of a channel row, as fp32 values
  float v[Elem<T>::N];
  static __device__ __forceinline__ Row load(const T* p) {
    T raw[Elem<T>::N];
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    __builtin_memcpy(raw, &u, 16);
    Row r;
#pragma unroll
    for (int j = 0; j < Elem<T>::N; ++j) r.v[j] = (float)raw[j];
    return r;
  }
  __device__ __forceinline__ void store(T* p) const {   // (the values are representable in T: rounded by Elem<T>::rnd)
    T raw[Elem<T>::N];
#pragma unroll
    for (int j = 0; j < Elem<T>::N; ++j) raw[j] = (T)v[j];
    uint4 u;
    __builtin_memcpy(&u, raw, 16);
    *reinterpret_cast<uint4*>(p) = u;
  }
};

// AvgPool2d(kernel_size=3, stride=2, padding=1, count_include_pad=False), students.py:657-666
// fp16: the window is summed and divided in fp32, one rounding (ATen's avg_pool2d accumulates a half input in float)
// ext (mixed-size batches): (h, w) of every image inside the H x W canvas - the window and its divisor count the taps inside
// the image, outputs exist up to ceil(h / 2) x ceil(w / 2); H, W, Ho, Wo of the canvas address
template <typename T>
__global__ void __launch_bounds__(256) avgpool_kernel(const T* x, int in_ld, T* y, int out_ld, int C, int N, int H, int W,
                                                      const int* ext) {
  constexpr int EN = Elem<T>::N;
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  const int c4 = C / EN;
  const size_t total = (size_t)N * Ho * Wo * c4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % c4) * EN;
    size_t p = i / c4;
    const int ox = (int)(p % Wo);
    p /= Wo;
    const int oy = (int)(p % Ho);
    const int n = (int)(p / Ho);
    int Hm = H, Wm = W;
    if (ext != nullptr) {
      Hm = ext[2 * n]; Wm = ext[2 * n + 1];
      if (oy >= ((Hm + 1) >> 1) || ox >= ((Wm + 1) >> 1)) continue;
    }
    Row<T> s;
#pragma unroll
    for (int j = 0; j < EN; ++j) s.v[j] = 0.f;
    int cnt = 0;
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = 2 * oy - 1 + ky;
      if ((unsigned)iy >= (unsigned)Hm) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = 2 * ox - 1 + kx;
        if ((unsigned)ix >= (unsigned)Wm) continue;
        const Row<T> v = Row<T>::load(x + (((size_t)n * H + iy) * W + ix) * in_ld + c);
#pragma unroll
        for (int j = 0; j < EN; ++j) s.v[j] += v.v[j];
        ++cnt;
      }
    }
    const float d = (float)cnt;
#pragma unroll
    for (int j = 0; j < EN; ++j) s.v[j] = Elem<T>::rnd(s.v[j] / d);
    s.store(y + (((size_t)n * Ho + oy) * Wo + ox) * out_ld + c);
  }
}

// SELayer, students.py:137-142: gate[n, c] = sigmoid(W2 relu(W1 mean_hw(x) + b1) + b2)
// one workgroup per image; w: fc1 (hid, C) | b1 (hid) | fc2 (C, hid) | b2 (C), fp32 (fp16: the values of the half parameters)
// fp16 rounds the mean (an fp32 sum divided by HW), each Linear behind its bias, and the sigmoid
constexpr int kSeMaxC = 512, kSeMaxHid = 128;
template <typename T>
// ext (mixed-size batches): image n's map is h x w inside a canvas of HW pixels with rows of Wc - the loops walk the image's
// own row-major pixel index p < h * w, as they would on the image alone (same fp32 summation order, same bits), and map it
// to the canvas pixel (p / w) * Wc + p % w; the mean divides by h * w
__global__ void __launch_bounds__(256) se_kernel(const T* x, int in_ld, int C, int hid, int HW, const float* w, T* gate,
                                                 int gate_ld, const int* ext, int Wc) {
  __shared__ float mean[kSeMaxC];
  __shared__ float part[4 * kSeMaxC];
  __shared__ float hbuf[kSeMaxHid];
  const int n = blockIdx.x;
  const T* xi = x + (size_t)n * HW * in_ld;
  const int wm = ext != nullptr ? ext[2 * n + 1] : 0;
  if (ext != nullptr) HW = ext[2 * n] * wm;
  auto canvas = [&](int p) { return ext != nullptr ? (p / wm) * Wc + (p - (p / wm) * wm) : p; };
  if constexpr (sizeof(T) == 4) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // each wave sums a quarter of the pixels; lanes stride over channels
    for (int c = lane; c < C; c += 64) {
      float s = 0.f;
      for (int p = wv; p < HW; p += 4) s += xi[(size_t)canvas(p) * in_ld + c];
      part[wv * kSeMaxC + c] = s;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256)
      mean[c] = (part[c] + part[kSeMaxC + c] + part[2 * kSeMaxC + c] + part[3 * kSeMaxC + c]) / (float)HW;
  } else {
    // 16-byte pieces of 8 channels: thread (g, o) sums piece o of the pixels g, g + G, ...; G = 256 / pieces >= 4 groups
    const int no = (C + 7) >> 3, G = 256 / no, row = no * 8;       // (G * row <= 2048 floats of part)
    const int g = threadIdx.x / no, o = threadIdx.x - g * no;
    if (g < G) {
      Row<T> s;
#pragma unroll
      for (int j = 0; j < 8; ++j) s.v[j] = 0.f;
      for (int p = g; p < HW; p += G) {
        const Row<T> v = Row<T>::load(xi + (size_t)canvas(p) * in_ld + o * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) s.v[j] += v.v[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) part[g * row + o * 8 + j] = s.v[j];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
      float s = part[c];
      for (int k = 1; k < G; ++k) s += part[k * row + c];
      mean[c] = Elem<T>::rnd(s / (float)HW);
    }
  }
  __syncthreads();
  const float* w1 = w;
  const float* b1 = w1 + (size_t)hid * C;
  const float* w2 = b1 + hid;
  const float* b2 = w2 + (size_t)C * hid;
  for (int j = threadIdx.x; j < hid; j += 256) {
    float s = b1[j];
    for (int c = 0; c < C; ++c) s = __builtin_fmaf(w1[(size_t)j * C + c], mean[c], s);
    s = Elem<T>::rnd(s);
    hbuf[j] = s > 0.f ? s : 0.f;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = b2[c];
    for (int j = 0; j < hid; ++j) s = __builtin_fmaf(w2[(size_t)c * hid + j], hbuf[j], s);
    s = Elem<T>::rnd(s);
    gate[(size_t)n * gate_ld + c] = (T)Elem<T>::rnd(1.f / (1.f + expf(-s)));
  }
  // padding channels of the gate row (C not a multiple of 4): finite zeros, the combine op multiplies them in
  for (int c = C + threadIdx.x; c < gate_ld; c += 256) gate[(size_t)n * gate_ld + c] = (T)0.f;
}

// ContextAwareModule tail, students.py:199-200: relu(residual + hdc * gate[n, c]); fp16 rounds the product and the sum
template <typename T>
__global__ void __launch_bounds__(256) cam_combine_kernel(const T* hdc, int hdc_ld, const T* res, int res_ld, const T* gate,
                                                          int gate_ld, T* y, int out_ld, int C, int N, size_t pix_per_image) {
  constexpr int EN = Elem<T>::N;
  const int c4 = C / EN;
  const size_t total = (size_t)N * pix_per_image * c4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t p = i / c4;
    const int c = (int)(i - p * c4) * EN;
    const int n = (int)(p / pix_per_image);
    const Row<T> h = Row<T>::load(hdc + p * hdc_ld + c);
    const Row<T> r = Row<T>::load(res + p * res_ld + c);
    const Row<T> g = Row<T>::load(gate + (size_t)n * gate_ld + c);
    Row<T> o;
#pragma unroll
    for (int j = 0; j < EN; ++j) {
      const float t = Elem<T>::rnd(h.v[j] * g.v[j]);
      const float v = Elem<T>::rnd(r.v[j] + t);
      o.v[j] = v > 0.f ? v : 0.f;
    }
    o.store(y + p * out_ld + c);
  }
}

// AttentionStudent.forward, students.py:755-756: att = sigmoid(att / 20); stem_out + att (broadcast over C);
// also emits att as the first NCHW output (N,1,H,W), fp32 in both precisions; fp16 rounds the quotient, the sigmoid and the sum
template <typename T>
__global__ void __launch_bounds__(256) sigmoid_add_kernel(const T* att, int att_ld, const T* x, int x_ld, T* y, int out_ld,
                                                          int C, size_t pixels, float* att_out) {
  constexpr int EN = Elem<T>::N;
  const int c4 = C / EN;
  const size_t total = pixels * c4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t p = i / c4;
    const int c = (int)(i - p * c4) * EN;
    const float l = Elem<T>::rnd((float)att[p * att_ld] / 20.f);
    const float a = Elem<T>::rnd(1.f / (1.f + expf(-l)));
    if (c == 0 && att_out) att_out[p] = a;
    Row<T> v = Row<T>::load(x + p * x_ld + c);
#pragma unroll
    for (int j = 0; j < EN; ++j) v.v[j] = Elem<T>::rnd(v.v[j] + a);
    v.store(y + p * out_ld + c);
  }
}

// AttentionStudentSteps.forward, students.py:1012-1040: att = sigmoid(att [/ att_divisor]); stem_out * att
// (broadcast over the channels); also emits att as the first NCHW output (N,1,H,W), fp32 in both precisions; fp16 (the half
// body of AttentionStudentStepsHalf; rounding points pinned by tests/test_steps_half_host.py) rounds the quotient, the sigmoid
// and each product
template <typename T>
__global__ void __launch_bounds__(256) gate_mul_kernel(const T* att, int att_ld, const T* x, int x_ld, T* y, int out_ld, int C,
                                                       size_t pixels, float div, float* att_out) {
  constexpr int EN = Elem<T>::N;
  const int c4 = C / EN;
  const size_t total = pixels * c4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t p = i / c4;
    const int c = (int)(i - p * c4) * EN;
    float l = (float)att[p * att_ld];
    if (div != 0.f) l = Elem<T>::rnd(l / div);
    const float a = Elem<T>::rnd(1.f / (1.f + expf(-l)));
    if (c == 0 && att_out) att_out[p] = a;
    Row<T> v = Row<T>::load(x + p * x_ld + c);
#pragma unroll
    for (int j = 0; j < EN; ++j) v.v[j] = Elem<T>::rnd(v.v[j] * a);
    v.store(y + p * out_ld + c);
  }
}

// the second network input: (N,3,H,W) fp32 NCHW -> NHWC rows of 16 bytes: fp32 (r, g, b, 0); fp16 (r, g, b, 0, 0, 0, 0, 0), each
// value rounded to nearest even (beyond the fp16 range: infinity), as alt.half()
template <typename T>
__global__ void __launch_bounds__(256) aux_pack_kernel(const float* a, T* y, int out_ld, int N, int H, int W) {
  const size_t plane = (size_t)H * W, total = (size_t)N * plane;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t n = i / plane, q = i - n * plane;
    const float* b = a + n * 3 * plane + q;
    Row<T> r;
#pragma unroll
    for (int j = 0; j < Elem<T>::N; ++j) r.v[j] = 0.f;
    r.v[0] = Elem<T>::rnd(b[0]); r.v[1] = Elem<T>::rnd(b[plane]); r.v[2] = Elem<T>::rnd(b[2 * plane]);
    r.store(y + i * out_ld);
  }
}

// F.interpolate(mode="bilinear", align_corners=False) on NHWC rows of C (multiple of 4) channels; PyTorch-CPU's
// arithmetic (see csrc/aggregate.hip): real = scale * (o + 0.5) - 0.5 clamped at 0, T = fma(v0, l0, v1 * l1)
__device__ __forceinline__ void axis_half_pixel(float scale, int n_in, int n_out, int o, int* i0, int* i1, float* l0, float* l1) {
  if (n_in == n_out) { *i0 = *i1 = o; *l0 = 1.f; *l1 = 0.f; return; }
  float real = __builtin_fmaf(scale, (float)o + 0.5f, -0.5f);   // ATen's build contracts scale * (o + 0.5) - 0.5
  real = real < 0.f ? 0.f : real;
  int a = (int)real;
  a = a < n_in - 1 ? a : n_in - 1;
  *i0 = a;
  *i1 = a + (a < n_in - 1 ? 1 : 0);
  float l = real - (float)a;
  l = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
  *l1 = l;
  *l0 = 1.f - l;
}

// MIXED (a mixed-size batch, rtpe_hip_mixed_aux.h): Hi, Wi, Ho, Wo are the canvas extents and only address; image n's own
// input and output extents come from its rows of the extent table (ext_in, ext_out), and with them everything that
// F.interpolate of that image alone derives from its size: the scale (the same correctly rounded float division as on the
// host), the clamp at h_n - 1, the n_in == n_out shortcut.  Nothing is stored beyond image n's output extent.  !MIXED: the
// kernel as it was, the scales from the host (an instantiation of its own, as conv_mfma_kernel's).
// fp16 (16-byte pieces of 8 channels, !MIXED only): the same coordinates and weights, fp32 arithmetic on the fp16 values and ONE
// rounding of the result.  The four taps are combined as PyTorch-CPU's kernel combines them - the weights multiplied first
// (ly * lx, rounded), then v01 * w01, fma(v00, w00, .), fma(v10, w10, .), fma(v11, w11, .) - not with the three fmas of the
// fp32 form: the two differ in the last fp32 bit at scales that are no fp32 numbers (33 -> 9), which an fp16 rounding next to
// a tie turns into a whole fp16 step (pinned by tests/test_steps_half_host.py).  The fp32 form keeps its arithmetic.
template <bool MIXED, typename T = float>
__global__ void __launch_bounds__(256) resize_nhwc_kernel(const T* x, int in_ld, int Hi, int Wi, T* y, int out_ld,
                                                          int Ho, int Wo, int C, int N, float sy, float sx,
                                                          const int* ext_in, const int* ext_out) {
  constexpr int EN = Elem<T>::N;
  const int c4 = C / EN;
  const size_t total = (size_t)N * Ho * Wo * c4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % c4) * EN;
    size_t p = i / c4;
    const int ox = (int)(p % Wo);
    p /= Wo;
    const int oy = (int)(p % Ho);
    const int n = (int)(p / Ho);
    int hi = Hi, wi = Wi, ho = Ho, wo = Wo;
    if constexpr (MIXED) {
      hi = ext_in[2 * n]; wi = ext_in[2 * n + 1];
      ho = ext_out[2 * n]; wo = ext_out[2 * n + 1];
      if (oy >= ho || ox >= wo) continue;
      sy = __fdiv_rn((float)hi, (float)ho);
      sx = __fdiv_rn((float)wi, (float)wo);
    }
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    axis_half_pixel(sy, hi, ho, oy, &y0, &y1, &ly0, &ly1);
    axis_half_pixel(sx, wi, wo, ox, &x0, &x1, &lx0, &lx1);
    const T* b = x + (size_t)n * Hi * Wi * in_ld + c;
    const Row<T> v00 = Row<T>::load(b + ((size_t)y0 * Wi + x0) * in_ld);
    const Row<T> v01 = Row<T>::load(b + ((size_t)y0 * Wi + x1) * in_ld);
    const Row<T> v10 = Row<T>::load(b + ((size_t)y1 * Wi + x0) * in_ld);
    const Row<T> v11 = Row<T>::load(b + ((size_t)y1 * Wi + x1) * in_ld);
    const float w00 = ly0 * lx0, w01 = ly0 * lx1, w10 = ly1 * lx0, w11 = ly1 * lx1;      // (read by the fp16 form only)
    auto one = [&](float a00, float a01, float a10, float a11) {
      if constexpr (sizeof(T) == 2) {
        return __builtin_fmaf(a11, w11, __builtin_fmaf(a10, w10, __builtin_fmaf(a00, w00, a01 * w01)));
      } else {
        const float t0 = __builtin_fmaf(a00, lx0, a01 * lx1);
        const float t1 = __builtin_fmaf(a10, lx0, a11 * lx1);
        return __builtin_fmaf(t0, ly0, t1 * ly1);
      }
    };
    Row<T> o;
#pragma unroll
    for (int j = 0; j < EN; ++j) o.v[j] = Elem<T>::rnd(one(v00.v[j], v01.v[j], v10.v[j], v11.v[j]));
    o.store(y + (((size_t)n * Ho + oy) * Wo + ox) * out_ld + c);
  }
}

// skimage.color.rgb2lab / rgb2hsv on (N,3,H,W) fp32 in [0,1] (rtpe/dataloaders.py:352-356 of the reference)
__global__ void __launch_bounds__(256) rgb_to_alt_kernel(const float* src, float* dst, int N, size_t plane, int mode) {
  const size_t total = (size_t)N * plane;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t n = i / plane, q = i - n * plane;
    const float* b = src + n * 3 * plane + q;
    float* o = dst + n * 3 * plane + q;
    const float r = b[0], g = b[plane], bl = b[2 * plane];
    float o0, o1, o2;
    rgb_to_alt_pixel(r, g, bl, mode, o0, o1, o2);        // alt_colour.h: frames_kernel calls the same function
    o[0] = o0; o[plane] = o1; o[2 * plane] = o2;
  }
}

// mixed-size batches: every element of the two fp32 NCHW outputs outside its image's own h x w becomes 0.0 (whatever the
// forward left there: tiles outside an image are never computed, sigmoid_add runs over the whole canvas)
__global__ void __launch_bounds__(256) mask_outputs_kernel(float* y0, int C0, int H0, int W0, const int* ext0, float* y1,
                                                           int C1, int H1, int W1, const int* ext1, int N) {
  const size_t t0 = (size_t)N * C0 * H0 * W0, t1 = (size_t)N * C1 * H1 * W1;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < t0 + t1; i += (size_t)gridDim.x * 256) {
    const bool second = i >= t0;
    const size_t k = second ? i - t0 : i;
    const int C = second ? C1 : C0, H = second ? H1 : H0, W = second ? W1 : W0;
    const int* ext = second ? ext1 : ext0;
    const int x = (int)(k % W), y = (int)((k / W) % H), n = (int)(k / ((size_t)W * H * C));
    if (y >= ext[2 * n] || x >= ext[2 * n + 1]) (second ? y1 : y0)[k] = 0.f;
  }
}

static unsigned grid_for(size_t total) {
  size_t b = (total + 255) / 256;
  if (b > 256 * 16) b = 256 * 16;
  return (unsigned)(b ? b : 1);
}

int cast_launch(const _Float16* x, int in_ld, float* y, int out_ld, int C, size_t pixels, hipStream_t s) {
  RTPE_REQUIRE(C % 4 == 0 && in_ld % 4 == 0 && out_ld % 4 == 0, "cast: channel counts must be multiples of 4");
  hipLaunchKernelGGL(cast_kernel, dim3(grid_for(pixels * (C / 4))), dim3(256), 0, s, x, in_ld, y, out_ld, C, pixels);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

template <typename T>
static int avgpool_launch_t(const T* x, int in_ld, T* y, int out_ld, int C, int N, int H, int W, hipStream_t s, const int* ext) {
  constexpr int EN = Elem<T>::N;
  RTPE_REQUIRE(C % EN == 0 && in_ld % EN == 0 && out_ld % EN == 0, "avgpool: channel counts must be multiples of %d", EN);
  const size_t total = (size_t)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / EN);
  hipLaunchKernelGGL(avgpool_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, x, in_ld, y, out_ld, C, N, H, W, ext);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

int avgpool_launch(const float* x, int in_ld, float* y, int out_ld, int C, int N, int H, int W, hipStream_t s, const int* ext) {
  return avgpool_launch_t<float>(x, in_ld, y, out_ld, C, N, H, W, s, ext);
}

int avgpool_launch(const _Float16* x, int in_ld, _Float16* y, int out_ld, int C, int N, int H, int W, hipStream_t s,
                   const int* ext) {
  return avgpool_launch_t<_Float16>(x, in_ld, y, out_ld, C, N, H, W, s, ext);
}

int se_launch(const float* x, int in_ld, int C, int hid, int N, int HW, const float* w, float* gate, int gate_ld,
              hipStream_t s, const int* ext, int Wc) {
  RTPE_REQUIRE(C <= kSeMaxC && hid <= kSeMaxHid && C > 0 && hid > 0, "se: C=%d hidden=%d unsupported", C, hid);
  hipLaunchKernelGGL(se_kernel<float>, dim3(N), dim3(256), 0, s, x, in_ld, C, hid, HW, w, gate, gate_ld, ext, Wc);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

// fp16: the rows of x are read in 16-byte pieces up to the piece that holds channel C - 1
int se_launch(const _Float16* x, int in_ld, int C, int hid, int N, int HW, const float* w, _Float16* gate, int gate_ld,
              hipStream_t s, const int* ext, int Wc) {
  RTPE_REQUIRE(C <= kSeMaxC && hid <= kSeMaxHid && C > 0 && hid > 0, "se: C=%d hidden=%d unsupported", C, hid);
  RTPE_REQUIRE(in_ld % 8 == 0 && in_ld >= (C + 7) / 8 * 8 && gate_ld >= C, "se: rows of %d and %d halves for C=%d", in_ld, gate_ld, C);
  hipLaunchKernelGGL(se_kernel<_Float16>, dim3(N), dim3(256), 0, s, x, in_ld, C, hid, HW, w, gate, gate_ld, ext, Wc);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

template <typename T>
static int cam_combine_launch_t(const T* hdc, int hdc_ld, const T* res, int res_ld, const T* gate, int gate_ld, T* y,
                                int out_ld, int C, int N, size_t pix_per_image, hipStream_t s) {
  constexpr int EN = Elem<T>::N;
  RTPE_REQUIRE(C % EN == 0 && gate_ld % EN == 0 && (EN == 4 || (hdc_ld % EN == 0 && res_ld % EN == 0 && out_ld % EN == 0)),
               "cam_combine: C must be a multiple of %d", EN);
  hipLaunchKernelGGL(cam_combine_kernel<T>, dim3(grid_for((size_t)N * pix_per_image * (C / EN))), dim3(256), 0, s, hdc,
                     hdc_ld, res, res_ld, gate, gate_ld, y, out_ld, C, N, pix_per_image);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

int cam_combine_launch(const float* hdc, int hdc_ld, const float* res, int res_ld, const float* gate, int gate_ld,
                       float* y, int out_ld, int C, int N, size_t pix_per_image, hipStream_t s) {
  return cam_combine_launch_t<float>(hdc, hdc_ld, res, res_ld, gate, gate_ld, y, out_ld, C, N, pix_per_image, s);
}

int cam_combine_launch(const _Float16* hdc, int hdc_ld, const _Float16* res, int res_ld, const _Float16* gate, int gate_ld,
                       _Float16* y, int out_ld, int C, int N, size_t pix_per_image, hipStream_t s) {
  return cam_combine_launch_t<_Float16>(hdc, hdc_ld, res, res_ld, gate, gate_ld, y, out_ld, C, N, pix_per_image, s);
}

template <typename T>
static int sigmoid_add_launch_t(const T* att, int att_ld, const T* x, int x_ld, T* y, int out_ld, int C, size_t pixels,
                                float* att_out, hipStream_t s) {
  constexpr int EN = Elem<T>::N;
  RTPE_REQUIRE(C % EN == 0 && (EN == 4 || (x_ld % EN == 0 && out_ld % EN == 0)), "sigmoid_add: C must be a multiple of %d", EN);
  hipLaunchKernelGGL(sigmoid_add_kernel<T>, dim3(grid_for(pixels * (C / EN))), dim3(256), 0, s, att, att_ld, x, x_ld, y,
                     out_ld, C, pixels, att_out);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

int sigmoid_add_launch(const float* att, int att_ld, const float* x, int x_ld, float* y, int out_ld, int C,
                       size_t pixels, float* att_out, hipStream_t s) {
  return sigmoid_add_launch_t<float>(att, att_ld, x, x_ld, y, out_ld, C, pixels, att_out, s);
}

int sigmoid_add_launch(const _Float16* att, int att_ld, const _Float16* x, int x_ld, _Float16* y, int out_ld, int C,
                       size_t pixels, float* att_out, hipStream_t s) {
  return sigmoid_add_launch_t<_Float16>(att, att_ld, x, x_ld, y, out_ld, C, pixels, att_out, s);
}

int mask_outputs_launch(float* y0, int C0, int H0, int W0, const int* ext0, float* y1, int C1, int H1, int W1, const int* ext1,
                        int N, hipStream_t s) {
  RTPE_REQUIRE(ext0 && ext1 && N > 0 && (y0 || C0 == 0) && (y1 || C1 == 0) && C0 >= 0 && C1 >= 0 && H0 > 0 && W0 > 0 && H1 > 0 && W1 > 0,
               "mask_outputs: bad argument");
  if (C0 + C1 == 0) return RTPE_OK;
  const size_t total = (size_t)N * C0 * H0 * W0 + (size_t)N * C1 * H1 * W1;
  hipLaunchKernelGGL(mask_outputs_kernel, dim3(grid_for(total)), dim3(256), 0, s, y0, C0, H0, W0, ext0, y1, C1, H1, W1, ext1, N);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

template <typename T>
static int gate_mul_launch_t(const T* att, int att_ld, const T* x, int x_ld, T* y, int out_ld, int C, size_t pixels, float div,
                             float* att_out, hipStream_t s) {
  constexpr int EN = Elem<T>::N;
  RTPE_REQUIRE(C > 0 && C % EN == 0 && x_ld % EN == 0 && out_ld % EN == 0, "gate_mul: channel counts must be multiples of %d", EN);
  hipLaunchKernelGGL(gate_mul_kernel<T>, dim3(grid_for(pixels * (C / EN))), dim3(256), 0, s, att, att_ld, x, x_ld, y, out_ld,
                     C, pixels, div, att_out);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

int gate_mul_launch(const float* att, int att_ld, const float* x, int x_ld, float* y, int out_ld, int C, size_t pixels,
                    float div, float* att_out, hipStream_t s) {
  return gate_mul_launch_t<float>(att, att_ld, x, x_ld, y, out_ld, C, pixels, div, att_out, s);
}

int gate_mul_launch(const _Float16* att, int att_ld, const _Float16* x, int x_ld, _Float16* y, int out_ld, int C, size_t pixels,
                    float div, float* att_out, hipStream_t s) {
  return gate_mul_launch_t<_Float16>(att, att_ld, x, x_ld, y, out_ld, C, pixels, div, att_out, s);
}

template <typename T>
static int aux_pack_launch_t(const float* aux_nchw, T* y, int out_ld, int N, int H, int W, hipStream_t s) {
  constexpr int EN = Elem<T>::N;
  RTPE_REQUIRE(aux_nchw != nullptr && out_ld >= EN && out_ld % EN == 0, "aux_pack: bad argument");
  hipLaunchKernelGGL(aux_pack_kernel<T>, dim3(grid_for((size_t)N * H * W)), dim3(256), 0, s, aux_nchw, y, out_ld, N, H, W);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

int aux_pack_launch(const float* aux_nchw, float* y, int out_ld, int N, int H, int W, hipStream_t s) {
  return aux_pack_launch_t<float>(aux_nchw, y, out_ld, N, H, W, s);
}

int aux_pack_launch(const float* aux_nchw, _Float16* y, int out_ld, int N, int H, int W, hipStream_t s) {
  return aux_pack_launch_t<_Float16>(aux_nchw, y, out_ld, N, H, W, s);
}

int resize_nhwc_launch(const float* x, int in_ld, int Hi, int Wi, float* y, int out_ld, int Ho, int Wo, int C, int N,
                       hipStream_t s, const int* ext_in, const int* ext_out) {
  RTPE_REQUIRE(C % 4 == 0 && in_ld % 4 == 0 && out_ld % 4 == 0, "resize: channel counts must be multiples of 4");
  RTPE_REQUIRE((ext_in == nullptr) == (ext_out == nullptr), "resize: a mixed-size batch brings both rows of the extent table");
  const dim3 grid(grid_for((size_t)N * Ho * Wo * (C / 4)));
  if (ext_in != nullptr)       // the scales are derived on the device, per image
    hipLaunchKernelGGL(resize_nhwc_kernel<true>, grid, dim3(256), 0, s, x, in_ld, Hi, Wi, y, out_ld, Ho, Wo, C, N, 0.f, 0.f,
                       ext_in, ext_out);
  else
    hipLaunchKernelGGL(resize_nhwc_kernel<false>, grid, dim3(256), 0, s, x, in_ld, Hi, Wi, y, out_ld, Ho, Wo, C, N,
                       (float)Hi / (float)Ho, (float)Wi / (float)Wo, ext_in, ext_out);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

// fp16: one size per batch only (the masked form of a mixed-size batch exists in fp32 alone)
int resize_nhwc_launch(const _Float16* x, int in_ld, int Hi, int Wi, _Float16* y, int out_ld, int Ho, int Wo, int C, int N,
                       hipStream_t s, const int* ext_in, const int* ext_out) {
  RTPE_REQUIRE(C > 0 && C % 8 == 0 && in_ld % 8 == 0 && out_ld % 8 == 0, "resize: fp16 channel counts must be multiples of 8");
  RTPE_REQUIRE(ext_in == nullptr && ext_out == nullptr, "resize: the fp16 form takes no mixed-size batch");
  const dim3 grid(grid_for((size_t)N * Ho * Wo * (C / 8)));
  hipLaunchKernelGGL((resize_nhwc_kernel<false, _Float16>), grid, dim3(256), 0, s, x, in_ld, Hi, Wi, y, out_ld, Ho, Wo, C, N,
                     (float)Hi / (float)Ho, (float)Wi / (float)Wo, ext_in, ext_out);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}

}  // namespace rtpe

extern "C" int rtpe_rgb_to_alt(const float* src_nchw, int32_t N, int32_t H, int32_t W, int32_t mode, float* dst_nchw,
                               void* stream) {
  using namespace rtpe;
  RTPE_REQUIRE(src_nchw && dst_nchw && N > 0 && H > 0 && W > 0 && (mode == 0 || mode == 1), "rgb_to_alt: bad argument");
  hipLaunchKernelGGL(rgb_to_alt_kernel, dim3(grid_for((size_t)N * H * W)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), src_nchw, dst_nchw, N, (size_t)H * W, mode);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}
