// The gradient of the distillation losses with respect to the student's output (include/rtpe_hip_distill_grad.h; the
// rules: DESIGN.md section 4, "Distillation losses: backward").  One elementwise kernel over grad_pred: no reduction, no
// LDS, no atomics.  A thread owns four consecutive pixels of one plane (16-byte loads and stores) or, for planes and
// pointers that do not allow it, one pixel; the arithmetic per pixel is the same function, so are the bits.
// The file is compiled without contraction: the float64 operations below are evaluated as written, and the header
// states their order.
#include "rtpe_common.h"
#include "rtpe_hip_distill.h"
#include "rtpe_hip_distill_grad.h"

#include <math.h>

namespace rtpe {
namespace {

constexpr int kThreads = 256;

struct GradArgs {
  const float* pred;
  const float* teacher;     // null: no teacher term
  const float* gt;
  const float* mask;        // null: m = 1, no products
  const float* grad_loss;   // 3 floats, device memory
  float* out;
  double alpha, n;          // n = N * J * h * w
  long long units;          // threads with work: N * pred_channels * (hw / V)
  int hw, J, pred_channels, kind;
  float pw_t, pw_g;
};

struct Weights { double wt, wg, pw_t, pw_g; };

// T, M: a teacher term, a mask (template parameters, so that the four-pixel loads of either stay whole)
template <bool T, bool M>
__device__ __forceinline__ float grad_one(const GradArgs& a, const Weights& k, float p, float t, float g, float m) {
  const bool dead = M && m == 0.f;        // its +0.0 is selected at the end, not computed (a branch here would have
  double md = 1.0;                        // the compiler split the 16-byte loads into the pixels that survive it)
  if (M) {
    p = p * m; t = t * m; g = g * m;
    md = (double)m;
  }
  const double x = (double)p, yt = (double)t, yg = (double)g;
  double r;
  if (a.kind == RTPE_DISTILL_MSE) {
    const double tg = (k.wg * 2.0) * (x - yg);
    r = T ? (k.wt * 2.0) * (x - yt) + tg : tg;
  } else {
    const double e = exp(-fabs(x));
    const double d = 1.0 + e;
    const double s = x >= 0.0 ? 1.0 / d : e / d;
    const double qg = k.pw_g * yg;
    double aa = k.wg * ((1.0 - yg) + qg), bb = k.wg * qg;
    if (T) {
      const double qt = k.pw_t * yt;
      aa = k.wt * ((1.0 - yt) + qt) + aa;
      bb = k.wt * qt + bb;
    }
    r = (aa * s) - bb;
  }
  return dead ? 0.f : (float)((r * md) / a.n);
}

template <int V, bool T, bool M>
__global__ __launch_bounds__(kThreads) void distill_grad_kernel(GradArgs a) {
  const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (u >= a.units) return;
  const int upp = a.hw / V;                                   // units of a plane
  const long long plane = u / upp;                            // of grad_pred: N * pred_channels of them
  const int q = (int)(u - plane * upp);
  const long long img = plane / a.pred_channels;
  const int c = (int)(plane - img * a.pred_channels);
  const size_t o = (size_t)plane * (size_t)a.hw + (size_t)q * V;
  if (c >= a.J) {                                             // a channel without a target: +0.0
    if (V == 4) *reinterpret_cast<float4*>(a.out + o) = make_float4(0.f, 0.f, 0.f, 0.f);
    else a.out[o] = 0.f;
    return;
  }
  const size_t i = ((size_t)img * (size_t)a.J + (size_t)c) * (size_t)a.hw + (size_t)q * V;
  const double g0 = (double)a.grad_loss[0], g1 = (double)a.grad_loss[1], g2 = (double)a.grad_loss[2];
  Weights k;
  k.wt = g0 + a.alpha * g2;
  k.wg = g1 + (1.0 - a.alpha) * g2;
  k.pw_t = (double)a.pw_t;
  k.pw_g = (double)a.pw_g;
  if (V == 4) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 p = *reinterpret_cast<const float4*>(a.pred + o);
    const float4 g = *reinterpret_cast<const float4*>(a.gt + i);
    const float4 t = T ? *reinterpret_cast<const float4*>(a.teacher + i) : zero;
    const float4 m = M ? *reinterpret_cast<const float4*>(a.mask + i) : zero;
    float4 r;
    r.x = grad_one<T, M>(a, k, p.x, t.x, g.x, m.x);
    r.y = grad_one<T, M>(a, k, p.y, t.y, g.y, m.y);
    r.z = grad_one<T, M>(a, k, p.z, t.z, g.z, m.z);
    r.w = grad_one<T, M>(a, k, p.w, t.w, g.w, m.w);
    *reinterpret_cast<float4*>(a.out + o) = r;
  } else {
    a.out[o] = grad_one<T, M>(a, k, a.pred[o], T ? a.teacher[i] : 0.f, a.gt[i], M ? a.mask[i] : 0.f);
  }
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace
}  // namespace rtpe

using namespace rtpe;

extern "C" int rtpe_distill_loss_backward(int32_t kind, const float* pred, int32_t pred_channels, const float* teacher_n,
                                          const float* gt_n, const float* mask_eff, int32_t N, int32_t J, int32_t h,
                                          int32_t w, double alpha, float teacher_pos_weight, float gt_pos_weight,
                                          const float* grad_loss, float* grad_pred, void* stream) {
  const char* who = "distill_loss_backward";
  RTPE_REQUIRE(pred && gt_n && grad_loss && grad_pred, "%s: null pred, gt_n, grad_loss or grad_pred", who);
  RTPE_REQUIRE(N > 0 && J > 0 && h > 0 && w > 0, "%s: N = %d, J = %d, h = %d, w = %d must be positive", who, N, J, h, w);
  RTPE_REQUIRE(pred_channels >= J, "%s: pred_channels = %d is below J = %d", who, pred_channels, J);
  RTPE_REQUIRE(kind == RTPE_DISTILL_BCE || kind == RTPE_DISTILL_MSE, "%s: kind = %d is neither 0 (bce) nor 1 (mse)", who,
               kind);
  RTPE_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "%s: alpha = %g outside [0, 1]", who, alpha);
  RTPE_REQUIRE(reinterpret_cast<uintptr_t>(grad_loss) % 4 == 0, "%s: grad_loss must be 4-byte aligned", who);
  RTPE_REQUIRE((long long)N * pred_channels <= 0x7fffffffLL && (long long)N * J <= 0x7fffffffLL &&
               (long long)h * w <= 0x7fffffffLL, "%s: N * pred_channels, N * J or h * w exceeds 2^31 - 1", who);
  GradArgs a;
  a.hw = h * w;
  const bool vec = a.hw % 4 == 0 && aligned16(pred) && aligned16(teacher_n) && aligned16(gt_n) && aligned16(mask_eff) &&
                   aligned16(grad_pred);
  a.units = (long long)N * pred_channels * (vec ? a.hw / 4 : a.hw);
  const long long blocks = (a.units + kThreads - 1) / kThreads;
  RTPE_REQUIRE(blocks <= 0x7fffffffLL, "%s: %lld workgroups, at most 2^31 - 1 fit one launch", who, blocks);
  a.pred = pred; a.teacher = teacher_n; a.gt = gt_n; a.mask = mask_eff; a.grad_loss = grad_loss; a.out = grad_pred;
  a.alpha = alpha;
  a.n = (double)((long long)N * J) * (double)((long long)h * w);         // both factors exact: one rounding at most
  a.J = J; a.pred_channels = pred_channels; a.kind = kind;
  a.pw_t = teacher_pos_weight; a.pw_g = gt_pos_weight;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  using Kernel = void (*)(GradArgs);
  static const Kernel kernels[2][2][2] = {          // [four pixels][teacher][mask]
      {{distill_grad_kernel<1, false, false>, distill_grad_kernel<1, false, true>},
       {distill_grad_kernel<1, true, false>, distill_grad_kernel<1, true, true>}},
      {{distill_grad_kernel<4, false, false>, distill_grad_kernel<4, false, true>},
       {distill_grad_kernel<4, true, false>, distill_grad_kernel<4, true, true>}}};
  hipLaunchKernelGGL(kernels[vec ? 1 : 0][teacher_n ? 1 : 0][mask_eff ? 1 : 0], dim3((unsigned)blocks), dim3(kThreads), 0,
                     st, a);
  RTPE_HIP_CHECK(hipGetLastError());
  return RTPE_OK;
}
