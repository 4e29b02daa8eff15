/*
 * rtpe_hip_distill_grad.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) that computes the gradient of the distillation losses of
 * rtpe_hip_distill.h with respect to the student's output.  The rules are DESIGN.md section 4, "Distillation losses:
 * backward".
 */
#ifndef RTPE_HIP_DISTILL_GRAD_H
#define RTPE_HIP_DISTILL_GRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* grad_pred (N, pred_channels, h, w) f32: the gradient of
 *     grad_loss[0] * teacher_loss + grad_loss[1] * gt_loss + grad_loss[2] * (alpha teacher_loss + (1 - alpha) gt_loss)
 * of rtpe_distill_loss with respect to `pred` (N, pred_channels >= J, h, w).  `kind`: RTPE_DISTILL_BCE or RTPE_DISTILL_MSE.
 * `teacher_n`, `gt_n`, `mask_eff` (N, J, h, w) f32 are the KEPT outputs of the forward (teacher_out, gt_out, mask_out of
 * rtpe_distill_loss): the normalised targets and the effective mask.  `teacher_n` null: the teacher's term is absent.
 * `mask_eff` null: m = 1 and there are no products.  `grad_loss`: 3 f32 in DEVICE memory, read by the kernel; the host
 * reads nothing and waits for nothing.  EVERY element of grad_pred is written: channels >= J and elements with m == 0
 * get +0.0 (stored, not computed), so the caller needs no memset.  One launch, asynchronous on `stream`.
 *
 * Per element, n = N * J * h * w, float32 up to the three products and float64 from there, each line one IEEE
 * operation per operator, evaluated exactly as bracketed (the file is compiled without contraction):
 *     x  = (double)(float)(pred * m)      yt = (double)(float)(teacher_n * m)      yg = (double)(float)(gt_n * m)
 *     wt = (double)grad_loss[0] + alpha * (double)grad_loss[2]
 *     wg = (double)grad_loss[1] + (1.0 - alpha) * (double)grad_loss[2]
 *   MSE:
 *     tt = (wt * 2.0) * (x - yt)          tg = (wg * 2.0) * (x - yg)
 *     v  = ((tt + tg) * m) / n            (without a teacher: v = (tg * m) / n)
 *   BCE with logits:
 *     e  = exp(-fabs(x))     d = 1.0 + e     s = x >= 0 ? 1.0 / d : e / d
 *     qt = pw_t * yt         qg = pw_g * yg            (pw_t, pw_g: the float pos_weights widened)
 *     a  = wt * ((1.0 - yt) + qt) + wg * ((1.0 - yg) + qg)         b = wt * qt + wg * qg
 *          (without a teacher: a = wg * ((1.0 - yg) + qg), b = wg * qg)
 *     v  = (((a * s) - b) * m) / n
 *   grad_pred = (float)v, one rounding.
 * A thread handles four consecutive pixels of one plane with 16-byte loads and stores when h * w is a multiple of 4 and
 * pred, teacher_n, gt_n, mask_eff and grad_pred are all 16-byte aligned (a null pointer counts as aligned), and one
 * pixel otherwise; both forms give the same bits.
 *
 * Refusals (a negative code and a message, before any launch): a null pred, gt_n, grad_loss or grad_pred; a size <= 0;
 * pred_channels < J; kind not 0 or 1; alpha outside [0, 1] or NaN; grad_loss not 4-byte aligned; N * pred_channels,
 * N * J or h * w beyond 2^31 - 1; more than 2^31 - 1 workgroups. */
int rtpe_distill_loss_backward(int32_t kind, const float* pred, int32_t pred_channels, const float* teacher_n,
                               const float* gt_n, const float* mask_eff, int32_t N, int32_t J, int32_t h, int32_t w,
                               double alpha, float teacher_pos_weight, float gt_pos_weight, const float* grad_loss,
                               float* grad_pred, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RTPE_HIP_DISTILL_GRAD_H */
