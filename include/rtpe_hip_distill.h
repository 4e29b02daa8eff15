/*
 * rtpe_hip_distill.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same conventions,
 * same error codes, rtpe_version() 4) that computes the distillation targets and the forward values of the distillation
 * losses on the device: the ground-truth Gaussian maps from a CSR people table, the targets at the students' output
 * grids (the ground-truth stamp and the teacher's two resizes fused into one pass), the normalisation and background
 * weighting of the BCE loss, and the masked BCE / MSE means in float64.  Forward values only: no gradients.
 * The rules are DESIGN.md section 4, "Distillation targets and losses".
 *
 * The people table: `offsets` (N + 1) i32, the people of image n are rows offsets[n] .. offsets[n + 1] of `joints`
 * (P_total, J, 3) f64 = (x, y, v) per joint.  Rows outside [0, P_total) are never read, whatever the offsets say.
 * The patch table of a sigma: (S, S) f32, S = ceil(6 * sigma + 3), the float32 values of
 * exp(-((x - x0)^2 + (y - y0)^2) / (2 sigma^2)), x0 = y0 = 3 sigma + 1, computed by the host in float64.
 * A resize with align_corners=False has the arithmetic of PyTorch-CPU (csrc/resize_nc.h), one with align_corners=True that
 * of the decode (csrc/decode.hip, Axis); both take PyTorch's small-output form when out_h + out_w <= 128.
 */
#ifndef RTPE_HIP_DISTILL_H
#define RTPE_HIP_DISTILL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTPE_DISTILL_CHUNK 64             /* people whose windows a workgroup holds in LDS at a time */
#define RTPE_DISTILL_MAX_PATCH 1024       /* S may not exceed this */
#define RTPE_DISTILL_MAX_BLOCKS 256       /* workgroups (= partial sums) of a loss or min/max reduction */
#define RTPE_DISTILL_SCRATCH_BYTES 16384  /* scratch of rtpe_distill_normalise and rtpe_distill_loss */
#define RTPE_DISTILL_LOSS_BYTES 40        /* f64 [teacher_loss, gt_loss, mixed], then the same three as f32, 4 bytes unused */
#define RTPE_DISTILL_BCE 0
#define RTPE_DISTILL_MSE 1

/* Ground-truth maps (N, J, H, W) f32: per pixel the maximum over the image's people of the patch value of the
 * joint's window; 0 where no window covers it.  Every element of `out` is written.  One launch. */
int rtpe_gt_heatmaps(const int32_t* offsets, const double* joints, int32_t P_total, int32_t N, int32_t J, int32_t H,
                     int32_t W, const float* patch, int32_t S, double sigma, float* out, void* stream);

/* bytes of rtpe_distill_targets' scratch: one min/max record per workgroup of its main launch */
int rtpe_distill_targets_scratch_bytes(int32_t N, int32_t J, int32_t h, int32_t w, size_t* bytes);

/* The targets of one batch of N images of size (H, W) at the detection grid (h, w) and the attention grid (ha, wa):
 *   gt_out      (N, J, h, w)   the ground-truth maps resized (H, W) -> (h, w), align_corners=False; the map at (H, W) is
 *                              never stored: each tap evaluates the stamp maximum.  Needs offsets, joints and patch.
 *   teacher_out (N, J, h, w)   `teacher` (N, J, ht, wt) resized to (H, W) with align_corners=True (a copy when the sizes
 *                              agree), then to (h, w) with align_corners=False, with the bits of the two-step chain
 *   mask_out    (N, 1, h, w)   `mask` (N, H, W) resized with align_corners=False
 *   segm_out    (N, 1, ha, wa) `segm` (N, H, W) likewise
 *   minmax      4 f32: min and max of gt_out, min and max of teacher_out (0, 0 for an absent one; NaNs are skipped)
 * Each of the four inputs may be null, with its output (ht, wt, ha, wa are then not read).  Asynchronous on `stream`. */
int rtpe_distill_targets(const int32_t* offsets, const double* joints, int32_t P_total, const float* patch, int32_t S,
                         double sigma, const float* teacher, int32_t ht, int32_t wt, const float* mask,
                         const float* segm, int32_t N, int32_t J, int32_t H, int32_t W, int32_t h, int32_t w,
                         int32_t ha, int32_t wa, float* gt_out, float* teacher_out, float* mask_out, float* segm_out,
                         float* minmax, void* scratch, size_t scratch_bytes, void* stream);

/* Steps 1 to 3 of the BCE distillation loss in float32 on (N, J, h, w) tensors:
 *   gt_out      gt, minus its minimum if that is negative, then divided by its maximum if that exceeds 1 (over the whole
 *               tensor);  teacher_out: the same for teacher (may be null with its output)
 *   mask_out    (N, J, h, w): mask, (N, mask_channels, h, w) with mask_channels 1 or J, times background_factor where
 *               gt_out == 0 (null with a null mask)
 * `minmax`: the four values of rtpe_distill_targets for these very tensors, or null: then they are computed here.
 * No input is written. */
int rtpe_distill_normalise(const float* gt, const float* teacher, const float* mask, int32_t mask_channels, int32_t N,
                           int32_t J, int32_t h, int32_t w, float background_factor, const float* minmax,
                           float* gt_out, float* teacher_out, float* mask_out, void* scratch, size_t scratch_bytes,
                           void* stream);

/* The loss values alpha * L(pred * m, teacher * m) + (1 - alpha) * L(pred * m, gt * m), L = the mean over all N*J*h*w
 * elements of BCE-with-logits (kind 0, with a pos_weight per term) or of the squared difference (kind 1); m = the
 * effective mask of rtpe_distill_normalise (no product without a mask).  `normalise` != 0 applies step 1 first.
 * `pred` is (N, pred_channels >= J, h, w), of which channels [0, J) are read.  `teacher` may be null: its loss is 0.
 * The products are float32, the elements and sums float64, summed in a fixed order (run-to-run bit-identical).
 * `loss_out`: RTPE_DISTILL_LOSS_BYTES bytes, 8-byte aligned.  gt_out / teacher_out / mask_out: as above, each may be
 * null.  Asynchronous on `stream`; nothing is read back. */
int rtpe_distill_loss(int32_t kind, int32_t normalise, const float* pred, int32_t pred_channels, const float* teacher,
                      const float* gt, const float* mask, int32_t mask_channels, int32_t N, int32_t J, int32_t h,
                      int32_t w, double alpha, float background_factor, float teacher_pos_weight, float gt_pos_weight,
                      const float* minmax, float* gt_out, float* teacher_out, float* mask_out, void* loss_out,
                      void* scratch, size_t scratch_bytes, void* stream);

/* Refusals (a negative code and a message, before any launch): a null required pointer, an output without its input or
 * an input without its output; a size <= 0; S != ceil(6 sigma + 3) or S > 1024; sigma not positive; more than 2^31 - 1
 * workgroups; mask_channels neither 1 nor J; pred_channels < J; kind not 0 or 1; alpha or background_factor outside
 * [0, 1]; scratch too small or not 8-byte aligned. */

#ifdef __cplusplus
}
#endif

#endif /* RTPE_HIP_DISTILL_H */
