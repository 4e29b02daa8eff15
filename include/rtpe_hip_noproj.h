/*
 * rtpe_hip_noproj.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) of the multi-scale (and flip) test WITHOUT projection to the image:
 * the upstream TEST.PROJECT2IMAGE = False branch of get_multi_stage_outputs / aggregate_results, i.e.
 * rtpe/inference.py multi_scale_inference(..., project2image=False), for a whole batch.
 *
 * The scales come in the loop order (descending); r_i = (h2[i], w2[i]) is the refined size of scale i, `base` the
 * index of scale 1.  The decode grid is r_0 - it is not an argument.  rs = F.interpolate(bilinear,
 * align_corners=False), a copy where the sizes agree.  Per image and joint:
 *     H_i = (A_o^i + A_f^i) / 2 with flip, A_o^i without, formed AT r_i (A_o, A_f: as for rtpe_ms_prep)
 *     F   = H_0;  F = F + rs_(r_i -> r_0)(H_i) for i = 1, 2, ... in that order;  F = F / S (a true division) if S > 1
 *     T   = [T_o, T_f] of the scale-1 entry (D = 1 + flip), resized r_base -> r_0 unless base == 0
 * and the result is bit for bit parser.parse(F, T, adjust, refine) on the r_0 grid: people rows (P, J, 4 + flip).
 *
 * The maps buffer, in floats, with P = N * J:
 *     F (P, h2_0, w2_0) | T_o (P, h2_b, w2_b) [| T_f (P, h2_b, w2_b)] | H_1 (P, h2_1, w2_1) | ... | H_{S-1}
 *     bytes = 4 * P * (h2_0 * w2_0 + (1 + flip) * h2_b * w2_b + sum_{i >= 1} h2_i * w2_i)
 * F is summed in place: rtpe_ms_np_prep of scale 0 writes H_0 into F; of a later scale it writes H_i and launches,
 * behind it, F += rs(H_i), with the / S on the last scale.  So for every image the preps must be enqueued in scale
 * order on ONE stream (sub-batches of different scales may interleave as long as that holds), each scale once.  The
 * tags stay at r_base: the decode takes the four taps of rs_(r_base -> r_0) where it reads one (the arithmetic of
 * aggregate_results' resize), an integer-pixel copy when base == 0.  Nothing of the input size is ever written.
 *
 * Refusals (a negative code and a message, before any launch): a null pointer, a non-positive size, S outside 1..4,
 * base outside 0..S-1 (scale 1 missing), J outside 1..32, more than 65535 planes, a maps buffer smaller than
 * rtpe_ms_np_maps_bytes says, a sub-batch beyond N, and what rtpe_ms_prep / rtpe_topk_ms / rtpe_adjust_refine_ms
 * refuse of their other arguments.
 */
#ifndef RTPE_HIP_NOPROJ_H
#define RTPE_HIP_NOPROJ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* host only: no GPU is touched */
int rtpe_ms_np_maps_bytes(int32_t N, int32_t J, int32_t S, const int32_t* h2, const int32_t* w2, int32_t base,
                          int32_t flip, size_t* bytes);
/* one scale, images n0..n0+n-1 of the batch of N: the arguments of rtpe_ms_prep */
int rtpe_ms_np_prep(const float* preds, int32_t h4, int32_t w4, int64_t preds_img_stride, const float* refined,
                    int64_t refined_img_stride, const float* preds_f, int64_t preds_f_img_stride,
                    const float* refined_f, int64_t refined_f_img_stride, int32_t n0, int32_t n, int32_t N,
                    int32_t J, const int32_t* flip_index, int32_t S, const int32_t* h2, const int32_t* w2,
                    int32_t base, int32_t flip, int32_t scale, float* maps, size_t maps_bytes, void* stream);
/* the arguments of rtpe_topk_ms / rtpe_adjust_refine_ms [_n] without (oh, ow); flat indices are y * w2[0] + x */
int rtpe_topk_ms_np(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2, const int32_t* w2,
                    int32_t base, int32_t flip, int32_t K, int32_t nms_ksize, int32_t nms_pad, float* val_k,
                    int32_t* ind_k, float* tag_k, size_t maps_bytes, void* scratch, size_t scratch_bytes,
                    void* stream);
int rtpe_adjust_refine_ms_np(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                             const int32_t* w2, int32_t base, int32_t flip, size_t maps_bytes, const float* ans_in,
                             float* ans_out, const int32_t* person_img, int32_t P, int32_t do_adjust,
                             int32_t do_refine, float* scores, const float* topk_val, const int32_t* topk_ind,
                             int32_t K, void* scratch, size_t scratch_bytes, void* stream);
int rtpe_adjust_refine_ms_np_n(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                               const int32_t* w2, int32_t base, int32_t flip, size_t maps_bytes, const float* ans_in,
                               float* ans_out, const int32_t* person_img, int32_t P, int32_t do_adjust,
                               int32_t do_refine, float* scores, const float* topk_val, const int32_t* topk_ind,
                               int32_t K, void* scratch, size_t scratch_bytes, void* stream, const int32_t* P_dev);

#ifdef __cplusplus
}
#endif
#endif /* RTPE_HIP_NOPROJ_H */
