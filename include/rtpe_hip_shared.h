/*
 * rtpe_hip_shared.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) that decodes the outputs of a dual-head student: J heat maps and
 * ONE tag map per image, shared by all joints.
 */
#ifndef RTPE_HIP_SHARED_H
#define RTPE_HIP_SHARED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Shared-tag decode: rtpe_topk_fused / rtpe_adjust_refine_fused_topk [_n] with `tg` read as one plane per image,
 * (N, 1, th, tw) f32 with image n at tg + n * tg_img_stride, instead of J planes per image.  Everything else - the
 * arguments, their order, the tables, the scratch sizes (rtpe_topk_scratch_bytes(N*J, oh, ow, K),
 * rtpe_adjust_refine_scratch_bytes), D = 1, the index encoding y * ow + x - is that of the entry without `_shared`.
 * hm and tg may point into one (N, J + 1, h, w) tensor (hm = its channel 0, tg = its channel J, both strides
 * (J + 1) * h * w): nothing is copied.
 *
 * Result: bit for bit that of the entry without `_shared` on the tag plane expanded to J equal channels,
 * F.interpolate(tag.expand(-1, J, -1, -1), (oh, ow), mode="bilinear", align_corners=True) on the CPU.  That
 * includes the small-output case oh + ow <= 128, where PyTorch's kernel sums the four products of a sample in another
 * order for the channels beyond the last full vector of 16 (for J = 17: joint 16): a sample of the shared plane taken
 * for joint j uses the order of channel j.
 *
 * Refusals (a negative code and a message, before any launch): a null pointer, a non-positive size or count,
 * J > 32, an image stride below the size of an image's planes (J * hh * hw, th * tw), and what the entries without
 * `_shared` refuse (NMS window, scratch sizes, ans_in == ans_out, a missing top-k table; P_dev null for `_n`). */
int rtpe_topk_fused_shared(const float* hm, int32_t hh, int32_t hw, int64_t hm_img_stride,
                           const float* tg, int32_t th, int32_t tw, int64_t tg_img_stride,
                           int32_t N, int32_t J, int32_t oh, int32_t ow, int32_t K,
                           int32_t nms_ksize, int32_t nms_pad,
                           float* val_k, int32_t* ind_k, float* tag_k,
                           void* scratch, size_t scratch_bytes, void* stream);
int rtpe_adjust_refine_fused_shared_topk(const float* hm, int32_t hh, int32_t hw, int64_t hm_img_stride,
                                         const float* tg, int32_t th, int32_t tw, int64_t tg_img_stride,
                                         int32_t N, int32_t J, int32_t oh, int32_t ow,
                                         const float* ans_in, float* ans_out, const int32_t* person_img, int32_t P,
                                         int32_t do_adjust, int32_t do_refine, float* scores,
                                         const float* topk_val, const int32_t* topk_ind, int32_t K,
                                         void* scratch, size_t scratch_bytes, void* stream);
int rtpe_adjust_refine_fused_shared_topk_n(const float* hm, int32_t hh, int32_t hw, int64_t hm_img_stride,
                                           const float* tg, int32_t th, int32_t tw, int64_t tg_img_stride,
                                           int32_t N, int32_t J, int32_t oh, int32_t ow,
                                           const float* ans_in, float* ans_out, const int32_t* person_img, int32_t P,
                                           int32_t do_adjust, int32_t do_refine, float* scores,
                                           const float* topk_val, const int32_t* topk_ind, int32_t K,
                                           void* scratch, size_t scratch_bytes, void* stream, const int32_t* P_dev);

#ifdef __cplusplus
}
#endif
#endif /* RTPE_HIP_SHARED_H */
