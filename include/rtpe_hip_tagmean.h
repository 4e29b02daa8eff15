/*
 * rtpe_hip_tagmean.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) of the averaged-tag test: every joint of an image is grouped by
 * ONE tag map, the mean of the J un-mirrored tag maps of the smallest scale (the reference's
 * legacy/valid_ae_avg.py:189-195, `tags[0].mean(dim=1)`).
 *
 * The mean's float order is part of the contract - PyTorch-CPU's mean(dim=1) of a contiguous float32 tensor:
 * channels in blocks of 16, each block summed channel after channel from +0.0f, the block sums added in order, the
 * C % 16 channels behind the last full block summed from +0.0f on their own and added last, then one true fp32
 * division by float(C).  ATen itself uses another order for the last (h * w) % 32 pixels of a plane; these entries use
 * the order above for every pixel.  The order is ATen's for C <= 272 (17 blocks of 16); from C = 273 on ATen groups
 * the block sums at one more level, which is not pinned here, so rtpe_channel_mean refuses C > 272 (the decode entries
 * have J <= 32).
 */
#ifndef RTPE_HIP_TAGMEAN_H
#define RTPE_HIP_TAGMEAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out (N, h, w) f32 dense = mean over the C channels of x (N, C, h, w) f32 in the order above.  Planes are dense
 * (h * w floats); channel c of image n starts at x + n * img_stride + c * ch_stride (in floats), so a channel slice of
 * a larger tensor is passed as it is.  Refusals: a null pointer, N outside 1..65535, C outside 1..272, a non-positive
 * size, ch_stride < h * w, img_stride < (C - 1) * ch_stride + h * w. */
int rtpe_channel_mean(const float* x, int32_t N, int32_t C, int32_t h, int32_t w, int64_t img_stride,
                      int64_t ch_stride, float* out, void* stream);

/* The multi-scale (and flip) test with the averaged tag.  The entries mirror rtpe_ms_ags_maps_bytes / rtpe_ms_ags_prep
 * / rtpe_topk_ms_ags / rtpe_adjust_refine_ms_ags [_n] of rtpe_hip.h - the same arguments in the same order, the same
 * tables and scratch sizes, D = 1, people rows (P, J, 4) - except that the maps buffer also depends on the decode size,
 * so rtpe_ms_mean_maps_bytes and rtpe_ms_mean_prep take (oh, ow) too (before `bytes` / before `maps`).
 *
 * The maps buffer, in floats: per scale i (descending) A_o^i then, with flip, A_f^i, (N*J, h2_i, w2_i) each, as ever;
 * then T, the J un-mirrored tag maps of the smallest scale L = S-1 at its refined size, (N*J, h2_L, w2_L); then M, the
 * shared tag planes at the decode size, (N, oh, ow):
 *     T[n*J + j] = rs_(h2_L,w2_L)(P_L[n, J + j])         M[n] = mean_j rs_(oh,ow)(T[n*J + j])
 * rs = F.interpolate(bilinear, align_corners=False), a copy where the sizes agree.  The mirror image's outputs are
 * not read for the tag.
 *
 * rtpe_ms_mean_prep with scale == S-1 launches two kernels: the prep of that scale, which also writes T for images
 * n0..n0+n-1, and behind it the kernel that writes M for those images.  For every other scale it is rtpe_ms_ags_prep.
 * rtpe_topk_ms_mean and rtpe_adjust_refine_ms_mean [_n] read M as a shared plane whose size is the decode size (the
 * kernels of the `_ags` entries, sampling an identity).  Result per image: bit for bit
 * parser.parse(F, M[None, ..., None], adjust, refine) with tag_per_joint = False.
 *
 * Refusals (a negative code and a message, before any launch): what the `_ags` entries refuse, a non-positive decode
 * size, oh * ow >= 2^31, a maps buffer smaller than rtpe_ms_mean_maps_bytes says. */
int rtpe_ms_mean_maps_bytes(int32_t N, int32_t J, int32_t S, const int32_t* h2, const int32_t* w2, int32_t base,
                            int32_t flip, int32_t oh, int32_t ow, size_t* bytes);
int rtpe_ms_mean_prep(const float* preds, int32_t h4, int32_t w4, int64_t preds_img_stride,
                      const float* refined, int64_t refined_img_stride, const float* preds_f,
                      int64_t preds_f_img_stride, const float* refined_f, int64_t refined_f_img_stride,
                      int32_t n0, int32_t n, int32_t N, int32_t J, const int32_t* flip_index, int32_t S,
                      const int32_t* h2, const int32_t* w2, int32_t base, int32_t flip, int32_t scale,
                      int32_t oh, int32_t ow, float* maps, size_t maps_bytes, void* stream);
int rtpe_topk_ms_mean(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                      const int32_t* w2, int32_t base, int32_t flip, int32_t oh, int32_t ow, int32_t K,
                      int32_t nms_ksize, int32_t nms_pad, float* val_k, int32_t* ind_k, float* tag_k,
                      size_t maps_bytes, void* scratch, size_t scratch_bytes, void* stream);
int rtpe_adjust_refine_ms_mean(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                               const int32_t* w2, int32_t base, int32_t flip, int32_t oh, int32_t ow,
                               size_t maps_bytes, const float* ans_in, float* ans_out,
                               const int32_t* person_img, int32_t P, int32_t do_adjust, int32_t do_refine,
                               float* scores, const float* topk_val, const int32_t* topk_ind, int32_t K,
                               void* scratch, size_t scratch_bytes, void* stream);
int rtpe_adjust_refine_ms_mean_n(const float* maps, int32_t N, int32_t J, int32_t S, const int32_t* h2,
                                 const int32_t* w2, int32_t base, int32_t flip, int32_t oh, int32_t ow,
                                 size_t maps_bytes, const float* ans_in, float* ans_out,
                                 const int32_t* person_img, int32_t P, int32_t do_adjust, int32_t do_refine,
                                 float* scores, const float* topk_val, const int32_t* topk_ind, int32_t K,
                                 void* scratch, size_t scratch_bytes, void* stream, const int32_t* P_dev);

#ifdef __cplusplus
}
#endif
#endif /* RTPE_HIP_TAGMEAN_H */
