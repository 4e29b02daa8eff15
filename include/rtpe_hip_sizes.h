/*
 * rtpe_hip_sizes.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) that decodes every image of a batch at its own size.
 */
#ifndef RTPE_HIP_SIZES_H
#define RTPE_HIP_SIZES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-image decode size: rtpe_topk_fused / rtpe_adjust_refine_fused_topk [_n] for a batch whose image n is decoded
 * at its own (oh_n, ow_n) - bit for bit what the one-size entries give for that image alone at (oh_n, ow_n).  Any
 * positive sizes, larger than, equal to or smaller than the maps, in any mix.
 *
 * The sizes travel in a table of N entries of 64 bytes (rtpe_decode_sizes_bytes(N) = 64 * N), 16 little-endian
 * 32-bit words each:
 *     [0] oh  [1] ow                                   int32
 *     [2..4] heat map rows  [5..7] heat map columns    one axis = { float32 scale; int32 n_in; int32 same }
 *     [8..10] tag map rows  [11..13] tag map columns
 *     [14] small = (oh + ow <= 128)   [15] reserved, zero
 * with n_in the map's extent along the axis, same = (n_in == n_out) - the axis is then copied - and
 * scale = float32(n_in - 1) / float32(n_out - 1), 0 when n_out == 1: F.interpolate(align_corners=True)'s scale.
 * small: PyTorch's CPU op resizes an output of oh + ow <= 128 with another kernel (the weights multiplied first, four
 * products summed); the samplers then use that kernel's arithmetic, as rtpe_topk_fused and rtpe_adjust_refine_fused*
 * do for such an (oh, ow).
 * rtpe_decode_sizes_fill is a HOST function: sizes_hw = N pairs (oh_n, ow_n) of host ints, (hh, hw) / (th, tw) the
 * sizes of the heat and tag maps; it writes the table into caller-owned host memory (pinned memory that the device
 * addresses, or pageable memory the caller then copies to the device) and, where not NULL, the largest height and
 * the largest width of the batch.  The entries below read the table on the device only (`sizes_table`:
 * device-visible, table_bytes >= 64 * N), so they take those two maxima as arguments: max_oh >= every oh_n and
 * max_ow >= every ow_n is the caller's promise - they size the one tile grid of the batch (an image's tiles beyond
 * its own size stay empty).  The top-k scratch is rtpe_topk_scratch_bytes(N*J, max_oh, max_ow, K).
 *
 * Index encoding: every flat pixel index that these entries write or read - ind_k, topk_ind, and with them the `w`
 * the matchers are called with (rtpe_match_by_tag_batch / rtpe_match_by_tag_dev) - is y * w_enc + x with the ONE
 * width w_enc of the call, max_ow <= w_enc, max_oh * w_enc <= INT32_MAX, the same value in all three entries.  For
 * x < ow_n <= w_enc the indices of an image keep the order of its own row-major pixels, so ties and the zero padding
 * of the top-k fall as in the one-size call; people rows are in the pixel coordinates of the image's own size. */
int rtpe_decode_sizes_bytes(int32_t N, size_t* bytes);
int rtpe_decode_sizes_fill(const int32_t* sizes_hw, int32_t N, int32_t hh, int32_t hw, int32_t th, int32_t tw,
                           void* table, size_t table_bytes, int32_t* max_oh, int32_t* max_ow);
int rtpe_topk_fused_sizes(const float* hm, int32_t hh, int32_t hw, int64_t hm_img_stride,
                          const float* tg, int32_t th, int32_t tw, int64_t tg_img_stride,
                          int32_t N, int32_t J, const void* sizes_table, size_t table_bytes,
                          int32_t max_oh, int32_t max_ow, int32_t w_enc, int32_t K,
                          int32_t nms_ksize, int32_t nms_pad,
                          float* val_k, int32_t* ind_k, float* tag_k,
                          void* scratch, size_t scratch_bytes, void* stream);
int rtpe_adjust_refine_fused_topk_sizes(const float* hm, int32_t hh, int32_t hw, int64_t hm_img_stride,
                                        const float* tg, int32_t th, int32_t tw, int64_t tg_img_stride,
                                        int32_t N, int32_t J, const void* sizes_table, size_t table_bytes,
                                        int32_t max_oh, int32_t max_ow, int32_t w_enc,
                                        const float* ans_in, float* ans_out, const int32_t* person_img, int32_t P,
                                        int32_t do_adjust, int32_t do_refine, float* scores,
                                        const float* topk_val, const int32_t* topk_ind, int32_t K,
                                        void* scratch, size_t scratch_bytes, void* stream);
int rtpe_adjust_refine_fused_topk_sizes_n(const float* hm, int32_t hh, int32_t hw, int64_t hm_img_stride,
                                          const float* tg, int32_t th, int32_t tw, int64_t tg_img_stride,
                                          int32_t N, int32_t J, const void* sizes_table, size_t table_bytes,
                                          int32_t max_oh, int32_t max_ow, int32_t w_enc,
                                          const float* ans_in, float* ans_out, const int32_t* person_img, int32_t P,
                                          int32_t do_adjust, int32_t do_refine, float* scores,
                                          const float* topk_val, const int32_t* topk_ind, int32_t K,
                                          void* scratch, size_t scratch_bytes, void* stream, const int32_t* P_dev);

#ifdef __cplusplus
}
#endif
#endif /* RTPE_HIP_SIZES_H */
