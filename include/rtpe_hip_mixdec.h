/*
 * rtpe_hip_mixdec.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) that decodes a mixed-size batch of a dual-head student in one pass,
 * straight from the output canvas of its one forward (rtpe_hip_mixed.h).
 */
#ifndef RTPE_HIP_MIXDEC_H
#define RTPE_HIP_MIXDEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Mixed-size decode: the per-image decode size of rtpe_hip_sizes.h and the shared tag plane of rtpe_hip_shared.h at
 * once, on maps that are REGIONS of larger planes.  hm is (N, J, hh, hw) f32 at hm_img_stride and tg ONE plane per
 * image, (N, 1, th, tw) f32 at tg_img_stride - possibly channels 0 and J of one (N, J + 1, Hc, Wc) canvas, nothing
 * is copied.  Image n's maps are the top-left (heat_h_n, heat_w_n) / (tag_h_n, tag_w_n) elements of its planes and it
 * is decoded at (oh_n, ow_n).  The decode therefore knows two extents per axis:
 *     the pitch    (hh, hw) / (th, tw): rows of hw / tw elements, planes of hh * hw / th * tw.  It only ADDRESSES.
 *     the extent   of image n, which only CLAMPS: the n_in of the axes of its table entry.  No tap lies outside it, so
 *                  whatever the planes hold outside an image's region (other values, NaN) is never part of a sample.
 * Result, per image: bit for bit that of the `_shared` entries on a contiguous copy of the image's region at its own
 * size - rtpe_topk_fused_shared(region_hm, heat_h_n, heat_w_n, ..., region_tg, tag_h_n, tag_w_n, ..., 1, J, oh_n,
 * ow_n, ...) - with the indices re-encoded as in rtpe_hip_sizes.h.
 *
 * The table is that of rtpe_hip_sizes.h, 64 bytes per image, same layout.  rtpe_decode_mixed_fill (a HOST function)
 * writes it: out_hw = N pairs (oh_n, ow_n), heat_hw / tag_hw = N pairs of extents (tag_hw NULL: the tag extents are
 * the heat extents), (hh, hw) / (th, tw) the pitch.  Entry n gets the axes of (heat_hw[n] -> out_hw[n]) and
 * (tag_hw[n] -> out_hw[n]) and small = (oh_n + ow_n <= 128).  Where every extent equals its pitch the table is byte
 * for byte that of rtpe_decode_sizes_fill.  It refuses (RTPE_E_INVALID and a message, nothing written): a null
 * pointer, a non-positive size, extent or pitch, an extent above its pitch, a table below 64 * N bytes - a wrong
 * table would make the device read outside the planes.
 *
 * The entries take the arguments of the `_sizes` entries with (hh, hw, th, tw) read as the pitch and `tg` as one
 * plane per image.  The scratch sizes, max_oh / max_ow (the caller's promise), w_enc and the index encoding
 * y * w_enc + x are those of rtpe_hip_sizes.h.  Refusals before any launch: those of the `_sizes` and the `_shared`
 * entries together - a null pointer, a non-positive size or count, J > 32, an image stride below J * hh * hw /
 * th * tw, a table below 64 * N bytes, w_enc < max_ow or max_oh * w_enc > INT32_MAX, the NMS window, the scratch
 * sizes, ans_in == ans_out, a missing top-k table; P_dev null for `_n`. */
int rtpe_decode_mixed_fill(const int32_t* out_hw, const int32_t* heat_hw, const int32_t* tag_hw, int32_t N,
                           int32_t hh, int32_t hw, int32_t th, int32_t tw, void* table, size_t table_bytes,
                           int32_t* max_oh, int32_t* max_ow);
int rtpe_topk_fused_mixed(const float* hm, int32_t hh, int32_t hw, int64_t hm_img_stride,
                          const float* tg, int32_t th, int32_t tw, int64_t tg_img_stride,
                          int32_t N, int32_t J, const void* sizes_table, size_t table_bytes,
                          int32_t max_oh, int32_t max_ow, int32_t w_enc, int32_t K,
                          int32_t nms_ksize, int32_t nms_pad,
                          float* val_k, int32_t* ind_k, float* tag_k,
                          void* scratch, size_t scratch_bytes, void* stream);
int rtpe_adjust_refine_fused_mixed_topk(const float* hm, int32_t hh, int32_t hw, int64_t hm_img_stride,
                                        const float* tg, int32_t th, int32_t tw, int64_t tg_img_stride,
                                        int32_t N, int32_t J, const void* sizes_table, size_t table_bytes,
                                        int32_t max_oh, int32_t max_ow, int32_t w_enc,
                                        const float* ans_in, float* ans_out, const int32_t* person_img, int32_t P,
                                        int32_t do_adjust, int32_t do_refine, float* scores,
                                        const float* topk_val, const int32_t* topk_ind, int32_t K,
                                        void* scratch, size_t scratch_bytes, void* stream);
int rtpe_adjust_refine_fused_mixed_topk_n(const float* hm, int32_t hh, int32_t hw, int64_t hm_img_stride,
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
#endif /* RTPE_HIP_MIXDEC_H */
