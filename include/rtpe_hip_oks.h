/*
 * rtpe_hip_oks.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same conventions,
 * same error codes, rtpe_version() 4) that scores the keypoint records on the device: COCO keypoint evaluation
 * (OKS between detections and annotations, greedy matching per threshold and area range) of every record in one
 * launch, one 64-lane workgroup per record.  The precision / recall accumulation over the compact result table is
 * the host's (rtpe/scoring.py).  The rules are DESIGN.md section 4, "Scoring".
 */
#ifndef RTPE_HIP_OKS_H
#define RTPE_HIP_OKS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTPE_OKS_GT_ROW 64       /* doubles per annotation row */
#define RTPE_OKS_MAX_DETS 64     /* max_dets may not exceed this (one lane per kept detection) */
#define RTPE_OKS_MAX_RANGES 16   /* nor n_rng this (one bit per range in an annotation's flag word) */
#define RTPE_OKS_LDS_DOUBLES 512 /* the OKS matrix of a record sits in LDS while max_dets * G <= this (4 KiB) */

/* Sizes of the two buffers of rtpe_oks_eval for n_records records and an annotation table of gt_total rows:
 *   result row = [i32 image_id, i32 n_dt, f32 scores[max_dets], u8 matched[n_thr][n_rng][max_dets],
 *                 u8 ignored[n_thr][n_rng][max_dets], zero bytes up to a multiple of 8]
 *   result_bytes  = n_records * row bytes                         ((10, 3, 20) -> rows of 1288 bytes)
 *   scratch_bytes = max(gt_total, 1) * (max_dets * 8 + 4 + n_thr * n_rng), rounded up to a multiple of 8
 * (the result row depends on the three counts, so they are arguments here too). */
int rtpe_oks_eval_bytes(int32_t n_records, int32_t gt_total, int32_t n_thr, int32_t n_rng, int32_t max_dets,
                        size_t* result_bytes, size_t* scratch_bytes);

/* Score every record against its image's annotations.  One launch, asynchronous on `stream`; all pointers are
 * device-addressable.
 *   rec          (n_records, 2 + max_people + max_people * J * 4) f32: [image_id, n_people, scores, kpts[.][J][4]]
 *   gt_image_ids (n_gt_images) i32, ASCENDING - a precondition: the table is device memory and is not read back;
 *                the kernel finds a record's image by binary search, an id without an entry has no annotations
 *   gt_offsets   (n_gt_images + 1) i32: the rows of image k are gt_rows[gt_offsets[k] : gt_offsets[k + 1]]
 *   gt_rows      (gt_total, 64) f64: 17 x (x, y, v), bbox x, y, w, h at 51..54, area at 55, iscrowd at 56,
 *                num_keypoints at 57, padding
 *   sigmas       (J) f64: the per-joint constants; vars = (2 * sigmas)^2 is formed on the device
 *   thresholds   (n_thr) f64;  area_ranges (n_rng, 2) f64, bounds inclusive
 *   result       n_records rows as above; EVERY byte of every row is written, the buffer needs no clearing
 *   scratch      per annotation row: the OKS column block, a flag word, the matched flags of the cells.  The number
 *                of annotation rows it holds is scratch_bytes / (max_dets * 8 + 4 + n_thr * n_rng); images whose
 *                rows end beyond that are scored as without annotations.  After the call the first part of scratch
 *                holds, for a record whose image has G rows from CSR offset o, its OKS matrix (n_dt, G) f64
 *                row-major at double index o * max_dets (detections in score order) - whether the kernel kept the
 *                matrix in LDS (max_dets * G <= 512) or worked in scratch.  Two records of one image id share
 *                that block: the host refuses such a table on the read-back (rtpe/scoring.py).
 * Per record: the people are ranked by descending score, stably, and cut to n_dt = min(n_people, max_dets).
 *
 * Refusals (a negative code and a message, before any launch): a null pointer; n_records, J, max_people,
 * n_gt_images, n_thr, n_rng or max_dets <= 0; max_dets > max_people or > 64; n_rng > 16; result_bytes or
 * scratch_bytes below rtpe_oks_eval_bytes(n_records, 0, ...).  `sigmas` must hold J entries for any J (17 for COCO). */
int rtpe_oks_eval(const float* rec, int32_t n_records, int32_t J, int32_t max_people, const int32_t* gt_image_ids,
                  const int32_t* gt_offsets, const double* gt_rows, int32_t n_gt_images, const double* sigmas,
                  const double* thresholds, int32_t n_thr, const double* area_ranges, int32_t n_rng,
                  int32_t max_dets, void* result, size_t result_bytes, void* scratch, size_t scratch_bytes,
                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RTPE_HIP_OKS_H */
