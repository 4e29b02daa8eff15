/*
 * rtpe_hip_records.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) that writes the fixed-size keypoint records of the all-gather on
 * the device, behind adjust + refine, from the rows as they lie there.
 */
#ifndef RTPE_HIP_RECORDS_H
#define RTPE_HIP_RECORDS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The record of one image: [image_id, n_people, scores[max_people], kpts[max_people][J][4]] as float32,
 * 2 + max_people + max_people * J * 4 floats ((17, 30) -> 2072 floats, 8288 bytes). */
int rtpe_records_floats(int32_t J, int32_t max_people, size_t* floats);

/* One record per image from the people of a whole batch, one workgroup per image, asynchronous on `stream`.
 *   rows      (cap, J, C) f32, C = 3 + D >= 4: the rows as adjust + refine write them, image after image
 *   scores    (cap) f32
 *   counts    (N) i32: people per image, image order; the rows of image n start at o = sum(counts[:n])
 *   image_ids (N) i32 (a float32 holds them exactly up to 2^24)
 *   xform     NULL, or (N, 6) f64: per image a row-major 2x3 matrix t
 *   rec       (N, rtpe_records_floats(J, max_people)) f32, rec_bytes its size
 * All pointers are device-addressable (device memory, or pinned host memory that the device reads in place).
 *
 * With n = min(counts[image], max_people):
 *   rec[image] = [float(image_ids[image]), float(n), scores[o:o+n], 0.., rows[o:o+n, :, 0:4] flattened, 0..]
 * EVERY float of every record is written (the zeros included: the buffer needs no clearing), with vector stores;
 * columns beyond the fourth are dropped; rows and scores at and beyond sum(counts) are never read (nor any beyond cap).
 *
 * With xform, columns 0 and 1 of every row (x, y) of the image become
 *   x' = (float)((t[0] * (double)x + t[1] * (double)y) + t[2]),   y' = (float)((t[3] * (double)x + t[4] * (double)y) + t[5])
 * in float64, in exactly this order - two products, the left addition, the right one, ONE rounding to float32, no
 * fused multiply-add: numpy's `t[:, 0] * pt[0] + t[:, 1] * pt[1] + t[:, 2]` of a float64 matrix and a float32 point,
 * assigned to a float32 row.  Every joint of a row is transformed, those with value 0 too.
 *
 * Refusals (a negative code and a message, before any launch): rows, scores, counts, image_ids or rec null; N, J, cap
 * or max_people <= 0; C < 4; rec_bytes below N records. */
int rtpe_pack_records(const float* rows, int32_t C, const float* scores, const int32_t* counts,
                      const int32_t* image_ids, const double* xform, int32_t N, int32_t J, int32_t cap,
                      int32_t max_people, float* rec, size_t rec_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RTPE_HIP_RECORDS_H */
