/*
 * rtpe_hip_anysize.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) that lets a program run on inputs whose sides are not multiples
 * of 32: the students (rtpe/students.py), which the reference feeds native COCO images (427 x 640, 640 x 480, ...).
 *
 * Extent rule.  A tensor with rtpe_tensor_desc::ds_log2 = d holds rtpe_extent(H, d) x rtpe_extent(W, d) pixels:
 *     rtpe_extent(n, d) = n >> d                       when n is a multiple of 32 (as before),
 *                         (n + (1 << d) - 1) >> d      otherwise: ceil(n / 2^d), what a chain of d stride-2 convs with
 *                                                      padding k / 2 or of AvgPool2d(3, 2, 1) leaves.
 * The two branches agree for d <= 5; the first one keeps a 32-wide input at d = 6 a tensor without pixels.
 *
 * A program takes such sizes only after rtpe_hrnet_set_any_size(h, 1); the teacher's four branches cannot be fused
 * at other sizes, so its handle never gets the property.  With it, a forward of a ragged shape (a side that is no
 * multiple of 32; both sides >= 32)
 *   - runs every conv on the one-workgroup-per-tile kernel and the stem on the VALU kernel (the general paths; no fused,
 *     persistent, direct or streaming launch, no plane-major tensor),
 *   - reads the up-sampled terms of a RTPE_OP_FUSE op with PyTorch-CPU's nearest rule for a given size,
 *         src = min((int)floorf(dst * scale), in - 1),   scale = (float)in / (float)out   per axis
 *     (the shift dst >> up is that rule only where out == in << up),
 *   - uses the default launch shapes: rtpe_hrnet_autotune [_aux] and rtpe_hrnet_import_tuned refuse ragged shapes.
 * Refused before the first launch (RTPE_E_INVALID): a ragged shape on a handle without the property; on a handle with
 * it, a program that holds a transposed conv, a fused BasicBlock pair or a group of stride-2 convs in one launch.
 * Shapes whose sides are both multiples of 32 run exactly as without the property.
 */
#ifndef RTPE_HIP_ANYSIZE_H
#define RTPE_HIP_ANYSIZE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* host only: pixels along a side of n input pixels of a tensor at 1 / 2^ds_log2 (0 for a bad argument) */
int32_t rtpe_extent(int32_t n, int32_t ds_log2);
/* host only: the index rule of the nearest-to-size sampler (-1 for a bad argument) */
int32_t rtpe_nearest_src(int32_t dst, int32_t n_in, int32_t n_out);
int rtpe_hrnet_set_any_size(rtpe_hrnet* h, int32_t on);
int rtpe_hrnet_get_any_size(const rtpe_hrnet* h, int32_t* on);

#ifdef __cplusplus
}
#endif
#endif /* RTPE_HIP_ANYSIZE_H */
