/*
 * rtpe_hip_frames.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) that turns uint8 frames into the students' input canvases.
 */
#ifndef RTPE_HIP_FRAMES_H
#define RTPE_HIP_FRAMES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The students' front end: N uint8 (h_n, w_n, 3) frames of different sizes -> the fp32 NCHW canvases (N, 3, Hc, Wc)
 * that a mixed-size forward takes (rtpe_hip_mixed.h, rtpe_hip_mixed_aux.h), in ONE launch whatever N is:
 *     canvas[n, c, y, x]     = (float(f_n[y, x, c]) / 255 - mean[c]) / stdev[c]        (ToTensor, then Normalize)
 *     alt_canvas[n, :, y, x] = rgb2lab or rgb2hsv of float(f_n[y, x, :]) / 255, the bits of rtpe_rgb_to_alt
 * for y < h_n and x < w_n, and exactly 0.0 at every other element of both canvases: the kernel writes every element,
 * the canvases need no memset.  Both divisions are true fp32 divisions (what torchvision computes on the CPU).
 *
 * The jobs travel in a table in device memory of N entries of 32 bytes (rtpe_frames_table_bytes), little-endian:
 *     [ 0] uint64 source address ((h, w, 3) uint8 on the device, any alignment)
 *     [ 8] int32 h   [12] int32 w   [16] int32 row stride in bytes (>= 3 * w)   [20] int32 reserved, zero
 *     [24] 8 bytes reserved, zero
 * rtpe_frames_table_fill is a HOST function and needs no GPU: src_addr = N device addresses, src_hws = N triples
 * (h, w, stride in bytes).  It writes the table into caller-owned host memory (any alignment), which the caller then
 * copies to the device, and refuses a table_bytes below rtpe_frames_table_bytes, null addresses, h or w below 32 or
 * larger than the canvas (Hc, Wc) and stride < 3 * w.  1 <= N <= 65535.
 *
 * rtpe_frames_to_canvases launches: table_dev = the table on the device (8-byte aligned), mean / stdev = 3 floats each
 * (host), alt_mode = -1 (no second canvas: alt_canvas must be null and nothing is written for it), 0 (LAB) or 1 (HSV;
 * alt_canvas must not be null).  Null pointers, stdev <= 0, an unknown mode and an alt_canvas that does not go with
 * the mode are RTPE_E_INVALID before anything is launched.  Stream-ordered; the table, the sources and the canvases
 * must stay valid until the kernel has run.  (Hc + 3) / 4 <= 65535. */
int rtpe_frames_table_bytes(int32_t n_images, size_t* bytes);
int rtpe_frames_table_fill(const uint64_t* src_addr, const int32_t* src_hws, int32_t n_images, int32_t Hc, int32_t Wc,
                           void* table, size_t table_bytes);
int rtpe_frames_to_canvases(const void* table_dev, int32_t n_images, int32_t Hc, int32_t Wc, const float* mean,
                            const float* stdev, int32_t alt_mode, void* canvas, void* alt_canvas, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RTPE_HIP_FRAMES_H */
