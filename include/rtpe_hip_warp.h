/*
 * rtpe_hip_warp.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) that warps a whole chunk of images at every test scale.
 */
#ifndef RTPE_HIP_WARP_H
#define RTPE_HIP_WARP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Batched pre-processing: rtpe_warp_normalize for N source images of different (h, w, stride) at S scales, written
 * straight into the S tensors (N, 3, H_s, W_s) fp32 of the chunk - one launch per scale, whatever N is, bit for bit
 * what rtpe_warp_normalize gives for image n alone with the same matrix (both kernels call one device function).
 *
 * The jobs travel in a table in device memory of S * N entries of 64 bytes (rtpe_warp_batch_table_bytes), the entry
 * of (scale s, image n) at index s * N + n, little-endian:
 *     [ 0] uint64 source address ((h, w, 3) uint8 on the device)
 *     [ 8] int32 h   [12] int32 w   [16] int32 row stride in bytes   [20] reserved, zero
 *     [24] float32 m[6], destination -> source: sx = m0*x + m1*y + m2, sy = m3*x + m4*y + m5
 *     [48] uint64 destination address: the (3, H_s, W_s) fp32 planes of image n in the tensor of scale s
 *     [56] reserved, zero
 * rtpe_warp_batch_table_fill is a HOST function and needs no GPU: src_addr = N device addresses, src_hws = N triples
 * (h, w, stride in bytes), matrices = S * N * 6 floats in the order of the table, dst_base = S device addresses of
 * contiguous (N, 3, H_s, W_s) fp32 tensors, sizes = S pairs (H_s, W_s).  It writes the table into caller-owned host
 * memory (any alignment), which the caller then copies to the device, and refuses a table_bytes below
 * rtpe_warp_batch_table_bytes, null addresses, non-positive sizes and stride < 3 * w.  1 <= N <= 65535, 1 <= S <= 16.
 *
 * rtpe_warp_normalize_batch launches: table_dev = the table on the device (8-byte aligned), sizes = the same S pairs
 * (host ints), mean / stdev / round_u8 as rtpe_warp_normalize (null pointers and stdev <= 0 refused).  Stream-ordered;
 * the table, the sources and the destinations must stay valid until the kernels have run.  Any H_s, W_s >= 1. */
int rtpe_warp_batch_table_bytes(int32_t n_images, int32_t n_scales, size_t* bytes);
int rtpe_warp_batch_table_fill(const uint64_t* src_addr, const int32_t* src_hws, const float* matrices,
                               const uint64_t* dst_base, const int32_t* sizes, int32_t n_images, int32_t n_scales,
                               void* table, size_t table_bytes);
int rtpe_warp_normalize_batch(const void* table_dev, int32_t n_images, int32_t n_scales, const int32_t* sizes,
                              const float* mean, const float* stdev, int32_t round_u8, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RTPE_HIP_WARP_H */
