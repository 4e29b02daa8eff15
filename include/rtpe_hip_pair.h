/*
 * rtpe_hip_pair.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) that runs the 1x1 pair kernel of layer1 on plain tensors.
 */
#ifndef RTPE_HIP_PAIR_H
#define RTPE_HIP_PAIR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The 1x1 pair kernel (csrc/conv_pair.hip) on dense NHWC fp16 tensors of ANY pixel count N * H * W
 * (the /4 maps of a program are multiples of 64 pixels): y = relu(bn1(conv1x1(t, w1)) + residual), (N,H,W,256), and
 * u = relu(bn2(conv1x1(y, w2))), (N,H,W,64), in one launch, with the half wrapper's rounding points (RTPE_F_ROUND_CONV).
 * t: (N,H,W,64).  The residual is res, (N,H,W,256) - or, with x (N,H,W,64) and the third layer (wd_host, alphad, betad:
 * conv 1x1 64 -> 256 + bn, no ReLU) given, bn_d(conv1x1(x, wd)), computed inside the kernel; res is then not read and may
 * be NULL.  Weights: HOST fp16 OIHW, alpha / beta: HOST fp32[cout].  Host-returning (layer-level tests). */
int rtpe_conv1x1_pair_nhwc(const void* t, const void* res, const void* x, int32_t N, int32_t H, int32_t W,
                           const void* w1_host, const float* alpha1, const float* beta1, const void* w2_host,
                           const float* alpha2, const float* beta2, const void* wd_host, const float* alphad,
                           const float* betad, void* y, void* u, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RTPE_HIP_PAIR_H */
