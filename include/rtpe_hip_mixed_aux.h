/*
 * rtpe_hip_mixed_aux.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) that runs ONE forward over a batch of images of different sizes for a
 * program with a SECOND input: AttentionStudentSteps (rtpe/students.py), whose `alt` image (the input in LAB or HSV)
 * travels in a canvas of its own.
 *
 * Data model: that of rtpe_hip_mixed.h.  The second input is a canvas (N, 3, Hc, Wc) of float32 like the first, image n
 * at [n, :, :h_n, :w_n], anything elsewhere.  The ops that only such a program has:
 *   aux pack   elementwise over the whole canvas; its readers (the resize, the 5x5 stride-2 conv) mask;
 *   resize     the one op whose ARITHMETIC depends on the image: F.interpolate(alt_n, (ceil(h_n / 4), ceil(w_n / 4)),
 *              mode="bilinear") of image n alone has the scale float(h_n) / float(ceil(h_n / 4)), clamps at h_n - 1 and
 *              copies where the extents agree.  The kernel reads image n's input and output extents from the rows of
 *              the extent table at the two levels, derives the scale on the device with the same correctly rounded
 *              float division, addresses by the canvas pitch and stores nothing beyond image n's output extent;
 *   gate_mul   elementwise over the whole canvas; its readers mask, its sigmoid map is an output and is zeroed outside
 *              the regions with the other output, behind the last op.
 * The 5x5 stride-2 convs of the second stem and the convs over the concatenated tensors run on the mixed instantiations
 * of the one-workgroup-per-tile conv like every other conv of a mixed forward.
 *
 * Refused before the first launch and before the table is copied (RTPE_E_INVALID): a null second input, a program
 * without a second input (rtpe_hrnet_forward_mixed is its entry), and everything rtpe_hrnet_forward_mixed refuses.
 * rtpe_hrnet_forward_mixed itself keeps refusing a program with a second input; rtpe_hrnet_mixed_workspace_bytes sizes
 * the workspace of either kind of program.
 */
#ifndef RTPE_HIP_MIXED_AUX_H
#define RTPE_HIP_MIXED_AUX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* rtpe_hrnet_forward_mixed plus the second input's canvas: aux = (N, 3, Hc, Wc) fp32 NCHW on the device */
int rtpe_hrnet_forward_mixed_aux(rtpe_hrnet* h, const void* x, int32_t x_dtype, const void* aux_nchw_f32, int32_t N,
                                 int32_t Hc, int32_t Wc, const int32_t* sizes_hw, int32_t* table_pinned,
                                 int32_t table_ints, void* preds, void* refined, int32_t out_dtype, void* workspace,
                                 size_t workspace_bytes, void* stream, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* RTPE_HIP_MIXED_AUX_H */
