/*
 * rtpe_hip_mixed.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) that runs ONE forward over a batch of images of different sizes:
 * the students (rtpe/students.py), which take native-size images and could otherwise batch only equal sizes.
 *
 * Data model.  N images lie in one canvas (N, 3, Hc, Wc): image n at [n, :, :h_n, :w_n], anything elsewhere (the
 * kernels never read it unmasked).  Every tensor of the forward is a canvas too, rtpe_extent(Hc, d) x rtpe_extent(Wc, d)
 * pixels per image at 1 / 2^d; those extents are the PITCH: they address and size the grids.  Image n's own extents,
 * rtpe_extent(h_n, d) x rtpe_extent(w_n, d), MASK: a conv's taps, an average pool's window and divisor, the nearest
 * sampler of a fuse sum and the mean of an SE gate (summed in the image's own row-major order) treat image n as if its
 * map ended there, and no kernel stores beyond them.  Image n's region of the outputs then holds the bits of a forward
 * of that image alone; every output element outside the regions is 0.0.
 *
 * Extent table: RTPE_MIXED_LEVELS rows, row d = N pairs (rtpe_extent(h_n, d), rtpe_extent(w_n, d)) of int32 - a kernel
 * gets the pointer to the row of its level.  rtpe_hrnet_forward_mixed fills it into `table_pinned` (page-locked host
 * memory of the caller, rtpe_mixed_table_ints(N) integers, not to be touched until the copy has run) and copies it in
 * stream order into the tail of the workspace: no blocking upload, no allocation.
 *
 * A mixed forward always takes the routes of a ragged shape (rtpe_hip_anysize.h), whatever the canvas size: the
 * one-workgroup-per-tile conv, the VALU stem, the nearest-to-size fuse, no plane-major tensor, default launch shapes;
 * rtpe_hrnet_autotune and rtpe_hrnet_import_tuned are not involved.
 *
 * Refused before the first launch and before the table is copied (RTPE_E_INVALID): a handle without the any_size
 * property, a program with a transposed conv, a fused BasicBlock pair, a grouped stride-2 launch or a second input
 * (aux pack, resize, gate_mul), an op below 1 / 32, a side below 32, an image larger than the canvas, outputs other
 * than float32.
 *
 * A program with a second input (AttentionStudentSteps) runs its mixed forward through the entry of
 * rtpe_hip_mixed_aux.h, which takes the second canvas; the forward entry of this file has no argument for it and keeps
 * refusing such a program.  rtpe_hrnet_mixed_workspace_bytes sizes the workspace of either kind.
 */
#ifndef RTPE_HIP_MIXED_H
#define RTPE_HIP_MIXED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTPE_MIXED_LEVELS 6 /* rows of the extent table: 1 / 2^0 .. 1 / 2^5 */

/* host only: integers of the extent table of N images (RTPE_MIXED_LEVELS * 2 * N) */
int rtpe_mixed_table_ints(int32_t N, int32_t* count);
/* host only: fills the table of N images of sizes_hw[2 n] x sizes_hw[2 n + 1] pixels in an Hc x Wc canvas */
int rtpe_mixed_table_fill(const int32_t* sizes_hw, int32_t N, int32_t Hc, int32_t Wc, int32_t* table, int32_t n_ints);
/* the workspace of a mixed forward: that of (N, Hc, Wc) and the table behind it */
int rtpe_hrnet_mixed_workspace_bytes(const rtpe_hrnet* h, int32_t N, int32_t Hc, int32_t Wc, size_t* bytes);
/* rtpe_hrnet_forward_flags on a canvas, plus the sizes (host, 2 N integers) and the pinned block for the table */
int rtpe_hrnet_forward_mixed(rtpe_hrnet* h, const void* x, int32_t x_dtype, int32_t N, int32_t Hc, int32_t Wc,
                             const int32_t* sizes_hw, int32_t* table_pinned, int32_t table_ints, void* preds,
                             void* refined, int32_t out_dtype, void* workspace, size_t workspace_bytes, void* stream,
                             uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* RTPE_HIP_MIXED_H */
