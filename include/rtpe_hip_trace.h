/*
 * rtpe_hip_trace.h - the part of the C ABI of librtpe_hip.so (rtpe_hip.h, which includes this file; same
 * conventions, same error codes, rtpe_version() 4) that reports what one forward enqueued: which op was launched on
 * which stream, and every event record and stream wait, in the order in which the host issued them.  It exists for
 * oracle/schedule.py, which checks that every reader of a tensor or a workspace slot is ordered behind its writer.
 *
 * A forward called with RTPE_FWD_TRACE (rtpe_hrnet_forward_flags, rtpe_hrnet_forward_mixed,
 * rtpe_hrnet_forward_aux_flags) launches exactly what it launches without the flag and leaves its trace with the
 * handle, replacing the previous one; a forward without the flag tests one pointer and leaves the kept trace alone.
 * The timed and the recorded forward stay on one stream and take no flags.
 *
 * A trace is a list of records of RTPE_TRACE_INTS integers {kind, a, b, c, d}:
 *   RTPE_TRACE_LAUNCH  a = op, b = stream, c = the route of the op (RTPE_ROUTE_*), d = the route's `by`
 *                      one per op, where the executor calls its launch function - also for the ops that launch nothing
 *                      there (RTPE_ROUTE_DONE_BY, _PAIR_HEAD, _PAIR_PROJ: the launch at op `by` computes them)
 *   RTPE_TRACE_RECORD  a = stream, b = event      hipEventRecord
 *   RTPE_TRACE_WAIT    a = stream, b = event      hipStreamWaitEvent
 *   RTPE_TRACE_MASK    a = stream                 the launch that zeroes the outputs of a mixed-size batch outside the images
 * Streams: 0 = the caller's, 1..3 = the lanes'.  Events: i < n_ops = the event behind op i, n_ops + l = the join of
 * lane l (1..3), n_ops + RTPE_TRACE_FORK_EVENT = the fork of a region.  The event records and waits are written by
 * the two functions that issue the HIP calls, so the trace cannot say anything else than what was enqueued.
 *
 * `by` of a route: _DONE_BY, _PAIR_HEAD: the op whose launch computes this one; _PAIR_PROJ: the pair's tail;
 * _PAIR_TAIL: the head; _S2_GROUP: the number of ops of the group (this one and the next by - 1); else 0.
 */
#ifndef RTPE_HIP_TRACE_H
#define RTPE_HIP_TRACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTPE_TRACE_INTS 5
#define RTPE_TRACE_LAUNCH 1
#define RTPE_TRACE_RECORD 2
#define RTPE_TRACE_WAIT 3
#define RTPE_TRACE_MASK 4
#define RTPE_TRACE_FORK_EVENT 4

/* route kinds (csrc/engine.hip); 0 = an op without a conv, 1..4 = a conv on the kernel of its launch shape (tile, stream, direct, conv64) */
#define RTPE_ROUTE_TILE 1
#define RTPE_ROUTE_HEAD 5
#define RTPE_ROUTE_S2 6
#define RTPE_ROUTE_S2_GROUP 7
#define RTPE_ROUTE_DECONV_MERGED 8 /* 9: on deconv48.hip */
#define RTPE_ROUTE_PAIR_HEAD 10
#define RTPE_ROUTE_PAIR_TAIL 11
#define RTPE_ROUTE_PAIR_PROJ 12
#define RTPE_ROUTE_BLOCK 13
#define RTPE_ROUTE_STEM_FUSED 14
#define RTPE_ROUTE_STEM_CONV1 15
#define RTPE_ROUTE_STEM_PLAIN 16
#define RTPE_ROUTE_DONE_BY 17

/* rtpe_hrnet_forward_aux with per-call switches (flags: RTPE_FWD_*; unknown bits are an error) */
int rtpe_hrnet_forward_aux_flags(rtpe_hrnet* h, const void* x, int32_t x_dtype, const void* aux_nchw_f32, int32_t N,
                                 int32_t H, int32_t W, void* preds, void* refined, int32_t out_dtype,
                                 void* workspace, size_t workspace_bytes, void* stream, uint32_t flags);

/* The trace of the last forward with RTPE_FWD_TRACE on this handle.  *count = its length in integers (0: none yet).
 * out == NULL: the length only; else the integers are copied to out[0 .. n_ints), RTPE_E_INVALID when they do not fit.
 * Host only; call it from the thread that issued the forward. */
int rtpe_hrnet_read_trace(const rtpe_hrnet* h, int32_t* out, int32_t n_ints, int32_t* count);

#ifdef __cplusplus
}
#endif
#endif /* RTPE_HIP_TRACE_H */
