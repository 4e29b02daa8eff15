"""ctypes binding of librtpe_hip.so (include/rtpe_hip.h).

The product path has no CPU fallback: if the shared library is missing or
cannot be loaded, importing anything that needs it raises with build
instructions (``python -c "import __graft_entry__ as g; g.build()"``).
"""
import ctypes
import os
from ctypes import (POINTER, Structure, byref, c_char_p, c_double, c_float, c_int32, c_int64,
                    c_size_t, c_uint32, c_uint64, c_void_p)

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# RTPE_LIBRARY: another build of the same ABI (A/B measurements of two builds on one GPU box)
LIB_PATH = os.environ.get("RTPE_LIBRARY") or os.path.join(_PKG_DIR, "librtpe_hip.so")

ABI_VERSION = 4          # rtpe_version() of the library this binding was written against (include/rtpe_hip.h)
RTPE_DTYPE_F16, RTPE_DTYPE_F32 = 1, 2
OP_STEM, OP_CONV, OP_DECONV, OP_FUSE, OP_CAST, OP_AVGPOOL, OP_SE, OP_CAM_COMBINE, OP_SIGMOID_ADD = range(9)
OP_AUX_PACK, OP_RESIZE, OP_GATE_MUL = 9, 10, 11
F_RELU, F_ROUND_CONV, F_OUT_PREDS, F_OUT_REFINED, F_NO_NHWC, F_F32 = 1, 2, 4, 8, 16, 32
F_PAIR_HEAD, F_PAIR_TAIL = 64, 128
F_PAIR_PROJ = 256        # the skip projection that a 1x1 pair may compute itself (include/rtpe_hip.h)


class TensorDesc(Structure):
    _fields_ = [("channels", c_int32), ("ds_log2", c_int32), ("slot", c_int32), ("reserved", c_int32)]


class OpDesc(Structure):
    _fields_ = [("kind", c_int32), ("flags", c_int32),
                ("in_t", c_int32), ("in_coff", c_int32),
                ("out_t", c_int32), ("out_coff", c_int32),
                ("res_t", c_int32), ("res_coff", c_int32),
                ("cin", c_int32), ("cout", c_int32),
                ("ksize", c_int32), ("stride", c_int32),
                ("w_off", c_int64), ("ab_off", c_int64),
                ("n_terms", c_int32), ("term_t", c_int32 * 4), ("term_up", c_int32 * 4),
                ("reserved", c_int32 * 3), ("lane", c_int32), ("region", c_int32)]


_SIGS = {
    "rtpe_last_error_string": (c_char_p, []),
    "rtpe_version": (c_int32, []),
    "rtpe_device_count": (c_int32, []),
    "rtpe_hrnet_create": (c_int32, [POINTER(OpDesc), c_int32, POINTER(TensorDesc), c_int32,
                                    c_void_p, c_size_t, c_int32, POINTER(c_void_p)]),
    "rtpe_hrnet_destroy": (c_int32, [c_void_p]),
    "rtpe_hrnet_workspace_bytes": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "rtpe_hrnet_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                     c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    "rtpe_hrnet_forward_flags": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                           c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p, c_uint32]),
    "rtpe_hrnet_forward_aux": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32,
                                         c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    "rtpe_rgb_to_alt": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "rtpe_hrnet_forward_timed": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                           c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p,
                                           POINTER(c_float), c_int32]),
    "rtpe_hrnet_forward_record": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                            c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p, c_int32]),
    "rtpe_hrnet_read_record": (c_int32, [c_void_p, c_int32, POINTER(c_float), c_int32]),
    "rtpe_hrnet_op_cost": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32,
                                     POINTER(c_double), POINTER(c_double)]),
    "rtpe_hrnet_autotune": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                      c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    "rtpe_hrnet_autotune_aux": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32,
                                          c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    "rtpe_set_option": (c_int32, [c_char_p, c_int32]),
    "rtpe_get_option": (c_int32, [c_char_p, POINTER(c_int32)]),
    "rtpe_hrnet_tuned_ints": (c_int32, [c_void_p, POINTER(c_int32)]),
    "rtpe_hrnet_export_tuned": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32), c_int32]),
    "rtpe_hrnet_import_tuned": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32), c_int32]),
    "rtpe_hrnet_op_tile": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    "rtpe_hrnet_plane_major_tensors": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    "rtpe_conv2d_nhwc": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                   POINTER(c_float), POINTER(c_float), c_int32, c_int32, c_int32,
                                   c_int32, c_void_p, c_void_p, c_void_p]),
    "rtpe_conv2d_nhwc_ex": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                      POINTER(c_float), POINTER(c_float), c_int32, c_int32, c_int32,
                                      c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "rtpe_deconv4x4s2_nhwc": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, POINTER(c_float),
                                        POINTER(c_float), c_int32, c_int32, c_void_p, c_void_p]),
    "rtpe_fuse_nhwc": (c_int32, [POINTER(c_void_p), POINTER(c_int32), c_int32, c_int32, c_int32, c_int32, c_int32,
                                 c_int32, c_void_p, c_void_p]),
    "rtpe_basicblock_nhwc": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, POINTER(c_float), POINTER(c_float),
                                       c_void_p, POINTER(c_float), POINTER(c_float), c_void_p, c_void_p]),
    "rtpe_warp_normalize": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_float), POINTER(c_float),
                                      POINTER(c_float), c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "rtpe_resize_combine": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), c_int32, c_int32,
                                      c_void_p, c_int32, c_int32, c_int32, c_float, c_void_p]),
    "rtpe_bilinear_upsample": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                         c_int32, c_void_p]),
    "rtpe_nms": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "rtpe_topk": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                            c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_size_t, c_void_p]),
    "rtpe_topk_scratch_bytes": (c_int32, [c_int32, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "rtpe_topk_fused": (c_int32, [c_void_p, c_int32, c_int32, c_int64, c_void_p, c_int32, c_int32, c_int64,
                                  c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rtpe_match_by_tag": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                    c_int32, c_double, c_double, c_int32, c_int32, c_void_p, c_int32,
                                    POINTER(c_int32)]),
    "rtpe_munkres": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, POINTER(c_int32)]),
    "rtpe_adjust_refine": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                     c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p,
                                     c_void_p, c_size_t, c_void_p]),
    "rtpe_adjust_refine_scratch_bytes": (c_int32, [c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "rtpe_adjust_refine_fused": (c_int32, [c_void_p, c_int32, c_int32, c_int64, c_void_p, c_int32, c_int32,
                                           c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                           c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t,
                                           c_void_p]),
    "rtpe_adjust_refine_fused_topk": (c_int32, [c_void_p, c_int32, c_int32, c_int64, c_void_p, c_int32, c_int32,
                                                c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                                c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                                c_int32, c_void_p, c_size_t, c_void_p]),
    "rtpe_flip_maps_bytes": (c_int32, [c_int32, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "rtpe_topk_flip": (c_int32, [c_void_p, c_int32, c_int32, c_int64, c_void_p, c_int32, c_int32, c_int64,
                                 c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, POINTER(c_int32),
                                 c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "rtpe_adjust_refine_flip": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                          c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p,
                                          c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    "rtpe_ms_maps_bytes": (c_int32, [c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), c_int32, c_int32,
                                     POINTER(c_size_t)]),
    "rtpe_ms_prep": (c_int32, [c_void_p, c_int32, c_int32, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                               c_int64, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), c_int32,
                               POINTER(c_int32), POINTER(c_int32), c_int32, c_int32, c_int32, c_void_p, c_size_t,
                               c_void_p]),
    "rtpe_topk_ms": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), c_int32,
                               c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                               c_size_t, c_void_p, c_size_t, c_void_p]),
    "rtpe_adjust_refine_ms": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32),
                                        c_int32, c_int32, c_int32, c_int32, c_size_t, c_void_p, c_void_p, c_void_p,
                                        c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                        c_size_t, c_void_p]),
    "rtpe_ms_ags_maps_bytes": (c_int32, [c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), c_int32,
                                         c_int32, POINTER(c_size_t)]),
    "rtpe_ms_ags_prep": (c_int32, [c_void_p, c_int32, c_int32, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                   c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), c_int32,
                                   POINTER(c_int32), POINTER(c_int32), c_int32, c_int32, c_int32, c_void_p, c_size_t,
                                   c_void_p]),
    "rtpe_topk_ms_ags": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32), c_int32,
                                   c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                   c_size_t, c_void_p, c_size_t, c_void_p]),
    "rtpe_adjust_refine_ms_ags": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32),
                                            c_int32, c_int32, c_int32, c_int32, c_size_t, c_void_p, c_void_p, c_void_p,
                                            c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                            c_size_t, c_void_p]),
    "rtpe_match_by_tag_batch": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                          c_int32, c_int32, c_double, c_double, c_int32, c_int32, c_void_p,
                                          c_int32, c_void_p, c_void_p, c_int32]),
    "rtpe_match_by_tag_dev_scratch_bytes": (c_int32, [c_int32, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "rtpe_match_by_tag_dev": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                        c_int32, c_double, c_double, c_int32, c_int32, c_void_p, c_int32, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}
# adjust + refine with the number of people read on the device: the plain entry's arguments + P_dev
for _name in ("rtpe_adjust_refine_fused_topk", "rtpe_adjust_refine_flip", "rtpe_adjust_refine_ms",
              "rtpe_adjust_refine_ms_ags"):
    _SIGS[_name + "_n"] = (c_int32, _SIGS[_name][1] + [c_void_p])

# per-image decode size (include/rtpe_hip_sizes.h): (oh, ow) of the one-size entries ->
# (sizes_table, table_bytes, max_oh, max_ow, w_enc)
_SIZES = [c_void_p, c_size_t, c_int32, c_int32, c_int32]
_SIGS_SIZES = {
    "rtpe_decode_sizes_bytes": (c_int32, [c_int32, POINTER(c_size_t)]),
    "rtpe_decode_sizes_fill": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t,
                                         POINTER(c_int32), POINTER(c_int32)]),
}
for _name in ("rtpe_topk_fused", "rtpe_adjust_refine_fused_topk"):
    _a = _SIGS[_name][1]
    _SIGS_SIZES[_name + "_sizes"] = (c_int32, _a[:10] + _SIZES + _a[12:])
_SIGS_SIZES["rtpe_adjust_refine_fused_topk_sizes_n"] = (
    c_int32, _SIGS_SIZES["rtpe_adjust_refine_fused_topk_sizes"][1] + [c_void_p])

# batched pre-processing (include/rtpe_hip_warp.h): the job table of a chunk (host) and its launch
_SIGS_WARP = {
    "rtpe_warp_batch_table_bytes": (c_int32, [c_int32, c_int32, POINTER(c_size_t)]),
    "rtpe_warp_batch_table_fill": (c_int32, [POINTER(c_uint64), POINTER(c_int32), POINTER(c_float), POINTER(c_uint64),
                                             POINTER(c_int32), c_int32, c_int32, c_void_p, c_size_t]),
    "rtpe_warp_normalize_batch": (c_int32, [c_void_p, c_int32, c_int32, POINTER(c_int32), POINTER(c_float),
                                            POINTER(c_float), c_int32, c_void_p]),
}

# shared-tag decode (include/rtpe_hip_shared.h): the arguments of the entries without "_shared", `tg` one plane per image
_SIGS_SHARED = {
    "rtpe_topk_fused_shared": (c_int32, list(_SIGS["rtpe_topk_fused"][1])),
    "rtpe_adjust_refine_fused_shared_topk": (c_int32, list(_SIGS["rtpe_adjust_refine_fused_topk"][1])),
    "rtpe_adjust_refine_fused_shared_topk_n": (c_int32, list(_SIGS["rtpe_adjust_refine_fused_topk_n"][1])),
}

EXPORTS = tuple(_SIGS)                  # the prototypes of include/rtpe_hip.h itself
EXPORTS_SIZES = tuple(_SIGS_SIZES)      # those of include/rtpe_hip_sizes.h, which it includes
EXPORTS_WARP = tuple(_SIGS_WARP)        # those of include/rtpe_hip_warp.h, likewise
_SIGS_PAIR = {
    "rtpe_conv1x1_pair_nhwc": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}
EXPORTS_SHARED = tuple(_SIGS_SHARED)    # those of include/rtpe_hip_shared.h, likewise
EXPORTS_PAIR = tuple(_SIGS_PAIR)        # that of include/rtpe_hip_pair.h, likewise
# device-resident keypoint records (include/rtpe_hip_records.h)
_SIGS_RECORDS = {
    "rtpe_records_floats": (c_int32, [c_int32, c_int32, POINTER(c_size_t)]),
    "rtpe_pack_records": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                    c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
}
EXPORTS_RECORDS = tuple(_SIGS_RECORDS)  # those of include/rtpe_hip_records.h, likewise
# averaged-tag test (include/rtpe_hip_tagmean.h): the channel mean, and the `_ags` entries of the multi-scale decode
# with the decode size (oh, ow) added where the maps buffer is sized or checked
_SIGS_TAGMEAN = {
    "rtpe_channel_mean": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int64, c_int64, c_void_p,
                                    c_void_p]),
    "rtpe_ms_mean_maps_bytes": (c_int32, _SIGS["rtpe_ms_ags_maps_bytes"][1][:7] + [c_int32, c_int32,
                                                                                   POINTER(c_size_t)]),
    "rtpe_ms_mean_prep": (c_int32, _SIGS["rtpe_ms_ags_prep"][1][:21] + [c_int32, c_int32] +
                          _SIGS["rtpe_ms_ags_prep"][1][21:]),
    "rtpe_topk_ms_mean": (c_int32, list(_SIGS["rtpe_topk_ms_ags"][1])),
    "rtpe_adjust_refine_ms_mean": (c_int32, list(_SIGS["rtpe_adjust_refine_ms_ags"][1])),
    "rtpe_adjust_refine_ms_mean_n": (c_int32, list(_SIGS["rtpe_adjust_refine_ms_ags_n"][1])),
}
EXPORTS_TAGMEAN = tuple(_SIGS_TAGMEAN)  # those of include/rtpe_hip_tagmean.h, likewise
# multi-scale / flip test without projection (include/rtpe_hip_noproj.h): the `_ms` entries; the decode grid is the
# refined size of the largest scale, so the top-k and adjust + refine entries take no (oh, ow)
_a = _SIGS["rtpe_adjust_refine_ms"][1]
_SIGS_NOPROJ = {
    "rtpe_ms_np_maps_bytes": (c_int32, list(_SIGS["rtpe_ms_maps_bytes"][1])),
    "rtpe_ms_np_prep": (c_int32, list(_SIGS["rtpe_ms_prep"][1])),
    "rtpe_topk_ms_np": (c_int32, _SIGS["rtpe_topk_ms"][1][:8] + _SIGS["rtpe_topk_ms"][1][10:]),
    "rtpe_adjust_refine_ms_np": (c_int32, _a[:8] + _a[10:]),
    "rtpe_adjust_refine_ms_np_n": (c_int32, _a[:8] + _a[10:] + [c_void_p]),
}
EXPORTS_NOPROJ = tuple(_SIGS_NOPROJ)    # those of include/rtpe_hip_noproj.h, likewise
# inputs whose sides are not multiples of 32 (include/rtpe_hip_anysize.h): the extent rule, the nearest-to-size index rule
# and the property of a handle that lets it take such shapes
_SIGS_ANYSIZE = {
    "rtpe_extent": (c_int32, [c_int32, c_int32]),
    "rtpe_nearest_src": (c_int32, [c_int32, c_int32, c_int32]),
    "rtpe_hrnet_set_any_size": (c_int32, [c_void_p, c_int32]),
    "rtpe_hrnet_get_any_size": (c_int32, [c_void_p, POINTER(c_int32)]),
}
EXPORTS_ANYSIZE = tuple(_SIGS_ANYSIZE)  # those of include/rtpe_hip_anysize.h, likewise
# one forward over images of different sizes (include/rtpe_hip_mixed.h): the extent table and the forward on a canvas
MIXED_LEVELS = 6
_SIGS_MIXED = {
    "rtpe_mixed_table_ints": (c_int32, [c_int32, POINTER(c_int32)]),
    "rtpe_mixed_table_fill": (c_int32, [POINTER(c_int32), c_int32, c_int32, c_int32, POINTER(c_int32), c_int32]),
    "rtpe_hrnet_mixed_workspace_bytes": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "rtpe_hrnet_forward_mixed": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32),
                                           c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_size_t,
                                           c_void_p, c_uint32]),
}
EXPORTS_MIXED = tuple(_SIGS_MIXED)      # those of include/rtpe_hip_mixed.h, likewise
# one-pass decode of a mixed-size batch from its canvas (include/rtpe_hip_mixdec.h): the table fill with the images' own
# map extents, and the arguments of the `_sizes` entries with (hh, hw, th, tw) read as the pitch, `tg` one plane per image
_SIGS_MIXDEC = {
    "rtpe_decode_mixed_fill": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                         c_void_p, c_size_t, POINTER(c_int32), POINTER(c_int32)]),
    "rtpe_topk_fused_mixed": (c_int32, list(_SIGS_SIZES["rtpe_topk_fused_sizes"][1])),
    "rtpe_adjust_refine_fused_mixed_topk": (c_int32, list(_SIGS_SIZES["rtpe_adjust_refine_fused_topk_sizes"][1])),
    "rtpe_adjust_refine_fused_mixed_topk_n": (c_int32, list(_SIGS_SIZES["rtpe_adjust_refine_fused_topk_sizes_n"][1])),
}
EXPORTS_MIXDEC = tuple(_SIGS_MIXDEC)    # those of include/rtpe_hip_mixdec.h, likewise
# what one forward enqueued (include/rtpe_hip_trace.h): forward_aux with the per-call flags, and the trace's read-back
FWD_TRACE = 2
TRACE_INTS, TRACE_LAUNCH, TRACE_RECORD, TRACE_WAIT, TRACE_MASK, TRACE_FORK_EVENT = 5, 1, 2, 3, 4, 4
_SIGS_TRACE = {
    "rtpe_hrnet_forward_aux_flags": (c_int32, _SIGS["rtpe_hrnet_forward_aux"][1] + [c_uint32]),
    "rtpe_hrnet_read_trace": (c_int32, [c_void_p, POINTER(c_int32), c_int32, POINTER(c_int32)]),
}
EXPORTS_TRACE = tuple(_SIGS_TRACE)      # those of include/rtpe_hip_trace.h, likewise
# a mixed-size batch for a program with a second input (include/rtpe_hip_mixed_aux.h): rtpe_hrnet_forward_mixed's arguments
# with the second canvas behind x_dtype, where rtpe_hrnet_forward_aux has it
_m = _SIGS_MIXED["rtpe_hrnet_forward_mixed"][1]
_SIGS_MIXAUX = {
    "rtpe_hrnet_forward_mixed_aux": (c_int32, _m[:3] + [c_void_p] + _m[3:]),
}
EXPORTS_MIXAUX = tuple(_SIGS_MIXAUX)    # that of include/rtpe_hip_mixed_aux.h, likewise
# the students' front end (include/rtpe_hip_frames.h): the job table of N uint8 frames (host) and the one launch that
# writes the image canvas and the LAB / HSV canvas
FRAMES_ALT_MODES = {None: -1, "LAB": 0, "HSV": 1}
_SIGS_FRAMES = {
    "rtpe_frames_table_bytes": (c_int32, [c_int32, POINTER(c_size_t)]),
    "rtpe_frames_table_fill": (c_int32, [POINTER(c_uint64), POINTER(c_int32), c_int32, c_int32, c_int32, c_void_p,
                                         c_size_t]),
    "rtpe_frames_to_canvases": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_float), POINTER(c_float),
                                          c_int32, c_void_p, c_void_p, c_void_p]),
}
EXPORTS_FRAMES = tuple(_SIGS_FRAMES)    # those of include/rtpe_hip_frames.h, likewise
# COCO keypoint scoring of the records (include/rtpe_hip_oks.h): the sizes of the result table and the scratch, and the
# one launch that ranks, computes OKS and matches per record
OKS_GT_ROW, OKS_MAX_DETS, OKS_MAX_RANGES, OKS_LDS_DOUBLES = 64, 64, 16, 512
_SIGS_OKS = {
    "rtpe_oks_eval_bytes": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_size_t), POINTER(c_size_t)]),
    "rtpe_oks_eval": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_size_t, c_void_p, c_size_t,
                                c_void_p]),
}
EXPORTS_OKS = tuple(_SIGS_OKS)          # those of include/rtpe_hip_oks.h, likewise
# distillation targets and losses (include/rtpe_hip_distill.h): the ground-truth maps, the targets at the output grids,
# the BCE loss's normalisation, and the loss values
DISTILL_CHUNK, DISTILL_MAX_PATCH, DISTILL_MAX_BLOCKS, DISTILL_SCRATCH_BYTES, DISTILL_LOSS_BYTES = 64, 1024, 256, 16384, 40
DISTILL_BCE, DISTILL_MSE = 0, 1
_SIGS_DISTILL = {
    "rtpe_gt_heatmaps": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                   c_double, c_void_p, c_void_p]),
    "rtpe_distill_targets_scratch_bytes": (c_int32, [c_int32, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "rtpe_distill_targets": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_double, c_void_p, c_int32,
                                       c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                       c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_size_t, c_void_p]),
    "rtpe_distill_normalise": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                         c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rtpe_distill_loss": (c_int32, [c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                    c_int32, c_int32, c_int32, c_double, c_float, c_float, c_float, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}
EXPORTS_DISTILL = tuple(_SIGS_DISTILL)  # those of include/rtpe_hip_distill.h, likewise
# the gradient of the distillation losses with respect to the student's output (include/rtpe_hip_distill_grad.h)
_SIGS_DISTILL_GRAD = {
    "rtpe_distill_loss_backward": (c_int32, [c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                             c_int32, c_int32, c_double, c_float, c_float, c_void_p, c_void_p, c_void_p]),
}
EXPORTS_DISTILL_GRAD = tuple(_SIGS_DISTILL_GRAD)    # that of include/rtpe_hip_distill_grad.h, likewise
_lib = None


def lib():
    """the loaded library (raises if it has not been built)"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "rtpe: %s not found - the HIP extension is not built and there is no CPU "
                "fallback.  Build it with `python -c \"import __graft_entry__ as g; g.build()\"` "
                "from the repository root (needs hipcc)." % LIB_PATH)
        # PyTorch brings its own copy of the HIP runtime (torch/lib/libamdhip64.so); this library is linked against the
        # system's.  Whichever is in the process first serves both (same SONAME) - but only if torch's is loaded BEFORE this
        # library: loaded after it, a second runtime instance comes up and one of the two finds "no ROCm-capable device"
        # (seen with `g.build(); g.smoke()` in one process: build() loaded this library before anything imported torch).
        import torch  # noqa: F401
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise RuntimeError("rtpe: cannot load %s: %s" % (LIB_PATH, e)) from e
        for name, (res, args) in list(_SIGS.items()) + list(_SIGS_SIZES.items()) + list(_SIGS_WARP.items()) + \
                list(_SIGS_SHARED.items()) + list(_SIGS_PAIR.items()) + list(_SIGS_RECORDS.items()) + \
                list(_SIGS_TAGMEAN.items()) + list(_SIGS_NOPROJ.items()) + list(_SIGS_ANYSIZE.items()) + \
                list(_SIGS_MIXED.items()) + list(_SIGS_MIXDEC.items()) + list(_SIGS_TRACE.items()) + \
                list(_SIGS_MIXAUX.items()) + list(_SIGS_FRAMES.items()) + list(_SIGS_OKS.items()) + \
                list(_SIGS_DISTILL.items()) + list(_SIGS_DISTILL_GRAD.items()):
            fn = getattr(L, name)       # AttributeError if an export is missing
            fn.restype, fn.argtypes = res, args
        got = L.rtpe_version()
        if got != ABI_VERSION:      # e.g. RTPE_LIBRARY pointing at a build of another round: descriptors and records differ
            raise RuntimeError("rtpe: %s has ABI revision %d, this binding needs %d - rebuild it from this tree "
                               "(`python -c \"import __graft_entry__ as g; g.build()\"`)" % (LIB_PATH, got, ABI_VERSION))
        _lib = L
    return _lib


def extent(n, ds):
    """pixels along a side of ``n`` input pixels of a tensor at 1 / 2^ds (csrc/rtpe_common.h ``extent``, the same rule):
    ``n >> ds`` for a multiple of 32, as ever; otherwise ``ceil(n / 2^ds)``, what ``ds`` stride-2 convs with padding k // 2
    or ``AvgPool2d(3, 2, 1)`` leave.  The two branches agree for ds <= 5; the first keeps a 32-wide input at ds = 6 a tensor
    without pixels, which the avgpool op refuses to pool into."""
    n, ds = int(n), int(ds)
    return (n + (1 << ds) - 1) >> ds if n % 32 else n >> ds


def ragged(H, W):
    """a side that is no multiple of 32: only programs with ``any_size`` take such an input"""
    return bool(int(H) % 32 or int(W) % 32)


def nearest_src(dst, n_in, n_out):
    """source index of ``F.interpolate(mode="nearest", size=n_out)`` on PyTorch-CPU, the rule of the fuse op at ragged
    shapes (csrc/rtpe_common.h ``nearest_src``): ``min(int(floorf(dst * scale)), n_in - 1)`` with the fp32 scale
    ``float(n_in) / float(n_out)`` and an fp32 product.  ``dst``: an int or an integer array."""
    import numpy as np
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.asarray(dst, np.float32) * scale).astype(np.int64)
    return np.minimum(src, n_in - 1)


def check(rc):
    if rc != 0:
        msg = lib().rtpe_last_error_string()
        raise RuntimeError("rtpe_hip error %d: %s" % (rc, msg.decode() if msg else "?"))


def require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(
            "rtpe: %s runs on the MI355X HIP path only and got a %s tensor; move it to a GPU "
            "(there is deliberately no CPU fallback in the product path)" % (what, t.device))


def stream_ptr(device):
    import torch
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def on_device(t):
    """context manager: the device of tensor ``t`` is HIP's current device inside the block.  The handle-less
    launch functions of the ABI act on the current device (include/rtpe_hip.h, conventions); PyTorch's default
    stream handle is 0 on every device, so without this a tensor on cuda:1 would be processed by kernels
    launched on cuda:0."""
    import torch
    return torch.cuda.device(t.device)


def same_device(what, first, *others):
    """all tensors of one native call must live on one GPU"""
    for t in others:
        if t is not None and t.device != first.device:
            raise RuntimeError("rtpe: %s: tensors on different devices (%s and %s)" % (what, first.device, t.device))


def host_threads(default_cap=16):
    """host threads this process may use: the cores it is allowed to run on, divided among the ranks of the node
    (LOCAL_WORLD_SIZE, set by torch.distributed.run) - 8 ranks x 16 matcher threads + 8 torch threads each is
    exactly the burst that exhausts a container's CPU quota and stalls the kernel launches"""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        local_world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))
    except ValueError:
        local_world = 1
    return max(1, min(default_cap, cores // local_world))
