"""CPU tests of the device grouping (csrc/match_dev.hip, HeatmapParser(match_on=...)): the ABI of the new entries and
their argument checks, the refusals raised before any GPU work, and the compiled kernels (no scratch memory, the
rounding points the bit-exactness rests on)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


NEW_SYMBOLS = ("rtpe_match_by_tag_dev_scratch_bytes", "rtpe_match_by_tag_dev", "rtpe_adjust_refine_fused_topk_n",
               "rtpe_adjust_refine_flip_n", "rtpe_adjust_refine_ms_n", "rtpe_adjust_refine_ms_ags_n")


def test_match_device_symbols_are_declared_and_resolve(built):
    hdr = open(os.path.join(ROOT, "include", "rtpe_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", hdr))
    lib = built.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in built.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.rtpe_version() == 4
    assert len(built.EXPORTS) == 59
    # the _n entries take the plain entries' arguments plus P_dev
    for name in NEW_SYMBOLS[2:]:
        assert built._SIGS[name][1][:-1] == built._SIGS[name[:-2]][1]


def test_match_device_entries_check_their_arguments_before_any_launch(built):
    """bad arguments and sizes beyond the limits come back as negative codes with a message naming the limit (no
    launch: the pointers are never read)"""
    L = built.lib()
    nb = ctypes.c_size_t()
    built.check(L.rtpe_match_by_tag_dev_scratch_bytes(32, 17, 30, 1, ctypes.byref(nb)))
    # people rows + one joint mask per possible person, and a device copy of the counts
    assert nb.value == 32 * 17 * 30 * (17 * 4 * 4 + 4) + 32 * 4
    built.check(L.rtpe_match_by_tag_dev_scratch_bytes(2, 17, 30, 2, ctypes.byref(nb)))
    assert nb.value == 2 * 17 * 30 * (17 * 5 * 4 + 4) + 2 * 4
    built.check(L.rtpe_match_by_tag_dev_scratch_bytes(2, 17, 30, 1, ctypes.byref(nb)))        # of call() below
    fake = ctypes.c_void_p(0x1000)

    def call(N=2, J=17, K=30, D=1, w=640, mp=30, cap=None, scratch_bytes=1 << 30, ans=fake, total=fake):
        return L.rtpe_match_by_tag_dev(fake, fake, fake, N, J, K, D, w, mp, 0.1, 1.0, 1, 0, ans,
                                       N * J * K if cap is None else cap, fake, fake, total, fake, scratch_bytes, None)
    for kw, words in ((dict(K=65), "at most 64"), (dict(mp=65), "max_num_people"), (dict(mp=0), "max_num_people"),
                      (dict(J=33), "at most 32"), (dict(D=33), "at most 32"), (dict(N=0), "bad argument"),
                      (dict(w=0), "bad argument"), (dict(ans=None), "bad argument"), (dict(total=None), "bad argument"),
                      (dict(cap=2 * 17 * 30 - 1), "N\\*J\\*K"), (dict(scratch_bytes=nb.value - 4), "scratch too small"),
                      (dict(J=32, K=64, D=8, mp=64), "LDS")):
        with pytest.raises(RuntimeError, match=words):
            built.check(call(**kw))
    for args in ((2, 17, 65, 1), (2, 33, 30, 1), (2, 17, 30, 33), (0, 17, 30, 1)):
        assert L.rtpe_match_by_tag_dev_scratch_bytes(*args, ctypes.byref(nb)) < 0
    assert L.rtpe_match_by_tag_dev_scratch_bytes(2, 17, 30, 1, None) < 0
    # the _n entries refuse a null P_dev
    assert L.rtpe_adjust_refine_flip_n(fake, 8, 8, 1, 17, 16, 16, fake, ctypes.c_void_p(0x2000), fake, 4, 1, 1, fake,
                                       None, None, 0, fake, 1 << 30, None, None) < 0
    assert b"P_dev" in L.rtpe_last_error_string()


def test_match_on_is_checked_and_needs_a_gpu():
    from rtpe import inference
    from rtpe.engine import TeacherPipeline
    from rtpe.third_party.group import HeatmapParser
    with pytest.raises(ValueError, match="match_on"):
        HeatmapParser(17, 30, 0.1, 1.0, True, False, match_on="nonsense")
    assert HeatmapParser(17, 30, 0.1, 1.0, True, False).match_on == "host"
    parser = HeatmapParser(17, 30, 0.1, 1.0, True, False, match_on="device")
    assert parser.match_on == "device"
    parser.match_on = "gpu"                                        # an attribute, like tag_per_joint: checked when used
    with pytest.raises(ValueError, match="match_on"):
        parser.match(np.zeros((1, 17, 30, 1), np.float32), np.zeros((1, 17, 30, 2), np.int64),
                     np.zeros((1, 17, 30), np.float32))
    with pytest.raises(ValueError, match="match_on"):
        TeacherPipeline(None, device="cuda:0", match_on="nonsense")
    img = np.zeros((480, 640, 3), np.uint8)
    for fn in (inference.flip_test_inference, inference.multi_scale_batch_inference):
        with pytest.raises(ValueError, match="match_on"):
            fn(None, HeatmapParser(17, 30, 0.1, 1.0, True, False), [img], 640, match_on="nonsense")
    if torch.cuda.is_available():
        return
    # without a GPU: the project's usual error, before any work - and never the host matcher in its place
    parser.match_on = "device"
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        parser.match_device(z(1, 17, 30, 1), z(1, 17, 30, dtype=torch.int32), z(1, 17, 30), 640)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        parser.match(np.zeros((1, 17, 30, 1), np.float32), np.zeros((1, 17, 30, 2), np.int64),
                     np.zeros((1, 17, 30), np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        parser.parse_lowres(z(1, 17, 64, 64), z(1, 17, 32, 32), (128, 128))


def _kernel_bodies(built, tmp_path):
    from test_flip_decode_host import _device_code
    dis = _device_code(built, tmp_path, "match_dev.hip")
    bodies = [b for b in re.split(r"\n(?=[0-9a-f]+ <)", dis) if re.match(r"[0-9a-f]+ <\S*_kernel", b)]
    return {b.split("<", 1)[1].split(">", 1)[0]: b for b in bodies}


def test_match_device_kernels_use_no_scratch_memory(built, tmp_path):
    """a per-lane array indexed at run time (the cost matrix, a tag list) would show up as scratch memory: they live in
    LDS, the marks of the solver in 64-bit masks"""
    bodies = _kernel_bodies(built, tmp_path)
    assert sum("match_by_tag_kernel" in n for n in bodies) == 1
    assert sum("match_compact_kernel" in n for n in bodies) == 1
    assert len(bodies) == 2
    for n, b in bodies.items():
        assert "scratch_" not in b, n + ": uses scratch memory"


def test_match_device_rounding_points(built, tmp_path):
    """what the bit-exactness rests on, in the compiled grouping kernel: the correctly rounded float32 division of
    the tag means (v_div_scale / v_div_fmas / v_div_fixup, not a bare reciprocal), the double square root followed by
    its Tuckerman check (exact residuals: v_fma_f64), ties-to-even rounding of the cost (v_rndne_f64), lane reads of the
    solver's masks without LDS traffic (v_readlane_b32)"""
    body = [b for n, b in _kernel_bodies(built, tmp_path).items() if "match_by_tag_kernel" in n][0]
    for ins in ("v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32", "v_rsq_f64", "v_fma_f64", "v_rndne_f64",
                "v_readlane_b32"):
        assert ins in body, ins
    # the sums of squares and nearbyint(d) * 100 - val are separate double operations in the source; what keeps them
    # separate in the code is the build flag checked below (the fused double operations present belong to the square
    # root's expansion and to its check)
    assert "v_mul_f64" in body and "v_add_f64" in body
    assert "v_mac_f32" not in body and "v_mad_f32" not in body
    # one build for every file of csrc/: the flag the claim above depends on
    import __graft_entry__ as g
    assert "-ffp-contract=off" in g.FLAGS
