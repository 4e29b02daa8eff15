"""CPU tests of the batched multi-scale test: the grouping of images by their input sizes at every scale, the
sub-batch plan under the forward pixel budget, the refusals raised before any GPU work, the ABI of the new entries
and the compiled multi-scale decode kernels (no registers spilled to scratch memory)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


def test_size_groups_over_all_scales():
    from rtpe.inference import check_scale_factors, group_by_input_size, multi_scale_input_sizes
    scales = check_scale_factors((1, 0.5, 2))
    assert scales == (2, 1, 0.5)
    shapes = [(427, 640), (640, 480), (640, 640), (427, 640), (640, 640), (640, 480), (427, 640)]
    sizes = [multi_scale_input_sizes(np.zeros(s + (3,), np.uint8), 640, scales) for s in shapes]
    # the short side is 320 at scale 0.5 and the long side is rounded up to 64 there, then scaled: the scale-1 size of
    # a 427 x 640 image is 1024 x 640 here, not the 960 x 640 of the single-scale test
    assert sizes[0] == ((2048, 1280), (1024, 640), (512, 320))
    assert sizes[1] == ((1280, 1792), (640, 896), (320, 448))
    assert sizes[2] == ((1280, 1280), (640, 640), (320, 320))
    assert group_by_input_size(sizes) == [(sizes[0], [0, 3, 6]), (sizes[1], [1, 5]), (sizes[2], [2, 4])]


def test_forward_plan_under_the_pixel_budget():
    from rtpe.engine import MAX_FORWARD_PIXELS, forward_plan
    assert MAX_FORWARD_PIXELS == 32 * 640 * 640
    assert forward_plan(32, (1280, 1280)) == [(0, 8), (8, 8), (16, 8), (24, 8)]
    assert forward_plan(32, (640, 640)) == [(0, 32)]
    assert forward_plan(32, (320, 320)) == [(0, 32)]
    assert forward_plan(5, (256, 256), 2 * 256 * 256) == [(0, 2), (2, 2), (4, 1)]
    assert forward_plan(3, (512, 384), 512 * 384) == [(0, 1), (1, 1), (2, 1)]
    for n0, n in forward_plan(32, (1280, 1920)):
        assert n * 1280 * 1920 <= MAX_FORWARD_PIXELS
    with pytest.raises(ValueError, match="budget"):
        forward_plan(1, (1280, 1280), 1280 * 1280 - 1)


@pytest.mark.parametrize("scales,match", [((2, 0.5), "1 must be among"), ((1, 2, 1.0), "not distinct"),
                                          ((2, 1, 0.5, 0.75, 1.5), "at most 4"), ((), "1 must be among")])
def test_scale_refusals(scales, match):
    from rtpe.inference import check_scale_factors
    with pytest.raises(ValueError, match=match):
        check_scale_factors(scales)


def test_batch_inference_refuses_before_any_gpu_work(monkeypatch):
    from rtpe import engine, inference
    from rtpe.third_party.group import HeatmapParser

    class NoGpu:
        def __init__(self, *a, **k):
            raise AssertionError("GPU work before the arguments were checked")
    monkeypatch.setattr(engine, "TeacherPipeline", NoGpu)
    parser = HeatmapParser(17, 30, 0.1, 1.0, True, False)
    img = np.zeros((480, 640, 3), np.uint8)
    for scales in ((2, 0.5), (1, 1), (2, 1, 0.5, 0.75, 1.5)):
        with pytest.raises(ValueError):
            inference.multi_scale_batch_inference(None, parser, [img], 640, scales)
    # scale 1.01 of a 640 input: 646 pixels, not a multiple of 32
    with pytest.raises(ValueError, match="multiple of 32"):
        inference.multi_scale_batch_inference(None, parser, [img], 640, (1.01, 1))
    with pytest.raises(ValueError, match="multiple of 32"):
        inference.multi_scale_input_sizes(img, 640, (1.01, 1))
    with pytest.raises(ValueError, match="tag_per_joint"):
        inference.multi_scale_batch_inference(None, HeatmapParser(17, 30, 0.1, 1.0, True, False, tag_per_joint=False),
                                              [img], 640, (2, 1, 0.5))


NEW_SYMBOLS = ("rtpe_ms_maps_bytes", "rtpe_ms_prep", "rtpe_topk_ms", "rtpe_adjust_refine_ms")


def test_ms_symbols_are_declared_and_resolve(built):
    hdr = open(os.path.join(ROOT, "include", "rtpe_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", hdr))
    lib = built.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in built.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.rtpe_version() == 4


def test_ms_maps_bytes_and_its_checks(built):
    L = built.lib()
    nb = ctypes.c_size_t()
    arr = lambda *v: (ctypes.c_int32 * len(v))(*v)     # noqa: E731
    h2, w2 = arr(640, 320, 160), arr(640, 320, 160)
    built.check(L.rtpe_ms_maps_bytes(32, 17, 3, h2, w2, 1, 1, ctypes.byref(nb)))
    assert nb.value == 4 * 32 * 17 * (2 * (640 * 640 + 320 * 320 + 160 * 160) + 2 * 320 * 320)
    built.check(L.rtpe_ms_maps_bytes(32, 17, 3, h2, w2, 1, 0, ctypes.byref(nb)))
    assert nb.value == 4 * 32 * 17 * (640 * 640 + 320 * 320 + 160 * 160 + 320 * 320)
    for args in ((32, 17, 5, arr(*[8] * 5), arr(*[8] * 5), 1, 1), (32, 17, 3, h2, w2, 3, 1),
                 (32, 17, 0, h2, w2, 0, 1), (32, 33, 3, h2, w2, 1, 1), (0, 17, 3, h2, w2, 1, 1),
                 (32, 17, 3, arr(640, 0, 160), w2, 1, 1), (4000, 17, 3, h2, w2, 1, 1), (32, 17, 3, h2, w2, 1, 2)):
        with pytest.raises(RuntimeError):
            built.check(L.rtpe_ms_maps_bytes(*args, ctypes.byref(nb)))


def test_ms_decode_kernels_do_not_spill(built, tmp_path):
    from test_flip_decode_host import _device_code
    dis = _device_code(built, tmp_path, "decode.hip")
    bodies = re.split(r"\n(?=[0-9a-f]+ <)", dis)
    ms = [b for b in bodies if re.match(r"[0-9a-f]+ <\S*(MultiScaleHeatMap|ms_prep_kernel)", b)]
    names = [b.split("<", 1)[1].split(">", 1)[0] for b in ms]
    assert sum("ms_prep_kernel" in n for n in names) == 4
    assert any("topk_tile_kernel" in n for n in names) and any("topk_merge_kernel" in n for n in names)
    assert any("refine_scan_kernel" in n for n in names) and any("adjust_prepare_kernel" in n for n in names)
    for n, b in zip(names, ms):
        assert "scratch_" not in b, n + ": registers spilled to scratch memory"
