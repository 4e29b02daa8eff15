"""CPU tests of the batched AGS multi-scale test (one tag map per image, shared by all joints): the ABI of the new
entries, the bytes of the AGS maps buffer and the checks of the entries, the refusals raised before any GPU work, and
the compiled AGS decode kernels (no registers spilled to scratch memory)."""
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


NEW_SYMBOLS = ("rtpe_ms_ags_maps_bytes", "rtpe_ms_ags_prep", "rtpe_topk_ms_ags", "rtpe_adjust_refine_ms_ags")


def test_ags_symbols_are_declared_and_resolve(built):
    hdr = open(os.path.join(ROOT, "include", "rtpe_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", hdr))
    lib = built.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in built.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.rtpe_version() == 4


def _arr(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_ags_maps_bytes_and_its_checks(built):
    L = built.lib()
    nb, old = ctypes.c_size_t(), ctypes.c_size_t()
    h2, w2 = _arr(640, 320, 160), _arr(640, 320, 160)
    # per scale A_o and A_f, no per-joint tag maps, then one plane per image at the smallest scale's refined size
    built.check(L.rtpe_ms_ags_maps_bytes(32, 17, 3, h2, w2, 1, 1, ctypes.byref(nb)))
    assert nb.value == 4 * (32 * 17 * 2 * (640 * 640 + 320 * 320 + 160 * 160) + 32 * 160 * 160)
    built.check(L.rtpe_ms_ags_maps_bytes(32, 17, 3, h2, w2, 1, 0, ctypes.byref(nb)))
    assert nb.value == 4 * (32 * 17 * (640 * 640 + 320 * 320 + 160 * 160) + 32 * 160 * 160)
    # the single-scale protocol at 640 x 640: 459 MB against the 891 MB of the per-joint layout
    built.check(L.rtpe_ms_ags_maps_bytes(32, 17, 1, _arr(320), _arr(320), 0, 1, ctypes.byref(nb)))
    built.check(L.rtpe_ms_maps_bytes(32, 17, 1, _arr(320), _arr(320), 0, 1, ctypes.byref(old)))
    assert nb.value == 4 * (32 * 17 * 2 + 32) * 320 * 320 == 458_752_000
    assert old.value == 4 * 32 * 17 * 4 * 320 * 320 == 891_289_600
    # the smallest scale is the last one, whatever the order of the sizes says
    built.check(L.rtpe_ms_ags_maps_bytes(2, 17, 2, _arr(64, 96), _arr(64, 96), 0, 0, ctypes.byref(nb)))
    assert nb.value == 4 * (2 * 17 * (64 * 64 + 96 * 96) + 2 * 96 * 96)
    for args in ((32, 17, 5, _arr(*[8] * 5), _arr(*[8] * 5), 1, 1), (32, 17, 3, h2, w2, 3, 1),
                 (32, 17, 0, h2, w2, 0, 1), (32, 33, 3, h2, w2, 1, 1), (0, 17, 3, h2, w2, 1, 1),
                 (32, 17, 3, _arr(640, 0, 160), w2, 1, 1), (4000, 17, 3, h2, w2, 1, 1), (32, 17, 3, h2, w2, 1, 2)):
        with pytest.raises(RuntimeError):
            built.check(L.rtpe_ms_ags_maps_bytes(*args, ctypes.byref(nb)))
    with pytest.raises(RuntimeError):
        built.check(L.rtpe_ms_ags_maps_bytes(32, 17, 3, h2, w2, 1, 1, None))


def test_ags_entries_check_their_arguments_before_any_launch(built):
    """bad arguments come back as negative codes (no launch: the pointers are never read)"""
    L = built.lib()
    h2, w2 = _arr(32, 16), _arr(48, 24)
    nb = ctypes.c_size_t()
    built.check(L.rtpe_ms_ags_maps_bytes(2, 17, 2, h2, w2, 0, 0, ctypes.byref(nb)))
    fake = ctypes.c_void_p(0x1000)
    perm = _arr(*range(17))

    def prep(scale=1, n0=0, n=2, maps_bytes=nb.value, flip=0, N=2):
        return L.rtpe_ms_ags_prep(fake, 8, 12, 2 * 17 * 8 * 12, fake, 17 * 16 * 24, fake, 2 * 17 * 8 * 12, fake,
                                  17 * 16 * 24, n0, n, N, 17, perm, 2, h2, w2, 0, flip, scale, fake, maps_bytes, None)
    for kw in (dict(scale=2), dict(scale=-1), dict(n0=1, n=2), dict(n=0), dict(maps_bytes=nb.value - 4),
               dict(N=0), dict(flip=1)):          # flip=1: the buffer was sized without the mirror maps
        assert prep(**kw) < 0, kw
    val = ctypes.c_void_p(0x2000)
    assert L.rtpe_topk_ms_ags(fake, 2, 17, 2, h2, w2, 0, 0, 64, 96, 30, 5, 2, val, val, val, nb.value - 4, fake,
                              1 << 30, None) < 0
    assert L.rtpe_topk_ms_ags(fake, 2, 17, 2, h2, w2, 0, 0, 64, 96, 0, 5, 2, val, val, val, nb.value, fake,
                              1 << 30, None) < 0
    assert L.rtpe_adjust_refine_ms_ags(fake, 2, 17, 2, h2, w2, 0, 0, 64, 96, nb.value - 4, val, fake, val, 1, 1, 1,
                                       val, None, None, 0, fake, 1 << 30, None) < 0
    assert L.rtpe_adjust_refine_ms_ags(fake, 2, 17, 2, h2, w2, 0, 0, 64, 96, nb.value, val, fake, val, 1, 1, 1,
                                       val, val, None, 30, fake, 1 << 30, None) < 0
    # P == 0: nothing to do, nothing launched
    built.check(L.rtpe_adjust_refine_ms_ags(fake, 2, 17, 2, h2, w2, 0, 0, 64, 96, nb.value, None, None, None, 0, 1, 1,
                                            None, None, None, 0, None, 0, None))


def test_ags_batch_inference_refuses_before_any_gpu_work(monkeypatch):
    from rtpe import engine, inference
    from rtpe.third_party.group import HeatmapParser

    class NoGpu:
        def __init__(self, *a, **k):
            assert k.get("ags") is True
            raise AssertionError("GPU work")
    monkeypatch.setattr(engine, "TeacherPipeline", NoGpu)
    img = np.zeros((480, 640, 3), np.uint8)
    no_tpj = HeatmapParser(17, 30, 0.1, 1.0, True, False, tag_per_joint=False)
    parser = HeatmapParser(17, 30, 0.1, 1.0, True, False)
    for scales in ((2, 0.5), (1, 1), (2, 1, 0.5, 0.75, 1.5)):
        with pytest.raises(ValueError):
            inference.multi_scale_batch_inference(None, parser, [img], 640, scales, ags=True)
    with pytest.raises(ValueError, match="multiple of 32"):
        inference.multi_scale_batch_inference(None, parser, [img], 640, (1.01, 1), ags=True)
    with pytest.raises(ValueError, match="batch_size"):
        inference.multi_scale_batch_inference(None, parser, [img], 640, (2, 1, 0.5), batch_size=0, ags=True)
    assert parser.tag_per_joint                  # refused before the parser was touched
    # a parser without per-joint tags is accepted with ags=True (the pipeline is reached) ...
    for p in (no_tpj, parser):
        with pytest.raises(AssertionError, match="GPU work"):
            inference.multi_scale_batch_inference(None, p, [img], 640, (2, 1, 0.5), ags=True)
        assert p.tag_per_joint is False          # ... and, as the per-image call, the flag is set on the caller's parser
    with pytest.raises(AssertionError, match="GPU work"):
        inference.flip_test_inference(None, HeatmapParser(17, 30, 0.1, 1.0, True, False, tag_per_joint=False), [img],
                                      640, ags=True)
    # ... and refused without it
    with pytest.raises(ValueError, match="tag_per_joint"):
        inference.multi_scale_batch_inference(None, no_tpj, [img], 640, (2, 1, 0.5))


def test_ags_pipeline_needs_scale_factors():
    from rtpe.engine import TeacherPipeline
    for kw in (dict(), dict(flip_test=True)):
        with pytest.raises(ValueError, match="scale_factors"):
            TeacherPipeline(None, device="cuda:0", ags=True, **kw)


def test_ags_decode_kernels_do_not_spill(built, tmp_path):
    from test_flip_decode_host import _device_code
    dis = _device_code(built, tmp_path, "decode.hip")
    bodies = re.split(r"\n(?=[0-9a-f]+ <)", dis)
    ags = [b for b in bodies if re.match(r"[0-9a-f]+ <\S*(AgsTag|ags_prep_kernel)", b)]
    names = [b.split("<", 1)[1].split(">", 1)[0] for b in ags]
    assert sum("ags_prep_kernel" in n for n in names) == 2
    for kernel in ("topk_merge_kernel", "refine_shortcut_kernel", "refine_scan_kernel"):
        assert any(kernel in n and "AgsTag" in n for n in names), kernel
    assert any("topk_merge_kernel" in n and "MultiScaleHeatMap" in n and "AgsTag" in n for n in names)
    for n, b in zip(names, ags):
        assert "scratch_" not in b, n + ": registers spilled to scratch memory"
