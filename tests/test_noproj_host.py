"""CPU tests of the multi-scale / flip test without projection to the image (``project2image=False``): the ABI of the
new entries (their own header, the binding's table), the bytes of the maps buffer against the documented closed form,
the refusals of every entry before any launch, the Python refusals with the native library out of reach, the
``[w2_0, h2_0]`` affine of the batched drivers against ``transforms.get_final_preds``, and the compiled kernels' use of
scratch memory read from the code object's metadata."""
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


def _arr(*v):
    return (ctypes.c_int32 * len(v))(*v)


NEW_SYMBOLS = {"rtpe_ms_np_maps_bytes", "rtpe_ms_np_prep", "rtpe_topk_ms_np", "rtpe_adjust_refine_ms_np",
               "rtpe_adjust_refine_ms_np_n"}


def _declared(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_noproj_symbols_are_declared_in_their_header_and_resolve(built):
    main = _declared("rtpe_hip.h")
    assert len(re.findall(r'#include "rtpe_hip_noproj.h"', main)) == 1
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", _declared("rtpe_hip_noproj.h")))
    assert declared == NEW_SYMBOLS == set(built.EXPORTS_NOPROJ)
    older = (built.EXPORTS, built.EXPORTS_SIZES, built.EXPORTS_WARP, built.EXPORTS_SHARED, built.EXPORTS_PAIR,
             built.EXPORTS_RECORDS, built.EXPORTS_TAGMEAN)
    for table in older:
        assert not declared & set(table)
    assert [len(t) for t in older] == [59, 5, 3, 3, 1, 2, 6]
    assert not declared & set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", main))
    lib = built.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == built._SIGS_NOPROJ[name][1], name
    # the `_ms` entries' arguments, the decode size dropped where there was one
    ms = built._SIGS["rtpe_adjust_refine_ms"][1]
    assert built._SIGS_NOPROJ["rtpe_ms_np_prep"][1] == built._SIGS["rtpe_ms_prep"][1]
    assert len(built._SIGS_NOPROJ["rtpe_adjust_refine_ms_np"][1]) == len(ms) - 2
    assert len(built._SIGS_NOPROJ["rtpe_adjust_refine_ms_np_n"][1]) == len(ms) - 1
    assert len(built._SIGS_NOPROJ["rtpe_topk_ms_np"][1]) == len(built._SIGS["rtpe_topk_ms"][1]) - 2
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4


# ---- bytes -----------------------------------------------------------------------------------------------------------------
def _closed_form(N, J, h2, w2, base, flip):
    """F at r_0, T_o [and T_f] at the refined size of scale 1, H_i of every later scale at its own"""
    later = sum(h * w for h, w in list(zip(h2, w2))[1:])
    return 4 * N * J * (h2[0] * w2[0] + (1 + flip) * h2[base] * w2[base] + later)


def test_maps_bytes_closed_form(built):
    L = built.lib()
    nb = ctypes.c_size_t()

    def size(N, J, h2, w2, base, flip):
        built.check(L.rtpe_ms_np_maps_bytes(N, J, len(h2), _arr(*h2), _arr(*w2), base, flip, ctypes.byref(nb)))
        assert nb.value == _closed_form(N, J, h2, w2, base, flip)
        return nb.value
    # the bench shape: batch 32 at 640 x 640, (2, 1, 0.5): refined sizes 640, 320, 160; the projected protocol's
    # buffer (rtpe_ms_maps_bytes) is 2,785,280,000 bytes with flip
    s3 = (640, 320, 160)
    assert size(32, 17, s3, s3, 1, 1) == 4 * 544 * (409600 + 2 * 102400 + 102400 + 25600) == 1_615_462_400
    assert size(32, 17, s3, s3, 1, 0) == 4 * 544 * (409600 + 102400 + 102400 + 25600) == 1_392_640_000
    # (1,): F and the tags at (320, 320); the projected flip test's buffer (rtpe_flip_maps_bytes) is 891,289,600 bytes
    assert size(32, 17, (320,), (320,), 0, 1) == 4 * 544 * 3 * 102400 == 668_467_200
    assert size(32, 17, (320,), (320,), 0, 0) == 4 * 544 * 2 * 102400 == 445_644_800
    ms, fl = ctypes.c_size_t(), ctypes.c_size_t()
    built.check(L.rtpe_ms_maps_bytes(32, 17, 3, _arr(*s3), _arr(*s3), 1, 1, ctypes.byref(ms)))
    built.check(L.rtpe_flip_maps_bytes(32, 17, 320, 320, ctypes.byref(fl)))
    assert ms.value == 2_785_280_000 and fl.value == 891_289_600
    # ragged sizes, scale 1 first and scale 1 last
    assert size(3, 17, (80, 40), (112, 56), 0, 1) == 4 * 51 * (3 * 80 * 112 + 40 * 56)
    assert size(3, 17, (160, 80), (224, 112), 1, 1) == 4 * 51 * (160 * 224 + 3 * 80 * 112)


def test_maps_bytes_refuses_bad_arguments(built):
    L = built.lib()
    nb = ctypes.c_size_t()
    h2 = w2 = _arr(640, 320, 160)
    for args in ((32, 17, 5, _arr(*[8] * 5), _arr(*[8] * 5), 1, 1),         # S > 4
                 (32, 17, 3, h2, w2, 3, 1), (32, 17, 3, h2, w2, -1, 1),      # scale 1 missing
                 (32, 17, 0, h2, w2, 0, 1), (32, 33, 3, h2, w2, 1, 1),       # no scale; J > 32
                 (0, 17, 3, h2, w2, 1, 1), (32, 0, 3, h2, w2, 1, 1),
                 (32, 17, 3, _arr(640, 0, 160), w2, 1, 1), (32, 17, 3, h2, _arr(640, 320, -160), 1, 1),
                 (4000, 17, 3, h2, w2, 1, 1), (32, 17, 3, h2, w2, 1, 2),
                 (32, 17, 3, None, w2, 1, 1), (32, 17, 3, h2, None, 1, 1)):
        with pytest.raises(RuntimeError):
            built.check(L.rtpe_ms_np_maps_bytes(*args, ctypes.byref(nb)))
    with pytest.raises(RuntimeError):
        built.check(L.rtpe_ms_np_maps_bytes(32, 17, 3, h2, w2, 1, 1, None))


# ---- refusals before any launch ------------------------------------------------------------------------------------------
def test_entries_check_their_arguments_before_any_launch(built):
    """negative codes; nothing is launched: the pointers are never read (there is no GPU here)"""
    L = built.lib()
    h2, w2 = _arr(32, 16), _arr(48, 24)
    nb = ctypes.c_size_t()
    built.check(L.rtpe_ms_np_maps_bytes(2, 17, 2, h2, w2, 0, 0, ctypes.byref(nb)))
    assert nb.value == 4 * 2 * 17 * (2 * 32 * 48 + 16 * 24)
    fake = ctypes.c_void_p(0x1000)
    perm = _arr(*range(17))

    def prep(scale=1, n0=0, n=2, maps_bytes=nb.value, flip=0, N=2, S=2, base=0, J=17, maps=fake, preds=fake, refined=fake,
             st=17 * 16 * 24, h4=8, hs=h2):
        return L.rtpe_ms_np_prep(preds, h4, 12, 2 * 17 * 8 * 12, refined, st, fake, 2 * 17 * 8 * 12, fake, 17 * 16 * 24,
                                 n0, n, N, J, perm, S, hs, w2, base, flip, scale, maps, maps_bytes, None)
    for kw in (dict(scale=2), dict(scale=-1), dict(n0=1, n=2), dict(n0=-1), dict(n=0), dict(n0=2, n=1),
               dict(maps_bytes=nb.value - 4), dict(N=0), dict(S=5), dict(S=0), dict(base=2), dict(base=-1), dict(J=33),
               dict(J=0), dict(flip=1),                  # (the buffer was sized without the mirror image's tag maps)
               dict(flip=2), dict(maps=None), dict(preds=None), dict(refined=None), dict(st=17 * 16 * 24 - 1),
               dict(h4=0), dict(hs=_arr(32, 0)), dict(hs=None)):
        assert prep(**kw) < 0, kw
    val = ctypes.c_void_p(0x2000)

    def topk(K=30, maps_bytes=nb.value, maps=fake, ksize=5, tables=val, S=2, base=0, J=17, hs=h2, scratch=fake):
        return L.rtpe_topk_ms_np(maps, 2, J, S, hs, w2, base, 0, K, ksize, 2, tables, val, val, maps_bytes, scratch,
                                 1 << 30, None)
    for kw in (dict(K=0), dict(maps_bytes=nb.value - 4), dict(maps=None), dict(ksize=4), dict(tables=None), dict(S=5),
               dict(base=2), dict(J=33), dict(hs=_arr(0, 16)), dict(hs=None), dict(scratch=None)):
        assert topk(**kw) < 0, kw

    def refine(maps_bytes=nb.value, table=(val, val, 30), ans_out=fake, tail=(), S=2, base=0, J=17, maps=fake):
        fn = L.rtpe_adjust_refine_ms_np_n if tail else L.rtpe_adjust_refine_ms_np
        return fn(maps, 2, J, S, h2, w2, base, 0, maps_bytes, val, ans_out, val, 1, 1, 1, val, *table, fake, 1 << 30,
                  None, *tail)
    for kw in (dict(maps_bytes=nb.value - 4), dict(table=(val, None, 30)), dict(table=(val, val, 0)), dict(ans_out=val),
               dict(S=5), dict(base=2), dict(J=33), dict(maps=None), dict(tail=(None,)), dict(tail=(val,), S=5),
               dict(tail=(val,), maps_bytes=8)):
        assert refine(**kw) < 0, kw
    # P == 0: nothing to do, nothing launched
    built.check(L.rtpe_adjust_refine_ms_np(fake, 2, 17, 2, h2, w2, 0, 0, nb.value, None, None, None, 0, 1, 1, None,
                                           None, None, 0, None, 0, None))


# ---- the keyword -----------------------------------------------------------------------------------------------------------
def test_python_refusals_hold_without_the_native_library(monkeypatch):
    from rtpe import _native, engine, inference
    from rtpe.third_party.group import HeatmapParser

    def no_lib():
        raise AssertionError("native library")
    monkeypatch.setattr(_native, "lib", no_lib)
    seen = []

    class NoGpu:
        def __init__(self, *a, **k):
            seen.append(k)
            raise AssertionError("GPU work")
    img = np.zeros((480, 640, 3), np.uint8)
    parser = HeatmapParser(17, 30, 0.1, 1.0, True, False)
    hw3 = [(128, 192), (64, 96), (32, 48)]
    for ags in (True, "first", "mean"):
        with pytest.raises(ValueError, match="ags"):
            parser.parse_multi_scale(None, None, (1,), True, ags=ags, project2image=False)
        with pytest.raises(ValueError, match="ags"):
            parser.ms_begin(2, hw3, None, (2, 1, 0.5), True, ags=ags, project2image=False)
        with pytest.raises(ValueError, match="ags"):
            engine.TeacherPipeline(None, parser, device="cuda:0", scale_factors=(2, 1, 0.5), ags=ags,
                                   project2image=False)
    for out_hw in ((64, 96), (256, 384), (128, 191)):                   # not r_0 = (128, 192)
        with pytest.raises(ValueError, match="decode grid"):
            parser.ms_begin(2, hw3, out_hw, (2, 1, 0.5), True, project2image=False)
    with pytest.raises(ValueError, match="contain 1"):                  # scale 1 missing
        parser.ms_begin(2, hw3, None, (2, 1.5, 0.5), True, project2image=False)
    with pytest.raises(ValueError, match="at most 4"):
        parser.ms_begin(2, hw3 + [(16, 24), (8, 12)], None, (4, 2, 1, 0.5, 0.25), True, project2image=False)
    with pytest.raises(ValueError, match="scale_factors"):
        engine.TeacherPipeline(None, parser, device="cuda:0", flip_test=True, project2image=False)
    with pytest.raises(ValueError):
        engine.StudentPipeline(None, parser, device="cuda:0", project2image=False)
    monkeypatch.setattr(engine, "TeacherPipeline", NoGpu)
    for ags in (True, "mean"):
        with pytest.raises(ValueError, match="ags"):
            inference.multi_scale_batch_inference(None, parser, [img], 640, (2, 1, 0.5), ags=ags, project2image=False)
        with pytest.raises(ValueError, match="ags"):
            inference.flip_test_inference(None, parser, [img], 640, ags=ags, project2image=False)
    with pytest.raises(ValueError):
        inference.multi_scale_batch_inference(None, parser, [img], 640, (2, 0.5), project2image=False)
    with pytest.raises(ValueError, match="at most 4"):
        inference.multi_scale_batch_inference(None, parser, [img], 640, (4, 3, 2, 1, 0.5), project2image=False)
    assert not seen and parser.tag_per_joint
    # what is not refused reaches the pipeline with the keyword; the default does not pass it
    with pytest.raises(AssertionError, match="GPU work"):
        inference.flip_test_inference(None, parser, [img], 640, project2image=False)
    assert seen.pop()["project2image"] is False and seen == []
    with pytest.raises(AssertionError, match="GPU work"):
        inference.multi_scale_batch_inference(None, parser, [img], 640, (2, 1, 0.5))
    assert "project2image" not in seen.pop()


def test_pipeline_refuses_another_decode_size_before_any_gpu_work():
    from rtpe import engine
    from rtpe.third_party.group import HeatmapParser

    class Model(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("GPU work")
    parser = HeatmapParser(17, 30, 0.1, 1.0, True, False)
    pipe = engine.TeacherPipeline(Model(), parser, device="cpu", flip_test=True, scale_factors=(2, 1),
                                  project2image=False)
    xs = [torch.zeros((2, 3, 256, 384)), torch.zeros((2, 3, 128, 192))]
    for out_hw in ((256, 384), (64, 96), (128, 190)):
        with pytest.raises(ValueError, match="decode grid"):
            pipe(xs, out_hw=out_hw)
    with pytest.raises(ValueError, match="per-image"):
        pipe(xs, out_hw=[(128, 192), (128, 192)])
    assert pipe._decode_hw((128, 192), xs) == (128, 192) and pipe._decode_hw(None, xs) is None


# ---- the drivers' affine ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scales", [(2, 1, 0.5), (1,), (1, 0.5)])
def test_drivers_map_back_from_the_heat_map_grid_of_the_largest_scale(monkeypatch, scales):
    """a stand-in pipeline hands out fixed people in heat-map pixels; the drivers must map them back with
    ``get_final_preds(., centre, scale, [w2_0, h2_0])`` - the size of the largest scale's heat map - with the centre /
    scale of the last (smallest) scale's warp, ask the pipeline for no other decode size, and build the records'
    ``xform`` from the same three"""
    from rtpe import engine, inference
    from rtpe.third_party import transforms
    from rtpe.third_party.group import HeatmapParser
    shapes = [(120, 160), (150, 200), (120, 160), (200, 150)]
    images = [np.zeros(s + (3,), np.uint8) for s in shapes]
    rng = np.random.default_rng(3)
    people = rng.uniform(0, 60, (2, 17, 5)).astype(np.float32)
    asked = []

    def warp_normalize(image, input_size, s, lo, device=None):
        (w, h), center, scale = transforms.get_multi_scale_size(image, input_size, s, lo)
        return torch.zeros((1, 3, h, w)), center, scale

    class Pipe:
        device = torch.device("cpu")

        def __init__(self, model, parser, **kw):
            assert kw["project2image"] is False and kw["scale_factors"] == tuple(sorted(scales, reverse=True))

        def stream(self, batches, out_hw=None, records=None):
            for k, xs in enumerate(batches):
                asked.append((out_hw, tuple(xs[0].shape[2:])))
                if records is not None:
                    yield records(k)
                else:
                    yield [(people, [np.float32(1)] * 2)] * xs[0].shape[0]
    monkeypatch.setattr(engine, "TeacherPipeline", Pipe)
    monkeypatch.setattr(transforms, "warp_normalize", warp_normalize)
    parser = HeatmapParser(17, 30, 0.1, 1.0, True, False, match_on="device")
    order = tuple(sorted(scales, reverse=True))
    got = inference.multi_scale_batch_inference(None, parser, images, 128, scales, True, batch_size=2,
                                                project2image=False)
    assert len(got) == 4 and asked
    for out_hw, in_hw in asked:
        assert out_hw == (in_hw[0] // 2, in_hw[1] // 2)             # r_0: half the largest scale's input
    for img, (final, _) in zip(images, got):
        (w0, h0), _, _ = transforms.get_multi_scale_size(img, 128, order[0], min(order))
        _, center, scale = transforms.get_multi_scale_size(img, 128, min(order), min(order))
        want = transforms.get_final_preds([people], center, scale, [w0 // 2, h0 // 2])
        assert len(final) == len(want) == 2
        for a, b in zip(final, want):
            assert np.array_equal(a, b)
        # (the projected protocol takes another size: the check has teeth)
        other = transforms.get_final_preds([people], center, scale, [w0, h0])
        assert not np.array_equal(final[0], other[0])
    # the records' xform: the same matrix (the stand-in hands the callback's answer through)
    seen = []
    monkeypatch.setattr(inference, "_in_input_order", lambda recs, order_, n, dev: seen.append((recs, order_)))
    inference.multi_scale_batch_inference(None, parser, images, 128, scales, True, batch_size=2,
                                          image_ids=[3, 2, 1, 0], project2image=False)
    (recs, rows), = seen
    flat = [(i, x) for ids, xf in recs for i, x in zip(ids, xf)]
    assert sorted(rows) == [0, 1, 2, 3] and len(flat) == 4
    for r, (image_id, xf) in zip(rows, flat):
        img = images[r]
        assert image_id == [3, 2, 1, 0][r]
        (w0, h0), _, _ = transforms.get_multi_scale_size(img, 128, order[0], min(order))
        _, center, scale = transforms.get_multi_scale_size(img, 128, min(order), min(order))
        assert np.array_equal(xf, transforms.final_preds_matrix(center, scale, [w0 // 2, h0 // 2]))


# ---- the compiled kernels --------------------------------------------------------------------------------------------------
def test_noproj_kernels_use_no_scratch_memory(built, tmp_path):
    """the kernel descriptors' metadata of the gfx950 code object (what tools/kernel_regs.sh prints): the new kernels -
    the flip-averaging prep, the in-place accumulate, and the decode stages instantiated for a dense heat map with the
    tag planes at their own resolution - have no private segment and spill no vector register"""
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin/"
    name = "decode.hip"
    obj = shutil.copy(os.path.join(os.path.dirname(built.LIB_PATH), "build", name + ".o"), str(tmp_path / (name + ".o")))
    fat, co = str(tmp_path / (name + ".fatbin")), str(tmp_path / (name + ".co"))
    subprocess.run([llvm + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj, str(tmp_path / "x.o")], check=True)
    subprocess.run([llvm + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + fat, "--output=" + co], check=True)
    notes = subprocess.run([llvm + "llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        m = re.search(r"\.name:\s+(\S+)", block)
        kernels[m.group(1)] = {k: int(v) for k, v in re.findall(
            r"\.(private_segment_fixed_size|vgpr_spill_count|vgpr_count):\s+(\d+)", block)}
    mine = {n: v for n, v in kernels.items()
            if "np_prep_kernel" in n or "np_accum_kernel" in n or ("DirectMap" in n and "FlipTag" in n)}
    assert sum("np_prep_kernel" in n for n in mine) == 2 and sum("np_accum_kernel" in n for n in mine) == 2
    for stage in ("topk_merge_kernel", "refine_scan_kernel"):
        assert any(stage in n for n in mine), stage
    for n, v in mine.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (n, v)
    # the prep of the projected multi-scale test keeps its four instantiations: the flip average is a kernel of its own
    assert sum("ms_prep_kernel" in n for n in kernels) == 4
