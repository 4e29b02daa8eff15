"""CPU tests of the per-image decode size (every image of a batch decoded at its own (h, w)): the ABI of the new
entries, the sizes table the host function fills, the checks of the entries, the refusals raised before any GPU work,
the batches ``plain_inference`` forms, and the compiled kernels (no registers spilled to scratch memory)."""
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


NEW_SYMBOLS = ("rtpe_decode_sizes_bytes", "rtpe_decode_sizes_fill", "rtpe_topk_fused_sizes",
               "rtpe_adjust_refine_fused_topk_sizes", "rtpe_adjust_refine_fused_topk_sizes_n")


def _declared(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_sizes_symbols_are_declared_and_resolve(built):
    """the new prototypes live in include/rtpe_hip_sizes.h, which rtpe_hip.h includes; the binding lists them in
    EXPORTS_SIZES and resolves them with the others"""
    main = _declared("rtpe_hip.h")
    assert re.search(r'#include "rtpe_hip_sizes.h"', main)
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", _declared("rtpe_hip_sizes.h")))
    assert declared == set(NEW_SYMBOLS) == set(built.EXPORTS_SIZES)
    assert not declared & set(built.EXPORTS)
    lib = built.lib()
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.argtypes == built._SIGS_SIZES[name][1], name
    sizes = built._SIGS_SIZES
    for plain in ("rtpe_topk_fused", "rtpe_adjust_refine_fused_topk"):      # (oh, ow) -> the five size arguments
        assert len(sizes[plain + "_sizes"][1]) == len(built._SIGS[plain][1]) + 3
    assert sizes["rtpe_adjust_refine_fused_topk_sizes_n"][1][:-1] == sizes["rtpe_adjust_refine_fused_topk_sizes"][1]
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4


def _fill(built, sizes, hh, hw, th, tw, table_bytes=None):
    L = built.lib()
    N = len(sizes)
    nb = ctypes.c_size_t()
    built.check(L.rtpe_decode_sizes_bytes(N, ctypes.byref(nb)))
    assert nb.value == 64 * N
    tab = np.full((N, 16), -1, np.int32)
    flat = (ctypes.c_int32 * (2 * N))(*[v for s in sizes for v in s])
    mh, mw = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = L.rtpe_decode_sizes_fill(flat, N, hh, hw, th, tw, tab.ctypes.data, nb.value if table_bytes is None else table_bytes,
                                  ctypes.byref(mh), ctypes.byref(mw))
    return rc, tab, mh.value, mw.value


def test_sizes_table_is_filled_on_the_host_with_the_samplers_axes(built):
    """no GPU: the table is host memory.  Its axis entries are make_axis's: float32(n_in - 1) / float32(n_out - 1),
    0 for n_out == 1, and the `same` flag where the sizes agree - per axis, per map"""
    hh, hw, th, tw = 128, 160, 64, 80
    sizes = [(128, 80), (1, 1), (256, 320), (100, 333), (64, 160), (31, 47), (300, 70), (427, 640), (128, 160), (64, 80)]
    rc, tab, mh, mw = _fill(built, sizes, hh, hw, th, tw)
    assert rc == 0 and (mh, mw) == (427, 640)
    f = tab.view(np.float32)
    for n, (oh, ow) in enumerate(sizes):
        assert tuple(tab[n, :2]) == (oh, ow) and tuple(tab[n, 14:]) == (int(oh + ow <= 128), 0)
        for word, n_in, n_out in ((2, hh, oh), (5, hw, ow), (8, th, oh), (11, tw, ow)):
            want = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
            assert f[n, word].tobytes() == np.float32(want).tobytes(), (n, word)
            assert tab[n, word + 1] == n_in and tab[n, word + 2] == int(n_in == n_out), (n, word)
    assert tab[0, 4] == 1 and tab[0, 7] == 0 and tab[0, 10] == 0 and tab[0, 13] == 1      # oh == hh, ow == tw only
    # its checks: a non-positive size, a table that is too small, null pointers
    for bad in ([(128, 0)], [(128, 160), (-1, 5)]):
        assert _fill(built, bad, hh, hw, th, tw)[0] < 0
    assert _fill(built, sizes, hh, hw, th, tw, table_bytes=64 * len(sizes) - 1)[0] < 0
    assert _fill(built, sizes, 0, hw, th, tw)[0] < 0
    L = built.lib()
    assert L.rtpe_decode_sizes_fill(None, 1, hh, hw, th, tw, tab.ctypes.data, 64, None, None) < 0
    assert L.rtpe_decode_sizes_fill(tab.ctypes.data, 1, hh, hw, th, tw, None, 64, None, None) < 0
    assert L.rtpe_decode_sizes_bytes(0, ctypes.byref(ctypes.c_size_t())) < 0
    assert L.rtpe_decode_sizes_bytes(4, None) < 0


def test_sizes_entries_check_their_arguments_before_any_launch(built):
    """bad arguments come back as negative codes (no launch: the pointers are never read)"""
    L = built.lib()
    fake, val = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)

    def topk(hm=fake, tab=fake, table_bytes=2 * 64, max_oh=427, max_ow=640, w_enc=640, K=30, out=val, scratch=fake,
             scratch_bytes=1 << 30, N=2, ksize=5, pad=2):
        return L.rtpe_topk_fused_sizes(hm, 320, 448, 17 * 320 * 448, fake, 160, 224, 34 * 160 * 224, N, 17, tab,
                                       table_bytes, max_oh, max_ow, w_enc, K, ksize, pad, out, val, val, scratch,
                                       scratch_bytes, None)

    def refine(n=False, hm=fake, tab=fake, table_bytes=2 * 64, max_oh=427, max_ow=640, w_enc=640, P=3, ans_out=fake,
               topk_val=val, K=30, p_dev=fake):
        args = (hm, 320, 448, 17 * 320 * 448, fake, 160, 224, 34 * 160 * 224, 2, 17, tab, table_bytes, max_oh, max_ow,
                w_enc, val, ans_out, val, P, 1, 1, val, topk_val, val if topk_val else None, K, fake, 16, None)
        if n:
            return L.rtpe_adjust_refine_fused_topk_sizes_n(*args, p_dev)
        return L.rtpe_adjust_refine_fused_topk_sizes(*args)
    nb = ctypes.c_size_t()
    built.check(L.rtpe_topk_scratch_bytes(2 * 17, 427, 640, 30, ctypes.byref(nb)))
    bad = (dict(hm=None), dict(tab=None), dict(table_bytes=2 * 64 - 1), dict(max_oh=0), dict(max_ow=-3),
           dict(w_enc=639), dict(max_oh=40000, w_enc=60000),          # y * w_enc + x beyond int32
           dict(N=0))
    for kw in bad + (dict(K=0), dict(out=None), dict(scratch=None), dict(scratch_bytes=nb.value - 8),
                     dict(ksize=4), dict(pad=5, ksize=11)):
        assert topk(**kw) < 0, kw
        assert b"topk" in L.rtpe_last_error_string() or b"nms" in L.rtpe_last_error_string()
    for n in (False, True):
        for kw in bad[:-1] + (dict(ans_out=val), dict(topk_val=None), dict(K=0)):
            assert refine(n, **kw) < 0, (n, kw)
        # the scratch of 16 bytes is refused too - after every argument check, before the first launch
        assert refine(n) < 0 and b"scratch too small" in L.rtpe_last_error_string()
    assert refine(True, p_dev=None) < 0
    # P == 0: nothing to do, nothing launched
    built.check(refine(False, P=0))


def test_parse_lowres_checks_the_sizes_before_any_gpu_work():
    """CPU tensors: a call that got as far as the GPU check raises RuntimeError, a refused size list ValueError"""
    from rtpe.third_party.group import HeatmapParser, per_image_sizes
    hp = HeatmapParser(17, 30, 0.1, 1.0, True, False)
    refined, tags = torch.zeros((3, 17, 32, 32)), torch.zeros((3, 17, 16, 16))
    for bad in ([(64, 64)] * 2, [(64, 64)] * 4, [(64, 64), (64, 0), (64, 64)], [(64, 64), (-1, 64), (64, 64)],
                [(64, 64), (64.5, 64), (64, 64)], [(64, 64), (64, 64, 3), (64, 64)], [(64, 64), 64, (64, 64)]):
        with pytest.raises(ValueError):
            hp.parse_lowres(refined, tags, bad)
        with pytest.raises(ValueError):
            hp.lowres_topk(refined, tags, bad)
    for ok in ((64, 64), [(64, 64), (31, 47), (100, 20)]):              # accepted: stopped by the missing GPU
        with pytest.raises(RuntimeError, match="HIP path only"):
            hp.parse_lowres(refined, tags, ok)
    assert per_image_sizes((64, 48), 5) is None and per_image_sizes(torch.Size([64, 48]), 2) is None
    assert per_image_sizes([np.array([64, 48]), (np.int64(3), 5)], 2) == [(64, 48), (3, 5)]
    assert per_image_sizes([(64, 48), (3, 5)], 2) == [(64, 48), (3, 5)]     # N == 2: two pairs, not one (h, w)


class _NoForward(torch.nn.Module):
    def forward(self, x):
        raise AssertionError("GPU work")


def test_pipeline_checks_the_sizes_before_any_gpu_work():
    """(``stream()`` asks for the device's streams first: its refusals are in the GPU tests)"""
    from rtpe.engine import TeacherPipeline
    x = torch.zeros((2, 3, 64, 64))
    sizes = [(60, 64), (64, 50)]
    pipe = TeacherPipeline(_NoForward(), device="cpu")
    for bad in ([(60, 64)], [(60, 64)] * 3, [(60, 64), (0, 64)], [(60, 64), (1.5, 64)]):
        with pytest.raises(ValueError):
            pipe(x, bad)
    for good in (sizes, (60, 64), None):                                 # accepted: the forward is reached
        with pytest.raises(AssertionError, match="GPU work"):
            pipe(x, good)
    for kw, images in ((dict(flip_test=True), x), (dict(scale_factors=(1,)), [x]), (dict(scale_factors=(2, 1)), [x, x]),
                       (dict(scale_factors=(1,), flip_test=True, ags=True), [x])):
        pipe = TeacherPipeline(_NoForward(), device="cpu", **kw)
        with pytest.raises(ValueError, match="per-image decode sizes"):
            pipe(images, sizes)


def _mix():
    """the seeded mix of 256 COCO-like sizes (h, w): 70 % landscape, 20 % portrait, 10 % width 500"""
    rng = np.random.default_rng(2017)
    sizes = []
    for _ in range(256):
        r = rng.uniform()
        if r < 0.7:
            sizes.append((int(rng.integers(360, 481)), 640))
        elif r < 0.9:
            sizes.append((640, int(rng.integers(360, 481))))
        else:
            sizes.append((int(rng.integers(300, 401)), 500))
    return sizes


class _Img:
    """an image the fake pipeline never reads: only its shape"""

    def __init__(self, h, w):
        self.shape = (h, w, 3)


def _recording_pipeline(monkeypatch, log):
    """TeacherPipeline and the warp replaced: a "warped image" is a (1,1,1,4) tensor [h, w, H, W] - the original size
    of the image it was made from and its network input size - so a batch tells which images it holds"""
    from rtpe import engine
    from rtpe.third_party import transforms

    def warp(img, input_size, s, lo, device=None):
        (w, h), center, scale = transforms.get_multi_scale_size(img, input_size, s, lo)
        return torch.tensor([[[[img.shape[0], img.shape[1], h, w]]]]), center, scale

    class Recorder:
        def __init__(self, model, parser, device=None, **kw):
            self.device = device
            log.append(("init", kw))

        def stream(self, batches, out_hw=None):
            for k, x in enumerate(batches):
                rows = [tuple(int(v) for v in r) for r in x[:, 0, 0]]
                log.append(("batch", rows, [tuple(s) for s in out_hw(k)]))
                yield [("people of", r[:2]) for r in rows]
    monkeypatch.setattr(engine, "TeacherPipeline", Recorder)
    monkeypatch.setattr(transforms, "warp_normalize", warp)


def test_plain_inference_batches_by_input_size_only(monkeypatch):
    from rtpe import inference
    from rtpe.engine import MAX_FORWARD_PIXELS
    from rtpe.third_party import transforms
    log = []
    _recording_pipeline(monkeypatch, log)
    shapes = _mix()
    images = [_Img(h, w) for h, w in shapes]
    inputs = [transforms.get_multi_scale_size(img, 640, 1.0, 1)[0] for img in images]
    one = max(w * h for w, h in inputs)           # the largest input fits, no two of the smallest do
    assert 2 * min(w * h for w, h in inputs) > one
    for batch_size, budget in ((32, 1 << 40), (32, None), (7, None), (32, one)):
        del log[:]
        out = inference.plain_inference(None, None, images, 640, batch_size, budget, device="cpu", match_on="device")
        assert log[0] == ("init", {"match_on": "device"})
        batches = log[1:]
        assert out == [("people of", s) for s in shapes]                 # results in input order
        for _, rows, hw in batches:
            assert hw == [r[:2] for r in rows]                           # image n of the batch with ITS (h, w)
            assert len({r[2:] for r in rows}) == 1                       # one network input size per batch
            assert len(rows) <= batch_size
            assert len(rows) * rows[0][2] * rows[0][3] <= (MAX_FORWARD_PIXELS if budget is None else budget)
        assert sum(len(b[1]) for b in batches) == 256
        if budget == 1 << 40:
            assert len(batches) == 15                                    # 11 input sizes, 156 original sizes
            assert len({b[1][0][2:] for b in batches}) == 11
        if budget == one:
            assert all(len(b[1]) == 1 for b in batches)                  # no two images fit: every forward takes one
    # the plan alone, without and with the original size in the key - what a decode with ONE size per batch needs
    assert len(set(shapes)) == 156
    plan = inference.plain_plan(shapes, 640, 32, 1 << 40)
    assert len(plan) == 15 and sorted(i for c in plan for i in c) == list(range(256))
    assert len(inference.plain_plan(shapes, 640, 32, 1 << 40, by_original_size=True)) == 156
    a = transforms.get_multi_scale_size(_Img(480, 640), 640, 1.0, 1)[0]
    b = transforms.get_multi_scale_size(_Img(375, 500), 640, 1.0, 1)[0]
    assert a == b == (896, 640)                   # two original sizes, one input size


def test_plain_inference_refuses_before_any_gpu_work(monkeypatch):
    from rtpe import engine, inference

    class NoGpu:
        def __init__(self, *a, **k):
            raise AssertionError("GPU work")
    monkeypatch.setattr(engine, "TeacherPipeline", NoGpu)
    img = _Img(480, 640)
    with pytest.raises(ValueError, match="batch_size"):
        inference.plain_inference(None, None, [img], 640, batch_size=0)
    with pytest.raises(ValueError, match="match_on"):
        inference.plain_inference(None, None, [img], 640, match_on="gpu")
    with pytest.raises(ValueError, match="pixel budget"):
        inference.plain_inference(None, None, [img], 640, max_forward_pixels=640 * 896 - 1)
    assert inference.plain_inference(None, None, [], 640) == []
    with pytest.raises(AssertionError, match="GPU work"):
        inference.plain_inference(None, None, [img], 640)


SIZED_KERNELS = ("topk_tile_kernel", "topk_merge_kernel", "adjust_prepare_kernel", "plane_argmax_kernel",
                 "refine_shortcut_kernel", "refine_scan_kernel", "refine_finalize_kernel")


def test_sizes_decode_kernels_exist_and_do_not_spill(built, tmp_path):
    from test_flip_decode_host import _device_code
    dis = _device_code(built, tmp_path, "decode.hip")
    bodies = re.split(r"\n(?=[0-9a-f]+ <)", dis)
    mine = [b for b in bodies if re.match(r"[0-9a-f]+ <\S*(NetSizesMap|NetSizesTag)", b)]
    names = [b.split("<", 1)[1].split(">", 1)[0] for b in mine]
    for kernel in SIZED_KERNELS:
        assert any(kernel in n for n in names), kernel
    # both NMS windows of the tile kernel: the 5 x 5 instantiation (PAD = 2) and the run-time one (PAD = -1)
    assert sum("topk_tile_kernel" in n for n in names) == 2
    for n, b in zip(names, mine):
        assert "scratch_" not in b, n + ": registers spilled to scratch memory"
        assert not any(s in n for s in ("FlipHeatMap", "FlipTag", "MultiScaleHeatMap", "AgsTag"))
