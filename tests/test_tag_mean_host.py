"""CPU tests of the averaged-tag test (``ags="mean"``: every joint of an image grouped by the mean of the joints' tag
maps, the reference's legacy/valid_ae_avg.py): the float order of the mean redone against ``torch.mean`` - with the
tail of a plane, where ATen takes another order, seen and not assumed -, the ABI of the new entries (their own header,
the binding's table), their refusals before any launch, the bytes of the maps buffer, and the refusal of an unknown
``ags`` string by every entry point before any GPU work."""
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


# ---- the order, shared with tests/test_tag_mean_gpu.py ---------------------------------------------------------------
def mean_restated(x):
    """the pinned order of ``x.mean(dim=1)`` in plain numpy, x (N,C,h,w) f32 -> (N,h,w) f32: channels in blocks of 16,
    every block summed channel after channel from +0.0f, block sums added in order; the C % 16 channels behind the last
    full block summed from +0.0f on their own and added last; one true division by float32(C)"""
    x = np.asarray(x, np.float32)
    C = x.shape[1]
    zero = np.zeros(x.shape[:1] + x.shape[2:], np.float32)
    full = C // 16 * 16
    blocks = None
    for b in range(0, full, 16):
        s = zero.copy()
        for c in range(b, b + 16):
            s = s + x[:, c]
        blocks = s if blocks is None else blocks + s
    rest = zero.copy()
    for c in range(full, C):
        rest = rest + x[:, c]
    total = rest if blocks is None else rest + blocks
    out = total / np.float32(C)
    assert out.dtype == np.float32
    return out


def seeded(shape, seed):
    """3 * randn: sums of 17 such values round at almost every step, so another order changes bits"""
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 3).float()


@pytest.mark.parametrize("threads", [1, 8])
@pytest.mark.parametrize("shape", [(1, 17, 64, 64), (2, 18, 64, 96), (1, 32, 8, 64), (1, 5, 1, 32)])
def test_restatement_equals_torch_mean(shape, threads):
    before = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        x = seeded(shape, 11)
        want = x.mean(dim=1).numpy()
    finally:
        torch.set_num_threads(before)
    assert np.array_equal(mean_restated(x.numpy()).view(np.uint32), want.view(np.uint32))
    # the order matters at these values: with two or more channels behind a full block (for 17 the two orders are the
    # same sum) the plain sequential sum differs somewhere
    if shape[1] > 17:
        seq = np.zeros_like(want)
        for c in range(shape[1]):
            seq = seq + x.numpy()[:, c]
        assert not np.array_equal(seq / np.float32(shape[1]), want)


FIT_CHANNELS = [1, 2, 5, 15, 16, 17, 18, 31, 32, 33, 34, 47, 48, 49, 64, 65, 100, 128, 255, 256, 257, 271, 272]


@pytest.mark.parametrize("C", FIT_CHANNELS)
def test_fit_of_the_order_over_the_accepted_channel_counts(C):
    """the fit the documents rest on: N in {1, 2}, 1 and 8 threads, contiguous tensors and a channel slice of a larger
    one (every plane a multiple of 32 pixels), up to the 272 channels the op accepts"""
    before = torch.get_num_threads()
    try:
        for threads in (1, 8):
            torch.set_num_threads(threads)
            for k, shape in enumerate(((1, C, 4, 64), (2, C, 1, 32))):
                x = seeded(shape, 100 + C + k)
                assert np.array_equal(mean_restated(x.numpy()).view(np.uint32), x.mean(dim=1).numpy().view(np.uint32))
            t = seeded((2, 2 * C + 3, 2, 32), 300 + C)[:, C + 1:2 * C + 1]
            assert t.shape[1] == C and not t.is_contiguous()
            assert np.array_equal(mean_restated(t.numpy()).view(np.uint32), t.mean(dim=1).numpy().view(np.uint32))
    finally:
        torch.set_num_threads(before)


@pytest.mark.parametrize("C", [273, 274, 288, 512])
def test_the_order_ends_at_272_channels(C):
    """from 273 channels on (more than 17 blocks of 16) ATen groups the block sums at one more level: the restatement no
    longer gives torch's bits, which is why ``channel_mean`` refuses more than ``MEAN_MAX_CHANNELS``"""
    from rtpe.third_party.group import MEAN_MAX_CHANNELS
    assert MEAN_MAX_CHANNELS == 272 == max(FIT_CHANNELS)
    x = seeded((1, C, 4, 64), 500 + C)
    want, got = x.mean(dim=1).numpy(), mean_restated(x.numpy())
    assert not np.array_equal(got, want)
    assert np.abs(got - want).max() < 1e-4                       # (another order of the same sum, nothing else)


def test_restatement_holds_below_the_tail_boundary_only():
    """(1,17,7,33): 231 pixels, the first 224 = 231 // 32 * 32 in the pinned order; ATen sends the last 7 through a
    scalar path with another order - at least one of them differs, which is why the GPU op is specified by the
    restatement and not by torch there"""
    x = seeded((1, 17, 7, 33), 12)
    want = x.mean(dim=1).numpy().reshape(-1)
    got = mean_restated(x.numpy()).reshape(-1)
    assert np.array_equal(got[:224].view(np.uint32), want[:224].view(np.uint32))
    assert (got[224:] != want[224:]).any()
    assert np.abs(got[224:] - want[224:]).max() < 1e-5          # (another order of the same sum, nothing else)


def test_restatement_signs_of_zero():
    x = np.full((1, 17, 2, 16), -0.0, np.float32)
    got = mean_restated(x)
    assert (got == 0).all() and not np.signbit(got).any()
    assert not np.signbit(torch.from_numpy(x).mean(dim=1).numpy()).any()


# ---- ABI -----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = {"rtpe_channel_mean", "rtpe_ms_mean_maps_bytes", "rtpe_ms_mean_prep", "rtpe_topk_ms_mean",
               "rtpe_adjust_refine_ms_mean", "rtpe_adjust_refine_ms_mean_n"}


def _declared(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_tagmean_symbols_are_declared_in_their_header_and_resolve(built):
    main = _declared("rtpe_hip.h")
    assert len(re.findall(r'#include "rtpe_hip_tagmean.h"', main)) == 1
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", _declared("rtpe_hip_tagmean.h")))
    assert declared == NEW_SYMBOLS == set(built.EXPORTS_TAGMEAN)
    older = (built.EXPORTS, built.EXPORTS_SIZES, built.EXPORTS_WARP, built.EXPORTS_SHARED, built.EXPORTS_PAIR,
             built.EXPORTS_RECORDS)
    for table in older:
        assert not declared & set(table)
    assert [len(t) for t in older] == [59, 5, 3, 3, 1, 2]
    assert not declared & set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", main))
    lib = built.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == built._SIGS_TAGMEAN[name][1], name
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4


def _arr(*v):
    return (ctypes.c_int32 * len(v))(*v)


# ---- bytes -----------------------------------------------------------------------------------------------------------------
def test_mean_maps_bytes_closed_form(built):
    """per scale A_o [and A_f], then the J un-mirrored tag maps of the smallest scale at its refined size, then one
    plane per image at the decode size"""
    L = built.lib()
    nb, ags = ctypes.c_size_t(), ctypes.c_size_t()
    h2 = w2 = _arr(640, 320, 160)
    # the bench shape: batch 32 at 640 x 640, W0, (2, 1, 0.5) + flip
    built.check(L.rtpe_ms_mean_maps_bytes(32, 17, 3, h2, w2, 1, 1, 640, 640, ctypes.byref(nb)))
    assert nb.value == 4 * (32 * 17 * 2 * (640 * 640 + 320 * 320 + 160 * 160) + 32 * 17 * 160 * 160 + 32 * 640 * 640)
    built.check(L.rtpe_ms_mean_maps_bytes(32, 17, 3, h2, w2, 1, 0, 640, 640, ctypes.byref(nb)))
    assert nb.value == 4 * (32 * 17 * (640 * 640 + 320 * 320 + 160 * 160) + 32 * 17 * 160 * 160 + 32 * 640 * 640)
    # single scale + flip: the tag maps are 223 MB, the planes 52 MB, on top of the 446 MB of heat maps
    built.check(L.rtpe_ms_mean_maps_bytes(32, 17, 1, _arr(320), _arr(320), 0, 1, 640, 640, ctypes.byref(nb)))
    built.check(L.rtpe_ms_ags_maps_bytes(32, 17, 1, _arr(320), _arr(320), 0, 1, ctypes.byref(ags)))
    assert nb.value == 4 * 32 * (17 * 3 * 320 * 320 + 640 * 640) == 720_896_000
    assert nb.value - ags.value == 4 * 32 * (16 * 320 * 320 + 640 * 640)
    assert 4 * 32 * 17 * 320 * 320 == 222_822_400 and 4 * 32 * 640 * 640 == 52_428_800
    # the decode size is part of the layout, and the smallest scale is the last entry whatever the sizes say
    built.check(L.rtpe_ms_mean_maps_bytes(2, 17, 2, _arr(64, 96), _arr(64, 96), 0, 0, 100, 60, ctypes.byref(nb)))
    assert nb.value == 4 * (2 * 17 * (64 * 64 + 96 * 96) + 2 * 17 * 96 * 96 + 2 * 100 * 60)
    for args in ((32, 17, 5, _arr(*[8] * 5), _arr(*[8] * 5), 1, 1, 640, 640), (32, 17, 3, h2, w2, 3, 1, 640, 640),
                 (32, 17, 0, h2, w2, 0, 1, 640, 640), (32, 33, 3, h2, w2, 1, 1, 640, 640),
                 (0, 17, 3, h2, w2, 1, 1, 640, 640), (32, 17, 3, _arr(640, 0, 160), w2, 1, 1, 640, 640),
                 (4000, 17, 3, h2, w2, 1, 1, 640, 640), (32, 17, 3, h2, w2, 1, 2, 640, 640),
                 (32, 17, 3, h2, w2, 1, 1, 0, 640), (32, 17, 3, h2, w2, 1, 1, 640, -1),
                 (32, 17, 3, h2, w2, 1, 1, 65536, 32768)):
        with pytest.raises(RuntimeError):
            built.check(L.rtpe_ms_mean_maps_bytes(*args, ctypes.byref(nb)))
    with pytest.raises(RuntimeError):
        built.check(L.rtpe_ms_mean_maps_bytes(32, 17, 3, h2, w2, 1, 1, 640, 640, None))


# ---- refusals before any launch ------------------------------------------------------------------------------------------
def test_channel_mean_refuses_bad_arguments_before_any_launch(built):
    """negative codes and a message; nothing is launched: the pointers are never read (there is no GPU here)"""
    L = built.lib()
    fake = ctypes.c_void_p(0x1000)
    good = dict(x=fake, N=2, C=17, h=8, w=12, img=34 * 96, ch=96, out=fake, stream=None)

    def call(**kw):
        return L.rtpe_channel_mean(*dict(good, **kw).values())
    for kw in (dict(x=None), dict(out=None), dict(N=0), dict(N=-2), dict(N=65536), dict(C=0), dict(C=273, img=273 * 96), dict(C=4096, img=4096 * 96), dict(h=0),
               dict(w=-1), dict(h=65536, w=65536, ch=1 << 40, img=1 << 50), dict(ch=95), dict(ch=0),
               dict(img=16 * 96 + 95), dict(img=0), dict(ch=200, img=17 * 96)):
        assert call(**kw) < 0, kw
        assert b"channel_mean" in L.rtpe_last_error_string(), kw
    assert call(C=273, img=273 * 96) < 0 and b"C <= 272" in L.rtpe_last_error_string()


def test_ms_mean_entries_check_their_arguments_before_any_launch(built):
    L = built.lib()
    h2, w2 = _arr(32, 16), _arr(48, 24)
    nb = ctypes.c_size_t()
    built.check(L.rtpe_ms_mean_maps_bytes(2, 17, 2, h2, w2, 0, 0, 64, 96, ctypes.byref(nb)))
    assert nb.value == 4 * (2 * 17 * (32 * 48 + 16 * 24) + 2 * 17 * 16 * 24 + 2 * 64 * 96)
    fake = ctypes.c_void_p(0x1000)
    perm = _arr(*range(17))

    def prep(scale=1, n0=0, n=2, maps_bytes=nb.value, flip=0, N=2, oh=64, ow=96, maps=fake, preds=fake, st=17 * 16 * 24):
        return L.rtpe_ms_mean_prep(preds, 8, 12, 2 * 17 * 8 * 12, fake, st, fake, 2 * 17 * 8 * 12, fake,
                                   17 * 16 * 24, n0, n, N, 17, perm, 2, h2, w2, 0, flip, scale, oh, ow, maps,
                                   maps_bytes, None)
    for kw in (dict(scale=2), dict(scale=-1), dict(n0=1, n=2), dict(n=0), dict(maps_bytes=nb.value - 4), dict(N=0),
               dict(flip=1),                        # (the buffer was sized without the mirror maps)
               dict(oh=0), dict(ow=-96), dict(oh=65),               # (a larger decode size needs a larger buffer)
               dict(maps=None), dict(preds=None), dict(st=17 * 16 * 24 - 1)):
        assert prep(**kw) < 0, kw
    val = ctypes.c_void_p(0x2000)

    def topk(K=30, maps_bytes=nb.value, oh=64, maps=fake, ksize=5, tables=val):
        return L.rtpe_topk_ms_mean(maps, 2, 17, 2, h2, w2, 0, 0, oh, 96, K, ksize, 2, tables, val, val, maps_bytes,
                                   fake, 1 << 30, None)
    for kw in (dict(K=0), dict(maps_bytes=nb.value - 4), dict(oh=0), dict(oh=65), dict(maps=None), dict(ksize=4),
               dict(tables=None)):
        assert topk(**kw) < 0, kw

    def refine(maps_bytes=nb.value, table=(val, val, 30), ans_out=fake, oh=64, tail=()):
        fn = L.rtpe_adjust_refine_ms_mean_n if tail else L.rtpe_adjust_refine_ms_mean
        return fn(fake, 2, 17, 2, h2, w2, 0, 0, oh, 96, maps_bytes, val, ans_out, val, 1, 1, 1, val, *table, fake,
                  1 << 30, None, *tail)
    for kw in (dict(maps_bytes=nb.value - 4), dict(table=(None, None, 0)), dict(table=(val, None, 30)),
               dict(ans_out=val), dict(oh=65), dict(oh=0), dict(tail=(None,)), dict(tail=(val,), oh=0),
               dict(tail=(val,), maps_bytes=8)):
        assert refine(**kw) < 0, kw
    # P == 0: nothing to do, nothing launched
    built.check(L.rtpe_adjust_refine_ms_mean(fake, 2, 17, 2, h2, w2, 0, 0, 64, 96, nb.value, None, None, None, 0, 1, 1,
                                             None, None, None, 0, None, 0, None))


# ---- the keyword -----------------------------------------------------------------------------------------------------------
def test_ags_mode():
    from rtpe.third_party.group import ags_mode
    assert ags_mode(False) is False and ags_mode(None) is False and ags_mode(0) is False
    assert ags_mode(True) is True and ags_mode(1) is True and ags_mode("first") is True and ags_mode([0]) is True
    assert ags_mode("mean") == "mean"
    for bad in ("avg", "", "Mean", "true", "False"):
        with pytest.raises(ValueError, match="ags"):
            ags_mode(bad)


def test_unknown_ags_string_is_refused_before_any_gpu_work(monkeypatch):
    from rtpe import engine, inference
    from rtpe.third_party.group import HeatmapParser
    seen = []

    class NoGpu:
        def __init__(self, *a, **k):
            seen.append(k.get("ags"))
            raise AssertionError("GPU work")
    img = np.zeros((480, 640, 3), np.uint8)
    parser = HeatmapParser(17, 30, 0.1, 1.0, True, False)
    with pytest.raises(ValueError, match="ags"):
        parser.parse_multi_scale(None, (128, 192), (1,), True, ags="avg")
    with pytest.raises(ValueError, match="ags"):
        parser.ms_begin(2, [(64, 96)], (128, 192), (1,), True, ags="avg")
    with pytest.raises(ValueError, match="ags"):
        engine.TeacherPipeline(None, parser, device="cuda:0", flip_test=True, scale_factors=(1,), ags="avg")
    with pytest.raises(ValueError, match="scale_factors"):
        engine.TeacherPipeline(None, parser, device="cuda:0", ags="mean")
    with pytest.raises(ValueError):
        engine.StudentPipeline(None, parser, device="cuda:0", ags="mean")
    with pytest.raises(ValueError, match="ags"):
        inference.multi_scale_inference(None, parser, img, 640, (1,), ags="avg")
    monkeypatch.setattr(engine, "TeacherPipeline", NoGpu)
    with pytest.raises(ValueError, match="ags"):
        inference.multi_scale_batch_inference(None, parser, [img], 640, (2, 1, 0.5), ags="avg")
    with pytest.raises(ValueError, match="ags"):
        inference.flip_test_inference(None, parser, [img], 640, ags="avg")
    assert not seen and parser.tag_per_joint                # refused before the parser was touched
    # the known ones reach the pipeline: "first" as True, "mean" as it is - and the parser's flag is set as with True
    for ags, want in (("first", True), ("mean", "mean")):
        for call in (lambda p: inference.multi_scale_batch_inference(None, p, [img], 640, (2, 1, 0.5), ags=ags),
                     lambda p: inference.flip_test_inference(None, p, [img], 640, ags=ags)):
            p = HeatmapParser(17, 30, 0.1, 1.0, True, False)
            with pytest.raises(AssertionError, match="GPU work"):
                call(p)
            assert seen.pop() == want and not seen and p.tag_per_joint is False
    # the scales are still checked first with "mean"
    with pytest.raises(ValueError):
        inference.multi_scale_batch_inference(None, parser, [img], 640, (2, 0.5), ags="mean")


def test_channel_mean_refuses_more_channels_than_the_order_is_pinned_for():
    """a ValueError from the Python op before any GPU work (a CPU tensor gets this far), never other bits"""
    from rtpe import inference
    with pytest.raises(ValueError, match="272"):
        inference.channel_mean(torch.zeros(1, 273, 2, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.channel_mean(torch.zeros(1, 272, 2, 16))


def test_channel_mean_has_no_cpu_fallback():
    from rtpe import inference
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.channel_mean(torch.zeros(1, 17, 4, 8))


def test_mean_kernels_do_not_spill_and_divide(built, tmp_path):
    """the compiled gfx950 kernels: no registers spilled to scratch memory, and the mean ends in a true division
    (the div_fixup of the IEEE sequence), not in a multiplication by the reciprocal"""
    from test_flip_decode_host import _device_code
    found = {}
    for src, kernels in (("tag_mean.hip", ("channel_mean_kernel", "mean_plane_kernel")),
                         ("decode.hip", ("mean_prep_kernel",))):
        for body in re.split(r"\n(?=[0-9a-f]+ <)", _device_code(built, tmp_path, src)):
            m = re.match(r"[0-9a-f]+ <(\S*(%s)\S*)>" % "|".join(kernels), body)
            if m:
                found.setdefault(m.group(2), []).append(body)
                assert "scratch_" not in body, m.group(1) + ": registers spilled to scratch memory"
    assert {k: len(v) for k, v in found.items()} == {"channel_mean_kernel": 1, "mean_plane_kernel": 1,
                                                     "mean_prep_kernel": 2}
    for k in ("channel_mean_kernel", "mean_plane_kernel"):
        assert "v_div_fixup_f32" in found[k][0], k
