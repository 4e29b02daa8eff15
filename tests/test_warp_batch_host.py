"""CPU tests of the batched pre-processing (a whole chunk of images warped at every test scale): the ABI of the new
entries, the job table the host function fills, the refusals raised before any GPU work, how the three batched drivers
call ``transforms.warp_normalize_batch`` with ``warp="batch"``, and the compiled kernel (no scratch memory)."""
import ctypes
import os
import re
import struct

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


NEW_SYMBOLS = ("rtpe_warp_batch_table_bytes", "rtpe_warp_batch_table_fill", "rtpe_warp_normalize_batch")


def _declared(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_warp_symbols_are_declared_and_resolve(built):
    """the prototypes live in include/rtpe_hip_warp.h, which rtpe_hip.h includes with one line; the binding lists them
    in EXPORTS_WARP and resolves them with the others; the two older tables and the ABI revision are as they were"""
    main = _declared("rtpe_hip.h")
    assert len(re.findall(r'#include "rtpe_hip_warp.h"', main)) == 1
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", _declared("rtpe_hip_warp.h")))
    assert declared == set(NEW_SYMBOLS) == set(built.EXPORTS_WARP)
    assert not declared & set(built.EXPORTS) and not declared & set(built.EXPORTS_SIZES)
    assert not declared & set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", main))
    assert len(built.EXPORTS) == 59 and len(built.EXPORTS_SIZES) == 5
    lib = built.lib()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).argtypes == built._SIGS_WARP[name][1], name
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4


# 3 images x 2 scales: (address, h, w, stride) per image, (address, H, W) per scale
SRC = [(0x7f0000001000, 96, 128, 384), (0x7f0000100000, 90, 128, 400), (0x7f0000200010, 97, 131, 393)]
DST = [(0x7e0000000000, 384, 256), (0x7e0001000000, 89, 134)]


def _fill(built, src=SRC, dst=DST, table_bytes=None, mats=None, null=None):
    L = built.lib()
    N, S = len(src), len(dst)
    nb = ctypes.c_size_t(0)
    rc = L.rtpe_warp_batch_table_bytes(N, S, ctypes.byref(nb))
    if rc:
        return rc, None, None
    assert nb.value == 64 * N * S
    if mats is None:
        mats = np.arange(S * N * 6, dtype=np.float32).reshape(S, N, 6) * np.float32(0.37) - np.float32(3.0)
    table = np.full(nb.value + 16, 0xAB, np.uint8)
    args = [(ctypes.c_uint64 * N)(*[a[0] for a in src]), (ctypes.c_int32 * (3 * N))(*[v for a in src for v in a[1:]]),
            mats.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), (ctypes.c_uint64 * S)(*[d[0] for d in dst]),
            (ctypes.c_int32 * (2 * S))(*[v for d in dst for v in d[1:]]), N, S, ctypes.c_void_p(table.ctypes.data),
            nb.value if table_bytes is None else table_bytes]
    if null is not None:
        args[null] = None
    return L.rtpe_warp_batch_table_fill(*args), table, mats


def test_warp_table_is_filled_on_the_host(built):
    """no GPU: the table is host memory.  Entry (scale s, image n) at index s * N + n, 64 bytes: source address, h, w,
    stride, zero, the six matrix entries bit for bit, the address of image n's planes in the tensor of scale s, zero"""
    rc, table, mats = _fill(built)
    assert rc == 0
    N, S = len(SRC), len(DST)
    assert bytes(table[64 * N * S:]) == b"\xab" * 16                      # nothing written past the table
    for s, (base, H, W) in enumerate(DST):
        for n, (addr, h, w, stride) in enumerate(SRC):
            e = bytes(table[64 * (s * N + n):64 * (s * N + n + 1)])
            src, eh, ew, es, zero = struct.unpack_from("<QiiiI", e, 0)
            assert (src, eh, ew, es, zero) == (addr, h, w, stride, 0), (s, n)
            assert e[24:48] == mats[s, n].tobytes(), (s, n)
            d, zero = struct.unpack_from("<QQ", e, 48)
            assert (d, zero) == (base + n * 3 * H * W * 4, 0), (s, n)


def test_warp_table_refusals(built):
    L = built.lib()
    N, S = len(SRC), len(DST)
    assert _fill(built, table_bytes=64 * N * S - 1)[0] < 0 and b"table" in L.rtpe_last_error_string()
    for n in range(N):                                                       # non-positive sizes, stride < 3 * w
        for bad in ((0, 128, 384), (96, 0, 384), (-1, 128, 384), (96, 128, 383), (96, 128, 0), (96, 128, -384)):
            src = list(SRC)
            src[n] = (SRC[n][0],) + bad
            assert _fill(built, src=src)[0] < 0, (n, bad)
    assert _fill(built, src=[SRC[0], (0,) + SRC[1][1:], SRC[2]])[0] < 0      # a null source
    for s in range(S):
        for bad in ((0, 256), (384, 0), (-384, 256)):
            dst = list(DST)
            dst[s] = (DST[s][0],) + bad
            assert _fill(built, dst=dst)[0] < 0, (s, bad)
    assert _fill(built, dst=[DST[0], (0, 89, 134)])[0] < 0                   # a null destination
    for k in (0, 1, 2, 3, 4, 7):                                             # null arguments
        assert _fill(built, null=k)[0] < 0, k
    assert _fill(built, src=[])[0] < 0 and _fill(built, dst=[])[0] < 0
    assert L.rtpe_warp_batch_table_bytes(3, 2, None) < 0
    assert L.rtpe_warp_batch_table_bytes(3, 0, ctypes.byref(ctypes.c_size_t())) < 0
    assert _fill(built, src=[SRC[0]], dst=[DST[1]])[0] == 0                  # (and the smallest table is accepted)


def test_warp_launch_entry_checks_its_arguments_before_any_launch(built):
    """the same null and std > 0 refusals as rtpe_warp_normalize (no launch: the pointers are never read)"""
    L = built.lib()
    fake = ctypes.c_void_p(0x1000)
    f3 = ctypes.c_float * 3

    def launch(table=fake, N=3, S=2, sizes=(384, 256, 89, 134), mean=(0.5, 0.5, 0.5), std=(0.2, 0.2, 0.2)):
        return L.rtpe_warp_normalize_batch(table, N, S, None if sizes is None else (ctypes.c_int32 * len(sizes))(*sizes),
                                           None if mean is None else f3(*mean), None if std is None else f3(*std), 1, None)
    for kw in (dict(table=None), dict(sizes=None), dict(mean=None), dict(std=None), dict(std=(0.2, 0.0, 0.2)),
               dict(std=(0.2, 0.2, -1.0)), dict(N=0), dict(S=0), dict(sizes=(384, 256, 0, 134)),
               dict(sizes=(384, 256, 89, -1)), dict(table=ctypes.c_void_p(0x1004))):
        assert launch(**kw) < 0, kw
        assert b"warp" in L.rtpe_last_error_string()
    one = L.rtpe_warp_normalize(fake, 96, 128, 384, (ctypes.c_float * 6)(), f3(), f3(0.2, 0.0, 0.2), fake, 192, 128, 1,
                                None)
    assert one < 0 and one == launch(std=(0.2, 0.0, 0.2))


def _img(h, w, dtype=np.uint8):
    return np.zeros((h, w, 3), dtype)


def test_warp_normalize_batch_refuses_before_any_gpu_work():
    """the default device is "cuda" and this test runs without a GPU: each refusal comes before the device is touched"""
    from rtpe.third_party import transforms
    a, b = _img(96, 128), _img(128, 96)
    assert transforms.get_multi_scale_size(a, 128, 1, 1)[0] == (192, 128)
    assert transforms.get_multi_scale_size(b, 128, 1, 1)[0] == (128, 192)
    with pytest.raises(ValueError, match=r"images 0 \(128 x 96\) and 2 \(96 x 128\).*192 x 128 and 128 x 192"):
        transforms.warp_normalize_batch([a, _img(90, 128), b], 128)
    # any scale: input 128 at (0.7, 1) gives 134 x 89 against 89 x 89
    c, d = _img(96, 128), _img(128, 128)
    assert transforms.get_multi_scale_size(c, 128, 0.7, 1)[0] == (134, 89)
    with pytest.raises(ValueError, match="different input sizes"):
        transforms.warp_normalize_batch([c, d], 128, ((0.7, 1),))
    with pytest.raises(ValueError):
        transforms.warp_normalize_batch([], 128)
    with pytest.raises(ValueError):
        transforms.warp_normalize_batch([a], 128, scales=())
    for bad in (_img(96, 128, np.float32), _img(96, 128, np.int8), np.zeros((96, 128), np.uint8),
                np.zeros((96, 128, 4), np.uint8), torch.zeros((96, 128, 3)), torch.zeros((3, 96, 128), dtype=torch.uint8),
                [[1, 2, 3]]):
        with pytest.raises(TypeError, match="image 1"):
            transforms.warp_normalize_batch([a, bad], 128)
    with pytest.raises(RuntimeError, match="HIP path only"):                 # accepted: stopped by the missing GPU
        transforms.warp_normalize_batch([a, torch.zeros((90, 128, 3), dtype=torch.uint8)], 128, device="cpu")


class _NoGpu:
    def __init__(self, *a, **k):
        raise AssertionError("GPU work")


class _Parser:
    tag_per_joint = True


def test_drivers_reject_an_unknown_warp_before_any_gpu_work(monkeypatch):
    from rtpe import engine, inference
    monkeypatch.setattr(engine, "TeacherPipeline", _NoGpu)
    imgs = [_img(96, 128)]
    for call in (lambda w: inference.plain_inference(None, _Parser(), imgs, 128, warp=w),
                 lambda w: inference.flip_test_inference(None, _Parser(), imgs, 128, warp=w),
                 lambda w: inference.flip_test_inference(None, _Parser(), imgs, 128, ags=True, warp=w),
                 lambda w: inference.multi_scale_batch_inference(None, _Parser(), imgs, 128, (2, 1, 0.5), warp=w)):
        for bad in ("other", None, "Batch"):
            with pytest.raises(ValueError, match="warp must be"):
                call(bad)
        for good in ("image", "batch"):                                      # accepted: the pipeline is reached
            with pytest.raises(AssertionError, match="GPU work"):
                call(good)


def _recording(monkeypatch, log):
    """TeacherPipeline and both warps replaced, in the style of test_sizes_decode_host._recording_pipeline: a "warped
    image" is a (1,1,1,4) tensor [index of the image, scale * 100, H, W]; the batch warp logs its call"""
    from rtpe import engine, inference
    from rtpe.third_party import transforms

    def one(img, input_size, s, lo, device=None):
        (w, h), center, scale = transforms.get_multi_scale_size(img, input_size, s, lo)
        return torch.tensor([[[[img.index, int(s * 100), h, w]]]]), center, scale

    def per_image(img, input_size, s=1, lo=1, device=None):
        log.append(("image warp", img.index, s, lo))
        return one(img, input_size, s, lo)

    def per_batch(images, input_size, scales=((1, 1),), device=None):
        log.append(("batch warp", [img.index for img in images], list(scales)))
        got = [[one(img, input_size, s, lo) for s, lo in scales] for img in images]
        ts = [torch.cat([g[k][0] for g in got]) for k in range(len(scales))]
        return ts, [[r[1] for r in g] for g in got], [[r[2] for r in g] for g in got]

    class Recorder:
        def __init__(self, model, parser, device=None, **kw):
            self.device = device
            log.append(("init", kw))

        def stream(self, batches, out_hw=None):
            for k, x in enumerate(batches):
                xs = x if isinstance(x, list) else [x]
                rows = [[tuple(int(v) for v in r) for r in t[:, 0, 0]] for t in xs]
                log.append(("batch", rows, out_hw(k) if callable(out_hw) else out_hw))
                yield [(np.full((1, 17, 4), float(r[0]), np.float32), [float(r[0])]) for r in rows[0]]

    def final(grouped, center, scale, heatmap_size):
        log.append(("final", int(grouped[0][0, 0, 0]), np.array(center), np.array(scale), list(heatmap_size)))
        return "final of %d" % int(grouped[0][0, 0, 0])
    monkeypatch.setattr(engine, "TeacherPipeline", Recorder)
    monkeypatch.setattr(transforms, "warp_normalize", per_image)
    monkeypatch.setattr(transforms, "warp_normalize_batch", per_batch)
    monkeypatch.setattr(transforms, "get_final_preds", final)
    return inference, transforms


class _Img:
    def __init__(self, index, h, w):
        self.index, self.shape = index, (h, w, 3)


# input 256: landscape 384 x 256 (images 0, 1, 4, 6, 7), portrait 256 x 384 (2, 5), and (150, 200) -> 384 x 256 too (3)
SHAPES = [(192, 256), (180, 256), (256, 192), (150, 200), (192, 256), (256, 180), (185, 256), (190, 256)]


def test_plain_inference_warp_batch_calls_the_batch_warp_once_per_chunk(monkeypatch):
    log = []
    inference, transforms = _recording(monkeypatch, log)
    images = [_Img(i, h, w) for i, (h, w) in enumerate(SHAPES)]
    plan = inference.plain_plan(SHAPES, 256, 2)
    assert plan == [[0, 1], [3, 4], [6, 7], [2, 5]]
    out = inference.plain_inference(None, None, images, 256, 2, device="cpu", warp="batch")
    assert [int(p[0, 0, 0]) for p, _ in out] == list(range(8)) and [s for _, s in out] == [[float(i)] for i in range(8)]
    assert not [e for e in log if e[0] == "image warp"]
    assert [e[1] for e in log if e[0] == "batch warp"] == plan               # once per chunk, its images in order
    assert all(e[2] == [(1, 1)] for e in log if e[0] == "batch warp")
    batches = [e for e in log if e[0] == "batch"]
    assert [[r[0] for r in b[1][0]] for b in batches] == plan
    assert [b[2] for b in batches] == [[SHAPES[i] for i in c] for c in plan]
    # the default path and warp="image": today's loop, the batch warp never called
    for kw in ({}, {"warp": "image"}):
        del log[:]
        out = inference.plain_inference(None, None, images, 256, 2, device="cpu", **kw)
        assert [int(p[0, 0, 0]) for p, _ in out] == list(range(8))
        assert not [e for e in log if e[0] == "batch warp"]
        assert [e[1] for e in log if e[0] == "image warp"] == [i for c in plan for i in c]


@pytest.mark.parametrize("driver", ["flip", "multi_scale", "flip_ags"])
def test_flip_and_multi_scale_warp_batch_plumbing(monkeypatch, driver):
    log = []
    inference, transforms = _recording(monkeypatch, log)
    images = [_Img(i, h, w) for i, (h, w) in enumerate(SHAPES)]
    factors = (1, 0.5, 2) if driver == "multi_scale" else (1,)
    order = sorted(factors, reverse=True)
    lo = min(factors)

    def run(**kw):
        del log[:]
        if driver == "multi_scale":
            return inference.multi_scale_batch_inference(None, _Parser(), images, 256, factors, batch_size=2,
                                                         device="cpu", **kw)
        return inference.flip_test_inference(None, _Parser(), images, 256, batch_size=2, device="cpu",
                                             ags=driver == "flip_ags", **kw)
    out = run(warp="batch")
    assert [r[0] for r in out] == ["final of %d" % i for i in range(8)]      # results in input order
    chunks = [[0, 1], [3, 4], [6, 7], [2, 5]]
    warps = [e for e in log if e[0] == "batch warp"]
    assert [e[1] for e in warps] == chunks                                   # once per chunk ...
    assert all(e[2] == [(s, lo) for s in order] for e in warps)              # ... with all of its scales, largest first
    assert not [e for e in log if e[0] == "image warp"]
    for b, c in zip([e for e in log if e[0] == "batch"], chunks):
        assert len(b[1]) == len(order)                                       # one tensor per scale reached the pipeline
        for rows, s in zip(b[1], order):
            assert [r[0] for r in rows] == c and all(r[1] == int(s * 100) for r in rows)
    # the centre / scale that reach get_final_preds: those of the smallest scale, at the projection size
    finals = {e[1]: e for e in log if e[0] == "final"}
    assert sorted(finals) == list(range(8))
    for i, img in enumerate(images):
        size, center, scale = transforms.get_multi_scale_size(img, 256, lo, lo)
        base = transforms.get_multi_scale_size(img, 256, 1.0, lo)[0]
        assert np.array_equal(finals[i][2], center) and np.array_equal(finals[i][3], scale)
        assert finals[i][4] == list(base)
    want = [(e[1], e[2].tolist(), e[3].tolist(), e[4]) for e in log if e[0] == "final"]
    # the default path: the same results and the same centre / scale, the batch warp never called
    assert [r[0] for r in run()] == ["final of %d" % i for i in range(8)]
    assert not [e for e in log if e[0] == "batch warp"]
    assert len([e for e in log if e[0] == "image warp"]) == 8 * len(order)
    assert [(e[1], e[2].tolist(), e[3].tolist(), e[4]) for e in log if e[0] == "final"] == want


def test_warp_batch_kernel_exists_and_uses_no_scratch(built, tmp_path):
    from test_flip_decode_host import _device_code
    dis = _device_code(built, tmp_path, "preprocess.hip")
    bodies = re.split(r"\n(?=[0-9a-f]+ <)", dis)
    mine = [b for b in bodies if re.match(r"[0-9a-f]+ <\S*warp_normalize\S*kernel", b)]
    names = [b.split("<", 1)[1].split(">", 1)[0] for b in mine]
    assert any("warp_normalize_batch_kernel" in n for n in names), names
    assert any("warp_normalize_kernel" in n for n in names), names
    for n, b in zip(names, mine):
        assert "scratch_" not in b, n + ": registers spilled to scratch memory"
