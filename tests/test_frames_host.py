"""CPU tests of the students' frames front end (uint8 HWC frames -> the canvases of ``forward_mixed``): the ABI of the
new entries (include/rtpe_hip_frames.h), the job table the host function fills, every refusal of the C and the Python
side that comes before any GPU work, ``StudentPipeline.frame_batches``, and the premises of the exact GPU tests
(tests/test_frames_gpu.py, which takes its frames and its oracles from this file): the numpy float32 oracle of
ToTensor + Normalize is torch-CPU's bit for bit, and the float32 HSV oracle agrees with the float64 one."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
OP_SIZES = [(33, 47), (47, 33), (64, 32)]                  # every image reaches one edge of the default 64 x 47 canvas
OP_CANVASES = [None, (72, 80)]                             # Wc % 4 = 3 / Wc % 4 = 0, no image at an edge, w = 33 ends inside a store


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


# --------------------------------------------------------------------------- #
# frames and oracles (shared with tests/test_frames_gpu.py)
# --------------------------------------------------------------------------- #
def seeded_frames(sizes=OP_SIZES, seed=0):
    rng = np.random.default_rng(1000 + seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def all_levels_frame():
    """32 x 256: row 0 the grey ramp (d == 0 at every level, both branches of the sRGB linearisation: 11 levels lie below
    0.04045), rows 1-3 the three single-channel ramps (one hue branch each), row 4 r max with g < b (the hue wraps through
    the floor), the rest seeded"""
    f = np.random.default_rng(77).integers(0, 256, (32, 256, 3), dtype=np.uint8)
    x = np.arange(256)
    f[0] = x[:, None]
    for c in range(3):
        f[1 + c] = 0
        f[1 + c, :, c] = x
    g = x % 128
    f[4, :, 0], f[4, :, 1], f[4, :, 2] = 255, g, g + 1 + (x // 128) * 60
    return f


def to_tensor32(frame):
    """``to_tensor``: (h, w, 3) uint8 -> (h, w, 3) float32, a true float32 division"""
    return frame.astype(np.float32) / np.float32(255)


def normalized32(frame, mean=MEAN, std=STD):
    """``Normalize(to_tensor(frame))`` in numpy float32 -> (3, h, w): one subtraction, one true division"""
    x = (to_tensor32(frame) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    assert x.dtype == np.float32
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def hsv32(t):
    """rgb2hsv of (h, w, 3) float32 in numpy float32 -> (3, h, w): only max, min, -, /, floor, each exact in float32, in
    the order of the kernel (csrc/alt_colour.h)"""
    t = np.asarray(t, np.float32)
    r, g, b = t[..., 0], t[..., 1], t[..., 2]
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    d = mx - mn
    six, two, four = np.float32(6), np.float32(2), np.float32(4)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.where(mx == r, (g - b) / d, np.where(mx == g, two + (b - r) / d, four + (r - g) / d))
        h = h / six
        h = h - np.floor(h)
        s = d / mx
    h = np.where(d == 0, np.float32(0), h)
    s = np.where(d == 0, np.float32(0), s)
    out = np.stack([h, s, mx]).astype(np.float32)
    assert h.dtype == s.dtype == np.float32
    return out


# --------------------------------------------------------------------------- #
# ABI
# --------------------------------------------------------------------------- #
NEW_SYMBOLS = ("rtpe_frames_table_bytes", "rtpe_frames_table_fill", "rtpe_frames_to_canvases")
OLDER = {"EXPORTS": 59, "EXPORTS_SIZES": 5, "EXPORTS_WARP": 3, "EXPORTS_SHARED": 3, "EXPORTS_PAIR": 1, "EXPORTS_RECORDS": 2,
         "EXPORTS_TAGMEAN": 6, "EXPORTS_NOPROJ": 5, "EXPORTS_ANYSIZE": 4, "EXPORTS_MIXED": 4, "EXPORTS_MIXDEC": 4,
         "EXPORTS_TRACE": 2, "EXPORTS_MIXAUX": 1}


def _declared(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_frames_symbols_are_declared_and_resolve(built):
    main = _declared("rtpe_hip.h")
    assert len(re.findall(r'#include "rtpe_hip_frames.h"', main)) == 1
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", _declared("rtpe_hip_frames.h")))
    assert declared == set(NEW_SYMBOLS) == set(built.EXPORTS_FRAMES)
    for table, n in OLDER.items():
        assert len(getattr(built, table)) == n, table
        assert not declared & set(getattr(built, table)), table
    assert not declared & set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", main))
    lib = built.lib()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).argtypes == built._SIGS_FRAMES[name][1], name
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4


# (address, h, w, stride) per frame, in a 200 x 131 canvas
SRC = [(0x7f0000001000, 96, 128, 384), (0x7f0000100003, 32, 32, 96), (0x7f0000200010, 200, 131, 400)]
CANVAS = (200, 131)


def _fill(built, src=SRC, canvas=CANVAS, table_bytes=None, null=None):
    L = built.lib()
    N = len(src)
    nb = ctypes.c_size_t(0)
    rc = L.rtpe_frames_table_bytes(N, ctypes.byref(nb))
    if rc:
        return rc, None
    assert nb.value == 32 * N
    table = np.full(nb.value + 16, 0xAB, np.uint8)
    args = [(ctypes.c_uint64 * N)(*[a[0] for a in src]), (ctypes.c_int32 * (3 * N))(*[v for a in src for v in a[1:]]),
            N, canvas[0], canvas[1], ctypes.c_void_p(table.ctypes.data), nb.value if table_bytes is None else table_bytes]
    if null is not None:
        args[null] = None
    return L.rtpe_frames_table_fill(*args), table


def test_frames_table_is_filled_on_the_host(built):
    """no GPU: the table is host memory.  32 bytes per frame: source address, h, w, row stride, and 12 zero bytes"""
    rc, table = _fill(built)
    assert rc == 0
    want = b"".join(struct.pack("<QiiiiQ", addr, h, w, stride, 0, 0) for addr, h, w, stride in SRC)
    assert len(want) == 32 * len(SRC) and bytes(table[:len(want)]) == want
    assert bytes(table[len(want):]) == b"\xab" * 16                          # nothing written past the table


def test_frames_table_refusals(built):
    L = built.lib()
    E = -1                                                                   # RTPE_E_INVALID
    N = len(SRC)
    assert _fill(built, table_bytes=32 * N - 1)[0] == E and b"table" in L.rtpe_last_error_string()
    for n in range(N):
        a, h, w, s = SRC[n]
        for bad in ((31, w, s), (h, 31, s), (0, w, s), (-1, w, s), (h, w, 3 * w - 1), (h, w, 0), (h, w, -s),
                    (CANVAS[0] + 1, w, s), (h, CANVAS[1] + 1, 3 * CANVAS[1] + 3)):
            src = list(SRC)
            src[n] = (a,) + bad
            assert _fill(built, src=src)[0] == E, (n, bad)
            assert b"frames_table_fill: image %d" % n in L.rtpe_last_error_string()
    assert _fill(built, src=[SRC[0], (0,) + SRC[1][1:], SRC[2]])[0] == E     # a null source
    assert _fill(built, canvas=(199, 131))[0] == E and _fill(built, canvas=(200, 130))[0] == E
    for k in (0, 1, 5):                                                      # null arguments
        assert _fill(built, null=k)[0] == E, k
    assert _fill(built, src=[])[0] == E                                      # n outside 1..65535
    nb = ctypes.c_size_t()
    assert L.rtpe_frames_table_bytes(0, ctypes.byref(nb)) == E and L.rtpe_frames_table_bytes(65536, ctypes.byref(nb)) == E
    assert L.rtpe_frames_table_bytes(65535, ctypes.byref(nb)) == 0 and nb.value == 32 * 65535
    assert L.rtpe_frames_table_bytes(3, None) == E
    assert _fill(built, src=[SRC[1]], canvas=(32, 32))[0] == 0               # (and the smallest table is accepted)


def launch_refusals(L, table, canvas, alt):
    """every refused call of rtpe_frames_to_canvases with these (real or fake) addresses -> [(what, return code)]"""
    f3 = ctypes.c_float * 3

    def go(table=table, N=3, Hc=64, Wc=47, mean=MEAN, std=STD, mode=0, canvas=canvas, alt=alt):
        return L.rtpe_frames_to_canvases(table, N, Hc, Wc, None if mean is None else f3(*mean),
                                         None if std is None else f3(*std), mode, canvas, alt, None)
    cases = [dict(table=None), dict(mean=None), dict(std=None), dict(canvas=None), dict(std=(0.2, 0.0, 0.2)),
             dict(std=(0.2, 0.2, -1.0)), dict(mode=2), dict(mode=-2), dict(alt=None), dict(mode=1, alt=None),
             dict(mode=-1), dict(N=0), dict(N=65536), dict(Hc=0), dict(Wc=-47)]
    return [(kw, go(**kw)) for kw in cases]


def test_frames_launch_entry_checks_its_arguments_before_any_launch(built):
    """no launch: the pointers are never read, so made-up addresses do"""
    L = built.lib()
    got = launch_refusals(L, ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000))
    assert len(got) == 15
    for kw, rc in got:
        assert rc == -1, kw
    assert b"frames_to_canvases" in L.rtpe_last_error_string()


# --------------------------------------------------------------------------- #
# Python refusals, before any GPU work (this machine has no GPU and the default device is "cuda")
# --------------------------------------------------------------------------- #
def _f(h, w, dtype=np.uint8):
    return np.zeros((h, w, 3), dtype)


def test_pack_frames_refuses_before_any_gpu_work():
    from rtpe.students import pack_frames
    with pytest.raises(ValueError, match="no frames"):
        pack_frames([])
    for bad in (_f(40, 40, np.float32), _f(40, 40, np.int8), np.zeros((40, 40), np.uint8), np.zeros((40, 40, 4), np.uint8),
                torch.zeros((40, 40, 3)), torch.zeros((3, 40, 40), dtype=torch.uint8), [[1, 2, 3]]):
        with pytest.raises(TypeError, match="frame 1"):
            pack_frames([_f(40, 40), bad])
    with pytest.raises(TypeError):
        pack_frames(np.zeros((40, 40, 3), np.uint8))                         # one frame is not a sequence of frames
    with pytest.raises(TypeError, match="frame 0"):
        pack_frames(np.zeros((2, 3, 40, 40), np.uint8))                      # NCHW
    for bad in (_f(31, 40), _f(40, 31)):
        with pytest.raises(ValueError, match="at least 32"):
            pack_frames([_f(40, 40), bad])
    with pytest.raises(ValueError, match="larger than the 40 x 47 canvas"):
        pack_frames([_f(40, 40), _f(48, 40)], canvas_hw=(40, 47))
    with pytest.raises(NotImplementedError, match="Unknown color space XYZ"):
        pack_frames([_f(40, 40)], alt_colorspace="XYZ")
    good = torch.empty(2, 3, 48, 40)
    for out in ((torch.empty(2, 3, 48, 41), None), (torch.empty(3, 3, 48, 40), None),
                (torch.empty(2, 3, 48, 40, dtype=torch.float16), None), (torch.empty(2, 3, 48, 40, dtype=torch.float64), None),
                (good, None),                                                # right shape and dtype, on the CPU
                (good, good), good, (good,)):
        with pytest.raises(ValueError, match="out"):
            pack_frames([_f(40, 40), _f(48, 40)], out=out)
    with pytest.raises(ValueError, match="out"):                             # a colour space and no second tensor
        pack_frames([_f(40, 40), _f(48, 40)], "LAB", out=(good, None))
    with pytest.raises(ValueError, match="out"):
        pack_frames([_f(40, 40), _f(48, 40)], "LAB", out=(good, torch.empty(2, 3, 48, 44)))
    with pytest.raises(RuntimeError, match="HIP path only"):                 # accepted: stopped by the missing GPU
        pack_frames([_f(40, 40), torch.zeros((48, 40, 3), dtype=torch.uint8)], "HSV", device="cpu")


class _Plain(torch.nn.Module):
    def forward_mixed(self, canvas, sizes):
        raise AssertionError("GPU work")


class _WithAlt(torch.nn.Module):
    def forward_mixed(self, canvas, sizes, alt=None):
        raise AssertionError("GPU work")


class _Refusing(_WithAlt):
    def refuse_mixed(self):
        raise NotImplementedError("masked fp16 forms")


def _pipe(model):
    from rtpe.engine import StudentPipeline
    pipe = StudentPipeline.__new__(StudentPipeline)                          # (the constructor asks for the current GPU)
    pipe.model, pipe.device = model, torch.device("cuda:0")
    return pipe


def test_call_frames_and_stream_frames_refuse_before_any_gpu_work(monkeypatch):
    from rtpe import students
    monkeypatch.setattr(students, "pack_frames", lambda *a, **k: (_ for _ in ()).throw(AssertionError("GPU work")))
    frames = [_f(40, 40)]
    with pytest.raises(ValueError, match="needs the second input"):
        _pipe(_WithAlt()).call_frames(frames)
    with pytest.raises(ValueError, match="takes no second input"):
        _pipe(_Plain()).call_frames(frames, alt_colorspace="LAB")
    with pytest.raises(ValueError, match="decode must be"):
        _pipe(_Plain()).call_frames(frames, decode="other")
    with pytest.raises(ValueError, match="has no forward_mixed"):
        _pipe(torch.nn.Identity()).call_frames(frames)
    with pytest.raises(NotImplementedError, match="masked fp16 forms"):
        _pipe(_Refusing()).call_frames(frames, alt_colorspace="LAB")
    with pytest.raises(ValueError, match="needs the second input"):
        _pipe(_WithAlt()).stream_frames(iter([frames]))
    with pytest.raises(ValueError, match="takes no second input"):
        _pipe(_Plain()).stream_frames(iter([frames]), alt_colorspace="HSV")
    with pytest.raises(NotImplementedError, match="masked fp16 forms"):
        _pipe(_Refusing()).stream_frames(iter([frames]), alt_colorspace="LAB")
    with pytest.raises(AssertionError, match="GPU work"):                    # accepted: the packing is reached
        _pipe(_Plain()).call_frames(frames)
    # the refusals of call_mixed are word for word what they were
    with pytest.raises(ValueError, match=r"StudentPipeline.call_mixed: decode must be 'batch' or 'per_image', not 'x'"):
        _pipe(_Plain()).call_mixed([torch.zeros(3, 40, 40)], decode="x")
    with pytest.raises(ValueError, match=r"StudentPipeline.call_mixed: the model has no forward_mixed"):
        _pipe(torch.nn.Identity()).call_mixed([torch.zeros(3, 40, 40)])


def test_an_unknown_colour_space_reaches_pack_frames_refusal():
    with pytest.raises(NotImplementedError, match="Unknown color space YUV"):
        _pipe(_WithAlt()).call_frames([_f(40, 40)], alt_colorspace="YUV")


# --------------------------------------------------------------------------- #
# frame_batches
# --------------------------------------------------------------------------- #
class _Shape:
    def __init__(self, *shape):
        self.shape = shape


def test_frame_batches_cuts_by_h_times_w_and_restores_the_order():
    from rtpe.engine import StudentPipeline
    hw = [(100, 40), (50, 70), (40, 100), (33, 200), (64, 50), (90, 32)]     # areas 4000 3500 4000 6600 3200 2880
    frames = [_Shape(h, w, 3) for h, w in hw]
    batches, restore = StudentPipeline.frame_batches(frames, batch_size=4)
    assert [[frames.index(f) for f in b] for b in batches] == [[5, 4, 1, 0], [2, 3]]      # ties (0, 2) keep their order
    assert restore([["r5", "r4", "r1", "r0"], ["r2", "r3"]]) == ["r%d" % i for i in range(6)]
    with pytest.raises(ValueError, match="frame_batches"):
        restore([["a"], ["b"]])
    with pytest.raises(ValueError, match="frame_batches: batch_size"):
        StudentPipeline.frame_batches(frames, 0)
    # mixed_batches reads shape[-2] * shape[-1] = w * 3 of such a shape: another order
    other, _ = StudentPipeline.mixed_batches(frames, batch_size=4)
    assert [[frames.index(f) for f in b] for b in other] == [[5, 0, 4, 1], [2, 3]]
    # ... and for (3, h, w) images it cuts what frame_batches cuts for their frames
    chw, _ = StudentPipeline.mixed_batches([_Shape(3, h, w) for h, w in hw], batch_size=4)
    assert [[(s.shape[1], s.shape[2]) for s in b] for b in chw] == [[f.shape[:2] for f in b] for b in batches]
    # real arrays, one batch, default size
    arrs = [_f(h, w) for h, w in hw]
    one, restore1 = StudentPipeline.frame_batches(arrs)
    assert len(one) == 1 and [a.shape[:2] for a in one[0]] == [hw[i] for i in (5, 4, 1, 0, 2, 3)]
    assert restore1([[5, 4, 1, 0, 2, 3]]) == list(range(6))
    assert StudentPipeline.frame_batches([]) [0] == []


# --------------------------------------------------------------------------- #
# premises of the exact GPU tests
# --------------------------------------------------------------------------- #
def test_the_numpy_oracle_is_torch_cpu_to_tensor_and_normalize_on_every_level():
    """all 256 levels x 3 channels: ``float().div(255)`` and ``sub_(mean).div_(std)`` (torchvision's to_tensor and
    Normalize) on the CPU give the bits of the numpy float32 oracle; the product with the rounded reciprocal (what a GPU
    ``tensor / 255`` computes) does not, at 126 of the 256 levels - the "old path" inputs of the GPU tests are made on the CPU"""
    frame = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)          # (1, 256, 3)
    t = torch.from_numpy(frame).permute(2, 0, 1).contiguous().float().div(255)
    assert np.array_equal(t.numpy(), to_tensor32(frame).transpose(2, 0, 1))
    x = t.clone().sub_(torch.as_tensor(MEAN, dtype=torch.float32)[:, None, None]).div_(
        torch.as_tensor(STD, dtype=torch.float32)[:, None, None])
    assert np.array_equal(x.numpy(), normalized32(frame))
    recip = np.arange(256, dtype=np.float32) * (np.float32(1) / np.float32(255))
    assert int((recip != to_tensor32(frame)[0, :, 0]).sum()) == 126


def test_the_float32_hsv_oracle_agrees_with_the_float64_one():
    from oracle import student_ref
    t = to_tensor32(all_levels_frame())
    got, want = hsv32(t), student_ref.rgb2hsv(t).transpose(2, 0, 1)
    dh = np.abs(got[0] - want[0])
    assert np.minimum(dh, 1.0 - dh).max() <= 1e-5                            # hue is circular
    assert np.abs(got[1:] - want[1:]).max() <= 1e-5
    f = all_levels_frame()
    assert (f[0, :, 0] == f[0, :, 1]).all() and int((t[0, :, 0] <= np.float32(0.04045)).sum()) == 11
    assert (f[4, :, 0] > f[4, :, 2]).all() and (f[4, :, 1] < f[4, :, 2]).all()
    assert got[0, 4].min() > 0.5                                             # the wrapped hues: (g - b) / d < 0 -> 1 - ...


def test_frames_kernels_exist_and_use_no_scratch(built, tmp_path):
    from test_flip_decode_host import _device_code
    dis = _device_code(built, tmp_path, "frames.hip")
    bodies = re.split(r"\n(?=[0-9a-f]+ <)", dis)
    mine = [b for b in bodies if re.match(r"[0-9a-f]+ <\S*frames_kernel", b)]
    assert len(mine) >= 3, [b.split(">", 1)[0] for b in bodies]
    for b in mine:
        assert "scratch_" not in b, b.split(">", 1)[0] + ": registers spilled to scratch memory"
