"""CPU tests of the one-pass decode of a mixed-size batch from its canvas (include/rtpe_hip_mixdec.h,
HeatmapParser.parse_lowres_mixed, StudentPipeline.call_mixed / stream_mixed / mixed_batches): the ABI of the new entries,
the table the host function fills with every image's own map extents, the refusals of the fill and of the entries, the
refusals that Python raises before any GPU work, and the batch-cutting helper.  The image set and the canvases of
tests/test_mixed_decode_gpu.py live here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = 17

# the batch of the GPU tests: the last three are small outputs (oh + ow <= 128), so one batch mixes both sample kernels and
# both tap orders.  The CPU oracle finds PEOPLE[n] people in image n
SIZES = [(100, 140), (64, 96), (96, 128), (33, 47), (47, 33), (64, 64)]
SEEDS = [51, 52, 53, 54, 55, 56]
PEOPLE = [3, 5, 5, 3, 4, 4]
EXTENTS = [(-(-h // 4), -(-w // 4)) for h, w in SIZES]
# Two more small outputs, images 6 and 7 of ``region`` / ``canvas_det``, never part of the batch above: a landscape and a
# portrait one with no axis at an exact scale, so that their joint-16 candidates fall between the source rows and columns and
# the two tap orders of the small-output kernel give different bits there (1 and 2 of 3 candidates each, on the CPU).  In
# 33 x 47 and 47 x 33 one axis has the scale 8 / 32 = 1 / 4 exactly and no candidate differs.
EXTRA_SIZES = [(38, 58), (58, 38)]
EXTRA_SEEDS = [58, 58]
EXTRA_PEOPLE = [3, 3]
ALL_SIZES = SIZES + EXTRA_SIZES
ALL_SEEDS = SEEDS + EXTRA_SEEDS
ALL_PEOPLE = PEOPLE + EXTRA_PEOPLE
ALL_EXTENTS = [(-(-h // 4), -(-w // 4)) for h, w in ALL_SIZES]
# the tight canvas, and one 2 rows and 3 columns larger: no image reaches an edge, the pitch equals no image's width
CANVASES = [(25, 35), (27, 38)]
NEW_SYMBOLS = {"rtpe_decode_mixed_fill", "rtpe_topk_fused_mixed", "rtpe_adjust_refine_fused_mixed_topk",
               "rtpe_adjust_refine_fused_mixed_topk_n"}

_REGIONS = {}


def region(n, scale=1):
    """image n's own maps (CPU): heat (1,J,eh,ew) and ONE tag map (1,1,eh,ew), the J tag planes of ``make_decode_maps``
    reduced with amax; ``scale`` = 2: maps of half the extent (a tag canvas at half the heat maps' resolution)"""
    key = (n, scale)
    if key not in _REGIONS:
        eh, ew = ALL_EXTENTS[n]
        eh, ew = -(-eh // scale), -(-ew // scale)
        det, tag = synth.make_decode_maps(3, eh, ew, seed=ALL_SEEDS[n], sigma=1.0)
        # (unsqueeze: the leading axis of the numpy arrays has stride 0, which no entry takes for an image stride)
        _REGIONS[key] = (torch.from_numpy(det[0].copy()).unsqueeze(0),
                         torch.from_numpy(tag[0, ..., 0].copy()).amax(0, keepdim=True).unsqueeze(0))
    return _REGIONS[key]


def canvas_det(canvas_hw, order=None, blank=()):
    """the (N, J + 1, Hc, Wc) det canvas of the batch (CPU): image n's maps in ``[n, :, :eh_n, :ew_n]``, NaN everywhere else.
    ``order``: the images of the batch (indices into ``ALL_SIZES``), default the six of ``SIZES``; ``blank``: positions whose heat maps are all zero"""
    order = list(range(len(SIZES))) if order is None else list(order)
    det = torch.full((len(order), J + 1) + tuple(canvas_hw), float("nan"))
    for i, n in enumerate(order):
        heat, tag = region(n)
        eh, ew = ALL_EXTENTS[n]
        det[i, :J, :eh, :ew] = 0.0 if i in blank else heat[0]
        det[i, J:, :eh, :ew] = tag[0]
    return det


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


def _declared(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


# --------------------------------------------------------------------------- #
# ABI
# --------------------------------------------------------------------------- #
def test_mixdec_symbols_are_declared_in_their_header_and_resolve(built):
    main, hdr = _declared("rtpe_hip.h"), _declared("rtpe_hip_mixdec.h")
    assert len(re.findall(r'#include "rtpe_hip_mixdec.h"', main)) == 1
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", hdr))
    assert declared == NEW_SYMBOLS == set(built.EXPORTS_MIXDEC)
    older = (built.EXPORTS, built.EXPORTS_SIZES, built.EXPORTS_WARP, built.EXPORTS_SHARED, built.EXPORTS_PAIR,
             built.EXPORTS_RECORDS, built.EXPORTS_TAGMEAN, built.EXPORTS_NOPROJ, built.EXPORTS_ANYSIZE, built.EXPORTS_MIXED)
    assert [len(t) for t in older] == [59, 5, 3, 3, 1, 2, 6, 5, 4, 4]      # no change to the existing tables
    for table in older:
        assert not declared & set(table)
    for name in os.listdir(os.path.join(ROOT, "include")):                # ... nor to what the older headers declare
        if name != "rtpe_hip_mixdec.h":
            assert not declared & set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", _declared(name))), name
    lib = built.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == built._SIGS_MIXDEC[name][1], name
    sizes, mix = built._SIGS_SIZES, built._SIGS_MIXDEC
    assert mix["rtpe_topk_fused_mixed"][1] == sizes["rtpe_topk_fused_sizes"][1]
    assert mix["rtpe_adjust_refine_fused_mixed_topk"][1] == sizes["rtpe_adjust_refine_fused_topk_sizes"][1]
    assert mix["rtpe_adjust_refine_fused_mixed_topk_n"][1] == sizes["rtpe_adjust_refine_fused_topk_sizes_n"][1]
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4


# --------------------------------------------------------------------------- #
# the table
# --------------------------------------------------------------------------- #
def _pairs(hw):
    return None if hw is None else (ctypes.c_int32 * (2 * len(hw)))(*[v for p in hw for v in p])


def _fill(built, out_hw, heat_hw, tag_hw, pitch, table_bytes=None):
    N = len(out_hw)
    tab = np.full((N, 16), -7, np.int32)
    mh, mw = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = built.lib().rtpe_decode_mixed_fill(_pairs(out_hw), _pairs(heat_hw), _pairs(tag_hw), N, *pitch, tab.ctypes.data,
                                            64 * N if table_bytes is None else table_bytes, ctypes.byref(mh),
                                            ctypes.byref(mw))
    return rc, tab, mh.value, mw.value


def _axis_words(n_in, n_out):
    """numpy restatement of make_axis: { float32 scale; int32 n_in; int32 same } as three 32-bit words"""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    return [int(np.float32(scale).view(np.int32)), n_in, int(n_in == n_out)]


def _want_table(out_hw, heat_hw, tag_hw):
    rows = []
    for (oh, ow), (eh, ew), (th, tw) in zip(out_hw, heat_hw, tag_hw):
        rows.append([oh, ow] + _axis_words(eh, oh) + _axis_words(ew, ow) + _axis_words(th, oh) + _axis_words(tw, ow) +
                    [int(oh + ow <= 128), 0])
    return np.array(rows, np.int64).astype(np.int32)


def test_mixed_table_holds_the_axes_of_every_images_own_extents(built):
    """entry n = make_axis(heat_hw[n], out_hw[n]) and make_axis(tag_hw[n], out_hw[n]) per axis, small from its own size:
    the pitch appears nowhere in the table"""
    for pitch in ((25, 35, 25, 35), (27, 38, 27, 38), (300, 400, 300, 400)):
        rc, tab, mh, mw = _fill(built, SIZES, EXTENTS, None, pitch)
        assert rc == 0 and (mh, mw) == (100, 140)
        assert np.array_equal(tab, _want_table(SIZES, EXTENTS, EXTENTS)), pitch
    assert tab[:, 14].tolist() == [0, 0, 0, 1, 1, 1]
    # tag extents of their own (a tag canvas at half the resolution), sizes below, at and above the extents, 1-pixel axes
    out_hw = [(100, 140), (13, 18), (25, 35), (1, 1), (7, 1), (64, 64)]
    heat_hw = [(25, 35), (25, 35), (25, 35), (1, 1), (3, 5), (16, 16)]
    tag_hw = [(13, 18), (13, 18), (25, 18), (1, 1), (2, 3), (8, 8)]
    rc, tab, mh, mw = _fill(built, out_hw, heat_hw, tag_hw, (25, 35, 25, 18))
    assert rc == 0 and (mh, mw) == (100, 140)
    assert np.array_equal(tab, _want_table(out_hw, heat_hw, tag_hw))
    assert tab[2, 4] == 1 and tab[2, 7] == 1 and tab[2, 10] == 1 and tab[2, 13] == 0 and tab[1, 10] == 1     # `same`
    L = built.lib()
    assert L.rtpe_decode_mixed_fill(_pairs(out_hw), _pairs(heat_hw), None, 6, 25, 35, 25, 35, tab.ctypes.data, 64 * 6,
                                    None, None) == 0                     # the maxima are optional


def test_mixed_table_equals_the_sizes_table_where_every_extent_is_the_pitch(built):
    out_hw = [(128, 80), (1, 1), (256, 320), (100, 333), (64, 160), (31, 47), (128, 160), (64, 80)]
    hh, hw, th, tw = 128, 160, 64, 80
    N = len(out_hw)
    want = np.full((N, 16), -1, np.int32)
    built.check(built.lib().rtpe_decode_sizes_fill(_pairs(out_hw), N, hh, hw, th, tw, want.ctypes.data, 64 * N, None, None))
    rc, tab, mh, mw = _fill(built, out_hw, [(hh, hw)] * N, [(th, tw)] * N, (hh, hw, th, tw))
    assert rc == 0 and tab.tobytes() == want.tobytes() and (mh, mw) == (256, 333)
    rc, tab, _, _ = _fill(built, out_hw, [(hh, hw)] * N, None, (hh, hw, hh, hw))       # tag_hw NULL: the heat extents
    built.check(built.lib().rtpe_decode_sizes_fill(_pairs(out_hw), N, hh, hw, hh, hw, want.ctypes.data, 64 * N, None, None))
    assert rc == 0 and tab.tobytes() == want.tobytes()


def test_mixed_fill_refusals(built):
    """a wrong table would make the device read outside the tensor: everything is refused, with a message, before the
    first entry is written"""
    L = built.lib()
    ok = dict(out_hw=[(100, 140), (64, 96)], heat_hw=[(25, 35), (16, 24)], tag_hw=[(13, 18), (8, 12)], pitch=(25, 35, 13, 18))
    assert _fill(built, **ok)[0] == 0
    for change, msg in ((dict(out_hw=[(100, 140), (0, 96)]), b"image 1 has size"),
                        (dict(out_hw=[(-1, 140), (64, 96)]), b"image 0 has size"),
                        (dict(heat_hw=[(25, 35), (16, 0)]), b"map extents"),
                        (dict(tag_hw=[(13, -2), (8, 12)]), b"map extents"),
                        (dict(heat_hw=[(26, 35), (16, 24)]), b"heat extent 26 x 35 is above the pitch 25 x 35"),
                        (dict(heat_hw=[(25, 35), (16, 36)]), b"heat extent 16 x 36 is above the pitch"),
                        (dict(tag_hw=[(13, 18), (14, 12)]), b"tag extent 14 x 12 is above the pitch 13 x 18"),
                        (dict(tag_hw=[(13, 19), (8, 12)]), b"tag extent 13 x 19 is above the pitch"),
                        (dict(tag_hw=None), b"tag extent 25 x 35 is above the pitch 13 x 18"),      # = the heat extents
                        (dict(pitch=(0, 35, 13, 18)), b"bad shape"), (dict(pitch=(25, 35, 13, -1)), b"bad shape"),
                        (dict(table_bytes=127), b"table too small")):
        rc, tab, mh, mw = _fill(built, **dict(ok, **change))
        assert rc == -1 and msg in L.rtpe_last_error_string(), (change, L.rtpe_last_error_string())
        assert (tab == -7).all() and (mh, mw) == (-1, -1), change           # nothing was written
    tab = np.zeros((2, 16), np.int32)
    o, h = _pairs(ok["out_hw"]), _pairs(ok["heat_hw"])
    assert L.rtpe_decode_mixed_fill(None, h, None, 2, 25, 35, 25, 35, tab.ctypes.data, 128, None, None) == -1
    assert L.rtpe_decode_mixed_fill(o, None, None, 2, 25, 35, 25, 35, tab.ctypes.data, 128, None, None) == -1
    assert L.rtpe_decode_mixed_fill(o, h, None, 2, 25, 35, 25, 35, None, 128, None, None) == -1
    assert L.rtpe_decode_mixed_fill(o, h, None, 0, 25, 35, 25, 35, tab.ctypes.data, 128, None, None) == -1


def test_mixed_entries_check_their_arguments_before_any_launch(built):
    """the refusals of the `_sizes` and of the `_shared` entries together; no launch: the pointers are never read"""
    L = built.lib()
    fake, val = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)
    Hc, Wc = 27, 38

    def topk(hm=fake, tg=fake, tab=fake, table_bytes=2 * 64, max_oh=100, max_ow=140, w_enc=140, K=30, out=val,
             scratch=fake, scratch_bytes=1 << 30, N=2, Jn=17, ksize=5, pad=2, hm_stride=18 * Hc * Wc,
             tg_stride=18 * Hc * Wc, hh=Hc, tw=Wc):
        return L.rtpe_topk_fused_mixed(hm, hh, Wc, hm_stride, tg, Hc, tw, tg_stride, N, Jn, tab, table_bytes, max_oh,
                                       max_ow, w_enc, K, ksize, pad, out, val, val, scratch, scratch_bytes, None)

    def refine(n=False, hm=fake, tg=fake, tab=fake, table_bytes=2 * 64, max_oh=100, max_ow=140, w_enc=140, P=3,
               ans_out=fake, topk_val=val, K=30, p_dev=fake, Jn=17, hm_stride=18 * Hc * Wc, tg_stride=18 * Hc * Wc):
        args = (hm, Hc, Wc, hm_stride, tg, Hc, Wc, tg_stride, 2, Jn, tab, table_bytes, max_oh, max_ow, w_enc, val,
                ans_out, val, P, 1, 1, val, topk_val, val if topk_val else None, K, fake, 16, None)
        if n:
            return L.rtpe_adjust_refine_fused_mixed_topk_n(*args, p_dev)
        return L.rtpe_adjust_refine_fused_mixed_topk(*args)
    nb = ctypes.c_size_t()
    built.check(L.rtpe_topk_scratch_bytes(2 * 17, 100, 140, 30, ctypes.byref(nb)))
    bad = (dict(hm=None), dict(tg=None), dict(tab=None), dict(table_bytes=2 * 64 - 1), dict(max_oh=0), dict(max_ow=-3),
           dict(w_enc=139), dict(max_oh=40000, w_enc=60000),              # y * w_enc + x beyond int32
           dict(Jn=33), dict(Jn=0),
           dict(hm_stride=17 * Hc * Wc - 1), dict(tg_stride=Hc * Wc - 1))  # an image stride below the image's planes
    for kw in bad + (dict(N=0), dict(hh=0), dict(tw=-1), dict(K=0), dict(out=None), dict(scratch=None),
                     dict(scratch_bytes=nb.value - 8), dict(ksize=4), dict(pad=5, ksize=11)):
        assert topk(**kw) < 0, kw
        assert b"topk" in L.rtpe_last_error_string() or b"nms" in L.rtpe_last_error_string()
    assert topk(w_enc=139) < 0 and b"topk_fused_mixed: w_enc=139" in L.rtpe_last_error_string()
    assert topk(tg_stride=Hc * Wc - 1) < 0 and b"image stride" in L.rtpe_last_error_string()
    assert topk(hm_stride=17 * Hc * Wc, tg_stride=Hc * Wc, scratch_bytes=8) < 0 and \
        b"scratch too small" in L.rtpe_last_error_string()                 # the smallest strides pass the argument checks
    for n in (False, True):
        for kw in bad + (dict(ans_out=val), dict(topk_val=None), dict(K=0)):
            assert refine(n, **kw) < 0, (n, kw)
            assert b"adjust_refine_fused_mixed_topk" in L.rtpe_last_error_string(), (n, kw)
        # the scratch of 16 bytes is refused too - after every argument check, before the first launch
        assert refine(n) < 0 and b"scratch too small" in L.rtpe_last_error_string()
    assert refine(True, p_dev=None) < 0 and b"P_dev is null" in L.rtpe_last_error_string()
    built.check(refine(False, P=0))                                         # P == 0: nothing to do, nothing launched


# --------------------------------------------------------------------------- #
# Python: every refusal before any GPU work
# --------------------------------------------------------------------------- #
def _parser(match_on="host"):
    from rtpe.third_party.group import HeatmapParser
    return HeatmapParser(J, 30, 0.1, 1.0, True, False, True, 5, 2, match_on=match_on)


def test_parse_lowres_mixed_checks_its_arguments_before_any_gpu_work(built):
    """CPU tensors: a call that got as far as the GPU check raises RuntimeError, a refused argument ValueError / TypeError"""
    hp = _parser()
    det = canvas_det(CANVASES[1])
    heat, tag = det[:, :J], det[:, J:]
    for maps in (det, (heat, tag), (heat, tag[:, 0]), [heat, tag]):          # accepted: stopped by the missing GPU
        with pytest.raises(RuntimeError, match="HIP path only"):
            hp.parse_lowres_mixed(maps, SIZES)
        with pytest.raises(RuntimeError, match="HIP path only"):
            hp.lowres_topk_mixed(maps, SIZES)
    with pytest.raises(RuntimeError, match="HIP path only"):                  # explicit extents, the tags' at half
        hp.parse_lowres_mixed((heat, tag[:, :, :14, :19]), SIZES, extents=(EXTENTS, [(-(-h // 2), -(-w // 2)) for h, w in EXTENTS]))
    with pytest.raises(RuntimeError, match="HIP path only"):
        hp.parse_lowres_mixed(det, SIZES, extents=(EXTENTS, None))
    bad_sizes = (SIZES[:5], SIZES + [(64, 64)], (100, 140), [(100, 140), (64, 0)] + SIZES[2:], [(100, 140), (64.5, 96)] + SIZES[2:],
                 [(100, 140), 64] + SIZES[2:], [(112, 140)] + SIZES[1:], [(100, 156)] + SIZES[1:])   # (28 rows / 39 columns)
    for bad in bad_sizes:
        with pytest.raises(ValueError):
            hp.parse_lowres_mixed(det, bad)
    with pytest.raises(ValueError, match="does not fit the 25 x 35 canvas"):
        hp.parse_lowres_mixed(canvas_det(CANVASES[0]), [(101, 140)] + SIZES[1:])
    for bad in ((EXTENTS,), (EXTENTS[:5], None), (EXTENTS, EXTENTS[:5]),
                ([(28, 35)] + EXTENTS[1:], None), (EXTENTS, [(25, 39)] + EXTENTS[1:]), ([(0, 35)] + EXTENTS[1:], None),
                ([(2.5, 35)] + EXTENTS[1:], None), 7):
        with pytest.raises(ValueError):
            hp.parse_lowres_mixed(det, SIZES, extents=bad)
    for maps in (det[0], det[:, :1], (heat,), (heat, tag, tag), (heat[0], tag), (heat, tag[0, 0]), (heat, det[:, J - 1:]),
                 (heat, tag[:5]), "det"):
        with pytest.raises(ValueError):
            hp.parse_lowres_mixed(maps, SIZES)
    with pytest.raises(TypeError, match="float32"):
        hp.parse_lowres_mixed(det.double(), SIZES)
    # records: the host matcher has none; a wrong number of ids
    with pytest.raises(ValueError, match="match_on='device'"):
        hp.parse_lowres_mixed(det, SIZES, records=(list(range(6)), None))
    with pytest.raises(ValueError):
        _parser("device").parse_lowres_mixed(det, SIZES, records=(list(range(5)), None))
    # parse_lowres_shared keeps refusing per-image sizes
    with pytest.raises(ValueError, match="one decode size"):
        hp.parse_lowres_shared(heat, tag, SIZES)


class _NoForward(torch.nn.Module):
    def forward(self, x):
        raise AssertionError("GPU work")

    def forward_mixed(self, canvas, sizes):
        raise AssertionError("GPU work: forward_mixed")


def test_call_mixed_checks_its_arguments_before_any_gpu_work():
    from rtpe.engine import StudentPipeline
    ims = [torch.zeros((3, h, w)) for h, w in SIZES[:3]]
    pipe = StudentPipeline(_NoForward(), _parser(), device="cpu")
    with pytest.raises(ValueError, match="decode must be 'batch' or 'per_image'"):
        pipe.call_mixed(ims, decode="each")
    for decode in ("batch", "per_image"):
        with pytest.raises(ValueError, match="2 image ids for 3 images"):
            pipe.call_mixed(ims, image_ids=[1, 2], decode=decode)
        with pytest.raises(ValueError, match="match_on='device'"):            # records need the device matcher
            pipe.call_mixed(ims, image_ids=[1, 2, 3], decode=decode)
        with pytest.raises(AssertionError, match="forward_mixed"):             # accepted: the forward is reached
            pipe.call_mixed(ims, decode=decode)
    with pytest.raises(ValueError, match="at least 32"):
        pipe.call_mixed([torch.zeros((3, 31, 40))])
    # what a step of stream_mixed does with a batch first
    (canvas, sizes), hw = pipe._mixed_begin(ims)
    assert canvas.shape == (3, 3, 100, 140) and sizes == hw == SIZES[:3]
    (c2, s2), hw2 = pipe._mixed_begin((canvas, [list(s) for s in sizes]))
    assert c2 is canvas and s2 == hw2 == SIZES[:3]
    for bad in (canvas, (canvas, None), [], (canvas[0], sizes), (canvas, sizes[:2]), (canvas, [(100, 141)] + sizes[1:])):
        with pytest.raises(ValueError):
            pipe._mixed_begin(bad)
    # stream() and __call__ keep refusing mixed batches
    with pytest.raises(ValueError, match="use call_mixed"):
        pipe(ims)
    with pytest.raises(ValueError, match="use call_mixed"):
        pipe._decode_hw(None, (canvas, sizes))

    # what forward_mixed (or on_forward) returns is checked as the one-size forward's is: (att, det (N, J + 1, h, w))
    class _Returns(torch.nn.Module):
        def __init__(self, out):
            super().__init__()
            self.out = out

        def forward_mixed(self, canvas, sizes):
            return self.out
    att, det = torch.zeros((3, 1, 25, 35)), torch.zeros((3, J + 1, 25, 35))
    for out in (det, (att,), (att, det, det), (att, None), (att, det[0]), (att, det[:, :1]), (att, det[:2])):
        bad = StudentPipeline(_Returns(out), _parser(), device="cpu")
        with pytest.raises(TypeError, match="StudentPipeline"):
            bad.call_mixed(ims)
        with pytest.raises(TypeError, match="StudentPipeline"):
            bad._mixed_forwards(0, (canvas, sizes), None)
        with pytest.raises(TypeError, match="StudentPipeline"):
            pipe._mixed_forwards(0, (canvas, sizes), lambda k, batch: out)
    with pytest.raises(RuntimeError, match="HIP path only"):                   # a good return reaches the decode
        StudentPipeline(_Returns((att, det)), _parser(), device="cpu").call_mixed(ims)

    class _Plain(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("GPU work")
    with pytest.raises(ValueError, match="no forward_mixed"):
        StudentPipeline(_Plain(), _parser(), device="cpu")._mixed_begin(ims)


# --------------------------------------------------------------------------- #
# the batch-cutting helper
# --------------------------------------------------------------------------- #
class _Img:
    def __init__(self, h, w):
        self.shape = (3, h, w)


def test_mixed_batches_sorts_by_area_and_restores_the_callers_order():
    from rtpe.engine import StudentPipeline
    rng = np.random.default_rng(2017)
    shapes = [(int(rng.integers(32, 641)), int(rng.integers(32, 641))) for _ in range(70)] + [(64, 64), (32, 128), (128, 32)]
    ims = [_Img(h, w) for h, w in shapes]
    batches, restore = StudentPipeline.mixed_batches(ims, 32)
    assert [len(b) for b in batches] == [32, 32, 9]
    flat = [im for b in batches for im in b]
    assert sorted(map(id, flat)) == sorted(map(id, ims))                      # every image once
    areas = [im.shape[1] * im.shape[2] for im in flat]
    assert areas == sorted(areas)
    tied = [ims.index(im) for im in flat if im.shape[1] * im.shape[2] == 4096]
    assert tied == [70, 71, 72]                                                # ties keep the caller's order
    results = [[("result", id(im)) for im in b] for b in batches]
    assert restore(results) == [("result", id(im)) for im in ims]
    assert restore(iter(results)) == [("result", id(im)) for im in ims]
    for bad in (results[:2], results + [[]], [results[0][:-1]] + results[1:]):
        with pytest.raises(ValueError):
            restore(bad)
    one, back = StudentPipeline.mixed_batches(ims[:5], 8)
    assert len(one) == 1 and len(one[0]) == 5 and back([[im.shape for im in one[0]]]) == [im.shape for im in ims[:5]]
    none, back = StudentPipeline.mixed_batches([], 8)
    assert none == [] and back([]) == []
    with pytest.raises(ValueError):
        StudentPipeline.mixed_batches(ims, 0)
    # real tensors: the batches are what call_mixed takes
    ts = [torch.zeros((3, h, w)) for h, w in SIZES]
    batches, restore = StudentPipeline.mixed_batches(ts, 4)
    assert [[tuple(t.shape[1:]) for t in b] for b in batches] == [[(33, 47), (47, 33), (64, 64), (64, 96)], [(96, 128), (100, 140)]]
    assert restore([[0, 1, 2, 3], [4, 5]]) == [5, 3, 4, 0, 1, 2]
