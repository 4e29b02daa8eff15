"""CPU tests of the shared-tag plain decode and ``StudentPipeline``: the ABI of the three new entries (their own header,
the binding's table, the older tables and the revision as they were), the refusals of the entries before any launch,
and the refusals of the parser and the pipeline before any GPU work."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


NEW_SYMBOLS = ("rtpe_topk_fused_shared", "rtpe_adjust_refine_fused_shared_topk",
               "rtpe_adjust_refine_fused_shared_topk_n")


def _declared(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_shared_symbols_are_declared_and_resolve(built):
    """the prototypes live in include/rtpe_hip_shared.h, which rtpe_hip.h includes with one line; the binding lists
    them in EXPORTS_SHARED and resolves them with the others; the three older tables and the ABI revision are as they
    were"""
    main = _declared("rtpe_hip.h")
    assert len(re.findall(r'#include "rtpe_hip_shared.h"', main)) == 1
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", _declared("rtpe_hip_shared.h")))
    assert declared == set(NEW_SYMBOLS) == set(built.EXPORTS_SHARED)
    for older in (built.EXPORTS, built.EXPORTS_SIZES, built.EXPORTS_WARP):
        assert not declared & set(older)
    assert not declared & set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", main))
    assert len(built.EXPORTS) == 59 and len(built.EXPORTS_SIZES) == 5 and len(built.EXPORTS_WARP) == 3
    lib = built.lib()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).argtypes == built._SIGS_SHARED[name][1], name
    # the arguments of the entries without "_shared"
    assert built._SIGS_SHARED["rtpe_topk_fused_shared"] == built._SIGS["rtpe_topk_fused"]
    assert built._SIGS_SHARED["rtpe_adjust_refine_fused_shared_topk"] == built._SIGS["rtpe_adjust_refine_fused_topk"]
    assert built._SIGS_SHARED["rtpe_adjust_refine_fused_shared_topk_n"][1] == \
        built._SIGS["rtpe_adjust_refine_fused_topk"][1] + [ctypes.c_void_p]
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4


FAKE = ctypes.c_void_p(0x1000)
OUT = ctypes.c_void_p(0x2000)
OUT2 = ctypes.c_void_p(0x3000)
# hm, hh, hw, hm_img_stride, tg, th, tw, tg_img_stride, N, J, oh, ow: both maps slices of one (2, 18, 12, 16) tensor
HEAD = dict(hm=FAKE, hh=12, hw=16, hm_st=18 * 12 * 16, tg=FAKE, th=12, tw=16, tg_st=18 * 12 * 16, N=2, J=17, oh=48,
            ow=64)
BAD_HEADS = [dict(hm=None), dict(tg=None), dict(hh=0), dict(hw=-1), dict(th=0), dict(tw=0), dict(N=0), dict(N=-2),
             dict(J=0), dict(J=33), dict(oh=0), dict(ow=-4), dict(hm_st=17 * 12 * 16 - 1), dict(tg_st=12 * 16 - 1)]


def _head(**kw):
    return tuple(dict(HEAD, **kw).values())


def test_shared_topk_refuses_bad_arguments_before_any_launch(built):
    """negative codes and a message; nothing is launched: the pointers are never read"""
    L = built.lib()

    def topk(K=30, ksize=5, pad=2, val=OUT, ind=OUT, tag=OUT, scratch=FAKE, scratch_bytes=1 << 30, **kw):
        return L.rtpe_topk_fused_shared(*_head(**kw), K, ksize, pad, val, ind, tag, scratch, scratch_bytes, None)
    for kw in BAD_HEADS + [dict(K=0), dict(ksize=4), dict(pad=5, ksize=11), dict(val=None), dict(ind=None),
                           dict(tag=None), dict(scratch=None), dict(scratch_bytes=16)]:
        assert topk(**kw) < 0, kw
        assert b"topk" in L.rtpe_last_error_string() or b"nms" in L.rtpe_last_error_string(), kw
    assert topk(J=33) < 0 and b"J <= 32" in L.rtpe_last_error_string()


@pytest.mark.parametrize("entry", NEW_SYMBOLS[1:])
def test_shared_adjust_refine_refuses_bad_arguments_before_any_launch(built, entry):
    L = built.lib()
    tail_n = (FAKE,) if entry.endswith("_n") else ()

    def refine(ans_in=OUT, ans_out=OUT2, P=3, topk_val=OUT, topk_ind=OUT, K=30, scratch=FAKE, scratch_bytes=1 << 30,
               tail=tail_n, **kw):
        return getattr(L, entry)(*_head(**kw), ans_in, ans_out, OUT, P, 1, 1, OUT, topk_val, topk_ind, K, scratch,
                                 scratch_bytes, None, *tail)
    for kw in BAD_HEADS + [dict(ans_in=None), dict(ans_out=None), dict(ans_out=OUT), dict(topk_val=None),
                           dict(topk_ind=None), dict(topk_val=None, topk_ind=None), dict(K=0), dict(scratch=None),
                           dict(scratch_bytes=16)]:
        assert refine(**kw) < 0, kw
        assert b"adjust_refine" in L.rtpe_last_error_string(), kw
    if tail_n:
        assert refine(tail=(None,)) < 0 and b"P_dev" in L.rtpe_last_error_string()
    # P == 0: nothing to do, nothing launched
    built.check(refine(ans_in=None, ans_out=None, P=0, scratch=None, scratch_bytes=0))


def _parser(**kw):
    from rtpe.third_party.group import HeatmapParser
    return HeatmapParser(17, 30, 0.1, 1.0, True, False, **kw)


def test_parse_lowres_shared_refuses_before_any_gpu_work():
    """CPU tensors: whatever reaches the GPU check raises RuntimeError, the refusals come first as ValueError"""
    det = torch.zeros((2, 18, 12, 16))
    heat = det[:, :17]
    for p in (_parser(), _parser(tag_per_joint=False), _parser(match_on="device")):
        for sizes in ([(48, 64), (40, 56)], [(48, 64)], [(48, 64), (0, 56)], ((48, 64), (48, 64))):
            with pytest.raises(ValueError):
                p.parse_lowres_shared(heat, det[:, 17:], sizes)
            with pytest.raises(ValueError):
                p.lowres_topk_shared(heat, det[:, 17:], sizes)
        for tag in (det[:, 16:], det[:, :17], det[:, 18:], det[:1, 17:], det[0, 17:], det[:, 17, 0]):
            with pytest.raises(ValueError):
                p.parse_lowres_shared(heat, tag, (48, 64))
        with pytest.raises(TypeError):
            p.parse_lowres_shared(heat, det[:, 17:].double(), (48, 64))
        # one size, one tag map (4- or 3-dimensional): accepted, and only then the missing GPU is noticed
        for tag in (det[:, 17:], det[:, 17]):
            with pytest.raises(RuntimeError, match="HIP path only"):
                p.parse_lowres_shared(heat, tag, (48, 64))


def test_student_pipeline_refuses_the_teachers_test_protocols():
    from rtpe.engine import StudentPipeline, TeacherPipeline
    assert issubclass(StudentPipeline, TeacherPipeline)
    for kw in (dict(flip_test=True), dict(scale_factors=(1,)), dict(scale_factors=(2, 1, 0.5)), dict(ags=True),
               dict(ags=True, scale_factors=(1,)), dict(flip_test=True, scale_factors=(1, 0.5))):
        with pytest.raises(ValueError, match="StudentPipeline"):
            StudentPipeline(None, device="cuda:0", **kw)
    with pytest.raises(ValueError, match="match_on"):
        StudentPipeline(None, device="cuda:0", match_on="gpu")


def test_student_pipeline_refuses_per_image_sizes_before_the_forward():
    from rtpe.engine import StudentPipeline

    class NoForward(torch.nn.Module):
        def forward(self, x, alt=None):
            raise AssertionError("GPU work")
    pipe = StudentPipeline.__new__(StudentPipeline)         # (the constructor moves the model to a GPU)
    pipe.model, pipe.parser = NoForward(), _parser()
    pipe.flip_test, pipe.scale_factors, pipe.ags = False, None, False
    x = torch.zeros((2, 3, 96, 128))
    with pytest.raises(ValueError, match="one decode size"):
        pipe(x, out_hw=[(96, 128), (90, 120)])
    with pytest.raises(ValueError):
        pipe(x, out_hw=[(96, 128)])
    with pytest.raises(AssertionError, match="GPU work"):
        pipe(x, out_hw=(96, 128))


def test_stream_loop_is_written_once():
    """StudentPipeline supplies its kinds of batch, not the loop and not the synchronous runner; and neither of those
    two names a protocol: what depends on one is a kind's"""
    import inspect
    from rtpe import engine
    from rtpe.engine import StudentPipeline, TeacherPipeline
    assert StudentPipeline.stream is TeacherPipeline.stream and StudentPipeline.gather is TeacherPipeline.gather
    for written_once in ("_stream_loop", "_run"):
        assert written_once not in vars(StudentPipeline) and written_once in vars(TeacherPipeline)
    assert "_kind" in vars(StudentPipeline) and StudentPipeline._kind is not TeacherPipeline._kind

    def pipe(cls, **kw):
        p = cls.__new__(cls)                        # (the constructors move the model to a GPU)
        p.flip_test, p.scale_factors = kw.get("flip_test", False), kw.get("scale_factors")
        return p
    teachers = {type(pipe(TeacherPipeline, **kw)._kind(None))
                for kw in ({}, dict(flip_test=True), dict(scale_factors=(2, 1)), dict(flip_test=True, scale_factors=(1,)))}
    assert teachers == {engine._TeacherPlain, engine._TeacherMultiScale}
    students = {type(pipe(StudentPipeline)._kind(None)), engine._StudentMixed}
    assert students == {engine._StudentPlain, engine._StudentMixed} and not students & teachers
    for kind in teachers | students:
        assert issubclass(kind, engine._Kind)
        for step in ("begin", "tensors", "open", "forwards", "topk"):
            assert callable(getattr(kind, step)), (kind, step)
    # (the loop and the runner: docstring included; a ``__call__`` documents the protocols, its body names none)
    sources = [inspect.getsource(fn) for fn in (TeacherPipeline._stream_loop, TeacherPipeline._run)]
    sources += [inspect.getsource(fn).split('"""')[2] for fn in (TeacherPipeline.__call__, StudentPipeline.__call__)]
    for source in sources:
        assert "_kind" in source or "kind." in source
        for word in ("scale_factors", "flip_test", "ms_", "is_tensor"):
            assert word not in source, (source.splitlines()[0], word)
